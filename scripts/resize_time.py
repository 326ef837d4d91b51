#!/usr/bin/env python
"""Time the Fourier resize kernel (csrc/resize.hip) and what it adds to an evaluation rollout.

    python scripts/resize_time.py [--reps 50] [--skip-rollout] [--out profiles/spectral_resize.json]

Part 1, per launch (a hipGraph of `reps` launches between two events, median of 5 graphs), batch 32: TC = 40 up
(res -> 128, the input window of an AR step) and TC = 4 down (128 -> res, the prediction), res in {41, 64, 86, 122}.
Printed per row: microseconds, algorithmic bytes (field read once + written once) / time against the 8 TB/s HBM roof,
EXECUTED FLOP (every MFMA the kernel issues, padding included) / time against 157.3 TF, and the yardstick: the same
operator as two launches of the project's batched fp32 GEMM (ops.gemm) through an HBM intermediate - its first term only
(Re Dx (x) Re Dy), so for the two-term size pairs the yardstick does LESS than the fused kernel.
Part 2: the DPOT-Tiny evaluation rollout (GraphedRollout, batch 32, T_ar = 10) at res 128 without resize, twice (their
difference is the run-to-run spread), and at res 86 with model_res = 128; the difference per AR step is the cost of the
feature.  One JSON line per row."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dpot_amd import ops  # noqa: E402
from oracle import dpot_ref as R  # noqa: E402   (model configurations only)

HBM, PEAK = 8.0e12, 157.3e12


def time_graph(fn, reps):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    out.sort()
    return out[2], out[0], out[4]


def executed_flop(B, nx, ny, mx, my, TC):
    """2 x 1024 per v_mfma_f32_16x16x4_f32 the kernel issues (csrc/resize.hip), summed over its workgroups"""
    nxp, nyp, mxp, myp = ops.ResizePlan.pads(nx, ny, mx, my)
    two_terms = ops.spectral_resize_im_factors(nx, mx) is not None
    mfma = 0
    for s in range(mxp // 32):
        tiles = 2 if 32 * s + 16 < mx else 1
        mfma += (nyp // 16) * (nxp // 4) * 4 * tiles                        # pass 1: y tiles x k steps x planes x row tiles
        mfma += (myp // 16) * (nyp // 4) * (4 * tiles + (1 if two_terms else 0))
    return 2048.0 * mfma * ((TC + 3) // 4) * B


def gemm_pair(x, mats, tmp, out):
    """the first term as two batched GEMMs: Tmp[b] = Re Dx @ in[b] (columns (y, p)), out[b, x'] = Re Dy/(nx ny) @ Tmp[b, x']"""
    ax, ay = mats
    B, nx, ny = x.shape[:3]
    TC = x.numel() // (B * nx * ny)
    mx, my = ax.shape[0], ay.shape[0]
    ops.gemm(ax, x, tmp, mx, ny * TC, nx, lda=nx, ldb=ny * TC, ldc=ny * TC, batch=B, strideA=0, strideB=nx * ny * TC,
             strideC=mx * ny * TC, splitk=1)
    ops.gemm(ay, tmp, out, my, TC, ny, lda=ny, ldb=TC, ldc=TC, batch=B * mx, strideA=0, strideB=ny * TC, strideC=my * TC,
             splitk=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-rollout", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, B = "cuda", 32
    rows = []
    for res in (41, 64, 86, 122):
        for kind, n, m, T, C in (("up", res, 128, 10, 4), ("down", 128, res, 1, 4)):
            TC = T * C
            x = torch.randn(B, n, n, T, C, device=dev)
            out = torch.empty(B, m, m, T, C, device=dev)
            t, lo, hi = time_graph(lambda: ops.spectral_resize(x, (m, m), out=out), args.reps)
            rx, _ = ops.spectral_resize_matrices(n, m, 0)
            ry, _ = ops.spectral_resize_matrices(n, m, 1)
            mats = (torch.from_numpy(rx).float().to(dev), torch.from_numpy(ry / (n * n)).float().to(dev))
            tmp, out2 = torch.empty(B, m, n, T, C, device=dev), torch.empty_like(out)
            ty, _, _ = time_graph(lambda: gemm_pair(x, mats, tmp, out2), args.reps)
            two = ops.spectral_resize_im_factors(n, m) is not None
            dev_err = None if two else float((out2 - out).abs().max() / out.abs().max())
            nbytes = 4.0 * B * TC * (n * n + m * m)
            fl = executed_flop(B, n, n, m, m, TC)
            row = {"what": f"resize {kind} {n}->{m}", "B": B, "TC": TC, "two_terms": two, "us": round(t, 2),
                   "us_min_max": [round(lo, 2), round(hi, 2)], "MB": round(nbytes / 1e6, 1),
                   "hbm_frac": round(nbytes / (t * 1e-6) / HBM, 3), "exec_GFLOP": round(fl / 1e9, 2),
                   "mfma_frac": round(fl / (t * 1e-6) / PEAK, 3), "gemm_pair_us": round(ty, 2),
                   "gemm_pair_over_fused": round(ty / t, 2), "gemm_pair_max_rel_dev": dev_err}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del x, out, tmp, out2
    if not args.skip_rollout:
        from dpot_amd import DPOTNet
        from dpot_amd.infer import GraphedRollout
        cfg = R.DPOTConfig(**R.TINY)
        model = DPOTNet(**R.TINY)
        model.load_state_dict(R.recipe_state_dict(cfg, salt=1))
        model.cuda().eval()
        T_ar, S = 10, cfg.img_size
        g = GraphedRollout(model, torch.randn(B, S, S, cfg.in_timesteps, cfg.in_channels, device=dev))

        def run(res, model_res, label):
            xx = torch.randn(B, res, res, cfg.in_timesteps, cfg.in_channels, device=dev)
            yy = torch.randn(B, res, res, T_ar, cfg.out_channels, device=dev)
            msk = torch.ones(B, res, res, 1, cfg.out_channels, device=dev)
            for _ in range(2):
                g(xx, yy, msk, model_res=model_res)
            torch.cuda.synchronize()
            ts = []
            for _ in range(7):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                g(xx, yy, msk, model_res=model_res)
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) / T_ar)
            ts.sort()
            row = {"what": label, "B": B, "T_ar": T_ar, "ms_per_ar_step": round(ts[3], 4),
                   "ms_min_max": [round(ts[0], 4), round(ts[-1], 4)]}
            rows.append(row)
            print(json.dumps(row), flush=True)
            return ts[3]

        p1 = run(S, None, "rollout res 128, no resize (run 1)")
        r = run(86, S, "rollout res 86, model_res 128")
        p2 = run(S, None, "rollout res 128, no resize (run 2)")
        row = {"what": "cost of the feature per AR step", "ms": round(r - 0.5 * (p1 + p2), 4),
               "plain_spread_ms": round(abs(p1 - p2), 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
