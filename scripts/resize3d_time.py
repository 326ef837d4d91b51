#!/usr/bin/env python
"""Time the 3-D Fourier resize (csrc/resize3.hip, ops.spectral_resize3) and what it adds to a graphed AR step.

    python scripts/resize3d_time.py [--window 0.25] [--rounds 5] [--skip-step] > profiles/resize3d.txt

Part 1, per shape ([1, 64^3, 10, 4] -> 128^3, [1, 128^3, 1, 4] -> 64^3, [4, 48^3, 10, 4] -> 64^3): the kernel and two
yardsticks taken in the same run, alternating with it - median of `rounds` rounds, each timed window `window` seconds of
back-to-back calls between two device events (the call count is fixed from a first estimate, nothing synchronises inside):
  * torch composition: the same operator from torch ops on the device - channels-first rfftn, the corner assignments, irfftn
    (tests/resize3_ref.py resize3_torch, float32);
  * copy: a plain device copy of the bytes the operator must move (input read once + output written once); the workspace's
    bytes (written once and read once between the two launches) are listed separately, not counted in it.
Printed: microseconds, the kernel's time as a ratio to each yardstick, and the EXECUTED FLOP of the matrix-core launches
(padding included) over the kernel's time as a fraction of the 157.3 TF fp32 matrix-core roof.
Part 2: one graphed AR step (GraphedRollout.step) of the small DPOTNet3D of the tests at img_size 16, plain on 16^3 data and
wrapped in Resized3D on 12 x 20 x 24 data: the difference is the cost of the two resizes inside the graph.
One JSON line per row."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dpot_amd import DPOTNet3D, _lib, ops  # noqa: E402
from dpot_amd.infer import GraphedRollout, Resized3D  # noqa: E402
from resize3_ref import resize3_torch  # noqa: E402   (the torch.fft composition, shared with the tests)

PEAK = 157.3e12
SHAPES = [((1, 64, 64, 64, 10, 4), (128, 128, 128)), ((1, 128, 128, 128, 1, 4), (64, 64, 64)),
          ((4, 48, 48, 48, 10, 4), (64, 64, 64))]


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def alternate(fns, window, rounds):
    """median per-call milliseconds of each fn; the fns take turns inside every round"""
    calls = []
    for fn in fns:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        est = window_ms(fn, 3)
        calls.append(max(3, int(window * 1e3 / max(est, 1e-3))))
    got = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            got[i].append(window_ms(fn, calls[i]))
    return [float(np.median(g)) for g in got], calls


def executed_flop(B, n, m, TC):
    """2 * M * N * K of every MFMA product the launches issue, padded extents, for the pass order the library takes"""
    pad = _lib.load().dpot_spectral_resize3_pad
    (nx, ny, nz), (mx, my, mz) = n, m
    two = lambda a, b: a != b and min(a, b) % 2 == 0
    ex, ey = two(nx, mx), two(ny, my)
    tcp = (TC + 3) // 4 * 4

    def plane(planes):            # Y pass [myp32 x nyp] x [nyp x nzp tcp], Z pass [rows x nzp] x [nzp x mzp]
        rows = pad(my, 1) * tcp + (pad(my, 1) // 2 * (tcp // 4) if ey else 0)     # + one 16-row tile per stripe and 4 planes
        return planes * 2.0 * (pad(my, 1) * pad(ny, 0) * pad(nz, 0) * tcp + rows * pad(nz, 0) * pad(mz, 0))

    plane_first = nx * my * mz <= mx * ny * nz
    cols = (my * mz if plane_first else ny * nz) * TC
    axis = B * 2.0 * pad(mx, 1) * pad(nx, 0) * ((cols + 255) // 256 * 256)
    return plane(B * (nx if plane_first else mx)) + (plane(B) if ex else 0.0) + axis, plane_first, ex, ey


def part1(args):
    for shape, m in SHAPES:
        B, n, TC = shape[0], tuple(shape[1:4]), shape[4] * shape[5]
        x = torch.randn(shape, device="cuda")
        out = torch.empty((B,) + m + shape[4:], device="cuda")
        ops.spectral_resize3(x, m, out=out)
        ref = resize3_torch(x, m)
        err = float((out - ref).abs().max() / ref.abs().max())
        n_in, n_out = x.numel(), out.numel()
        src, dst = torch.empty(n_in + n_out, device="cuda"), torch.empty(n_in + n_out, device="cuda")
        n_ws = _lib.load().dpot_spectral_resize3_ws_elems(B, *n, *m, TC)
        (t_k, t_t, t_c), calls = alternate([lambda: ops.spectral_resize3(x, m, out=out), lambda: resize3_torch(x, m),
                                            lambda: dst[:(n_in + n_out) // 2].copy_(src[:(n_in + n_out) // 2])],
                                           args.window, args.rounds)
        flop, plane_first, ex, ey = executed_flop(B, n, m, TC)
        print(json.dumps({"shape": list(shape), "to": list(m), "order": "planes, X" if plane_first else "X, planes",
                          "two_term_x": ex, "two_term_y": ey, "kernel_us": round(t_k * 1e3, 1),
                          "torch_fft_us": round(t_t * 1e3, 1), "copy_us": round(t_c * 1e3, 1),
                          "kernel_over_torch_fft": round(t_k / t_t, 3), "kernel_over_copy": round(t_k / t_c, 2),
                          "moved_MB": round(4e-6 * (n_in + n_out), 1), "workspace_MB": round(4e-6 * n_ws, 1),
                          "executed_GFLOP": round(flop * 1e-9, 2), "fraction_of_fp32_mfma_roof": round(flop / (t_k * 1e-3) / PEAK, 3),
                          "max_rel_diff_vs_torch_fft": float(f"{err:.2e}"), "calls_per_window": calls}), flush=True)
        del x, out, ref, src, dst
        torch.cuda.empty_cache()


def part2(args):
    cfg = dict(img_size=16, patch_size=4, in_channels=2, out_channels=2, in_timesteps=3, embed_dim=32, depth=2, n_blocks=2,
               modes=4)
    torch.manual_seed(2003)
    m = DPOTNet3D(**cfg).cuda().eval()
    B, data = 2, (12, 20, 24)
    x_plain = torch.randn(B, 16, 16, 16, 3, 2, device="cuda")
    x_data = torch.randn((B,) + data + (3, 2), device="cuda")
    g_plain, g_wrapped = GraphedRollout(m, x_plain), GraphedRollout(Resized3D(m, 16), x_data)
    (t_p, t_w), calls = alternate([lambda: g_plain.step(x_plain), lambda: g_wrapped.step(x_data)], args.window, args.rounds)
    print(json.dumps({"graphed_ar_step": "DPOTNet3D img_size 16, embed 32, depth 2, B 2", "data": list(data),
                      "plain_us": round(t_p * 1e3, 1), "wrapped_us": round(t_w * 1e3, 1),
                      "two_resizes_add_us": round((t_w - t_p) * 1e3, 1), "calls_per_window": calls}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resize3d_time.py needs the MI355X: there is nothing to time without it")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "window_s": args.window, "rounds": args.rounds}), flush=True)
    with torch.no_grad():
        part1(args)
        if not args.skip_step:
            part2(args)


if __name__ == "__main__":
    main()
