#!/usr/bin/env python
"""Time RolloutEvaluator.update (csrc/evalmetrics.hip) against the same metrics composed from library calls, and what the
evaluator adds to an evaluation rollout.

    python scripts/evalmetrics_time.py [--reps 20] [--skip-rollout] [--out profiles/eval_metrics.txt]

Part 1, per update, shapes [32,128,128,10,4], [32,128,128,1,4], [16,256,256,20,4], [32,86,86,10,4]: `reps` calls between two
events, median of 5 such windows (in-loop figure: inputs stay in the caches as far as they fit), and single calls after a
512 MB buffer was written (cold-cache figure, median of 7).  The yardstick is the vectorised composition a user would write
with torch on the GPU: torch.fft.rfft2 of pred - target, |.|^2 of the positive quadrant, ONE index_add_ over the shell table,
torch reductions for the pointwise keys, added into an accumulator tensor.  It is checked against the kernel before it is
timed.  Printed per shape: both times, their ratio, and the kernel's time against the two roofs - bytes = pred + target once
over 6.29 TB/s, FLOP = planes x (2 nx^2 ny + 2 nx ny^2) over 157.3 TF (fp32 MFMA) - with the binding one named.
Part 2: the DPOT-Tiny evaluation rollout (GraphedRollout, batch 32, T_ar = 10) with and without evaluator=, the two variants
alternated in one process, median of the rounds."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dpot_amd import RolloutEvaluator, ops  # noqa: E402
from oracle import dpot_ref as R  # noqa: E402   (model configurations only)

HBM, PEAK = 6.29e12, 157.3e12
SHAPES = [(32, 128, 128, 10, 4), (32, 128, 128, 1, 4), (16, 256, 256, 20, 4), (32, 86, 86, 10, 4)]


class Yardstick:
    """the accumulator of RolloutEvaluator out of torch calls"""

    def __init__(self, shape, device):
        B, nx, ny, T, C = shape
        self.K = min(nx // 2, ny // 2)
        sh = ops.eval_shell_table(nx, ny).astype(np.int64)
        self.idx = torch.from_numpy(np.where(sh < 0, self.K, sh).reshape(-1)).to(device)      # dropped -> a spare shell
        self.c = torch.zeros(3, C, dtype=torch.float64, device=device)
        self.tc = torch.zeros(4, T, C, dtype=torch.float64, device=device)
        self.spec = torch.zeros(T * C, self.K + 1, dtype=torch.float64, device=device)
        self.count = 0

    def update(self, pred, target):
        B, nx, ny, T, C = pred.shape
        e = pred - target
        ae, at, e2 = e.abs(), target.abs(), e * e
        s_ae, s_at, s_e2, s_t2 = ae.sum((1, 2)), at.sum((1, 2)), e2.sum((1, 2)), (target * target).sum((1, 2))
        m_e, m_t = ae.amax((1, 2)), at.amax((1, 2))
        bd = e2[:, 0].sum(1) + e2[:, -1].sum(1) + e2[:, :, 0].sum(1) + e2[:, :, -1].sum(1)
        self.tc[0] += (s_ae / s_at).sum(0)
        self.tc[1] += (s_e2 / s_t2).sqrt().sum(0)
        self.tc[2] += (m_e / m_t).sum(0)
        self.tc[3] += (bd / (2 * nx + 2 * ny)).sqrt().sum(0)
        self.c[0] += (s_ae.sum(1) / s_at.sum(1)).sum(0)
        self.c[1] += (s_e2.sum(1) / s_t2.sum(1)).sqrt().sum(0)
        self.c[2] += (m_e.amax(1) / m_t.amax(1)).sum(0)
        F = torch.fft.rfft2(e, dim=(1, 2))[:, :nx // 2, :ny // 2]
        pw = (F.real * F.real + F.imag * F.imag).sum(0).reshape(-1, T * C)                    # [(i, j), (t, c)]
        self.spec += torch.zeros(self.K + 1, T * C, device=e.device).index_add_(0, self.idx, pw).t()
        self.count += B

    def acc_vector(self):
        return np.concatenate([[0.0, 0.0], self.c.reshape(-1).cpu().numpy(), self.tc.reshape(-1).cpu().numpy(),
                               self.spec[:, :self.K].reshape(-1).cpu().numpy()])


def windows(fn, reps):
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def cold(fn, flush):
    out = []
    for _ in range(7):
        flush.add_(1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-rollout", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda"
    lines = [f"# {torch.cuda.get_device_name(0)}; RolloutEvaluator.update against the torch composition; microseconds per "
             f"update, median of 5 windows of {args.reps} calls [min, max]; cold = single calls after a 512 MB write"]
    flush = torch.zeros(128 << 20, device=dev)
    gen = torch.Generator(device=dev).manual_seed(16)
    worst = 0.0
    for shape in SHAPES:
        B, nx, ny, T, C = shape
        target = torch.randn(shape, device=dev, generator=gen) + 0.5
        pred = target + 0.05 * torch.randn(shape, device=dev, generator=gen)
        ev = RolloutEvaluator(dev, n_channels=C, T_max=T)
        ys = Yardstick(shape, dev)
        ev.update(pred, target)
        ys.update(pred, target)
        got = ev.read()
        want = ops.eval_finish(ys.acc_vector(), ys.count, nx, ny, T, C)
        dev_max = max(float(np.nanmax(np.abs(got[k] - want[k]) / np.abs(want[k]))) for k in ops.EVAL_KEYS)
        for _ in range(3):
            ev.update(pred, target)
            ys.update(pred, target)
        torch.cuda.synchronize()
        tk, tk_lo, tk_hi = windows(lambda: ev.update(pred, target), args.reps)
        ty, ty_lo, ty_hi = windows(lambda: ys.update(pred, target), args.reps)
        tk_cold, ty_cold = cold(lambda: ev.update(pred, target), flush), cold(lambda: ys.update(pred, target), flush)
        nbytes = 2.0 * 4.0 * pred.numel()
        flop = float(B * T * C) * (2.0 * nx * nx * ny + 2.0 * nx * ny * ny)
        t_hbm, t_mfma = nbytes / HBM * 1e6, flop / PEAK * 1e6
        bound = "FLOP" if t_mfma > t_hbm else "HBM"
        ratio = tk / ty
        worst = max(worst, ratio)
        lines.append(f"{list(shape)}: kernel {tk:.1f} [{tk_lo:.1f}, {tk_hi:.1f}]  yardstick {ty:.1f} [{ty_lo:.1f}, {ty_hi:.1f}]  "
                     f"ratio kernel/yardstick {ratio:.3f}  cold: kernel {tk_cold:.1f} yardstick {ty_cold:.1f}  "
                     f"largest relative deviation of a key {dev_max:.1e}")
        lines.append(f"    roofs: {nbytes / 1e6:.0f} MB -> {t_hbm:.1f} us = {t_hbm / tk:.3f} of the kernel's time; "
                     f"{flop / 1e9:.2f} GFLOP -> {t_mfma:.1f} us = {t_mfma / tk:.3f}; binding: {bound}")
        print("\n".join(lines[-2:]), flush=True)
        del pred, target, ev, ys
    lines.append(f"largest ratio kernel/yardstick over the shapes: {worst:.3f} (the bar is <= 1.0)")
    print(lines[-1], flush=True)
    if not args.skip_rollout:
        from dpot_amd import DPOTNet
        from dpot_amd.infer import GraphedRollout
        cfg = R.DPOTConfig(**R.TINY)
        model = DPOTNet(**R.TINY)
        model.load_state_dict(R.recipe_state_dict(cfg, salt=1))
        model.cuda().eval()
        B, T_ar, S = 32, 10, cfg.img_size
        g = GraphedRollout(model, torch.randn(B, S, S, cfg.in_timesteps, cfg.in_channels, device=dev))
        xx = torch.randn(B, S, S, cfg.in_timesteps, cfg.in_channels, device=dev)
        yy = torch.randn(B, S, S, T_ar, cfg.out_channels, device=dev)
        msk = torch.ones(B, S, S, 1, cfg.out_channels, device=dev)
        ev = RolloutEvaluator(dev, n_channels=cfg.out_channels, T_max=T_ar)
        variants = {"plain": {}, "plain'": {}, "evaluator": {"evaluator": ev}}

        def run(kw, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                g(xx, yy, msk, **kw)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / n

        for kw in variants.values():
            run(kw, 2)
        rows = {n: [] for n in variants}
        for r in range(6):
            order = list(variants) if r % 2 == 0 else list(variants)[::-1]
            for n in order:
                rows[n].append(run(variants[n], 3))
        med = {n: statistics.median(v) for n, v in rows.items()}
        spread = max(abs(a - b) for a, b in zip(rows["plain"], rows["plain'"]))
        lines.append(f"# DPOT-Tiny GraphedRollout, batch {B}, {T_ar} AR steps at {S} x {S}, ms per rollout, 6 alternated rounds "
                     "of 3 rollouts")
        lines.append("median: " + "  ".join(f"{n} {m:.3f}" for n, m in med.items()))
        lines.append(f"largest |plain - plain'| of a round (the spread): {spread:.3f} ms; evaluator - plain (medians): "
                     f"{med['evaluator'] - med['plain']:+.3f} ms per rollout ({(med['evaluator'] / med['plain'] - 1) * 100:+.2f} %)")
        print("\n".join(lines[-3:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
