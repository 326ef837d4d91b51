#!/usr/bin/env python
"""Time RolloutEvaluator.update on 3-D fields (csrc/evalmetrics3d.hip) against the same accumulator composed from library
calls, against a plain device copy of the bytes the kernels must move, and what the evaluator adds to a graphed 3-D rollout.

    python scripts/evalmetrics3d_time.py [--reps 20] [--skip-rollout] [--out profiles/eval_metrics3d.txt]

Part 1, per update, shapes [4,64,64,64,1,4], [4,64,64,64,10,4], [1,128,128,128,1,4] and, for comparison in the same process,
the 2-D evaluator on [32,128,128,10,4]: `reps` calls between two events, median of 5 such windows (in-loop figure: inputs stay
in the caches as far as they fit), and single calls after a 512 MB buffer was written (cold-cache figure, median of 7).  The
yardstick is the vectorised composition a user would write with torch on the GPU: torch.fft.fftn over the three axes of
pred - target, |.|^2 of the positive octant, ONE index_add_ over the shell table, torch reductions for the pointwise keys,
added into an accumulator tensor.  It is checked against the kernel before it is timed.  Printed per shape: both times, their
ratio, the time of a device copy (Tensor.copy_) of the bytes the kernels must move - pred and target read once, the half
spectrum written once and read once: 4 x the bytes of one field, copied as 2 x that (a copy reads and writes) - and the
fraction of that copy's rate the update reaches.
Part 2: a small DPOTNet3D (32^3, patch 8) as GraphedRollout, batch 4, 3 AR steps, with and without evaluator=, the two
variants alternated in one process, median of the rounds."""
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

SHAPES = [(4, 64, 64, 64, 1, 4), (4, 64, 64, 64, 10, 4), (1, 128, 128, 128, 1, 4), (32, 128, 128, 10, 4)]


class Yardstick:
    """the accumulator of RolloutEvaluator out of torch calls, 2-D or 3-D fields"""

    def __init__(self, shape, device):
        sizes, (T, C) = shape[1:-2], shape[-2:]
        self.sp = tuple(range(1, 1 + len(sizes)))
        self.K = min(n // 2 for n in sizes)
        sh = ops.eval_shell_table(*sizes).astype(np.int64)
        self.idx = torch.from_numpy(np.where(sh < 0, self.K, sh).reshape(-1)).to(device)      # dropped -> a spare shell
        self.faces = float(2 * sum(sizes)) if len(sizes) == 2 else float(
            2 * (sizes[0] * sizes[1] + sizes[1] * sizes[2] + sizes[2] * sizes[0]))
        self.c = torch.zeros(3, C, dtype=torch.float64, device=device)
        self.tc = torch.zeros(4, T, C, dtype=torch.float64, device=device)
        self.spec = torch.zeros(T * C, self.K + 1, dtype=torch.float64, device=device)
        self.count = 0

    def update(self, pred, target):
        sp, (T, C) = self.sp, pred.shape[-2:]
        e = pred - target
        ae, at, e2 = e.abs(), target.abs(), e * e
        s_ae, s_at, s_e2, s_t2 = ae.sum(sp), at.sum(sp), e2.sum(sp), (target * target).sum(sp)
        m_e, m_t = ae.amax(sp), at.amax(sp)
        bd = 0.0
        for ax in sp:
            rest = tuple(a for a in sp if a != ax)
            rest = tuple(a - 1 if a > ax else a for a in rest)
            bd = bd + e2.select(ax, 0).sum(rest) + e2.select(ax, -1).sum(rest)
        self.tc[0] += (s_ae / s_at).sum(0)
        self.tc[1] += (s_e2 / s_t2).sqrt().sum(0)
        self.tc[2] += (m_e / m_t).sum(0)
        self.tc[3] += (bd / self.faces).sqrt().sum(0)
        self.c[0] += (s_ae.sum(1) / s_at.sum(1)).sum(0)
        self.c[1] += (s_e2.sum(1) / s_t2.sum(1)).sqrt().sum(0)
        self.c[2] += (m_e.amax(1) / m_t.amax(1)).sum(0)
        F = torch.fft.fftn(e, dim=sp)[(slice(None),) + tuple(slice(0, n // 2) for n in pred.shape[1:-2])]
        pw = (F.real * F.real + F.imag * F.imag).sum(0).reshape(-1, T * C)                    # [(i, j, k), (t, c)]
        self.spec += torch.zeros(self.K + 1, T * C, device=e.device).index_add_(0, self.idx, pw).t()
        self.count += pred.shape[0]

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
    gen = torch.Generator(device=dev).manual_seed(20)
    worst = 0.0
    for shape in SHAPES:
        three = len(shape) == 6
        T, C = shape[-2:]
        target = torch.randn(shape, device=dev, generator=gen) + 0.5
        pred = target + 0.05 * torch.randn(shape, device=dev, generator=gen)
        ev = RolloutEvaluator(dev, n_channels=C, T_max=T)
        ys = Yardstick(shape, dev)
        ev.update(pred, target)
        ys.update(pred, target)
        got = ev.read()
        want = ops.eval_finish(ys.acc_vector(), ys.count, *shape[1:])
        dev_max = max(float(np.nanmax(np.abs(got[k] - want[k]) / np.abs(want[k]))) for k in ops.EVAL_KEYS
                      if np.isfinite(want[k]).any())
        for _ in range(3):
            ev.update(pred, target)
            ys.update(pred, target)
        torch.cuda.synchronize()
        tk, tk_lo, tk_hi = windows(lambda: ev.update(pred, target), args.reps)
        ty, ty_lo, ty_hi = windows(lambda: ys.update(pred, target), args.reps)
        tk_cold, ty_cold = cold(lambda: ev.update(pred, target), flush), cold(lambda: ys.update(pred, target), flush)
        ratio = tk / ty
        if three:
            worst = max(worst, ratio)
        lines.append(f"{list(shape)}{'' if three else ' (the 2-D evaluator)'}: kernel {tk:.1f} [{tk_lo:.1f}, {tk_hi:.1f}]  "
                     f"yardstick {ty:.1f} [{ty_lo:.1f}, {ty_hi:.1f}]  ratio kernel/yardstick {ratio:.3f}  cold: kernel "
                     f"{tk_cold:.1f} yardstick {ty_cold:.1f}  largest relative deviation of a key {dev_max:.1e}")
        # the bytes the kernels must move: 3-D pred + target read, G written and read = 4 fields; 2-D pred + target = 2 fields
        fields = 4 if three else 2
        src = torch.empty(fields // 2 * pred.numel(), device=dev)
        dst = torch.empty_like(src)
        dst.copy_(src)
        tc_, tc_lo, tc_hi = windows(lambda: dst.copy_(src), args.reps)
        tc_cold = cold(lambda: dst.copy_(src), flush)
        moved = fields * 4.0 * pred.numel()
        lines.append(f"    device copy of the {moved / 1e6:.0f} MB the kernels must move: {tc_:.1f} [{tc_lo:.1f}, {tc_hi:.1f}] "
                     f"(cold {tc_cold:.1f}) = {moved / tc_ / 1e6:.2f} TB/s; the update reaches {tc_ / tk:.3f} of that rate "
                     f"(cold {tc_cold / tk_cold:.3f})")
        print("\n".join(lines[-2:]), flush=True)
        del pred, target, ev, ys, src, dst
    lines.append(f"largest ratio kernel/yardstick over the 3-D shapes: {worst:.3f} (the aim is <= 1.0)")
    print(lines[-1], flush=True)
    if not args.skip_rollout:
        from dpot_amd import DPOTNet3D
        from dpot_amd.infer import GraphedRollout
        torch.manual_seed(3)
        kw = dict(img_size=32, patch_size=8, in_channels=4, out_channels=4, in_timesteps=10, embed_dim=64, depth=4,
                  n_blocks=4, modes=4)
        model = DPOTNet3D(**kw).cuda().eval()
        B, T_ar, S = 4, 3, kw["img_size"]
        xx = torch.randn(B, S, S, S, kw["in_timesteps"], kw["in_channels"], device=dev)
        yy = torch.randn(B, S, S, S, T_ar, kw["out_channels"], device=dev)
        msk = torch.ones(B, S, S, S, 1, kw["out_channels"], device=dev)
        g = GraphedRollout(model, torch.randn_like(xx))
        ev = RolloutEvaluator(dev, n_channels=kw["out_channels"], T_max=T_ar)
        variants = {"plain": {}, "plain'": {}, "evaluator": {"evaluator": ev}}

        def run(kwargs, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                g(xx, yy, msk, **kwargs)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / n

        for kwargs in variants.values():
            run(kwargs, 2)
        rows = {n: [] for n in variants}
        for r in range(6):
            order = list(variants) if r % 2 == 0 else list(variants)[::-1]
            for n in order:
                rows[n].append(run(variants[n], 3))
        med = {n: statistics.median(v) for n, v in rows.items()}
        spread = max(abs(a - b) for a, b in zip(rows["plain"], rows["plain'"]))
        lines.append(f"# DPOTNet3D ({S}^3, patch {kw['patch_size']}, width {kw['embed_dim']}, depth {kw['depth']}) GraphedRollout, "
                     f"batch {B}, {T_ar} AR steps, ms per rollout, 6 alternated rounds of 3 rollouts")
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
