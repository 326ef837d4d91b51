#!/usr/bin/env python
"""A/B of the DPOT-Tiny batch-32 hipGraph train step with StepMetrics + dataset labels attached (cls_weight = 0) against the
same step without them, interleaved on one GPU: `--pairs` rounds of (plain, plain', attached), `--reps` replays each, median
of the rounds.  plain' is a second, independently captured plain step: |plain - plain'| is the pair-to-pair spread the
attached step is judged against.  Also counts the C-ABI calls each capture made (every new metrics entry point is exactly one
kernel launch; the plain capture must count what it counted before the feature existed).

    python scripts/metrics_ab.py [--pairs 6] [--reps 40] [--out profiles/metrics_ab.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dpot_amd import DPOTNet, StepMetrics, _lib, ops  # noqa: E402
from dpot_amd.train import FlatParams, FusedAdam, GraphedTrainStep  # noqa: E402

TINY = dict(img_size=128, patch_size=8, in_channels=4, out_channels=4, in_timesteps=10, out_timesteps=1, n_blocks=4,
            embed_dim=512, out_layer_dim=32, depth=4, modes=32, mlp_ratio=1, n_cls=12)


def make(attach, B=32):
    torch.manual_seed(0)
    model = DPOTNet(**TINY).cuda()
    opt = FusedAdam(FlatParams(model), lr=1e-4, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
    xx = torch.randn(B, 128, 128, 10, 4, device="cuda")
    yy = torch.randn(B, 128, 128, 1, 4, device="cuda")
    msk = torch.ones(B, 128, 128, 1, 4, device="cuda")
    kw = {}
    if attach:
        kw = dict(cls=torch.randint(0, 12, (B, 1), device="cuda"), metrics=StepMetrics("cuda", 1))
    calls = {}
    real = ops.check

    def counting(rc, what=""):
        if torch.cuda.is_current_stream_capturing():
            calls[what] = calls.get(what, 0) + 1
        return real(rc, what)

    ops.check = counting
    try:
        step = GraphedTrainStep(model, opt, xx, yy, msk, noise_scale=0.0005, warmup=2, **kw)
    finally:
        ops.check = real
    return step, calls


def time_step(step, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        step.replay(1e-4)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.load()
    variants = [("plain", False), ("plain'", False), ("attached", True)]
    steps = {}
    lines = [f"# {torch.cuda.get_device_name(0)}; DPOT-Tiny batch 32, hipGraph step, {args.reps} replays per timing, ms per step"]
    for name, attach in variants:
        steps[name], calls = make(attach)
        lines.append(f"C-ABI calls in the capture of {name}: {sum(calls.values())}"
                     + (f"  (metrics entries: { {k: v for k, v in calls.items() if k in ('cls_ce_fwd', 'rel_l2_combine', 'metrics_accum')} })"
                        if attach else ""))
    for name in steps:                                           # settle clocks and caches
        time_step(steps[name], 10)
    rows = {name: [] for name in steps}
    for r in range(args.pairs):
        order = list(steps) if r % 2 == 0 else list(steps)[::-1]
        for name in order:
            rows[name].append(time_step(steps[name], args.reps))
        lines.append(f"round {r}: " + "  ".join(f"{n} {rows[n][-1]:.4f}" for n in steps))
    med = {n: statistics.median(v) for n, v in rows.items()}
    spread = max(abs(a - b) for a, b in zip(rows["plain"], rows["plain'"]))
    lines.append("median: " + "  ".join(f"{n} {m:.4f}" for n, m in med.items()))
    lines.append(f"largest |plain - plain'| of a round (the spread): {spread:.4f} ms; "
                 f"attached - plain (medians): {med['attached'] - med['plain']:+.4f} ms "
                 f"({(med['attached'] / med['plain'] - 1) * 100:+.2f} %)")
    d = steps["attached"].metrics.read()
    lines.append(f"read() after the run: opt_steps {d['opt_steps']} samples {d['samples']} train_l2_step_avg "
                 f"{d['train_l2_step_avg']:.4f} cls_acc {d['cls_acc']:.3f} nonfinite_steps {d['nonfinite_steps']}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
