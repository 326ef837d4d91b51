#!/usr/bin/env python
"""Time the fused LAMB step against the fused Adam step on DPOT-Tiny- and DPOT-M-sized flat buffers (the models' own
parameter size lists, FlatParams padding), each as a replayed hipGraph of the optimiser launches alone.

    python scripts/lamb_time.py [--reps 200] [--out profiles/lamb_time.json]

Prints one JSON line per (model, optimiser): microseconds per step (median of 5 timed batches of `reps` replays) and the
bytes the step must move at the least (Adam and LAMB adam=True: read p, g, m, v + write p, m, v = 28 B per parameter;
LAMB adam=False: + read p, m, v + write p = 44 B).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dpot_amd import ops  # noqa: E402
from dpot_amd.model import DPOTNet  # noqa: E402
from oracle import dpot_ref as R  # noqa: E402   (model configurations only)


def sizes_of(cfg):
    with torch.device("meta"):
        net = DPOTNet(**cfg)
    return [p.numel() for _, p in net.named_parameters()]


def time_graph(fn, reps):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            g.replay()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    out.sort()
    return out[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda"
    rows = []
    for name, cfg in (("DPOT-Tiny", R.TINY), ("DPOT-M", R.MEDIUM)):
        sizes = sizes_of(cfg)
        offs, off = [], 0
        for n in sizes:
            offs.append(off)
            off += (n + 3) // 4 * 4
        n_par = sum(sizes)
        p = torch.randn(off, device=dev) * 0.02
        g = torch.randn(off, device=dev) * 1e-3
        m = torch.zeros(off, device=dev)
        v = torch.zeros(off, device=dev)
        hyper = torch.zeros(16, device=dev)
        step = torch.zeros(1, dtype=torch.int64, device=dev)
        ops.adam_stage(hyper, step, 1e-6, 0.9, 0.999, 1e-8, 0.0, 0.0)
        t_adam = time_graph(lambda: ops.adam_step(p, g, m, v, hyper, None), args.reps)
        plan = ops.LambPlan(offs, sizes, off, dev)
        norms = torch.zeros(3 * len(sizes), device=dev)
        lh = torch.zeros(16, device=dev)
        ops.lamb_stage(lh, step, 1e-6, 0.9, 0.999, 1e-6, 1e-4, 0.0, 10.0, False)
        res = {"adam_kernel": (t_adam, 28)}
        for adam in (True, False):
            t = time_graph(lambda: ops.lamb_step(plan, p, g, m, v, lh, None, norms, adam=adam), args.reps)
            res["lamb adam=True" if adam else "lamb adam=False"] = (t, 28 if adam else 44)
        for opt, (t, bpp) in res.items():
            row = {"model": name, "params": n_par, "tensors": len(sizes), "chunks": plan.nchunks, "step": opt,
                   "us": round(t, 2), "TB_s": round(bpp * n_par / (t * 1e-6) / 1e12, 3),
                   "vs_adam": round(t / t_adam, 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del p, g, m, v
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
