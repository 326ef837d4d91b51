#!/usr/bin/env python
"""Bit-level fingerprint of the table plans of dpot_amd/ops.py (ResizePlan, Resize3Plan, EvalPlan, AAPlan, FNOPlan) and of the
operators that read them, for comparing two trees that must build the same tables and compute the same thing:
python scripts/plan_fingerprint.py [--host] > a.txt   in each tree (on the GPU: on the same machine with the same built
library), then `diff`.

One SHA-256 line per item.  --host, no GPU needed: every entry of the host dicts (ResizePlan.host_matrices,
Resize3Plan.host_matrices, EvalPlan.host_tables), the anti-aliasing word tables and the fp32-rounded FNO twiddles - key name,
dtype, shape and bytes, in dict order.  Without --host, on the GPU, also every device tensor of the cached plans after upload and
the outputs of the operators on seeded inputs at the same sizes."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dpot_amd import ops  # noqa: E402

# (nx, ny, mx, my): min(n, m) even with n != m on the full-spectrum axis (the imaginary term exists: up, down and the smallest),
# min(n, m) odd, n == m; no size a multiple of 16 or 32 but the two 16s
RESIZE = [(10, 12, 18, 20), (20, 18, 6, 7), (4, 4, 6, 6), (9, 11, 16, 13), (12, 12, 12, 12)]
# (nx, ny, nz, mx, my, mz): terms = 1 (X odd, Y equal), 2 (X only), 2 (Y only), 4, 4 (the smallest)
RESIZE3 = [(5, 7, 9, 8, 7, 6), (6, 7, 9, 10, 9, 7), (7, 6, 9, 9, 10, 7), (4, 6, 5, 6, 10, 8), (4, 4, 4, 6, 6, 6)]
RESIZE3_TERMS = [1, 2, 2, 4, 4]
EVAL = [(4, 4), (10, 12), (17, 9), (4, 4, 4), (6, 5, 7)]
AA = [(2, 2, 0, 0), (2, 2, 3, 3), (5, 7, 0, 0), (5, 7, 9, 8), (12, 9, 17, 9)]
FNO = [(4, 4, 1, 1), (11, 13, 3, 4), (20, 18, 5, 6), (4, 4, 4, 1, 1, 1), (7, 6, 9, 3, 2, 4)]


def tag(sizes):
    return "x".join(map(str, sizes))


def line(name, items):
    """items: (key, numpy array | None) in order"""
    h = hashlib.sha256()
    for key, a in items:
        h.update(key.encode())
        if a is None:
            h.update(b"<none>")
            continue
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype}{a.shape}".encode())
        h.update(a.tobytes())
    print(f"{name}: {h.hexdigest()}", flush=True)


def twiddles(sizes):
    tabs = (ops.fno_twiddles if len(sizes) == 4 else ops.fno3_twiddles)(*sizes)
    return [(k, t.astype(np.float32)) for k, t in zip(("tx", "ty", "tz"), tabs)]


def host():
    for s in RESIZE:
        line(f"host ResizePlan {tag(s)}", ops.ResizePlan.host_matrices(*s).items())
    for s, terms in zip(RESIZE3, RESIZE3_TERMS):
        h = ops.Resize3Plan.host_matrices(*s)
        assert 1 + (h["nux"] is not None) + (h["uy2"] is not None) + (h["nux"] is not None and h["uy2"] is not None) == terms, s
        line(f"host Resize3Plan {tag(s)}", h.items())
    for s in EVAL:
        line(f"host EvalPlan {tag(s)}", ops.EvalPlan.host_tables(*s).items())
    for h, w, H, W in AA:
        line(f"host aa_core_tables {h}x{w}", [("tab", ops.aa_core_tables(h, w))])
        if H or W:
            line(f"host aa_up_tables {tag((h, w, H, W))}", [("vtab", ops.aa_up_tables(h, w, H, W))])
    for s in FNO:
        line(f"host fno twiddles {tag(s)}", twiddles(s))


def cpu(t):
    return None if t is None else t.detach().contiguous().cpu().numpy()


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


def device():
    for k, s in enumerate(RESIZE):
        y = ops.spectral_resize(seeded((2, s[0], s[1], 3, 2), 10 + k), s[2:])
        line(f"dev ResizePlan {tag(s)}", [(n, cpu(t)) for n, t in ops.resize_plan(*s, "cuda").dev.items()])
        line(f"out spectral_resize {tag(s)}", [("y", cpu(y))])
    for k, (s, terms) in enumerate(zip(RESIZE3, RESIZE3_TERMS)):
        y = ops.spectral_resize3(seeded((2, *s[:3], 3, 2), 20 + k), s[3:])
        plan = ops.resize3_plan(*s, "cuda")
        assert plan.terms == terms, (s, plan.terms)
        line(f"dev Resize3Plan {tag(s)}", [(n, cpu(t)) for n, t in plan.dev.items()])
        line(f"out spectral_resize3 {tag(s)}", [("y", cpu(y))])
    for k, s in enumerate(EVAL):
        T, C = 3, 2
        acc = ops.eval_acc_alloc(*s, T, C, "cuda")
        for b in range(2):                                  # two batches: the accumulator adds
            ops.eval_metrics_update(seeded((2, *s, T, C), 30 + 2 * k + b), seeded((2, *s, T, C), 60 + 2 * k + b), acc)
        line(f"dev EvalPlan {tag(s)}", [(n, cpu(t)) for n, t in ops.eval_plan(*s, "cuda").dev.items()])
        line(f"out eval_metrics_update {tag(s)}", [("acc", cpu(acc))])
    for k, (h, w, H, W) in enumerate(AA):
        x, bias = seeded((2, h, w, 6), 90 + k), seeded((3,), 100 + k)
        y = ops.aa_lrelu(x, bias, (H, W) if H or W else None, slope=0.2)
        dx, dbias = ops.aa_lrelu_bwd(x, seeded(tuple(y.shape), 110 + k), 3, slope=0.2)
        plan = ops.aa_plan(h, w, H, W, "cuda")
        line(f"dev AAPlan {tag((h, w, H, W))}", [("tab", cpu(plan.tab)), ("vtab", cpu(plan.vtab))])
        line(f"out aa_lrelu {tag((h, w, H, W))}", [("y", cpu(y))])
        line(f"out aa_lrelu_bwd {tag((h, w, H, W))}", [("dx", cpu(dx)), ("dbias", cpu(dbias))])
    for k, s in enumerate(FNO):
        rank = len(s) // 2
        dims, modes = s[:rank], s[rank:]
        x = seeded((2, *dims, 5), 120 + k)
        rfft, irfft, plan = ((ops.fno_rfft2, ops.fno_irfft2, ops.fno_plan) if rank == 2 else
                             (ops.fno3_rfft3, ops.fno3_irfft3, ops.fno3_plan))
        S = rfft(x, *modes)
        y, pre = irfft(S, *dims, add=x, act=ops.ACT_IDS["gelu"], save_pre=True)
        gS = rfft(x, *modes, adjoint=True)
        gx, _ = irfft(S, *dims, adjoint=True)
        p = plan(*s, "cuda")
        line(f"dev FNOPlan {tag(s)}", [(n, cpu(t)) for n, t in zip(("tx", "ty", "tz"), p.tables)])
        line(f"out fno rfft {tag(s)}", [("S", cpu(S)), ("adjoint", cpu(gS))])
        line(f"out fno irfft {tag(s)}", [("y", cpu(y)), ("pre", cpu(pre)), ("adjoint", cpu(gx))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true", help="the host tables only: needs no GPU")
    args = ap.parse_args()
    host()
    if not args.host:
        if not torch.cuda.is_available():
            raise SystemExit("plan_fingerprint: needs the GPU (or --host)")
        device()
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
