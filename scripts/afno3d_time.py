#!/usr/bin/env python
"""Time the 3-D transforms (csrc/dft3.hip: ops.rfft3 / ops.irfft3) and the whole AFNO3D operator (functional.AFNO3DFn,
forward and forward + backward) against the same operator composed from torch.fft.

    python scripts/afno3d_time.py [--reps 50] [--out profiles/afno3d.txt]

Shapes [B, X*Y*Z, E]: [4, 8^3, 512], [4, 8^3, 1024], [2, 16^3, 512]; nb = 8, modes = 32 (kept box 8x8x5 and 16x16x8).
Yardstick: torch.fft.rfftn / irfftn over the three axes of the channels-last field, the box slice or the zero-pad, and the
layout copies between complex [B, mx, my, mz, E] and the planar-per-block rows [B*mx*my*mz, 2E] the mixer reads - the same
box, the same weights w(kz); the mixer in the middle of the whole operator is the project's own in both columns.
Transforms alone: a hipGraph of `reps` launches between two events, median of 5 replays.  Whole operator: `reps` eager calls
between two events after a warm-up, median of 5 (autograd included on both sides).  Per row: microseconds, the yardstick
over ours, and the algorithmic bytes (one read of the input, of the residual where there is one, one write of the output) over
the time as a fraction of the copy rate MEASURED in the same run (a 1 GiB device copy: read + write).  Every field here is
4 - 16 MB: it stays in the 256 MB Infinity Cache between launches, so the byte rates are cache rates, not HBM traffic."""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dpot_amd import ops  # noqa: E402
from dpot_amd.functional import _AFNO_PARAMS, AFNO3DFn, MixerWeights, _mixer_core, _mixer_core_bwd, _Sink, _WgradRoute  # noqa: E402

SHAPES = [(4, (8, 8, 8), 512), (4, (8, 8, 8), 1024), (2, (16, 16, 16), 512)]
NB, MODES = 8, 32


def median5(run, reps):
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return sorted(out)[2]


def time_graph(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return median5(g.replay, reps)


def time_eager(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()

    def run():
        for _ in range(reps):
            fn()
    return median5(run, reps)


def zw(mz, Z, cw, dev):
    w = torch.full((mz,), 2.0 if cw else 1.0, device=dev)
    if cw:
        w[0] = 1.0
        if Z % 2 == 0 and Z // 2 < mz:
            w[Z // 2] = 1.0
    return w.view(1, 1, 1, mz, 1)


def fft_fwd(x, dims, m3, nb, w):
    """composed rfft3: x [B, X*Y*Z, E] -> rows [B*mx*my*mz, 2E]"""
    B, _, E = x.shape
    mx, my, mz = m3
    S = torch.fft.rfftn(x.view(B, *dims, E), dim=(1, 2, 3), norm="ortho")[:, :mx, :my, :mz] * w
    S = S.reshape(-1, nb, E // nb)
    return torch.stack([S.real, S.imag], dim=2).reshape(-1, 2 * E)


def fft_inv(rows, B, dims, E, m3, nb, w, res):
    """composed irfft3 (w = w_cw / w_1: irfftn applies w_1 itself)"""
    mx, my, mz = m3
    r = rows.view(B, mx, my, mz, nb, 2, E // nb)
    S = torch.complex(r[..., 0, :], r[..., 1, :]).reshape(B, mx, my, mz, E) * w
    full = torch.zeros(B, dims[0], dims[1], dims[2] // 2 + 1, E, dtype=torch.complex64, device=rows.device)
    full[:, :mx, :my, :mz] = S
    y = torch.fft.irfftn(full, s=dims, dim=(1, 2, 3), norm="ortho").reshape(B, -1, E)
    return y + res if res is not None else y


class ComposedAFNO3D(torch.autograd.Function):
    """AFNO3DFn with the two transforms composed from torch.fft (the yardstick of the whole operator)"""

    @staticmethod
    def forward(ctx, x, packed, dims3, nb, m3, act, ws):
        B, tok, E = x.shape
        mw = MixerWeights.of(packed)
        S = fft_fwd(x, dims3, m3, nb, ws[0])
        O2, O1pre, O1 = _mixer_core(S, mw, nb, act)
        y = fft_inv(O2, B, dims3, E, m3, nb, ws[0], x)
        ctx.save_for_backward(S, O1pre, O1)
        ctx.args = (mw.for_backward(False), act, dims3, nb, m3, ws)
        return y

    @staticmethod
    def backward(ctx, dy):
        mw, act, dims3, nb, m3, ws = ctx.args
        B, _, E = dy.shape
        dO2 = fft_fwd(dy.contiguous(), dims3, m3, nb, ws[1])
        wg = _WgradRoute(_AFNO_PARAMS, [_Sink(None, False) for _ in range(4)])
        dS = _mixer_core_bwd(dO2, *ctx.saved_tensors, mw, nb, act, wg)
        return fft_inv(dS, B, dims3, E, m3, nb, ws[2], dy), None, None, None, None, None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "afno3d.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("afno3d_time: needs the GPU (nothing is measured without one)")
    dev = "cuda"
    lines = [f"device: {torch.cuda.get_device_name(0)}   reps {args.reps}, median of 5   nb {NB}, modes {MODES}"]
    big = torch.empty(1 << 28, device=dev)
    big2 = torch.empty_like(big)
    t_copy = time_graph(lambda: big2.copy_(big), 10)
    rate = 2.0 * big.numel() * 4 / (t_copy * 1e-6)
    lines.append(f"measured copy rate (1 GiB read + 1 GiB write): {rate / 1e12:.2f} TB/s")
    del big, big2
    hdr = f"{'op':34s} {'shape':18s} {'ours us':>9s} {'torch.fft us':>13s} {'yard/ours':>9s} {'MB':>7s} {'of copy rate':>12s}"
    lines.append(hdr)
    act = ops.ACT_IDS["gelu"]
    for B, dims3, E in SHAPES:
        m3 = ops.kept_modes3(dims3, MODES)
        tok = dims3[0] * dims3[1] * dims3[2]
        M3 = m3[0] * m3[1] * m3[2]
        shape = f"[{B},{dims3[0]}^3,{E}]"
        x = torch.randn(B, tok, E, device=dev)
        rows = torch.randn(B * M3, 2 * E, device=dev)
        w0, w1 = zw(m3[2], dims3[2], 0, dev), zw(m3[2], dims3[2], 1, dev)
        ws = (w0, w1, w0 / w1)                 # forward, adjoint of irfft3, adjoint of rfft3 fed to irfftn
        fb, ib = 4.0 * B * (tok * E + M3 * 2 * E), 4.0 * B * (2 * tok * E + M3 * 2 * E)
        # agreement first: a yardstick that computes something else measures nothing
        d = (ops.rfft3(x, dims3, NB, m3, 0) - fft_fwd(x, dims3, m3, NB, w0)).abs().max().item()
        d2 = (ops.irfft3(rows, B, dims3, E, NB, m3, 1, res=x) - fft_inv(rows, B, dims3, E, m3, NB, w0, x)).abs().max().item()
        assert d < 1e-4 and d2 < 1e-3, (d, d2)
        for what, ours, yard, nbytes in (
                ("rfft3", lambda: ops.rfft3(x, dims3, NB, m3, 0), lambda: fft_fwd(x, dims3, m3, NB, w0), fb),
                ("irfft3 (+ res)", lambda: ops.irfft3(rows, B, dims3, E, NB, m3, 1, res=x),
                 lambda: fft_inv(rows, B, dims3, E, m3, NB, w0, x), ib)):
            to, ty = time_graph(ours, args.reps), time_graph(yard, args.reps)
            lines.append(f"{what:34s} {shape:18s} {to:9.1f} {ty:13.1f} {ty / to:9.2f} {nbytes / 1e6:7.1f} "
                         f"{nbytes / (to * 1e-6) / rate:12.3f}")
            print(lines[-1], flush=True)
        bs = E // NB
        wts = [(torch.rand(2, NB, bs, bs, device=dev) - 0.5) * (2.0 / bs ** 0.5) if i % 2 == 0
               else (torch.rand(2, NB, bs, device=dev) - 0.5) * (2.0 / bs ** 0.5) for i in range(4)]
        packed = tuple(ops.AfnoPacks([(wts[0], wts[1]), (wts[2], wts[3])]).refresh())
        g = torch.randn(B, tok, E, device=dev)
        xg = x.clone().requires_grad_(True)

        def ours_f():
            with torch.no_grad():
                return AFNO3DFn.apply(x, *wts, dims3, NB, MODES, act, packed)

        def yard_f():
            with torch.no_grad():
                return ComposedAFNO3D.apply(x, packed, dims3, NB, m3, act, ws)

        def ours_fb():
            xg.grad = None
            AFNO3DFn.apply(xg, *wts, dims3, NB, MODES, act, packed).backward(g)

        def yard_fb():
            xg.grad = None
            ComposedAFNO3D.apply(xg, packed, dims3, NB, m3, act, ws).backward(g)

        dev_f = (ours_f() - yard_f()).abs().max().item()
        assert dev_f < 1e-3, dev_f
        for what, ours, yard in (("AFNO3D forward", ours_f, yard_f), ("AFNO3D forward + backward", ours_fb, yard_fb)):
            to, ty = time_eager(ours, args.reps), time_eager(yard, args.reps)
            lines.append(f"{what:34s} {shape:18s} {to:9.1f} {ty:13.1f} {ty / to:9.2f} {'-':>7s} {'-':>12s}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:3]))


if __name__ == "__main__":
    main()
