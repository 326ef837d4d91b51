#!/usr/bin/env python
"""Timings of the 3-D FNO baseline on one MI355X (written to profiles/fno3d.txt by `--out`), by the method of scripts/fno_time.py
(its `compare`: device events around windows of back-to-back calls, candidates alternating inside every round, the median):

  kernels    ops.fno3_rfft3 / fno3_irfft3 (both roles each) and ops.fno3_mix / fno3_mix_wgrad at two shapes - the reference default
             (B 4, 64^3, width 256, modes 12) and a narrow one (width 32) - beside two yardsticks taken in the same run:
               torch     the same operator composed from torch ops on the device as the reference's layer does it (channels-first
                         torch.fft.rfftn and four slices; a zero spectrum, four slice assignments and irfftn; one complex einsum
                         per corner; the backward through autograd) - not the code under test, not tuned
               copy      a plain device copy of the bytes the operator must read and write (the workspace between a transform's
                         two launches is NOT counted: it is traffic the kernels add)
  model      one training step (forward, loss, backward, clip, fused Adam with the pair rule) of FNO3d at both shapes, 4 layers,
             T_ar 1, eager and as one captured graph

    python scripts/fno3d_time.py --out profiles/fno3d.txt
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fno_time import compare, copy_of, emit, verdict  # noqa: E402  (scripts/)

SHAPES = [("default B4 64^3 C256 modes 12", 4, 64, 256, 12), ("narrow  B4 64^3 C32  modes 12", 4, 64, 32, 12)]


def corner_slices(N, m):
    return [(slice(0, m), slice(0, m)), (slice(N - m, N), slice(0, m)), (slice(0, m), slice(N - m, N)),
            (slice(N - m, N), slice(N - m, N))]


def kept_corners(m):
    lo, hi = slice(0, m), slice(m, 2 * m)
    return [(lo, lo), (hi, lo), (lo, hi), (hi, hi)]


def kernel_section(lines, window, rounds):
    from dpot_amd import ops
    for name, B, N, C, m in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, N, N, N, C, device="cuda", generator=gen)
        g = torch.randn(B, N, N, N, C, device="cuda", generator=gen)
        ws = [torch.randn(C, C, m, m, m, 2, device="cuda", generator=gen) / C for _ in range(4)]
        S = ops.fno3_rfft3(x, m, m, m)
        O = ops.fno3_mix(S, ws)
        y, _ = ops.fno3_irfft3(O, N, N, N)
        n_f, n_s, n_w = x.numel(), S.numel(), 4 * ws[0].numel()
        n_ws = B * N * 2 * m * m * 2 * C
        lines.append(f"shape {name}: field {4 * n_f / 1e6:.1f} MB, kept spectrum {4 * n_s / 1e6:.1f} MB, weights "
                     f"{4 * n_w / 1e6:.1f} MB, workspace between the two launches {4 * n_ws / 1e6:.1f} MB")
        # ---- the torch composition (channels-first, as the reference holds its fields) ----
        xc = x.permute(0, 4, 1, 2, 3).contiguous()
        gc = g.permute(0, 4, 1, 2, 3).contiguous()
        Oc = torch.complex(O[..., 0, :], O[..., 1, :]).permute(0, 4, 1, 2, 3).contiguous()          # [B, C, 2 m, 2 m, m]
        Sc = torch.complex(S[..., 0, :], S[..., 1, :]).permute(0, 4, 1, 2, 3).contiguous()
        wc = [torch.view_as_complex(w) for w in ws]

        def t_rfft(src=xc):
            full = torch.fft.rfftn(src, dim=(-3, -2, -1))
            return [full[:, :, r, q, :m] for r, q in corner_slices(N, m)]

        def t_irfft(Sk=Oc):
            half = Sk.new_zeros(B, C, N, N, N // 2 + 1)
            for (r, q), (kr, kq) in zip(corner_slices(N, m), kept_corners(m)):
                half[:, :, r, q, :m] = Sk[:, :, kr, kq]
            return torch.fft.irfftn(half, s=(N, N, N))

        def t_mix(Sk=Sc, w=wc):
            return [torch.einsum("bixyz,ioxyz->boxyz", Sk[:, :, kr, kq], wk) for (kr, kq), wk in zip(kept_corners(m), w)]

        ref = t_irfft().permute(0, 2, 3, 4, 1)
        err = ((y - ref).abs().max() / ref.abs().max()).item()
        lines.append(f"  (kernel irfft3 vs torch composition: max|d| / max|ref| = {err:.1e})")
        del ref
        xg = xc.clone().requires_grad_(True)
        Og = Oc.clone().requires_grad_(True)
        Sg = Sc.clone().requires_grad_(True)
        wg = [w.clone().requires_grad_(True) for w in wc]
        gs = torch.randn(B, C, m, m, m, dtype=torch.cfloat, device="cuda")

        def t_rfft_fb():
            xg.grad = None
            torch.autograd.backward(t_rfft(xg), [gs] * 4)

        def t_irfft_fb():
            Og.grad = None
            t_irfft(Og).backward(gc)

        def t_mix_fb():
            Sg.grad = None
            for w in wg:
                w.grad = None
            torch.autograd.backward(t_mix(Sg, wg), [gs] * 4)

        S_out, y_out = torch.empty_like(S), torch.empty_like(x)
        r = compare({"kernel rfft3": lambda: ops.fno3_rfft3(x, m, m, m, out=S_out),
                     "kernel rfft3 (adjoint role)": lambda: ops.fno3_rfft3(x, m, m, m, adjoint=True, out=S_out),
                     "torch rfftn + slices": t_rfft, "torch fwd+bwd": t_rfft_fb, "copy": copy_of(n_f + n_s)}, window, rounds)
        emit(lines, "field -> kept spectrum", r, f"   bytes {4 * (n_f + n_s) / 1e6:.1f} MB (the copy moves them twice)")
        t_bwd_r = r["torch fwd+bwd"][0] - r["torch rfftn + slices"][0]
        verdict(lines, "rfft3", r["kernel rfft3"][0], r["torch rfftn + slices"][0])
        r2 = compare({"kernel irfft3": lambda: ops.fno3_irfft3(O, N, N, N, out=y_out),
                      "kernel irfft3 (adjoint role)": lambda: ops.fno3_irfft3(O, N, N, N, adjoint=True, out=y_out),
                      "kernel irfft3 + add, gelu, pre": lambda: ops.fno3_irfft3(O, N, N, N, add=g, act=1, save_pre=True,
                                                                               out=y_out),
                      "torch zeros + assign + irfftn": t_irfft, "torch fwd+bwd": t_irfft_fb, "copy": copy_of(n_f + n_s)},
                     window, rounds)
        emit(lines, "kept spectrum -> field", r2, f"   bytes {4 * (n_f + n_s) / 1e6:.1f} MB")
        t_bwd_i = r2["torch fwd+bwd"][0] - r2["torch zeros + assign + irfftn"][0]
        verdict(lines, "irfft3", r2["kernel irfft3"][0], r2["torch zeros + assign + irfftn"][0])
        lines.append(f"    torch backward only: of rfftn {t_bwd_r:.1f} us (kernel: irfft3 in its adjoint role), of irfftn "
                     f"{t_bwd_i:.1f} us (kernel: rfft3 in its adjoint role)")
        verdict(lines, "backward of rfft3", r2["kernel irfft3 (adjoint role)"][0], t_bwd_r)
        verdict(lines, "backward of irfft3", r["kernel rfft3 (adjoint role)"][0], t_bwd_i)
        ds = [torch.empty_like(w) for w in ws]
        r3 = compare({"kernel mix": lambda: ops.fno3_mix(S, ws),
                      "kernel mix (data gradient)": lambda: ops.fno3_mix(O, ws, adjoint=True),
                      "kernel mix_wgrad": lambda: ops.fno3_mix_wgrad(S, O, ds),
                      "torch complex einsum x 4": t_mix, "torch fwd+bwd": t_mix_fb,
                      "copy weights + spectra": copy_of(n_w + 2 * n_s)}, window, rounds)
        emit(lines, "per-mode mixing", r3, f"   bytes {4 * (n_w + 2 * n_s) / 1e6:.1f} MB per launch")
        t_bwd_m = r3["torch fwd+bwd"][0] - r3["torch complex einsum x 4"][0]
        verdict(lines, "mix", r3["kernel mix"][0], r3["torch complex einsum x 4"][0])
        lines.append(f"    torch backward only (data and weight gradient together) {t_bwd_m:.1f} us")
        verdict(lines, "mix backward (data gradient + weight gradient)",
                r3["kernel mix (data gradient)"][0] + r3["kernel mix_wgrad"][0], t_bwd_m)
        del x, g, S, O, y, xc, gc, Oc, Sc, xg, Og, Sg, S_out, y_out
        torch.cuda.empty_cache()


def model_section(lines, window, rounds):
    from dpot_amd import FNO3d
    from dpot_amd.train import FlatParams, FusedAdam, GraphedTrainStep, train_step
    for name, B, N, C, m in SHAPES:
        cfg = dict(modes1=m, modes2=m, modes3=m, width=C, img_size=N, n_channels=1, in_timesteps=10, out_timesteps=1, n_layers=4)
        gen = torch.Generator(device="cuda").manual_seed(2)
        xx = torch.randn(B, N, N, N, 10, 1, device="cuda", generator=gen)
        yy = torch.randn(B, N, N, N, 1, 1, device="cuda", generator=gen)
        msk = torch.ones(B, N, N, N, 1, 1, device="cuda")
        steps = {}
        for graphed in (False, True):
            torch.manual_seed(3)
            mdl = FNO3d(**cfg).cuda()
            opt = FusedAdam(FlatParams(mdl), lr=1e-4, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
            if graphed:
                gstep = GraphedTrainStep(mdl, opt, xx, yy, msk, warmup=2)
                steps["FNO3d graphed"] = lambda s=gstep: s.replay(1e-4)
            else:
                steps["FNO3d eager"] = lambda a=mdl, o=opt: train_step(a, o, xx, yy, msk, lr=1e-4)
        res = compare(steps, window, rounds)
        lines.append(f"train step, FNO3d {name}, T 10, C 1, 4 layers, T_ar 1, fp32")
        for k, (med, lo, hi) in res.items():
            lines.append(f"    {k:26s} {med / 1e3:8.3f} ms   [{lo / 1e3:.3f} .. {hi / 1e3:.3f}]")
        del steps, xx, yy, msk
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fno3d_time.py measures on an MI355X; no GPU found")
    lines = [f"# scripts/fno3d_time.py  window {a.window} s  rounds {a.rounds}  device {torch.cuda.get_device_name(0)}",
             "# us per call: median [min .. max] over the rounds; a timed window = as many back-to-back calls as fill `window`",
             "# seconds between two device events; candidates alternating inside a round"]
    kernel_section(lines, a.window, a.rounds)
    if not a.skip_model:
        model_section(lines, a.window, a.rounds)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
