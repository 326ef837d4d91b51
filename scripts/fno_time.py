#!/usr/bin/env python
"""Timings of the FNO baseline on one MI355X (written to profiles/fno.txt by `--out`):

  kernels    ops.fno_rfft2 / fno_irfft2 (both roles each) and ops.fno_mix / fno_mix_wgrad at two shapes - the FNO header of the
             reference's configs (128 x 128, modes 20, width 32, batch 20) and a wide one (width 64, modes 32, batch 32) - beside
             two yardsticks taken in the same run, candidates alternating inside every round:
               torch     the same operator composed from torch ops on the device as the reference's layer does it (channels-first
                         torch.fft.rfft2 and two slices; a zero spectrum, slice assignment and irfft2; four real einsums per block;
                         the backward through autograd) - not the code under test, not tuned
               copy      a plain device copy of the bytes the kernel must read and write
             and, for the transforms, the share of the fp32 matrix / vector roof (157.3 TFLOP/s, the same for both engines) their
             dense sums reach, from the operation count of the two passes
  model      one training step (forward, loss, backward, clip, fused Adam), eager and as one captured graph, of FNO2d, beside the
             float32 torch restatement of the model (tests/fno_ref.py) with torch.optim.Adam on the device

    python scripts/fno_time.py --out profiles/fno.txt

Times are device events around a window of back-to-back calls (as many as fill `--window` seconds, 0.25 by default) after a
warm-up, the median of `rounds` rounds; no profiler."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROOF = 157.3e12
SHAPES = [("header  B20 128x128 C32 modes 20", 20, 128, 128, 32, 20, 20), ("wide    B32 128x128 C64 modes 32", 32, 128, 128, 64, 32, 32)]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def compare(fns, window, rounds):
    """{name: (median us, min, max)} with the candidates alternating inside every round; every candidate's timed window holds as
    many back-to-back calls as fill `window` seconds (from a trial of 10 calls after the warm-up), at least 10"""
    iters = {}
    for k, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        iters[k] = max(10, int(window * 1e6 / max(timed(fn, 10), 1e-3)) + 1)
    rec = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            rec[k].append(timed(fn, iters[k]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in rec.items()}


def copy_of(n_floats):
    src = torch.empty(n_floats, device="cuda")
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


def four_einsum_mix(s_re, s_im, w):
    """one block of the per-mode mixing as FOUR REAL einsums - the composition the reference's layer uses instead of one complex
    product - on channels-first planes s_re, s_im [B, Cin, rows, m2] and w [2, Cin, Cout, rows, m2]:
    (a + ib)(p + iq) = (ap - bq) + i(aq + bp)"""
    p, q = w[0], w[1]
    ap, bq = torch.einsum("ncrk,cdrk->ndrk", s_re, p), torch.einsum("ncrk,cdrk->ndrk", s_im, q)
    aq, bp = torch.einsum("ncrk,cdrk->ndrk", s_re, q), torch.einsum("ncrk,cdrk->ndrk", s_im, p)
    return torch.complex(ap - bq, aq + bp)


def emit(lines, title, res, extra=""):
    lines.append(f"  {title}{extra}")
    for k, (med, lo, hi) in res.items():
        lines.append(f"    {k:22s} {med:9.1f} us   [{lo:.1f} .. {hi:.1f}]")


def verdict(lines, what, t_kernel, t_torch):
    lines.append(f"    -> {what}: kernel {'faster' if t_kernel < t_torch else 'SLOWER'} than the composition "
                 f"({t_torch / t_kernel:.2f}x)")


def kernel_section(lines, window, rounds):
    from dpot_amd import ops
    for name, B, H, W, C, m1, m2 in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, H, W, C, device="cuda", generator=gen)
        g = torch.randn(B, H, W, C, device="cuda", generator=gen)
        w1 = torch.randn(2, C, C, m1, m2, device="cuda", generator=gen) / C
        w2 = torch.randn(2, C, C, m1, m2, device="cuda", generator=gen) / C
        X = ops.fno_rfft2(x, m1, m2)
        O = ops.fno_mix(X, w1, w2)
        y, _ = ops.fno_irfft2(O, H, W)
        n_f, n_s, n_w = x.numel(), X.numel(), 2 * w1.numel()
        lines.append(f"shape {name}: field {4 * n_f / 1e6:.1f} MB, kept spectrum {4 * n_s / 1e6:.1f} MB, weights "
                     f"{4 * n_w / 1e6:.1f} MB")
        # ---- the torch composition (channels-first, as the reference holds its fields) ----
        xc = x.permute(0, 3, 1, 2).contiguous()
        gc = g.permute(0, 3, 1, 2).contiguous()
        Oc = torch.complex(O[:, :, :, 0], O[:, :, :, 1]).permute(0, 3, 1, 2).contiguous()          # [B, C, 2 m1, m2]
        Xc = torch.complex(X[:, :, :, 0], X[:, :, :, 1]).permute(0, 3, 1, 2).contiguous()

        def t_rfft():
            full = torch.fft.rfft2(xc)
            return full[:, :, 0:m1, 0:m2], full[:, :, H - m1:H, 0:m2]

        def t_irfft(S=Oc):
            # a zero half spectrum of the full size, the two kept corner blocks assigned, the library's inverse
            half = S.new_zeros(B, C, H, W // 2 + 1)
            low, high = S.split(m1, dim=2)
            half[:, :, 0:m1, 0:m2] = low
            half[:, :, H - m1:H, 0:m2] = high
            return torch.fft.irfft2(half, s=(H, W))

        def t_mix(S=Xc, a=w1, b=w2):
            low, high = S.split(m1, dim=2)
            return four_einsum_mix(low.real, low.imag, a), four_einsum_mix(high.real, high.imag, b)

        ref = t_irfft().permute(0, 2, 3, 1)
        err = ((y - ref).abs().max() / ref.abs().max()).item()
        lines.append(f"  (kernel irfft2 vs torch composition: max|d| / max|ref| = {err:.1e})")
        xg = xc.clone().requires_grad_(True)
        Og = Oc.clone().requires_grad_(True)
        Xg = Xc.clone().requires_grad_(True)
        w1g, w2g = w1.clone().requires_grad_(True), w2.clone().requires_grad_(True)
        gs = torch.randn(B, C, m1, m2, dtype=torch.cfloat, device="cuda")

        def t_rfft_fb():
            full = torch.fft.rfft2(xg)
            xg.grad = None
            torch.autograd.backward([full[:, :, 0:m1, 0:m2], full[:, :, H - m1:H, 0:m2]], [gs, gs])

        def t_irfft_fb():
            Og.grad = None
            t_irfft(Og).backward(gc)

        def t_mix_fb():
            Xg.grad = w1g.grad = w2g.grad = None
            a, b = t_mix(Xg, w1g, w2g)
            torch.autograd.backward([a, b], [gs, gs])

        # ---- transforms ----
        fl_f = 4.0 * B * H * W * C * m2 + 8.0 * B * 2 * m1 * m2 * C * H          # y pass (real in, complex out), x pass (complex)
        fl_i = 8.0 * B * 2 * m1 * m2 * C * H + 4.0 * B * H * W * C * m2
        S_out = torch.empty_like(X)
        y_out = torch.empty_like(x)
        r = compare({"kernel rfft2": lambda: ops.fno_rfft2(x, m1, m2, out=S_out),
                     "kernel rfft2 (adjoint role)": lambda: ops.fno_rfft2(x, m1, m2, adjoint=True, out=S_out),
                     "torch rfft2 + slices": t_rfft, "torch fwd+bwd": t_rfft_fb, "copy": copy_of(n_f + n_s)}, window, rounds)
        emit(lines, "field -> kept spectrum", r, f"   bytes {4 * (n_f + n_s) / 1e6:.1f} MB (the copy moves them twice), "
             f"{fl_f / 1e9:.2f} GFLOP: {100 * fl_f / (r['kernel rfft2'][0] * 1e-6) / ROOF:.1f} % of the fp32 roof")
        t_bwd_r = r["torch fwd+bwd"][0] - r["torch rfft2 + slices"][0]
        verdict(lines, "rfft2", r["kernel rfft2"][0], r["torch rfft2 + slices"][0])
        r2 = compare({"kernel irfft2": lambda: ops.fno_irfft2(O, H, W, out=y_out),
                      "kernel irfft2 (adjoint role)": lambda: ops.fno_irfft2(O, H, W, adjoint=True, out=y_out),
                      "kernel irfft2 + add, gelu, pre": lambda: ops.fno_irfft2(O, H, W, add=g, act=1, save_pre=True, out=y_out),
                      "torch zeros + assign + irfft2": t_irfft, "torch fwd+bwd": t_irfft_fb, "copy": copy_of(n_f + n_s)},
                     window, rounds)
        emit(lines, "kept spectrum -> field", r2, f"   bytes {4 * (n_f + n_s) / 1e6:.1f} MB, {fl_i / 1e9:.2f} GFLOP: "
             f"{100 * fl_i / (r2['kernel irfft2'][0] * 1e-6) / ROOF:.1f} % of the fp32 roof")
        t_bwd_i = r2["torch fwd+bwd"][0] - r2["torch zeros + assign + irfft2"][0]
        verdict(lines, "irfft2", r2["kernel irfft2"][0], r2["torch zeros + assign + irfft2"][0])
        lines.append(f"    torch backward only: of rfft2 {t_bwd_r:.1f} us (kernel: irfft2 in its adjoint role), of irfft2 {t_bwd_i:.1f} us "
                     "(kernel: rfft2 in its adjoint role)")
        verdict(lines, "backward of rfft2", r2["kernel irfft2 (adjoint role)"][0], t_bwd_r)
        verdict(lines, "backward of irfft2", r["kernel rfft2 (adjoint role)"][0], t_bwd_i)
        # ---- mixing ----
        d1, d2 = torch.empty_like(w1), torch.empty_like(w2)
        r3 = compare({"kernel mix": lambda: ops.fno_mix(X, w1, w2),
                      "kernel mix (data gradient)": lambda: ops.fno_mix(O, w1, w2, adjoint=True),
                      "kernel mix_wgrad": lambda: ops.fno_mix_wgrad(X, O, d1, d2),
                      "torch 4 einsums x 2": t_mix, "torch fwd+bwd": t_mix_fb,
                      "copy weights + spectra": copy_of(n_w + 2 * n_s)}, window, rounds)
        emit(lines, "per-mode mixing", r3, f"   bytes {4 * (n_w + 2 * n_s) / 1e6:.1f} MB per launch")
        t_bwd_m = r3["torch fwd+bwd"][0] - r3["torch 4 einsums x 2"][0]
        verdict(lines, "mix", r3["kernel mix"][0], r3["torch 4 einsums x 2"][0])
        lines.append(f"    torch backward only (data and weight gradient together) {t_bwd_m:.1f} us")
        verdict(lines, "mix backward (data gradient + weight gradient)", r3["kernel mix (data gradient)"][0] + r3["kernel mix_wgrad"][0],
                t_bwd_m)
        del x, g, X, O, y, xc, gc, Oc, Xc, xg, Og, Xg
        torch.cuda.empty_cache()


def model_section(lines, window, rounds):
    import fno_ref as FR
    from dpot_amd import FNO2d
    from dpot_amd.train import FlatParams, FusedAdam, GraphedTrainStep, train_step
    cfg = dict(modes1=20, modes2=20, width=32, img_size=128, n_channels=4, in_timesteps=10, out_timesteps=1, n_layers=4,
               patch_size=1, use_ln=False, normalize=False, n_cls=12)
    B, S, T, C = 20, cfg["img_size"], cfg["in_timesteps"], cfg["n_channels"]
    gen = torch.Generator(device="cuda").manual_seed(2)
    xx = torch.randn(B, S, S, T, C, device="cuda", generator=gen)
    yy = torch.randn(B, S, S, 1, C, device="cuda", generator=gen)
    msk = torch.ones(B, S, S, 1, C, device="cuda")
    torch.manual_seed(3)
    m = FNO2d(**cfg).cuda()
    opt = FusedAdam(FlatParams(m), lr=1e-4, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
    torch.manual_seed(3)
    m2 = FNO2d(**cfg).cuda()
    opt2 = FusedAdam(FlatParams(m2), lr=1e-4, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
    step = GraphedTrainStep(m2, opt2, xx, yy, msk, warmup=2)
    torch.manual_seed(3)
    sd = {k: v.detach().clone().cuda().requires_grad_(True) for k, v in FNO2d(**cfg).state_dict().items()}
    topt = torch.optim.Adam(list(sd.values()), lr=1e-4, betas=(0.9, 0.9), weight_decay=1e-6)

    def torch_step():
        topt.zero_grad(set_to_none=True)
        pred, _ = FR.fno_forward(sd, xx, cfg)
        loss = FR.R.rel_l2_loss(pred, yy, msk)
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p for p in sd.values() if p.grad is not None], 10000.0)
        topt.step()

    res = compare({"FNO2d eager": lambda: train_step(m, opt, xx, yy, msk, lr=1e-4), "FNO2d graphed": lambda: step.replay(1e-4),
                   "torch restatement, eager": torch_step}, window, rounds)
    lines.append(f"train step, the header's FNO (128 x 128, modes 20, width 32, T 10, C 4, P 1, 4 layers), batch {B}, T_ar 1, fp32")
    for k, (med, lo, hi) in res.items():
        lines.append(f"    {k:26s} {med / 1e3:8.3f} ms   [{lo / 1e3:.3f} .. {hi / 1e3:.3f}]")
    lines.append("    (the restatement's layer is two dense complex einsums, not torch.fft: a yardstick for the step around the "
                 "kernels, not for them)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fno_time.py measures on an MI355X; no GPU found")
    lines = [f"# scripts/fno_time.py  window {a.window} s  rounds {a.rounds}  device {torch.cuda.get_device_name(0)}",
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
