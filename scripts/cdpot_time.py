#!/usr/bin/env python
"""Timings of the CDPOT model on one MI355X (written to profiles/cdpot.txt by `--out`):

  operator   ops.aa_lrelu / ops.aa_lrelu_bwd at the two shapes the Tiny model line of configs/cdpot_parallel.yaml runs at
             batch 32 (128 x 128 image, patch 8): the embed form [32, 16, 16, 10 * 35] and the output form
             [32, 16, 16, 32] -> 128 x 128, beside two yardsticks taken in the same run, rounds alternating:
               torch     the same operator composed from torch ops on the device (permute, three F.interpolate(antialias=True),
                         leaky_relu, bias, permute back; backward through autograd) - not the code under test, not tuned
               copy      a plain device copy of the bytes the kernels must read and write
  model      one training step (forward, loss, backward, clip, fused Adam), eager and as one captured graph, of CDPOTNet and of
             DPOTNet with the same hyper-parameters, batch 32

    python scripts/cdpot_time.py --out profiles/cdpot.txt

Times are device events around `iters` back-to-back calls after a warm-up, the median of `rounds` rounds; no profiler."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TINY = dict(img_size=128, patch_size=8, in_channels=4, out_channels=4, in_timesteps=10, out_timesteps=1, n_blocks=4,
            embed_dim=512, out_layer_dim=32, depth=4, modes=32, mlp_ratio=1, n_cls=12)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def compare(fns, iters, rounds):
    """{name: (median us, min, max)} with the candidates alternating inside every round"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rec = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            rec[k].append(timed(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in rec.items()}


def torch_composition(x_cf, bias, size, out_size, slope):
    """the reference's operator on a channels-first tensor, from a channels-last input and back"""
    u = F.interpolate(x_cf, size=2 * size, mode="bilinear", antialias=True)
    u = F.leaky_relu(u, slope)
    u = F.interpolate(u, size=size, mode="bilinear", antialias=True)
    if out_size != size:
        u = F.interpolate(u, size=out_size, mode="bilinear", antialias=True)
    return u.permute(0, 2, 3, 1) + bias


def operator_section(lines, iters, rounds):
    from dpot_amd import ops
    shapes = [("embed  [32,16,16,350] bias[35]", (32, 16, 16, 350), 35, None),
              ("output [32,16,16,32] -> 128x128", (32, 16, 16, 32), 32, 128)]
    for name, shape, Cb, out in shapes:
        N, h, w, C = shape
        H = out or h
        gen = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(shape, device="cuda", generator=gen)
        g = torch.randn(N, H, H, C, device="cuda", generator=gen)
        bias = torch.randn(Cb, device="cuda", generator=gen)
        y = torch.empty(N, H, H, C, device="cuda")
        # the torch composition (the reference applies its bias per channel: the embed form runs it on [N * T, hid, h, w])
        T = C // Cb

        def torch_fwd():
            xc = x.view(N, h, w, T, Cb).permute(0, 3, 4, 1, 2).reshape(N * T, Cb, h, w)
            o = torch_composition(xc, bias, h, H, 0.01)                          # [N * T, H, H, Cb]
            return o.view(N, T, H, H, Cb).permute(0, 2, 3, 1, 4).reshape(N, H, H, C).contiguous()

        xg = x.clone().requires_grad_(True)
        bg = bias.clone().requires_grad_(True)

        def torch_fwd_bwd():
            xc = xg.view(N, h, w, T, Cb).permute(0, 3, 4, 1, 2).reshape(N * T, Cb, h, w)
            o = torch_composition(xc, bg, h, H, 0.01)
            o = o.view(N, T, H, H, Cb).permute(0, 2, 3, 1, 4).reshape(N, H, H, C)
            xg.grad = bg.grad = None
            o.backward(g)

        ref = torch_fwd()
        got = ops.aa_lrelu(x, bias, out)
        err = ((got - ref).abs().max() / ref.abs().max()).item()
        # bytes the kernels must move: forward reads x, writes y; backward reads x and dy, writes dx
        src_f = torch.empty(x.numel() + y.numel(), device="cuda")
        dst_f = torch.empty_like(src_f)
        src_b = torch.empty(2 * x.numel() + y.numel(), device="cuda")
        dst_b = torch.empty_like(src_b)
        fwd = compare({"kernel": lambda: ops.aa_lrelu(x, bias, out, out=y), "torch": torch_fwd,
                       "copy": lambda: dst_f.copy_(src_f)}, iters, rounds)
        t_f = compare({"torch fwd": torch_fwd}, iters, rounds)["torch fwd"][0]
        bwd = compare({"kernel": lambda: ops.aa_lrelu_bwd(x, g, Cb), "torch fwd+bwd": torch_fwd_bwd,
                       "copy": lambda: dst_b.copy_(src_b)}, iters, rounds)
        lines.append(f"operator {name}   (kernel vs torch composition: max|d| / max|ref| = {err:.1e})")
        lines.append(f"  forward   bytes {4 * src_f.numel() / 1e6:7.1f} MB (the copy moves them twice: read + write)")
        for k, (med, lo, hi) in fwd.items():
            lines.append(f"    {k:14s} {med:9.1f} us   [{lo:.1f} .. {hi:.1f}]")
        lines.append(f"  backward  bytes {4 * src_b.numel() / 1e6:7.1f} MB")
        for k, (med, lo, hi) in bwd.items():
            lines.append(f"    {k:14s} {med:9.1f} us   [{lo:.1f} .. {hi:.1f}]")
        tb = bwd["torch fwd+bwd"][0] - t_f
        lines.append(f"    torch bwd only (fwd+bwd minus fwd {t_f:.1f}) {tb:9.1f} us")
        ok_f, ok_b = fwd["kernel"][0] < fwd["torch"][0], bwd["kernel"][0] < tb
        lines.append(f"  kernel faster than the composition: forward {'yes' if ok_f else 'NO'} "
                     f"({fwd['torch'][0] / fwd['kernel'][0]:.1f}x), backward {'yes' if ok_b else 'NO'} ({tb / bwd['kernel'][0]:.1f}x)")


def model_section(lines, batch, iters, rounds):
    from dpot_amd import CDPOTNet, DPOTNet
    from dpot_amd.train import FlatParams, FusedAdam, GraphedTrainStep, train_step
    S, T, C = TINY["img_size"], TINY["in_timesteps"], TINY["in_channels"]
    gen = torch.Generator(device="cuda").manual_seed(2)
    xx = torch.randn(batch, S, S, T, C, device="cuda", generator=gen)
    yy = torch.randn(batch, S, S, 1, C, device="cuda", generator=gen)
    msk = torch.ones(batch, S, S, 1, C, device="cuda")
    fns = {}
    keep = []
    for name, cls, kw in (("CDPOTNet", CDPOTNet, dict(TINY, out_channels=4)), ("DPOTNet", DPOTNet, TINY)):
        torch.manual_seed(3)
        m = cls(**kw).cuda()
        opt = FusedAdam(FlatParams(m), lr=1e-4, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
        fns[f"{name} eager"] = (lambda m=m, opt=opt: train_step(m, opt, xx, yy, msk, lr=1e-4))
        torch.manual_seed(3)
        m2 = cls(**kw).cuda()
        opt2 = FusedAdam(FlatParams(m2), lr=1e-4, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
        step = GraphedTrainStep(m2, opt2, xx, yy, msk, warmup=2)
        fns[f"{name} graphed"] = (lambda step=step: step.replay(1e-4))
        keep += [m, opt, m2, opt2, step]
    res = compare(fns, iters, rounds)
    lines.append(f"train step, Tiny model line (128 x 128, patch 8, E 512, depth 4), batch {batch}, T_ar 1, fp32")
    for k, (med, lo, hi) in res.items():
        lines.append(f"    {k:18s} {med / 1e3:8.3f} ms   [{lo / 1e3:.3f} .. {hi / 1e3:.3f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cdpot_time.py measures on an MI355X; no GPU found")
    lines = [f"# scripts/cdpot_time.py  iters {a.iters}  rounds {a.rounds}  device {torch.cuda.get_device_name(0)}",
             "# us per call: median [min .. max] over the rounds, device events, candidates alternating inside a round"]
    operator_section(lines, a.iters, a.rounds)
    if not a.skip_model:
        model_section(lines, a.batch, max(a.iters // 5, 5), a.rounds)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
