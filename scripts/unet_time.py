#!/usr/bin/env python
"""Timings of the UNet baseline on one MI355X (written to profiles/unet.txt by `--out`):

  kernels    ops.conv3x3 / conv3x3_bwd_data / conv3x3_wgrad / bn_act (with pooling) / bn_act_bwd at two layers of the reference's
             width-32 model at batch 20, 128 x 128, 42 input channels - a level-1 layer (32 -> 32 channels on the 128 x 128 field)
             and a bottleneck layer (512 -> 512 on 8 x 8) - beside two yardsticks taken in the same run, candidates alternating
             inside every round:
               torch     the same operator from torch ops on the device, on channels-first fields as the reference holds them
                         (conv2d and its two gradient functions; batch_norm + gelu + max_pool2d and their autograd backward) -
                         not the code under test, not tuned
               copy      a plain device copy of the bytes the operator must read and write
             and, for the three convolution kernels, the share of the fp32 matrix-core roof (157.3 TFLOP/s) from 2 * 9 * B H W
             Cin Cout operations
  model      one training step (forward, loss, backward, clip, fused Adam) of that UNet, eager and as one captured graph, and
             the time of the torch glue of one forward and backward (input assembly, the four concatenations and their splits)

    python scripts/unet_time.py --out profiles/unet.txt

Times are device events around a window of back-to-back calls (as many as fill `--window` seconds, 0.25 by default) after a
warm-up, the median of `rounds` rounds; no profiler."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 157.3e12
LAYERS = [("level 1     B20 128x128  32 ->  32", 20, 128, 128, 32, 32), ("bottleneck  B20   8x8   512 -> 512", 20, 8, 8, 512, 512)]
GELU = 1


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def compare(fns, window, rounds):
    """{name: (median us, min, max)} with the candidates alternating inside every round"""
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
    src = torch.empty(int(n_floats), device="cuda")
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


def emit(lines, title, res, extra=""):
    lines.append(f"  {title}{extra}")
    for k, (med, lo, hi) in res.items():
        lines.append(f"    {k:30s} {med:9.1f} us   [{lo:.1f} .. {hi:.1f}]")
    ks = list(res)
    lines.append(f"    -> kernel / torch {res[ks[0]][0] / res[ks[1]][0]:.2f}, kernel / copy {res[ks[0]][0] / res[ks[2]][0]:.2f} "
                 f"({'faster' if res[ks[0]][0] < res[ks[1]][0] else 'SLOWER'} than torch)")


def kernel_section(lines, window, rounds):
    from dpot_amd import ops
    for name, B, H, W, Ci, Co in LAYERS:
        gen = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, H, W, Ci, device="cuda", generator=gen)
        w = torch.randn(Co, Ci, 3, 3, device="cuda", generator=gen) / (3 * Ci ** 0.5)
        dz = torch.randn(B, H, W, Co, device="cuda", generator=gen)
        gamma, beta = torch.rand(Co, device="cuda", generator=gen) + 0.5, torch.randn(Co, device="cuda", generator=gen)
        n_x, n_z, n_w = x.numel(), dz.numel(), w.numel()
        flop = 2.0 * 9 * B * H * W * Ci * Co
        lines.append(f"layer {name}: x {4 * n_x / 1e6:.1f} MB, z {4 * n_z / 1e6:.1f} MB, weight {4 * n_w / 1e6:.2f} MB, "
                     f"{flop / 1e9:.1f} GFLOP per convolution")
        xc, dzc = x.permute(0, 3, 1, 2).contiguous(), dz.permute(0, 3, 1, 2).contiguous()
        z, part = ops.conv3x3(x, w, stats=True)
        mean, invstd = ops.bn_stats(part, B * H * W, Co)
        ref = F.conv2d(xc, w, padding=1).permute(0, 2, 3, 1)
        lines.append(f"  (kernel conv3x3 vs torch conv2d: max|d| / max|ref| = {((z - ref).abs().max() / ref.abs().max()).item():.1e})")
        out_z, out_x, out_w = torch.empty_like(z), torch.empty_like(x), torch.empty_like(w)

        def share(r):
            return f"   {100 * flop / (r[next(iter(r))][0] * 1e-6) / ROOF:.1f} % of the fp32 matrix-core roof"

        r = compare({"kernel conv3x3 (+ statistics)": lambda: ops.conv3x3(x, w, stats=True, out=out_z),
                     "torch conv2d": lambda: F.conv2d(xc, w, padding=1), "copy x + z": copy_of(n_x + n_z)}, window, rounds)
        emit(lines, "forward", r, share(r))
        r = compare({"kernel conv3x3_bwd_data": lambda: ops.conv3x3_bwd_data(dz, w, out=out_x),
                     "torch conv2d_input": lambda: torch.nn.grad.conv2d_input(xc.shape, w, dzc, padding=1),
                     "copy dz + dx": copy_of(n_x + n_z)}, window, rounds)
        emit(lines, "data gradient", r, share(r))
        r = compare({"kernel conv3x3_wgrad": lambda: ops.conv3x3_wgrad(x, dz, out=out_w),
                     "torch conv2d_weight": lambda: torch.nn.grad.conv2d_weight(xc, w.shape, dzc, padding=1),
                     "copy x + dz": copy_of(n_x + n_z)}, window, rounds)
        emit(lines, "weight gradient", r, share(r))
        # ---- normalise + activation + pooling ----
        zc = z.permute(0, 3, 1, 2).contiguous()
        y_out, p_out = torch.empty_like(z), torch.empty(B, H // 2, W // 2, Co, device="cuda")

        def t_bn(zz=zc):
            y = F.gelu(F.batch_norm(zz, None, None, gamma, beta, training=True, momentum=0.1, eps=1e-5))
            return y, F.max_pool2d(y, 2, 2)

        zg = zc.clone().requires_grad_(True)
        gy, gp = torch.randn_like(zc), torch.randn(B, Co, H // 2, W // 2, device="cuda")
        dy, dp = gy.permute(0, 2, 3, 1).contiguous(), gp.permute(0, 2, 3, 1).contiguous()

        def t_bn_fb():
            zg.grad = None
            y, p = t_bn(zg)
            torch.autograd.backward([y, p], [gy, gp])

        r = compare({"kernel bn_act + pool": lambda: ops.bn_act(z, mean, invstd, gamma, beta, GELU, True, out=y_out, out_pool=p_out),
                     "torch batch_norm, gelu, max_pool2d": t_bn, "copy z + y + pooled": copy_of(2.25 * n_z)}, window, rounds)
        emit(lines, "normalise + gelu + 2x2 pooling (torch also computes the statistics)", r)
        t_fwd = r["torch batch_norm, gelu, max_pool2d"][0]
        r = compare({"kernel bn_act_bwd (2 launches)": lambda: ops.bn_act_bwd(dy, dp, z, mean, invstd, gamma, beta, GELU, out=y_out),
                     "torch forward + backward": t_bn_fb, "copy dy + dpool + 2 z + dz": copy_of(4.25 * n_z)}, window, rounds)
        emit(lines, "its backward (z is read twice: the sums, then dz)", r)
        lines.append(f"    torch backward only {r['torch forward + backward'][0] - t_fwd:.1f} us")
        del x, dz, z, xc, dzc, zc, zg, gy, gp, dy, dp
        torch.cuda.empty_cache()


def model_section(lines, window, rounds):
    from dpot_amd import UNet
    from dpot_amd.train import FlatParams, FusedAdam, GraphedTrainStep, train_step
    B, S, T, C, width = 20, 128, 10, 4, 32
    gen = torch.Generator(device="cuda").manual_seed(2)
    xx = torch.randn(B, S, S, T, C, device="cuda", generator=gen)
    yy = torch.randn(B, S, S, 1, C, device="cuda", generator=gen)

    def make():
        torch.manual_seed(3)
        m = UNet(2, in_channels=C, out_channels=C, in_timesteps=T, in_shape=(S, S), width=width).cuda().train()
        return m, FusedAdam(FlatParams(m), lr=1e-4, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)

    m, opt = make()
    m2, opt2 = make()
    step = GraphedTrainStep(m2, opt2, xx, yy, None, warmup=2)
    f = width
    parts = [(torch.randn(B, S >> k, S >> k, f << k, device="cuda"), torch.randn(B, S >> k, S >> k, f << k, device="cuda"))
             for k in range(4)]
    gx = torch.linspace(0, 1, S, device="cuda")

    def glue():
        x = xx.reshape(B, S, S, T * C)
        torch.cat([gx.view(1, S, 1, 1).expand(B, S, S, 1), gx.view(1, 1, S, 1).expand(B, S, S, 1), x], dim=-1).contiguous()
        for a, b in parts:
            d = torch.cat([a, b], dim=-1)
            d[..., :a.shape[-1]].contiguous(), d[..., a.shape[-1]:].contiguous()          # the backward's split of the gradient

    res = compare({"UNet eager": lambda: train_step(m, opt, xx, yy, None, lr=1e-4), "UNet graphed": lambda: step.replay(1e-4),
                   "torch glue of one step": glue}, window, rounds)
    lines.append(f"train step, the reference's UNet (128 x 128, width 32, T 10, C 4: 42 input channels), batch {B}, T_ar 1, fp32")
    for k, (med, lo, hi) in res.items():
        lines.append(f"    {k:26s} {med / 1e3:8.3f} ms   [{lo / 1e3:.3f} .. {hi / 1e3:.3f}]")
    lines.append(f"    -> the glue (input assembly, the four concatenations, the four splits of their gradients) is "
                 f"{100 * res['torch glue of one step'][0] / res['UNet graphed'][0]:.1f} % of the graphed step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unet_time.py measures on an MI355X; no GPU found")
    lines = [f"# scripts/unet_time.py  window {a.window} s  rounds {a.rounds}  device {torch.cuda.get_device_name(0)}",
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
