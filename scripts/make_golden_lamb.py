#!/usr/bin/env python
"""Generate tests/golden/g14_lamb.npz from the REFERENCE's Lamb optimiser (utils/optimizer.py:359-499).  TEST
INFRASTRUCTURE ONLY: the reference is imported at run time from $DPOT_REFERENCE and nothing of it is copied.

    DPOT_REFERENCE=/path/to/DPOT python scripts/make_golden_lamb.py

A DPOT-like tensor set (an AFNO [2, nb, bs, bs] weight, a conv weight of odd size, the 12-element cls_head bias, an
all-zero tensor, a tensor whose norm exceeds clamp_value, and a small tensor next to its x100 copy) runs 4 seeded steps
under three configurations:
  a  adam=True,  debias=False, weight_decay=1e-4, betas=(0.9, 0.9)   what train_temporal.py:132-135 builds
  b  adam=False, debias=True,  weight_decay=1e-4
  c  adam=False, weight_decay=0, clip_grad_norm_ (train_temporal.py:228) before every step
Stored: the initial parameters, the (unclipped) gradients of every step, the parameters after every step, the final
moments, the per-step weight_norm / adam_norm / trust_ratio of every tensor (trust_ratio 1 where the reference keeps
the plain number), and the key layout of the reference's state_dict.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DPOT_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from utils.optimizer import Lamb  # noqa: E402  (reference)

OUT = os.path.join(ROOT, "tests", "golden", "g14_lamb.npz")
STEPS = 4
LR = 1e-2
CONFIGS = {
    "a": dict(betas=(0.9, 0.9), weight_decay=1e-4, adam=True, debias=False, max_norm=None),
    "b": dict(betas=(0.9, 0.999), weight_decay=1e-4, adam=False, debias=True, max_norm=None),
    "c": dict(betas=(0.9, 0.999), weight_decay=0.0, adam=False, debias=False, max_norm=0.5),
}


def tensor_set(gen):
    small = 1e-3 * torch.randn(9, 4, generator=gen)
    return [
        ("afno_w", 0.02 * torch.randn(2, 4, 8, 8, generator=gen)),      # AFNO2D.w1 [2, nb, bs, bs]
        ("conv_w", 0.1 * torch.randn(10, 5, 3, 3, generator=gen)),      # 450 elements: not a multiple of 4
        ("cls_bias", 0.05 * torch.randn(12, generator=gen)),            # cls_head bias
        ("zero", torch.zeros(7, 5)),                                    # ||p|| == 0: trust ratio 1
        ("big", torch.randn(48, 33, generator=gen)),                    # ||p|| ~ 40 > clamp_value 10
        ("small", small.clone()),
        ("small_x100", 100.0 * small),                                  # trust ratios x100 apart
    ]


def main():
    gen = torch.Generator().manual_seed(1414)
    named = tensor_set(gen)
    names = [n for n, _ in named]
    grads = [[torch.randn(p.shape, generator=gen) * (0.01 if n != "big" else 1.0) for n, p in named]
             for _ in range(STEPS)]
    out = {"names": np.array(names), "lr": np.float64(LR), "steps": np.int64(STEPS), "clamp_value": np.float64(10.0),
           "eps": np.float64(1e-6)}
    for n, p in named:
        out[f"p0.{n}"] = p.numpy()
    for k in range(STEPS):
        for (n, _), g in zip(named, grads[k]):
            out[f"g{k}.{n}"] = g.numpy()
    for cname, cfg in CONFIGS.items():
        params = [torch.nn.Parameter(p.clone()) for _, p in named]
        opt = Lamb(params, lr=LR, betas=cfg["betas"], weight_decay=cfg["weight_decay"], adam=cfg["adam"],
                   debias=cfg["debias"])
        out[f"{cname}.betas"] = np.array(cfg["betas"], dtype=np.float64)
        out[f"{cname}.weight_decay"] = np.float64(cfg["weight_decay"])
        out[f"{cname}.adam"] = np.int64(cfg["adam"])
        out[f"{cname}.debias"] = np.int64(cfg["debias"])
        out[f"{cname}.max_norm"] = np.float64(cfg["max_norm"] if cfg["max_norm"] is not None else 0.0)
        for k in range(STEPS):
            for p, g in zip(params, grads[k]):
                p.grad = g.clone()
            if cfg["max_norm"] is not None:
                tn = torch.nn.utils.clip_grad_norm_(params, cfg["max_norm"])
                out[f"{cname}.total_norm{k}"] = np.float64(tn.item())
            opt.step()
            for n, p in zip(names, params):
                st = opt.state[p]
                out[f"{cname}.p{k + 1}.{n}"] = p.detach().numpy().copy()
                out[f"{cname}.weight_norm{k + 1}.{n}"] = np.float32(float(st["weight_norm"]))
                out[f"{cname}.adam_norm{k + 1}.{n}"] = np.float32(float(st["adam_norm"]))
                out[f"{cname}.trust_ratio{k + 1}.{n}"] = np.float32(float(st["trust_ratio"]))
                out[f"{cname}.trust_is_number{k + 1}.{n}"] = np.int64(not torch.is_tensor(st["trust_ratio"]))
        for n, p in zip(names, params):
            st = opt.state[p]
            out[f"{cname}.exp_avg.{n}"] = st["exp_avg"].numpy().copy()
            out[f"{cname}.exp_avg_sq.{n}"] = st["exp_avg_sq"].numpy().copy()
        sd = opt.state_dict()
        out[f"{cname}.state_keys"] = np.array(sorted(sd["state"][0].keys()))
        out[f"{cname}.group_keys"] = np.array(sorted(sd["param_groups"][0].keys()))
        out[f"{cname}.state_step"] = np.int64(sd["state"][0]["step"])
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.0f} KiB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
