"""What scripts/make_golden_finetune3d.py and the 3-D fine-tuning tests share: the cases of tests/golden/g18_finetune3d.npz,
their closed-form inputs, and a float64 restatement of the reference's training loop finetune3d.py:206-222 around
afno3d_ref.model3d_ref (no reference needed).  TEST INFRASTRUCTURE ONLY."""
import math
from collections import OrderedDict

import torch

import afno3d_ref as A3
from oracle import dpot_ref as R

B = 2
NOISE_SCALE = 0.01
OPT = dict(lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=1.0)        # max_norm below the gradient norm: the clip acts
# tag: model config, AR frames, frames per call, salt of the recipes
CASES = OrderedDict([
    ("ft", dict(cfg=A3.MINI3D, T_ar=3, T_bundle=1, salt=184)),
    ("ftb", dict(cfg=dict(A3.MINI3D, out_timesteps=2), T_ar=4, T_bundle=2, salt=188)),      # the window slides by two
])
SUB_STRIDE = 3              # strided subsample of the noisy inputs, of gradients above SUB_MIN elements and of the parameters
SUB_MIN = 1024


def noise3d(xx, scale, eps):
    """finetune3d.py:210 - one norm per (b, t, c), over X*Y*Z"""
    return xx + scale * torch.sum(xx ** 2, dim=(1, 2, 3), keepdim=True) ** 0.5 * eps


def noise2d_rule(xx, scale, eps):
    """train_temporal.py:205 applied to the same 6-D tensor as a [B, X, Y*Z, T, C] window: one norm per (b, c), over the space
    AND the time axis - what a rank-blind kernel call computes"""
    return xx + scale * torch.sum(xx ** 2, dim=(1, 2, 3, 4), keepdim=True) ** 0.5 * eps


def inputs(tag):
    """(xx, yy, msk, [eps_k]) of a case, float32"""
    c = CASES[tag]
    cfg, salt = c["cfg"], c["salt"]
    S, T, C = cfg["img_size"], cfg["in_timesteps"], cfg["in_channels"]
    xx = R.recipe_input((B, S, S, S, T, C), salt)
    yy = R.recipe_input((B, S, S, S, c["T_ar"], C), salt + 1)
    msk = A3.recipe_mask((B, S, S, S, 1, C), salt)
    n_steps = len(range(0, c["T_ar"], c["T_bundle"]))
    # unit-variance, zero-mean stand-ins for torch.randn_like (closed form)
    eps = [((R.recipe_tensor("eps", tuple(xx.shape), salt + 10 + k) - 0.5) * math.sqrt(12.0)).to(torch.float32)
           for k in range(n_steps)]
    return xx, yy, msk, eps


def shapes_of(model):
    return OrderedDict((k, tuple(v.shape)) for k, v in model.state_dict().items())


def recipe_weights(tag, model):
    """state dict of the case for `model` (any DPOTNet3D with the reference's layout) before the 2-D components are loaded,
    and the 2-D state dict whose blocks and time aggregator are then loaded over it"""
    c = CASES[tag]
    return (A3.recipe_sd(shapes_of(model), c["cfg"]["n_blocks"], c["salt"]),
            R.recipe_state_dict(R.DPOTConfig(**A3.MINI2D), c["salt"] + 1))


def loop_ref(sd, tag, noise=noise3d):
    """the loop in float64 through A3.model3d_ref: (loss, l2_full, [noisy input of every AR step])"""
    c = CASES[tag]
    xx, yy, msk, eps = (t.double() if torch.is_tensor(t) else [e.double() for e in t] for t in inputs(tag))
    loss, preds, noisy = 0., [], []
    for k, t in enumerate(range(0, c["T_ar"], c["T_bundle"])):
        xx = noise(xx, NOISE_SCALE, eps[k])
        noisy.append(xx)
        im = A3.model3d_ref(sd, xx, c["cfg"])
        loss = loss + R.rel_l2_loss(im, yy[..., t:t + c["T_bundle"], :], msk)
        preds.append(im)
        xx = torch.cat((xx[..., c["T_bundle"]:, :], im), dim=-2)
    return loss, R.rel_l2_loss(torch.cat(preds, dim=-2), yy, msk), noisy
