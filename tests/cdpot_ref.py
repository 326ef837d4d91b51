"""Restatement of the reference's CDPOT model (models/dpot_res.py:393-586) and of its anti-aliased activation
(models/filter_networks.py:481-518, LReLu_torch), written from torch ops, oracle/dpot_ref.py and ops.aa_resize_matrix - no
reference code.  Runs in whatever dtype its inputs have (the tests use float64); tests/test_cpu_cdpot.py holds it to the
reference's recorded float64 results (tests/golden/g21_cdpot.npz), the GPU tests use it for shapes the fixture does not hold.
Also the cases, mini configurations and closed-form weights the fixture script and the tests share.
"""
from __future__ import annotations

from collections import OrderedDict

import math

import numpy as np
import torch

from oracle import dpot_ref as R

SLOPE = 0.01
KINK = 1e-5          # no up-sampled value of a backward test input may lie in (0, KINK): fp32 and float64 could disagree on its sign

# operator cases recorded from the reference's own class (square, Cb == C: all it can run): name -> (N, h, C, out size | None)
OP_CASES = OrderedDict([
    ("n1_h1_c1", (1, 1, 1, None)),
    ("n3_h2_c3_x2", (3, 2, 3, 4)),
    ("n1_h5_c35", (1, 5, 35, None)),
    ("n1_h4_c3_x5", (1, 4, 3, 20)),
    ("n1_h7_c1_30", (1, 7, 1, 30)),
    ("n1_h4_c3_x8", (1, 4, 3, 32)),
    ("n1_h16_c5", (1, 16, 5, None)),
    ("n2_h32_c1", (2, 32, 1, None)),
    ("n1_h4_c36_x2", (1, 4, 36, 8)),
])
OP_SALT = 400        # case i: x = recipe_input(salt OP_SALT + i), upstream gradient salt OP_SALT + 50 + i, bias 'aa_bias'

MINI1 = dict(img_size=20, patch_size=5, in_channels=3, out_channels=3, in_timesteps=6, out_timesteps=1, n_blocks=4,
             embed_dim=32, out_layer_dim=16, depth=2, modes=2, mlp_ratio=1.0, n_cls=3, normalize=False, act="gelu",
             time_agg="exp_mlp")
MINI2 = dict(MINI1, normalize=True, time_agg="mlp", out_timesteps=2)
MINI3 = dict(MINI1, img_size=32, patch_size=4, modes=4)
# (salts stepped by 3 from 410 / 420 / 430 / 440 until the kink condition holds for both activation inputs, in every AR step)
MODELS = OrderedDict([("m1", (MINI1, 413)), ("m2", (MINI2, 420)), ("m3", (MINI3, 433))])
MODEL_B = 2
DX_STRIDE = 5        # the fixture keeps every fifth element of a mini model's input gradient
STEP_STRIDE = 3      # ... and every third of the step's flat gradient and parameters
STEP = dict(T_ar=2, lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=5.0, salt=443)


def op_inputs(name):
    """(x [N, h, h, C], upstream gradient [N, H, H, C], bias [C]) of a recorded operator case, fp32"""
    i = list(OP_CASES).index(name)
    N, h, C, out = OP_CASES[name]
    H = out or h
    x = R.recipe_input((N, h, h, C), OP_SALT + i)
    g = R.recipe_input((N, H, H, C), OP_SALT + 50 + i)
    bias = ((R.recipe_tensor("aa_bias", (C,), OP_SALT + i) - 0.5) * 0.4).float()
    return x, g, bias


def hash_input(shape, salt):
    """inputs of the tests outside the fixture (the same closed form)"""
    return R.recipe_input(tuple(shape), salt)


# ---- the operator ---------------------------------------------------------------------------------------------------------
def _mat(n, m, like):
    from dpot_amd import ops
    return torch.from_numpy(ops.aa_resize_matrix(n, m)).to(like.dtype)


def aa_upsampled(x):
    """U_h x U_w^T of a channels-last x [N, h, w, C]: the 2h x 2w field the LeakyReLU sees"""
    h, w = x.shape[1:3]
    return torch.einsum("ap,npqc,bq->nabc", _mat(h, 2 * h, x), x, _mat(w, 2 * w, x))


def aa_lrelu_ref(x, bias, out_size=None, slope=SLOPE):
    """y = V D lrelu(U x U^T) D^T V^T + bias[c % Cb] for a channels-last x [N, h, w, C]"""
    N, h, w, C = x.shape
    u = aa_upsampled(x)
    u = torch.where(u > 0, u, slope * u)
    z = torch.einsum("ia,nabc,jb->nijc", _mat(2 * h, h, x), u, _mat(2 * w, w, x))
    if out_size is not None:
        H, W = (out_size, out_size) if isinstance(out_size, int) else out_size
        if (H, W) != (h, w):
            z = torch.einsum("Ii,nijc,Jj->nIJc", _mat(h, H, x), z, _mat(w, W, x))
    return z + bias.repeat(C // bias.shape[0])


def kink_margin(x):
    """the smallest non-zero |value| of the float64 up-sampled field (inf if there is none)"""
    u = aa_upsampled(x.double()).abs()
    u = u[u > 0]
    return float(u.min()) if u.numel() else math.inf


# ---- weights --------------------------------------------------------------------------------------------------------------
def recipe_sd(shapes, cfg, salt):
    """closed-form weights keyed by parameter name (oracle.dpot_ref.recipe_tensor), with the magnitudes of
    oracle.dpot_ref.recipe_state_dict; `shapes`: the state_dict name -> shape list of the model (either implementation)"""
    sd = OrderedDict()
    E, bs = cfg["embed_dim"], cfg["embed_dim"] // cfg["n_blocks"]
    for name, shape in shapes.items():
        shape = tuple(shape)
        u = R.recipe_tensor(name, shape, salt)
        if name == "pos_embed":
            v = (u - 0.5) * 0.08
        elif ".filter." in name:
            v = (u - 0.5) * (2.0 / math.sqrt(bs))
        elif name.endswith("norm1.weight") or name.endswith("norm2.weight"):
            v = 0.75 + 0.5 * u
        elif name.endswith("norm1.bias") or name.endswith("norm2.bias"):
            v = (u - 0.5) * 0.2
        elif name == "time_agg_layer.gamma":
            v = (2.0 ** torch.linspace(-10, 10, E, dtype=torch.float64)).unsqueeze(0) * (0.9 + 0.2 * u)
        elif name == "time_agg_layer.w":
            v = (u - 0.5) * 2.0 * math.sqrt(3.0) / (cfg["in_timesteps"] * math.sqrt(E)) * 3.0
        elif name.endswith(".bias"):
            v = (u - 0.5) * 0.1
        else:
            v = (u - 0.5) * 2.0 * math.sqrt(3.0 / int(np.prod(shape[1:])))
        sd[name] = v.to(torch.float32).contiguous()
    # one module registered twice: both names hold ONE tensor
    sd["patch_embed.proj.1.bias"] = sd["patch_embed.act_patching.bias"]
    return sd


def model_inputs(tag):
    """(x, y, mask, cls cotangent) of a recorded mini model, fp32"""
    cfg, salt = MODELS[tag]
    S, B = cfg["img_size"], MODEL_B
    x = R.recipe_input((B, S, S, cfg["in_timesteps"], cfg["in_channels"]), salt)
    y = R.recipe_input((B, S, S, cfg["out_timesteps"], cfg["out_channels"]), salt + 1)
    msk = (R.recipe_tensor("mask", tuple(y.shape), salt) > 0.25).to(torch.float32)
    gc = R.recipe_input((B, cfg["n_cls"]), salt + 2)
    return x, y, msk, gc


def _cfg(cfg):
    return R.DPOTConfig(**{k: v for k, v in cfg.items()})


# ---- the model ------------------------------------------------------------------------------------------------------------
def cdpot_forward(sd, x, cfg, probe=None):
    """x [B, X, Y, T, C] -> (pred [B, X, Y, T_out, C_out], cls_pred [B, n_cls]); sd: name -> tensor of x's dtype.
    probe: a list that receives the two fields the anti-aliased activation is applied to (for the kink condition)"""
    c = _cfg(cfg)
    act = R._act(c.act)
    B, S, _, T, _ = x.shape
    P, E, old = c.patch_size, c.embed_dim, c.out_layer_dim
    if c.normalize:
        mu = x.mean(dim=(1, 2, 3), keepdim=True)
        sigma = x.std(dim=(1, 2, 3), keepdim=True) + 1e-6
        x = (x - mu) / sigma
        stat = torch.cat([mu, sigma], dim=-1)[:, 0, 0, 0, :]
        s_mu = stat @ sd["scale_feats_mu.weight"].t() + sd["scale_feats_mu.bias"]
        s_sg = stat @ sd["scale_feats_sigma.weight"].t() + sd["scale_feats_sigma.bias"]
    # patch embedding: conv (no activation), the operator at the latent size, 1x1 conv, + pos_embed
    a = R.patchify(R.append_grid(x), P)                                         # [B, h, w, T, K]
    w0 = sd["patch_embed.proj.0.weight"]
    hid = w0.shape[0]
    hpre = a @ w0.reshape(hid, -1).t() + sd["patch_embed.proj.0.bias"]          # [B, h, w, T, hid]
    h = hpre.shape[1]
    if probe is not None:
        probe.append(hpre.reshape(B, h, h, T * hid).detach())
    hact = aa_lrelu_ref(hpre.reshape(B, h, h, T * hid), sd["patch_embed.act_patching.bias"]).reshape(B, h, h, T, hid)
    z = hact @ sd["patch_embed.proj.2.weight"].reshape(E, hid).t() + sd["patch_embed.proj.2.bias"]
    z = z + sd["pos_embed"][0].permute(1, 2, 0)[None, :, :, None, :]
    v = time_aggregate(sd, z, c)
    if c.normalize:
        v = s_sg[:, None, None, :] * v + s_mu[:, None, None, :]
    for i in range(c.depth):
        v = R.block_forward(sd, i, v, c)
    cls_pred = R.cls_head(sd, v, c)
    # output layer: (the frequency filter with K = 1 keeps everything) 1x1 conv at the latent size, the operator up to the image
    u = v @ sd["out_layer.0.convolution.weight"].reshape(old, E).t() + sd["out_layer.0.convolution.bias"]
    if probe is not None:
        probe.append(u.detach())
    u = aa_lrelu_ref(u, sd["out_layer.0.activation.bias"], (S, S))
    u = act(u @ sd["out_layer.1.weight"].reshape(old, old).t() + sd["out_layer.1.bias"])
    co = c.out_channels * c.out_timesteps
    u = u @ sd["out_layer.3.weight"].reshape(co, old).t() + sd["out_layer.3.bias"]
    y = u.reshape(B, S, S, c.out_timesteps, c.out_channels)
    if c.normalize:
        y = y * sigma + mu
    return y, cls_pred


def time_aggregate(sd, z, c):
    """[B, h, w, T, E] -> [B, h, w, E] (models/dpot_res.py:360-385).  The time axis is torch.linspace in the run's own dtype, as
    the reference builds it - a float64 run of the reference has a float64 axis (oracle.dpot_ref.time_aggregate keeps the
    float32 axis there)"""
    w = sd["time_agg_layer.w"]
    if c.time_agg == "mlp":
        return torch.einsum("tij,...ti->...j", w, z)
    t = torch.linspace(0, 1, z.shape[-2], dtype=z.dtype).unsqueeze(-1)
    return torch.einsum("tij,...ti->...j", w, z * torch.cos(t @ sd["time_agg_layer.gamma"]))


def model_loss(pred, cls_pred, y, msk, gc):
    """what the fixture differentiates: the reference's SimpleLpLoss(size_average=False) + <cls_pred, gc> (so that cls_head
    receives a gradient too)"""
    return R.rel_l2_loss(pred, y, msk) + (cls_pred * gc).sum()


def ref_shapes(fx, tag):
    """state_dict name -> shape of a recorded layout (`sd`, `m1`, ...)"""
    return OrderedDict((str(n), tuple(int(v) for v in s if v))                     # rows are zero-padded to 4 entries
                       for n, s in zip(fx[f"{tag}.names"], fx[f"{tag}.shapes"]))


def step_inputs():
    """(xx, yy, mask) of the recorded two-AR-step training step"""
    cfg, st = MINI1, STEP
    S, B = cfg["img_size"], MODEL_B
    xx = R.recipe_input((B, S, S, cfg["in_timesteps"], cfg["in_channels"]), st["salt"])
    yy = R.recipe_input((B, S, S, st["T_ar"], cfg["out_channels"]), st["salt"] + 1)
    msk = (R.recipe_tensor("mask", (B, S, S, 1, cfg["out_channels"]), st["salt"]) > 0.25).to(torch.float32)
    return xx, yy, msk


def step_probe():
    """the fields the anti-aliased activation sees in the two AR steps of the recorded training step (float64 restatement)"""
    from dpot_amd import CDPOTNet
    cfg, st = MINI1, STEP
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in CDPOTNet(**cfg).state_dict().items())
    sd = {k: v.double() for k, v in recipe_sd(shapes, cfg, st["salt"]).items()}
    xx = step_inputs()[0].double()
    probe = []
    with torch.no_grad():
        for _ in range(st["T_ar"]):
            im, _c = cdpot_forward(sd, xx, cfg, probe)
            xx = torch.cat((xx[..., 1:, :], im), dim=-2)
    return probe


# ---- the operator cases of the GPU tests (tests/test_gpu_cdpot.py; the CPU tests hold their inputs to the kink condition) -----
# salts replaced because the closed-form input of 500 + k has an up-sampled value inside (0, KINK) (the larger the field, the
# likelier); found by stepping the salt by 100 until the condition holds
_SALT_FIX = {26: 626, 34: 634, 38: 638, 44: 644, 45: 745, 47: 647, 48: 748, 49: 1749, 54: 954, 55: 955, 57: 957, 58: 658, 59: 759}


def _gpu_op_cases():
    sizes = [(1, 1), (2, 2), (5, 7), (8, 8), (16, 16), (32, 32)]
    chans = [(1, 1), (3, 1), (35, 7), (36, 12), (40, 4)]          # (C, the Cb < C that divides it: C / T)
    mults = [None, 2, 4, 5, 8]
    cases, k = [], 0
    for si, (h, w) in enumerate(sizes):
        for ci, (C, Cd) in enumerate(chans):
            for r in range(2):
                mult = mults[(si + 2 * ci + 3 * r) % 5]
                N = (1, 3)[(si + ci + r) % 2]
                Cb = Cd if (k % 2) else C
                out = None if mult is None else (h * mult, w * mult)
                if out is not None and N * out[0] * out[1] * C > (1 << 21):
                    N = 1
                cases.append((N, h, w, C, Cb, out, _SALT_FIX.get(k, 500 + k)))
                k += 1
    cases += [(3, 7, 7, 35, 35, (30, 30), 500 + k), (1, 7, 7, 36, 12, (30, 30), 501 + k), (2, 5, 7, 3, 1, (30, 30), 502 + k)]
    return cases


GPU_OP_CASES = _gpu_op_cases()          # (N, h, w, C, Cb, out size | None, salt): x salt, upstream gradient salt + 1000


def gpu_op_inputs(case):
    N, h, w, C, Cb, out, salt = case
    H, W = out or (h, w)
    x = R.recipe_input((N, h, w, C), salt)
    g = R.recipe_input((N, H, W, C), salt + 1000)
    bias = ((R.recipe_tensor("aa_bias", (Cb,), salt) - 0.5) * 0.4).float()
    return x, g, bias


def run_op_ref(x, g, bias, out, dtype=torch.float64):
    """(y, dx, dbias) of the restatement in `dtype`"""
    xi = x.detach().clone().to(dtype).requires_grad_(True)
    bi = bias.detach().clone().to(dtype).requires_grad_(True)
    y = aa_lrelu_ref(xi, bi, out)
    (y * g.to(dtype)).sum().backward()
    return y.detach(), xi.grad, bi.grad


def run_model_ref(tag, dtype=torch.float64, probe=None):
    """restatement of a recorded mini model in `dtype`: (pred, cls_pred, {name: gradient}, input gradient)"""
    cfg, salt = MODELS[tag]
    x, y, msk, gc = model_inputs(tag)
    from dpot_amd import CDPOTNet
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in CDPOTNet(**cfg).state_dict().items())
    sd = {k: v.to(dtype).requires_grad_(True) for k, v in recipe_sd(shapes, cfg, salt).items() if k != "patch_embed.proj.1.bias"}
    xi = x.detach().clone().to(dtype).requires_grad_(True)
    pred, cls_pred = cdpot_forward(sd, xi, cfg, probe)
    model_loss(pred, cls_pred, y.to(dtype), msk.to(dtype), gc.to(dtype)).backward()
    return pred.detach(), cls_pred.detach(), {k: v.grad for k, v in sd.items()}, xi.grad
