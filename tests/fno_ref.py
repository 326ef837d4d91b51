"""Restatement of the reference's FNO baseline (models/fno.py: SpectralConv2d_fast, FNO2d), written from the mathematics with
torch ops and oracle/dpot_ref.py - no reference code.  The spectral layer is the dense sums over the kept modes with a complex
spectrum of the run's own precision (complex128 for float64 inputs: the reference allocates its output spectrum as complex64
whatever the input, so its own float64 run is only good to 5e-8 and cannot be the yardstick).  Channels-last throughout.
tests/test_cpu_fno.py holds it to the reference's records (tests/golden/g22_fno.npz); the GPU tests use it as the float64
yardstick.  Also the cases, mini configurations and closed-form weights the fixture script and the tests share.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dpot_ref as R

# ---- cases ----------------------------------------------------------------------------------------------------------------
# the spectral layer, recorded from the reference's own class: name -> (B, H, W, Cin, Cout, m1, m2)
LAYER_CASES = OrderedDict([
    ("h6_m3x4", (2, 6, 6, 3, 3, 3, 4)),                 # 2 m1 = H, the Nyquist column kept
    ("h7x9_c3to5", (2, 7, 9, 3, 5, 3, 4)),              # odd, non-square, Cin != Cout
    ("h16_c8", (1, 16, 16, 8, 8, 4, 5)),
    ("h12x10_c4to2", (3, 12, 10, 4, 2, 2, 6)),          # W even with its Nyquist column kept, Cin != Cout
])
LAYER_SALT = 600      # case i: x salt LAYER_SALT + i, upstream gradient + 50, weights by name with that salt

# the transforms on the GPU: (B, H, W, C, m1, m2).  Cases 5-8 and 10 cross the kernels' tile boundaries, case 9 is the declared
# maximum (tests/test_gpu_fno.py names them)
TRANSFORM_CASES = [
    (2, 7, 9, 3, 3, 4), (1, 8, 8, 4, 4, 5), (1, 6, 7, 4, 1, 4), (1, 5, 5, 1, 1, 1), (1, 40, 24, 36, 12, 12),
    (1, 72, 20, 20, 5, 9), (1, 18, 34, 18, 2, 6), (1, 17, 16, 4, 8, 4), (2, 16, 17, 16, 1, 8),
    (1, 256, 256, 4, 64, 64), (1, 130, 12, 4, 40, 3),
]
# (B, Cin, Cout, m1, m2); the last one has more than 16 channels on both sides: a second output-tile row in both roles
MIX_CASES = [(1, 1, 1, 1, 1), (3, 5, 7, 2, 3), (2, 8, 8, 5, 7), (33, 4, 4, 2, 2), (5, 20, 36, 2, 3)]
OP_SALT = 700

MINI1 = dict(modes1=5, modes2=6, width=12, img_size=10, n_channels=2, in_timesteps=3, out_timesteps=1, n_layers=2,
             patch_size=1, use_ln=False, normalize=False, n_cls=3)
MINI2 = dict(modes1=3, modes2=4, width=8, img_size=7, n_channels=2, in_timesteps=3, out_timesteps=1, n_layers=2,
             patch_size=1, use_ln=4, normalize=True, n_cls=5)
MINI3 = dict(modes1=2, modes2=3, width=8, img_size=12, n_channels=2, in_timesteps=3, out_timesteps=1, n_layers=2,
             patch_size=3, use_ln=False, normalize=False, n_cls=2)
MODELS = OrderedDict([("m1", (MINI1, 810)), ("m2", (MINI2, 820)), ("m3", (MINI3, 830))])
MODEL_B = 2
DX_STRIDE = 3
STEP_STRIDE = 3
STEP = dict(T_ar=2, lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=5.0, salt=840)


def hash_input(shape, salt):
    return R.recipe_input(tuple(shape), salt)


def _cdtype(dtype):
    return torch.complex128 if dtype == torch.float64 else torch.complex64


# ---- the transforms -------------------------------------------------------------------------------------------------------
def kept_rows(H, m1):
    return np.concatenate([np.arange(m1), np.arange(H - m1, H)])


def col_weights(W, m2, dtype=torch.float64):
    """irfft2 on a spectrum that is not Hermitian: weight 1 at ky = 0 and, for even W, at ky = W / 2, else 2"""
    w = torch.full((m2,), 2.0, dtype=dtype)
    w[0] = 1.0
    if W % 2 == 0 and W // 2 < m2:
        w[W // 2] = 1.0
    return w


def dft_matrices(H, W, m1, m2, dtype=torch.float64):
    """(Fx [2 m1, H], Fy [W, m2]) complex: e^{-2 pi i kx x / H} over the kept rows, e^{-2 pi i ky y / W}; float64 angles
    reduced in integers"""
    kx = kept_rows(H, m1)
    ax = 2.0 * np.pi * ((kx[:, None] * np.arange(H)[None, :]) % H) / H
    ay = 2.0 * np.pi * ((np.arange(W)[:, None] * np.arange(m2)[None, :]) % W) / W
    return (torch.from_numpy(np.exp(-1j * ax)).to(_cdtype(dtype)), torch.from_numpy(np.exp(-1j * ay)).to(_cdtype(dtype)))


def rfft2_kept(x, m1, m2):
    """x [B, H, W, C] real -> complex [B, 2 m1, m2, C]: the kept modes of the unnormalised rfft2"""
    Fx, Fy = (f.to(x.device) for f in dft_matrices(x.shape[1], x.shape[2], m1, m2, x.dtype))
    return torch.einsum("rx,bxyc,yk->brkc", Fx, x.to(Fx.dtype), Fy)


def irfft2_kept(S, H, W, weights=True, scale=None):
    """complex [B, 2 m1, m2, C] -> real [B, H, W, C]: irfft2 of the spectrum that is zero off the kept modes (weights=True,
    scale 1 / (H W)); weights=False, scale=1: the adjoint of rfft2_kept"""
    m1, m2 = S.shape[1] // 2, S.shape[2]
    rdt = torch.float64 if S.dtype == torch.complex128 else torch.float32
    Fx, Fy = (f.to(S.device) for f in dft_matrices(H, W, m1, m2, rdt))
    w = (col_weights(W, m2, rdt) if weights else torch.ones(m2, dtype=rdt)).to(S.device)
    scale = 1.0 / (H * W) if scale is None else scale
    return torch.einsum("rx,brkc,yk->bxyc", Fx.conj(), S * w.view(1, 1, m2, 1).to(S.dtype), Fy.conj()).real * scale


def mix(X, w1, w2, adjoint=False):
    """X complex [B, 2 m1, m2, K]; w1, w2 real [2, Cin, Cout, m1, m2] -> complex [B, 2 m1, m2, N]: sum_i X W[i, o] per mode,
    weights1 on the rows below m1, weights2 above; adjoint: sum_o X conj(W[i, o])"""
    m1 = w1.shape[3]
    outs = []
    for blk, w in ((X[:, :m1], w1), (X[:, m1:], w2)):
        Wc = torch.complex(w[0], w[1]).to(X.dtype)
        outs.append(torch.einsum("brko,iork->brki", blk, Wc.conj()) if adjoint else torch.einsum("brki,iork->brko", blk, Wc))
    return torch.cat(outs, dim=1)


def mix_wgrad(X, dO):
    """(dweights1, dweights2) real [2, Cin, Cout, m1, m2]: dW = sum_b conj(X) dO"""
    m1 = X.shape[1] // 2
    outs = []
    for a, b in ((X[:, :m1], dO[:, :m1]), (X[:, m1:], dO[:, m1:])):
        d = torch.einsum("brki,brko->iork", a.conj(), b)
        outs.append(torch.stack([d.real, d.imag]))
    return outs


def spectral_conv(x, w1, w2):
    """SpectralConv2d_fast on a channels-last x [B, H, W, Cin] -> [B, H, W, Cout]"""
    m1, m2 = w1.shape[3], w1.shape[4]
    return irfft2_kept(mix(rfft2_kept(x, m1, m2), w1, w2), x.shape[1], x.shape[2])


def spectral_conv_grads(x, w1, w2, g):
    """the dense formulas of the backward: (dx, dweights1, dweights2) for the upstream gradient g [B, H, W, Cout]"""
    H, W = x.shape[1], x.shape[2]
    m1, m2 = w1.shape[3], w1.shape[4]
    X = rfft2_kept(x, m1, m2)
    dO = rfft2_kept(g, m1, m2) * (col_weights(W, m2, x.dtype) / (H * W)).view(1, 1, m2, 1)
    dx = irfft2_kept(mix(dO, w1, w2, adjoint=True), H, W, weights=False, scale=1.0)
    d1, d2 = mix_wgrad(X, dO)
    return dx, d1, d2


def to_planes(S):
    """complex [B, R, m2, C] -> the kernels' layout, real [B, R, m2, 2, C]"""
    return torch.stack([S.real, S.imag], dim=3)


def from_planes(P):
    return torch.complex(P[:, :, :, 0], P[:, :, :, 1])


def fno_layer(x, w1, w2, cw, cb):
    """gelu(SpectralConv2d_fast(x) + Conv2d 1x1(x)); cw [Cout, Cin]"""
    return F.gelu(spectral_conv(x, w1, w2) + x @ cw.t() + cb)


# ---- weights and inputs -----------------------------------------------------------------------------------------------------
def layer_inputs(name):
    """(x [B, H, W, Cin], g [B, H, W, Cout], weights1, weights2) of a recorded layer case, fp32"""
    i = list(LAYER_CASES).index(name)
    B, H, W, Cin, Cout, m1, m2 = LAYER_CASES[name]
    x = R.recipe_input((B, H, W, Cin), LAYER_SALT + i)
    g = R.recipe_input((B, H, W, Cout), LAYER_SALT + 50 + i)
    w1 = spectral_weight("weights1", (2, Cin, Cout, m1, m2), LAYER_SALT + i)
    w2 = spectral_weight("weights2", (2, Cin, Cout, m1, m2), LAYER_SALT + i)
    return x, g, w1, w2


def spectral_weight(name, shape, salt):
    """the reference initialises with rand / (Cin Cout), which makes the spectral branch invisible beside the convolution:
    scaled up by Cin and centred"""
    return ((R.recipe_tensor(name, tuple(shape), salt) - 0.5) * (2.0 / shape[2])).to(torch.float32).contiguous()


def recipe_sd(shapes, salt):
    """closed-form weights keyed by parameter name; `shapes`: the state_dict name -> shape list of the model"""
    sd = OrderedDict()
    for name, shape in shapes.items():
        shape = tuple(shape)
        u = R.recipe_tensor(name, shape, salt)
        if ".weights" in name:
            sd[name] = spectral_weight(name, shape, salt)
            continue
        if name.startswith("ln_layers.") and name.endswith(".weight"):
            v = 0.75 + 0.5 * u
        elif name.startswith("ln_layers."):
            v = (u - 0.5) * 0.2
        elif name.endswith(".bias"):
            v = (u - 0.5) * 0.1
        else:
            v = (u - 0.5) * 2.0 * math.sqrt(3.0 / max(int(np.prod(shape[1:])), 1))
        sd[name] = v.to(torch.float32).contiguous()
    return sd


def model_inputs(tag):
    """(x, y, mask, cls cotangent) of a recorded mini model, fp32; the target lives where the prediction does (latent size)"""
    cfg, salt = MODELS[tag]
    S, B, h = cfg["img_size"], MODEL_B, cfg["img_size"] // cfg["patch_size"]
    x = R.recipe_input((B, S, S, cfg["in_timesteps"], cfg["n_channels"]), salt)
    y = R.recipe_input((B, h, h, cfg["out_timesteps"], cfg["n_channels"]), salt + 1)
    msk = (R.recipe_tensor("mask", tuple(y.shape), salt) > 0.25).to(torch.float32)
    gc = R.recipe_input((B, cfg["n_cls"]), salt + 2)
    return x, y, msk, gc


def step_inputs():
    cfg, st = MINI1, STEP
    S, B = cfg["img_size"], MODEL_B
    xx = R.recipe_input((B, S, S, cfg["in_timesteps"], cfg["n_channels"]), st["salt"])
    yy = R.recipe_input((B, S, S, st["T_ar"], cfg["n_channels"]), st["salt"] + 1)
    msk = (R.recipe_tensor("mask", (B, S, S, 1, cfg["n_channels"]), st["salt"]) > 0.25).to(torch.float32)
    return xx, yy, msk


def expected_shapes(cfg):
    """the reference's state_dict layout, restated: name -> shape, in order"""
    Wd, P, K = cfg["width"], cfg["patch_size"], cfg["n_channels"] * cfg["in_timesteps"]
    hid = K * P + 2
    sh = OrderedDict()
    sh["patch_embed.proj.0.weight"], sh["patch_embed.proj.0.bias"] = (hid, K + 2, P, P), (hid,)
    sh["patch_embed.proj.2.weight"], sh["patch_embed.proj.2.bias"] = (Wd, hid, 1, 1), (Wd,)
    for i in range(cfg["n_layers"]):
        for n in ("weights1", "weights2"):
            sh[f"spectral_convs.{i}.{n}"] = (2, Wd, Wd, cfg["modes1"], cfg["modes2"])
    for i in range(cfg["n_layers"]):
        sh[f"convs.{i}.weight"], sh[f"convs.{i}.bias"] = (Wd, Wd, 1, 1), (Wd,)
    if cfg["normalize"]:
        sh["scale_feats.weight"], sh["scale_feats.bias"] = (Wd, 2 * cfg["n_channels"]), (Wd,)
    if cfg["use_ln"]:
        for i in range(cfg["n_layers"]):
            sh[f"ln_layers.{i}.weight"], sh[f"ln_layers.{i}.bias"] = (Wd,), (Wd,)
    sh["fc1.weight"], sh["fc1.bias"] = (Wd, Wd), (Wd,)
    sh["fc2.weight"], sh["fc2.bias"] = (cfg["n_channels"] * cfg["out_timesteps"], Wd), (cfg["n_channels"] * cfg["out_timesteps"],)
    for j, n in ((0, Wd), (2, Wd), (4, cfg["n_cls"])):
        sh[f"cls_head.{j}.weight"], sh[f"cls_head.{j}.bias"] = (n, Wd), (n,)
    return sh


# ---- the model --------------------------------------------------------------------------------------------------------------
def fno_forward(sd, x, cfg):
    """x [B, X, Y, T, C] -> (pred [B, X/P, Y/P, T_out, C], cls_pred [B, n_cls]); sd: name -> tensor of x's dtype"""
    B, S, _, T, C = x.shape
    P, Wd = cfg["patch_size"], cfg["width"]
    h = S // P
    sf = 0.0
    if cfg["normalize"]:
        mu = x.mean(dim=(1, 2, 3), keepdim=True)
        sigma = x.std(dim=(1, 2, 3), keepdim=True) + 1e-6
        x = (x - mu) / sigma
        stat = torch.cat([mu, sigma], dim=-1)[:, 0, 0, 0, :]
        sf = (stat @ sd["scale_feats.weight"].t() + sd["scale_feats.bias"])[:, None, None, :]
    v = x.reshape(B, S, S, T * C)
    gx = R.unit_grid(S).to(x).view(1, S, 1, 1).expand(B, S, S, 1)
    gy = R.unit_grid(S).to(x).view(1, 1, S, 1).expand(B, S, S, 1)
    v = torch.cat([v, gx, gy], dim=-1)                                                   # [B, S, S, K + 2]
    K2 = v.shape[-1]
    a = v.view(B, h, P, h, P, K2).permute(0, 1, 3, 5, 2, 4).reshape(B, h, h, K2 * P * P)  # columns (c, i, j)
    w0 = sd["patch_embed.proj.0.weight"]
    hid = w0.shape[0]
    v = F.gelu(a @ w0.reshape(hid, -1).t() + sd["patch_embed.proj.0.bias"])
    v = v @ sd["patch_embed.proj.2.weight"].reshape(Wd, hid).t() + sd["patch_embed.proj.2.bias"] + sf
    for i in range(cfg["n_layers"]):
        v = fno_layer(v, sd[f"spectral_convs.{i}.weights1"], sd[f"spectral_convs.{i}.weights2"],
                      sd[f"convs.{i}.weight"].reshape(Wd, Wd), sd[f"convs.{i}.bias"])
        if cfg["use_ln"]:
            v = F.group_norm(v.permute(0, 3, 1, 2), 4, sd[f"ln_layers.{i}.weight"], sd[f"ln_layers.{i}.bias"]).permute(0, 2, 3, 1)
    c = v.mean(dim=(1, 2))
    c = F.gelu(c @ sd["cls_head.0.weight"].t() + sd["cls_head.0.bias"])
    c = F.gelu(c @ sd["cls_head.2.weight"].t() + sd["cls_head.2.bias"])
    cls_pred = c @ sd["cls_head.4.weight"].t() + sd["cls_head.4.bias"]
    v = F.gelu(v @ sd["fc1.weight"].t() + sd["fc1.bias"])
    v = v @ sd["fc2.weight"].t() + sd["fc2.bias"]
    y = v.reshape(B, h, h, cfg["out_timesteps"], C)
    if cfg["normalize"]:
        y = y * sigma + mu
    return y, cls_pred


def model_loss(pred, cls_pred, y, msk, gc):
    return R.rel_l2_loss(pred, y, msk) + (cls_pred * gc).sum()


def run_model_ref(tag, dtype=torch.float64):
    """restatement of a recorded mini model in `dtype`: (pred, cls_pred, {name: gradient}, input gradient)"""
    cfg, salt = MODELS[tag]
    x, y, msk, gc = model_inputs(tag)
    sd = {k: v.to(dtype).requires_grad_(True) for k, v in recipe_sd(expected_shapes(cfg), salt).items()}
    xi = x.detach().clone().to(dtype).requires_grad_(True)
    pred, cls_pred = fno_forward(sd, xi, cfg)
    model_loss(pred, cls_pred, y.to(dtype), msk.to(dtype), gc.to(dtype)).backward()
    return pred.detach(), cls_pred.detach(), {k: v.grad for k, v in sd.items()}, xi.grad


# ---- inputs and float32 compositions of the GPU operator cases ---------------------------------------------------------------
def transform_inputs(case):
    """(x [B, H, W, C], spectrum planes [B, 2 m1, m2, 2, C]) fp32"""
    B, H, W, C, m1, m2 = case
    k = TRANSFORM_CASES.index(case)
    return R.recipe_input((B, H, W, C), OP_SALT + k), R.recipe_input((B, 2 * m1, m2, 2, C), OP_SALT + 100 + k)


def mix_inputs(case):
    """(X planes [B, 2 m1, m2, 2, Cin], dO planes [.., Cout], weights1, weights2) fp32"""
    B, Cin, Cout, m1, m2 = case
    k = MIX_CASES.index(case)
    X = R.recipe_input((B, 2 * m1, m2, 2, Cin), OP_SALT + 200 + k)
    dO = R.recipe_input((B, 2 * m1, m2, 2, Cout), OP_SALT + 300 + k)
    w1 = spectral_weight("weights1", (2, Cin, Cout, m1, m2), OP_SALT + 200 + k)
    w2 = spectral_weight("weights2", (2, Cin, Cout, m1, m2), OP_SALT + 200 + k)
    return X, dO, w1, w2


def transform_ref(case, dtype=torch.float64):
    """the four roles in `dtype` from the dense sums: dict fwd (rfft2 kept), adj_inv (the adjoint of irfft2: weights and
    1 / (H W)), inv (irfft2), adj_fwd (the adjoint of rfft2); spectra as planes"""
    B, H, W, C, m1, m2 = case
    x, Sp = transform_inputs(case)
    x, S = x.to(dtype), from_planes(Sp.to(dtype))
    Xk = rfft2_kept(x, m1, m2)
    return {"fwd": to_planes(Xk),
            "adj_inv": to_planes(Xk * (col_weights(W, m2, dtype) / (H * W)).view(1, 1, m2, 1)),
            "inv": irfft2_kept(S, H, W),
            "adj_fwd": irfft2_kept(S, H, W, weights=False, scale=1.0)}


def transform_fft32(case):
    """the same four roles as the float32 composition of torch.fft the reference's layer (and its autograd) runs: rfft2 and a
    slice; a zero-filled half spectrum and irfft2; for the adjoint of rfft2 a zero-filled FULL spectrum and ifft2"""
    B, H, W, C, m1, m2 = case
    x, Sp = transform_inputs(case)
    S = from_planes(Sp)
    Xf = torch.fft.rfft2(x, dim=(1, 2))
    Xk = torch.cat([Xf[:, :m1, :m2], Xf[:, H - m1:, :m2]], dim=1)
    half = torch.zeros(B, H, W // 2 + 1, C, dtype=torch.complex64)
    half[:, :m1, :m2], half[:, H - m1:, :m2] = S[:, :m1], S[:, m1:]
    full = torch.zeros(B, H, W, C, dtype=torch.complex64)
    full[:, :m1, :m2], full[:, H - m1:, :m2] = S[:, :m1], S[:, m1:]
    return {"fwd": to_planes(Xk),
            "adj_inv": to_planes(Xk * (col_weights(W, m2, torch.float32) / (H * W)).view(1, 1, m2, 1)),
            "inv": torch.fft.irfft2(half, s=(H, W), dim=(1, 2)),
            "adj_fwd": torch.fft.ifft2(full, dim=(1, 2)).real * (H * W)}


def mix_ref(case, dtype=torch.float64):
    """dict fwd, dgrad (planes), dw1, dw2 in `dtype` with a complex spectrum of that precision"""
    X, dO, w1, w2 = (t.to(dtype) for t in mix_inputs(case))
    Xc, dOc = from_planes(X), from_planes(dO)
    d1, d2 = mix_wgrad(Xc, dOc)
    return {"fwd": to_planes(mix(Xc, w1, w2)), "dgrad": to_planes(mix(dOc, w1, w2, adjoint=True)), "dw1": d1, "dw2": d2}


def mix_einsum32(case):
    """the reference's float32 composition: four real einsums per block (compl_mul2d), and their autograd"""
    X, dO, w1, w2 = mix_inputs(case)
    m1 = w1.shape[3]
    w1, w2 = w1.clone().requires_grad_(True), w2.clone().requires_grad_(True)
    X = X.clone().requires_grad_(True)

    def cm(inp, w):                      # inp planes [B, m1, m2, 2, Cin]
        re, im = inp[:, :, :, 0], inp[:, :, :, 1]
        o_re = torch.einsum("bxyi,ioxy->bxyo", re, w[0]) - torch.einsum("bxyi,ioxy->bxyo", im, w[1])
        o_im = torch.einsum("bxyi,ioxy->bxyo", re, w[1]) + torch.einsum("bxyi,ioxy->bxyo", im, w[0])
        return torch.stack([o_re, o_im], dim=3)

    O = torch.cat([cm(X[:, :m1], w1), cm(X[:, m1:], w2)], dim=1)
    (O * dO).sum().backward()
    fwd = O.detach()
    # the data gradient takes dO as its input: <cm(X), dO> differentiated in X is sum_o dO conj(W)
    return {"fwd": fwd, "dw1": w1.grad, "dw2": w2.grad, "dgrad": X.grad}


def nerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
