"""Restatement of the reference's 3-D FNO baseline (models/fno.py:290-435: SpectralConv3d, FNO3d) and of its Adam on complex
parameters (utils/optimizer.py:40-52), written from the mathematics with torch ops and oracle/dpot_ref.py - no reference code.
The spectral layer is the dense sums over the kept modes, one axis after the other, with a complex spectrum of the run's own
precision (complex128 for float64 inputs: the reference allocates its output spectrum as cfloat whatever the input, so its own
float64 run cannot be the yardstick).  Channels-last throughout; the spectral weights are complex [Cin, Cout, m1, m2, m3], the
reference's layout (the package stores their view_as_real).
tests/test_cpu_fno3d.py holds it to the reference's records (tests/golden/g23_fno3d.npz); the GPU tests use it as the float64
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
# the spectral layer, recorded from the reference's own class: name -> (B, X, Y, Z, Cin, Cout, m1, m2, m3)
LAYER_CASES = OrderedDict([
    ("x6y5z7_c3", (2, 6, 5, 7, 3, 3, 3, 2, 2)),               # odd, non-cubic, 2 m1 = X
    ("x8_c4to2_nyq", (1, 8, 8, 8, 4, 2, 4, 4, 5)),            # both axes full, the Nyquist plane kept, Cin != Cout
    ("x5y4z6_c2to5", (2, 5, 4, 6, 2, 5, 2, 2, 4)),            # even Z with its Nyquist plane, 2 m2 = Y, Cin != Cout
])
LAYER_SALT = 1600     # case i: x salt LAYER_SALT + i, upstream gradient + 50, weights by name with that salt

# the transforms on the GPU: (B, X, Y, Z, C, m1, m2, m3).  Cases 0-3 are the issue's, 4-6 cross the kernels' tile boundaries,
# case 7 is the declared maximum (tests/test_gpu_fno3d.py names them)
TRANSFORM_CASES = [
    (2, 6, 5, 7, 3, 3, 2, 2), (1, 8, 8, 8, 4, 4, 4, 5), (1, 5, 4, 6, 4, 2, 2, 4), (1, 4, 6, 5, 1, 1, 1, 1),
    (1, 9, 17, 17, 20, 4, 5, 9), (1, 8, 16, 16, 18, 4, 2, 8), (2, 17, 8, 14, 16, 8, 4, 8),
    (1, 128, 128, 128, 4, 32, 32, 32),
]
# (B, Cin, Cout, m1, m2, m3): the issue's
MIX_CASES = [(1, 1, 1, 1, 1, 1), (3, 5, 7, 2, 3, 2), (33, 4, 4, 2, 1, 2), (5, 20, 36, 1, 2, 3)]
OP_SALT = 1700
WEIGHT_NAMES = ("weights1", "weights2", "weights3", "weights4")

# mini models: (constructor arguments, the (X, Y, Z) of the input window - the forward takes non-cubic fields -, salt)
MINI1 = dict(modes1=2, modes2=2, modes3=3, width=8, img_size=6, n_channels=2, in_timesteps=3, out_timesteps=1, n_layers=2,
             patch_size=1, use_ln=False, normalize=False, n_cls=0)
MINI2 = dict(modes1=2, modes2=3, modes3=2, width=8, img_size=6, n_channels=2, in_timesteps=3, out_timesteps=1, n_layers=2,
             patch_size=1, use_ln=True, normalize=True, n_cls=0)
MODELS = OrderedDict([("m1", (MINI1, (6, 5, 7), 1810)), ("m2", (MINI2, (4, 6, 5), 1820))])
MODEL_B = 2
DX_STRIDE = 3
STEP_STRIDE = 3       # over (re, im) PAIRS of the flat buffers (every recorded tensor has an even length): pairs stay whole
STEP = dict(T_ar=2, lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=5.0, eps=1e-8, salt=1840, size=(6, 5, 7))


def hash_input(shape, salt):
    return R.recipe_input(tuple(shape), salt)


def _cdtype(dtype):
    return torch.complex128 if dtype in (torch.float64, torch.complex128) else torch.complex64


def _rdtype(dtype):
    return torch.float64 if dtype in (torch.float64, torch.complex128) else torch.float32


# ---- the transforms -------------------------------------------------------------------------------------------------------
def kept(N, m):
    """the 2 m kept wavenumbers of a two-sided axis, in the spectrum's order"""
    return np.concatenate([np.arange(m), np.arange(N - m, N)])


def plane_weights(Z, m3, dtype=torch.float64):
    """irfftn on a spectrum that is not Hermitian: weight 1 at kz = 0 and, for even Z, at kz = Z / 2, else 2 (the imaginary
    parts of those planes' z-transforms are dropped)"""
    w = torch.full((m3,), 2.0, dtype=dtype)
    w[0] = 1.0
    if Z % 2 == 0 and Z // 2 < m3:
        w[Z // 2] = 1.0
    return w


def dft_matrix(N, ks, dtype=torch.float64):
    """complex [N, len(ks)]: e^{-2 pi i k n / N}; float64 angles reduced in integers"""
    a = 2.0 * np.pi * ((np.arange(N)[:, None] * np.asarray(ks)[None, :]) % N) / N
    return torch.from_numpy(np.exp(-1j * a)).to(_cdtype(dtype))


def dft_matrices(X, Y, Z, m1, m2, m3, dtype=torch.float64):
    return dft_matrix(X, kept(X, m1), dtype), dft_matrix(Y, kept(Y, m2), dtype), dft_matrix(Z, np.arange(m3), dtype)


def rfft3_kept(x, m1, m2, m3):
    """x [B, X, Y, Z, C] real -> complex [B, 2 m1, 2 m2, m3, C]: the kept modes of the unnormalised rfftn"""
    Fx, Fy, Fz = (f.to(x.device) for f in dft_matrices(*x.shape[1:4], m1, m2, m3, x.dtype))
    t = torch.einsum("bxyzc,zk->bxykc", x.to(Fz.dtype), Fz)
    t = torch.einsum("bxykc,yq->bxqkc", t, Fy)
    return torch.einsum("bxqkc,xr->brqkc", t, Fx)


def irfft3_kept(S, X, Y, Z, weights=True, scale=None):
    """complex [B, 2 m1, 2 m2, m3, C] -> real [B, X, Y, Z, C]: irfftn of the spectrum that is zero off the kept modes
    (weights=True, scale 1 / (X Y Z)); weights=False, scale=1: the adjoint of rfft3_kept"""
    m1, m2, m3 = S.shape[1] // 2, S.shape[2] // 2, S.shape[3]
    rdt = _rdtype(S.dtype)
    Fx, Fy, Fz = (f.to(S.device) for f in dft_matrices(X, Y, Z, m1, m2, m3, rdt))
    w = (plane_weights(Z, m3, rdt) if weights else torch.ones(m3, dtype=rdt)).to(S.device)
    scale = 1.0 / (X * Y * Z) if scale is None else scale
    t = torch.einsum("brqkc,xr->bxqkc", S * w.view(1, 1, 1, m3, 1).to(S.dtype), Fx.conj())
    t = torch.einsum("bxqkc,yq->bxykc", t, Fy.conj())
    return torch.einsum("bxykc,zk->bxyzc", t, Fz.conj()).real * scale


def corners(m1, m2):
    """(rows, columns) slices of the four corner blocks in weight order: weights1 low kx low ky, weights2 high kx low ky,
    weights3 low kx high ky, weights4 high kx high ky"""
    lo1, hi1, lo2, hi2 = slice(0, m1), slice(m1, 2 * m1), slice(0, m2), slice(m2, 2 * m2)
    return [(lo1, lo2), (hi1, lo2), (lo1, hi2), (hi1, hi2)]


def mix(Xs, ws, adjoint=False):
    """Xs complex [B, 2 m1, 2 m2, m3, K]; ws four complex [Cin, Cout, m1, m2, m3] -> complex [B, 2 m1, 2 m2, m3, N]: sum_i X
    W[i, o] per mode of each corner; adjoint: sum_o X conj(W[i, o])"""
    m1, m2 = ws[0].shape[2], ws[0].shape[3]
    N = ws[0].shape[0] if adjoint else ws[0].shape[1]
    out = torch.zeros(*Xs.shape[:4], N, dtype=Xs.dtype)
    for (r, q), w in zip(corners(m1, m2), ws):
        w = w.to(Xs.dtype)
        out[:, r, q] = torch.einsum("brqko,iorqk->brqki", Xs[:, r, q], w.conj()) if adjoint else \
            torch.einsum("brqki,iorqk->brqko", Xs[:, r, q], w)
    return out


def mix_wgrad(Xs, dO):
    """(dweights1..4) complex [Cin, Cout, m1, m2, m3]: dW = sum_b conj(X) dO per corner"""
    m1, m2 = Xs.shape[1] // 2, Xs.shape[2] // 2
    return [torch.einsum("brqki,brqko->iorqk", Xs[:, r, q].conj(), dO[:, r, q]) for r, q in corners(m1, m2)]


def spectral_conv(x, ws):
    """SpectralConv3d on a channels-last x [B, X, Y, Z, Cin] -> [B, X, Y, Z, Cout]"""
    m1, m2, m3 = ws[0].shape[2:5]
    return irfft3_kept(mix(rfft3_kept(x, m1, m2, m3), ws), *x.shape[1:4])


def spectral_conv_grads(x, ws, g):
    """the dense formulas of the backward: (dx, [dweights1..4] complex) for the upstream gradient g [B, X, Y, Z, Cout].  The
    weight gradients follow torch's convention for complex leaves: dL/dRe + i dL/dIm"""
    X, Y, Z = x.shape[1:4]
    m1, m2, m3 = ws[0].shape[2:5]
    Xs = rfft3_kept(x, m1, m2, m3)
    dO = rfft3_kept(g, m1, m2, m3) * (plane_weights(Z, m3, x.dtype) / (X * Y * Z)).view(1, 1, 1, m3, 1)
    dx = irfft3_kept(mix(dO, ws, adjoint=True), X, Y, Z, weights=False, scale=1.0)
    return dx, mix_wgrad(Xs, dO)


def to_planes(S):
    """complex [B, R, Q, m3, C] -> the kernels' layout, real [B, R, Q, m3, 2, C]"""
    return torch.stack([S.real, S.imag], dim=4)


def from_planes(P):
    return torch.complex(P[:, :, :, :, 0], P[:, :, :, :, 1])


def pairs(w):
    """complex weight -> the package's parameter, real [..., 2]"""
    return torch.view_as_real(w.resolve_conj()).contiguous()


def fno3_layer(x, ws, cw, cb):
    """gelu(SpectralConv3d(x) + Conv3d 1x1x1(x)); cw [Cout, Cin]"""
    return F.gelu(spectral_conv(x, ws) + x @ cw.t() + cb)


# ---- weights and inputs -----------------------------------------------------------------------------------------------------
def spectral_weight(name, shape, salt):
    """complex64 [Cin, Cout, m1, m2, m3].  The reference initialises with rand / (Cin Cout), which makes the spectral branch
    invisible beside the convolution: scaled up by Cin and centred, so that |g| of the training step is far from Adam's eps"""
    re = (R.recipe_tensor(name + ".re", tuple(shape), salt) - 0.5) * (2.0 / shape[1])
    im = (R.recipe_tensor(name + ".im", tuple(shape), salt) - 0.5) * (2.0 / shape[1])
    return torch.complex(re.to(torch.float32), im.to(torch.float32)).contiguous()


def layer_inputs(name):
    """(x [B, X, Y, Z, Cin], g [B, X, Y, Z, Cout], [weights1..4] complex64) of a recorded layer case"""
    i = list(LAYER_CASES).index(name)
    B, X, Y, Z, Cin, Cout, m1, m2, m3 = LAYER_CASES[name]
    x = R.recipe_input((B, X, Y, Z, Cin), LAYER_SALT + i)
    g = R.recipe_input((B, X, Y, Z, Cout), LAYER_SALT + 50 + i)
    return x, g, [spectral_weight(n, (Cin, Cout, m1, m2, m3), LAYER_SALT + i) for n in WEIGHT_NAMES]


def conv_inputs(Cin, Cout):
    cw = ((R.recipe_tensor("convw", (Cout, Cin), 61) - 0.5) * 2.0 / math.sqrt(Cin)).float()
    cb = ((R.recipe_tensor("convb", (Cout,), 61) - 0.5) * 0.2).float()
    return cw, cb


def expected_layout(cfg):
    """the reference's state_dict layout, restated: name -> (shape, dtype), in order"""
    Wd, K = cfg["width"], cfg["n_channels"] * cfg["in_timesteps"]
    f, c = torch.float32, torch.complex64
    sh = OrderedDict()
    sh["fc0.weight"], sh["fc0.bias"] = ((Wd, K + 3), f), ((Wd,), f)
    for i in range(cfg["n_layers"]):
        for n in WEIGHT_NAMES:
            sh[f"spectral_convs.{i}.{n}"] = ((Wd, Wd, cfg["modes1"], cfg["modes2"], cfg["modes3"]), c)
    for i in range(cfg["n_layers"]):
        sh[f"convs.{i}.weight"], sh[f"convs.{i}.bias"] = ((Wd, Wd, 1, 1, 1), f), ((Wd,), f)
    if cfg["normalize"]:
        sh["scale_feats.weight"], sh["scale_feats.bias"] = ((Wd, 2 * cfg["n_channels"]), f), ((Wd,), f)
    if cfg["use_ln"]:
        for i in range(cfg["n_layers"]):
            sh[f"ln_layers.{i}.weight"], sh[f"ln_layers.{i}.bias"] = ((Wd,), f), ((Wd,), f)
    sh["fc1.weight"], sh["fc1.bias"] = ((Wd, Wd), f), ((Wd,), f)
    n_out = cfg["n_channels"] * cfg["out_timesteps"]
    sh["fc2.weight"], sh["fc2.bias"] = ((n_out, Wd), f), ((n_out,), f)
    return sh


def recipe_sd(layout, salt):
    """closed-form weights keyed by parameter name; `layout`: name -> (shape, dtype); complex64 where the reference's are"""
    sd = OrderedDict()
    for name, (shape, dtype) in layout.items():
        shape = tuple(shape)
        if dtype.is_complex:
            sd[name] = spectral_weight(name, shape, salt)
            continue
        u = R.recipe_tensor(name, shape, salt)
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
    """(x, y, mask) of a recorded mini model, fp32"""
    cfg, (X, Y, Z), salt = MODELS[tag]
    x = R.recipe_input((MODEL_B, X, Y, Z, cfg["in_timesteps"], cfg["n_channels"]), salt)
    y = R.recipe_input((MODEL_B, X, Y, Z, cfg["out_timesteps"], cfg["n_channels"]), salt + 1)
    msk = (R.recipe_tensor("mask", tuple(y.shape), salt) > 0.25).to(torch.float32)
    return x, y, msk


def step_inputs():
    cfg, st = MINI1, STEP
    X, Y, Z = st["size"]
    xx = R.recipe_input((MODEL_B, X, Y, Z, cfg["in_timesteps"], cfg["n_channels"]), st["salt"])
    yy = R.recipe_input((MODEL_B, X, Y, Z, st["T_ar"], cfg["n_channels"]), st["salt"] + 1)
    msk = (R.recipe_tensor("mask", (MODEL_B, X, Y, Z, 1, cfg["n_channels"]), st["salt"]) > 0.25).to(torch.float32)
    return xx, yy, msk


def pair_stride(t):
    """every STEP_STRIDE-th (re, im) pair of a flat real buffer"""
    return t.reshape(-1, 2)[::STEP_STRIDE].reshape(-1)


# ---- the model --------------------------------------------------------------------------------------------------------------
def fno3_forward(sd, x, cfg):
    """x [B, X, Y, Z, T, C] -> pred [B, X, Y, Z, T_out, C]; sd: name -> tensor of x's precision (complex weights complex).
    scale_feats is never read, as in the reference"""
    B, X, Y, Z, T, C = x.shape
    Wd = cfg["width"]
    g = [R.unit_grid(n).to(x) for n in (X, Y, Z)]
    v = torch.cat([x.reshape(B, X, Y, Z, T * C), g[0].view(1, X, 1, 1, 1).expand(B, X, Y, Z, 1),
                   g[1].view(1, 1, Y, 1, 1).expand(B, X, Y, Z, 1), g[2].view(1, 1, 1, Z, 1).expand(B, X, Y, Z, 1)], dim=-1)
    v = v @ sd["fc0.weight"].t() + sd["fc0.bias"]
    for i in range(cfg["n_layers"]):
        v = fno3_layer(v, [sd[f"spectral_convs.{i}.{n}"] for n in WEIGHT_NAMES], sd[f"convs.{i}.weight"].reshape(Wd, Wd),
                       sd[f"convs.{i}.bias"])
        if cfg["use_ln"]:
            v = F.group_norm(v.permute(0, 4, 1, 2, 3), 4, sd[f"ln_layers.{i}.weight"],
                             sd[f"ln_layers.{i}.bias"]).permute(0, 2, 3, 4, 1)
    v = F.gelu(v @ sd["fc1.weight"].t() + sd["fc1.bias"])
    v = v @ sd["fc2.weight"].t() + sd["fc2.bias"]
    return v.reshape(B, X, Y, Z, cfg["out_timesteps"], C)


def sd_to(sd, dtype):
    """the recipe weights in float64 / complex128 (or float32 / complex64) leaves"""
    return {k: v.to(_cdtype(dtype) if v.is_complex() else dtype).requires_grad_(True) for k, v in sd.items()}


def real_grad(g):
    """a leaf's gradient as the package reports it: complex ones as (re, im) pairs"""
    return pairs(g) if g.is_complex() else g


def run_model_ref(tag, dtype=torch.float64):
    """restatement of a recorded mini model in `dtype`: (pred, {name: gradient, complex ones as pairs}, input gradient);
    scale_feats has no gradient"""
    cfg, _, salt = MODELS[tag]
    x, y, msk = model_inputs(tag)
    sd = sd_to(recipe_sd(expected_layout(cfg), salt), dtype)
    xi = x.detach().clone().to(dtype).requires_grad_(True)
    pred = fno3_forward(sd, xi, cfg)
    R.rel_l2_loss(pred, y.to(dtype), msk.to(dtype)).backward()
    return pred.detach(), {k: real_grad(v.grad) for k, v in sd.items() if v.grad is not None}, xi.grad


def run_step_ref(dtype=torch.float64):
    """the two-AR-step loop of finetune3d.py:206-229 up to the clip, restated: (step losses, {name: gradient as the package
    reports it}, gradient norm, {name: starting parameter as pairs})"""
    cfg, st = MINI1, STEP
    xx, yy, msk = (t.to(dtype) for t in step_inputs())
    sd0 = recipe_sd(expected_layout(cfg), st["salt"])
    sd = sd_to(sd0, dtype)
    loss, losses = 0.0, []
    for t in range(st["T_ar"]):
        im = fno3_forward(sd, xx, cfg)
        l = R.rel_l2_loss(im, yy[..., t:t + 1, :], msk)
        losses.append(l.item())
        loss = loss + l
        xx = torch.cat((xx[..., 1:, :], im), dim=-2)
    loss.backward()
    grads = OrderedDict((k, real_grad(v.grad)) for k, v in sd.items() if v.grad is not None)
    gnorm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values()))
    return losses, grads, gnorm, OrderedDict((k, real_grad(v) if v.is_complex() else v) for k, v in sd0.items())


def adam_first_step(p0, g, gnorm, is_pair, per_component=False):
    """ONE step of the reference's Adam (utils/optimizer.py:26-52) from zero moments, after clip_grad_norm_, in float64 on real
    buffers: g' = c g + wd p; m = (1 - b1) g'; v = (1 - b2) |g'|^2 with |g'|^2 = g're^2 + g'im^2 shared by the two slots of a
    pair (exp_avg_sq accumulates grad * conj(grad)) where is_pair, else g'^2 per element; p - lr / bc1 * m / (sqrt(v) /
    sqrt(bc2) + eps).  per_component=True: Adam on the real view instead (what the pair rule replaces)"""
    st = STEP
    b1, b2 = st["betas"]
    c = min(1.0, st["max_norm"] / (gnorm + 1e-6))
    p0, g = p0.double().reshape(-1), g.double().reshape(-1)
    ge = c * g + st["weight_decay"] * p0
    sq = ge * ge
    if is_pair and not per_component:
        sq = sq.view(-1, 2).sum(dim=1, keepdim=True).expand(-1, 2).reshape(-1)
    m, v = (1 - b1) * ge, (1 - b2) * sq
    return p0 - st["lr"] / (1 - b1) * m / (v.sqrt() / math.sqrt(1 - b2) + st["eps"])


def step_param_tolerance(ref_g, ref_p, p0, owner, names, gnorm):
    """Per-element tolerance of the parameters after the recorded Adam step (all arguments as recorded: every STEP_STRIDE-th pair
    of the flat buffers, float64; owner: the index into `names` of each element).  The contract on the parameters themselves
    (1e-4 |p| + 1e-4 max|p| per tensor) plus what Adam's first step makes of a gradient that differs within ITS contract
    tol_g = c (1e-4 |g| + 1e-4 max|g|): the step is -lr u(g'), u(g') = g' / (|g'| + eps), with |g'| the modulus of the complex
    number for a pair and of the element otherwise.  The Jacobian of u is I / (|g'| + eps) - g' g'^T / (|g'| (|g'| + eps)^2),
    of norm at most 1 / (|g'| + eps), so a perturbation of size d moves u by at most d / (|g'| - d + eps) (and never by more
    than 2); d = tol_g for an element, the sum of the two elements' tol_g for a pair."""
    st = STEP
    c = min(1.0, st["max_norm"] / (gnorm + 1e-6))
    tol = torch.zeros_like(ref_p)
    for i, n in enumerate(names):
        sel = owner == i
        if not sel.any():
            continue
        g, p = ref_g[sel], ref_p[sel]
        d = c * (1e-4 * g.abs() + 1e-4 * g.abs().max())
        ge = (c * g + st["weight_decay"] * p0[sel]).abs()
        if ".weights" in n:
            ge = ge.view(-1, 2).pow(2).sum(dim=1, keepdim=True).sqrt().expand(-1, 2).reshape(-1)
            d = d.view(-1, 2).sum(dim=1, keepdim=True).expand(-1, 2).reshape(-1)
        move = st["lr"] * torch.clamp(d / ((ge - d).clamp(min=0.0) + st["eps"]), max=2.0)
        tol[sel] = 1e-4 * p.abs() + 1e-4 * p.abs().max() + move
    return tol


# ---- inputs and float32 compositions of the GPU operator cases ---------------------------------------------------------------
def transform_inputs(case):
    """(x [B, X, Y, Z, C], spectrum planes [B, 2 m1, 2 m2, m3, 2, C]) fp32"""
    B, X, Y, Z, C, m1, m2, m3 = case
    k = TRANSFORM_CASES.index(case)
    return R.recipe_input((B, X, Y, Z, C), OP_SALT + k), R.recipe_input((B, 2 * m1, 2 * m2, m3, 2, C), OP_SALT + 100 + k)


def mix_inputs(case):
    """(X planes [B, 2 m1, 2 m2, m3, 2, Cin], dO planes [.., Cout], [weights1..4] complex64); every corner's weights are their
    own recipe (the name is the salt), so a kernel that reads the wrong block cannot pass"""
    B, Cin, Cout, m1, m2, m3 = case
    k = MIX_CASES.index(case)
    X = R.recipe_input((B, 2 * m1, 2 * m2, m3, 2, Cin), OP_SALT + 200 + k)
    dO = R.recipe_input((B, 2 * m1, 2 * m2, m3, 2, Cout), OP_SALT + 300 + k)
    return X, dO, [spectral_weight(n, (Cin, Cout, m1, m2, m3), OP_SALT + 200 + k) for n in WEIGHT_NAMES]


def transform_ref(case, dtype=torch.float64):
    """the four roles in `dtype` from the dense sums: dict fwd (rfftn kept), adj_inv (the adjoint of irfftn: weights and
    1 / (X Y Z)), inv (irfftn), adj_fwd (the adjoint of rfftn); spectra as planes"""
    B, X, Y, Z, C, m1, m2, m3 = case
    x, Sp = transform_inputs(case)
    x, S = x.to(dtype), from_planes(Sp.to(dtype))
    Xk = rfft3_kept(x, m1, m2, m3)
    return {"fwd": to_planes(Xk),
            "adj_inv": to_planes(Xk * (plane_weights(Z, m3, dtype) / (X * Y * Z)).view(1, 1, 1, m3, 1)),
            "inv": irfft3_kept(S, X, Y, Z),
            "adj_fwd": irfft3_kept(S, X, Y, Z, weights=False, scale=1.0)}


def scatter(S, shape, X, Y, m1, m2, m3):
    """the kept spectrum written into a zero-filled spectrum of `shape`, as the reference fills its out_ft"""
    out = torch.zeros(shape, dtype=S.dtype)
    for (r, q), (rx, qy) in zip(corners(m1, m2), [(slice(0, m1), slice(0, m2)), (slice(X - m1, X), slice(0, m2)),
                                                  (slice(0, m1), slice(Y - m2, Y)), (slice(X - m1, X), slice(Y - m2, Y))]):
        out[:, rx, qy, :m3] = S[:, r, q]
    return out


def transform_fft32(case):
    """the same four roles as the float32 composition of torch.fft the reference's layer (and its autograd) runs: rfftn and
    four slices; a zero-filled half spectrum and irfftn; for the adjoint of rfftn a zero-filled FULL spectrum and ifftn"""
    B, X, Y, Z, C, m1, m2, m3 = case
    x, Sp = transform_inputs(case)
    S = from_planes(Sp)
    Xf = torch.fft.rfftn(x, dim=(1, 2, 3))
    rows, cols = torch.from_numpy(kept(X, m1)), torch.from_numpy(kept(Y, m2))
    Xk = Xf[:, rows][:, :, cols][:, :, :, :m3]
    half = scatter(S, (B, X, Y, Z // 2 + 1, C), X, Y, m1, m2, m3)
    full = scatter(S, (B, X, Y, Z, C), X, Y, m1, m2, m3)
    return {"fwd": to_planes(Xk),
            "adj_inv": to_planes(Xk * (plane_weights(Z, m3, torch.float32) / (X * Y * Z)).view(1, 1, 1, m3, 1)),
            "inv": torch.fft.irfftn(half, s=(X, Y, Z), dim=(1, 2, 3)),
            "adj_fwd": torch.fft.ifftn(full, dim=(1, 2, 3)).real * (X * Y * Z)}


def mix_ref(case, dtype=torch.float64):
    """dict fwd, dgrad (planes), dw1..dw4 (pairs) in `dtype` with a complex spectrum of that precision"""
    X, dO, ws = mix_inputs(case)
    Xc, dOc = from_planes(X.to(dtype)), from_planes(dO.to(dtype))
    ws = [w.to(_cdtype(dtype)) for w in ws]
    out = {"fwd": to_planes(mix(Xc, ws)), "dgrad": to_planes(mix(dOc, ws, adjoint=True))}
    out.update({f"dw{k + 1}": pairs(d) for k, d in enumerate(mix_wgrad(Xc, dOc))})
    return out


def mix_einsum32(case):
    """the reference's float32 composition: one complex64 einsum per corner (compl_mul3d), and its autograd"""
    X, dO, ws = mix_inputs(case)
    m1, m2 = ws[0].shape[2], ws[0].shape[3]
    ws = [w.clone().requires_grad_(True) for w in ws]
    Xc = from_planes(X).requires_grad_(True)
    O = torch.zeros(*Xc.shape[:4], ws[0].shape[1], dtype=torch.complex64)
    for (r, q), w in zip(corners(m1, m2), ws):
        O[:, r, q] = torch.einsum("brqki,iorqk->brqko", Xc[:, r, q], w)
    Op = to_planes(O)
    (Op * dO).sum().backward()
    out = {"fwd": Op.detach(), "dgrad": to_planes(Xc.grad)}
    out.update({f"dw{k + 1}": pairs(w.grad) for k, w in enumerate(ws)})
    return out


def nerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
