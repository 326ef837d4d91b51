"""float64 torch restatement of the reference's 3-D model pieces (models/dpot3d.py) and of the two transform definitions the
kernels of csrc/dft3.hip implement - a test-local oracle like tests/resize_ref.py.  It shares no code with dpot_amd.

Definitions (field x[B, X, Y, Z, E], kept box kx < mx, ky < my, kz < mz, w(kz) = 1 for kz = 0 and - Z even - kz = Z/2,
else 2; col_weights = 0 makes w = 1):

    rfft3(x)  = w(kz) * rfftn(x, dim=(1,2,3), ortho)[:, :mx, :my, :mz]
    irfft3(S) = Re sum_{kx,ky,kz} w(kz) S[kx,ky,kz] e^{+2 pi i (kx x/X + ky y/Y + kz z/Z)} / sqrt(XYZ)

irfft3 with w is what torch.fft.irfftn(s=(X,Y,Z), ortho) returns for the zero-padded box also when S is not Hermitian on the
kz = 0 / Nyquist planes (the AFNO MLP's output is not); `afno3d_ref` is built on that sum and tests/test_cpu_dpot3d.py holds
it to the reference's recorded outputs and gradients.

Also here: the closed-form recipes of the fixture g17_dpot3d (weights and inputs are regenerated, not stored)."""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dpot_ref as R

TEMPORAL_MODES = 8


def modes3(dims, modes):
    X, Y, Z = dims
    return min(modes, X), min(modes, Y), min(TEMPORAL_MODES, Z // 2 + 1)


def z_weights(mz, Z, col_weights=1):
    w = torch.full((mz,), 2.0 if col_weights else 1.0, dtype=torch.float64)
    if col_weights:
        w[0] = 1.0
        if Z % 2 == 0 and Z // 2 < mz:
            w[Z // 2] = 1.0
    return w


def rfft3_def(x, m3, col_weights=0):
    """x [B, X, Y, Z, E] -> complex128 [B, mx, my, mz, E]"""
    x = x.double()
    mx, my, mz = m3
    S = torch.fft.rfftn(x, dim=(1, 2, 3), norm="ortho")[:, :mx, :my, :mz]
    return S * z_weights(mz, x.shape[3], col_weights).view(1, 1, 1, mz, 1)


def _expm(n, m):
    """complex128 [n, m]: e^{+2 pi i k j / n}, j < n, k < m"""
    j = torch.arange(n, dtype=torch.float64)[:, None]
    k = torch.arange(m, dtype=torch.float64)[None, :]
    a = 2.0 * math.pi * j * k / n
    return torch.complex(torch.cos(a), torch.sin(a))


def irfft3_def(S, dims, col_weights=1):
    """complex S [B, mx, my, mz, E] -> float64 [B, X, Y, Z, E]: the real-part sum above (dense, no FFT)"""
    X, Y, Z = dims
    S = S.to(torch.complex128)
    mx, my, mz = S.shape[1:4]
    Fz = _expm(Z, mz) * z_weights(mz, Z, col_weights).view(1, mz)
    y = torch.einsum("xa,yb,zc,nabce->nxyze", _expm(X, mx), _expm(Y, my), Fz, S)
    return y.real / math.sqrt(X * Y * Z)


def irfftn_padded(S, dims):
    """torch.fft.irfftn (float64, CPU) of the zero-padded box: equals irfft3_def(S, dims, 1)"""
    X, Y, Z = dims
    B, mx, my, mz, E = S.shape
    full = torch.zeros(B, X, Y, Z // 2 + 1, E, dtype=torch.complex128)
    full[:, :mx, :my, :mz] = S.to(torch.complex128)
    return torch.fft.irfftn(full, s=(X, Y, Z), dim=(1, 2, 3), norm="ortho")


def to_rows(S, nb):
    """complex [B, mx, my, mz, E] -> real [B*mx*my*mz, 2E], per channel block [re(bs) | im(bs)] (the kernels' layout)"""
    E = S.shape[-1]
    bs = E // nb
    Sb = S.reshape(-1, nb, bs)
    return torch.stack([Sb.real, Sb.imag], dim=2).reshape(-1, 2 * E)


def from_rows(rows, B, m3, E, nb):
    mx, my, mz = m3
    bs = E // nb
    r = rows.reshape(B, mx, my, mz, nb, 2, bs)
    return torch.complex(r[..., 0, :], r[..., 1, :]).reshape(B, mx, my, mz, E)


def afno3d_ref(x, w1, b1, w2, b2, nb, modes, act="gelu"):
    """AFNO3D.forward (models/dpot3d.py:46-97) on x [B, X, Y, Z, E], float64, differentiable"""
    x = x.double()
    w1, b1, w2, b2 = w1.double(), b1.double(), w2.double(), b2.double()
    B, X, Y, Z, E = x.shape
    bs = E // nb
    m3 = modes3((X, Y, Z), modes)
    f = R._act(act)
    S = rfft3_def(x, m3, 0).reshape(B, *m3, nb, bs)
    W1, W2 = torch.complex(w1[0], w1[1]), torch.complex(w2[0], w2[1])
    o1 = torch.einsum("...bi,bio->...bo", S, W1)
    o1 = torch.complex(f(o1.real + b1[0]), f(o1.imag + b1[1]))            # the activation acts on re and im separately
    o2 = torch.einsum("...bi,bio->...bo", o1, W2) + torch.complex(b2[0], b2[1])
    return irfft3_def(o2.reshape(B, *m3, E), (X, Y, Z), 1) + x


def group_norm_cl(x, weight, bias, groups=8, eps=1e-5):
    """GroupNorm of a channels-last field [B, ..., E]"""
    xc = x.movedim(-1, 1)
    return F.group_norm(xc, groups, weight, bias, eps).movedim(1, -1)


def block3d_ref(x, p, nb, modes, act="gelu"):
    """Block.forward (models/dpot3d.py:208-225, double_skip=False) on x [B, X, Y, Z, E]; p: the block's state dict"""
    p = {k: v.double() for k, v in p.items()}
    x = x.double()
    f = R._act(act)
    E = x.shape[-1]
    y = group_norm_cl(x, p["norm1.weight"], p["norm1.bias"])
    y = afno3d_ref(y, p["filter.w1"], p["filter.b1"], p["filter.w2"], p["filter.b2"], nb, modes, act)
    y = group_norm_cl(y, p["norm2.weight"], p["norm2.bias"])
    mh = p["mlp.0.weight"].shape[0]
    y = f(y @ p["mlp.0.weight"].reshape(mh, E).t() + p["mlp.0.bias"])
    y = y @ p["mlp.2.weight"].reshape(E, mh).t() + p["mlp.2.bias"]
    return y + x


def model3d_ref(sd, x, cfg):
    """DPOTNet3D.forward (models/dpot3d.py:354-390) in float64: torch CPU convolutions around block3d_ref"""
    sd = {k: v.double() for k, v in sd.items()}
    x = x.double()
    f = R._act(cfg.get("act", "gelu"))
    B, S, _, _, T, C = x.shape
    P, E = cfg["patch_size"], cfg["embed_dim"]
    if cfg.get("normalize", False):
        mu, sigma = x.mean(dim=(1, 2, 3, 4), keepdim=True), x.std(dim=(1, 2, 3, 4), keepdim=True) + 1e-6
        x = (x - mu) / sigma
        stat = torch.cat([mu, sigma], dim=-1)[:, 0, 0, 0, 0]
        s_mu = stat @ sd["scale_feats_mu.weight"].t() + sd["scale_feats_mu.bias"]
        s_sigma = stat @ sd["scale_feats_sigma.weight"].t() + sd["scale_feats_sigma.bias"]
    gs = torch.tensor(np.linspace(0, 1, S), dtype=torch.float32).double()
    gt = torch.tensor(np.linspace(0, 1, T), dtype=torch.float32).double()
    grid = torch.stack([gs.view(S, 1, 1, 1).expand(S, S, S, T), gs.view(1, S, 1, 1).expand(S, S, S, T),
                        gs.view(1, 1, S, 1).expand(S, S, S, T), gt.view(1, 1, 1, T).expand(S, S, S, T)], dim=-1)
    xg = torch.cat([x, grid.unsqueeze(0).expand(B, S, S, S, T, 4)], dim=-1)
    z = xg.permute(0, 4, 5, 1, 2, 3).reshape(B * T, C + 4, S, S, S)
    z = F.conv3d(z, sd["patch_embed.proj.0.weight"], sd["patch_embed.proj.0.bias"], stride=P)
    z = F.conv3d(f(z), sd["patch_embed.proj.2.weight"], sd["patch_embed.proj.2.bias"]) + sd["pos_embed"]
    h = S // P
    z = z.reshape(B, T, E, h, h, h).permute(0, 3, 4, 5, 1, 2)                   # b x y z t c
    w = sd["time_agg_layer.w"]
    if cfg.get("time_agg", "exp_mlp") == "exp_mlp":
        t = torch.linspace(0, 1, T).double().unsqueeze(-1)
        z = z * torch.cos(t @ sd["time_agg_layer.gamma"])
    lat = torch.einsum("tij,...ti->...j", w, z)
    if cfg.get("normalize", False):
        lat = s_sigma.view(B, 1, 1, 1, E) * lat + s_mu.view(B, 1, 1, 1, E)
    for i in range(cfg["depth"]):
        pre = f"blocks.{i}."
        lat = block3d_ref(lat, {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, cfg["n_blocks"],
                          cfg["modes"], cfg.get("act", "gelu"))
    y = lat.permute(0, 4, 1, 2, 3)
    y = f(F.conv_transpose3d(y, sd["out_layer.0.weight"], sd["out_layer.0.bias"], stride=P))
    y = f(F.conv3d(y, sd["out_layer.2.weight"], sd["out_layer.2.bias"]))
    y = F.conv3d(y, sd["out_layer.4.weight"], sd["out_layer.4.bias"]).permute(0, 2, 3, 4, 1)
    y = y.reshape(B, S, S, S, cfg["out_timesteps"], cfg["out_channels"])
    if cfg.get("normalize", False):
        y = y * sigma + mu
    return y


# ------------------------------------------------------------------------------------------------------
# fixture recipes (closed forms: identical wherever they are evaluated)
# ------------------------------------------------------------------------------------------------------
MINI3D = dict(img_size=8, patch_size=2, in_channels=2, out_channels=2, in_timesteps=3, out_timesteps=1, embed_dim=32,
              depth=2, n_blocks=4, mlp_ratio=2, out_layer_dim=16, modes=3)
MINI3D_NORM = dict(MINI3D, modes=32, normalize=True)
# the 2-D model whose checkpoint the 'step' case loads blocks and time_agg from (same width, depth, blocks, timesteps)
MINI2D = dict(img_size=16, patch_size=8, in_channels=2, out_channels=2, in_timesteps=3, out_timesteps=1, embed_dim=32,
              depth=2, n_blocks=4, mlp_ratio=2, out_layer_dim=16, modes=3, n_cls=5)
# name: (B, (X, Y, Z), E, nb, modes)
AFNO_CASES = {"A": (2, (4, 4, 4), 32, 4, 32), "B": (2, (6, 5, 4), 64, 2, 3), "C": (2, (4, 3, 16), 64, 1, 2)}
BLOCK_CASE = dict(B=2, dims=(4, 4, 4), E=32, nb=4, mlp_ratio=2, modes=32)
STEP = dict(lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=1e4, T_ar=2)


def recipe_sd(shapes, n_blocks, salt=0):
    """recipe weights for a state dict given as {name: shape}: the rules of oracle.dpot_ref.recipe_state_dict applied to any
    (2-D or 3-D) DPOT shape table"""
    E = shapes["pos_embed"][1]
    T = shapes["time_agg_layer.w"][0]
    bs = E // n_blocks
    sd = OrderedDict()
    for name, shape in shapes.items():
        shape = tuple(int(s) for s in shape)
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
            v = (u - 0.5) * 2.0 * math.sqrt(3.0) / (T * math.sqrt(E)) * 3.0
        elif name.endswith(".bias"):
            v = (u - 0.5) * 0.1
        else:
            fan = shape[0] if name.startswith("out_layer.0.weight") else int(np.prod(shape[1:])) if len(shape) >= 2 else 1
            v = (u - 0.5) * 2.0 * math.sqrt(3.0 / fan)
        sd[name] = v.to(torch.float32).contiguous()
    return sd


def afno_recipe(E, nb, salt):
    """(w1, b1, w2, b2) of one AFNO3D filter"""
    bs = E // nb
    out = []
    for name, shape in (("filter.w1", (2, nb, bs, bs)), ("filter.b1", (2, nb, bs)), ("filter.w2", (2, nb, bs, bs)),
                        ("filter.b2", (2, nb, bs))):
        out.append(((R.recipe_tensor(name, shape, salt) - 0.5) * (2.0 / math.sqrt(bs))).to(torch.float32))
    return out


def block_shapes(E, nb, mh):
    bs = E // nb
    return OrderedDict([("norm1.weight", (E,)), ("norm1.bias", (E,)), ("filter.w1", (2, nb, bs, bs)),
                        ("filter.b1", (2, nb, bs)), ("filter.w2", (2, nb, bs, bs)), ("filter.b2", (2, nb, bs)),
                        ("norm2.weight", (E,)), ("norm2.bias", (E,)), ("mlp.0.weight", (mh, E, 1, 1, 1)),
                        ("mlp.0.bias", (mh,)), ("mlp.2.weight", (E, mh, 1, 1, 1)), ("mlp.2.bias", (E,))])


def block_recipe(E, nb, mh, salt):
    shapes = OrderedDict([("pos_embed", (1, E)), ("time_agg_layer.w", (1, E, E))])
    shapes.update(("blocks.0." + k, v) for k, v in block_shapes(E, nb, mh).items())
    sd = recipe_sd(shapes, nb, salt)
    return OrderedDict((k[len("blocks.0."):], v) for k, v in sd.items() if k.startswith("blocks.0."))


def recipe_mask(shape, salt):
    """a 0/1 mask with both values present"""
    return (R.recipe_tensor("mask", shape, salt) > 0.25).to(torch.float32)


def sub_record(t, stride):
    """what tests/helpers.assert_sub reads: a strided subsample and two checksums"""
    f = t.detach().reshape(-1)
    return {".sub": f[::stride].numpy().copy(), ".stride": np.int64(stride), ".sum": np.float64(f.double().sum().item()),
            ".abssum": np.float64(f.double().abs().sum().item())}
