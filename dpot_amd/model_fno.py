"""FNO2d for MI355X: the baseline every table of the DPOT paper is read against (the reference's models/fno.py:85-283), the
third 2-D choice of its entry scripts' ``--model`` switch.

Same constructor signature and defaults, same ``state_dict`` keys / shapes / order, same call contract

    pred, cls_pred = model(x)          # x: [B, X, Y, T_in, C]  ->  [B, X/P, Y/P, T_out, C], [B, n_cls]

  normalize        per-sample mean and std (+ 1e-6) over (X, Y, T); ONE scale_feats = Linear(2C, width) of cat(mu, sigma) is
                   added after the patch embedding (not DPOT's two AdaIN layers); the prediction is de-normalised
  patch embedding  the T * C planes + the (x, y) unit grid -> Conv2d(k = s = P) -> GELU -> Conv2d 1x1 (functional.FNOEmbedFn)
  layers           n_layers times gelu(SpectralConv2d_fast(x) + Conv2d 1x1(x)) (functional.FNOLayerFn, csrc/fno.hip), then
                   GroupNorm(4, width) if use_ln.  GELU follows every layer, the last included.
  head             cls_head on the mean over space (an empty [B, 0] when n_cls = 0); fc1, GELU, fc2 at the LATENT size: with
                   P > 1 the prediction lives on the X/P x Y/P grid, as in the reference, and cannot feed a rollout.

The activation is always the exact-erf GELU; ``multi_channel`` is accepted and unused, as in the reference.  Narrower than
the reference in two places, both a ValueError that names the sizes: 2 * modes1 <= X/P (the reference lets weights2 silently
overwrite the rows it shares with weights1) and modes2 <= (Y/P) // 2 + 1 (the reference raises inside its slice assignment).
The spectral weights are read in place by the kernels: the model owns no derived copy (no ``packs``).  The torch modules are
parameter containers only.  CUDA (ROCm) tensors only; there is no CPU path.

Not here (see README): SegmentedTrainStep / make_dp_step (they read ``model.blocks``), bf16 modes for the FNO layers.
"""
from __future__ import annotations

import numpy as np

import torch
import torch.nn as nn

from . import ops
from .model import _ModelBase
from .functional import ClsHeadFn, FNOEmbedFn, FNOLayerFn, GroupNormFn, Mlp2Fn, TokenMeanFn

GELU = ops.ACT_IDS["gelu"]


class _SpectralConvParams(nn.Module):
    """weights of SpectralConv2d_fast (models/fno.py:27-29): real [2, Cin, Cout, m1, m2], the mode index innermost"""

    def __init__(self, in_channels: int, out_channels: int, modes1: int, modes2: int):
        super().__init__()
        self.in_channels, self.out_channels, self.modes1, self.modes2 = in_channels, out_channels, modes1, modes2
        self.scale = 1 / (in_channels * out_channels)
        self.weights1 = nn.Parameter(self.scale * torch.rand(2, in_channels, out_channels, modes1, modes2))
        self.weights2 = nn.Parameter(self.scale * torch.rand(2, in_channels, out_channels, modes1, modes2))


class _FNOPatchEmbedParams(nn.Module):
    def __init__(self, img_size: int, patch_size: int, in_chans: int, hidden: int, out_dim: int):
        super().__init__()
        self.img_size = (img_size, img_size)
        self.patch_size = (patch_size, patch_size)
        self.out_size = (img_size // patch_size, img_size // patch_size)
        self.num_patches = self.out_size[0] * self.out_size[1]
        self.out_dim = out_dim
        self.proj = nn.Sequential(nn.Conv2d(in_chans, hidden, patch_size, patch_size), nn.Identity(),
                                  nn.Conv2d(hidden, out_dim, 1))


class FNO2d(_ModelBase):
    cls_output = True

    def __init__(self, modes1, modes2, width, img_size=64, n_channels=1, in_timesteps=10, out_timesteps=1, n_layers=4,
                 patch_size=1, use_ln=False, multi_channel=True, normalize=False, n_cls=0):
        super().__init__()
        h = img_size // patch_size
        ops.fno_check_modes(h, h, modes1, modes2, f"FNO2d (img_size {img_size}, patch_size {patch_size}: a {h}x{h} field)")
        self.modes1, self.modes2, self.width, self.n_layers = modes1, modes2, width, n_layers
        self.n_channels, self.in_timesteps, self.out_timesteps = n_channels, in_timesteps, out_timesteps
        self.img_size, self.use_ln, self.padding, self.patch_size = img_size, use_ln, 2, patch_size
        self.normalize, self.n_cls = normalize, n_cls
        self.latent_size = (h, h)

        K = n_channels * in_timesteps
        self.patch_embed = _FNOPatchEmbedParams(img_size, patch_size, K + 2, K * patch_size + 2, width)
        self.spectral_convs = nn.ModuleList([_SpectralConvParams(width, width, modes1, modes2) for _ in range(n_layers)])
        self.convs = nn.ModuleList([nn.Conv2d(width, width, 1) for _ in range(n_layers)])
        if normalize:
            self.scale_feats = nn.Linear(2 * n_channels, width)
        if use_ln:
            self.ln_layers = nn.ModuleList([nn.GroupNorm(4, width) for _ in range(n_layers)])
        self.fc1 = nn.Linear(width, width)
        self.fc2 = nn.Linear(width, n_channels * out_timesteps)
        self.cls_head = nn.Sequential(nn.Linear(width, width), nn.Identity(), nn.Linear(width, width), nn.Identity(),
                                      nn.Linear(width, n_cls))

        # get_grid (models/fno.py:276-283): np.linspace in float64, then cast; the third table feeds the coordinate channel
        # ops.patchify appends beyond FNO2d's two - its weights are zero (FNOEmbedFn)
        for name, n in (("_gx", img_size), ("_gy", img_size)):
            self.register_buffer(name, torch.tensor(np.linspace(0, 1, n), dtype=torch.float32), persistent=False)
        self.register_buffer("_gt", torch.zeros(1), persistent=False)

    def _forward(self, x):
        self._check_device(x)
        B, X, Y, T, C = x.shape
        S, P, (h, w), Wd = self.img_size, self.patch_size, self.latent_size, self.width
        assert X == S and Y == S, f"Input image size ({X}*{Y}) doesn't match model ({S}*{S})."
        assert T == self.in_timesteps and C == self.n_channels, "input timesteps / channels mismatch"
        x = x.float()
        mu = sigma = sf = None
        if self.normalize:               # per-sample statistics + one tiny Linear(2C -> width): O(B * C) glue, as DPOTNet's
            mu = x.mean(dim=(1, 2, 3), keepdim=True)
            sigma = x.std(dim=(1, 2, 3), keepdim=True) + 1e-6
            x = (x - mu) / sigma
            sf = self.scale_feats(torch.cat([mu, sigma], dim=-1)[:, 0, 0, 0])                    # [B, width]

        pe = self.patch_embed.proj
        hid = pe[0].weight.shape[0]
        w0 = torch.cat([pe[0].weight, pe[0].weight.new_zeros(hid, 1, P, P)], dim=1).view(hid, -1)
        z = FNOEmbedFn.apply(x.reshape(B, X, Y, 1, T * C), self._gx, self._gy, self._gt, w0, pe[0].bias,
                             pe[2].weight.view(Wd, hid), pe[2].bias, sf, P, GELU).view(B, h, w, Wd)

        for i in range(self.n_layers):
            sc, cv = self.spectral_convs[i], self.convs[i]
            z = FNOLayerFn.apply(z, sc.weights1, sc.weights2, cv.weight.view(Wd, Wd), cv.bias, GELU)
            if self.use_ln:
                ln = self.ln_layers[i]
                z = GroupNormFn.apply(z.view(B, h * w, Wd), ln.weight, ln.bias, 4).view(B, h, w, Wd)

        ch = self.cls_head
        if self.n_cls > 0:
            cls_pred = ClsHeadFn.apply(TokenMeanFn.apply(z.view(B, h * w, Wd)), ch[0].weight, ch[0].bias, ch[2].weight,
                                       ch[2].bias, ch[4].weight, ch[4].bias, GELU)
        else:
            cls_pred = z.new_zeros(B, 0)
        pred = Mlp2Fn.apply(z.view(B * h * w, Wd), self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, GELU)
        pred = pred.view(B, h, w, self.out_timesteps, C)
        if self.normalize:
            pred = pred * sigma + mu
        return pred, cls_pred

    def extra_repr(self) -> str:
        return (f"img_size={self.img_size}, patch_size={self.patch_size}, width={self.width}, n_layers={self.n_layers}, "
                f"modes=({self.modes1}, {self.modes2}), backend=libdpot_hip(gfx950)")
