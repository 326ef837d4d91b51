"""DPOTNet3D for MI355X: the reference's 3-D fine-tuning model (models/dpot3d.py:228-390).

Same constructor signature and defaults, same ``state_dict`` keys / shapes / order, same call contract

    pred = model(x)          # x: [B, X, Y, Z, T_in, C_in]  ->  [B, X, Y, Z, T_out, C_out]   (one tensor, no cls output)

so ``blocks`` and ``time_agg_layer`` take a pretrained 2-D checkpoint's weights (infer.load_3d_components_from_2d).  The torch
modules below (Conv3d, ConvTranspose3d, GroupNorm, Linear) are parameter containers only; their forward() is never called.

The hot path is the block stack: depth x [GroupNorm -> AFNO3D -> GroupNorm -> channel MLP] on the kernels of csrc/dft3.hip, the
mixer kernels of the 2-D model and the project's GEMMs (functional.block3d).  Patch embedding and the output layer are
k = s = P convolutions: the index rearrangements of csrc/patch3d.hip (ops.patchify3 / unpatchify3 / fold3) around the same
GEMMs (functional.PatchEmbed3DFn / TimeAggFn / Head3DFn).
CUDA (ROCm) tensors only; there is no CPU path.
"""
from __future__ import annotations

import torch.nn as nn

from . import ops
from .functional import AdaINFn, Head3DFn, PatchEmbed3DFn, TimeAggFn, block3d
from .model import _AFNOParams, _DPOTBase

TEMPORAL_MODES = 8          # Block builds AFNO3D without temporal_modes (models/dpot3d.py:191): always the default


class _Block3DParams(nn.Module):
    def __init__(self, width: int, n_blocks: int, mlp_ratio: float):
        super().__init__()
        self.norm1 = nn.GroupNorm(8, width)
        self.filter = _AFNOParams(width, n_blocks)
        self.norm2 = nn.GroupNorm(8, width)
        hidden = int(width * mlp_ratio)
        self.mlp = nn.Sequential(nn.Conv3d(width, hidden, 1), nn.Identity(), nn.Conv3d(hidden, width, 1))


class _PatchEmbed3DParams(nn.Module):
    def __init__(self, img_size: int, patch_size: int, in_chans: int, hidden: int, out_dim: int):
        super().__init__()
        self.img_size = (img_size,) * 3
        self.patch_size = (patch_size,) * 3
        self.out_size = (img_size // patch_size,) * 3
        self.num_patches = self.out_size[0] ** 3
        self.proj = nn.Sequential(nn.Conv3d(in_chans, hidden, patch_size, patch_size), nn.Identity(),
                                  nn.Conv3d(hidden, out_dim, 1))


class DPOTNet3D(_DPOTBase):
    cls_output = False          # forward returns the prediction alone (train.rollout: no classification branch)

    def __init__(self, img_size=224, patch_size=16, mixing_type='afno', in_channels=1, out_channels=3, in_timesteps=1,
                 out_timesteps=1, n_blocks=4, embed_dim=768, out_layer_dim=32, depth=12, modes=32, mlp_ratio=1.,
                 n_cls=1, normalize=False, act='gelu', time_agg='exp_mlp'):
        super().__init__(
            img_size, patch_size, mixing_type, in_channels, out_channels, in_timesteps, out_timesteps, n_blocks, embed_dim,
            out_layer_dim, depth, modes, mlp_ratio, n_cls, normalize, act, time_agg, coords=("_gs",),
            patch_embed=lambda: _PatchEmbed3DParams(img_size, patch_size, in_channels + 4, out_channels * patch_size + 4, embed_dim),
            block=lambda: _Block3DParams(embed_dim, n_blocks, mlp_ratio),
            out_layer=lambda: nn.Sequential(
                nn.ConvTranspose3d(embed_dim, out_layer_dim, patch_size, patch_size), nn.Identity(),
                nn.Conv3d(out_layer_dim, out_layer_dim, 1), nn.Identity(),
                nn.Conv3d(out_layer_dim, out_channels * out_timesteps, 1)))
        self._checked = False

    def _check_grid(self):
        h = self.latent_size[0]
        dims3 = (h, h, h)
        m3 = ops.kept_modes3(dims3, self.modes, TEMPORAL_MODES)
        if not ops.dft3_supported(dims3, self.embed_dim, m3):
            raise ValueError(f"DPOTNet3D: the latent grid {h}x{h}x{h} (img_size {self.img_size} / patch_size {self.patch_size}, "
                             f"kept modes {m3[0]}x{m3[1]}x{m3[2]}, {self.embed_dim} channels) is not supported by the 3-D "
                             "transform kernels: one sample's channel slab does not fit the LDS")
        self._checked = True

    def _forward(self, x):
        self._check_device(x)
        B, X, Y, Z, T, Cin = x.shape
        S, P, h, E = self.img_size, self.patch_size, self.latent_size[0], self.embed_dim
        assert X == S and Y == S and Z == S, f"Input image size ({X}*{Y}*{Z}) doesn't match model ({S}*{S}*{S})."
        assert T == self.in_timesteps and Cin == self.in_channels, "input timesteps / channels mismatch"
        if not self._checked:
            self._check_grid()
        x, mu, sigma, s_mu, s_sigma = self._normalize_in(x.float(), (1, 2, 3, 4))

        # patches with the four coordinate channels x, y, z, t: rows ((b, t), hx, hy, hz), columns (c, i, j, k) (ops.patchify3)
        Cc = Cin + 4
        tok = h * h * h
        pe, ta = self.patch_embed.proj, self.time_agg_layer
        hid = pe[0].weight.shape[0]
        posT = self.pos_embed.view(E, tok).t()                                  # [tok, E]
        z = PatchEmbed3DFn.apply(x, self._gs, self._gt, pe[0].weight.view(hid, Cc * P ** 3), pe[0].bias,
                                 pe[2].weight.view(E, hid), pe[2].bias, posT, P, self._act)  # conv, act, 1x1 conv, + pos_embed
        A1 = z.view(B, T, tok, E).permute(0, 2, 1, 3).reshape(B * tok, T * E)   # rows (b, token), columns (t, channel)
        lat = TimeAggFn.apply(A1, ta.w, self._time_agg_gamma(), self._tt).view(B, tok, E)
        if self.normalize:
            lat = AdaINFn.apply(lat, s_sigma, s_mu)                             # AdaIN (models/dpot3d.py:378)

        pk = self.packs.afno(self).refresh()
        for i, blk in enumerate(self.blocks):
            f = blk.filter
            lat = block3d(lat, blk.norm1.weight, blk.norm1.bias, f.w1, f.b1, f.w2, f.b2, blk.norm2.weight, blk.norm2.bias,
                          blk.mlp[0].weight, blk.mlp[0].bias, blk.mlp[2].weight, blk.mlp[2].bias, (h, h, h), self.n_blocks,
                          self.modes, self._act, (pk[2 * i], pk[2 * i + 1]))

        ol = self.out_layer
        old, Co = self.out_layer_dim, self.out_channels * self.out_timesteps
        pred = Head3DFn.apply(lat.view(B * tok, E), ol[0].weight.view(E, old * P ** 3),
                              ol[0].bias.view(old, 1).expand(old, P ** 3).reshape(-1), ol[2].weight.view(old, old), ol[2].bias,
                              ol[4].weight.view(Co, old), ol[4].bias, B, h, P, self._act)
        pred = pred.view(B, X, Y, Z, self.out_timesteps, self.out_channels)
        return self._denormalize(pred, mu, sigma)
