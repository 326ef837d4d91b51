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

import numpy as np

import torch
import torch.nn as nn

from . import _lib, ops
from .functional import AdaINFn, Head3DFn, PatchEmbed3DFn, TimeAggFn, block3d
from .model import ACTIVATIONS, _AFNOParams, _TimeAggParams

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


class DPOTNet3D(nn.Module):
    cls_output = False          # forward returns the prediction alone (train.rollout: no classification branch)

    def __init__(self, img_size=224, patch_size=16, mixing_type='afno', in_channels=1, out_channels=3, in_timesteps=1,
                 out_timesteps=1, n_blocks=4, embed_dim=768, out_layer_dim=32, depth=12, modes=32, mlp_ratio=1.,
                 n_cls=1, normalize=False, act='gelu', time_agg='exp_mlp'):
        super().__init__()
        if act not in ACTIVATIONS:
            raise KeyError(act)
        if mixing_type != 'afno':
            raise ValueError("only mixing_type='afno' exists in the reference")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.in_timesteps, self.out_timesteps = in_timesteps, out_timesteps
        self.n_blocks, self.modes = n_blocks, modes
        self.num_features = self.embed_dim = embed_dim
        self.mlp_ratio = mlp_ratio
        self.normalize, self.time_agg, self.n_cls = normalize, time_agg, n_cls
        self.mixing_type = mixing_type
        self.img_size, self.patch_size = img_size, patch_size
        self.out_layer_dim = out_layer_dim
        self.act_name, self._act = act, ops.ACT_IDS[act]

        self.patch_embed = _PatchEmbed3DParams(img_size, patch_size, in_channels + 4, out_channels * patch_size + 4,
                                               embed_dim)
        self.latent_size = self.patch_embed.out_size
        h = self.latent_size[0]
        self.pos_embed = nn.Parameter(torch.zeros(1, embed_dim, h, h, h))
        self.blocks = nn.ModuleList([_Block3DParams(embed_dim, n_blocks, mlp_ratio) for _ in range(depth)])
        if normalize:
            self.scale_feats_mu = nn.Linear(2 * in_channels, embed_dim)
            self.scale_feats_sigma = nn.Linear(2 * in_channels, embed_dim)
        # constructed, never called (models/dpot3d.py:288-294): it keeps the reference's state_dict and gets no gradient
        self.cls_head = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.Identity(), nn.Linear(embed_dim, embed_dim),
                                      nn.Identity(), nn.Linear(embed_dim, n_cls))
        self.time_agg_layer = _TimeAggParams(in_timesteps, embed_dim, time_agg)
        self.out_layer = nn.Sequential(
            nn.ConvTranspose3d(embed_dim, out_layer_dim, patch_size, patch_size), nn.Identity(),
            nn.Conv3d(out_layer_dim, out_layer_dim, 1), nn.Identity(),
            nn.Conv3d(out_layer_dim, out_channels * out_timesteps, 1))
        torch.nn.init.trunc_normal_(self.pos_embed, std=.02)

        # coordinate tables of get_grid_4d (models/dpot3d.py:338-350: np.linspace in float64, then cast)
        for name, n in (("_gs", img_size), ("_gt", in_timesteps)):
            self.register_buffer(name, torch.tensor(np.linspace(0, 1, n), dtype=torch.float32), persistent=False)
        self.register_buffer("_tt", torch.linspace(0, 1, in_timesteps), persistent=False)
        self.gemm_precision = None          # as DPOTNet: None = the process default
        self._packs = None                  # (key, ops.AfnoPacks): the packed AFNO weights, persistent buffers
        self._checked = False

    # ------------------------------------------------------------------------------------------------
    def _afno_packs(self):
        """packed forms of every block's complex weights: persistent buffers re-filled by ONE launch per forward (so a
        captured forward replays the refresh with the weights of the day); rebuilt when the parameters move"""
        pairs = []
        for blk in self.blocks:
            f = blk.filter
            pairs += [(f.w1, f.b1), (f.w2, f.b2)]
        key = tuple(p.data_ptr() for pr in pairs for p in pr)
        if self._packs is None or self._packs[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.DpotHipError("DPOTNet3D: run one forward before capturing (the weight-pack tables are built by it)")
            self._packs = (key, ops.AfnoPacks(pairs))
        return self._packs[1].refresh()

    def _check_grid(self):
        h = self.latent_size[0]
        dims3 = (h, h, h)
        m3 = ops.kept_modes3(dims3, self.modes, TEMPORAL_MODES)
        if not ops.dft3_supported(dims3, self.embed_dim, m3):
            raise ValueError(f"DPOTNet3D: the latent grid {h}x{h}x{h} (img_size {self.img_size} / patch_size {self.patch_size}, "
                             f"kept modes {m3[0]}x{m3[1]}x{m3[2]}, {self.embed_dim} channels) is not supported by the 3-D "
                             "transform kernels: one sample's channel slab does not fit the LDS")
        self._checked = True

    def forward(self, x):
        with ops.precision_scope(self.gemm_precision, None):
            return self._forward(x)

    def _forward(self, x):
        if not x.is_cuda:
            raise _lib.DpotHipError("DPOTNet3D (dpot_amd) runs on MI355X only: move the model and the input to 'cuda'. "
                                    "There is no CPU fallback.")
        B, X, Y, Z, T, Cin = x.shape
        S, P, h, E = self.img_size, self.patch_size, self.latent_size[0], self.embed_dim
        assert X == S and Y == S and Z == S, f"Input image size ({X}*{Y}*{Z}) doesn't match model ({S}*{S}*{S})."
        assert T == self.in_timesteps and Cin == self.in_channels, "input timesteps / channels mismatch"
        if not self._checked:
            self._check_grid()
        x = x.float()
        if self.normalize:
            # models/dpot3d.py:356-360 - per-sample statistics + two tiny Linear(2C -> E): O(B*C) glue
            mu = x.mean(dim=(1, 2, 3, 4), keepdim=True)
            sigma = x.std(dim=(1, 2, 3, 4), keepdim=True) + 1e-6
            x = (x - mu) / sigma
            stat = torch.cat([mu, sigma], dim=-1)[:, 0, 0, 0, 0, :]
            s_mu = self.scale_feats_mu(stat)
            s_sigma = self.scale_feats_sigma(stat)

        # patches with the four coordinate channels x, y, z, t: rows ((b, t), hx, hy, hz), columns (c, i, j, k) (ops.patchify3)
        Cc = Cin + 4
        tok = h * h * h
        pe, ta = self.patch_embed.proj, self.time_agg_layer
        hid = pe[0].weight.shape[0]
        posT = self.pos_embed.view(E, tok).t()                                  # [tok, E]
        z = PatchEmbed3DFn.apply(x, self._gs, self._gt, pe[0].weight.view(hid, Cc * P ** 3), pe[0].bias,
                                 pe[2].weight.view(E, hid), pe[2].bias, posT, P, self._act)  # conv, act, 1x1 conv, + pos_embed
        A1 = z.view(B, T, tok, E).permute(0, 2, 1, 3).reshape(B * tok, T * E)   # rows (b, token), columns (t, channel)
        lat = TimeAggFn.apply(A1, ta.w, ta.gamma if self.time_agg == "exp_mlp" else None, self._tt).view(B, tok, E)
        if self.normalize:
            lat = AdaINFn.apply(lat, s_sigma, s_mu)                             # AdaIN (models/dpot3d.py:378)

        pk = self._afno_packs()
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
        if self.normalize:
            pred = pred * sigma + mu
        return pred

    def extra_repr(self) -> str:
        return (f"img_size={self.img_size}, patch_size={self.patch_size}, embed_dim={self.embed_dim}, "
                f"depth={len(self.blocks)}, n_blocks={self.n_blocks}, modes={self.modes}, act={self.act_name}, "
                f"backend=libdpot_hip(gfx950)")
