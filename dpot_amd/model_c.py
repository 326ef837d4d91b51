"""CDPOTNet for MI355X: the reference's second 2-D model (models/dpot_res.py:393-586), the one its varying-resolution
evaluation is written for.

Same constructor signature and defaults, same ``state_dict`` keys / shapes / order (``patch_embed.proj.1`` IS
``patch_embed.act_patching``: one module registered twice, so ``state_dict()`` has one entry more than ``named_parameters()``
and the reference's checkpoints load with ``strict=True``), same call contract as DPOTNet

    pred, cls_pred = model(x)          # x: [B, X, Y, T_in, C_in]  ->  [B, X, Y, T_out, C_out], [B, n_cls]

It differs from DPOTNet in two places, both the anti-aliased activation of csrc/aa_act.hip (functional.AALReLUFn: bilinear up
by 2, LeakyReLU(0.01), anti-aliased bilinear down by 2, optionally bilinear up to the image size, + a per-channel bias):

  patch embedding  Conv2d(k = s = P) with NO activation -> the operator at the latent size -> 1x1 conv (+ pos_embed)
  output layer     1x1 conv E -> out_layer_dim at the LATENT size -> the operator with output size img_size -> 1x1 conv, act,
                   1x1 conv at full resolution.  There is no transposed convolution.  The reference's CNOBlock first runs a
                   frequency filter with K = conv_kernel = 1, which keeps every frequency - the identity (its fp32 round trip
                   moves the input by 2.4e-7) - so it is implemented as nothing.

Everything else is the 2-D model's: grid channels, time aggregation, AdaIN (normalize=True), the Blocks through the unchanged
functional.BlockFn with the AFNO pack table of packs.ModelPacks.afno, cls_head on the token mean.  The drop
arguments are accepted and change nothing, as in the reference, whose forward never uses them.  The torch modules below are
parameter containers only.  CUDA (ROCm) tensors only; there is no CPU path.

Not here (see README): bf16 channel-MLP packs and Adam-written packs, recompute_blocks, SegmentedTrainStep / make_dp_step,
the one-launch embed and de-embed fusions of DPOTNet.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .functional import AALReLUFn, AdaINFn, BlockFn, ClsHeadFn, LinearFn, Mlp2Fn, PatchConvFn, TimeAggFn, TokenMeanFn
from .model import _BlockParams, _DPOTBase

AA_SLOPE = 0.01          # nn.LeakyReLU()'s default - not the 0.1 of the model's 'leaky_relu' activation


class _AAActParams(nn.Module):
    """LReLu_torch: its one parameter"""

    def __init__(self, channels: int):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(channels))


class _CNOPatchEmbedParams(nn.Module):
    def __init__(self, img_size: int, patch_size: int, in_chans: int, hidden: int, out_dim: int):
        super().__init__()
        self.img_size = (img_size, img_size)
        self.patch_size = (patch_size, patch_size)
        self.out_size = (img_size // patch_size, img_size // patch_size)
        self.num_patches = self.out_size[0] * self.out_size[1]
        self.out_dim = out_dim
        self.act_patching = _AAActParams(hidden)
        self.proj = nn.Sequential(nn.Conv2d(in_chans, hidden, patch_size, patch_size), self.act_patching,
                                  nn.Conv2d(hidden, out_dim, 1))


class _CNOBlockParams(nn.Module):
    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.convolution = nn.Conv2d(in_channels, out_channels, 1)
        self.activation = _AAActParams(out_channels)


class CDPOTNet(_DPOTBase):
    def __init__(self, img_size=224, patch_size=16, mixing_type='afno', in_channels=1, out_channels=3, in_timesteps=1,
                 out_timesteps=1, n_blocks=4, embed_dim=768, out_layer_dim=32, depth=12, modes=32, mlp_ratio=1.,
                 representation_size=None, uniform_drop=False, drop_rate=0., drop_path_rate=0., dropcls=0, n_cls=1,
                 normalize=False, act='gelu', time_agg='exp_mlp'):
        super().__init__(
            img_size, patch_size, mixing_type, in_channels, out_channels, in_timesteps, out_timesteps, n_blocks, embed_dim,
            out_layer_dim, depth, modes, mlp_ratio, n_cls, normalize, act, time_agg,
            patch_embed=lambda: _CNOPatchEmbedParams(img_size, patch_size, in_channels + 3, out_channels * patch_size + 3, embed_dim),
            block=lambda: _BlockParams(embed_dim, n_blocks, mlp_ratio),
            out_layer=lambda: nn.Sequential(_CNOBlockParams(embed_dim, out_layer_dim), nn.Conv2d(out_layer_dim, out_layer_dim, 1),
                                            nn.Identity(), nn.Conv2d(out_layer_dim, out_channels * out_timesteps, 1)))

    def _forward(self, x):
        self._check_device(x)
        B, X, Y, T, Cin = x.shape
        S, P, h, E = self.img_size, self.patch_size, self.latent_size[0], self.embed_dim
        assert X == S and Y == S, f"Input image size ({X}*{Y}) doesn't match model ({S}*{S})."
        assert T == self.in_timesteps and Cin == self.in_channels, "input timesteps / channels mismatch"
        x, mu, sigma, s_mu, s_sigma = self._normalize_in(x.float(), (1, 2, 3))

        # patch embedding: rows (b, hx, hy, t) throughout, so the field [B, h, h, T*hid] of the operator (bias[c % hid]) and the
        # rows (b, token) x columns (t, e) of the time aggregation are views
        tok = h * h
        pe, ta = self.patch_embed.proj, self.time_agg_layer
        hid = pe[0].weight.shape[0]
        hpre = PatchConvFn.apply(x, self._gx, self._gy, self._gt, pe[0].weight.view(hid, -1), pe[0].bias, P)
        hact = AALReLUFn.apply(hpre.view(B, h, h, T * hid), self.patch_embed.act_patching.bias, None, AA_SLOPE)
        posT = self.pos_embed.view(E, tok).t()                                  # [tok, E]
        z = LinearFn.apply(hact.view(B * tok * T, hid), pe[2].weight.view(E, hid), pe[2].bias, posT, T, tok)
        lat = TimeAggFn.apply(z.view(B * tok, T * E), ta.w, self._time_agg_gamma(), self._tt).view(B, tok, E)
        if self.normalize:
            lat = AdaINFn.apply(lat, s_sigma, s_mu)                             # AdaIN (models/dpot_res.py:563-564)

        pk = self.packs.afno(self).refresh()
        grad = torch.is_grad_enabled()
        for i, blk in enumerate(self.blocks):
            f = blk.filter
            lat = BlockFn.apply(lat, blk.norm1.weight, blk.norm1.bias, f.w1, f.b1, f.w2, f.b2, blk.norm2.weight,
                                blk.norm2.bias, blk.mlp[0].weight, blk.mlp[0].bias, blk.mlp[2].weight, blk.mlp[2].bias,
                                h, h, self.n_blocks, self.modes, self._act, (pk[2 * i], pk[2 * i + 1]), False, None, grad,
                                False, None)

        ch = self.cls_head
        cls_pred = ClsHeadFn.apply(TokenMeanFn.apply(lat), ch[0].weight, ch[0].bias, ch[2].weight, ch[2].bias, ch[4].weight,
                                   ch[4].bias, self._act)

        ol = self.out_layer
        old, Co = self.out_layer_dim, self.out_channels * self.out_timesteps
        u = LinearFn.apply(lat.view(B * tok, E), ol[0].convolution.weight.view(old, E), ol[0].convolution.bias)
        u = AALReLUFn.apply(u.view(B, h, h, old), ol[0].activation.bias, (S, S), AA_SLOPE)
        pred = Mlp2Fn.apply(u.view(B * S * S, old), ol[1].weight.view(old, old), ol[1].bias, ol[3].weight.view(Co, old),
                            ol[3].bias, self._act)
        pred = pred.view(B, X, Y, self.out_timesteps, self.out_channels)
        return self._denormalize(pred, mu, sigma), cls_pred
