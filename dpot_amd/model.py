"""DPOTNet for MI355X.

Drop-in for the reference model class (models/dpot.py:245-403): identical constructor signature, identical
``state_dict`` keys / shapes / ordering (so pretrained ``.pth`` files load unchanged, also through
utils/utilities.py:99-166 style per-component loading) and the same call contract

    pred, cls_pred = model(x)          # x: [B, X, Y, T_in, C_in]  ->  [B, X, Y, T_out, C_out], [B, n_cls]

but the compute is the hand-written HIP path in libdpot_hip.so (functional.py / ops.py).  The torch modules
below (Conv2d, GroupNorm, Linear, ...) are used purely as *parameter containers* - they own the weights with the
reference's names and default initialisation; their own forward() is never called.

The model only runs on a CUDA (ROCm) device; calling it with CPU tensors raises - there is no fallback path.
"""
from __future__ import annotations

import numpy as np

import torch
import torch.nn as nn

from . import _lib, ops
import contextlib

from .functional import AdaINFn, BlockFn, EmbedFn, HeadFn, WgradBatch
from .packs import ModelPacks

ACTIVATIONS = ("gelu", "tanh", "sigmoid", "relu", "leaky_relu", "softplus", "ELU", "silu")


class _AFNOParams(nn.Module):
    """weights of the block-diagonal complex MLP shared by all Fourier modes (models/dpot.py:41-48)"""

    def __init__(self, width: int, num_blocks: int):
        super().__init__()
        assert width % num_blocks == 0, f"hidden_size {width} should be divisble by num_blocks {num_blocks}"
        bs = width // num_blocks
        scale = 1.0 / (bs * bs)
        self.w1 = nn.Parameter(scale * torch.rand(2, num_blocks, bs, bs))
        self.b1 = nn.Parameter(scale * torch.rand(2, num_blocks, bs))
        self.w2 = nn.Parameter(scale * torch.rand(2, num_blocks, bs, bs))
        self.b2 = nn.Parameter(scale * torch.rand(2, num_blocks, bs))


class _BlockParams(nn.Module):
    def __init__(self, width: int, n_blocks: int, mlp_ratio: float):
        super().__init__()
        self.norm1 = nn.GroupNorm(8, width)
        self.filter = _AFNOParams(width, n_blocks)
        self.norm2 = nn.GroupNorm(8, width)
        hidden = int(width * mlp_ratio)
        self.mlp = nn.Sequential(nn.Conv2d(width, hidden, 1), nn.Identity(), nn.Conv2d(hidden, width, 1))


class _PatchEmbedParams(nn.Module):
    def __init__(self, img_size: int, patch_size: int, in_chans: int, hidden: int, out_dim: int):
        super().__init__()
        self.img_size = (img_size, img_size)
        self.patch_size = (patch_size, patch_size)
        self.out_size = (img_size // patch_size, img_size // patch_size)
        self.num_patches = self.out_size[0] * self.out_size[1]
        self.proj = nn.Sequential(nn.Conv2d(in_chans, hidden, patch_size, patch_size), nn.Identity(),
                                  nn.Conv2d(hidden, out_dim, 1))


class _TimeAggParams(nn.Module):
    def __init__(self, n_timesteps: int, width: int, kind: str):
        super().__init__()
        self.type = kind
        self.w = nn.Parameter(1.0 / (n_timesteps * width ** 0.5) * torch.randn(n_timesteps, width, width))
        if kind == "exp_mlp":
            self.gamma = nn.Parameter(2 ** torch.linspace(-10, 10, width).unsqueeze(0))
        elif kind != "mlp":
            raise ValueError(f"unknown time_agg {kind!r}")


class _ModelBase(nn.Module):
    """What every model of the package shares (the DPOT family below, FNO2d, FNO3d): the precision scope around ``_forward``,
    its two settings and the input check.  It registers nothing: module order, ``state_dict()`` and the train.FlatParams layout
    are the subclass's alone."""
    # precision of the channel-MLP GEMMs of THIS model: None = the process default (ops.set_mlp_precision /
    # DPOT_MLP_PRECISION), or 'f32' | 'bf16x6' | 'auto' | 'bf16' (BASELINE configs[2]: "bf16 channel-MLP on MFMA")
    mlp_precision = None
    # precision of every OTHER fp32 GEMM of this model: None = the process default (ops.set_gemm_precision /
    # DPOT_GEMM_PRECISION), or 'f32' (native fp32 MFMA) | 'bf16x6' | 'auto' (the fp32-accurate operand split where faster)
    gemm_precision = None

    def forward(self, x):
        with ops.precision_scope(self.gemm_precision, self.mlp_precision):
            return self._forward(x)

    def _check_device(self, x) -> None:
        if not x.is_cuda:
            raise _lib.DpotHipError(f"{type(self).__name__} (dpot_amd) runs on MI355X only: move the model and the input to "
                                    "'cuda'. There is no CPU fallback.")


class _DPOTBase(_ModelBase):
    """What DPOTNet, DPOTNet3D and CDPOTNet share: the reference's attributes and argument checks, the modules all three register
    in ONE order - patch_embed, pos_embed, blocks, scale_feats_mu / _sigma (normalize=True), cls_head, time_agg_layer, out_layer:
    the order of ``state_dict()`` and of the train.FlatParams layout - built in that order too (it decides which random numbers
    initialise which weight), the coordinate tables and the normalize=True prologue and epilogue.  A subclass keeps the
    reference's constructor signature, hands its own patch embedding, Block and output layer over as factories, and writes
    ``_forward``."""
    cls_output = True           # forward returns (pred, cls_pred); False: the prediction alone (train.rollout: no classification branch)

    def __init__(self, img_size, patch_size, mixing_type, in_channels, out_channels, in_timesteps, out_timesteps, n_blocks,
                 embed_dim, out_layer_dim, depth, modes, mlp_ratio, n_cls, normalize, act, time_agg, *, patch_embed, block,
                 out_layer, coords=("_gx", "_gy")):
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

        self.patch_embed = patch_embed()
        self.latent_size = self.patch_embed.out_size
        self.pos_embed = nn.Parameter(torch.zeros(1, embed_dim, *self.latent_size))
        self.blocks = nn.ModuleList([block() for _ in range(depth)])
        if normalize:
            self.scale_feats_mu = nn.Linear(2 * in_channels, embed_dim)
            self.scale_feats_sigma = nn.Linear(2 * in_channels, embed_dim)
        # (DPOTNet3D constructs it and never calls it, models/dpot3d.py:288-294: it keeps the reference's state_dict, no gradient)
        self.cls_head = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.Identity(), nn.Linear(embed_dim, embed_dim),
                                      nn.Identity(), nn.Linear(embed_dim, n_cls))
        self.time_agg_layer = _TimeAggParams(in_timesteps, embed_dim, time_agg)
        self.out_layer = out_layer()
        torch.nn.init.trunc_normal_(self.pos_embed, std=.02)

        # coordinate tables of the reference's get_grid_3d / get_grid_4d (np.linspace in float64, then cast) - not part of state_dict
        for name, n in [(c, img_size) for c in coords] + [("_gt", in_timesteps)]:
            self.register_buffer(name, torch.tensor(np.linspace(0, 1, n), dtype=torch.float32), persistent=False)
        self.register_buffer("_tt", torch.linspace(0, 1, in_timesteps), persistent=False)
        # every weight-derived copy the kernels read (packed / padded / transposed weights) and when it is fresh
        self.packs = ModelPacks()

    def _normalize_in(self, x, dims):
        """normalize=True (models/dpot.py:366-370): per-sample statistics over `dims` + two tiny Linear(2C -> E), O(B*C) host-side
        glue -> (normalised x, mu, sigma, the AdaIN shift and scale); x and four None without it"""
        if not self.normalize:
            return x, None, None, None, None
        mu = x.mean(dim=dims, keepdim=True)
        sigma = x.std(dim=dims, keepdim=True) + 1e-6
        x = (x - mu) / sigma
        stat = torch.cat([mu, sigma], dim=-1)[(slice(None),) + (0,) * len(dims)]
        return x, mu, sigma, self.scale_feats_mu(stat), self.scale_feats_sigma(stat)

    def _denormalize(self, pred, mu, sigma):
        return pred * sigma + mu if self.normalize else pred

    def _time_agg_gamma(self):
        return self.time_agg_layer.gamma if self.time_agg == "exp_mlp" else None

    def extra_repr(self) -> str:
        return (f"img_size={self.img_size}, patch_size={self.patch_size}, embed_dim={self.embed_dim}, "
                f"depth={len(self.blocks)}, n_blocks={self.n_blocks}, modes={self.modes}, act={self.act_name}, "
                f"backend=libdpot_hip(gfx950)")


class DPOTNet(_DPOTBase):
    def __init__(self, img_size=224, patch_size=16, mixing_type='afno', in_channels=1, out_channels=4, in_timesteps=1,
                 out_timesteps=1, n_blocks=4, embed_dim=768, out_layer_dim=32, depth=12, modes=32, mlp_ratio=1.,
                 n_cls=12, normalize=False, act='gelu', time_agg='exp_mlp'):
        super().__init__(
            img_size, patch_size, mixing_type, in_channels, out_channels, in_timesteps, out_timesteps, n_blocks, embed_dim,
            out_layer_dim, depth, modes, mlp_ratio, n_cls, normalize, act, time_agg,
            patch_embed=lambda: _PatchEmbedParams(img_size, patch_size, in_channels + 3, out_channels * patch_size + 3, embed_dim),
            block=lambda: _BlockParams(embed_dim, n_blocks, mlp_ratio),
            out_layer=lambda: nn.Sequential(
                nn.ConvTranspose2d(embed_dim, out_layer_dim, patch_size, patch_size), nn.Identity(),
                nn.Conv2d(out_layer_dim, out_layer_dim, 1), nn.Identity(),
                nn.Conv2d(out_layer_dim, out_channels * out_timesteps, 1)))
        # activation recomputation inside every Block (functional.BlockFn): keep only block inputs between forward
        # and backward - for long auto-regressive rollouts at 256^2 (BASELINE configs[4])
        self.recompute_blocks = False
        # selective recomputation in an auto-regressive rollout (train.rollout tells the model which AR step a call is): the LAST
        # `recompute_keep_last` AR steps keep their activations like an ordinary forward - their backward runs first and frees them
        # before the first recomputation, so the peak stays at the end of the forward - and skip the second forward pass
        # (bit-identical either way; spends free HBM on time: DPOT-L, 20 steps, batch 16: 112 GB with 0 kept)
        self.recompute_keep_last = 0
        self._ar_pos = None                          # (index, count) of the current AR step, set by train.rollout
        # optional callable(b, lat) -> lat, called with the latent ENTERING stage b (1..depth = block b-1,
        # depth+1 = the head); train.SegmentedTrainStep cuts the autograd graph there
        self._boundary_hook = None

    # ------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def weights_scope(self):
        """Inside this scope the weight-only products of the forward (block-diagonal complex weights packed as real
        GEMM matrices, padded / transposed conv weights, the folded embed matrices) are computed by the FIRST forward
        call and re-used by the following ones: an auto-regressive rollout calls the model T_ar times per optimiser
        step on unchanged weights (train_temporal.py:201-219, evaluate.py:193-213).  The caller promises not to
        modify parameters inside the scope; outside a scope every forward derives them afresh (packs.ModelPacks)."""
        with self.packs.scope(self):
            yield self

    def _forward(self, x):
        self._check_device(x)
        B, X, Y, T, Cin = x.shape
        assert X == self.img_size and Y == self.img_size, \
            f"Input image size ({X}*{Y}) doesn't match model ({self.img_size}*{self.img_size})."
        assert T == self.in_timesteps and Cin == self.in_channels, "input timesteps / channels mismatch"
        x, mu, sigma, s_mu, s_sigma = self._normalize_in(x.float(), (1, 2, 3))

        pe, ta = self.patch_embed.proj, self.time_agg_layer
        P = self.patch_size
        h = self.latent_size[0]
        d_emb, pk, d_head, mlp_pk = self.packs.derive(self, defer=True)
        try:       # EmbedFn.forward joins the side lane that `derive` may have left forked, between its two launches
            lat = EmbedFn.apply(x, self.pos_embed, pe[0].weight, pe[0].bias, pe[2].weight, pe[2].bias, ta.w,
                                self._time_agg_gamma(), self._gx, self._gy, self._gt, self._tt,
                                P, self._act, d_emb)
        finally:
            ops.side_lane_join()
        if self.normalize:
            lat = AdaINFn.apply(lat, s_sigma, s_mu)                     # AdaIN (models/dpot.py:386-387)
        recompute = self.recompute_blocks and torch.is_grad_enabled()
        if recompute and self.recompute_keep_last > 0 and self._ar_pos is not None \
                and self._ar_pos[0] >= self._ar_pos[1] - self.recompute_keep_last:
            recompute = False
        hook = self._boundary_hook
        # the Blocks' weight gradients in batched launches after the last Block's backward (functional.WgradBatch) - not
        # with a boundary hook (the segmented data-parallel step wants every bucket's gradients final as the backward passes
        # it) and not under recomputation (a recomputing Block must not keep its re-derived activations alive)
        wb = WgradBatch() if (hook is None and not recompute and torch.is_grad_enabled()
                              and ops.wgrad_batch_enabled()) else None
        for i, blk in enumerate(self.blocks):
            cut = False
            if hook is not None:
                lat0 = lat
                lat = hook(i + 1, lat)
                cut = lat is not lat0          # the autograd graph is cut here (train.SegmentedTrainStep): this Block's input
            f = blk.filter                     # gradient goes to a leaf, not to the previous Block - no gradient packs
            lat = BlockFn.apply(lat, blk.norm1.weight, blk.norm1.bias, f.w1, f.b1, f.w2, f.b2, blk.norm2.weight,
                                blk.norm2.bias, blk.mlp[0].weight, blk.mlp[0].bias, blk.mlp[2].weight,
                                blk.mlp[2].bias, h, h, self.n_blocks, self.modes, self._act,
                                (pk[2 * i], pk[2 * i + 1]), recompute, mlp_pk[i] if mlp_pk is not None else None,
                                torch.is_grad_enabled(), i > 0 and not cut, wb)
        if hook is not None:
            lat = hook(len(self.blocks) + 1, lat)
        ol, ch = self.out_layer, self.cls_head
        pred, cls_pred = HeadFn.apply(lat, ol[0].weight, ol[0].bias, ol[2].weight, ol[2].bias, ol[4].weight,
                                      ol[4].bias, ch[0].weight, ch[0].bias, ch[2].weight, ch[2].bias, ch[4].weight,
                                      ch[4].bias, h, h, P, self._act, d_head)
        pred = pred.view(B, X, Y, self.out_timesteps, self.out_channels)
        return self._denormalize(pred, mu, sigma), cls_pred
