"""FNO3d for MI355X: the baseline of the 3-D fine-tuning script (the reference's models/fno.py:290-435), the other choice of
finetune3d.py's ``--model`` switch.

Same constructor signature and defaults, same ``state_dict`` keys / shapes / dtypes / order, same call contract

    pred = model(x)          # x: [B, X, Y, Z, T_in, C]  ->  [B, X, Y, Z, T_out, C]   (ONE tensor, like DPOTNet3D)

  lift       the T * C planes + the (x, y, z) unit grid (np.linspace(0, 1, n) per axis in float64, cast to fp32) -> fc0 =
             Linear(T * C + 3, width).  The grid is appended with ``torch.cat`` and fc0 runs as functional.LinearFn: glue on a
             (T * C + 3)-wide tensor, a few per cent of one layer's bytes at the reference width.
  layers     n_layers times gelu(SpectralConv3d(x) + Conv3d 1x1x1(x)) (functional.FNO3dLayerFn, csrc/fno3.hip), then
             GroupNorm(4, width) if use_ln.  GELU follows every layer, the last included.
  head       fc1, GELU, fc2 (functional.Mlp2Fn), reshaped to [B, X, Y, Z, T_out, C].

As in the reference, ``img_size``, ``patch_size``, ``n_cls`` and ``multi_channel`` are stored and never read by the forward, and
``normalize=True`` only creates ``scale_feats = Linear(2 C, width)``: the forward never reads it and normalises nothing.  It
exists for ``state_dict`` parity and has ``requires_grad=False``, so FlatParams leaves it out - the reference's optimiser skips
it too (it never gets a gradient), where a zero gradient plus weight decay would shrink it.

The forward takes any [B, X, Y, Z, T, C] whose sizes pass ops.fno3_check_modes: 2 * modes1 <= X and 2 * modes2 <= Y (the
reference silently lets later corner blocks overwrite earlier ones) and modes3 <= Z // 2 + 1, both a ValueError that names the
sizes; the constructor checks the ``img_size`` cube the same way.

The spectral weights: the reference holds four cfloat tensors [Cin, Cout, m1, m2, m3] per layer.  Here each is a REAL
nn.Parameter [Cin, Cout, m1, m2, m3, 2], its view_as_real, so FlatParams, the gradient slots, the clip and ``sumsq`` work
unchanged (the norm over the real view is the norm of the complex tensor) and the kernels read it in place.
``named_parameters()`` therefore yields real pairs, while ``state_dict()`` emits - and ``load_state_dict`` takes - the reference's
complex64 tensors.  The parameters carry ``_dpot_complex_pairs = True``: train.FusedAdam gives each pair one second moment, as the
reference's Adam does on complex parameters.  The torch modules are parameter containers only.  CUDA (ROCm) tensors only; there
is no CPU path.
"""
from __future__ import annotations

import numpy as np

import torch
import torch.nn as nn

from . import ops
from .model import _ModelBase
from .functional import FNO3dLayerFn, GroupNormFn, LinearFn, Mlp2Fn

GELU = ops.ACT_IDS["gelu"]


class _SpectralConv3dParams(nn.Module):
    """weights of SpectralConv3d (models/fno.py:305-316): four corner blocks, cfloat [Cin, Cout, m1, m2, m3] in the reference
    and in the state_dict, real pairs [Cin, Cout, m1, m2, m3, 2] as parameters"""
    NAMES = ("weights1", "weights2", "weights3", "weights4")

    def __init__(self, in_channels: int, out_channels: int, modes1: int, modes2: int, modes3: int):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.modes1, self.modes2, self.modes3 = modes1, modes2, modes3
        self.scale = 1 / (in_channels * out_channels)
        for name in self.NAMES:                      # torch.rand of a cfloat tensor draws the real and the imaginary part
            p = nn.Parameter(self.scale * torch.rand(in_channels, out_channels, modes1, modes2, modes3, 2))
            p._dpot_complex_pairs = True
            setattr(self, name, p)

    def weights(self):
        return tuple(getattr(self, n) for n in self.NAMES)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for name in self.NAMES:
            p = getattr(self, name)
            destination[prefix + name] = torch.view_as_complex(p if keep_vars else p.detach())

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        for name in self.NAMES:
            key, p = prefix + name, getattr(self, name)
            if key not in state_dict:
                if strict:
                    missing_keys.append(key)
                continue
            v = state_dict[key]
            if not torch.is_tensor(v) or not v.is_complex() or tuple(v.shape) != tuple(p.shape[:-1]):
                error_msgs.append(f"size mismatch for {key}: the checkpoint holds "
                                  f"{tuple(v.shape) if torch.is_tensor(v) else type(v).__name__} "
                                  f"{v.dtype if torch.is_tensor(v) else ''}, the model a complex {tuple(p.shape[:-1])}")
                continue
            with torch.no_grad():
                p.copy_(torch.view_as_real(v.detach().resolve_conj()))
        if strict:
            for key in state_dict:
                if key.startswith(prefix) and key[len(prefix):] not in self.NAMES and "." not in key[len(prefix):]:
                    unexpected_keys.append(key)


class FNO3d(_ModelBase):
    cls_output = False          # forward returns the prediction alone (train.rollout: no classification branch)

    def __init__(self, modes1, modes2, modes3, width, img_size=64, n_channels=1, in_timesteps=10, out_timesteps=1, n_layers=4,
                 patch_size=1, use_ln=False, multi_channel=True, normalize=False, n_cls=0):
        super().__init__()
        ops.fno3_check_modes(img_size, img_size, img_size, modes1, modes2, modes3,
                             f"FNO3d (img_size {img_size}: a {img_size}^3 field)")
        self.modes1, self.modes2, self.modes3, self.width, self.n_layers = modes1, modes2, modes3, width, n_layers
        self.n_channels, self.in_timesteps, self.out_timesteps = n_channels, in_timesteps, out_timesteps
        self.img_size, self.use_ln, self.padding, self.patch_size = img_size, use_ln, 6, patch_size
        self.normalize, self.n_cls = normalize, n_cls

        self.fc0 = nn.Linear(in_timesteps * n_channels + 3, width)
        self.spectral_convs = nn.ModuleList([_SpectralConv3dParams(width, width, modes1, modes2, modes3)
                                             for _ in range(n_layers)])
        self.convs = nn.ModuleList([nn.Conv3d(width, width, 1) for _ in range(n_layers)])
        if normalize:                    # never read by the forward, as in the reference: state_dict parity only
            self.scale_feats = nn.Linear(2 * n_channels, width)
            for p in self.scale_feats.parameters():
                p.requires_grad_(False)
        if use_ln:
            self.ln_layers = nn.ModuleList([nn.GroupNorm(4, width) for _ in range(n_layers)])
        self.fc1 = nn.Linear(width, width)
        self.fc2 = nn.Linear(width, n_channels * out_timesteps)
        self._grids = {}                 # (X, Y, Z, device) -> the unit grid [X, Y, Z, 3]

    def grid(self, X: int, Y: int, Z: int, device):
        """get_grid (models/fno.py:427-435) without the batch axis: np.linspace in float64 per axis, cast to fp32; cached per
        size and device (first use uploads: run one eager forward before capturing a graph)"""
        key = (X, Y, Z, torch.device(device))
        g = self._grids.get(key)
        if g is None:
            ax = [torch.tensor(np.linspace(0, 1, n), dtype=torch.float32) for n in (X, Y, Z)]
            g = torch.stack([ax[0].view(X, 1, 1).expand(X, Y, Z), ax[1].view(1, Y, 1).expand(X, Y, Z),
                             ax[2].view(1, 1, Z).expand(X, Y, Z)], dim=-1).contiguous().to(device)
            self._grids[key] = g
        return g

    def _forward(self, x):
        self._check_device(x)
        if x.dim() != 6:
            raise ValueError(f"FNO3d: the input must be [B, X, Y, Z, T, C], got {tuple(x.shape)}")
        B, X, Y, Z, T, C = x.shape
        ops.fno3_check_modes(X, Y, Z, self.modes1, self.modes2, self.modes3, f"FNO3d (a {X}x{Y}x{Z} field)")
        assert T == self.in_timesteps and C == self.n_channels, "input timesteps / channels mismatch"
        Wd, n = self.width, B * X * Y * Z
        x = x.float()
        v = torch.cat([x.reshape(B, X, Y, Z, T * C), self.grid(X, Y, Z, x.device).expand(B, X, Y, Z, 3)], dim=-1)
        z = LinearFn.apply(v.view(n, T * C + 3), self.fc0.weight, self.fc0.bias).view(B, X, Y, Z, Wd)
        for i in range(self.n_layers):
            sc, cv = self.spectral_convs[i], self.convs[i]
            z = FNO3dLayerFn.apply(z, *sc.weights(), cv.weight.view(Wd, Wd), cv.bias, GELU)
            if self.use_ln:
                ln = self.ln_layers[i]
                z = GroupNormFn.apply(z.view(B, X * Y * Z, Wd), ln.weight, ln.bias, 4).view(B, X, Y, Z, Wd)
        pred = Mlp2Fn.apply(z.view(n, Wd), self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, GELU)
        return pred.view(B, X, Y, Z, self.out_timesteps, C)

    def extra_repr(self) -> str:
        return (f"img_size={self.img_size}, width={self.width}, n_layers={self.n_layers}, "
                f"modes=({self.modes1}, {self.modes2}, {self.modes3}), backend=libdpot_hip(gfx950)")
