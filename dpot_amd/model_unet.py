"""UNet for MI355X: the second baseline the tables of the DPOT paper are read against (the reference's models/unet.py:372-564),
the fifth choice of its entry scripts' ``--model`` switch (finetune3d.py:125-126, evaluate_varyingres.py:29).

Same constructor signature and defaults, same ``state_dict`` (118 entries: keys, shapes, dtypes, order - convolution weights
[Cout, Cin, 3, 3], transposed-convolution weights [Cin, Cout, 2, 2], num_batches_tracked int64), same call contract

    pred, cls = model(x)          # x: [B, X, Y, T_in, C]  ->  [B, X, Y, T_out, C_out], zeros [B, n_cls]

  input      (T, C) flattened, the (x, y) unit grid (torch.linspace, float32) IN FRONT of the data channels, zero padding at the
             high end of both axes to the next multiple of 16 of ``in_shape``
  block      conv3x3 (padding 1, no bias), BatchNorm2d, act, twice (functional.ConvBNActFn, csrc/unet.hip); four encoder blocks
             with 2x2 max pooling behind each (the pooled field comes out of the block's last launch), the bottleneck, then four
             times transposed convolution k = s = 2 (functional.UpConv2Fn), concatenation with the skip, decoder block
  output     the padding cropped, Conv2d 1x1 (functional.LinearFn)

As in the reference the batch statistics are taken over the PADDED field.  ``model.train()``: every BatchNorm normalises with the
batch statistics and updates running_mean / running_var (momentum 0.1, unbiased variance, eps 1e-5) and num_batches_tracked by
device work that is legal under stream capture; ``model.eval()``: the running statistics, nothing is written, and a backward
raises.  The weights are read in place by the kernels: the model owns no derived copy (no ``packs``).  The torch modules are
parameter and buffer containers only.  CUDA (ROCm) tensors only; there is no CPU path.

Narrower than the reference, each a ValueError that says so: ``n_dim`` 2 only; no ``out_shape`` that differs from ``in_shape``
(the Interpolate branch); a window must be padded to a multiple of 16 by ``in_shape``'s padding (the reference fails inside
torch.cat).  ``cls`` carries no gradient: a weighted classification loss raises (``cls_trainable``).

Not here (see README): SegmentedTrainStep / make_dp_step, bf16 convolutions, a backward in eval mode, SyncBatchNorm.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
import torch.nn as nn

from . import ops
from .model import ACTIVATIONS, _ModelBase
from .functional import ConvBNActFn, LinearFn, UpConv2Fn


def _block(in_channels: int, features: int, name: str) -> nn.Sequential:
    """the reference's ``_block`` (models/unet.py:534-564) as a container: the activation has no state and is left out"""
    return nn.Sequential(OrderedDict([
        (name + "conv1", nn.Conv2d(in_channels, features, kernel_size=3, padding=1, bias=False)),
        (name + "norm1", nn.BatchNorm2d(features)),
        (name + "conv2", nn.Conv2d(features, features, kernel_size=3, padding=1, bias=False)),
        (name + "norm2", nn.BatchNorm2d(features)),
    ]))


class UNet(_ModelBase):
    cls_output = True
    cls_trainable = False       # cls is a constant: train.rollout_total refuses cls_weight != 0 (no gradient path to weigh)

    def __init__(self, n_dim, in_channels=3, out_channels=1, in_timesteps=10, out_timesteps=1, multi_channel=False,
                 in_shape=None, out_shape=None, width=32, act='gelu', n_cls=1):
        super().__init__()
        if n_dim != 2:
            raise ValueError(f"UNet (dpot_amd): only n_dim == 2 is built (the 3x3 convolution, BatchNorm2d and 2x2 pooling "
                             f"kernels), got n_dim = {n_dim}")
        if in_shape is None or len(in_shape) != 2:
            raise ValueError(f"UNet: in_shape must be (X, Y), got {in_shape!r}")
        if out_shape is not None and tuple(out_shape) != tuple(in_shape):
            raise ValueError(f"UNet (dpot_amd): out_shape {tuple(out_shape)} differs from in_shape {tuple(in_shape)}: the "
                             "reference's Interpolate output branch is not built")
        if act not in ACTIVATIONS:
            raise KeyError(act)
        self.n_dim, self.features = n_dim, width
        self.act_name, self._act = act, ops.ACT_IDS[act]
        self.in_channels, self.out_channels = in_channels, out_channels
        self.in_timesteps, self.out_timesteps = in_timesteps, out_timesteps
        self.multi_channel, self.n_cls = multi_channel, n_cls
        self.in_shape, self.out_shape = tuple(in_shape), None if out_shape is None else tuple(out_shape)
        self.padding = [int(math.ceil(s / 16) * 16 - s) for s in in_shape]
        f = width
        ops.unet_check_sizes(in_shape[1] + self.padding[1], (in_channels * in_timesteps + n_dim, 16 * f),
                             f"UNet (in_shape {self.in_shape}, width {width})")

        self.encoder1 = _block(in_channels * in_timesteps + n_dim, f, "enc1")
        self.encoder2 = _block(f, f * 2, "enc2")
        self.encoder3 = _block(f * 2, f * 4, "enc3")
        self.encoder4 = _block(f * 4, f * 8, "enc4")
        self.bottleneck = _block(f * 8, f * 16, "bottleneck")
        self.upconv4 = nn.ConvTranspose2d(f * 16, f * 8, kernel_size=2, stride=2)
        self.decoder4 = _block(f * 16, f * 8, "dec4")
        self.upconv3 = nn.ConvTranspose2d(f * 8, f * 4, kernel_size=2, stride=2)
        self.decoder3 = _block(f * 8, f * 4, "dec3")
        self.upconv2 = nn.ConvTranspose2d(f * 4, f * 2, kernel_size=2, stride=2)
        self.decoder2 = _block(f * 4, f * 2, "dec2")
        self.upconv1 = nn.ConvTranspose2d(f * 2, f, kernel_size=2, stride=2)
        self.decoder1 = _block(f * 2, f, "dec1")
        self.conv = nn.Conv2d(f, out_timesteps * out_channels, kernel_size=1)
        self._axes = {}                              # (length, device) -> the unit grid of one axis (_axis)

    def _axis(self, n: int, device) -> torch.Tensor:
        """torch.linspace(0, 1, n) as the reference's get_grid computes it (on the host, float32), kept per length and device:
        the upload happens in the first call of a shape - a warm-up - and never under a stream capture"""
        key = (n, str(device))
        t = self._axes.get(key)
        if t is None:
            t = self._axes[key] = torch.linspace(0, 1, n, dtype=torch.float32).to(device)
        return t

    def _layer(self, x, conv, norm, pool: bool = False):
        return ConvBNActFn.apply(x, conv.weight, norm.weight, norm.bias, norm.running_mean, norm.running_var,
                                 norm.num_batches_tracked, self._act, pool, self.training)

    def _run(self, x, block, pool: bool = False):
        conv1, norm1, conv2, norm2 = block
        return self._layer(self._layer(x, conv1, norm1), conv2, norm2, pool)

    def _forward(self, x):
        B, X, Y, T, C = x.shape
        assert T == self.in_timesteps and C == self.in_channels, "input timesteps / channels mismatch"
        Hp, Wp = X + self.padding[0], Y + self.padding[1]
        if Hp % 16 or Wp % 16:
            raise ValueError(f"UNet: a {X}x{Y} window padded by {tuple(self.padding)} (in_shape {self.in_shape}) is {Hp}x{Wp}, "
                             "not a multiple of 16 on both axes: the four poolings and transposed convolutions would not "
                             "return to its size")
        ops.unet_check_sizes(Wp, (), "UNet")
        self._check_device(x)
        # input assembly (torch glue): (T, C) flattened, grid first (get_grid, models/unet.py:448-470), zero padding
        x = x.float().reshape(B, X, Y, T * C)
        gx = self._axis(X, x.device).view(1, X, 1, 1).expand(B, X, Y, 1)
        gy = self._axis(Y, x.device).view(1, 1, Y, 1).expand(B, X, Y, 1)
        x = torch.cat([gx, gy, x], dim=-1)
        if Hp != X or Wp != Y:
            x = nn.functional.pad(x, (0, 0, 0, Wp - Y, 0, Hp - X))
        x = x.contiguous()

        enc1, p = self._run(x, self.encoder1, pool=True)
        enc2, p = self._run(p, self.encoder2, pool=True)
        enc3, p = self._run(p, self.encoder3, pool=True)
        enc4, p = self._run(p, self.encoder4, pool=True)
        d = self._run(p, self.bottleneck)
        for up, skip, dec in ((self.upconv4, enc4, self.decoder4), (self.upconv3, enc3, self.decoder3),
                              (self.upconv2, enc2, self.decoder2), (self.upconv1, enc1, self.decoder1)):
            d = self._run(torch.cat([UpConv2Fn.apply(d, up.weight, up.bias), skip], dim=-1), dec)

        f = self.features
        rows = d[:, :X, :Y, :].reshape(B * X * Y, f)
        No = self.out_timesteps * self.out_channels
        pred = LinearFn.apply(rows, self.conv.weight.view(No, f), self.conv.bias)
        return pred.view(B, X, Y, self.out_timesteps, self.out_channels), x.new_zeros(B, self.n_cls)

    def extra_repr(self) -> str:
        return (f"in_shape={self.in_shape}, padding={tuple(self.padding)}, width={self.features}, act={self.act_name}, "
                f"backend=libdpot_hip(gfx950)")
