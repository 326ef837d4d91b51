"""CPU restatement of the 3-D input pipeline's sample transform.  TEST INFRASTRUCTURE ONLY.

Restates TemporalDataset3D of the reference (utils/griddataset.py:488-501 `pad_data`: trilinear resize of every (t, c)
volume with F.interpolate(mode='trilinear'), channel pad with ones; :503-518 `get_target_mask`; :544-558 the training and
test windows and the strided down-sampling) for one raw sample [H, W, L, T, C].
Pinned by tests/golden/g19_data3d.npz, written by the reference's own `TemporalDataset3D.__getitem__`
(scripts/make_golden_data3d.py, which demands bit equality with this file before it writes anything).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

Tensor = torch.Tensor


def pad_data3(x: Tensor, res: int, n_channels: int) -> Tensor:
    """[H,W,L,T,C] -> [res,res,res,T,n_channels]   (griddataset.py:488-501)"""
    H, W, L, T, Cc = x.shape
    vol = x.reshape(H, W, L, T * Cc).permute(3, 0, 1, 2).unsqueeze(0)                  # [1, T*C, H, W, L]
    vol = F.interpolate(vol, size=(res, res, res), mode="trilinear").squeeze(0).permute(1, 2, 3, 0)
    out = torch.ones(res, res, res, T, n_channels)
    out[..., :Cc] = vol.reshape(res, res, res, T, Cc)
    return out


def window(sample: Tensor, t0: int, t_in: int, t_ar: int):
    """griddataset.py:546: x = sample[..., t0:t0+t_in, :], y = sample[..., t0+t_in : min(t0+t_in+t_ar, T), :]"""
    return sample[..., t0:t0 + t_in, :], sample[..., t0 + t_in:min(t0 + t_in + t_ar, sample.shape[-2]), :]


def test_window(sample: Tensor, t_in: int, t_test: int):
    """griddataset.py:550-551 (test datasets): x = the first t_in frames, y = sample[..., t_in : t_in + t_test, :]"""
    return sample[..., 0:t_in, :], sample[..., t_in:t_in + t_test, :]


test_window.__test__ = False          # a helper, not a test (its name is the reference's wording)


def target_mask3(sample: Tensor, size_orig) -> Tensor:
    """griddataset.py:503-518 get_target_mask: ones on the grid points / channels the dataset itself has"""
    msk = torch.zeros(*sample.shape[:3], 1, sample.shape[-1])
    kx, ky, kz = (sample.shape[i] // size_orig[i] for i in range(3))
    kx, ky, kz = (1 if kx == 0 else kx), (1 if ky == 0 else ky), (1 if kz == 0 else kz)
    msk[::kx, ::ky, ::kz, :, :size_orig[-1]] = 1
    return msk


def downsample3(x: Tensor, y: Tensor, d):
    """griddataset.py:557-558"""
    return x[::d[0], ::d[1], ::d[2]], y[::d[0], ::d[1], ::d[2]]


def recipe_sample3(shape, salt: int) -> Tensor:
    """closed-form raw trajectory [H,W,L,T,C] (a smooth field + a hash texture), evaluated in float64 and rounded to
    float32 once, so that it is the same wherever it is evaluated"""
    H, W, L, T, Cc = shape
    n = H * W * L * T * Cc
    u = np.sin(np.arange(n, dtype=np.float64) * 12.9898 + (311 + 17 * salt) * 78.233 + 0.5) * 43758.5453
    u = torch.from_numpy((u - np.floor(u)).reshape(shape))
    g = [torch.linspace(0, 1, s, dtype=torch.float64) for s in (H, W, L, T)]
    gx, gy, gz, gt = g[0].view(H, 1, 1, 1, 1), g[1].view(1, W, 1, 1, 1), g[2].view(1, 1, L, 1, 1), g[3].view(1, 1, 1, T, 1)
    c = torch.arange(1, Cc + 1, dtype=torch.float64).view(1, 1, 1, 1, Cc)
    field = torch.sin(6.0 * gx * c + 3.0 * gt) * torch.cos(4.0 * gy + c) * torch.cos(5.0 * gz - 2.0 * gt + 0.5 * c)
    return (field + 0.25 * (u - 0.5)).float().contiguous()
