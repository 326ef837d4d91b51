"""CPU tests of the 3-D input pipeline's host logic and of its restatement (tests/data3d_ref.py) against the golden vectors
(g19: written by the reference's own `TemporalDataset3D.__getitem__`, utils/griddataset.py:521-561, with an in-memory
stand-in for h5py - scripts/make_golden_data3d.py, which demands bit equality; here the tolerance of the GPU test, since
another host's vector path may round F.interpolate differently)."""
import ctypes

import numpy as np
import pytest
import torch

import data3d_ref as D3
from helpers import assert_close, load

TOL = dict(rtol=1e-6, atol_scale=1e-6)


def test_restatement_matches_golden_training_cases():
    fx = load("g19_data3d")
    k = 0
    while f"c{k}.meta" in fx.files:
        H, W, L, T, Cc, res, nc, t_in, t_ar, t0 = (int(v) for v in fx[f"c{k}.meta"])
        raw = D3.recipe_sample3((H, W, L, T, Cc), salt=100 + k)
        x, y = D3.window(D3.pad_data3(raw, res, nc), t0, t_in, t_ar)
        assert_close(x, fx[f"c{k}.x"], f"case {k} x", **TOL)
        assert_close(y, fx[f"c{k}.y"], f"case {k} y", **TOL)
        assert tuple(x.shape) == (res, res, res, t_in, nc) and tuple(y.shape) == (res, res, res, t_ar, nc)
        assert (x[..., Cc:] == 1).all() and (y[..., Cc:] == 1).all()           # padded channels are ones
        k += 1
    assert k == 4


def test_restatement_and_host_helpers_match_golden_test_mode_cases():
    from dpot_amd.data import _down_shape, eval_window, target_mask3
    fx = load("g19_data3d")
    k = 0
    while f"t{k}.meta" in fx.files:
        H, W, L, T, Cc, res, nc, t_in, t_test, d0, d1, d2, pc = (int(v) for v in fx[f"t{k}.meta"])
        raw = D3.recipe_sample3((H, W, L, T, Cc), salt=200 + k)
        padded = D3.pad_data3(raw, res, nc)
        x, y = D3.downsample3(*D3.test_window(padded, t_in, t_test), (d0, d1, d2))
        assert_close(x, fx[f"t{k}.x"], f"test case {k} x", **TOL)
        assert_close(y, fx[f"t{k}.y"], f"test case {k} y", **TOL)
        size_orig = [H, W, L, T, Cc if pc < 0 else pc]
        assert np.array_equal(D3.target_mask3(padded, size_orig).numpy(), fx[f"t{k}.msk"])
        assert np.array_equal(target_mask3(res, size_orig, nc).numpy(), fx[f"t{k}.msk"])
        t0, t_ar = eval_window(T, t_in, t_test)
        assert t0 == 0 and t_ar == fx[f"t{k}.y"].shape[3]
        assert _down_shape(res, (d0, d1, d2)) == fx[f"t{k}.x"].shape[:3]
        k += 1
    assert k == 4


def test_target_mask3_strides_channels_and_coarse_target():
    from dpot_amd.data import target_mask3
    # griddataset.py:503-518 transcribed
    res, size_orig, nc = 12, [4, 6, 3, 20, 2], 3
    msk = torch.zeros(res, res, res, 1, nc)
    msk[::3, ::2, ::4, :, :2] = 1
    got = target_mask3(res, size_orig, nc)
    assert tuple(got.shape) == (res, res, res, 1, nc) and torch.equal(got, msk)
    # target coarser than the data on two axes (k == 0 -> 1), finer on the third
    got = target_mask3(8, [16, 9, 4, 5, 1], 2)
    assert got[..., 0].sum() == 8 * 8 * 4 and got[..., 1].sum() == 0
    assert torch.equal(got[:, :, 1::2], torch.zeros(8, 8, 4, 1, 2))


def test_window_only_staging_arithmetic_and_descriptor_table():
    from dpot_amd import _lib
    from dpot_amd.data import DESC_BYTES, _fill_table, staged_floats
    assert ctypes.sizeof(_lib.Sample3Desc) == 32 == DESC_BYTES
    # the README's figures: 11 of 21 frames of a [128,128,128,21,5] trajectory are 461 MB of its 880 MB
    assert staged_floats((128, 128, 128, 21, 5), 10, 1) * 4 == 461373440
    assert staged_floats((6, 5, 7, 30), 3, 2) == 6 * 5 * 7 * 5
    table = np.zeros(2 * DESC_BYTES, dtype=np.uint8)
    ptrs = [0x7F0012345600, 0x7F0012345604]
    _fill_table(table, ptrs, [(6, 5, 7, 8, 2), (3, 4, 5, 9, 3)], [1, 2], 4, 2, 5, _lib.Sample3Desc)
    d = (_lib.Sample3Desc * 2).from_buffer(table)
    assert [(x.data, x.H, x.W, x.L, x.T, x.C, x.t0) for x in d] == [(ptrs[0], 6, 5, 7, 8, 2, 1), (ptrs[1], 3, 4, 5, 9, 3, 2)]
    # the layout the kernel reads: pointer, then six int32
    assert table[8:32].view(np.int32).tolist() == [6, 5, 7, 8, 2, 1]
    with pytest.raises(ValueError, match="sample 1"):                      # window past the trajectory
        _fill_table(table, ptrs, [(6, 5, 7, 8, 2), (3, 4, 5, 9, 3)], [1, 4], 4, 2, 5, _lib.Sample3Desc)
    with pytest.raises(ValueError, match="sample 0"):                      # more channels than the batch has
        _fill_table(table, ptrs, [(6, 5, 7, 8, 6), (3, 4, 5, 9, 3)], [1, 2], 4, 2, 5, _lib.Sample3Desc)
    with pytest.raises(ValueError, match="sample 0"):
        _fill_table(table, ptrs, [(6, 5, 7, 8, 2), (3, 4, 5, 9, 3)], [-1, 2], 4, 2, 5, _lib.Sample3Desc)
