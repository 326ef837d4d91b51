"""CPU tests of the Fourier resize (utils/utilities.py:277-305) and the varying-resolution rollout's host parts: the closed
form against the fixture the reference wrote (g15_resize), the host matrices of ops.ResizePlan, refill_mask."""
import numpy as np
import pytest
import torch

from helpers import load
from resize_ref import hash_field, refill_mask_ref, resize_ref, ulps_apply

SMALL_PAIRS = [(16, 9), (16, 10), (9, 16), (10, 16), (10, 10), (16, 16), (9, 9), (12, 16), (16, 7), (128, 41), (50, 128),
               (128, 122), (41, 128), (128, 32), (64, 128)]


def cases(fx):
    return [str(n) for n in fx["names"]]


def case_input(fx, name):
    if f"{name}.x" in fx.files:
        return fx[f"{name}.x"]
    return hash_field(tuple(int(s) for s in fx[f"{name}.x_shape"]), int(fx[f"{name}.x_salt"]))


def assert_matches_f64_fixture(got, fx, name, what):
    """1e-10 of the tensor's maximum against the reference's float64 result.  The evaluation-sized cases store that result
    rounded to fp32 only (the fixture's size limit): there the stored number is itself up to half an fp32 ulp, 2^-24 |y|, away
    from the float64 value, and that much is added - nothing else"""
    if f"{name}.y64d" in fx.files:
        ref = fx[f"{name}.y64d"]
        tol = 1e-10 * np.abs(ref).max()
    else:
        ref = fx[f"{name}.y64"].astype(np.float64)
        tol = 1e-10 * np.abs(ref).max() + 2.0 ** -24 * np.abs(ref)
    assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
    err = np.abs(got - ref)
    assert np.isfinite(got).all() and (err <= tol).all(), (what, name, float(err.max()), float(np.abs(ref).max()))


def dense_apply(x, out_size):
    """the operator of ops.spectral_resize_matrices applied in float64: Re Dx in Re Dy^T - Im Dx in Im Dy^T, scaled"""
    from dpot_amd import ops
    B, nx, ny = x.shape[:3]
    mx, my = out_size
    rx, ix = ops.spectral_resize_matrices(nx, mx, 0)
    ry, iy = ops.spectral_resize_matrices(ny, my, 1)
    flat = np.asarray(x, dtype=np.float64).reshape(B, nx, ny, -1)
    out = np.einsum("ux,vy,bxyp->buvp", rx, ry, flat) - np.einsum("ux,vy,bxyp->buvp", ix, iy, flat)
    return (out / (nx * ny)).reshape((B, mx, my) + x.shape[3:])


def test_fixture_is_complete_and_small():
    import os
    from helpers import GOLDEN
    fx = load("g15_resize")
    assert len(cases(fx)) == 12
    assert os.path.getsize(os.path.join(GOLDEN, "g15_resize.npz")) <= os.path.getsize(os.path.join(GOLDEN, "g14_lamb.npz"))
    for name in cases(fx):
        y32 = ulps_apply(fx[f"{name}.y64"], fx[f"{name}.y32ulps"])
        assert np.isfinite(y32).all() and np.abs(y32 - fx[f"{name}.y64"]).max() <= 1e-4 * np.abs(y32).max()


def test_restatement_equals_reference_float64():
    fx = load("g15_resize")
    for name in cases(fx):
        got = resize_ref(case_input(fx, name), tuple(int(s) for s in fx[f"{name}.out_size"]))
        assert_matches_f64_fixture(got, fx, name, "resize_ref")


def test_ops_matrices_equal_reference_float64():
    fx = load("g15_resize")
    for name in cases(fx):
        got = dense_apply(case_input(fx, name), tuple(int(s) for s in fx[f"{name}.out_size"]))
        assert_matches_f64_fixture(got, fx, name, "spectral_resize_matrices")


@pytest.mark.parametrize("n,m", SMALL_PAIRS)
def test_im_dx_vanishes_or_has_rank_one(n, m):
    from dpot_amd import ops
    re, im = ops.spectral_resize_matrices(n, m, 0)
    uv = ops.spectral_resize_im_factors(n, m)
    if min(n, m) % 2 == 1 or n == m:
        assert np.abs(im).max() < 1e-12 and uv is None
        return
    sv = np.linalg.svd(im, compute_uv=False)
    assert sv[0] > 0.5 and sv[1] < 1e-12 * sv[0], sv[:3]
    assert np.abs(np.outer(uv[0], uv[1]) - im).max() < 1e-12


@pytest.mark.parametrize("sizes", [(16, 16, 9, 9), (10, 10, 16, 16), (12, 10, 16, 14), (16, 14, 7, 10), (128, 128, 41, 41),
                                   (50, 50, 128, 128), (128, 128, 122, 122), (59, 113, 128, 128)])
def test_plan_host_matrices_padding_is_zero_and_values_are_the_rounded_operator(sizes):
    from dpot_amd import ops
    nx, ny, mx, my = sizes
    nxp, nyp, mxp, myp = ops.ResizePlan.pads(*sizes)
    assert nxp % 16 == 0 and nyp % 16 == 0 and myp % 16 == 0 and mxp % 32 == 0
    assert 0 <= nxp - nx < 16 and 0 <= nyp - ny < 16 and 0 <= myp - my < 16 and 0 <= mxp - mx < 32
    h = ops.ResizePlan.host_matrices(*sizes)
    two = min(nx, mx) % 2 == 0 and nx != mx
    assert (h["byT"] is not None) == two and (h["u"] is not None) == two and (h["v"] is not None) == two
    shapes = {"axT": ((nxp, mxp), (nx, mx)), "ayT": ((nyp, myp), (ny, my)), "byT": ((nyp, myp), (ny, my)),
              "u": ((mxp,), (mx,)), "v": ((nxp,), (nx,))}
    for key, (full, used) in shapes.items():
        a = h[key]
        if a is None:
            continue
        assert a.dtype == np.float32 and a.shape == full and np.isfinite(a).all(), key
        pad = np.ones(full, dtype=bool)
        pad[tuple(slice(0, s) for s in used)] = False
        assert not a[pad].any(), f"{key}: non-zero padding"
    rx, _ = ops.spectral_resize_matrices(nx, mx, 0)
    ry, iy = ops.spectral_resize_matrices(ny, my, 1)
    assert np.array_equal(h["axT"][:nx, :mx], rx.T.astype(np.float32))
    assert np.array_equal(h["ayT"][:ny, :my], (ry.T / (nx * ny)).astype(np.float32))
    if two:
        assert np.array_equal(h["byT"][:ny, :my], (-iy.T / (nx * ny)).astype(np.float32))


def test_refill_mask_against_fixture():
    from dpot_amd.infer import refill_mask
    fx = load("g15_resize")
    msk, res = torch.from_numpy(fx["mask.in"]), int(fx["mask.res"])
    got = refill_mask(msk, res)
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert np.array_equal(got.numpy(), fx["mask.out"])
    assert np.array_equal(refill_mask_ref(fx["mask.in"], res), fx["mask.out"])
    assert tuple(refill_mask(msk, (4, 7)).shape) == (2, 4, 7, 1, 3)


def test_cpu_tensors_raise():
    """the product path has no CPU fallback: the resize and the rollout (with and without model_res) refuse CPU tensors"""
    import dpot_amd
    from dpot_amd import _lib, ops
    from dpot_amd.infer import rollout_eval
    from oracle import dpot_ref as R
    with pytest.raises(_lib.DpotHipError):
        ops.spectral_resize(torch.zeros(1, 8, 8, 1, 1), 6)
    model = dpot_amd.DPOTNet(**R.MINI)
    cfg = R.DPOTConfig(**R.MINI)
    S = cfg.img_size
    xx = torch.zeros(1, S, S, cfg.in_timesteps, cfg.in_channels)
    yy = torch.zeros(1, S, S, 2, cfg.out_channels)
    for kw in ({}, {"model_res": S}):
        with pytest.raises(Exception):
            rollout_eval(model, xx, yy, None, **kw)
    for name in ("rollout_eval", "GraphedRollout", "refill_mask", "spectral_resize", "spectral_resize_matrices", "ResizePlan"):
        assert hasattr(dpot_amd, name)


def test_abi_has_the_resize_entry_points():
    from dpot_amd import _lib
    lib = _lib.load()
    assert lib.dpot_version() >= 264
    assert lib.dpot_spectral_resize_pad(41, 0) == 48 and lib.dpot_spectral_resize_pad(41, 1) == 64
    assert lib.dpot_spectral_resize_pad(128, 0) == 128 and lib.dpot_spectral_resize_pad(128, 1) == 128
    # argument checks run before any device work: a null field is refused with a message
    rc = lib.dpot_spectral_resize(None, None, None, None, None, None, None, 1, 8, 8, 8, 8, 1, None)
    assert rc != 0 and b"spectral_resize" in lib.dpot_last_error()
