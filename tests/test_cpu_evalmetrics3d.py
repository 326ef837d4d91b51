"""CPU tests of the 3-D evaluation metrics (dpot_amd.RolloutEvaluator on [B, X, Y, Z, T, C], csrc/evalmetrics3d.hip): the float64
restatement (tests/eval3d_ref.py) against the fixture the reference wrote (g20_evalmetrics3d), the host tables the kernels
read (shell table, its range form, the DFT tables along three axes), the arithmetic of read() and its additivity over
batches, the argument errors that need no GPU, and the ABI additions."""
import math

import numpy as np
import pytest
import torch

import eval3d_ref as E
from helpers import assert_close, load

CASES = ["o6x5x7_t3c2", "e8_t10c4", "r10x12x9_t2c3", "r12x10x8_t1c1", "two_batches", "r20x33x26_t1c2", "e16_default", "big32",
         "big64"]
FIXTURE = "g20_evalmetrics3d"


def whole(fx, name):
    pairs = E.case_fields(fx, name)
    return np.concatenate([p for p, _ in pairs]), np.concatenate([t for _, t in pairs])


def test_fixture_lists_the_cases_of_the_gpu_file_and_of_its_generator():
    import ast
    import os
    import test_gpu_evalmetrics3d as G
    fx = load(FIXTURE)
    assert [str(n) for n in fx["names"]] == CASES == G.CASES
    # the generator's own table, read without importing it (it imports the reference)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts",
                            "make_golden_evalmetrics3d.py")).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and n.targets[0].id == "CASES")
    table = ast.literal_eval(node.value)
    assert list(table) == CASES
    for name, (batches, nx, ny, nz, T, C, ilow, ihigh, kind) in table.items():
        assert tuple(fx[f"{name}.shape"]) == (sum(batches), nx, ny, nz, T, C)
        assert tuple(fx[f"{name}.batches"]) == batches and tuple(fx[f"{name}.bands"]) == (ilow, ihigh)
        assert (f"{name}.salt" in fx.files) == (kind == "hash") and (f"{name}.pred" in fx.files) == (kind != "hash")
    # the shapes, planes and bands the fixture is meant to hold
    assert sorted((tuple(fx[f"{n}.shape"][1:]), tuple(fx[f"{n}.bands"])) for n in CASES) == sorted([
        ((6, 5, 7, 3, 2), (1, 2)), ((8, 8, 8, 10, 4), (1, 3)), ((10, 12, 9, 2, 3), (1, 3)), ((12, 10, 8, 1, 1), (1, 2)),
        ((12, 10, 8, 2, 2), (1, 2)), ((20, 33, 26, 1, 2), (4, 8)), ((16, 16, 16, 2, 2), (4, 12)),
        ((32, 32, 32, 2, 2), (4, 12)), ((64, 64, 64, 1, 2), (4, 12))])
    assert tuple(fx["two_batches.batches"]) == (2, 3)


@pytest.mark.parametrize("name", CASES)
def test_restatement_vs_reference_fixture(name):
    """the float64 restatement against the reference's float64 result at the parity tolerance (and, tighter than that, at
    1e-9: float64 against float64); NaN exactly where the reference has NaN"""
    fx = load(FIXTURE)
    p, t = whole(fx, name)
    ilow, ihigh = (int(v) for v in fx[f"{name}.bands"])
    got = E.eval_ref(p, t, ilow, ihigh)
    T, C = p.shape[-2:]
    shapes = {"nmae": (1, C), "nmse": (1, C), "nmxe": (1, C), "nmae_t": (1, T, C), "nmse_t": (1, T, C), "nmxe_t": (1, T, C),
              "bdmse": (C, T), "fmse_low": (T, C), "fmse_mid": (T, C), "fmse_high": (T, C)}
    for key in E.KEYS:
        want = fx[f"{name}.{key}.r64"]
        assert want.dtype == np.float64 and got[key].shape == want.shape == shapes[key], key
        assert fx[f"{name}.{key}.r32"].dtype == np.float32 and fx[f"{name}.{key}.r32"].shape == want.shape, key
        assert np.array_equal(np.isnan(got[key]), np.isnan(want)), key
        fin = ~np.isnan(want)
        assert np.isfinite(want[fin]).all()
        if fin.any():
            assert_close(got[key][fin], want[fin], f"{name} {key}")
            assert (np.abs(got[key][fin] - want[fin]) <= 1e-9 * np.abs(want[fin])).all(), key
    K = min(s // 2 for s in p.shape[1:4])
    assert np.isnan(fx[f"{name}.fmse_high.r64"]).all() == (K <= ihigh)
    assert not np.isnan(fx[f"{name}.fmse_low.r64"]).any() and not np.isnan(fx[f"{name}.fmse_mid.r64"]).any()


def test_fixture_has_the_two_empty_band_cases():
    fx = load(FIXTURE)
    empty = [n for n in CASES if np.isnan(fx[f"{n}.fmse_high.r64"]).any()]
    assert empty == ["o6x5x7_t3c2", "e16_default"]
    for n in empty:
        assert np.isnan(fx[f"{n}.fmse_high.r64"]).all() and np.isnan(fx[f"{n}.fmse_high.r32"]).all()


def test_hashed_inputs_are_fp32_and_repeatable():
    p, t = E.hashed_pair((1, 6, 5, 7, 2, 3), 4)
    q, u = E.hashed_pair((1, 6, 5, 7, 2, 3), 4)
    assert p.dtype == t.dtype == np.float32 and p.shape == (1, 6, 5, 7, 2, 3)
    assert np.array_equal(p, q) and np.array_equal(t, u) and not np.array_equal(p, t)
    assert np.abs(p - t).max() <= 0.08 and np.abs(t).max() < 3.0        # near-equal fields of order one


@pytest.mark.parametrize("sizes", [(8, 8, 8), (16, 16, 16), (6, 5, 7), (9, 11, 10), (20, 33, 26), (33, 16, 48), (17, 40, 12),
                                   (4, 6, 40)])
def test_shell_table_is_the_integer_square_root(sizes):
    from dpot_amd import ops
    nx, ny, nz = sizes
    hx, hy, hz = nx // 2, ny // 2, nz // 2
    K = min(hx, hy, hz)
    tab = ops.eval_shell_table(nx, ny, nz)
    assert tab.shape == (hx, hy, hz) and tab.dtype == np.int32
    dropped = 0
    for i in range(hx):
        for j in range(hy):
            for k in range(hz):
                s = math.isqrt(i * i + j * j + k * k)
                assert tab[i, j, k] == (s if s < K else -1), (i, j, k)
                dropped += s >= K
    assert (tab == -1).sum() == dropped > 0                        # the far corner of the octant lies beyond shell K - 1
    # the range form the kernel walks describes the same table: row (k, i), shell s = the j range [k, i, s] .. [k, i, s + 1]
    rng = ops.eval_shell_ranges(nx, ny, nz)
    assert rng.shape == (hz, hx, K + 1) and rng.dtype == np.int32
    rebuilt = np.full_like(tab, -1)
    for k in range(hz):
        for i in range(hx):
            assert rng[k, i, 0] == 0 and (np.diff(rng[k, i]) >= 0).all() and rng[k, i, K] <= hy
            for s in range(K):
                rebuilt[i, rng[k, i, s]:rng[k, i, s + 1], k] = s
    assert np.array_equal(rebuilt, tab)
    with pytest.raises(ValueError):
        ops.eval_shell_table(nx, 1, nz)


@pytest.mark.parametrize("sizes", [(6, 5, 7), (8, 8, 8), (10, 12, 9), (20, 33, 26), (16, 40, 12)])
def test_dft_tables_along_three_axes_reproduce_fftn_on_the_positive_octant(sizes):
    from dpot_amd import ops
    nx, ny, nz = sizes
    hx, hy, hz = nx // 2, ny // 2, nz // 2
    rs = np.random.RandomState(nx * 10000 + ny * 100 + nz)
    e = rs.randn(nx, ny, nz)
    (cx, sx), (cy, sy), (cz, sz) = ops.eval_dft_tables(nx), ops.eval_dft_tables(ny), ops.eval_dft_tables(nz)
    # the kernels' order: z first (Gc - 1j Gs), then x (U), then y (E)
    gc, gs = np.einsum("kz,xyz->kxy", cz, e), np.einsum("kz,xyz->kxy", sz, e)
    ur = np.einsum("ix,kxy->kiy", cx, gc) - np.einsum("ix,kxy->kiy", sx, gs)
    ui = -(np.einsum("ix,kxy->kiy", cx, gs) + np.einsum("ix,kxy->kiy", sx, gc))
    re = np.einsum("kiy,jy->ijk", ur, cy) + np.einsum("kiy,jy->ijk", ui, sy)
    im = np.einsum("kiy,jy->ijk", ui, cy) - np.einsum("kiy,jy->ijk", ur, sy)
    want = np.fft.fftn(e)[:hx, :hy, :hz]
    scale = np.abs(want).max()
    assert np.abs(re - want.real).max() <= 1e-12 * scale and np.abs(im - want.imag).max() <= 1e-12 * scale
    # what the kernels receive: fp32, transposed where they want them K-major, zero in the padding
    pads = ops.EvalPlan.pads(nx, ny, nz)
    assert all(v % 16 == 0 for v in pads) and pads[0] >= nx and pads[4] >= hy and pads[5] - hz < 16
    nxp, nyp, nzp, hxp, hyp, hzp = pads
    h = ops.EvalPlan.host_tables(nx, ny, nz)
    for key, full, used, src in (("cxT", (nxp, hxp), (nx, hx), cx.T), ("sxT", (nxp, hxp), (nx, hx), sx.T),
                                 ("cy", (nyp, hyp), (ny, hy), cy.T), ("sy", (nyp, hyp), (ny, hy), sy.T),
                                 ("czT", (nzp, hzp), (nz, hz), cz.T), ("szT", (nzp, hzp), (nz, hz), sz.T)):
        a = h[key]
        assert a.dtype == np.float32 and a.shape == full and np.isfinite(a).all(), key
        pad = np.ones(full, dtype=bool)
        pad[:used[0], :used[1]] = False
        assert not a[pad].any(), f"{key}: non-zero padding"
        assert np.array_equal(a[:used[0], :used[1]], src.astype(np.float32)), key
    assert np.array_equal(h["jlo"], ops.eval_shell_ranges(nx, ny, nz)) and h["jlo"].flags["C_CONTIGUOUS"]


def acc_vector(sums, nx, ny, nz, T, C):
    """tests/eval3d_ref.batch_sums laid out as the device accumulator (ops.eval_acc_layout)"""
    from dpot_amd import ops
    off, total = ops.eval_acc_layout(nx, ny, nz, T, C)
    acc = np.zeros(total)
    acc[off["c"]:off["tc"]] = sums["c"].reshape(-1)
    acc[off["tc"]:off["spec"]] = sums["tc"].reshape(-1)
    acc[off["spec"]:] = sums["spec"].reshape(-1)
    return acc


@pytest.mark.parametrize("name", ["two_batches", "o6x5x7_t3c2", "r10x12x9_t2c3"])
def test_read_arithmetic_and_batch_additivity(name):
    """the numpy model of read() (ops.eval_finish) on sums added over two batches equals eval_ref and the reference on the
    concatenation; shapes and dtypes are the 2-D evaluator's"""
    from dpot_amd import ops
    fx = load(FIXTURE)
    p, t = whole(fx, name)
    B, nx, ny, nz, T, C = p.shape
    ilow, ihigh = (int(v) for v in fx[f"{name}.bands"])
    cut = 1 if B < 3 else 2
    s = E.add_sums(E.batch_sums(p[:cut], t[:cut]), E.batch_sums(p[cut:], t[cut:]))
    assert s["count"] == B
    got = ops.eval_finish(acc_vector(s, nx, ny, nz, T, C), B, nx, ny, nz, T, C, ilow, ihigh)
    ref = E.eval_ref(p, t, ilow, ihigh)
    assert got["samples"] == B and set(got) == set(E.KEYS) | {"samples"} and set(ops.EVAL_KEYS) == set(E.KEYS)
    for key in E.KEYS:
        want = fx[f"{name}.{key}.r64"]
        assert got[key].dtype == np.float32 and got[key].shape == want.shape == ref[key].shape, key
        assert np.array_equal(np.isnan(got[key]), np.isnan(want)), key
        fin = ~np.isnan(want)
        assert (np.abs(got[key][fin] - want[fin]) <= 2.0 ** -23 * np.abs(want[fin])).all(), key     # one fp32 rounding
        assert (np.abs(got[key][fin] - ref[key][fin]) <= 2.0 ** -23 * np.abs(ref[key][fin])).all(), key
    with pytest.raises(ValueError):
        ops.eval_finish(np.zeros(3), 1, nx, ny, nz, T, C)
    none = ops.eval_finish(np.zeros(ops.eval_acc_layout(nx, ny, nz, T, C)[1]), 0, nx, ny, nz, T, C, ilow, ihigh)
    assert none["samples"] == 0 and np.isnan(none["nmae"]).all()


def test_cpu_tensors_and_bad_arguments_raise():
    """no CPU fallback: the evaluator and the op refuse CPU tensors; shape rules are host-side checks"""
    from dpot_amd import RolloutEvaluator, _lib, ops
    ev = RolloutEvaluator("cuda", n_channels=2, T_max=3)
    z = torch.zeros(1, 8, 8, 8, 3, 2)
    with pytest.raises(_lib.DpotHipError, match="MI355X"):
        ev.update(z, z)                                            # CPU tensors
    with pytest.raises(_lib.DpotHipError):
        ev.update(torch.zeros(1, 8, 8, 8, 4, 2), torch.zeros(1, 8, 8, 8, 4, 2))      # T > T_max
    with pytest.raises(_lib.DpotHipError):
        ev.update(torch.zeros(1, 8, 8, 8, 3, 3), torch.zeros(1, 8, 8, 8, 3, 3))      # another channel count
    with pytest.raises(_lib.DpotHipError):
        ev.update(z, torch.zeros(1, 8, 8, 9, 3, 2))                # shapes differ
    with pytest.raises(_lib.DpotHipError):
        ev.update(torch.zeros(8, 8, 3, 2), torch.zeros(8, 8, 3, 2))                  # neither 5-D nor 6-D
    with pytest.raises(_lib.DpotHipError):
        ev.read()                                                  # nothing to read
    acc = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(_lib.DpotHipError, match="MI355X"):
        ops.eval_metrics_update(z, z, acc)
    for bad in (z.double(), z.transpose(1, 2)):
        with pytest.raises(_lib.DpotHipError):
            ops.eval_metrics_update(bad, bad, acc)
    with pytest.raises(ValueError):
        ops.eval_shell_ranges(1, 8, 8)


def test_rollout_eval_takes_an_evaluator_but_no_model_res_for_6d_windows():
    """model_res= with a 6-D window is a ValueError that names model_res alone; evaluator= is no longer refused (without a
    GPU the rollout then fails later, in the model's own device check, not with that ValueError)"""
    import dpot_amd
    from dpot_amd import _lib, infer
    m = dpot_amd.DPOTNet3D(img_size=8, patch_size=4, in_channels=2, out_channels=2, in_timesteps=3, embed_dim=16, depth=1,
                           n_blocks=2, modes=2)
    xx, yy = torch.zeros(1, 8, 8, 8, 3, 2), torch.zeros(1, 8, 8, 8, 2, 2)
    with pytest.raises(ValueError, match="model_res") as info:
        infer.rollout_eval(m, xx, yy, None, model_res=8)
    assert "evaluator" not in str(info.value)
    with pytest.raises(_lib.DpotHipError):
        infer.rollout_eval(m, xx, yy, None, evaluator=dpot_amd.RolloutEvaluator("cuda", n_channels=2, T_max=2))

    class Other:                                                   # written for [B,X,Y,T,C]: refused before the rollout
        def update(self, pred, target):
            raise AssertionError("never reached")
    with pytest.raises(ValueError, match="RolloutEvaluator"):
        infer.rollout_eval(m, xx, yy, None, evaluator=Other())


def test_abi_has_the_eval3_entry_points():
    from dpot_amd import _lib, ops
    lib = _lib.load()
    assert lib.dpot_version() >= 270
    assert lib.dpot_eval3_pad(41, 0) == 48 and lib.dpot_eval3_pad(41, 1) == 32
    assert lib.dpot_eval3_pad(128, 0) == 128 and lib.dpot_eval3_pad(128, 1) == 64
    assert lib.dpot_eval3_pad(2, 1) == 16 and lib.dpot_eval3_pad(0, 0) == 0
    limits = [lib.dpot_eval3_max_size(a) for a in range(3)]
    assert min(limits) >= 128                                      # 128^3: the raw resolution of the reference's 3-D data
    for shape in ((128, 128, 128, 1, 4), (6, 5, 7, 3, 2), (16, 300, 9, 1, 1)):
        assert lib.dpot_eval3_acc_elems(*shape) == ops.eval_acc_layout(*shape)[1]
    assert lib.dpot_eval3_acc_elems(8, 1, 8, 1, 1) == 0
    # the workspace of a batch: statistics partials, shell partials [B, TC, nz/2, stripes of 16 i, K], the half spectrum
    assert lib.dpot_eval3_work_elems(0, 2, 20, 33, 26, 3) % (2 * 3 * 8) == 0 and lib.dpot_eval3_work_elems(0, 2, 20, 33, 26, 3) > 0
    assert lib.dpot_eval3_work_elems(1, 2, 20, 33, 26, 3) == 2 * 3 * 13 * 1 * 10
    assert lib.dpot_eval3_work_elems(2, 2, 20, 33, 26, 3) == 2 * 3 * 13 * 2 * 20 * 33
    assert lib.dpot_eval3_work_elems(2, 1, 20, limits[1] + 1, 26, 3) == 0
    # argument checks run before any device work: a null field is refused, a size beyond the limit is "unsupported size"
    rc = lib.dpot_eval3_stats(*([None] * 12), 1, 8, 8, 8, 1, None)
    assert rc == -1 and b"eval3_stats" in lib.dpot_last_error()
    fake = 4096                                                    # never dereferenced: the size check comes first
    for axis in range(3):
        sizes = [16, 16, 16]
        sizes[axis] = limits[axis] + 1
        rc = lib.dpot_eval3_stats(*([fake] * 12), 1, *sizes, 1, None)
        assert rc == -2 and b"beyond the supported size" in lib.dpot_last_error()
        assert f"{sizes[0]}x{sizes[1]}x{sizes[2]}".encode() in lib.dpot_last_error()
        assert lib.dpot_eval3_finalize(fake, fake, fake, 1, *sizes, 1, 1, None) == -2


# ---- one host path for both ranks: what a plane and a field must agree on --------------------------------------------
RANK_SIZES = [(6, 5, 7), (9, 11, 10), (16, 16, 16), (17, 40, 12), (12, 10, 8), (33, 16, 48)]


@pytest.mark.parametrize("sizes", RANK_SIZES)
def test_shell_tables_of_both_ranks_agree_on_the_plane_k_equals_0(sizes):
    """k = 0 adds nothing to i^2 + j^2: the field's rows of k = 0 are the plane's, cut at the field's smaller K"""
    from dpot_amd import ops
    nx, ny, nz = sizes
    K3 = min(nx // 2, ny // 2, nz // 2)
    assert np.array_equal(ops.eval_shell_ranges(nx, ny, nz)[0], ops.eval_shell_ranges(nx, ny)[:, :K3 + 1])
    plane = ops.eval_shell_table(nx, ny)
    assert np.array_equal(ops.eval_shell_table(nx, ny, nz)[:, :, 0], np.where(plane >= K3, -1, plane))
    for bad in ((nx,), (nx, ny, nz, 4)):
        with pytest.raises(ValueError):
            ops.eval_shell_table(*bad)


@pytest.mark.parametrize("TC", [(1, 1), (3, 2), (10, 4)])
@pytest.mark.parametrize("sizes", RANK_SIZES)
def test_accumulator_layout_of_both_ranks_and_of_the_library(sizes, TC):
    from dpot_amd import _lib, ops
    lib = _lib.load()
    (nx, ny, nz), (T, C) = sizes, TC
    K2, K3 = min(nx // 2, ny // 2), min(nx // 2, ny // 2, nz // 2)
    (off2, total2), (off3, total3) = ops.eval_acc_layout(nx, ny, T, C), ops.eval_acc_layout(nx, ny, nz, T, C)
    assert off2 == off3 and total2 - total3 == T * C * (K2 - K3)
    assert lib.dpot_eval_metrics_acc_elems(nx, ny, T, C) == total2
    assert lib.dpot_eval3_acc_elems(nx, ny, nz, T, C) == total3


@pytest.mark.parametrize("sizes", [(6, 5, 8), (9, 11, 16), (16, 16, 16)])
def test_finish_of_both_ranks_differs_by_the_spectrum_divisor_alone(sizes):
    """the same words read as the accumulator of a field and of its plane (nx, ny), whose K is the field's (nz // 2 is not the
    smallest): fmse_* of the plane is nz times the field's, every other key is equal.  nz is a power of two, so the factor
    is exact in every rounding on the way (a / (nx ny nz) = (a / (nx ny)) / nz bit for bit, the band mean and the float32
    rounding commute with it)."""
    from dpot_amd import ops
    nx, ny, nz = sizes
    T, C, B = 3, 2, 5
    assert min(nx // 2, ny // 2) <= nz // 2 and nz & (nz - 1) == 0
    total = ops.eval_acc_layout(nx, ny, nz, T, C)[1]
    assert total == ops.eval_acc_layout(nx, ny, T, C)[1]
    acc = np.random.RandomState(nx * 100 + nz).uniform(0.5, 40.0, total)
    for ilow, ihigh in ((1, 2), (2, 5), (4, 12)):
        field = ops.eval_finish(acc, B, nx, ny, nz, T, C, ilow, ihigh)
        plane = ops.eval_finish(acc, B, nx, ny, T, C, ilow, ihigh)
        assert set(field) == set(plane) == set(ops.EVAL_KEYS) | {"samples"} and field["samples"] == plane["samples"] == B
        for key in ops.EVAL_KEYS:
            want = field[key] * np.float32(nz) if key.startswith("fmse_") else field[key]
            assert plane[key].dtype == np.float32 and np.array_equal(plane[key], want, equal_nan=True), (key, ilow, ihigh)
        assert np.isfinite(field["fmse_low"]).all() and (field["fmse_low"] > 0).all()
