"""CPU tests of the evaluation-metric feature (dpot_amd.RolloutEvaluator, csrc/evalmetrics.hip): the float64 restatement
against the fixture the reference wrote (g16_evalmetrics), the host tables the kernel reads (shell table, DFT tables), the
arithmetic of read() and its additivity over batches, the argument errors that need no GPU, and the ABI additions."""
import math

import numpy as np
import pytest
import torch

import eval_ref as E
from helpers import load

CASES = ["e16_default", "e16_t10c4", "o9x11_t3c2", "r12x10_t1c1", "two_batches", "big64", "big128"]


def whole(fx, name):
    pairs = E.case_fields(fx, name)
    return np.concatenate([p for p, _ in pairs]), np.concatenate([t for _, t in pairs])


def test_fixture_lists_the_cases_of_the_gpu_file_and_of_its_generator():
    import ast
    import os
    import test_gpu_evalmetrics as G
    names = [str(n) for n in load("g16_evalmetrics")["names"]]
    assert names == CASES == G.CASES
    # the generator's own table, read without importing it (it imports the reference)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts",
                            "make_golden_evalmetrics.py")).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and n.targets[0].id == "CASES")
    table = ast.literal_eval(node.value)
    assert list(table) == CASES
    fx = load("g16_evalmetrics")
    for name, (batches, nx, ny, T, C, ilow, ihigh, _) in table.items():
        assert tuple(fx[f"{name}.shape"]) == (sum(batches), nx, ny, T, C)
        assert tuple(fx[f"{name}.batches"]) == batches and tuple(fx[f"{name}.bands"]) == (ilow, ihigh)


@pytest.mark.parametrize("name", CASES)
def test_restatement_vs_reference_fixture(name):
    """float64 against float64 at 1e-10; NaN exactly where the reference has NaN"""
    fx = load("g16_evalmetrics")
    p, t = whole(fx, name)
    ilow, ihigh = (int(v) for v in fx[f"{name}.bands"])
    got = E.eval_ref(p, t, ilow, ihigh)
    for key in E.KEYS:
        want = fx[f"{name}.{key}.r64"]
        assert want.dtype == np.float64 and got[key].shape == want.shape, key
        assert np.array_equal(np.isnan(got[key]), np.isnan(want)), key
        fin = ~np.isnan(want)
        assert np.isfinite(want[fin]).all()
        assert (np.abs(got[key][fin] - want[fin]) <= 1e-10 * np.abs(want[fin])).all(), key
    K = min(p.shape[1] // 2, p.shape[2] // 2)
    assert np.isnan(fx[f"{name}.fmse_high.r64"]).all() == (K <= ihigh)
    assert not np.isnan(fx[f"{name}.fmse_low.r64"]).any() and not np.isnan(fx[f"{name}.fmse_mid.r64"]).any()


def test_fixture_has_an_empty_band_case():
    fx = load("g16_evalmetrics")
    assert np.isnan(fx["e16_default.fmse_high.r64"]).all() and np.isnan(fx["e16_default.fmse_high.r32"]).all()
    assert sum(np.isnan(fx[f"{n}.fmse_high.r64"]).any() for n in CASES) == 1


@pytest.mark.parametrize("sizes", [(9, 9), (16, 16), (41, 41), (128, 128), (256, 256), (9, 16), (41, 128), (256, 9)])
def test_shell_table_is_the_integer_square_root(sizes):
    from dpot_amd import ops
    nx, ny = sizes
    K = min(nx // 2, ny // 2)
    tab = ops.eval_shell_table(nx, ny)
    assert tab.shape == (nx // 2, ny // 2) and tab.dtype == np.int32
    for i in range(nx // 2):
        for j in range(ny // 2):
            s = math.isqrt(i * i + j * j)
            assert tab[i, j] == (s if s < K else -1), (i, j)
    # the range form the kernel walks describes the same table: row i, shell s = the j range [i, s] .. [i, s + 1]
    rng = ops.eval_shell_ranges(nx, ny)
    assert rng.shape == (nx // 2, K + 1) and rng.dtype == np.int32
    rebuilt = np.full_like(tab, -1)
    for i in range(nx // 2):
        assert rng[i, 0] == 0 and (np.diff(rng[i]) >= 0).all() and rng[i, K] <= ny // 2
        for s in range(K):
            rebuilt[i, rng[i, s]:rng[i, s + 1]] = s
    assert np.array_equal(rebuilt, tab)


@pytest.mark.parametrize("sizes", [(9, 11), (16, 16), (12, 10), (41, 59), (64, 128)])
def test_dft_tables_reproduce_fft2_on_the_positive_quadrant(sizes):
    from dpot_amd import ops
    nx, ny = sizes
    rs = np.random.RandomState(nx * 1000 + ny)
    e = rs.randn(nx, ny)
    cx, sx = ops.eval_dft_tables(nx)
    cy, sy = ops.eval_dft_tables(ny)
    assert cx.dtype == np.float64 and cx.shape == (nx // 2, nx) and sy.shape == (ny // 2, ny)
    P, Q = cx @ e, sx @ e
    re, im = P @ cy.T - Q @ sy.T, -(Q @ cy.T + P @ sy.T)
    want = np.fft.fft2(e)[:nx // 2, :ny // 2]
    scale = np.abs(want).max()
    assert np.abs(re - want.real).max() <= 1e-12 * scale and np.abs(im - want.imag).max() <= 1e-12 * scale
    # what the kernel receives: fp32, transposed where it wants them K-major, zero in the padding
    nxp, nyp, hxp, hyp = ops.EvalPlan.pads(nx, ny)
    assert (nxp % 16, nyp % 16, hxp % 16, hyp % 16) == (0, 0, 0, 0) and nxp >= nx and hyp >= ny // 2 and hxp - nx // 2 < 16
    h = ops.EvalPlan.host_tables(nx, ny)
    for key, full, used, src in (("cxT", (nxp, hxp), (nx, nx // 2), cx.T), ("sxT", (nxp, hxp), (nx, nx // 2), sx.T),
                                 ("cy", (nyp, hyp), (ny, ny // 2), cy.T), ("sy", (nyp, hyp), (ny, ny // 2), sy.T)):
        a = h[key]
        assert a.dtype == np.float32 and a.shape == full and np.isfinite(a).all(), key
        pad = np.ones(full, dtype=bool)
        pad[:used[0], :used[1]] = False
        assert not a[pad].any(), f"{key}: non-zero padding"
        assert np.array_equal(a[:used[0], :used[1]], src.astype(np.float32)), key
    assert np.array_equal(h["jlo"], ops.eval_shell_ranges(nx, ny)) and h["jlo"].flags["C_CONTIGUOUS"]


def acc_vector(sums, nx, ny, T, C):
    """tests/eval_ref.batch_sums laid out as the device accumulator (ops.eval_acc_layout)"""
    from dpot_amd import ops
    off, total = ops.eval_acc_layout(nx, ny, T, C)
    acc = np.zeros(total)
    acc[off["c"]:off["tc"]] = sums["c"].reshape(-1)
    acc[off["tc"]:off["spec"]] = sums["tc"].reshape(-1)
    acc[off["spec"]:] = sums["spec"].reshape(-1)
    return acc


@pytest.mark.parametrize("name", ["two_batches", "e16_default", "o9x11_t3c2"])
def test_read_arithmetic_and_batch_additivity(name):
    """the numpy model of read() (ops.eval_finish) on sums added over two batches equals the reference on the
    concatenation; shapes and dtypes are the reference's"""
    from dpot_amd import ops
    fx = load("g16_evalmetrics")
    p, t = whole(fx, name)
    B, nx, ny, T, C = p.shape
    ilow, ihigh = (int(v) for v in fx[f"{name}.bands"])
    cut = 1 if B < 3 else 2
    s = E.add_sums(E.batch_sums(p[:cut], t[:cut]), E.batch_sums(p[cut:], t[cut:]))
    assert s["count"] == B
    got = ops.eval_finish(acc_vector(s, nx, ny, T, C), B, nx, ny, T, C, ilow, ihigh)
    assert got["samples"] == B and set(got) == set(E.KEYS) | {"samples"} and set(ops.EVAL_KEYS) == set(E.KEYS)
    shapes = {"nmae": (1, C), "nmse": (1, C), "nmxe": (1, C), "nmae_t": (1, T, C), "nmse_t": (1, T, C), "nmxe_t": (1, T, C),
              "bdmse": (C, T), "fmse_low": (T, C), "fmse_mid": (T, C), "fmse_high": (T, C)}
    for key in E.KEYS:
        want = fx[f"{name}.{key}.r64"]
        assert got[key].dtype == np.float32 and got[key].shape == shapes[key] == want.shape, key
        assert np.array_equal(np.isnan(got[key]), np.isnan(want)), key
        fin = ~np.isnan(want)
        assert (np.abs(got[key][fin] - want[fin]) <= 2.0 ** -23 * np.abs(want[fin])).all(), key     # one fp32 rounding
    with pytest.raises(ValueError):
        ops.eval_finish(np.zeros(3), 1, nx, ny, T, C)
    none = ops.eval_finish(np.zeros(ops.eval_acc_layout(nx, ny, T, C)[1]), 0, nx, ny, T, C, ilow, ihigh)
    assert none["samples"] == 0 and np.isnan(none["nmae"]).all()


def test_cpu_tensors_and_bad_arguments_raise():
    """no CPU fallback: the evaluator and the op refuse CPU tensors and a CPU device; shape rules are host-side checks"""
    import dpot_amd
    from dpot_amd import RolloutEvaluator, _lib, ops
    assert dpot_amd.RolloutEvaluator is RolloutEvaluator and "RolloutEvaluator" in dpot_amd.__all__
    with pytest.raises(_lib.DpotHipError):
        RolloutEvaluator("cpu", n_channels=2, T_max=3)
    for kw in (dict(n_channels=0, T_max=1), dict(n_channels=1, T_max=0), dict(n_channels=1, T_max=1, ilow=5, ihigh=4),
               dict(n_channels=1, T_max=1, ilow=-1)):
        with pytest.raises(ValueError):
            RolloutEvaluator("cuda", **kw)
    ev = RolloutEvaluator("cuda", n_channels=2, T_max=3)
    z = torch.zeros(1, 8, 8, 3, 2)
    with pytest.raises(_lib.DpotHipError):
        ev.update(z, z)                                            # CPU tensors
    with pytest.raises(_lib.DpotHipError):
        ev.update(torch.zeros(1, 8, 8, 4, 2), torch.zeros(1, 8, 8, 4, 2))      # T > T_max
    with pytest.raises(_lib.DpotHipError):
        ev.update(torch.zeros(1, 8, 8, 3, 3), torch.zeros(1, 8, 8, 3, 3))      # another channel count
    with pytest.raises(_lib.DpotHipError):
        ev.update(z, torch.zeros(1, 8, 9, 3, 2))                   # shapes differ
    with pytest.raises(_lib.DpotHipError):
        ev.read()                                                  # nothing to read
    with pytest.raises(_lib.DpotHipError):
        ops.eval_metrics_update(z, z, torch.zeros(4, dtype=torch.int64))
    model = dpot_amd.DPOTNet(**__import__("oracle.dpot_ref", fromlist=["MINI"]).MINI)
    with pytest.raises(Exception):
        dpot_amd.rollout_eval(model, torch.zeros(1, 32, 32, 4, 3), torch.zeros(1, 32, 32, 2, 3), None, evaluator=ev)


def test_abi_has_the_eval_metrics_entry_points():
    from dpot_amd import _lib, ops
    lib = _lib.load()
    assert lib.dpot_version() >= 265
    assert lib.dpot_eval_metrics_pad(41, 0) == 48 and lib.dpot_eval_metrics_pad(41, 1) == 32
    assert lib.dpot_eval_metrics_pad(128, 0) == 128 and lib.dpot_eval_metrics_pad(128, 1) == 64
    assert lib.dpot_eval_metrics_pad(2, 1) == 16 and lib.dpot_eval_metrics_pad(0, 0) == 0
    ny_max = lib.dpot_eval_metrics_max_size(1)
    assert ny_max >= 256 and lib.dpot_eval_metrics_max_size(0) >= 256
    for shape in ((128, 128, 10, 4), (9, 11, 3, 2), (16, 300, 1, 1)):
        assert lib.dpot_eval_metrics_acc_elems(*shape) == ops.eval_acc_layout(*shape)[1]
    # argument checks run before any device work: a null field is refused, a plane beyond the limit is "unsupported size"
    rc = lib.dpot_eval_metrics_stats(None, None, None, None, None, None, None, None, None, 1, 8, 8, 1, None)
    assert rc == -1 and b"eval_metrics_stats" in lib.dpot_last_error()
    fake = 4096                                                    # never dereferenced: the size check comes first
    rc = lib.dpot_eval_metrics_stats(*([fake] * 9), 1, 16, ny_max + 1, 1, None)
    assert rc == -2 and b"beyond the supported size" in lib.dpot_last_error()
    rc = lib.dpot_eval_metrics_finalize(fake, fake, fake, 1, 16, ny_max + 1, 1, 1, None)
    assert rc == -2
