"""GPU tests of the evaluation metrics (csrc/evalmetrics.hip, ops.eval_metrics_update, dpot_amd.RolloutEvaluator and the
`evaluator=` argument of the rollouts): the fixture the reference wrote (g16_evalmetrics, its float64 results), the float64
restatement (tests/eval_ref.py), determinism, guards, accumulation over batches, graph replay, and the rollouts.  The op
tests run on the guarded, poisoned allocator (tests/guard.py)."""
import math

import numpy as np
import pytest
import torch

import eval_ref as E
import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close, load
from oracle import dpot_ref as R
from resize_ref import hash_field

pytestmark = pytest.mark.gpu

CASES = ["e16_default", "e16_t10c4", "o9x11_t3c2", "r12x10_t1c1", "two_batches", "big64", "big128"]


def spectrum_allowance(nx, ny, e_ref32):
    """what the kernel's spectrum keys may be off by, relative to float64: sqrt(terms of a dense pass / stages of an FFT)
    times the reference's own float32 error (the rule of test_gpu_resize.ERR_FACTOR, per size), or the random-walk rounding
    of the two dense passes' nx + ny fp32 terms, sqrt(nx + ny) 2^-23 - whichever is larger"""
    n = max(nx, ny)
    return max(math.sqrt(n / math.log2(n)) * e_ref32, math.sqrt(nx + ny) * 2.0 ** -23)


def rel_err(a, ref):
    """largest element-wise relative error over the finite entries of ref (0.0 if there are none)"""
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64)[fin] - ref[fin]) / np.abs(ref[fin])))


def run_case(fx, name):
    from dpot_amd import RolloutEvaluator
    shape = tuple(int(s) for s in fx[f"{name}.shape"])
    ilow, ihigh = (int(v) for v in fx[f"{name}.bands"])
    ev = RolloutEvaluator("cuda", n_channels=shape[4], T_max=shape[3], ilow=ilow, ihigh=ihigh)
    for p, t in E.case_fields(fx, name):
        ev.update(guard.wrap(torch.from_numpy(p), "cuda"), guard.wrap(torch.from_numpy(t), "cuda"))
    return ev, ev.read(), shape


def compare(got, want, what):
    """every key: NaN exactly where `want` has NaN (checked explicitly), the rest at the parity tolerance"""
    for key in E.KEYS:
        g, w = got[key], np.asarray(want[key], dtype=np.float64)
        assert g.dtype == np.float32 and g.shape == w.shape, f"{what} {key}: {g.dtype} {g.shape} vs {w.shape}"
        assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what} {key}: NaN pattern differs"
        fin = ~np.isnan(w)
        if fin.any():
            assert_close(g[fin], w[fin], f"{what} {key}")


def test_fixture_lists_the_cases_of_this_file():
    assert [str(n) for n in load("g16_evalmetrics")["names"]] == CASES


@pytest.mark.parametrize("name", CASES)
def test_evaluator_vs_reference_fixture(name, guarded):
    fx = load("g16_evalmetrics")
    _, got, shape = run_case(fx, name)
    assert got["samples"] == shape[0]
    compare(got, {k: fx[f"{name}.{k}.r64"] for k in E.KEYS}, f"evaluator {name}")
    if name == "e16_default":
        assert np.isnan(got["fmse_high"]).all()                    # the empty band


@pytest.mark.parametrize("name", CASES)
def test_evaluator_error_relative_to_the_reference_float32(name, guarded):
    """per key: the kernel's largest relative error against the reference's float64 result beside the same figure of the
    reference's own float32 run; the spectrum keys are held to spectrum_allowance"""
    fx = load("g16_evalmetrics")
    _, got, shape = run_case(fx, name)
    for key in E.KEYS:
        r64 = fx[f"{name}.{key}.r64"]
        e_got, e_ref = rel_err(got[key], r64), rel_err(fx[f"{name}.{key}.r32"], r64)
        line = f"evalmetrics-error {name} {key}: kernel {e_got:.3e}  reference-fp32 {e_ref:.3e}"
        if key in E.SPECTRUM_KEYS:
            allowed = spectrum_allowance(shape[1], shape[2], e_ref)
            print(f"{line}  allowed {allowed:.3e}")
            assert e_got <= allowed, (name, key, e_got, e_ref, allowed)
        else:
            print(line)


def fields(shape, salt, near):
    if near:
        return E.hashed_pair(shape, salt, hash_field)
    return hash_field(shape, 2 * salt), hash_field(shape, 2 * salt + 1) + np.float32(0.25)


def bands_for(nx, ny):
    return (4, 12) if min(nx // 2, ny // 2) > 12 else (2, 5)


@pytest.mark.parametrize("TC", [(1, 1), (1, 3), (10, 4)])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("plane", [(16, 16), (41, 41), (59, 113), (64, 64), (128, 128), (33, 48)])
def test_evaluator_vs_restatement(plane, B, TC, guarded):
    from dpot_amd import RolloutEvaluator
    (nx, ny), (T, C) = plane, TC
    p, t = fields((B, nx, ny, T, C), 3 + B + T + C, near=(nx + B) % 2 == 0)
    ilow, ihigh = bands_for(nx, ny)
    ev = RolloutEvaluator("cuda", n_channels=C, T_max=max(T, 12), ilow=ilow, ihigh=ihigh)
    ev.update(guard.wrap(torch.from_numpy(p), "cuda"), guard.wrap(torch.from_numpy(t), "cuda"))
    got = ev.read()
    assert got["samples"] == B
    compare(got, E.eval_ref(p, t, ilow, ihigh), f"evaluator {plane} B={B} TC={TC}")


def test_default_bands_on_a_small_plane_give_nan_and_nothing_else_does(guarded):
    from dpot_amd import RolloutEvaluator
    p, t = fields((2, 16, 16, 2, 3), 9, near=False)
    ev = RolloutEvaluator("cuda", n_channels=3, T_max=2)
    ev.update(guard.wrap(torch.from_numpy(p), "cuda"), guard.wrap(torch.from_numpy(t), "cuda"))
    got = ev.read()
    assert np.isnan(got["fmse_high"]).all()
    for key in E.KEYS:
        if key != "fmse_high":
            assert np.isfinite(got[key]).all(), key
    compare(got, E.eval_ref(p, t), "default bands at 16 x 16")


def test_largest_supported_plane_and_one_beyond(guarded):
    from dpot_amd import RolloutEvaluator, _lib, ops
    lib = _lib.load()
    ny_max = lib.dpot_eval_metrics_max_size(1)
    assert ny_max >= 256
    p, t = fields((1, 40, ny_max, 1, 2), 21, near=True)
    ev = RolloutEvaluator("cuda", n_channels=2, T_max=1)
    ev.update(guard.wrap(torch.from_numpy(p), "cuda"), guard.wrap(torch.from_numpy(t), "cuda"))
    compare(ev.read(), E.eval_ref(p, t), f"evaluator 40 x {ny_max}")
    # beyond: the wrapper refuses, and so does the library itself - with the "unsupported size" code and without a launch
    big = torch.zeros(1, 16, ny_max + 1, 1, 1, device="cuda")
    with pytest.raises(_lib.DpotHipError):
        RolloutEvaluator("cuda", n_channels=1, T_max=1).update(big, big)
    d = ops.eval_plan(16, 16, "cuda").dev
    statp = guard.full_nan((64,), dtype=torch.float64)
    specp = guard.full_nan((64,))
    rc = lib.dpot_eval_metrics_stats(big.data_ptr(), big.data_ptr(), d["cxT"].data_ptr(), d["sxT"].data_ptr(),
                                     d["cy"].data_ptr(), d["sy"].data_ptr(), d["jlo"].data_ptr(), statp.data_ptr(),
                                     specp.data_ptr(), 1, 16, ny_max + 1, 1, None)
    torch.cuda.synchronize()
    assert rc == -2 and b"beyond the supported size" in lib.dpot_last_error()
    assert statp.isnan().all() and specp.isnan().all()             # nothing written
    guard.check()


@pytest.mark.parametrize("TC", [3, 4])
@pytest.mark.parametrize("plane", [(41, 41), (59, 113), (113, 59), (128, 128), (10, 256)])
def test_update_is_deterministic_and_stays_inside_its_buffers(plane, TC, guarded):
    """two updates on equal inputs from equal (zero) accumulators give identical accumulator bits, twice more as well; the
    guards around the accumulator, the workspace and the tables are intact, ragged sizes"""
    from dpot_amd import ops
    nx, ny = plane
    p, t = fields((2, nx, ny, 1, TC), 5, near=True)
    pd, td = guard.wrap(torch.from_numpy(p), "cuda"), guard.wrap(torch.from_numpy(t), "cuda")
    a1, a2 = ops.eval_acc_alloc(nx, ny, 1, TC, "cuda"), ops.eval_acc_alloc(nx, ny, 1, TC, "cuda")
    ops.eval_metrics_update(pd, td, a1)
    ops.eval_metrics_update(pd, td, a2)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2) and int(a1[0]) == 2
    ops.eval_metrics_update(pd, td, a1)
    ops.eval_metrics_update(pd, td, a2)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2) and int(a1[0]) == 4
    ilow, ihigh = bands_for(nx, ny)
    got = ops.eval_finish(np.concatenate([[4.0], a1[1:].view(torch.float64).cpu().numpy()]), 4, nx, ny, 1, TC, ilow, ihigh)
    compare(got, E.eval_ref(np.concatenate([p, p]), np.concatenate([t, t]), ilow, ihigh), f"accumulator {plane} TC={TC}")
    guard.check()


def test_accumulation_reset_and_read(guarded):
    from dpot_amd import RolloutEvaluator, _lib
    fx = load("g16_evalmetrics")
    ev, got, shape = run_case(fx, "two_batches")                   # update(2 samples), update(3 samples)
    assert [int(b) for b in fx["two_batches.batches"]] == [2, 3] and got["samples"] == 5
    compare(got, {k: fx[f"two_batches.{k}.r64"] for k in E.KEYS}, "two batches")
    before = ev.acc.clone()
    again = ev.read()
    assert torch.equal(ev.acc, before)                             # read() leaves the state alone
    for key in E.KEYS:
        assert np.array_equal(again[key], got[key], equal_nan=True)
    with pytest.raises(_lib.DpotHipError):                         # another shape between two resets
        ev.update(torch.zeros(1, 12, 12, 2, 2, device="cuda"), torch.zeros(1, 12, 12, 2, 2, device="cuda"))
    ev.reset()
    assert not ev.acc.any()
    (p, t), _ = E.case_fields(fx, "two_batches")
    ev.update(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda())
    il, ih = (int(v) for v in fx["two_batches.bands"])
    one = ev.read()
    assert one["samples"] == 2
    compare(one, E.eval_ref(p, t, il, ih), "after reset")


def test_zero_target_channel_follows_ieee(guarded):
    """a channel whose target is identically zero: inf (or NaN where the prediction is zero too), as the reference's
    division by a zero norm; the other channel and the keys without a target norm are untouched"""
    from dpot_amd import RolloutEvaluator
    p, t = fields((2, 16, 16, 2, 2), 4, near=False)
    t[..., 1] = 0.0
    ev = RolloutEvaluator("cuda", n_channels=2, T_max=2, ilow=2, ihigh=5)
    ev.update(guard.wrap(torch.from_numpy(p), "cuda"), guard.wrap(torch.from_numpy(t), "cuda"))
    got, want = ev.read(), E.eval_ref(p, t, 2, 5)
    for key in ("nmae", "nmse", "nmxe", "nmae_t", "nmse_t", "nmxe_t"):
        assert np.isposinf(got[key][..., 1]).all() and np.isposinf(want[key][..., 1]).all(), key
        assert_close(got[key][..., 0], want[key][..., 0], key)
    for key in ("bdmse", "fmse_low", "fmse_mid", "fmse_high"):
        assert_close(got[key], want[key], key)


@pytest.mark.parametrize("plane", [(41, 41), (64, 64)])
def test_update_under_graph_capture_replays_to_the_eager_bits(plane):
    from dpot_amd import RolloutEvaluator
    nx, ny = plane
    p, t = (torch.from_numpy(a).cuda() for a in fields((3, nx, ny, 2, 4), 11, near=True))
    eager = RolloutEvaluator("cuda", n_channels=4, T_max=2)
    for _ in range(3):
        eager.update(p, t)
    ev = RolloutEvaluator("cuda", n_channels=4, T_max=2)
    ev.update(p, t)                                                # tables, workspace and accumulator: outside the capture
    ev.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ev.update(p, t)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert int(ev.acc[0]) == 3 * p.shape[0] and torch.equal(ev.acc, eager.acc)      # three replays of one batch
    compare(ev.read(), E.eval_ref(np.concatenate([p.cpu().numpy()] * 3), np.concatenate([t.cpu().numpy()] * 3)),
            f"graphed update {plane}")


# ---- the rollouts ---------------------------------------------------------------------------------------------------------
MODEL64 = dict(R.MINI, img_size=64)


def build(kw, salt):
    from dpot_amd import DPOTNet
    cfg = R.DPOTConfig(**kw)
    m = DPOTNet(**kw)
    m.load_state_dict(R.recipe_state_dict(cfg, salt=salt))
    return m.cuda().eval(), cfg


@pytest.mark.parametrize("res", [None, 41])
def test_rollouts_with_an_evaluator(res):
    """evaluator= changes nothing that is returned (bit for bit), and read() is the restatement applied to the returned
    prediction and yy: eager and graphed, with and without model_res=, with and without metrics="""
    from dpot_amd import RolloutEvaluator, StepMetrics
    from dpot_amd.infer import GraphedRollout, rollout_eval
    m, cfg = build(R.MINI if res is None else MODEL64, salt=2)
    B, T_ar, S = 3, 3, cfg.img_size
    D = S if res is None else res
    kw = {} if res is None else {"model_res": S}
    xx = R.recipe_input((B, D, D, cfg.in_timesteps, cfg.in_channels), salt=5).cuda()
    yy = R.recipe_input((B, D, D, T_ar, cfg.out_channels), salt=6).cuda()
    msk = torch.ones(B, D, D, 1, cfg.out_channels, device="cuda")
    g = GraphedRollout(m, torch.zeros(B, S, S, cfg.in_timesteps, cfg.in_channels, device="cuda"))
    for run in (lambda **k: rollout_eval(m, xx, yy, msk, **kw, **k), lambda **k: g(xx, yy, msk, **kw, **k)):
        plain = run()
        ev = RolloutEvaluator("cuda", n_channels=cfg.out_channels, T_max=T_ar)
        with_ev = run(evaluator=ev)
        for a, b in zip(plain, with_ev):
            assert torch.equal(a, b)
        got = ev.read()
        assert got["samples"] == B
        want = E.eval_ref(with_ev[0].cpu().numpy(), yy.cpu().numpy())
        compare(got, want, f"rollout evaluator res={res}")
        # with metrics= as well: the same returned values as with metrics= alone, the evaluator sees the second rollout
        met_a, met_b = StepMetrics("cuda", T_ar), StepMetrics("cuda", T_ar)
        only_met = run(metrics=met_a)
        both = run(metrics=met_b, evaluator=ev)
        for a, b in zip(only_met, both):
            assert torch.equal(a, b)
        assert torch.equal(met_a.acc, met_b.acc)
        twice = ev.read()
        assert twice["samples"] == 2 * B
        compare(twice, want, f"rollout evaluator res={res}, two equal rollouts")     # means over equal samples
