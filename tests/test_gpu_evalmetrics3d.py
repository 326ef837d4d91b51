"""GPU tests of the 3-D evaluation metrics (csrc/evalmetrics3d.hip, ops.eval_metrics_update, dpot_amd.RolloutEvaluator on
[B, X, Y, Z, T, C] and the `evaluator=` argument of the 3-D rollouts): the fixture the reference wrote per component
(g20_evalmetrics3d, its float64 results), the float64 restatement (tests/eval3d_ref.py), determinism, guards, accumulation
over batches, graph replay, and the eager and graphed rollouts of a DPOTNet3D.  The op tests run on the guarded, poisoned
allocator (tests/guard.py)."""
import functools
import math

import numpy as np
import pytest
import torch

import eval3d_ref as E
import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close, load

pytestmark = pytest.mark.gpu

CASES = ["o6x5x7_t3c2", "e8_t10c4", "r10x12x9_t2c3", "r12x10x8_t1c1", "two_batches", "r20x33x26_t1c2", "e16_default", "big32",
         "big64"]
FIXTURE = "g20_evalmetrics3d"


def spectrum_allowance(nx, ny, nz, e_ref32):
    """what the kernel's spectrum keys may be off by, relative to float64 - spectrum_allowance of test_gpu_evalmetrics.py with
    one more axis: sqrt(terms of a dense pass / stages of an FFT) times the reference's own float32 error, or the random-walk
    rounding of the three dense passes' nx + ny + nz fp32 terms, sqrt(nx + ny + nz) 2^-23 - whichever is larger"""
    n = max(nx, ny, nz)
    return max(math.sqrt(n / math.log2(n)) * e_ref32, math.sqrt(nx + ny + nz) * 2.0 ** -23)


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
    ev = RolloutEvaluator("cuda", n_channels=shape[5], T_max=shape[4], ilow=ilow, ihigh=ihigh)
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
    assert [str(n) for n in load(FIXTURE)["names"]] == CASES


@pytest.mark.parametrize("name", CASES)
def test_evaluator_vs_reference_fixture(name, guarded):
    fx = load(FIXTURE)
    _, got, shape = run_case(fx, name)
    assert got["samples"] == shape[0]
    compare(got, {k: fx[f"{name}.{k}.r64"] for k in E.KEYS}, f"evaluator {name}")
    if name in ("o6x5x7_t3c2", "e16_default"):
        assert np.isnan(got["fmse_high"]).all()                    # the empty band


@pytest.mark.parametrize("name", CASES)
def test_evaluator_error_relative_to_the_reference_float32(name, guarded):
    """per key: the kernel's largest relative error against the reference's float64 result beside the same figure of the
    reference's own float32 run; the spectrum keys are held to spectrum_allowance"""
    fx = load(FIXTURE)
    _, got, shape = run_case(fx, name)
    for key in E.KEYS:
        r64 = fx[f"{name}.{key}.r64"]
        e_got, e_ref = rel_err(got[key], r64), rel_err(fx[f"{name}.{key}.r32"], r64)
        line = f"evalmetrics3d-error {name} {key}: kernel {e_got:.3e}  reference-fp32 {e_ref:.3e}"
        if key in E.SPECTRUM_KEYS:
            allowed = spectrum_allowance(shape[1], shape[2], shape[3], e_ref)
            print(f"{line}  allowed {allowed:.3e}")
            assert e_got <= allowed, (name, key, e_got, e_ref, allowed)
        else:
            print(line)


def fields(shape, salt, near):
    return E.hashed_pair(shape, salt) if near else E.independent_pair(shape, salt)


def bands_for(nx, ny, nz):
    K = min(nx // 2, ny // 2, nz // 2)
    return (4, 12) if K > 12 else (2, 5) if K > 5 else (1, 2)


@functools.lru_cache(maxsize=None)
def sweep_case(cube, B, TC):
    """inputs and the float64 restatement of one sweep case, computed once and shared (never modified)"""
    (nx, ny, nz), (T, C) = cube, TC
    p, t = fields((B, nx, ny, nz, T, C), 3 + B + T + C, near=(nx + B) % 2 == 0)
    ilow, ihigh = bands_for(nx, ny, nz)
    return p, t, ilow, ihigh, E.eval_ref(p, t, ilow, ihigh)


SWEEP = [(c, B, TC) for c in [(6, 5, 7), (8, 8, 8), (9, 11, 10), (16, 16, 16), (17, 40, 12), (33, 16, 48), (32, 32, 32)]
         for B in (1, 5) for TC in ((1, 1), (1, 3), (10, 4))] + [((64, 64, 64), 1, (1, 2)), ((64, 64, 64), 1, (1, 3))]


@pytest.mark.parametrize("cube,B,TC", SWEEP, ids=["x".join(map(str, c)) + f"-B{B}-T{TC[0]}C{TC[1]}" for c, B, TC in SWEEP])
def test_evaluator_vs_restatement(cube, B, TC, guarded):
    """an axis below one 16-tile, axes that are no multiple of 16, K limited by x, by y and by z in turn, the 16-byte and the
    scalar load path (T * C = 40 against 1 and 3), near-equal and independent fields alternating"""
    from dpot_amd import RolloutEvaluator
    p, t, ilow, ihigh, want = sweep_case(cube, B, TC)
    ev = RolloutEvaluator("cuda", n_channels=TC[1], T_max=max(TC[0], 12), ilow=ilow, ihigh=ihigh)
    ev.update(guard.wrap(torch.from_numpy(p), "cuda"), guard.wrap(torch.from_numpy(t), "cuda"))
    got = ev.read()
    assert got["samples"] == B
    compare(got, want, f"evaluator {cube} B={B} TC={TC}")


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_largest_supported_size_and_one_beyond(axis, guarded):
    from dpot_amd import RolloutEvaluator, _lib, ops
    lib = _lib.load()
    n_max = lib.dpot_eval3_max_size(axis)
    assert n_max >= 128
    sizes = [4, 6, 6]
    sizes[axis] = n_max
    p, t = fields((1, *sizes, 1, 2), 21 + axis, near=True)
    ev = RolloutEvaluator("cuda", n_channels=2, T_max=1, ilow=1, ihigh=2)
    ev.update(guard.wrap(torch.from_numpy(p), "cuda"), guard.wrap(torch.from_numpy(t), "cuda"))
    compare(ev.read(), E.eval_ref(p, t, 1, 2), f"evaluator {sizes}")
    # beyond: the wrapper refuses and names the size, and so does the library itself - with the "unsupported size" code and
    # without a launch
    sizes[axis] = n_max + 1
    big = torch.zeros(1, *sizes, 1, 1, device="cuda")
    with pytest.raises(_lib.DpotHipError, match=f"{sizes[0]} x {sizes[1]} x {sizes[2]}"):
        RolloutEvaluator("cuda", n_channels=1, T_max=1).update(big, big)
    d = ops.eval_plan(16, 16, 16, "cuda").dev
    statp = guard.full_nan((64,), dtype=torch.float64)
    specp, G = guard.full_nan((64,)), guard.full_nan((64,))
    rc = lib.dpot_eval3_stats(big.data_ptr(), big.data_ptr(), d["cxT"].data_ptr(), d["sxT"].data_ptr(), d["cy"].data_ptr(),
                              d["sy"].data_ptr(), d["czT"].data_ptr(), d["szT"].data_ptr(), d["jlo"].data_ptr(),
                              statp.data_ptr(), specp.data_ptr(), G.data_ptr(), 1, *sizes, 1, None)
    torch.cuda.synchronize()
    assert rc == -2 and b"beyond the supported size" in lib.dpot_last_error()
    assert statp.isnan().all() and specp.isnan().all() and G.isnan().all()          # nothing written
    guard.check()


@pytest.mark.parametrize("TC", [3, 4])
@pytest.mark.parametrize("cube", [(9, 11, 10), (17, 40, 12), (12, 17, 40), (32, 32, 32), (6, 10, 70)])
def test_update_is_deterministic_and_stays_inside_its_buffers(cube, TC, guarded):
    """two updates on equal inputs from equal (zero) accumulators give identical accumulator bits, twice more as well; the
    guards around the accumulator, the workspace and the tables are intact, ragged sizes (70: more than two k tiles)"""
    from dpot_amd import ops
    nx, ny, nz = cube
    p, t = fields((2, nx, ny, nz, 1, TC), 5, near=True)
    pd, td = guard.wrap(torch.from_numpy(p), "cuda"), guard.wrap(torch.from_numpy(t), "cuda")
    a1, a2 = ops.eval_acc_alloc(nx, ny, nz, 1, TC, "cuda"), ops.eval_acc_alloc(nx, ny, nz, 1, TC, "cuda")
    ops.eval_metrics_update(pd, td, a1)
    ops.eval_metrics_update(pd, td, a2)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2) and int(a1[0]) == 2
    ops.eval_metrics_update(pd, td, a1)
    ops.eval_metrics_update(pd, td, a2)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2) and int(a1[0]) == 4
    ilow, ihigh = bands_for(nx, ny, nz)
    got = ops.eval_finish(np.concatenate([[4.0], a1[1:].view(torch.float64).cpu().numpy()]), 4, nx, ny, nz, 1, TC, ilow, ihigh)
    compare(got, E.eval_ref(np.concatenate([p, p]), np.concatenate([t, t]), ilow, ihigh), f"accumulator {cube} TC={TC}")
    guard.check()


def test_accumulation_reset_and_read(guarded):
    from dpot_amd import RolloutEvaluator, _lib
    import eval_ref as E2
    fx = load(FIXTURE)
    ev, got, shape = run_case(fx, "two_batches")                   # update(2 samples), update(3 samples)
    assert [int(b) for b in fx["two_batches.batches"]] == [2, 3] and got["samples"] == 5
    compare(got, {k: fx[f"two_batches.{k}.r64"] for k in E.KEYS}, "two batches")
    before = ev.acc.clone()
    again = ev.read()
    assert torch.equal(ev.acc, before)                             # read() leaves the state alone
    for key in E.KEYS:
        assert np.array_equal(again[key], got[key], equal_nan=True)
    with pytest.raises(_lib.DpotHipError):                         # another shape between two resets
        ev.update(torch.zeros(1, 12, 12, 8, 2, 2, device="cuda"), torch.zeros(1, 12, 12, 8, 2, 2, device="cuda"))
    with pytest.raises(_lib.DpotHipError):                         # another rank between two resets
        ev.update(torch.zeros(1, 12, 10, 2, 2, device="cuda"), torch.zeros(1, 12, 10, 2, 2, device="cuda"))
    assert torch.equal(ev.acc, before)
    ev.reset()
    assert not ev.acc.any()
    (p, t), _ = E.case_fields(fx, "two_batches")
    ev.update(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda())
    il, ih = (int(v) for v in fx["two_batches.bands"])
    one = ev.read()
    assert one["samples"] == 2
    compare(one, E.eval_ref(p, t, il, ih), "after reset")
    # a 5-D batch after reset() on the same evaluator: the 2-D kernels, another accumulator
    ev.reset()
    p2, t2 = np.ascontiguousarray(p[:, :, :, 0]), np.ascontiguousarray(t[:, :, :, 0])
    ev.update(torch.from_numpy(p2).cuda(), torch.from_numpy(t2).cuda())
    flat = ev.read()
    assert flat["samples"] == 2
    want = E2.eval_ref(p2, t2, il, ih)
    for key in E.KEYS:
        assert np.array_equal(np.isnan(flat[key]), np.isnan(want[key])), key
        fin = ~np.isnan(want[key])
        assert_close(flat[key][fin], want[key][fin], f"5-D after reset {key}")


def test_zero_target_channel_follows_ieee(guarded):
    """a channel whose target is identically zero: inf, as the reference's division by a zero norm; the other channel and the
    keys without a target norm are untouched"""
    from dpot_amd import RolloutEvaluator
    p, t = fields((2, 8, 10, 12, 2, 2), 4, near=False)
    t = t.copy()
    t[..., 1] = 0.0
    ev = RolloutEvaluator("cuda", n_channels=2, T_max=2, ilow=1, ihigh=3)
    ev.update(guard.wrap(torch.from_numpy(p), "cuda"), guard.wrap(torch.from_numpy(t), "cuda"))
    got, want = ev.read(), E.eval_ref(p, t, 1, 3)
    for key in ("nmae", "nmse", "nmxe", "nmae_t", "nmse_t", "nmxe_t"):
        assert np.isposinf(got[key][..., 1]).all() and np.isposinf(want[key][..., 1]).all(), key
        assert_close(got[key][..., 0], want[key][..., 0], key)
    for key in ("bdmse", "fmse_low", "fmse_mid", "fmse_high"):
        assert_close(got[key], want[key], key)


@pytest.mark.parametrize("cube", [(9, 11, 10), (32, 32, 32)])
def test_update_under_graph_capture_replays_to_the_eager_bits(cube):
    from dpot_amd import RolloutEvaluator
    nx, ny, nz = cube
    p, t = (torch.from_numpy(a).cuda() for a in fields((3, nx, ny, nz, 2, 4), 11, near=True))
    ilow, ihigh = bands_for(nx, ny, nz)
    eager = RolloutEvaluator("cuda", n_channels=4, T_max=2, ilow=ilow, ihigh=ihigh)
    for _ in range(3):
        eager.update(p, t)
    ev = RolloutEvaluator("cuda", n_channels=4, T_max=2, ilow=ilow, ihigh=ihigh)
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
    compare(ev.read(), E.eval_ref(np.concatenate([p.cpu().numpy()] * 3), np.concatenate([t.cpu().numpy()] * 3), ilow, ihigh),
            f"graphed update {cube}")


# ---- the rollouts ---------------------------------------------------------------------------------------------------------
MODEL3D = dict(img_size=16, patch_size=4, in_channels=2, out_channels=2, in_timesteps=3, embed_dim=32, depth=2, n_blocks=2,
               modes=4)


@functools.lru_cache(maxsize=None)
def model3d():
    from dpot_amd import DPOTNet3D
    torch.manual_seed(2003)
    return DPOTNet3D(**MODEL3D).cuda().eval()


@pytest.mark.parametrize("B", [2, 3])
def test_rollouts_of_a_3d_model_with_an_evaluator(B):
    """GraphedRollout of a model whose forward returns one tensor reproduces the eager rollout bit for bit, as the 2-D test
    demands (B = 2: the whole batch, not its two samples unpacked into (pred, cls)); evaluator= changes nothing that is
    returned, and read() is the restatement applied to the returned prediction and yy"""
    from dpot_amd import RolloutEvaluator, StepMetrics
    from dpot_amd.infer import GraphedRollout, rollout_eval
    m, T_ar, S = model3d(), 3, MODEL3D["img_size"]
    xx = torch.from_numpy(E.independent_pair((B, S, S, S, 3, 2), 31 + B)[0]).cuda()
    yy = torch.from_numpy(E.independent_pair((B, S, S, S, T_ar, 2), 41 + B)[1]).cuda()
    msk = torch.ones(B, S, S, S, 1, 2, device="cuda")
    eager = rollout_eval(m, xx, yy, msk)
    assert tuple(eager[0].shape) == (B, S, S, S, T_ar, 2) and torch.isfinite(eager[0]).all()
    g = GraphedRollout(m, torch.zeros_like(xx))
    assert g.cls is None and tuple(g.im.shape) == (B, S, S, S, 1, 2)
    graphed = g(xx, yy, msk)
    for a, b in zip(eager, graphed):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        g(xx[:1], yy[:1], msk[:1])                                 # not the captured shape
    with pytest.raises(ValueError):
        g(xx, yy, msk, model_res=S)
    with pytest.raises(ValueError, match="model_res"):
        rollout_eval(m, xx, yy, msk, model_res=S)
    want = E.eval_ref(eager[0].cpu().numpy(), yy.cpu().numpy(), 2, 5)
    for run in (lambda **k: rollout_eval(m, xx, yy, msk, **k), lambda **k: g(xx, yy, msk, **k)):
        ev = RolloutEvaluator("cuda", n_channels=2, T_max=T_ar, ilow=2, ihigh=5)
        with_ev = run(evaluator=ev)
        for a, b in zip(eager, with_ev):
            assert torch.equal(a, b)
        got = ev.read()
        assert got["samples"] == B
        compare(got, want, f"3-D rollout evaluator B={B}")
        # with metrics= as well: the same returned values as with metrics= alone, the evaluator sees the second rollout
        met_a, met_b = StepMetrics("cuda", T_ar), StepMetrics("cuda", T_ar)
        only_met = run(metrics=met_a)
        both = run(metrics=met_b, evaluator=ev)
        for a, b in zip(only_met, both):
            assert torch.equal(a, b)
        assert torch.equal(met_a.acc, met_b.acc)
        twice = ev.read()
        assert twice["samples"] == 2 * B
        compare(twice, want, f"3-D rollout evaluator B={B}, two equal rollouts")     # means over equal samples


def test_one_evaluator_across_ranks(guarded):
    """planes, a field and the planes again through ONE evaluator: the plan and accumulator caches both ranks now share
    keep them apart (every read equals a fresh evaluator's on the same pair, the third the first), and a change of rank
    without reset() is refused"""
    import eval_ref as E2
    from dpot_amd import RolloutEvaluator, _lib
    from resize_ref import hash_field

    def pair(shape, salt):
        p, t = fields(shape, salt, near=True) if len(shape) == 6 else E2.hashed_pair(shape, salt, hash_field)
        return guard.wrap(torch.from_numpy(p), "cuda"), guard.wrap(torch.from_numpy(t), "cuda")

    def fresh(p, t):
        one = RolloutEvaluator("cuda", n_channels=2, T_max=3)
        one.update(p, t)
        return one.read()

    def same(a, b, what):
        assert a["samples"] == b["samples"] == 2, what
        for key in E.KEYS:
            assert np.array_equal(a[key], b[key], equal_nan=True), f"{what} {key}"

    plane, field = pair((2, 9, 11, 3, 2), 31), pair((2, 9, 11, 10, 3, 2), 32)
    ev = RolloutEvaluator("cuda", n_channels=2, T_max=3)
    ev.update(*plane)
    first = ev.read()
    same(first, fresh(*plane), "planes")
    with pytest.raises(_lib.DpotHipError):                         # a 6-D update without the reset() in between
        ev.update(*field)
    ev.reset()
    ev.update(*field)
    same(ev.read(), fresh(*field), "field")
    ev.reset()
    ev.update(*plane)
    third = ev.read()
    same(third, fresh(*plane), "planes again")
    same(third, first, "third against first")
    assert np.isfinite(first["nmse"]).all() and not np.array_equal(first["nmse"], fresh(*field)["nmse"])
    guard.check()
