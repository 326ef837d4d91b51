"""GPU tests of the 3-D Fourier resize (csrc/resize3.hip, ops.spectral_resize3) and of the resolution wrapper
(infer.Resized3D under rollout_eval and GraphedRollout): the float64 rfftn restatement (tests/resize3_ref.py), the error
beside a float32 torch.fft run, determinism, guards, argument checks, graph replay, and the wrapped rollouts of a DPOTNet3D
and an FNO3d against the loop written out by hand.  The op tests run on the guarded, poisoned allocator (tests/guard.py):
the workspace of every call is such a buffer too."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import afno3d_ref as A3
import fno3d_ref as FR
import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close
from resize3_ref import resize3_ref, resize3_torch
from resize_ref import hash_field
from test_gpu_resize import ERR_FACTOR

pytestmark = pytest.mark.gpu

# the smallest tuples that reach every parity pattern, both directions, the two-term pairs on each axis, and more than one
# 16- and 32-row tile
SIZES = [((8, 8, 8), (5, 5, 5)), ((5, 6, 7), (8, 8, 8)), ((16, 16, 16), (8, 8, 8)), ((8, 8, 8), (16, 16, 16)),
         ((8, 8, 8), (8, 8, 8)), ((10, 12, 6), (16, 14, 9)), ((6, 10, 12), (9, 16, 7)), ((33, 20, 18), (34, 17, 24))]
IDS = ["x".join(map(str, n)) + "-" + "x".join(map(str, m)) for n, m in SIZES]


@functools.lru_cache(maxsize=None)
def case(n, m, B, TC):
    """(input, float64 restatement), computed once and shared; no test writes to either"""
    xh = hash_field((B,) + n + ((10, 4) if TC == 40 else (TC,)), 7 + TC + B)
    return xh, resize3_ref(xh, m)


@pytest.mark.parametrize("TC", [1, 3, 4, 40])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n,m", SIZES, ids=IDS)
def test_resize3_vs_restatement(n, m, B, TC, guarded):
    from dpot_amd import ops
    xh, want = case(n, m, B, TC)
    x = guard.wrap(torch.from_numpy(xh), "cuda")
    got = ops.spectral_resize3(x, m)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B,) + m + xh.shape[4:]
    assert_close(got, want, f"spectral_resize3 {n} -> {m} B={B} TC={TC}")


@pytest.mark.parametrize("n,m", SIZES, ids=IDS)
def test_resize3_error_relative_to_a_float32_fft(n, m, guarded):
    """norm-wise error against the float64 restatement, beside the same figure of the restatement run in float32 torch.fft on
    the CPU; the kernel is allowed the ERR_FACTOR multiple of that figure the 2-D kernel is allowed (test_gpu_resize.py)"""
    from dpot_amd import ops
    xh, y64 = case(n, m, 2, 4)
    y32 = resize3_torch(torch.from_numpy(xh), m).double().numpy()
    got = ops.spectral_resize3(guard.wrap(torch.from_numpy(xh), "cuda"), m).double().cpu().numpy()
    assert np.isfinite(got).all()
    e_ref = np.linalg.norm(y32 - y64) / np.linalg.norm(y64)
    e_got = np.linalg.norm(got - y64) / np.linalg.norm(y64)
    print(f"resize3-error {n} -> {m}: kernel {e_got:.3e}  torch.fft-fp32 {e_ref:.3e}  ratio {e_got / e_ref:.2f} "
          f"(allowed {ERR_FACTOR:.2f})")
    assert e_got <= ERR_FACTOR * e_ref, (n, m, e_got, e_ref)


@pytest.mark.parametrize("TC", [3, 4])
@pytest.mark.parametrize("n,m", [((33, 20, 18), (34, 17, 24)), ((34, 17, 24), (33, 20, 18)), ((16, 16, 16), (8, 8, 8)),
                                 ((10, 12, 6), (16, 14, 9)), ((9, 16, 7), (6, 10, 12))])
def test_resize3_is_deterministic_and_stays_inside_its_output(n, m, TC, guarded):
    """two launches give identical bits; out= into a guarded NaN slot is written completely, correctly, and nothing around it
    or around the workspace is touched (the guards are checked here and at teardown), ragged sizes in both pass orders"""
    from dpot_amd import ops
    B = 2
    xh = hash_field((B,) + n + (1, TC), 3)
    x = guard.wrap(torch.from_numpy(xh), "cuda")
    out1 = guard.full_nan((B,) + m + (1, TC))
    out2 = guard.full_nan((B,) + m + (1, TC))
    r1 = ops.spectral_resize3(x, m, out=out1)
    r2 = ops.spectral_resize3(x, m, out=out2)
    torch.cuda.synchronize()
    assert r1 is out1 and r2 is out2
    assert torch.equal(out1.view(torch.int32), out2.view(torch.int32))
    assert_close(out1, resize3_ref(xh, m), f"spectral_resize3 {n} -> {m} TC={TC} into out=")
    guard.check()


def test_resize3_argument_checks():
    from dpot_amd import _lib, ops
    x = torch.zeros(2, 8, 8, 8, 1, 2, device="cuda")
    with pytest.raises(_lib.DpotHipError, match="out must be"):
        ops.spectral_resize3(x, 6, out=torch.zeros(2, 6, 6, 5, 1, 2, device="cuda"))
    with pytest.raises(_lib.DpotHipError, match=">= 2"):
        ops.spectral_resize3(x, (6, 1, 6))
    with pytest.raises(_lib.DpotHipError, match=">= 2"):
        ops.spectral_resize3(torch.zeros(1, 8, 1, 8, 2, device="cuda"), 6)
    with pytest.raises(_lib.DpotHipError, match="float32"):
        ops.spectral_resize3(x.double(), 6)
    with pytest.raises(_lib.DpotHipError, match="contiguous"):
        ops.spectral_resize3(x.permute(0, 2, 1, 3, 4, 5)[:, ::2], 6)
    with pytest.raises(_lib.DpotHipError, match="alias"):
        ops.spectral_resize3(x, 8, out=x)
    with pytest.raises(_lib.DpotHipError, match=r"\[B, X, Y, Z"):
        ops.spectral_resize3(x[0, 0], 6)
    cap = _lib.load().dpot_spectral_resize3_max_size()
    assert cap >= 128
    for axis in range(3):                                         # one past the limit, on either side: the error names the size
        big = [2, 2, 2]
        big[axis] = cap + 1
        with pytest.raises(_lib.DpotHipError, match=str(cap + 1)):
            ops.spectral_resize3(torch.zeros(1, *big, 1, device="cuda"), 4)
        with pytest.raises(_lib.DpotHipError, match=str(cap + 1)):
            ops.spectral_resize3(torch.zeros(1, 4, 4, 4, 1, device="cuda"), tuple(big))
    # the C side on its own: DPOT_EUNSUP beyond the limit, nothing launched
    lib = _lib.load()
    p = x.data_ptr()
    rc = lib.dpot_spectral_resize3(p, p + 64, p, p, p, p, None, None, None, None, None, 1, 8, 8, cap + 1, 8, 8, 8, 1, None)
    assert rc == -2 and str(cap + 1).encode() in lib.dpot_last_error()


@pytest.mark.parametrize("n,m", [((10, 12, 6), (16, 14, 9)), ((16, 16, 16), (8, 8, 8))])
def test_resize3_under_graph_capture_replays_to_the_eager_bits(n, m):
    from dpot_amd import ops
    x = torch.from_numpy(hash_field((2,) + n + (2, 4), 11)).cuda()
    eager = ops.spectral_resize3(x, m)                      # builds the plan outside the capture
    static_out = torch.full_like(eager, float("nan"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.spectral_resize3(x, m, out=static_out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out.view(torch.int32), eager.view(torch.int32))
    x.copy_(torch.from_numpy(hash_field((2,) + n + (2, 4), 12)))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out.view(torch.int32), ops.spectral_resize3(x, m).view(torch.int32))


def test_resize3_capture_without_a_plan_raises(monkeypatch):
    """a size tuple first seen while the stream captures: an error that says what to do, before anything is uploaded (the
    capture state is stubbed: aborting a real capture is not something a test should leave behind)"""
    from dpot_amd import _lib, ops
    n, m = (7, 9, 11), (11, 7, 9)                           # a tuple no other test uses: no plan yet
    x = torch.zeros((1,) + n + (4,), device="cuda")
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(_lib.DpotHipError, match="before capturing"):
            ops.spectral_resize3(x, m)
        with pytest.raises(_lib.DpotHipError, match="before capturing"):
            ops.resize3_plan(*n, *m, "cuda")
    plan = ops.resize3_plan(*n, *m, "cuda")                 # built outside a capture it works, and is cached
    assert plan is ops.resize3_plan(*n, *m, x.device) and plan.terms == 1
    assert_close(ops.spectral_resize3(x + 1.0, m), np.ones((1,) + m + (4,)), "a constant field stays constant")


# ---- the wrapper ----------------------------------------------------------------------------------------------------------
DATA = (6, 10, 12)                                          # non-cubic, every axis another size than the models' grids


@functools.lru_cache(maxsize=None)
def dpot3d():
    from dpot_amd import DPOTNet3D
    m = DPOTNet3D(**A3.MINI3D)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())
    m.load_state_dict(A3.recipe_sd(shapes, A3.MINI3D["n_blocks"], 176))
    return m.cuda().eval(), A3.MINI3D["img_size"], A3.MINI3D["in_timesteps"], A3.MINI3D["in_channels"]


@functools.lru_cache(maxsize=None)
def fno3d():
    from dpot_amd import FNO3d
    cfg = FR.MINI1
    m = FNO3d(**cfg)
    m.load_state_dict(FR.recipe_sd(OrderedDict((k, (tuple(v.shape), v.dtype)) for k, v in m.state_dict().items()), 1810),
                      strict=True)
    return m.cuda().eval(), cfg["img_size"], cfg["in_timesteps"], cfg["n_channels"]


def windows(T, C, B=2, T_ar=3):
    xx = torch.from_numpy(hash_field((B,) + DATA + (T, C), 51)).cuda()
    yy = torch.from_numpy(hash_field((B,) + DATA + (T_ar, C), 52)).cuda()
    msk = torch.ones((B,) + DATA + (1, C), device="cuda")
    msk[1, ..., 1] = 0.0                                    # one masked-out channel
    return xx, yy, msk


@torch.no_grad()
def by_hand(m, S, xx, yy, msk):
    """rollout_eval's loop written out with ops.spectral_resize3 around the model"""
    from dpot_amd import ops
    from dpot_amd.functional import rel_l2_loss
    loss, preds = None, []
    for t in range(yy.shape[-2]):
        im = ops.spectral_resize3(m(ops.spectral_resize3(xx, S)).contiguous(), DATA)
        l = rel_l2_loss(im, yy[..., t:t + 1, :].contiguous(), msk)
        loss = l if loss is None else loss + l
        preds.append(im)
        if t + 1 < yy.shape[-2]:
            xx = ops.window_slide(xx, im.contiguous())
    pred = torch.cat(preds, dim=-2)
    return pred, loss, rel_l2_loss(pred.contiguous(), yy.contiguous(), msk)


@pytest.mark.parametrize("which", ["dpot3d", "fno3d"])
def test_wrapped_rollout_is_the_loop_written_out_by_hand(which):
    from dpot_amd import RolloutEvaluator, StepMetrics
    from dpot_amd.infer import GraphedRollout, Resized3D, rollout_eval
    m, S, T, C = dpot3d() if which == "dpot3d" else fno3d()
    xx, yy, msk = windows(T, C)
    T_ar = yy.shape[-2]
    w = Resized3D(m, S)
    assert list(w.parameters(recurse=False)) == [] and w.model_res == (S, S, S)
    eager = rollout_eval(w, xx, yy, msk)
    assert tuple(eager[0].shape) == tuple(yy.shape)
    for a, b in zip(eager, by_hand(m, S, xx, yy, msk)):
        assert torch.equal(a, b)
    # the first step against restatement -> model -> restatement (float64 resizes on the host, the model's fp32 forward)
    with torch.no_grad():
        up = torch.from_numpy(resize3_ref(xx.cpu().numpy(), S)).float().cuda()
        mid = m(up)
        want = resize3_ref(mid.cpu().numpy(), DATA)
    assert_close(w(xx), want, f"{which}: first step of the wrapper")
    assert_close(eager[0][..., :1, :], want, f"{which}: first step of the rollout")
    # model_res= on a 6-D window still raises, wrapped or not
    with pytest.raises(ValueError, match="model_res"):
        rollout_eval(w, xx, yy, msk, model_res=S)
    # one graph at the DATA resolution, both resizes inside
    g = GraphedRollout(w, torch.zeros_like(xx))
    assert g.cls is None and tuple(g.im.shape) == tuple(xx.shape[:4]) + (1, C)
    for a, b in zip(eager, g(xx, yy, msk)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="model_res"):
        g(xx, yy, msk, model_res=S)
    for run in (lambda **k: rollout_eval(w, xx, yy, msk, **k), lambda **k: g(xx, yy, msk, **k)):
        ev = RolloutEvaluator("cuda", n_channels=C, T_max=T_ar, ilow=1, ihigh=2)
        for a, b in zip(eager, run(evaluator=ev)):
            assert torch.equal(a, b)
        assert ev.read()["samples"] == xx.shape[0]
    met_e, met_g, ev = StepMetrics("cuda", T_ar), StepMetrics("cuda", T_ar), RolloutEvaluator("cuda", C, T_ar, 1, 2)
    with_met = rollout_eval(w, xx, yy, msk, metrics=met_e)
    for a, b in zip(with_met, g(xx, yy, msk, metrics=met_g, evaluator=ev)):
        assert torch.equal(a, b)
    assert torch.equal(met_e.acc, met_g.acc) and torch.equal(with_met[0], eager[0]) and torch.equal(with_met[1], eager[1])
    assert_close(with_met[2], eager[2], "full loss from the step statistics")


def test_wrapper_at_the_data_resolution_still_resizes_and_capture_needs_the_plans(monkeypatch):
    """model_res equal to the data resolution: both resizes run (the identity up to rounding), as in the reference's 2-D
    loop; a capture of the wrapper whose plans do not exist raises the plan's error (the capture state is stubbed)"""
    from dpot_amd import _lib, ops
    from dpot_amd.infer import Resized3D
    m, S, T, C = fno3d()
    x = torch.from_numpy(hash_field((1, S, S, S, T, C), 61)).cuda()
    calls, real = [], ops.spectral_resize3

    def counted(t, out_size, out=None):
        calls.append(out_size)
        return real(t, out_size, out)

    monkeypatch.setattr(ops, "spectral_resize3", counted)
    with torch.no_grad():
        got = Resized3D(m, S)(x)
        plain = m(x)
    assert calls == [(S, S, S), (S, S, S)]
    assert_close(got, plain, "wrapper at the model's own resolution")
    odd = torch.zeros(1, 5, 7, 9, T, C, device="cuda")      # data sizes no other test uses: no plans yet
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.DpotHipError, match="before capturing"):
        Resized3D(m, S)(odd)
