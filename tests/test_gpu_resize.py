"""GPU tests of the Fourier resize kernel (csrc/resize.hip, ops.spectral_resize) and of the varying-resolution rollout
(infer.rollout_eval(model_res=), GraphedRollout(...)(..., model_res=)): the fixture the reference wrote (g15_resize), the
float64 restatement (tests/resize_ref.py), determinism, guards, graph replay, and the rollout against the oracle's forward
composed with the restatement.  The op tests run on the guarded, poisoned allocator (tests/guard.py)."""
import math

import numpy as np
import pytest
import torch

import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close, load
from oracle import dpot_ref as R
from resize_ref import hash_field, refill_mask_ref, resize_ref, ulps_apply

pytestmark = pytest.mark.gpu

CASES = ["e16_o9", "e16_e10", "o9_e16", "e10_e16", "e10_e10", "e16_e16", "o9_o9", "rect_up", "rect_down", "big128_41",
         "big50_128", "big128_122"]
# the kernel sums up to 128 terms per pass where the FFT sums 7 stages: the factor the term count predicts, and no more
ERR_FACTOR = math.sqrt(128.0 / 7.0)


def case_input(fx, name):
    if f"{name}.x" in fx.files:
        return fx[f"{name}.x"]
    return hash_field(tuple(int(s) for s in fx[f"{name}.x_shape"]), int(fx[f"{name}.x_salt"]))


def test_fixture_lists_the_cases_of_this_file():
    assert [str(n) for n in load("g15_resize")["names"]] == CASES


@pytest.mark.parametrize("name", CASES)
def test_resize_vs_reference_fixture(name, guarded):
    from dpot_amd import ops
    fx = load("g15_resize")
    x = guard.wrap(torch.from_numpy(case_input(fx, name)), "cuda")
    got = ops.spectral_resize(x, tuple(int(s) for s in fx[f"{name}.out_size"]))
    torch.cuda.synchronize()
    assert_close(got, fx[f"{name}.y64"], f"spectral_resize {name}")


@pytest.mark.parametrize("name", CASES)
def test_resize_error_relative_to_the_reference_float32(name, guarded):
    """norm-wise error against the reference's float64 result, beside the same figure of the reference's own float32 run;
    the kernel is allowed ERR_FACTOR times the reference's figure"""
    from dpot_amd import ops
    fx = load("g15_resize")
    y64 = (fx[f"{name}.y64d"] if f"{name}.y64d" in fx.files else fx[f"{name}.y64"]).astype(np.float64)
    y32 = ulps_apply(fx[f"{name}.y64"], fx[f"{name}.y32ulps"]).astype(np.float64)
    x = guard.wrap(torch.from_numpy(case_input(fx, name)), "cuda")
    got = ops.spectral_resize(x, tuple(int(s) for s in fx[f"{name}.out_size"])).double().cpu().numpy()
    assert np.isfinite(got).all()
    e_ref = np.linalg.norm(y32 - y64) / np.linalg.norm(y64)
    e_got = np.linalg.norm(got - y64) / np.linalg.norm(y64)
    print(f"resize-error {name}: kernel {e_got:.3e}  reference-fp32 {e_ref:.3e}  ratio {e_got / e_ref:.2f} "
          f"(allowed {ERR_FACTOR:.2f})")
    assert e_got <= ERR_FACTOR * e_ref, (name, e_got, e_ref)


@pytest.mark.parametrize("TC", [1, 3, 4, 40])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("sizes", [(16, 16, 9, 9), (10, 10, 16, 16), (12, 10, 16, 14), (41, 41, 64, 64), (64, 64, 50, 50),
                                   (33, 48, 34, 17)])
def test_resize_vs_restatement(sizes, B, TC, guarded):
    from dpot_amd import ops
    nx, ny, mx, my = sizes
    xh = hash_field((B, nx, ny, TC), 7 + TC + B)
    if TC == 40:
        xh = xh.reshape(B, nx, ny, 10, 4)
    x = guard.wrap(torch.from_numpy(xh), "cuda")
    got = ops.spectral_resize(x, (mx, my))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, mx, my) + xh.shape[3:]
    assert_close(got, resize_ref(xh, (mx, my)), f"spectral_resize {sizes} B={B} TC={TC}")


@pytest.mark.parametrize("TC", [3, 4])
@pytest.mark.parametrize("sizes", [(128, 128, 41, 41), (41, 41, 128, 128), (128, 128, 59, 59), (59, 59, 128, 128),
                                   (128, 128, 113, 113), (113, 113, 128, 128), (59, 113, 41, 128)])
def test_resize_is_deterministic_and_stays_inside_its_output(sizes, TC, guarded):
    """two launches give identical bits; out= into a guarded NaN slot is written completely, correctly, and nothing around
    it is touched (the guards are checked at teardown), ragged sizes in both directions"""
    from dpot_amd import ops
    nx, ny, mx, my = sizes
    B = 2
    xh = hash_field((B, nx, ny, 1, TC), 3)
    x = guard.wrap(torch.from_numpy(xh), "cuda")
    out1 = guard.full_nan((B, mx, my, 1, TC))
    out2 = guard.full_nan((B, mx, my, 1, TC))
    r1 = ops.spectral_resize(x, (mx, my), out=out1)
    r2 = ops.spectral_resize(x, (mx, my), out=out2)
    torch.cuda.synchronize()
    assert r1 is out1 and r2 is out2
    assert torch.equal(out1.view(torch.int32), out2.view(torch.int32))
    assert_close(out1, resize_ref(xh, (mx, my)), f"spectral_resize {sizes} TC={TC} into out=")
    guard.check()


def test_resize_argument_checks():
    from dpot_amd import _lib, ops
    x = torch.zeros(2, 8, 8, 1, 2, device="cuda")
    with pytest.raises(_lib.DpotHipError):
        ops.spectral_resize(x, 6, out=torch.zeros(2, 6, 5, 1, 2, device="cuda"))
    with pytest.raises(_lib.DpotHipError):
        ops.spectral_resize(x, 1)
    with pytest.raises(_lib.DpotHipError):
        ops.spectral_resize(x.double(), 6)
    with pytest.raises(_lib.DpotHipError):
        ops.spectral_resize(x.permute(0, 2, 1, 3, 4)[:, ::2], 6)
    with pytest.raises(_lib.DpotHipError):
        ops.spectral_resize(torch.zeros(1, 8, 300, 1, device="cuda"), 8)         # n_y beyond the LDS intermediate


@pytest.mark.parametrize("sizes", [(41, 41, 64, 64), (64, 64, 50, 50)])
def test_resize_under_graph_capture_replays_to_the_eager_bits(sizes):
    from dpot_amd import ops
    nx, ny, mx, my = sizes
    x = torch.from_numpy(hash_field((3, nx, ny, 2, 4), 11)).cuda()
    eager = ops.spectral_resize(x, (mx, my))                # builds the plan outside the capture
    static_out = torch.full_like(eager, float("nan"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.spectral_resize(x, (mx, my), out=static_out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out.view(torch.int32), eager.view(torch.int32))
    x.copy_(torch.from_numpy(hash_field((3, nx, ny, 2, 4), 12)))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out.view(torch.int32), ops.spectral_resize(x, (mx, my)).view(torch.int32))


# ---- the varying-resolution rollout -------------------------------------------------------------------------------------
MODEL64 = dict(R.MINI, img_size=64)


def build(kw, salt):
    from dpot_amd import DPOTNet
    cfg = R.DPOTConfig(**kw)
    m = DPOTNet(**kw)
    m.load_state_dict(R.recipe_state_dict(cfg, salt=salt))
    return m.cuda().eval(), cfg


def oracle_rollout(sd, cfg, xx, yy, msk, model_res):
    """evaluate_varyingres.py:228-248 with the oracle's forward and the float64 restatement of the resize"""
    data_res = tuple(xx.shape[1:3])
    loss, preds = 0.0, []
    for t in range(yy.shape[-2]):
        up = torch.from_numpy(resize_ref(xx.numpy(), model_res)).float()
        im, _ = R.dpot_forward(sd, up, cfg)
        im = torch.from_numpy(resize_ref(im.numpy(), data_res)).float()
        loss = loss + R.rel_l2_loss(im, yy[..., t:t + 1, :], msk)
        preds.append(im)
        xx = torch.cat((xx[..., 1:, :], im), dim=-2)
    pred = torch.cat(preds, dim=-2)
    return pred, loss, R.rel_l2_loss(pred, yy, msk)


@pytest.mark.parametrize("res", [41, 50])
def test_varying_resolution_rollout_vs_oracle(res):
    from dpot_amd import StepMetrics
    from dpot_amd.infer import GraphedRollout, refill_mask, rollout_eval
    m, cfg = build(MODEL64, salt=2)
    sd = R.recipe_state_dict(cfg, salt=2)
    B, T_ar, S = 2, 3, cfg.img_size
    xx = R.recipe_input((B, res, res, cfg.in_timesteps, cfg.in_channels), salt=5)
    yy = R.recipe_input((B, res, res, T_ar, cfg.out_channels), salt=6)
    msk0 = torch.ones(B, S, S, 1, cfg.out_channels)
    msk0[1, :, :, :, 2] = 0.0                                           # one masked-out channel
    msk = refill_mask(msk0.cuda(), res)
    assert np.array_equal(msk.cpu().numpy(), refill_mask_ref(msk0.numpy(), res))
    with torch.no_grad():
        pred_ref, steps_ref, full_ref = oracle_rollout(sd, cfg, xx, yy, msk.cpu(), (S, S))
    pred, l_steps, l_full = rollout_eval(m, xx.cuda(), yy.cuda(), msk, model_res=S)
    assert tuple(pred.shape) == (B, res, res, T_ar, cfg.out_channels)
    assert_close(pred, pred_ref, f"rollout pred at res {res}")
    assert_close(l_steps, steps_ref, "sum of step losses")
    assert_close(l_full, full_ref, "full-trajectory loss")
    g = GraphedRollout(m, torch.zeros(B, S, S, cfg.in_timesteps, cfg.in_channels, device="cuda"))
    pred_g, l_steps_g, l_full_g = g(xx.cuda(), yy.cuda(), msk, model_res=S)
    assert torch.equal(pred_g, pred) and torch.equal(l_steps_g, l_steps) and torch.equal(l_full_g, l_full)
    met = StepMetrics("cuda", T_ar)
    _, s1, f1 = rollout_eval(m, xx.cuda(), yy.cuda(), msk, model_res=S, metrics=met)
    _, s2, f2 = g(xx.cuda(), yy.cuda(), msk, model_res=S, metrics=met)
    d = met.read()
    assert_close(torch.tensor(d["l2_step"]), 2 * steps_ref.double(), "test_l2_step")
    assert_close(torch.tensor(d["l2_full"]), 2 * full_ref.double(), "test_l2_full")
    assert_close(f1, full_ref, "full loss from the step statistics")
    with pytest.raises(ValueError):
        g(xx.cuda(), yy.cuda(), msk)                                    # data resolution without model_res
    with pytest.raises(ValueError):
        g(xx.cuda(), yy.cuda(), msk, model_res=32)                      # not the captured resolution


def test_model_res_none_is_the_plain_rollout_and_equal_size_still_resizes():
    """model_res=None returns the bits of the call without the keyword; model_res equal to the data size follows the
    reference, which resizes then too.  (With every frequency kept the operator of a REAL field is the identity - the
    reference's float64 result of the 16 -> 16 fixture case equals its input to 2e-16 - so that rollout is compared with
    the oracle composed with the restatement, not required to differ from the plain one.)"""
    from dpot_amd.infer import GraphedRollout, rollout_eval
    m, cfg = build(R.MINI, salt=2)
    sd = R.recipe_state_dict(cfg, salt=2)
    B, T_ar, S = 3, 3, cfg.img_size
    xx = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=5)
    yy = R.recipe_input((B, S, S, T_ar, cfg.out_channels), salt=6)
    msk = torch.ones(B, S, S, 1, cfg.out_channels)
    plain = rollout_eval(m, xx.cuda(), yy.cuda(), msk.cuda())
    none = rollout_eval(m, xx.cuda(), yy.cuda(), msk.cuda(), model_res=None)
    for a, b in zip(plain, none):
        assert torch.equal(a, b)
    g = GraphedRollout(m, xx.cuda())
    for a, b in zip(g(xx.cuda(), yy.cuda(), msk.cuda()), g(xx.cuda(), yy.cuda(), msk.cuda(), model_res=None)):
        assert torch.equal(a, b)
    with torch.no_grad():
        pred_ref, steps_ref, full_ref = oracle_rollout(sd, cfg, xx, yy, msk, (S, S))
    same = rollout_eval(m, xx.cuda(), yy.cuda(), msk.cuda(), model_res=S)
    assert_close(same[0], pred_ref, "rollout pred, model_res == data size")
    assert_close(same[1], steps_ref, "sum of step losses")
    assert_close(same[2], full_ref, "full-trajectory loss")
    assert_close(g(xx.cuda(), yy.cuda(), msk.cuda(), model_res=S)[0], pred_ref, "graphed rollout, model_res == data size")
