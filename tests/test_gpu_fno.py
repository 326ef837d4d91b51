"""GPU tests of the FNO baseline: the truncated transforms and the per-mode mixing (csrc/fno.hip, ops.fno_*) against the float64
restatement (tests/fno_ref.py) and beside the float32 error of the reference's own composition (tests/golden/g22_fno.npz), the
layer functions, and FNO2d through the training step, the captured step and the rollouts.  The operator tests run on the guarded,
poisoned allocator (tests/guard.py)."""
import functools
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import fno_ref as FR
import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close, load
from oracle import dpot_ref as R
from resize_ref import resize_ref

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24          # unit roundoff of float32
GELU = 1


def _lg(n):
    return max(1, math.ceil(math.log2(n)))


def _tf_factors(case):
    """Allowed factor over the float32 error of the reference's FFT composition: the ratio of the lengths of the longest chains
    of rounded operations behind one element (worst-case error bounds grow linearly with them).
      reference   an FFT of n points has at least ceil(log2 n) butterfly levels: log2 H + log2 W, + 1 for the scaling / slice
      rfft2       kernel: one fma per y (W), then two per x (the real and imaginary part of T each feed an output: 2 H), + 1
                  for the scale and column weight
      irfft2      kernel: two fmas per kept row (2 * 2 m1), one product with the weight, two fmas per kept column (2 m2), + 1
                  for the epilogue's add
    never below 2 (the kernels' twiddles are rounded float64 values, the FFT's its own)."""
    B, H, W, C, m1, m2 = case
    ref = _lg(H) + _lg(W) + 1
    f = max(2.0, (W + 2 * H + 1) / ref)
    i = max(2.0, (4 * m1 + 1 + 2 * m2 + 1) / ref)
    return {"fwd": f, "adj_inv": f, "inv": i, "adj_fwd": i}


def _report(what, got, ref64, e_ref, factor):
    e = FR.nerr(got.detach().cpu().numpy(), ref64.numpy())
    print(f"fno-error {what}: kernel {e:.3e}  reference-fp32 {e_ref:.3e}  allowed {factor:.2f} x max(reference, 2^-24) = "
          f"{factor * max(e_ref, U32):.3e}")
    return e


@pytest.mark.parametrize("case", FR.TRANSFORM_CASES, ids=lambda c: "b%d_%dx%d_c%d_m%dx%d" % c)
def test_transforms_vs_float64_and_the_reference_float32_error(case, guarded):
    """rfft2 and irfft2 in both roles (the transform itself and the adjoint of the other one).  Cases 0-4 are the issue's; the
    others cross the tiles of the kernels as built (rfft2: 512 threads, items (row, channel quad) in pass 1 - one sweep covers 128
    rows - and (kept row pair, column of 4, channel quad) in pass 2 - one sweep covers m1 = 32 with a full chunk; 4 columns ky and
    16 channels per workgroup.  irfft2: 256 threads, 16 rows and 16 channels per workgroup, pass-1 items (column, 8 row pairs,
    channel quad) - one sweep covers m2 = 8 -, the 4 waves own 16 columns y per sweep):
      (1, 130, 12, 4, 40, 3)  H = 130: a ragged second sweep of rfft2's pass-1 items (520 > 512) and a ragged ninth row stripe of
                              irfft2; m1 = 40: a ragged second sweep of rfft2's pass-2 items (640 > 512); m2 = 3: a ragged chunk
      (1, 72, 20, 20, 5, 9)   more than four 16-row stripes of irfft2; W = 20: a second sweep of the 16 columns the waves of irfft2
                              own; C = 20: across the 16-channel chunk on the 16-byte path; m2 = 9: three 4-column chunks of rfft2
                              with a ragged last one, and a second sweep of irfft2's first-pass items (m2 > 8)
      (1, 18, 34, 18, 2, 6)   the same channel boundary on the scalar path (C % 4 != 0), rows across one 16-row stripe
      (1, 17, 16, 4, 8, 4)    one row past a stripe, exactly one column sweep, m2 = exactly one chunk, 2 m1 = H - 1
      (2, 16, 17, 16, 1, 8)   exactly one stripe and one channel chunk, one column past a sweep, m2 = two chunks
      (1, 256, 256, 4, 64, 64) the declared maximum (dpot_fno_max_size): two full sweeps of both rfft2 passes"""
    from dpot_amd import ops
    fx = load("g22_fno")
    i = FR.TRANSFORM_CASES.index(case)
    B, H, W, C, m1, m2 = case
    x0, S0 = FR.transform_inputs(case)
    x, S = guard.wrap(x0, "cuda"), guard.wrap(S0, "cuda")
    got = {"fwd": ops.fno_rfft2(x, m1, m2), "adj_inv": ops.fno_rfft2(x, m1, m2, adjoint=True),
           "inv": ops.fno_irfft2(S, H, W)[0], "adj_fwd": ops.fno_irfft2(S, H, W, adjoint=True)[0]}
    again = {"fwd": ops.fno_rfft2(x, m1, m2), "inv": ops.fno_irfft2(S, H, W)[0]}
    torch.cuda.synchronize()
    ref = FR.transform_ref(case)
    fac = _tf_factors(case)
    errs = {k: _report(f"{case}.{k}", got[k], ref[k], float(fx[f"tf.{i}.e32.{k}"]), fac[k]) for k in ref}
    for k in ref:
        assert tuple(got[k].shape) == tuple(ref[k].shape)
        assert_close(got[k], ref[k], f"fno transform {case} {k}")
        assert errs[k] <= fac[k] * max(float(fx[f"tf.{i}.e32.{k}"]), U32), (case, k, errs[k])
    for k in again:                                                               # the same bits on every run
        assert torch.equal(again[k].view(torch.int32), got[k].view(torch.int32)), k
    guard.check()


def test_irfft2_epilogue_add_pre_activation_and_out(guarded):
    from dpot_amd import ops
    for case in (FR.TRANSFORM_CASES[0], FR.TRANSFORM_CASES[5]):
        B, H, W, C, m1, m2 = case
        _, S0 = FR.transform_inputs(case)
        add0 = FR.hash_input((B, H, W, C), 991)
        out = guard.full_nan((B, H, W, C))
        y, pre = ops.fno_irfft2(guard.wrap(S0, "cuda"), H, W, add=guard.wrap(add0, "cuda"), act=GELU, save_pre=True, out=out)
        torch.cuda.synchronize()
        assert y is out
        want = FR.irfft2_kept(FR.from_planes(S0.double()), H, W) + add0.double()
        assert_close(pre, want, f"{case} pre")
        assert_close(y, torch.nn.functional.gelu(want), f"{case} y")
    guard.check()


@pytest.mark.parametrize("case", FR.MIX_CASES, ids=lambda c: "b%d_c%dto%d_m%dx%d" % c)
def test_mixing_vs_float64_and_the_reference_float32_error(case, guarded):
    """forward, data gradient, weight gradient with and without accumulate; (5, 20, 36, 2, 3) has more than 16 channels on both
    sides, so both roles of the mixing run a second output-tile row and the weight gradient 45 channel tiles.
    Factor: the kernel adds two fmas per reduced channel to each real accumulator (2 Cin, 2 Cout for the data gradient, 2 B for the weight gradient); the reference's four
    real einsums reduce K terms each and are combined by one more operation (K + 1): 2 K / (K + 1) < 2."""
    from dpot_amd import ops
    fx = load("g22_fno")
    i = FR.MIX_CASES.index(case)
    X0, dO0, w10, w20 = FR.mix_inputs(case)
    X, dO, w1, w2 = (guard.wrap(t, "cuda") for t in (X0, dO0, w10, w20))
    d1, d2 = ops.fno_mix_wgrad(X, dO)
    got = {"fwd": ops.fno_mix(X, w1, w2), "dgrad": ops.fno_mix(dO, w1, w2, adjoint=True), "dw1": d1, "dw2": d2}
    base1, base2 = FR.hash_input(d1.shape, 992), FR.hash_input(d2.shape, 993)
    a1, a2 = guard.wrap(base1, "cuda"), guard.wrap(base2, "cuda")
    r1, r2 = ops.fno_mix_wgrad(X, dO, a1, a2, accumulate=True)
    o1, o2 = ops.fno_mix_wgrad(X, dO, guard.full_nan(tuple(d1.shape)), guard.full_nan(tuple(d2.shape)))
    again = ops.fno_mix(X, w1, w2)
    torch.cuda.synchronize()
    ref = FR.mix_ref(case)
    errs = {k: _report(f"{case}.{k}", got[k], ref[k], float(fx[f"mix.{i}.e32.{k}"]), 2.0) for k in ref}
    for k in ref:
        assert tuple(got[k].shape) == tuple(ref[k].shape)
        assert_close(got[k], ref[k], f"fno mix {case} {k}")
        assert errs[k] <= 2.0 * max(float(fx[f"mix.{i}.e32.{k}"]), U32), (case, k, errs[k])
    assert r1 is a1 and r2 is a2
    assert torch.equal(a1.cpu(), base1 + d1.cpu()) and torch.equal(a2.cpu(), base2 + d2.cpu())   # one fp32 add per element
    assert torch.equal(o1, d1) and torch.equal(o2, d2) and torch.equal(again, got["fwd"])
    guard.check()


def _ints(shape, salt):
    """float32 integers in [-3, 3] from the hash recipe: floor(7 u) - 3 with u = hash / 3 + 1 / 2 in [0, 1)"""
    u = FR.hash_input(shape, salt).double() / 3.0 + 0.5
    return (torch.floor(7.0 * u).clamp_(0.0, 6.0) - 3.0).float()


def test_mixing_is_exact_on_integers_past_the_first_mode_block(guarded):
    """B 5, Cin 8, Cout 4, modes (5, 7): G = 70 kept modes, so modes 64..69 (all of weights2) sit in the second 64-mode block of
    the grid, on the 16-byte path (both channel counts are multiples of 4, the buffers aligned); B = 5 is a ragged second sample
    tile.  Integer operands in [-3, 3], both weights and both accumulate bases their own salt: each partial sum is an integer of
    magnitude at most 8 * 2 * 9 = 144 < 2^24, so fp32 is exact whatever the summation order and so is the float64
    restatement - every result must EQUAL it."""
    from dpot_amd import ops
    B, Cin, Cout, m1, m2 = 5, 8, 4, 5, 7
    X0, dO0 = _ints((B, 2 * m1, m2, 2, Cin), 996), _ints((B, 2 * m1, m2, 2, Cout), 997)
    ws0 = [_ints((2, Cin, Cout, m1, m2), 998 + k) for k in range(2)]
    bases = [_ints((2, Cin, Cout, m1, m2), 1000 + k) for k in range(2)]
    X, dO = guard.wrap(X0, "cuda"), guard.wrap(dO0, "cuda")
    w1, w2 = (guard.wrap(w, "cuda") for w in ws0)
    fwd, dgrad = ops.fno_mix(X, w1, w2), ops.fno_mix(dO, w1, w2, adjoint=True)
    ds = ops.fno_mix_wgrad(X, dO)
    accs = ops.fno_mix_wgrad(X, dO, *(guard.wrap(b, "cuda") for b in bases), accumulate=True)
    nans = ops.fno_mix_wgrad(X, dO, *(guard.full_nan(tuple(w.shape)) for w in ws0))
    torch.cuda.synchronize()
    Xc, dOc = FR.from_planes(X0.double()), FR.from_planes(dO0.double())
    wd = [w.double() for w in ws0]
    assert torch.equal(fwd.cpu().double(), FR.to_planes(FR.mix(Xc, *wd)))
    assert torch.equal(dgrad.cpu().double(), FR.to_planes(FR.mix(dOc, *wd, adjoint=True)))
    for k, ref in enumerate(FR.mix_wgrad(Xc, dOc)):
        assert torch.equal(ds[k].cpu().double(), ref), k
        assert torch.equal(nans[k].cpu().double(), ref), k
        assert torch.equal(accs[k].cpu().double(), bases[k].double() + ref), k
    guard.check()


def test_act_bwd_mul(guarded):
    from dpot_amd import ops
    for n in (1, 7, 1024, 4099):
        dy0, pre0 = FR.hash_input((n,), 994), FR.hash_input((n,), 995)
        got = ops.act_bwd_mul(guard.wrap(dy0, "cuda"), guard.wrap(pre0, "cuda"), GELU)
        p = pre0.double().requires_grad_(True)
        torch.nn.functional.gelu(p).backward(dy0.double())
        assert_close(got, p.grad, f"act_bwd_mul n={n}")
    guard.check()


def test_argument_checks_and_limits():
    from dpot_amd import _lib, ops
    lib = _lib.load()
    n = lib.dpot_fno_max_size(0)
    with pytest.raises(ValueError, match=f"{n + 1}x8"):
        ops.fno_rfft2(torch.zeros(1, n + 1, 8, 4, device="cuda"), 2, 2)
    with pytest.raises(ValueError):
        ops.fno_irfft2(torch.zeros(1, 4, 3, 2, 4, device="cuda"), 8, n + 8)
    with pytest.raises((ValueError, _lib.DpotHipError)):
        ops.fno_rfft2(torch.zeros(1, 8, 8, 4, device="cuda").double(), 2, 2)
    with pytest.raises(ValueError):
        ops.fno_mix(torch.zeros(1, 4, 3, 2, 5, device="cuda"), *(torch.zeros(2, 4, 4, 2, 3, device="cuda"),) * 2)
    s = torch.cuda.current_stream().cuda_stream                 # the C entry points: DPOT_EUNSUP with the size named, no launch
    d = torch.zeros(64, device="cuda")
    assert lib.dpot_fno_rfft2(d.data_ptr(), d.data_ptr() + 64, d.data_ptr(), d.data_ptr(), 1, n + 1, 8, 1, 1, 1, 0, 1.0, s) == -2
    assert f"{n + 1}x8".encode() in lib.dpot_last_error()
    assert lib.dpot_fno_irfft2(d.data_ptr(), None, d.data_ptr() + 64, None, d.data_ptr(), d.data_ptr(), 1, 8, n + 2, 1, 1, 1, 1,
                               1.0, 0, s) == -2
    assert lib.dpot_fno_rfft2(d.data_ptr(), d.data_ptr() + 64, d.data_ptr(), d.data_ptr(), 1, 8, 8, 1, 5, 1, 0, 1.0, s) == -1
    torch.cuda.synchronize()
    assert not d.any()


def test_plan_under_capture_is_an_error_and_a_warmed_up_size_captures(monkeypatch):
    """a size tuple first seen while the stream captures: an error that says what to do, before anything is uploaded (the
    capture state is stubbed: aborting a real capture is not something a test should leave behind); after one eager use the
    operators capture and replay to the eager bits"""
    from dpot_amd import _lib, ops
    x = FR.hash_input((2, 11, 13, 6), 996).cuda()               # a size tuple no other test uses
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.DpotHipError, match="before capturing"):
        ops.fno_rfft2(x, 3, 5)
    monkeypatch.undo()
    w1, w2 = (FR.spectral_weight(n, (2, 6, 6, 3, 5), 996).cuda() for n in ("weights1", "weights2"))
    eager, _ = ops.fno_irfft2(ops.fno_mix(ops.fno_rfft2(x, 3, 5), w1, w2), 11, 13)
    static_out = torch.full_like(eager, float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        X = ops.fno_rfft2(x, 3, 5)
        ops.fno_irfft2(ops.fno_mix(X, w1, w2), 11, 13, out=static_out)
        dw = ops.fno_mix_wgrad(X, X)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out.view(torch.int32), eager.view(torch.int32))
    x.copy_(FR.hash_input((2, 11, 13, 6), 997))
    graph.replay()
    torch.cuda.synchronize()
    X2 = ops.fno_rfft2(x, 3, 5)
    assert torch.equal(static_out, ops.fno_irfft2(ops.fno_mix(X2, w1, w2), 11, 13)[0])
    assert torch.equal(dw[0], ops.fno_mix_wgrad(X2, X2)[0])


# ---- the layer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FR.LAYER_CASES))
def test_spectral_conv_fn_vs_the_fixture(name, guarded):
    from dpot_amd.functional import SpectralConv2dFn
    fx = load("g22_fno")
    x0, g0, w10, w20 = FR.layer_inputs(name)
    x, w1, w2 = (guard.wrap(t, "cuda").requires_grad_(True) for t in (x0, w10, w20))
    y = SpectralConv2dFn.apply(x, w1, w2)
    y.backward(guard.wrap(g0, "cuda"))
    torch.cuda.synchronize()
    for k, t in (("y", y.detach()), ("dx", x.grad), ("dw1", w1.grad), ("dw2", w2.grad)):
        e = FR.nerr(t.cpu().numpy(), fx[f"layer.{name}.{k}64"])
        print(f"fno-layer {name}.{k}: kernels {e:.3e}  reference-fp32 {float(fx[f'layer.{name}.e32.{k}']):.3e}")
        assert_close(t, fx[f"layer.{name}.{k}64"], f"layer.{name}.{k} vs float64")
        assert_close(t, fx[f"layer.{name}.{k}32"], f"layer.{name}.{k} vs the reference's float32")


def test_frozen_spectral_weights_still_give_the_data_gradient(guarded):
    """weights1 / weights2 without requires_grad: no weight-gradient launch, the same dx and convolution gradients"""
    from dpot_amd.functional import FNOLayerFn, SpectralConv2dFn
    name = "h7x9_c3to5"
    B, H, W, Cin, Cout, m1, m2 = FR.LAYER_CASES[name]
    x0, g0, w10, w20 = FR.layer_inputs(name)
    cw0 = ((R.recipe_tensor("convw", (Cout, Cin), 61) - 0.5) * 2.0 / math.sqrt(Cin)).float()
    cb0 = ((R.recipe_tensor("convb", (Cout,), 61) - 0.5) * 0.2).float()
    res = []
    for frozen in (False, True):
        x, cw, cb = (guard.wrap(t, "cuda").requires_grad_(True) for t in (x0, cw0, cb0))
        w1, w2 = (guard.wrap(t, "cuda").requires_grad_(not frozen) for t in (w10, w20))
        FNOLayerFn.apply(x, w1, w2, cw, cb, GELU).backward(guard.wrap(g0, "cuda"))
        xs = guard.wrap(x0, "cuda").requires_grad_(True)
        SpectralConv2dFn.apply(xs, w1.detach().requires_grad_(not frozen), w2.detach()).backward(guard.wrap(g0, "cuda"))
        torch.cuda.synchronize()
        assert (w1.grad is None) == frozen and (w2.grad is None) == frozen
        res.append((x.grad, cw.grad, cb.grad, xs.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", list(FR.LAYER_CASES))
def test_whole_layer_vs_restatement(name, guarded):
    """gelu(spectral + 1x1 convolution), Cin != Cout included, every gradient against the float64 restatement's autograd"""
    from dpot_amd.functional import FNOLayerFn
    B, H, W, Cin, Cout, m1, m2 = FR.LAYER_CASES[name]
    x0, g0, w10, w20 = FR.layer_inputs(name)
    cw0 = ((R.recipe_tensor("convw", (Cout, Cin), 61) - 0.5) * 2.0 / math.sqrt(Cin)).float()
    cb0 = ((R.recipe_tensor("convb", (Cout,), 61) - 0.5) * 0.2).float()
    dev = [guard.wrap(t, "cuda").requires_grad_(True) for t in (x0, w10, w20, cw0, cb0)]
    y = FNOLayerFn.apply(*dev, GELU)
    y.backward(guard.wrap(g0, "cuda"))
    torch.cuda.synchronize()
    ref = [t.double().requires_grad_(True) for t in (x0, w10, w20, cw0, cb0)]
    y64 = FR.fno_layer(*ref)
    (y64 * g0.double()).sum().backward()
    assert_close(y, y64.detach(), f"layer {name} y")
    for nm, a, b in zip(("dx", "dweights1", "dweights2", "dconv.weight", "dconv.bias"), dev, ref):
        assert_close(a.grad, b.grad, f"layer {name} {nm}")


# ---- the model ---------------------------------------------------------------------------------------------------------------
def build(cfg, salt):
    from dpot_amd import FNO2d
    m = FNO2d(**cfg)
    sd = FR.recipe_sd(OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items()), salt)
    m.load_state_dict(sd, strict=True)
    return m.cuda(), sd


@pytest.mark.parametrize("tag", list(FR.MODELS))
def test_mini_model_vs_reference(tag):
    from dpot_amd.functional import rel_l2_loss
    fx = load("g22_fno")
    cfg, salt = FR.MODELS[tag]
    m, _ = build(cfg, salt)
    x, y, msk, gc = (t.cuda() for t in FR.model_inputs(tag))
    x.requires_grad_(True)
    pred, cls_pred = m(x)
    assert tuple(pred.shape) == tuple(y.shape)
    (rel_l2_loss(pred, y, msk) + (cls_pred * gc).sum()).backward()
    torch.cuda.synchronize()
    for k, t in (("pred", pred), ("cls_pred", cls_pred)):
        ref = torch.from_numpy(fx[f"{tag}.{k}"]).double()
        print(f"{tag}.{k}: kernels {(t.detach().double().cpu() - ref).abs().max().item() / ref.abs().max().item():.2e}  "
              f"reference-fp32 {float(fx[f'{tag}.err32.{k}']):.2e} (max|d| / max|float64|)")
    assert_close(pred, fx[f"{tag}.pred"], f"{tag}.pred")
    assert_close(cls_pred, fx[f"{tag}.cls_pred"], f"{tag}.cls_pred")
    assert_close(x.grad.reshape(-1)[::FR.DX_STRIDE], fx[f"{tag}.dx"], f"{tag}.dx")
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert sorted(grads) == sorted(str(n) for n in fx[f"{tag}.gnames"])
    for k, g in grads.items():
        assert g is not None, k
        assert_close(g, fx[f"{tag}.g.{k}"], f"{tag}.g.{k}")


def _per_tensor(model, names, flat_of):
    params = dict(model.named_parameters())
    flat = torch.cat([flat_of(params[n]).detach().reshape(-1) for n in names]).cpu()
    owner = torch.cat([torch.full((params[n].numel(),), i, dtype=torch.int64) for i, n in enumerate(names)])
    return flat[::FR.STEP_STRIDE], owner[::FR.STEP_STRIDE]


def _step_batch():
    return tuple(t.cuda() for t in FR.step_inputs())


def _opt(m, update_tail=False):
    from dpot_amd.train import FlatParams, FusedAdam
    st = FR.STEP
    return FusedAdam(FlatParams(m), lr=st["lr"], betas=st["betas"], weight_decay=st["weight_decay"], max_norm=st["max_norm"],
                     update_tail=update_tail)


def test_two_ar_step_train_step_vs_reference():
    """train_temporal.py's loop, two AR steps, noise off: loss, gradient before the clip, its norm, parameters after Adam, with
    the tolerances of tests/test_gpu_cdpot.py: gradients per tensor at the contract, parameters at the contract plus what Adam's
    first step (a move of size lr whatever |g| is) makes of a gradient that differs within the gradient tolerance:
    lr min(2, c tol_g eps / (max(0, |g'| - c tol_g) + eps)^2), g' = c g + wd p, c the clip coefficient."""
    from dpot_amd.train import train_step
    fx = load("g22_fno")
    st = FR.STEP
    m, sd0 = build(FR.MINI1, st["salt"])
    xx, yy, msk = _step_batch()
    opt = _opt(m)
    cls_before = [p.detach().clone() for p in m.cls_head.parameters()]
    loss, pred = train_step(m, opt, xx, yy, msk, lr=st["lr"])
    torch.cuda.synchronize()
    assert tuple(pred.shape) == tuple(yy.shape)
    assert_close(loss, fx["step.loss"], "step loss")
    gnorm = float(fx["step.grad_norm"])
    assert abs(opt.grad_norm().item() - gnorm) <= 1e-4 * gnorm
    names = [str(n) for n in fx["step.names"]]
    assert names == [n for n, _ in m.named_parameters() if not n.startswith("cls_head.")]
    assert [str(n) for n in fx["step.nograd"]] == [n for n, _ in m.named_parameters() if n.startswith("cls_head.")]
    got_g, owner = _per_tensor(m, names, lambda p: p.grad)
    got_p, _ = _per_tensor(m, names, lambda p: p)
    ref_g, ref_p = torch.from_numpy(fx["step.grad"]).double(), torch.from_numpy(fx["step.params"]).double()
    p0 = torch.cat([sd0[n].reshape(-1) for n in names])[::FR.STEP_STRIDE].double()
    assert got_g.shape == ref_g.shape and got_p.shape == ref_p.shape
    c = min(1.0, st["max_norm"] / (gnorm + 1e-6))
    eps = 1e-8
    for i, n in enumerate(names):
        sel = owner == i
        if not sel.any():
            continue
        assert_close(got_g[sel], ref_g[sel], f"step gradient {n}")
        g, p = ref_g[sel], ref_p[sel]
        tol_g = c * (1e-4 * g.abs() + 1e-4 * g.abs().max())
        geff = (c * g + st["weight_decay"] * p0[sel]).abs()
        move = st["lr"] * torch.clamp(tol_g * eps / ((geff - tol_g).clamp(min=0.0) + eps) ** 2, max=2.0)
        err = (got_p[sel].double() - p).abs()
        tol = 1e-4 * p.abs() + 1e-4 * p.abs().max() + move
        assert torch.isfinite(got_p[sel]).all() and (err <= tol).all(), \
            (f"step parameters {n}: {int((err > tol).sum())}/{err.numel()} out of tolerance, worst {float((err - tol).max()):.3e} "
             f"over it")
    for p, q in zip(m.cls_head.parameters(), cls_before):                          # no gradient: untouched, as the reference
        assert torch.equal(p.detach(), q)


@pytest.mark.parametrize("with_cls", [False, True], ids=["plain", "cls_metrics"])
def test_graphed_train_step_replays_the_eager_step_bit_for_bit(with_cls):
    from dpot_amd import StepMetrics
    from dpot_amd.train import GraphedTrainStep, train_step
    st = FR.STEP
    xx, yy, msk = _step_batch()
    cls = torch.tensor([2, 0], device="cuda")
    runs = []
    for graphed in (False, True):
        m, _ = build(FR.MINI1, st["salt"])
        opt = _opt(m, update_tail=with_cls)
        met = StepMetrics("cuda", st["T_ar"]) if with_cls else None
        kw = dict(cls=cls, cls_weight=0.3, metrics=met) if with_cls else {}
        if graphed:
            step = GraphedTrainStep(m, opt, xx, yy, msk, warmup=1, **kw)
            loss, pred = step.replay(st["lr"]).clone(), step.pred.clone()
        else:
            loss, pred = train_step(m, opt, xx, yy, msk, lr=st["lr"], **kw)
        torch.cuda.synchronize()
        runs.append((loss.clone(), pred.clone(), {n: p.detach().clone() for n, p in m.named_parameters()},
                     met.read() if met is not None else None))
    (l0, p0, w0, d0), (l1, p1, w1, d1) = runs
    assert torch.equal(l1, l0) and torch.equal(p1, p0)
    for n in w0:
        assert torch.equal(w1[n], w0[n]), n
    if with_cls:
        m0, _ = build(FR.MINI1, st["salt"])
        start = dict(m0.named_parameters())
        assert all(not torch.equal(w0[n], start[n].detach()) for n in w0 if n.startswith("cls_head."))
        for k in ("cls_correct", "cls_total", "samples", "ar_steps", "opt_steps"):
            assert d1[k] == d0[k], k
        assert d0["opt_steps"] == 1 and d0["cls_total"] == 2 * st["T_ar"]


@functools.lru_cache(maxsize=None)
def _rollout_model():
    m, sd = build(FR.MINI1, 850)
    return m.eval(), {k: v.double() for k, v in sd.items()}


def _ref_rollout(sd, xx, yy, msk, model_res=None):
    data_res = tuple(xx.shape[1:3])
    xx, yy, msk = xx.double(), yy.double(), msk.double()
    loss, preds = 0.0, []
    for t in range(yy.shape[-2]):
        inp = torch.from_numpy(resize_ref(xx.numpy(), model_res)) if model_res is not None else xx
        im, _ = FR.fno_forward(sd, inp, FR.MINI1)
        if model_res is not None:
            im = torch.from_numpy(resize_ref(im.numpy(), data_res))
        loss = loss + R.rel_l2_loss(im, yy[..., t:t + 1, :], msk)
        preds.append(im)
        xx = torch.cat((xx[..., 1:, :], im), dim=-2)
    pred = torch.cat(preds, dim=-2)
    return pred, loss, R.rel_l2_loss(pred, yy, msk)


@pytest.mark.parametrize("res", [None, 7], ids=["model_resolution", "data7_model10"])
def test_rollout_eval_and_graphed_rollout(res):
    from dpot_amd.infer import GraphedRollout, refill_mask, rollout_eval
    m, sd = _rollout_model()
    cfg = FR.MINI1
    B, T_ar, S = 2, 3, cfg["img_size"]
    D = res or S
    xx = FR.hash_input((B, D, D, cfg["in_timesteps"], cfg["n_channels"]), 851)
    yy = FR.hash_input((B, D, D, T_ar, cfg["n_channels"]), 852)
    msk0 = torch.ones(B, S, S, 1, cfg["n_channels"])
    msk0[1, :, :, :, 1] = 0.0
    msk = refill_mask(msk0.cuda(), D) if res else msk0.cuda()
    kw = dict(model_res=S) if res else {}
    with torch.no_grad():
        pred_ref, steps_ref, full_ref = _ref_rollout(sd, xx, yy, msk.cpu(), (S, S) if res else None)
    pred, l_steps, l_full = rollout_eval(m, xx.cuda(), yy.cuda(), msk, **kw)
    assert tuple(pred.shape) == (B, D, D, T_ar, cfg["n_channels"])
    assert_close(pred, pred_ref, "rollout pred")
    assert_close(l_steps, steps_ref, "sum of step losses")
    assert_close(l_full, full_ref, "full-trajectory loss")
    g = GraphedRollout(m, torch.zeros(B, S, S, cfg["in_timesteps"], cfg["n_channels"], device="cuda"))
    pred_g, l_steps_g, l_full_g = g(xx.cuda(), yy.cuda(), msk, **kw)
    torch.cuda.synchronize()
    assert torch.equal(pred_g, pred) and torch.equal(l_steps_g, l_steps) and torch.equal(l_full_g, l_full)


def test_rollout_evaluator_and_checkpoint_loader():
    from dpot_amd import FNO2d, RolloutEvaluator
    from dpot_amd.infer import GraphedRollout, load_model_from_checkpoint, rollout_eval
    m, _ = _rollout_model()
    cfg = FR.MINI1
    B, T_ar, S = 2, 2, cfg["img_size"]
    xx = FR.hash_input((B, S, S, cfg["in_timesteps"], cfg["n_channels"]), 861).cuda()
    yy = FR.hash_input((B, S, S, T_ar, cfg["n_channels"]), 862).cuda()
    msk = torch.ones(B, S, S, 1, cfg["n_channels"], device="cuda")
    m2 = FNO2d(**cfg)
    load_model_from_checkpoint(m2, {"model": OrderedDict(("module." + k, v.cpu()) for k, v in m.state_dict().items())})
    m2 = m2.cuda().eval()
    ev1, ev2 = (RolloutEvaluator("cuda", cfg["n_channels"], T_ar, ilow=2, ihigh=4) for _ in range(2))
    p1, _, _ = rollout_eval(m, xx, yy, msk, evaluator=ev1)
    p2, _, _ = GraphedRollout(m2, xx)(xx, yy, msk, evaluator=ev2)
    torch.cuda.synchronize()
    assert torch.equal(p1, p2)
    r1, r2 = ev1.read(), ev2.read()
    assert set(r1) == set(r2)
    for k in r1:
        assert np.array_equal(np.asarray(r1[k]), np.asarray(r2[k])), k
