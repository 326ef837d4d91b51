"""GPU tests of the 3-D FNO baseline: the truncated transforms and the four-corner mixing (csrc/fno3.hip, ops.fno3_*) against
the float64 restatement (tests/fno3d_ref.py) and beside the float32 error of the reference's own composition
(tests/golden/g23_fno3d.npz), the layer functions, and FNO3d through the training step with Adam's pair rule, the captured step
and the rollouts.  The operator tests run on the guarded, poisoned allocator (tests/guard.py)."""
import functools
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import fno3d_ref as FR
import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close, load
from oracle import dpot_ref as R

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24          # unit roundoff of float32
GELU = 1
CASE_ID = "b%d_%dx%dx%d_c%d_m%dx%dx%d"


def _lg(n):
    return max(1, math.ceil(math.log2(n)))


def _tf_factors(case):
    """Allowed factor over the float32 error of the reference's FFT composition: the ratio of the lengths of the longest chains
    of rounded operations behind one element (worst-case error bounds grow linearly with them).
      reference   an FFT of n points has at least ceil(log2 n) butterfly levels: log2 X + log2 Y + log2 Z, + 1 for the scaling /
                  slices
      rfft3       launch 1 (the plane kernel): one fma per z (Z), then two per y (the real and imaginary part of the
                  intermediate each feed an output: 2 Y), + 1 for the scale and plane weight; launch 2 (the axis kernel): two
                  fmas per x into each accumulator (2 X)
      irfft3      launch 1 (the axis kernel): two fmas per kept row (2 * 2 m1); launch 2 (the plane kernel): two per kept row of
                  ky (2 * 2 m2), one product with the weight, two per kept kz (2 m3), + 1 for the epilogue's add
    never below 2 (the kernels' twiddles are rounded float64 values, the FFT's its own)."""
    B, X, Y, Z, C, m1, m2, m3 = case
    ref = _lg(X) + _lg(Y) + _lg(Z) + 1
    f = max(2.0, (Z + 2 * Y + 1 + 2 * X) / ref)
    i = max(2.0, (4 * m1 + 4 * m2 + 1 + 2 * m3 + 1) / ref)
    return {"fwd": f, "adj_inv": f, "inv": i, "adj_fwd": i}


def _report(what, got, ref64, e_ref, factor):
    e = FR.nerr(got.detach().cpu().numpy(), ref64.numpy())
    print(f"fno3-error {what}: kernel {e:.3e}  reference-fp32 {e_ref:.3e}  allowed {factor:.2f} x max(reference, 2^-24) = "
          f"{factor * max(e_ref, U32):.3e}")
    return e


@pytest.mark.parametrize("case", FR.TRANSFORM_CASES, ids=lambda c: CASE_ID % c)
def test_transforms_vs_float64_and_the_reference_float32_error(case, guarded):
    """rfft3 and irfft3 in both roles (the transform itself and the adjoint of the other one).  Cases 0-3 are the issue's; the
    others cross the tiles of the kernels as built.  The plane kernels are FNO2d's over the B X planes [Y, Z, C] with modes
    (m2, m3) (rfft2: 512 threads, pass-1 items (row y, channel quad) - one sweep covers Y = 128, the declared maximum - and pass-2
    items (kept row pair of ky, column of 4 kz, channel quad) - one sweep covers m2 = 32, the maximum; 4 columns kz and 16
    channels per workgroup.  irfft2: 256 threads, 16 rows y and 16 channels per workgroup, pass-1 items (column kz, 8 row pairs,
    channel quad) - one sweep covers m3 = 8 -, the 4 waves own 16 columns z per sweep).  The axis kernel: 256 items (mode
    (q, kz) of 2 m2 m3, channel quad) and 8 output rows per workgroup (rows: 2 m1 forward, X inverse):
      (1, 9, 17, 17, 20, 4, 5, 9)   X = 9: one row past an 8-row chunk of the inverse axis kernel, 2 m1 = 8: exactly one chunk
                                    forward (2 m1 is even, never one past; 2 m1 = 6 of case 0 is a ragged single chunk); Y = 17:
                                    one row past a 16-row stripe; Z = 17: one column past a sweep of the z columns; C = 20: across
                                    the 16-channel chunk on the 16-byte path; m3 = 9: one past two kz chunks and one past a sweep
                                    of the inverse pass-1 items; 90 modes x 5 quads = 450 axis items: a ragged second item block
      (1, 8, 16, 16, 18, 4, 2, 8)   the same channel boundary on the scalar path (C % 4 != 0); X = 8, Y = 16, Z = 16: exactly one
                                    row chunk, stripe and column sweep; m3 = 8: exactly two kz chunks, exactly one sweep of the
                                    inverse pass-1 items, and the Nyquist plane is not kept although Z is even
      (2, 17, 8, 14, 16, 8, 4, 8)   2 m1 = 16: exactly two row chunks forward, X = 17: one past two inverse; 64 modes x 4 quads =
                                    exactly one block of 256 axis items; C = 16: exactly one channel chunk; 2 m2 = Y; m3 = 8 with
                                    Z = 14: the Nyquist plane kept; B = 2
      (1, 128, 128, 128, 4, 32, 32, 32)  the declared maximum (dpot_fno3_max_size): exactly one full sweep of both rfft2 passes
                                    (nothing larger is accepted, so neither sweep can be exceeded), 16 inverse row chunks"""
    from dpot_amd import ops
    fx = load("g23_fno3d")
    i = FR.TRANSFORM_CASES.index(case)
    B, X, Y, Z, C, m1, m2, m3 = case
    x0, S0 = FR.transform_inputs(case)
    x, S = guard.wrap(x0, "cuda"), guard.wrap(S0, "cuda")
    got = {"fwd": ops.fno3_rfft3(x, m1, m2, m3), "adj_inv": ops.fno3_rfft3(x, m1, m2, m3, adjoint=True),
           "inv": ops.fno3_irfft3(S, X, Y, Z)[0], "adj_fwd": ops.fno3_irfft3(S, X, Y, Z, adjoint=True)[0]}
    again = {"fwd": ops.fno3_rfft3(x, m1, m2, m3), "inv": ops.fno3_irfft3(S, X, Y, Z)[0]}
    torch.cuda.synchronize()
    ref = FR.transform_ref(case)
    fac = _tf_factors(case)
    errs = {k: _report(f"{case}.{k}", got[k], ref[k], float(fx[f"tf.{i}.e32.{k}"]), fac[k]) for k in ref}
    for k in ref:
        assert tuple(got[k].shape) == tuple(ref[k].shape)
        assert_close(got[k], ref[k], f"fno3 transform {case} {k}")
        assert errs[k] <= fac[k] * max(float(fx[f"tf.{i}.e32.{k}"]), U32), (case, k, errs[k])
    for k in again:                                                               # the same bits on every run
        assert torch.equal(again[k].view(torch.int32), got[k].view(torch.int32)), k
    guard.check()


def test_irfft3_epilogue_add_pre_activation_and_out(guarded):
    from dpot_amd import ops
    for case in (FR.TRANSFORM_CASES[0], FR.TRANSFORM_CASES[4]):
        B, X, Y, Z, C, m1, m2, m3 = case
        _, S0 = FR.transform_inputs(case)
        add0 = FR.hash_input((B, X, Y, Z, C), 1991)
        out = guard.full_nan((B, X, Y, Z, C))
        y, pre = ops.fno3_irfft3(guard.wrap(S0, "cuda"), X, Y, Z, add=guard.wrap(add0, "cuda"), act=GELU, save_pre=True,
                                 out=out)
        torch.cuda.synchronize()
        assert y is out
        want = FR.irfft3_kept(FR.from_planes(S0.double()), X, Y, Z) + add0.double()
        assert_close(pre, want, f"{case} pre")
        assert_close(y, torch.nn.functional.gelu(want), f"{case} y")
        So = guard.full_nan(tuple(S0.shape))
        assert ops.fno3_rfft3(y, m1, m2, m3, out=So) is So
        assert_close(So, FR.to_planes(FR.rfft3_kept(y.double().cpu(), m1, m2, m3)), f"{case} rfft3 out=")
    guard.check()


@pytest.mark.parametrize("case", FR.MIX_CASES, ids=lambda c: "b%d_c%dto%d_m%dx%dx%d" % c)
def test_mixing_vs_float64_and_the_reference_float32_error(case, guarded):
    """forward, data gradient, weight gradient plain, into NaN-filled outputs and accumulated; every corner's weights are their
    own recipe, so reading the wrong block cannot pass.  (33, ...): nine sample tiles with a ragged last one; (5, 20, 36, ...):
    more than 16 channels on both sides, so both roles run a second output-tile row and the weight gradient 45 channel tiles.
    Factor: the kernel adds two fmas per reduced channel to each real accumulator (2 Cin, 2 Cout for the data gradient, 2 B for
    the weight gradient); the reference's complex64 einsum adds the two real products of each of its K complex terms to every
    real output (2 K): the ratio is 1, and the factor its floor 2."""
    from dpot_amd import ops
    fx = load("g23_fno3d")
    i = FR.MIX_CASES.index(case)
    X0, dO0, ws0 = FR.mix_inputs(case)
    X, dO = guard.wrap(X0, "cuda"), guard.wrap(dO0, "cuda")
    ws = [guard.wrap(FR.pairs(w), "cuda") for w in ws0]
    ds = ops.fno3_mix_wgrad(X, dO)
    got = {"fwd": ops.fno3_mix(X, ws), "dgrad": ops.fno3_mix(dO, ws, adjoint=True)}
    got.update({f"dw{k + 1}": d for k, d in enumerate(ds)})
    bases = [FR.hash_input(d.shape, 1992 + k) for k, d in enumerate(ds)]
    accs = [guard.wrap(b, "cuda") for b in bases]
    racc = ops.fno3_mix_wgrad(X, dO, accs, accumulate=True)
    nans = ops.fno3_mix_wgrad(X, dO, [guard.full_nan(tuple(d.shape)) for d in ds])
    again = ops.fno3_mix(X, ws)
    torch.cuda.synchronize()
    ref = FR.mix_ref(case)
    errs = {k: _report(f"{case}.{k}", got[k], ref[k], float(fx[f"mix.{i}.e32.{k}"]), 2.0) for k in ref}
    for k in ref:
        assert tuple(got[k].shape) == tuple(ref[k].shape)
        assert_close(got[k], ref[k], f"fno3 mix {case} {k}")
        assert errs[k] <= 2.0 * max(float(fx[f"mix.{i}.e32.{k}"]), U32), (case, k, errs[k])
    for k in range(4):
        assert racc[k] is accs[k]
        assert torch.equal(accs[k].cpu(), bases[k] + ds[k].cpu())                 # one fp32 add per element
        assert torch.equal(nans[k], ds[k])
    assert torch.equal(again, got["fwd"])
    guard.check()


def _ints(shape, salt):
    """float32 integers in [-3, 3] from the hash recipe: floor(7 u) - 3 with u = hash / 3 + 1 / 2 in [0, 1)"""
    u = FR.hash_input(shape, salt).double() / 3.0 + 0.5
    return (torch.floor(7.0 * u).clamp_(0.0, 6.0) - 3.0).float()


def test_mixing_is_exact_on_integers_past_the_first_mode_block(guarded):
    """B 5, Cin 8, Cout 4, modes (3, 2, 3): G = 72 kept modes, so modes 64..71 sit in the second 64-mode block of the grid, on the
    16-byte path (both channel counts are multiples of 4, the buffers aligned) - where the corner decode of g >= 64 meets
    VEC = true; B = 5 is a ragged second sample tile.  Integer operands in [-3, 3], every corner's weights and every accumulate
    base their own salt: each partial sum is an integer of magnitude at most 8 * 2 * 9 = 144 < 2^24, so fp32 is exact
    whatever the summation order and so is the float64 restatement - every result must EQUAL it."""
    from dpot_amd import ops
    B, Cin, Cout, m1, m2, m3 = 5, 8, 4, 3, 2, 3
    X0, dO0 = _ints((B, 2 * m1, 2 * m2, m3, 2, Cin), 1993), _ints((B, 2 * m1, 2 * m2, m3, 2, Cout), 1994)
    ws0 = [_ints((Cin, Cout, m1, m2, m3, 2), 1995 + k) for k in range(4)]
    bases = [_ints((Cin, Cout, m1, m2, m3, 2), 1999 + k) for k in range(4)]
    X, dO = guard.wrap(X0, "cuda"), guard.wrap(dO0, "cuda")
    ws = [guard.wrap(w, "cuda") for w in ws0]
    fwd, dgrad = ops.fno3_mix(X, ws), ops.fno3_mix(dO, ws, adjoint=True)
    ds = ops.fno3_mix_wgrad(X, dO)
    accs = ops.fno3_mix_wgrad(X, dO, [guard.wrap(b, "cuda") for b in bases], accumulate=True)
    nans = ops.fno3_mix_wgrad(X, dO, [guard.full_nan(tuple(w.shape)) for w in ws0])
    torch.cuda.synchronize()
    Xc, dOc = FR.from_planes(X0.double()), FR.from_planes(dO0.double())
    wc = [torch.view_as_complex(w.double()) for w in ws0]
    assert torch.equal(fwd.cpu().double(), FR.to_planes(FR.mix(Xc, wc)))
    assert torch.equal(dgrad.cpu().double(), FR.to_planes(FR.mix(dOc, wc, adjoint=True)))
    for k, d in enumerate(FR.mix_wgrad(Xc, dOc)):
        ref = FR.pairs(d)
        assert torch.equal(ds[k].cpu().double(), ref), k
        assert torch.equal(nans[k].cpu().double(), ref), k
        assert torch.equal(accs[k].cpu().double(), bases[k].double() + ref), k
    guard.check()


def test_transform_workspace_outlives_its_launches(monkeypatch):
    """the workspace between the two launches of a 3-D transform must still be referenced when the library is called: a raw
    pointer alone would let the allocator free (or re-issue) it before the kernels run"""
    import weakref
    from dpot_amd import _lib, ops
    lib = _lib.load()
    B, X, Y, Z, C, m1, m2, m3 = FR.TRANSFORM_CASES[0]
    x0, S0 = FR.transform_inputs(FR.TRANSFORM_CASES[0])
    x, S = x0.cuda(), S0.cuda()
    refs, alive = [], []
    real_scratch = ops._scratch
    monkeypatch.setattr(ops, "_scratch", lambda t: refs.append(weakref.ref(t)) or real_scratch(t))
    for name in ("dpot_fno3_rfft3", "dpot_fno3_irfft3"):
        monkeypatch.setattr(lib, name, lambda *a, _r=getattr(lib, name): alive.append(refs[-1]() is not None) or _r(*a))
    ops.fno3_rfft3(x, m1, m2, m3)
    ops.fno3_irfft3(S, X, Y, Z)
    torch.cuda.synchronize()
    assert len(refs) == 2 and alive == [True, True]


def test_argument_checks_and_limits():
    from dpot_amd import _lib, ops
    lib = _lib.load()
    n = lib.dpot_fno3_max_size(0)
    with pytest.raises(ValueError, match=f"{n + 1}x8x8"):
        ops.fno3_rfft3(torch.zeros(1, n + 1, 8, 8, 4, device="cuda"), 2, 2, 2)
    with pytest.raises(ValueError):
        ops.fno3_irfft3(torch.zeros(1, 4, 4, 3, 2, 4, device="cuda"), 8, 8, n + 8)
    with pytest.raises((ValueError, _lib.DpotHipError)):
        ops.fno3_rfft3(torch.zeros(1, 8, 8, 8, 4, device="cuda").double(), 2, 2, 2)
    with pytest.raises(ValueError):
        ops.fno3_mix(torch.zeros(1, 4, 4, 3, 2, 5, device="cuda"), [torch.zeros(4, 4, 2, 2, 3, 2, device="cuda")] * 4)
    with pytest.raises(ValueError):
        ops.fno3_mix(torch.zeros(1, 4, 4, 3, 2, 4, device="cuda"), [torch.zeros(4, 4, 2, 2, 3, 2, device="cuda")] * 3)
    s = torch.cuda.current_stream().cuda_stream                 # the C entry points: DPOT_EUNSUP with the size named, no launch
    d = torch.zeros(256, device="cuda")
    p = d.data_ptr()
    assert lib.dpot_fno3_rfft3(p, p + 64, p + 128, p, p, p, 1, n + 1, 8, 8, 1, 1, 1, 1, 0, 1.0, s) == -2
    assert f"{n + 1}x8x8".encode() in lib.dpot_last_error()
    assert lib.dpot_fno3_irfft3(p, None, p + 64, None, p + 128, p, p, p, 1, 8, 8, n + 2, 1, 1, 1, 1, 1, 1.0, 0, s) == -2
    assert lib.dpot_fno3_rfft3(p, p + 64, p + 128, p, p, p, 1, 8, 8, 8, 1, 1, 5, 1, 0, 1.0, s) == -1
    torch.cuda.synchronize()
    assert not d.any()


def test_plan_under_capture_is_an_error_and_a_warmed_up_size_captures(monkeypatch):
    """a size tuple first seen while the stream captures: an error that says what to do, before anything is uploaded (the
    capture state is stubbed: aborting a real capture is not something a test should leave behind); after one eager use the
    operators capture - their workspace included - and replay to the eager bits"""
    from dpot_amd import _lib, ops
    shape, modes = (2, 7, 6, 9, 6), (3, 2, 4)                   # a size tuple no other test uses
    x = FR.hash_input(shape, 1996).cuda()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.DpotHipError, match="before capturing"):
        ops.fno3_rfft3(x, *modes)
    monkeypatch.undo()
    ws = [FR.pairs(FR.spectral_weight(n, (6, 6) + modes, 1996)).cuda() for n in FR.WEIGHT_NAMES]
    eager, _ = ops.fno3_irfft3(ops.fno3_mix(ops.fno3_rfft3(x, *modes), ws), *shape[1:4])
    static_out = torch.full_like(eager, float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        S = ops.fno3_rfft3(x, *modes)
        ops.fno3_irfft3(ops.fno3_mix(S, ws), *shape[1:4], out=static_out)
        dw = ops.fno3_mix_wgrad(S, S)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out.view(torch.int32), eager.view(torch.int32))
    x.copy_(FR.hash_input(shape, 1997))
    graph.replay()
    torch.cuda.synchronize()
    S2 = ops.fno3_rfft3(x, *modes)
    assert torch.equal(static_out, ops.fno3_irfft3(ops.fno3_mix(S2, ws), *shape[1:4])[0])
    assert torch.equal(dw[3], ops.fno3_mix_wgrad(S2, S2)[3])


# ---- the layer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FR.LAYER_CASES))
def test_spectral_conv_fn_vs_the_fixture(name, guarded):
    from dpot_amd.functional import SpectralConv3dFn
    fx = load("g23_fno3d")
    x0, g0, ws0 = FR.layer_inputs(name)
    x = guard.wrap(x0, "cuda").requires_grad_(True)
    ws = [guard.wrap(FR.pairs(w), "cuda").requires_grad_(True) for w in ws0]
    y = SpectralConv3dFn.apply(x, *ws)
    y.backward(guard.wrap(g0, "cuda"))
    torch.cuda.synchronize()
    for k, t in [("y", y.detach()), ("dx", x.grad)] + [(f"dw{j + 1}", w.grad) for j, w in enumerate(ws)]:
        e = FR.nerr(t.cpu().numpy(), fx[f"layer.{name}.{k}64"])
        print(f"fno3-layer {name}.{k}: kernels {e:.3e}  reference-fp32 {float(fx[f'layer.{name}.e32.{k}']):.3e}")
        assert_close(t, fx[f"layer.{name}.{k}64"], f"layer.{name}.{k} vs float64")
        assert_close(t, fx[f"layer.{name}.{k}32"], f"layer.{name}.{k} vs the reference's float32")


def test_frozen_spectral_weights_still_give_the_data_gradient(guarded, monkeypatch):
    """the four weights without requires_grad: no weight-gradient launch, the same dx and convolution gradients"""
    from dpot_amd import ops
    from dpot_amd.functional import FNO3dLayerFn, SpectralConv3dFn
    name = "x5y4z6_c2to5"
    B, X, Y, Z, Cin, Cout, m1, m2, m3 = FR.LAYER_CASES[name]
    x0, g0, ws0 = FR.layer_inputs(name)
    cw0, cb0 = FR.conv_inputs(Cin, Cout)
    calls = []
    real_wgrad = ops.fno3_mix_wgrad
    monkeypatch.setattr(ops, "fno3_mix_wgrad", lambda *a, **k: calls.append(1) or real_wgrad(*a, **k))
    res, launched = [], []
    for frozen in (False, True):
        calls.clear()
        x, cw, cb = (guard.wrap(t, "cuda").requires_grad_(True) for t in (x0, cw0, cb0))
        ws = [guard.wrap(FR.pairs(w), "cuda").requires_grad_(not frozen) for w in ws0]
        FNO3dLayerFn.apply(x, *ws, cw, cb, GELU).backward(guard.wrap(g0, "cuda"))
        xs = guard.wrap(x0, "cuda").requires_grad_(True)
        SpectralConv3dFn.apply(xs, *[w.detach().requires_grad_(not frozen) for w in ws]).backward(guard.wrap(g0, "cuda"))
        torch.cuda.synchronize()
        assert all((w.grad is None) == frozen for w in ws)
        res.append((x.grad, cw.grad, cb.grad, xs.grad))
        launched.append(len(calls))
    assert launched == [2, 0]
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", list(FR.LAYER_CASES))
def test_whole_layer_vs_restatement(name, guarded):
    """gelu(spectral + 1x1x1 convolution), Cin != Cout included, every gradient against the float64 restatement's autograd"""
    from dpot_amd.functional import FNO3dLayerFn
    B, X, Y, Z, Cin, Cout, m1, m2, m3 = FR.LAYER_CASES[name]
    x0, g0, ws0 = FR.layer_inputs(name)
    cw0, cb0 = FR.conv_inputs(Cin, Cout)
    x, cw, cb = (guard.wrap(t, "cuda").requires_grad_(True) for t in (x0, cw0, cb0))
    ws = [guard.wrap(FR.pairs(w), "cuda").requires_grad_(True) for w in ws0]
    y = FNO3dLayerFn.apply(x, *ws, cw, cb, GELU)
    y.backward(guard.wrap(g0, "cuda"))
    torch.cuda.synchronize()
    xr, cwr, cbr = (t.double().requires_grad_(True) for t in (x0, cw0, cb0))
    wr = [w.to(torch.complex128).requires_grad_(True) for w in ws0]
    y64 = FR.fno3_layer(xr, wr, cwr, cbr)
    (y64 * g0.double()).sum().backward()
    assert_close(y, y64.detach(), f"layer {name} y")
    for nm, a, b in [("dx", x, xr), ("dconv.weight", cw, cwr), ("dconv.bias", cb, cbr)]:
        assert_close(a.grad, b.grad, f"layer {name} {nm}")
    for k, (a, b) in enumerate(zip(ws, wr)):
        assert_close(a.grad, FR.pairs(b.grad), f"layer {name} dweights{k + 1}")


# ---- the model ---------------------------------------------------------------------------------------------------------------
def build(cfg, salt):
    from dpot_amd import FNO3d
    m = FNO3d(**cfg)
    sd = FR.recipe_sd(OrderedDict((k, (tuple(v.shape), v.dtype)) for k, v in m.state_dict().items()), salt)
    m.load_state_dict(sd, strict=True)
    return m.cuda(), sd


@pytest.mark.parametrize("tag", list(FR.MODELS))
def test_mini_model_vs_reference(tag):
    """non-cubic windows; m2 has use_ln and normalize (scale_feats exists, is never read and gets no gradient)"""
    from dpot_amd.functional import rel_l2_loss
    fx = load("g23_fno3d")
    cfg, size, salt = FR.MODELS[tag]
    m, _ = build(cfg, salt)
    x, y, msk = (t.cuda() for t in FR.model_inputs(tag))
    x.requires_grad_(True)
    pred = m(x)
    assert torch.is_tensor(pred) and tuple(pred.shape) == tuple(y.shape)
    rel_l2_loss(pred, y, msk).backward()
    torch.cuda.synchronize()
    p64, g64, dx64 = FR.run_model_ref(tag)
    assert_close(pred, fx[f"{tag}.pred"], f"{tag}.pred")
    assert_close(pred, p64, f"{tag}.pred vs float64")
    assert_close(x.grad.reshape(-1)[::FR.DX_STRIDE], fx[f"{tag}.dx"], f"{tag}.dx")
    assert_close(x.grad, dx64, f"{tag}.dx vs float64")
    grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert sorted(grads) == sorted(str(n) for n in fx[f"{tag}.gnames"])
    assert [k for k, p in m.named_parameters() if p.grad is None] == [str(n) for n in fx[f"{tag}.nograd"]]
    for k, g in grads.items():
        assert_close(g, fx[f"{tag}.g.{k}"], f"{tag}.g.{k}")
        assert_close(g, g64[k], f"{tag}.g.{k} vs float64")


def _flat_of(model, names, of):
    params = dict(model.named_parameters())
    flat = torch.cat([FR.pair_stride(of(params[n]).detach().reshape(-1)) for n in names]).cpu()
    owner = torch.cat([torch.full((FR.pair_stride(params[n].detach().reshape(-1)).numel(),), i, dtype=torch.int64)
                       for i, n in enumerate(names)])
    return flat, owner


def _step_batch():
    return tuple(t.cuda() for t in FR.step_inputs())


def _opt(m, cls=None, **kw):
    from dpot_amd.train import FlatParams, FusedAdam
    st = FR.STEP
    return (cls or FusedAdam)(FlatParams(m), lr=st["lr"], betas=st["betas"], weight_decay=st["weight_decay"],
                              max_norm=st["max_norm"], **kw)


def test_two_ar_step_train_step_vs_reference():
    """finetune3d.py's loop, two AR steps, noise off: losses, gradient before the clip, its norm (also as StepMetrics reports
    it), parameters after the reference's Adam on complex parameters.  Gradients per tensor at the contract, parameters at
    fno3d_ref.step_param_tolerance (the contract plus what the first Adam step makes of a gradient within its tolerance).
    Without the pair rule the spectral weights miss that tolerance (tests/test_cpu_fno3d.py prints the margin)."""
    from dpot_amd import StepMetrics
    from dpot_amd.train import train_step
    fx = load("g23_fno3d")
    st = FR.STEP
    m, sd0 = build(FR.MINI1, st["salt"])
    xx, yy, msk = _step_batch()
    opt = _opt(m)
    assert opt.pair_ranges is not None and opt.pair_ranges.shape == (8, 2)
    met = StepMetrics("cuda", st["T_ar"])
    loss, pred = train_step(m, opt, xx, yy, msk, lr=st["lr"], metrics=met)
    torch.cuda.synchronize()
    assert tuple(pred.shape) == tuple(yy.shape)
    assert_close(loss, fx["step.loss"], "step loss")
    gnorm = float(fx["step.grad_norm"])
    assert abs(opt.grad_norm().item() - gnorm) <= 1e-4 * gnorm
    assert abs(met.read()["grad_norm"] - gnorm) <= 1e-4 * gnorm
    names = [str(n) for n in fx["step.names"]]
    assert names == [n for n, _ in m.named_parameters()]
    got_g, owner = _flat_of(m, names, lambda p: p.grad)
    got_p, _ = _flat_of(m, names, lambda p: p)
    ref_g, ref_p = torch.from_numpy(fx["step.grad"]).double(), torch.from_numpy(fx["step.params"]).double()
    p0 = torch.cat([FR.pair_stride((FR.pairs(sd0[n]) if sd0[n].is_complex() else sd0[n]).reshape(-1)) for n in names]).double()
    assert got_g.shape == ref_g.shape and got_p.shape == ref_p.shape
    tol = FR.step_param_tolerance(ref_g, ref_p, p0, owner, names, gnorm)
    for i, n in enumerate(names):
        sel = owner == i
        assert_close(got_g[sel], ref_g[sel], f"step gradient {n}")
        err = (got_p[sel].double() - ref_p[sel]).abs()
        print(f"step parameters {n}: worst err / tol {float((err / tol[sel]).max()):.2e}")
        assert torch.isfinite(got_p[sel]).all() and (err <= tol[sel]).all(), \
            (f"step parameters {n}: {int((err > tol[sel]).sum())}/{err.numel()} out of tolerance, worst "
             f"{float((err / tol[sel]).max()):.2f} x the tolerance")
    # both slots of a pair hold the one second moment
    v = opt.exp_avg_sq
    for lo, hi in opt.pair_ranges.cpu().tolist():
        pr = v[lo:hi].view(-1, 2)
        assert torch.equal(pr[:, 0], pr[:, 1]) and (pr > 0).any()


def test_graphed_train_step_replays_the_eager_step_bit_for_bit():
    from dpot_amd.train import GraphedTrainStep, train_step
    st = FR.STEP
    xx, yy, msk = _step_batch()
    runs = []
    for graphed in (False, True):
        m, _ = build(FR.MINI1, st["salt"])
        opt = _opt(m)
        if graphed:
            step = GraphedTrainStep(m, opt, xx, yy, msk, warmup=1)
            loss, pred = step.replay(st["lr"]).clone(), step.pred.clone()
        else:
            loss, pred = train_step(m, opt, xx, yy, msk, lr=st["lr"])
        torch.cuda.synchronize()
        runs.append((loss.clone(), pred.clone(), {n: p.detach().clone() for n, p in m.named_parameters()},
                     opt.exp_avg_sq.clone()))
    (l0, p0, w0, v0), (l1, p1, w1, v1) = runs
    assert torch.equal(l1, l0) and torch.equal(p1, p0) and torch.equal(v1, v0)
    start, _ = build(FR.MINI1, st["salt"])
    for n, p in start.named_parameters():
        assert torch.equal(w1[n], w0[n]), n
        assert not torch.equal(w0[n], p.detach()), n


@functools.lru_cache(maxsize=None)
def _rollout_model():
    m, sd = build(FR.MINI2, 1850)
    return m.eval(), {k: v.to(torch.complex128 if v.is_complex() else torch.float64) for k, v in sd.items()}


def test_rollouts_on_a_6d_window_with_an_evaluator():
    """rollout_eval against the float64 restatement's rollout; GraphedRollout and a checkpoint-loaded copy reproduce it bit for
    bit, and a RolloutEvaluator reads the same from both"""
    from dpot_amd import FNO3d, RolloutEvaluator
    from dpot_amd.infer import GraphedRollout, load_model_from_checkpoint, rollout_eval
    m, sd = _rollout_model()
    cfg = FR.MINI2
    B, T_ar, (X, Y, Z) = 2, 3, (4, 6, 5)
    xx = FR.hash_input((B, X, Y, Z, cfg["in_timesteps"], cfg["n_channels"]), 1851)
    yy = FR.hash_input((B, X, Y, Z, T_ar, cfg["n_channels"]), 1852)
    msk = torch.ones(B, X, Y, Z, 1, cfg["n_channels"])
    msk[1, ..., 1] = 0.0
    with torch.no_grad():
        cur, loss_ref, preds = xx.double(), 0.0, []
        for t in range(T_ar):
            im = FR.fno3_forward(sd, cur, cfg)
            loss_ref = loss_ref + R.rel_l2_loss(im, yy.double()[..., t:t + 1, :], msk.double())
            preds.append(im)
            cur = torch.cat((cur[..., 1:, :], im), dim=-2)
        pred_ref = torch.cat(preds, dim=-2)
        full_ref = R.rel_l2_loss(pred_ref, yy.double(), msk.double())
    xx, yy, msk = xx.cuda(), yy.cuda(), msk.cuda()
    ev1, ev2 = (RolloutEvaluator("cuda", n_channels=cfg["n_channels"], T_max=T_ar, ilow=1, ihigh=2) for _ in range(2))
    pred, l_steps, l_full = rollout_eval(m, xx, yy, msk, evaluator=ev1)
    assert tuple(pred.shape) == (B, X, Y, Z, T_ar, cfg["n_channels"])
    assert_close(pred, pred_ref, "rollout pred")
    assert_close(l_steps, loss_ref, "sum of step losses")
    assert_close(l_full, full_ref, "full-trajectory loss")
    m2 = FNO3d(**cfg)
    load_model_from_checkpoint(m2, {"model": OrderedDict(("module." + k, v.cpu()) for k, v in m.state_dict().items())})
    g = GraphedRollout(m2.cuda().eval(), torch.zeros_like(xx))
    assert g.cls is None
    pred_g, l_steps_g, l_full_g = g(xx, yy, msk, evaluator=ev2)
    torch.cuda.synchronize()
    assert torch.equal(pred_g, pred) and torch.equal(l_steps_g, l_steps) and torch.equal(l_full_g, l_full)
    r1, r2 = ev1.read(), ev2.read()
    assert set(r1) == set(r2) and r1["samples"] == B
    for k in r1:
        assert np.array_equal(np.asarray(r1[k]), np.asarray(r2[k]), equal_nan=True), k     # an empty band of a tiny grid: NaN


def test_adam_entry_by_model_and_lamb_refusal(monkeypatch):
    """a model without pair tensors (an FNO2d mini) takes the old Adam entry and never the pair one; FNO3d the pair one;
    FusedLamb on FNO3d raises and names the first pair parameter"""
    from dpot_amd import FNO2d, ops
    from dpot_amd.train import FlatParams, FusedAdam, FusedLamb
    calls = []
    for name in ("adam_step", "adam_step_pairs", "adam_step_packs"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: calls.append(_n) or _r(*a, **k))
    m2 = FNO2d(2, 2, 8, img_size=6, n_channels=2, in_timesteps=3, n_cls=1).cuda()
    opt2 = FusedAdam(FlatParams(m2), lr=1e-3, max_norm=1.0)
    assert opt2.pair_ranges is None
    opt2.fp.grad.fill_(1e-3)
    opt2.step()
    assert calls == ["adam_step"]
    calls.clear()
    m3, _ = build(FR.MINI1, 1860)
    opt3 = _opt(m3)
    opt3.fp.grad.fill_(1e-3)
    opt3.step()
    torch.cuda.synchronize()
    assert calls == ["adam_step_pairs"]
    m4, _ = build(FR.MINI1, 1860)
    with pytest.raises(ValueError, match=r"spectral_convs\.0\.weights1"):
        _opt(m4, FusedLamb)


def test_pair_adam_kernel_vs_the_float64_formula(guarded):
    """dpot_adam_step_pairs on a flat buffer with a real tensor, a pair tensor and a real tensor again (ragged tail, gradients
    spread over six decades, some far below eps): pairs follow the pair formula, the rest dpot_adam_step bit for bit"""
    from dpot_amd import ops
    n, lo, hi = 4 * 700 + 8, 1000, 2200
    p0 = FR.hash_input((n,), 1870)
    g0 = FR.hash_input((n,), 1871) * (10.0 ** (-6.0 * R.recipe_tensor("mag", (n,), 1872))).float()
    g0[lo:lo + 8] *= 1e-9
    st = FR.STEP
    bufs = []
    for pairs_on in (False, True):
        p, g = guard.wrap(p0, "cuda"), guard.wrap(g0, "cuda")
        m, v = guard.wrap(torch.zeros(n), "cuda"), guard.wrap(torch.zeros(n), "cuda")
        hyper, step = torch.zeros(8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        ops.adam_stage(hyper, step, st["lr"], st["betas"][0], st["betas"][1], st["eps"], st["weight_decay"], 0.0, 1)
        if pairs_on:
            ops.adam_step_pairs(p, g, m, v, hyper, None, ops.adam_pair_ranges([(lo, hi)], "cuda"))
        else:
            ops.adam_step(p, g, m, v, hyper, None)
        torch.cuda.synchronize()
        bufs.append((p.cpu(), m.cpu(), v.cpu()))
    (pa, ma, va), (pb, mb, vb) = bufs
    out = torch.ones(n, dtype=torch.bool)
    out[lo:hi] = False
    for a, b in ((pa, pb), (ma, mb), (va, vb)):
        assert torch.equal(a[out], b[out])
    assert torch.equal(ma, mb)                                                   # the first moment is per component everywhere
    want = FR.adam_first_step(p0[lo:hi], g0[lo:hi], 0.0, True)                   # gnorm 0: clip coefficient 1
    move, got = (want - p0[lo:hi].double()).abs(), pb[lo:hi].double()
    assert ((got - want).abs() <= 2.0 ** -22 * p0[lo:hi].abs().double() + 1e-5 * move).all()
    pr = vb[lo:hi].view(-1, 2)
    assert torch.equal(pr[:, 0], pr[:, 1])
    guard.check()
