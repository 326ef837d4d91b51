"""GPU tests of the UNet operators (csrc/unet.hip through ops.conv3x3 / conv3x3_bwd_data / conv3x3_wgrad / bn_stats / bn_act /
bn_act_bwd and functional.ConvBNActFn / UpConv2Fn) against the float64 restatement (tests/unet_ref.py), on the guarded, poisoned
allocator (tests/guard.py).  Shapes (B, H, W, Cin, Cout) of unet_ref.OP_SHAPES:

  (1, 1, 1, 1, 1)      smallest possible
  (2, 1, 1, 5, 3)      only the centre tap contributes: the bottleneck of a 16x16 window; B H W = 2 (the unbiased factor 2)
  (1, 2, 3, 3, 2)      tiny, all sizes different
  (2, 5, 7, 6, 10)     odd sizes, scalar path
  (3, 6, 6, 4, 8)      36 pixels per sample: a 128-pixel tile spans rows AND samples - the halo must not leak across either
  (1, 16, 16, 8, 2)    Cin = 8: the flattened (T, C) of the fixture model plus the 2 grid channels; ragged narrow N
  (1, 33, 17, 4, 36)   ragged pixel tile (561 = 4 x 128 + 49) and ragged N tile (36 = 32 + 4)
  (1, 8, 8, 128, 16)   more than one K chunk (8 of 16 channels)
  (2, 4, 4, 32, 64)    clean multiples of the tile sizes, 16-byte path
"""
import pytest
import torch

import guard
import unet_ref as UR
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close

pytestmark = pytest.mark.gpu

IDS = ["b%d_%dx%d_c%dto%d" % s for s in UR.OP_SHAPES]
RSTD_TOL = dict(rtol=2e-5, atol_scale=2e-5)          # the bound of the GroupNorm statistics tests (tests/gn_cases.py TOL)


def _conv_inputs(shape, integer=False):
    B, H, W, Cin, Cout = shape
    make = (lambda s, salt: UR.ints(s, salt)) if integer else UR.hash_input
    return make((B, H, W, Cin), 701), make((Cout, Cin, 3, 3), 702), make((B, H, W, Cout), 703)


def _run_conv(shape, integer):
    from dpot_amd import ops
    x0, w0, dz0 = _conv_inputs(shape, integer)
    x, w, dz = (guard.wrap(t, "cuda") for t in (x0, w0, dz0))
    got = {"fwd": ops.conv3x3(x, w), "dgrad": ops.conv3x3_bwd_data(dz, w), "wgrad": ops.conv3x3_wgrad(x, dz)}
    base0 = UR.ints(w0.shape, 704) if integer else UR.hash_input(w0.shape, 704)
    acc = guard.wrap(base0, "cuda")
    r = ops.conv3x3_wgrad(x, dz, out=acc, accumulate=True)
    o = ops.conv3x3_wgrad(x, dz, out=guard.full_nan(tuple(w0.shape)))
    zs, part = ops.conv3x3(x, w, stats=True)
    torch.cuda.synchronize()
    assert r is acc and torch.equal(o, got["wgrad"]) and torch.equal(zs, got["fwd"])
    ref = {"fwd": UR.conv3x3(x0.double(), w0.double()), "dgrad": UR.conv3x3_bwd_data(dz0.double(), w0.double()),
           "wgrad": UR.conv3x3_wgrad(x0.double(), dz0.double())}
    return got, ref, acc, base0, part


@pytest.mark.parametrize("shape", UR.OP_SHAPES, ids=IDS)
def test_convolution_vs_float64(shape, guarded):
    """forward, data gradient, weight gradient (written, into an out= slot, and added); the epilogue's statistics partials
    merged by bn_stats against the float64 batch statistics of the same field"""
    from dpot_amd import ops
    got, ref, acc, base0, part = _run_conv(shape, integer=False)
    for k in ref:
        assert tuple(got[k].shape) == tuple(ref[k].shape), k
        assert_close(got[k], ref[k], f"conv3x3 {shape} {k}")
    assert torch.equal(acc.cpu(), base0 + got["wgrad"].cpu())                     # one fp32 add per element
    B, H, W, Cin, Cout = shape
    if B * H * W > 1:
        mean, invstd = ops.bn_stats(part, B * H * W, Cout)
        torch.cuda.synchronize()
        m64, _, i64 = UR.bn_stats(ref["fwd"])
        assert_close(mean, m64, f"{shape} batch mean")
        assert_close(invstd, i64, f"{shape} invstd", **RSTD_TOL)
    else:
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            ops.bn_stats(part, 1, Cout)
    guard.check()


@pytest.mark.parametrize("shape", UR.OP_SHAPES, ids=IDS)
def test_convolution_is_exact_on_small_integers(shape, guarded):
    """operands in [-3, 3]: every partial sum is an integer below 2^24, so fp32 is exact in any order - the results equal the
    restatement bit for bit.  A wrong tap, a mirrored tap or one dropped halo element cannot hide in a tolerance"""
    got, ref, acc, base0, _ = _run_conv(shape, integer=True)
    for k in ref:
        assert float(ref[k].abs().max()) < 2 ** 24
        assert torch.equal(got[k].cpu().double(), ref[k]), (shape, k, float((got[k].cpu().double() - ref[k]).abs().max()))
    assert torch.equal(acc.cpu().double(), base0.double() + ref["wgrad"])
    guard.check()


def _identity_weight(C):
    w = torch.zeros(C, C, 3, 3)
    for c in range(C):
        w[c, c, 1, 1] = 1.0
    return w


def test_batch_statistics_of_a_field_with_mean_1e3_and_std_1(guarded):
    """sum and sum of squares cancel in fp32 here (1e6 against 1); the Welford / Chan partials do not.  The convolution is the
    identity (centre tap), so the field the statistics see is the input itself: 960 pixels, 8 tiles, the last one ragged"""
    from dpot_amd import ops
    B, H, W, C = 2, 24, 20, 4
    x0 = (1e3 + UR.hash_input((B, H, W, C), 711) / 0.866).float()               # the recipe is uniform on [-1.5, 1.5): std 0.866
    z, part = ops.conv3x3(guard.wrap(x0, "cuda"), guard.wrap(_identity_weight(C), "cuda"), stats=True)
    mean, invstd = ops.bn_stats(part, B * H * W, C)
    torch.cuda.synchronize()
    assert torch.equal(z.cpu(), x0)
    m64, v64, i64 = UR.bn_stats(x0.double())
    assert float((v64 - 1).abs().max()) < 0.1
    assert_close(mean, m64, "mean", rtol=1e-6, atol_scale=1e-6)
    assert_close(invstd, i64, "invstd", **RSTD_TOL)
    guard.check()


@pytest.mark.parametrize("shape", [(2, 1, 1, 5, 3), (3, 6, 6, 4, 8)], ids=["two_values", "b3_6x6"])
def test_running_buffers_after_two_calls(shape, guarded):
    """momentum 0.1, the UNBIASED variance (at B H W = 2 twice the biased one), the int64 counter - twice, from buffers that are
    neither 0 nor 1"""
    from dpot_amd import ops
    B, H, W, Cin, Cout = shape
    x0, w0, _ = _conv_inputs(shape)
    rm0, rv0 = UR.hash_input((Cout,), 721), UR.hash_input((Cout,), 722).abs() + 0.5
    rm, rv = guard.wrap(rm0, "cuda"), guard.wrap(rv0, "cuda")
    nbt = guard.wrap(torch.tensor(7, dtype=torch.int64), "cuda")
    x, w = guard.wrap(x0, "cuda"), guard.wrap(w0, "cuda")
    z64 = UR.conv3x3(x0.double(), w0.double())
    want = (rm0.double(), rv0.double(), torch.tensor(7))
    for _ in range(2):
        _, part = ops.conv3x3(x, w, stats=True)
        ops.bn_stats(part, B * H * W, Cout, rm, rv, nbt)
        want = UR.bn_running(z64, *want)
    torch.cuda.synchronize()
    assert_close(rm, want[0], "running_mean")
    assert_close(rv, want[1], "running_var")
    assert int(nbt) == 9
    guard.check()


BN_SHAPES = [(2, 6, 8, 8), (1, 2, 6, 5), (3, 4, 2, 3), (2, 64, 40, 4), (2, 5, 7, 6)]       # the last one: no pooling (odd)


@pytest.mark.parametrize("name", ["gelu", "relu", "leaky_relu"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "b%d_%dx%d_c%d" % s)
def test_bn_act_with_pooling_forward_and_backward(shape, name, guarded):
    """(2, 6, 8, 8) the 16-byte path; (1, 2, 6, 5) H = 2 and an odd C; (3, 4, 2, 3) W = 2; (2, 64, 40, 4) 5120 pixels: three
    backward chunks and several workgroups; (2, 5, 7, 6) odd field, no pooling.  relu runs on an integer field with gamma 1,
    beta 0, mean 0, invstd 1: its zeros tie in most windows, and the pooled gradient must land on the first of them."""
    from dpot_amd import ops
    B, H, W, C = shape
    pool = H % 2 == 0 and W % 2 == 0
    if name == "relu":
        z0 = UR.ints(shape, 731, -2, 2)
        mean0, inv0, gamma0, beta0 = torch.zeros(C), torch.ones(C), torch.ones(C), torch.zeros(C)
    else:
        z0 = UR.hash_input(shape, 731)
        mean0, inv0 = UR.hash_input((C,), 732) * 0.2, UR.hash_input((C,), 733).abs() + 0.5
        gamma0, beta0 = UR.hash_input((C,), 734) + 2.0, UR.hash_input((C,), 735) * 0.3
    dy0 = UR.hash_input(shape, 736)
    dp0 = UR.hash_input((B, H // 2, W // 2, C), 737) if pool else None
    z, mean, inv, gamma, beta, dy = (guard.wrap(t, "cuda") for t in (z0, mean0, inv0, gamma0, beta0, dy0))
    dp = guard.wrap(dp0, "cuda") if pool else None
    act = UR.ACT_IDS[name]
    out = ops.bn_act(z, mean, inv, gamma, beta, act, pool)
    y, yp = out if pool else (out, None)
    dz, dgamma, dbeta = ops.bn_act_bwd(dy, dp, z, mean, inv, gamma, beta, act)
    torch.cuda.synchronize()
    d = lambda t: t.double()
    ref = UR.bn_act(d(z0), d(mean0), d(inv0), d(gamma0), d(beta0), name, pool)
    y64, yp64 = ref if pool else (ref, None)
    assert_close(y, y64, f"{name} y")
    if pool:
        if name == "relu":
            win = y64.reshape(B, H // 2, 2, W // 2, 2, C)
            assert int(((win == win.amax(dim=(2, 4), keepdim=True)).sum(dim=(2, 4)) > 1).sum()) > 0          # ties are there
            assert torch.equal(yp.cpu().double(), yp64)
        assert_close(yp, yp64, f"{name} pooled")
        only_pool = ops.bn_act_bwd(None, dp, z, mean, inv, gamma, beta, act)
        torch.cuda.synchronize()
        for k, a, b in zip(("dz", "dgamma", "dbeta"), only_pool,
                           UR.bn_act_bwd(None, d(dp0), d(z0), d(mean0), d(inv0), d(gamma0), d(beta0), name)):
            assert_close(a, b, f"{name} pooled gradient alone: {k}")
    r = UR.bn_act_bwd(d(dy0), d(dp0) if pool else None, d(z0), d(mean0), d(inv0), d(gamma0), d(beta0), name)
    for k, a, b in zip(("dz", "dgamma", "dbeta"), (dz, dgamma, dbeta), r):
        assert_close(a, b, f"{name} {shape} {k}")
    guard.check()


def test_eval_mode_reads_the_running_statistics_and_writes_nothing(guarded):
    from dpot_amd.functional import ConvBNActFn
    shape = (2, 4, 6, 4, 8)
    B, H, W, Cin, Cout = shape
    x0, w0, _ = _conv_inputs(shape)
    rm0, rv0 = UR.hash_input((Cout,), 741), UR.hash_input((Cout,), 742).abs() + 0.5
    gamma0, beta0 = UR.hash_input((Cout,), 743) + 2.0, UR.hash_input((Cout,), 744)
    x, w, rm, rv, gamma, beta = (guard.wrap(t, "cuda") for t in (x0, w0, rm0, rv0, gamma0, beta0))
    nbt = guard.wrap(torch.tensor(5, dtype=torch.int64), "cuda")
    w.requires_grad_(True)
    y, yp = ConvBNActFn.apply(x, w, gamma, beta, rm, rv, nbt, UR.ACT_IDS["gelu"], True, False)
    torch.cuda.synchronize()
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and int(nbt) == 5
    z64 = UR.conv3x3(x0.double(), w0.double())
    y64, yp64 = UR.bn_act(z64, rm0.double(), 1 / torch.sqrt(rv0.double() + UR.EPS), gamma0.double(), beta0.double(), "gelu", True)
    assert_close(y, y64, "eval y")
    assert_close(yp, yp64, "eval pooled")
    with pytest.raises(RuntimeError, match="eval mode"):
        y.sum().backward()
    guard.check()


def test_layer_function_trains_and_counts(guarded):
    """ConvBNActFn in training mode end to end on a pooled layer: outputs, the four gradients, the buffers"""
    from dpot_amd.functional import ConvBNActFn
    shape = (2, 6, 4, 5, 7)
    B, H, W, Cin, Cout = shape
    x0, w0, _ = _conv_inputs(shape)
    gamma0, beta0 = UR.hash_input((Cout,), 751) + 2.0, UR.hash_input((Cout,), 752)
    gy0, gp0 = UR.hash_input((B, H, W, Cout), 753), UR.hash_input((B, H // 2, W // 2, Cout), 754)
    x, w, gamma, beta, gy, gp = (guard.wrap(t, "cuda") for t in (x0, w0, gamma0, beta0, gy0, gp0))
    rm, rv = guard.wrap(torch.zeros(Cout), "cuda"), guard.wrap(torch.ones(Cout), "cuda")
    nbt = guard.wrap(torch.tensor(0, dtype=torch.int64), "cuda")
    for t in (x, w, gamma, beta):
        t.requires_grad_(True)
    y, yp = ConvBNActFn.apply(x, w, gamma, beta, rm, rv, nbt, UR.ACT_IDS["gelu"], True, True)
    ((y * gy).sum() + (yp * gp).sum()).backward()
    torch.cuda.synchronize()
    z64 = UR.conv3x3(x0.double(), w0.double())
    mean, _, inv = UR.bn_stats(z64)
    y64, yp64 = UR.bn_act(z64, mean, inv, gamma0.double(), beta0.double(), "gelu", True)
    dz, dgamma, dbeta = UR.bn_act_bwd(gy0.double(), gp0.double(), z64, mean, inv, gamma0.double(), beta0.double(), "gelu")
    assert_close(y, y64, "y")
    assert_close(yp, yp64, "pooled")
    assert_close(gamma.grad, dgamma, "dgamma")
    assert_close(beta.grad, dbeta, "dbeta")
    assert_close(w.grad, UR.conv3x3_wgrad(x0.double(), dz), "dw")
    assert_close(x.grad, UR.conv3x3_bwd_data(dz, w0.double()), "dx")
    want = UR.bn_running(z64, torch.zeros(Cout).double(), torch.ones(Cout).double(), torch.tensor(0))
    assert_close(rm, want[0], "running_mean")
    assert_close(rv, want[1], "running_var")
    assert int(nbt) == 1
    guard.check()


@pytest.mark.parametrize("dims", [(2, 3, 5, 6, 4), (1, 1, 1, 3, 5)], ids=str)
def test_transposed_convolution(dims, guarded):
    from dpot_amd.functional import UpConv2Fn
    B, h, w, Cin, Cout = dims
    x0, W0, b0 = UR.hash_input((B, h, w, Cin), 761), UR.hash_input((Cin, Cout, 2, 2), 762), UR.hash_input((Cout,), 763)
    g0 = UR.hash_input((B, 2 * h, 2 * w, Cout), 764)
    x, W, b, g = (guard.wrap(t, "cuda") for t in (x0, W0, b0, g0))
    for t in (x, W, b):
        t.requires_grad_(True)
    y = UpConv2Fn.apply(x, W, b)
    (y * g).sum().backward()
    torch.cuda.synchronize()
    assert_close(y, UR.upconv2(x0.double(), W0.double(), b0.double()), "upconv y")
    dx, dW, db = UR.upconv2_bwd(g0.double(), x0.double(), W0.double())
    assert_close(x.grad, dx, "upconv dx")
    assert_close(W.grad, dW, "upconv dW")
    assert_close(b.grad, db, "upconv db")
    guard.check()


def test_sizes_beyond_the_limit_are_named():
    from dpot_amd import ops
    max_w, _ = ops.unet_limits()
    x = torch.zeros(1, 1, max_w + 1, 1, device="cuda")
    with pytest.raises(ValueError, match=str(max_w + 1)):
        ops.conv3x3(x, torch.zeros(1, 1, 3, 3, device="cuda"))
    with pytest.raises(ValueError, match="even field"):
        ops.bn_act(torch.zeros(1, 3, 4, 1, device="cuda"), *(torch.zeros(1, device="cuda"),) * 4, 1, pool=True)
