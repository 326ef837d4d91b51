"""GPU parity tests of the streaming kernels of csrc/loss_opt.hip: relative-L2 loss, noise injection (explicit eps, in-kernel
generator, backward) and the window slide, on every code path the kernels choose by channel count, pointer alignment, chunk
count and unroll depth.  Shapes: tests/streaming_cases.py (their premises are asserted in tests/test_cpu_streaming.py).
References: float64 torch / oracle/dpot_ref.py on the same seeded inputs; the generator against tests/philox_ref.py.
Tolerance: helpers.assert_close at its default (rtol 1e-4 + 1e-4 * max|ref|); the loss scalar 1e-5 relative."""
import pytest
import torch

import guard
from guard import guarded  # noqa: F401  (fixture)
import philox_ref
import streaming_cases as SC
from helpers import assert_close
from oracle import dpot_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dpot_amd import ops as _ops
    from dpot_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(autouse=True)
def _guard(guarded):
    """every test of this module runs on guarded, poisoned allocations (tests/guard.py) and checks the guards when it ends"""
    yield guarded


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def dev(t, off=0):
    """a test input on the GPU inside a guarded buffer; off > 0: a view that starts `off` floats into a larger buffer"""
    if not off:
        return guard.wrap(t, "cuda")
    buf = guard.wrap(torch.cat([torch.zeros(off), t.reshape(-1), torch.zeros(4 - off % 4)]), "cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 4 * (off % 4) and v.is_contiguous()
    return v


# ---- relative-L2 loss ------------------------------------------------------------------------------------------------------
_rel_l2_cache = {}


def _rel_l2_inputs(case, masked):
    """x, y, mask and the float64 reference (loss, d(1.7 loss)/dx, the [B, C, 4] statistics) - computed once per case"""
    key = (case.shape, masked)
    if key not in _rel_l2_cache:
        B, C, Tt = case.B, case.C, case.Tt
        x, y = rnd(*case.shape, seed=1), rnd(*case.shape, seed=2)            # continuous draws: x != y everywhere
        msk = None
        if masked:
            msk = torch.ones(case.shape[:-2] + (1, C))
            flat = msk.view(B, -1, C)
            if C > 1:
                flat[0, :, 1] = 0.0              # one fully dead channel in one sample (at C == 1 it would leave sample 0 with
                #                                  no live channel: the reference itself is then 0 / 0, nothing to compare)
            flat[B - 1, ::3, C - 1] = 0.0        # one partly dead channel
        xr = x.double().requires_grad_(True)
        lref = R.rel_l2_loss(xr, y.double(), msk.double() if masked else None)
        (lref * 1.7).backward()
        m = (msk.double() if masked else torch.ones(case.shape[:-2] + (1, C), dtype=torch.float64))
        d2 = (((x.double() - y.double()) * m) ** 2).reshape(B, -1, C).sum(1)
        y2 = ((y.double() * m) ** 2).reshape(B, -1, C).sum(1)
        ms = m.reshape(B, -1, C).sum(1)
        stats = torch.stack([d2, y2, ms, d2.sqrt() / (y2.sqrt() + 1e-8)], dim=-1)
        _rel_l2_cache[key] = (x, y, msk, lref.detach(), xr.grad, stats)
    return _rel_l2_cache[key]


def _rel_l2_run(ops, case, masked, off):
    from dpot_amd.functional import rel_l2_loss
    x, y, msk, _, _, _ = _rel_l2_inputs(case, masked)
    B, S, C, Tt = case.B, case.S, case.C, case.Tt
    xd, yd = dev(x, off), dev(y, off)
    md = dev(msk) if masked else None
    xg = xd.requires_grad_(True)
    loss = rel_l2_loss(xg, yd, md)
    (loss * 1.7).backward()
    # the same through the op-level entry points, where the statistics can be inspected.  Tt is passed with and without a
    # mask (functional passes 1 without one): "sum m" then counts the S / Tt grid points either way
    l2, stats = ops.rel_l2_fwd(xd.detach(), yd, md, B, S, C, Tt)
    assert stats.shape == (1 + case.chunks, B, C, 4)
    dx2 = ops.rel_l2_bwd(xd.detach(), yd, md, stats, dev(torch.tensor([1.7])), B, S, C, Tt)
    assert torch.equal(l2.view(()), loss.detach()) and torch.equal(dx2, xg.grad)
    return loss.detach().cpu(), xg.grad.cpu(), stats[0].cpu()


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("case", SC.REL_L2, ids=lambda c: c.name)
def test_rel_l2_paths(ops, case, masked):
    _, _, _, lref, gref, sref = _rel_l2_inputs(case, masked)
    loss, dx, stats = _rel_l2_run(ops, case, masked, case.off)
    what = f"rel_l2 {case.name} {'mask' if masked else 'no mask'}"
    print(f"{what}: loss {loss.item():.9g} reference {lref.item():.9g} rel err {abs(loss.item() - lref.item()) / abs(lref.item()):.2e}")
    assert abs(loss.item() - lref.item()) <= 1e-5 * abs(lref.item()), what
    assert_close(dx, gref, what + " dx")
    for k, name in enumerate(("sum ((x-y) m)^2", "sum (y m)^2", "sum m", "channel term")):
        assert_close(stats[..., k], sref[..., k], f"{what} stats[{k}] = {name}")
    if case.off:
        # the generic path at C == 4 must agree with the float4 path of the aligned run
        loss_a, dx_a, stats_a = _rel_l2_run(ops, case, masked, 0)
        assert abs(loss.item() - loss_a.item()) <= 1e-5 * abs(loss_a.item())
        assert_close(dx, dx_a, what + " dx vs aligned run")
        for k in range(4):
            assert_close(stats[..., k], stats_a[..., k], f"{what} stats[{k}] vs aligned run")


# ---- noise injection -------------------------------------------------------------------------------------------------------
def _noise_ref(x, eps, s, B, S, C):
    """float64 xx + s * ||xx||_(over S per (b, c')) * eps on the [B, S, C'] view (train_temporal.py:205, finetune3d.py:210)"""
    xv, ev = x.reshape(B, S, C), eps.reshape(B, S, C)
    return (xv + s * (xv ** 2).sum(1, keepdim=True).sqrt() * ev).reshape(x.shape)


@pytest.mark.parametrize("case", SC.NOISE_FWD, ids=lambda c: c.name)
def test_noise_forward_explicit_eps(ops, case):
    B, S, C = case.B, case.S, case.C
    s = 0.05
    x = rnd(*case.shape, seed=11) * (1.0 + torch.arange(case.shape[-1]))     # a different scale per channel
    eps = rnd(*case.shape, seed=12)
    xd, ed = dev(x, case.off), dev(eps, case.off)
    assert ops.noise_dims(xd) == (B, S, C)
    out, norms = ops.noise_inject(xd, ed, s, return_norms=True)
    assert_close(out, _noise_ref(x.double(), eps.double(), s, B, S, C), f"noise_inject {case.name}")
    assert_close(norms[:B * C].view(B, C), (x.double().reshape(B, S, C) ** 2).sum(1).sqrt(), f"norms {case.name}")


def _noise_bwd_check(ops, case, x, what):
    from dpot_amd.train import _NoiseFn
    B, S, C = case.B, case.S, case.C
    s = 0.3
    eps, g = rnd(*case.shape, seed=22), rnd(*case.shape, seed=23)
    xd, ed, gd = dev(x), dev(eps), dev(g)
    a = dev(x).requires_grad_(True)
    out = _NoiseFn.apply(a, ed, s)
    out.backward(gd)
    _, norms = ops.noise_inject(xd, ed, s, return_norms=True)
    dx = ops.noise_inject_bwd(xd, ed, None, gd, norms, s)
    assert torch.equal(dx, a.grad), what + ": ops.noise_inject_bwd and _NoiseFn.backward disagree"
    return a.grad.cpu(), eps, g, s


@pytest.mark.parametrize("case", SC.NOISE_BWD, ids=lambda c: c.name)
def test_noise_backward_vs_float64_autograd(ops, case):
    B, S, C = case.B, case.S, case.C
    x = rnd(*case.shape, seed=21)
    dx, eps, g, s = _noise_bwd_check(ops, case, x, case.name)
    x64 = x.double().requires_grad_(True)
    _noise_ref(x64, eps.double(), s, B, S, C).backward(g.double())
    assert_close(dx, x64.grad, f"noise backward {case.name}")


def test_noise_backward_zero_sample(ops):
    """norm 0: the reference's autograd divides 0 by 0 there; the kernel's `nrm > 1e-30` guard gives dx == g, no NaN"""
    case = SC.NOISE_BWD_ZERO
    B, S, C = case.B, case.S, case.C
    x = rnd(*case.shape, seed=21)
    x[1] = 0.0
    dx, eps, g, s = _noise_bwd_check(ops, case, x, case.name)
    assert torch.equal(dx[1], g[1])
    x64 = x[:1].double().requires_grad_(True)
    _noise_ref(x64, eps[:1].double(), s, 1, S, C).backward(g[:1].double())
    assert_close(dx[:1], x64.grad, "noise backward, the live sample")


# ---- in-kernel generator: which Philox counter each element gets -------------------------------------------------------------
SEED, OFFSET0 = 0x1234567_89ABCDEF, (1 << 32) + 41          # both words of the key and of the offset are non-zero


@pytest.mark.parametrize("case", SC.NOISE_RNG, ids=lambda c: c.name)
def test_noise_generator_counter_mapping(ops, case):
    B, S, C = case.B, case.S, case.C
    n = S * C
    s = 0.05
    x = rnd(*case.shape, seed=31) * (1.0 + torch.arange(case.shape[-1]))
    g = rnd(*case.shape, seed=32)
    xd, gd = dev(x), dev(g)
    st = ops.rng_state(xd.device)
    before = st.clone()
    st.copy_(torch.tensor([SEED, OFFSET0], dtype=torch.int64))
    norm64 = (x.double().reshape(B, S, C) ** 2).sum(1, keepdim=True).sqrt()
    try:
        _generator_calls(ops, case, x, xd, gd, s, norm64)
    finally:
        st.copy_(before)                                    # the process-wide generator state, as the test found it


def _generator_calls(ops, case, x, xd, gd, s, norm64):
    B, S, C = case.B, case.S, case.C
    n = S * C
    for call in (1, 2):                                     # the second call must match the next offset
        out, norms = ops.noise_inject(xd, None, s, return_norms=True)
        snap = ops.rng_state(xd.device).clone()             # the kernel advances the offset BEFORE it draws
        seed, offset = (int(v) for v in snap.cpu())
        assert (seed, offset) == (SEED, OFFSET0 + call)
        want = torch.from_numpy(philox_ref.field_noise(seed, offset, B, n)).view(B, S, C)
        z = (out.double().cpu().reshape(B, S, C) - x.double().reshape(B, S, C)) / (s * norm64)
        assert_close(z, want, f"generator {case.name}, call {call}: (out - x) / (s * norm)")
        # the backward re-draws from the snapshot: equal to the explicit-eps backward fed with the reference noise
        dx = ops.noise_inject_bwd(xd, None, snap, gd, norms, s)
        dx_eps = ops.noise_inject_bwd(xd, dev(want.float().view(case.shape)), None, gd, norms, s)
        assert_close(dx, dx_eps, f"generator {case.name}, call {call}: backward from the snapshot")


# ---- window slide (exact) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,Tb", [((2, 3, 4, 2, 3), 2), ((2, 3, 4, 5, 3), 1)], ids=["nothing_kept", "Tb1_of_5"])
def test_window_slide_edges(ops, shape, Tb):
    T = shape[-2]
    xx, im = rnd(*shape, seed=41), rnd(*shape[:-2], Tb, shape[-1], seed=42)
    out = ops.window_slide(dev(xx), dev(im))
    assert torch.equal(out.cpu(), torch.cat((xx[..., Tb:, :], im), dim=-2))
    if Tb == T:
        assert torch.equal(out.cpu(), im)
    dout = rnd(*shape, seed=43)
    want_xx = torch.cat((torch.zeros(*shape[:-2], Tb, shape[-1]), dout[..., :T - Tb, :]), dim=-2)
    want_im = dout[..., T - Tb:, :]
    for need_xx, need_im in ((True, False), (False, True), (True, True)):
        dxx, dim = ops.window_slide_bwd(dev(dout), Tb, need_xx, need_im)
        assert (dxx is not None) == need_xx and (dim is not None) == need_im
        if need_xx:
            assert torch.equal(dxx.cpu(), want_xx)
        if need_im:
            assert torch.equal(dim.cpu(), want_im)
