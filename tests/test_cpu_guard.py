"""The checks can fail: self-tests of helpers.assert_close (NaN / inf are rejected, finite behaviour is unchanged) and of the
guarded, poisoned allocator of tests/guard.py, on the CPU (Harness(cpu=True)) and once on a device buffer.  Every fault here
is made by the test itself with ordinary indexing; no kernel is made to misbehave."""
import types

import pytest
import torch

import guard
import helpers
from helpers import assert_close


def _raises(fn, *needles):
    with pytest.raises(AssertionError) as e:
        fn()
    for n in needles:
        assert n in str(e.value), (n, str(e.value))
    return str(e.value)


# ---- assert_close ------------------------------------------------------------------------------------------------------
def test_assert_close_rejects_one_nan_in_a():
    b = torch.randn(4, 5, generator=torch.Generator().manual_seed(0))
    a = b.clone()
    a[2, 3] = float("nan")
    _raises(lambda: assert_close(a, b, "x"), "1 NaN and 0 inf", "index (2, 3)")


def test_assert_close_rejects_all_nan_a():
    b = torch.randn(4, 4, generator=torch.Generator().manual_seed(0))
    a = torch.full((4, 4), float("nan"))
    _raises(lambda: assert_close(a, b, "x"), "16 NaN and 0 inf", "index (0, 0)")


def test_assert_close_rejects_inf_against_finite():
    b = torch.randn(6, generator=torch.Generator().manual_seed(0))
    a = b.clone()
    a[4] = float("inf")
    _raises(lambda: assert_close(a, b, "x"), "0 NaN and 1 inf", "index (4,)")
    a[4] = float("-inf")
    _raises(lambda: assert_close(a, b, "x"), "0 NaN and 1 inf")


def test_assert_close_rejects_nan_in_b_only():
    a = torch.randn(3, 3, generator=torch.Generator().manual_seed(0))
    b = a.clone()
    b[1, 1] = float("nan")
    _raises(lambda: assert_close(a, b, "x"), "reference has 1 NaN", "index (1, 1)")
    _raises(lambda: assert_close(a, b, "x", equal_nan=True), "index (1, 1)")      # one side only: always fails


def test_assert_close_nan_in_both_only_with_equal_nan():
    b = torch.randn(3, 3, generator=torch.Generator().manual_seed(0))
    b[0, 2] = float("nan")
    b[2, 0] = float("inf")
    a = b.clone()
    _raises(lambda: assert_close(a, b, "x"), "1 NaN and 1 inf")
    assert assert_close(a, b, "x", equal_nan=True) == 0.0
    a[2, 0] = float("-inf")                                                        # not the same non-finite value
    _raises(lambda: assert_close(a, b, "x", equal_nan=True), "index (2, 0)")
    a[2, 0] = float("inf")
    a[1, 1] += 1.0                                                                 # the finite rest is still compared
    _raises(lambda: assert_close(a, b, "x", equal_nan=True), "1/9 elements out of tolerance", "index (1, 1)",
            "(1 NaN, 1 inf equal to the reference and not compared)")


def test_assert_close_finite_behaviour_is_pinned():
    b = torch.tensor([[1.0, -2.0], [0.5, 4.0]], dtype=torch.float64)
    a = b + torch.tensor([[1e-4, 0.0], [-2e-4, 3e-4]], dtype=torch.float64)
    # tol = 1e-4 * |b| + 1e-4 * 4: every element inside; the return value is max|d| / max|b| = 3e-4 / 4
    assert assert_close(a, b, "x") == pytest.approx(7.5e-5, rel=1e-9)
    assert helpers.RTOL == 1e-4
    a[1, 0] = 0.5 - 4.6e-4                                                         # tol there: 0.5e-4 + 4e-4 = 4.5e-4
    msg = _raises(lambda: assert_close(a, b, "x"), "1/4 elements out of tolerance", "index (1, 0)")
    assert "0 NaN, 0 inf" in msg
    a[1, 0] = 0.5 - 4.4e-4
    assert assert_close(a, b, "x") == pytest.approx(4.4e-4 / 4, rel=1e-6)
    assert assert_close(a, b, "x", rtol=0.0, atol_scale=2e-4) == pytest.approx(4.4e-4 / 4, rel=1e-6)
    _raises(lambda: assert_close(a, b, "x", rtol=0.0, atol_scale=0.5e-4), "2/4 elements")
    _raises(lambda: assert_close(torch.zeros(2, 3), torch.zeros(3, 2), "x"), "shape")


def test_assert_sub_names_nan():
    t = torch.arange(12.0)
    fx = {"k.stride": 3, "k.sub": t[::3].numpy(), "k.sum": t.sum().item(), "k.abssum": t.abs().sum().item()}
    helpers.assert_sub(t, fx, "k", "x")
    t2 = t.clone()
    t2[7] = float("nan")                                                           # not on the subsample
    _raises(lambda: helpers.assert_sub(t2, fx, "k", "x"), "1 NaN and 0 inf", "index (7,)")


# ---- the harness, on the CPU -------------------------------------------------------------------------------------------
def _fake_ops(proxy):
    """a wrapper module in the style of dpot_amd.ops: allocates its result through the module attribute `torch`"""
    m = types.ModuleType("fake_ops")
    m.torch = proxy

    def copy_rows(x, skip_last=False):
        out = m.torch.empty_like(x)
        n = x.shape[0] - (1 if skip_last else 0)
        out[:n] = x[:n]
        return out
    m.copy_rows = copy_rows
    return m


def test_unwritten_row_is_nan_and_fails_the_comparison():
    h = guard.Harness(cpu=True)
    ops = _fake_ops(h.proxy)
    x = torch.randn(7, 5, generator=torch.Generator().manual_seed(1))
    assert_close(ops.copy_rows(x), x, "whole copy")
    h.check()
    got = ops.copy_rows(x, skip_last=True)
    msg = _raises(lambda: assert_close(got, x, "n-1 of n rows"), "5 NaN and 0 inf", "index (6, 0)")
    assert "out of tolerance" not in msg
    h.check()                                                                      # nothing strayed: the guards are whole


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.int32])
def test_one_stray_byte_is_named_with_side_and_offset(dtype):
    h = guard.Harness(cpu=True)
    t = h.proxy.empty(3, 11, dtype=dtype)
    h.check()                                                                      # untouched: passes (and releases)
    for side, at in (("below", -1), ("above", 0), ("above", 700), ("below", -guard.guard_bytes(3 * 11 * dtype.itemsize))):
        t = h.proxy.empty(3, 11, dtype=dtype, device="cpu")
        rec = h.records[-1]
        raw = rec.raw
        pos = (rec.lo[1] if side == "below" else rec.hi[0]) + at
        assert pos == (t.data_ptr() - raw.data_ptr()) + (at if side == "below" else t.numel() * t.element_size() + at)
        raw[pos] = 0x5A                                                            # ordinary indexing on the raw buffer
        msg = _raises(h.check, f"overwritten {side} the buffer", f"byte offset {at}", "1 guard byte(s)", "(3, 11)",
                      str(dtype).replace("torch.", ""))
        assert "stray writes into 1 of 1" in msg
        h.check()                                                                  # references were released


def test_check_names_the_allocating_function_and_only_the_hit_buffer():
    h = guard.Harness(cpu=True, modules=("fake_ops", __name__))
    ops = _fake_ops(h.proxy)
    x = torch.randn(4, 4)
    ops.copy_rows(x)
    t = h.proxy.zeros(8)
    h.proxy.empty_like(x)
    r = h.records[1]
    r.raw[r.hi[0]:r.hi[0] + 3] = 1
    msg = _raises(h.check, "stray writes into 1 of 3", "3 guard byte(s) overwritten above", "byte offset 0", "(8,)",
                  "test_check_names_the_allocating_function")
    assert "copy_rows" not in msg


def test_bodies_zeros_and_integers():
    h = guard.Harness(cpu=True)
    p = h.proxy
    assert torch.isnan(p.empty(5, 3)).all() and torch.isnan(p.empty((5, 3), dtype=torch.bfloat16).float()).all()
    assert torch.isnan(p.empty_like(torch.ones(2, 2, dtype=torch.float16)).float()).all()
    z = p.zeros(4, 6)
    assert torch.equal(z, torch.zeros(4, 6))
    assert torch.equal(p.zeros_like(torch.ones(3)), torch.zeros(3))
    for r in h.records:                                                            # float buffers: guards are all 0xFF
        assert r.pat == 0xFF and int(r.raw[r.lo[0]:r.lo[1]].min()) == 255 and int(r.raw[r.hi[0]:r.hi[1]].min()) == 255
    n0 = len(h.records)
    for t in (p.empty(9, dtype=torch.int32), p.zeros(9, dtype=torch.int64), p.empty_like(torch.ones(9, dtype=torch.uint8)),
              p.empty(3, dtype=torch.bool)):
        assert not t.any()
    for r in h.records[n0:]:                                                       # integer buffers: zero body, zero guards
        assert r.pat == 0 and int(r.raw.max()) == 0
    h.check()


@pytest.mark.parametrize("shape,dtype", [((1,), torch.float32), ((33, 7), torch.bfloat16), ((2, 3, 5), torch.float32),
                                         ((1025,), torch.int32), ((3,), torch.uint8), ((4096, 4096), torch.float32)])
def test_returned_tensors_are_contiguous_aligned_and_as_requested(shape, dtype):
    h = guard.Harness(cpu=True)
    src = torch.zeros(shape, dtype=dtype)
    made = (h.proxy.empty(*shape, dtype=dtype), h.proxy.empty(shape, dtype=dtype, device="cpu"),
            h.proxy.zeros(shape, dtype=dtype), h.proxy.empty_like(src), h.proxy.zeros_like(src), h.wrap(src),
            h.proxy.empty_like(src, dtype=torch.float32))
    assert len(h.records) == len(made)
    for t, want in zip(made, [dtype] * 6 + [torch.float32]):
        assert t.is_contiguous() and tuple(t.shape) == shape and t.dtype == want and t.data_ptr() % 512 == 0
    assert h.records[0].dtype == dtype and h.records[-1].dtype == torch.float32
    nbytes = src.numel() * src.element_size()
    g = guard.guard_bytes(nbytes)
    assert g % 512 == 0 and g == min(max(nbytes, 64 << 10), 8 << 20) + (-min(max(nbytes, 64 << 10), 8 << 20)) % 512
    r = h.records[0]
    assert r.lo[1] - r.lo[0] == g and r.hi[1] - r.hi[0] == g and r.hi[0] - r.lo[1] == nbytes
    h.check()


def test_wrap_and_full_nan():
    h = guard.Harness(cpu=True)
    x = torch.randn(5, 9, generator=torch.Generator().manual_seed(2))[:, :7]       # a non-contiguous test input
    w = h.wrap(x)
    assert torch.equal(w, x) and w.is_contiguous() and w.data_ptr() != x.data_ptr()
    o = h.full_nan((3, 4), device="cpu")
    assert o.shape == (3, 4) and torch.isnan(o).all() and o.data_ptr() % 512 == 0
    r = h.records[0]
    r.raw[r.lo[1] - 2] = 0                                                         # a store 2 bytes before the input
    _raises(h.check, "guard.wrap", "below", "byte offset -2")


def test_everything_else_reaches_the_real_torch():
    h = guard.Harness(cpu=True)
    p = h.proxy
    assert p.float32 is torch.float32 and p.cuda is torch.cuda and p.Tensor is torch.Tensor and p.nn is torch.nn
    assert p.full is torch.full and p.ones is torch.ones and p.autograd.Function is torch.autograd.Function
    assert torch.equal(p.arange(4), torch.arange(4))
    with pytest.raises(AttributeError):
        p.no_such_attribute
    assert not h.records


def test_cpu_and_odd_forms_pass_through_by_default():
    h = guard.Harness()                                                            # cpu=False: CPU tensors are torch's own
    t = h.proxy.empty(4, 4)
    assert not h.records and t.shape == (4, 4) and h.passed_through == 1
    h = guard.Harness(cpu=True)
    assert h.proxy.empty(0, 5).shape == (0, 5) and not h.records                   # zero elements: nothing to guard
    nc = torch.zeros(6, 4).t()
    assert h.proxy.empty_like(nc).stride() == torch.empty_like(nc).stride() and not h.records
    assert h.passed_through == 2


def test_early_check_above_the_hold_limit(monkeypatch):
    monkeypatch.setattr(guard, "HOLD_LIMIT", 1 << 20)
    h = guard.Harness(cpu=True)
    for _ in range(20):
        h.proxy.empty(1000)                                                        # ~ 135 KiB each with the guards, dropped
    assert 0 < len(h.records) < 20 and h.held <= 1 << 20                           # released: nothing else used them
    r = h.records[-1]
    r.raw[r.hi[0]] = 0
    with pytest.raises(guard.GuardError):
        for _ in range(20):
            h.proxy.empty(1000)                                                    # the early check reports the stray byte


def test_early_check_keeps_the_buffers_still_in_use(monkeypatch):
    monkeypatch.setattr(guard, "HOLD_LIMIT", 1 << 20)
    h = guard.Harness(cpu=True)
    live = h.proxy.empty(10, 100)
    view = h.proxy.empty(1000).view(10, 100)[2:4]                                  # only a view of a view survives
    rec_live, rec_view = h.records[0], h.records[1]
    for _ in range(30):
        h.proxy.empty(1000)
    assert h.records[0] is rec_live and h.records[1] is rec_view                   # early checks ran, both stayed on record
    assert len(h.records) < 12
    rec_view.raw[rec_view.hi[0] + 5] = 1                                           # a stray write after the early checks
    _raises(h.check, "stray writes into 1 of", "above", "byte offset 5")
    assert torch.isnan(live).all() and torch.isnan(view).all() and not h.records


def test_fixture_installs_and_removes_the_proxy(guarded):
    from guard import guarded as _fixture                                          # the fixture is importable by test modules
    import dpot_amd.ops as ops
    import dpot_amd.functional as F
    assert ops.torch is guarded.proxy and F.torch is guarded.proxy and guard._active is guarded
    assert guard.full_nan((2, 2), device="cpu").shape == (2, 2)                    # CPU: passes through, no record
    assert not guarded.records


from guard import guarded  # noqa: E402,F401  (fixture used by the test above and the GPU self-test)


def test_proxy_is_gone_after_the_fixture():
    import dpot_amd.ops as ops
    assert ops.torch is torch and guard._active is None


@pytest.mark.gpu
def test_one_stray_byte_on_a_device_buffer(guarded):
    """the same one-byte check on the GPU; the byte is written by indexing from the test"""
    import dpot_amd.ops as ops
    t = ops.torch.empty(100, 35, device="cuda")
    assert t.is_cuda and torch.isnan(t).all() and t.is_contiguous() and t.data_ptr() % 512 == 0
    i32 = ops.torch.empty(17, dtype=torch.int32, device="cuda")
    assert not i32.any()
    guarded.check()                                                                # untouched: passes
    t = ops.torch.empty(100, 35, device="cuda")
    r = guarded.records[-1]
    r.raw[r.hi[0]] = 0
    msg = _raises(guarded.check, "above", "byte offset 0", "1 guard byte(s)", "(100, 35)")
    assert "test_one_stray_byte_on_a_device_buffer" in msg
    w = guard.wrap(torch.ones(3, 3), "cuda")
    r = guarded.records[-1]
    r.raw[r.lo[1] - 1] = 0
    _raises(guarded.check, "below", "byte offset -1")
    g = torch.cuda.CUDAGraph()                                                     # capturing: allocations pass through
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            c = ops.torch.empty(64, device="cuda")
            c.fill_(1.0)
    assert not guarded.records
