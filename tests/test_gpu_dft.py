"""Every 2-D DFT kernel the library can select (tests/dft_cases.py reaches each, tests/test_cpu_dft.py proves it) against
float64 torch.fft on the host (tests/dft_ref.py).  Two assertions per result:

  1. the project's element-wise tolerance, helpers.assert_close with its defaults;
  2. a norm-wise bound taken from the reference: e = ||got - ref64|| / ||ref64|| <= 4 * e32, where e32 is the same quantity
     for torch.fft run in float32 on the host on the same input.  e32 is 0.6e-7 .. 1.3e-7 on these grids; an fp32 emulation of
     the least accurate algorithm in use (sequential direct sums with float twiddle tables) stays within 2.2 x e32 at 128 x 128
     and 1.4 x at 32 x 32 and below, and the register FFTs round less often.  4 leaves room for FMA contraction and the
     128-point split stage and still fails on an error of 1e-6 - a twiddle wrong in the fifth digit, a column weight off on one
     column - which the element-wise tolerance (1e-4 of the tensor's maximum) lets through.  Measured on an MI355X the largest
     e / e32 of any case is 1.63 (the generic kernel at 32 x 32); DESIGN.md has the table per kind.

Before it launches, every case asserts that the library selects the kernel the table names.
"""
import pytest
import torch

import dft_cases as DC
import dft_ref as DR
import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close

pytestmark = pytest.mark.gpu

FACTOR = 4.0


@pytest.fixture(scope="module")
def ops():
    from dpot_amd import ops as _ops
    from dpot_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _ops


def dev(t):
    return guard.wrap(t, "cuda")


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).float()


def hold(got, ref64, ref32, what):
    """both assertions; prints the figures first so that a run with -s shows every e / e32"""
    e, e32 = DR.rel_err(got, ref64), DR.rel_err(ref32, ref64)
    print(f"{what}: e {e:.3e} e32 {e32:.3e} e/e32 {e / e32 if e32 else float(e > 0):.2f}")
    if ref64.is_complex():
        got = got.detach().cpu()
        assert_close(got.real, ref64.real, what + " (re)")
        assert_close(got.imag, ref64.imag, what + " (im)")
    else:
        assert_close(got, ref64, what)
    assert e <= FACTOR * e32, f"{what}: norm-wise error {e:.3e} above {FACTOR:g} x {e32:.3e}, the float32 host FFT's"


@pytest.mark.parametrize("c", DC.RUNNABLE, ids=DC.case_id)
def test_rfft2_vs_float64(ops, guarded, c):
    assert ops.dft2_kernel_kind(c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, False) == c.kind_fwd
    x = rnd(c.B, c.h, c.w, c.E, seed=1)
    xd = dev(x).view(c.B, c.h * c.w, c.E)
    s64, s32 = DR.rfft2_ref(x, c.mx, c.my), DR.rfft2_ref(x, c.mx, c.my, torch.float32)
    for cw in (0, 1):
        spec = ops.rfft2(xd, c.h, c.w, c.nb, c.mx, c.my, cw)
        assert spec.shape == (c.B * c.mx * c.my, 2 * c.E)
        hold(DR.from_planar(spec, c.B, c.mx, c.my, c.nb), DR.weighted(s64, c.w) if cw else s64,
             DR.weighted(s32, c.w) if cw else s32, f"rfft2 kind {c.kind_fwd} col_weights {cw}")


@pytest.mark.parametrize("c", DC.RUNNABLE, ids=DC.case_id)
def test_irfft2_vs_float64(ops, guarded, c):
    assert ops.dft2_kernel_kind(c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, True) == c.kind_inv
    # an arbitrary spectrum: no Hermitian symmetry, imaginary parts in the DC and Nyquist columns
    spec = torch.complex(rnd(c.B, c.mx, c.my, c.E, seed=2), rnd(c.B, c.mx, c.my, c.E, seed=3))
    res = rnd(c.B, c.h, c.w, c.E, seed=4)
    sd, rd = dev(DR.to_planar(spec, c.nb)), dev(res).view(c.B, c.h * c.w, c.E)
    for cw in (1, 0):
        y64, y32 = DR.irfft2_ref(spec, c.h, c.w, cw), DR.irfft2_ref(spec, c.h, c.w, cw, torch.float32)
        y = ops.irfft2(sd, c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, cw)
        hold(y.view(c.B, c.h, c.w, c.E), y64, y32, f"irfft2 kind {c.kind_inv} col_weights {cw}")
        y = ops.irfft2(sd, c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, cw, res=rd)
        hold(y.view(c.B, c.h, c.w, c.E), y64 + res.double(), y32 + res, f"irfft2 kind {c.kind_inv} col_weights {cw} + res")


@pytest.mark.parametrize("c,G", DC.NORM_CASES, ids=lambda v: DC.case_id(v) if isinstance(v, tuple) else f"G{v}")
def test_groupnorm_on_the_load_is_bit_identical(ops, guarded, c, G):
    """rfft2(norm=...) and irfft2(res_norm=...) against the plain kernels fed groupnorm_fwd's output: the same bits"""
    assert ops.dft2_kernel_kind(c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, False, True) == c.kind_fwd > 0
    assert ops.dft2_kernel_kind(c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, True, True) == c.kind_inv > 0
    tok = c.h * c.w
    # per-sample, per-channel offsets and scales: every (sample, group) has statistics of its own, far from (0, 1)
    x = rnd(c.B, tok, c.E, seed=1) * (0.5 + rnd(c.B, 1, c.E, seed=5).abs()) + 2.0 * rnd(c.B, 1, c.E, seed=6)
    x, g, b = dev(x), dev(1 + 0.3 * rnd(c.E, seed=2)), dev(0.2 * rnd(c.E, seed=3))
    xn, mean, rstd = ops.groupnorm_fwd(x, g, b, G)
    assert_close(mean, x.double().view(c.B, tok, G, c.E // G).mean(dim=(1, 3)), "GroupNorm mean")
    for cw in (0, 1):
        S_ref = ops.rfft2(xn, c.h, c.w, c.nb, c.mx, c.my, cw)
        S = ops.rfft2(x, c.h, c.w, c.nb, c.mx, c.my, cw, norm=(mean, rstd, g, b))
        assert not torch.isnan(S).any() and torch.equal(S, S_ref)
        y_ref = ops.irfft2(S_ref, c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, cw, res=xn)
        y = ops.irfft2(S_ref, c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, cw, res=x, res_norm=(mean, rstd, g, b))
        assert not torch.isnan(y).any() and torch.equal(y, y_ref)


def _refusal_operands(c, G):
    """full-size operands (nothing would be read or written out of bounds even by a launch) and NaN-filled outputs"""
    tok = c.h * c.w
    x = dev(rnd(c.B, tok, c.E, seed=1))
    spec_in = dev(rnd(c.B * c.mx * c.my, 2 * c.E, seed=2))
    stats = [dev(rnd(c.B, G, seed=3)), dev(rnd(c.B, G, seed=4).abs() + 0.5), dev(rnd(c.E, seed=5)), dev(rnd(c.E, seed=6))]
    return x, spec_in, stats, guard.full_nan((c.B * c.mx * c.my, 2 * c.E)), guard.full_nan((c.B, tok, c.E))


@pytest.mark.parametrize("c", DC.REFUSED, ids=DC.case_id)
def test_grid_too_large_for_lds_raises_and_launches_nothing(ops, guarded, c):
    from dpot_amd import _lib
    assert ops.dft2_kernel_kind(c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, False) == -1
    assert ops.dft2_kernel_kind(c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, True) == -1
    x, spec_in, _, spec_out, y_out = _refusal_operands(c, 1)
    with pytest.raises((ValueError, _lib.DpotHipError)):
        ops.rfft2(x, c.h, c.w, c.nb, c.mx, c.my, 0)
    with pytest.raises((ValueError, _lib.DpotHipError)):
        ops.irfft2(spec_in, c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, 1, res=x)
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream      # the C entry points: DPOT_EUNSUP before any launch
    dims = (c.B, c.h, c.w, c.E, c.nb, c.mx, c.my)
    assert lib.dpot_rfft2(x.data_ptr(), spec_out.data_ptr(), *dims, 0, s) == -2
    assert lib.dpot_irfft2(spec_in.data_ptr(), x.data_ptr(), y_out.data_ptr(), *dims, 1, s) == -2
    torch.cuda.synchronize()
    assert torch.isnan(spec_out).all() and torch.isnan(y_out).all()


@pytest.mark.parametrize("c,G", DC.NORM_REFUSED, ids=lambda v: DC.case_id(v) if isinstance(v, tuple) else f"G{v}")
def test_norm_without_a_register_path_raises_and_launches_nothing(ops, guarded, c, G):
    from dpot_amd import _lib
    assert ops.dft2_kernel_kind(c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, False, True) == -1
    assert ops.dft2_kernel_kind(c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, True, True) == -1
    x, spec_in, stats, spec_out, y_out = _refusal_operands(c, G)
    with pytest.raises((ValueError, _lib.DpotHipError)):
        ops.rfft2(x, c.h, c.w, c.nb, c.mx, c.my, 0, norm=tuple(stats))
    with pytest.raises((ValueError, _lib.DpotHipError)):
        ops.irfft2(spec_in, c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, 1, res=x, res_norm=tuple(stats))
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    dims = (c.B, c.h, c.w, c.E, c.nb, c.mx, c.my)
    sp = [t.data_ptr() for t in stats]
    rc_f = lib.dpot_rfft2_norm(x.data_ptr(), *sp, G, spec_out.data_ptr(), *dims, 0, s)
    rc_i = lib.dpot_irfft2_norm(spec_in.data_ptr(), x.data_ptr(), *sp, G, y_out.data_ptr(), *dims, 1, s)
    assert rc_f < 0 and rc_i < 0
    torch.cuda.synchronize()
    assert torch.isnan(spec_out).all() and torch.isnan(y_out).all()
