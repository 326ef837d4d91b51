"""GPU parity tests of the small reductions and data-movement kernels of csrc/misc.hip at ragged shapes: every colsum
instantiation, the token-mean unroll bound, more than one 64-column block, second trips of the 256-wide loops, P = 1 and
single-channel pixel shuffles, and patchify with X != Y.  Shapes: tests/streaming_cases.py.  References: float64 torch and
oracle/dpot_ref.py; pure data movement is compared exactly.  Tolerance: helpers.assert_close at its default, except the
TimeAggregator gradients (2e-4: cos of an fp32-rounded argument near 1e3 rad, as test_gpu_ops.test_timeagg_scale)."""
import pytest
import torch

import guard
from guard import guarded  # noqa: F401  (fixture)
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


def dev(t):
    return guard.wrap(t, "cuda")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


# ---- column sums -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3], ids=["ld_eq_N", "ld_gt_N"])
@pytest.mark.parametrize("case", SC.COLSUM, ids=lambda c: f"{c.M}x{c.N}")
def test_colsum_every_instantiation(ops, case, pad):
    M, N = case.M, case.N
    ld = N + pad
    X = rnd(M, ld, seed=1) + 0.25                       # a non-zero mean: a dropped row shows in every column
    out = guard.full_nan((N,))
    got = ops.colsum(dev(X), M, N, ld=ld, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert_close(out, X[:, :N].double().sum(0), f"colsum {M}x{N} ld={ld} (colsum_kernel<{case.width}>, {case.parts} part(s))")


def test_colsum_scatter_with_a_gap(ops):
    M, N, _, segs = SC.COLSUM_SCATTER
    X = rnd(M, N, seed=2) + 0.25
    dsts = [guard.full_nan((n,)) for _, n in segs]
    ops.colsum_scatter(dev(X), M, N, [(s, d) for (s, _), d in zip(segs, dsts)])
    ref = X.double().sum(0)
    for (s, n), d in zip(segs, dsts):
        assert_close(d, ref[s:s + n], f"colsum_scatter columns [{s}, {s + n})")


# ---- group_rowsum, token_mean, scale/shift, bias_add -------------------------------------------------------------------------
@pytest.mark.parametrize("B,Rr,T,N", SC.GROUP_ROWSUM)
def test_group_rowsum_ragged(ops, B, Rr, T, N):
    X = rnd(B * Rr * T, N, seed=3) + 0.25
    assert_close(ops.group_rowsum(dev(X), B, Rr, T, N), X.double().view(B, Rr, T, N).sum((0, 2)), f"group_rowsum {B, Rr, T, N}")


@pytest.mark.parametrize("E", SC.TOKEN_MEAN_E)
@pytest.mark.parametrize("T", SC.TOKEN_MEAN_T)
def test_token_mean_unroll_bound(ops, T, E):
    B = SC.TOKEN_MEAN_B
    x = rnd(B, T, E, seed=4) + 0.5
    assert_close(ops.token_mean(dev(x)), x.double().mean(1), f"token_mean T={T} E={E}")
    dy, add = rnd(B, E, seed=5), rnd(B, T, E, seed=6)
    want = (dy.double() / T)[:, None, :].expand(B, T, E)
    assert_close(ops.token_mean_bwd(dev(dy), T), want, f"token_mean_bwd T={T} E={E}")
    assert_close(ops.token_mean_bwd(dev(dy), T, add=dev(add)), want + add.double(), f"token_mean_bwd + add T={T} E={E}")


@pytest.mark.parametrize("B,T,E", SC.SCALE_SHIFT)
def test_scale_shift_ragged(ops, B, T, E):
    x, dy = rnd(B, T, E, seed=7), rnd(B, T, E, seed=8)
    sc, sh = rnd(B, E, seed=9), rnd(B, E, seed=10)
    assert_close(ops.scale_shift(dev(x), dev(sc), dev(sh)), x.double() * sc.double()[:, None] + sh.double()[:, None],
                 f"scale_shift {B, T, E}")
    dx, dsc, dsh = ops.scale_shift_bwd(dev(dy), dev(x), dev(sc))
    assert_close(dx, dy.double() * sc.double()[:, None], "scale_shift_bwd dx")
    assert_close(dsc, (dy.double() * x.double()).sum(1), "scale_shift_bwd dscale")
    assert_close(dsh, dy.double().sum(1), "scale_shift_bwd dshift")


def test_bias_add_and_tile(ops):
    Rr, N = 7, 65
    x, v = rnd(Rr, N, seed=11), rnd(N, seed=12)
    assert torch.equal(ops.bias_add(dev(x), dev(v)).cpu(), x + v)
    assert torch.equal(ops.tile_vec(dev(v), Rr).cpu(), v.repeat(Rr))          # bias_add with x = None


# ---- TimeAggregator scaling --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,E", SC.TIMEAGG)
def test_timeagg_scale_wide(ops, T, E):
    w = rnd(T, E, E, seed=1)
    gamma = (2 ** torch.linspace(-10, 10, E)).unsqueeze(0) * (0.9 + 0.2 * torch.rand(1, E, generator=torch.Generator().manual_seed(2)))
    tt = torch.linspace(0, 1, T) if T > 1 else torch.tensor([0.7])            # linspace(0, 1, 1) = [0]: cos 1, sin 0
    ws = ops.timeagg_scale_w(dev(w), dev(gamma), dev(tt))
    temb = torch.cos(tt.unsqueeze(-1) @ gamma)                                   # fp32 arguments, as the reference
    assert_close(ws, w.double() * temb.double()[:, :, None], "timeagg scale")
    dws = rnd(T, E, E, seed=3)
    wd, gd = w.double().requires_grad_(True), gamma.double().requires_grad_(True)
    ((wd * torch.cos(tt.double().unsqueeze(-1) @ gd)[:, :, None]) * dws.double()).sum().backward()
    out_dw, out_dg = guard.full_nan((T, E, E)), guard.full_nan((1, E))
    ops.timeagg_scale_w_bwd(dev(dws), dev(w), dev(gamma), dev(tt), out_dw=out_dw, out_dgamma=out_dg)
    assert_close(out_dw, wd.grad, "timeagg dw", rtol=2e-4, atol_scale=2e-4)   # cos of fp32-rounded t*gamma (~1e3 rad)
    assert_close(out_dg, gd.grad, "timeagg dgamma", rtol=2e-4, atol_scale=2e-4)


# ---- data movement (exact) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbatch,Rr,Cn", SC.TRANSPOSE)
def test_transpose2d_tile_edges(ops, nbatch, Rr, Cn):
    t = rnd(nbatch, Rr, Cn, seed=13)
    out = guard.full_nan((nbatch, Cn, Rr))
    ops.transpose2d(dev(t), nbatch, Rr, Cn, out=out)
    assert torch.equal(out.cpu(), t.transpose(1, 2).contiguous())


@pytest.mark.parametrize("B,h,w,P,Cc", [(2, 3, 5, 1, 3), (2, 3, 5, 4, 1)], ids=["P1", "Cc1_h_ne_w"])
def test_pixel_shuffle_edges(ops, B, h, w, P, Cc):
    z = rnd(B * h * w * P * P, Cc, seed=14)
    out = ops.pixel_shuffle(dev(z), B, h, w, P, Cc)
    ref = z.view(B, h, w, P, P, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B, h * P, w * P, Cc)
    assert torch.equal(out.cpu(), ref)
    back = ops.pixel_shuffle(dev(ref.contiguous()), B, h, w, P, Cc, inverse=True)
    assert torch.equal(back.cpu(), z)


def test_copy2d_pad_rows_while_cropping_columns(ops):
    src = rnd(5, 9, seed=15)
    out = guard.full_nan((7, 6))
    ops.copy2d_pad(dev(src), 5, 9, 7, 6, out=out)
    assert torch.equal(out.cpu(), torch.cat([src[:, :6], torch.zeros(2, 6)]))


@pytest.mark.parametrize("B,X,Y,T,Cc,P", SC.PATCHIFY)
def test_patchify_unpatchify_rectangular(ops, B, X, Y, T, Cc, P):
    K0 = (Cc + 3) * P * P
    x = rnd(B, X, Y, T, Cc, seed=16)
    # the reference's grid: unit_grid(X) along x, unit_grid(Y) along y - two different vectors here (X != Y)
    gx, gy, gt = R.unit_grid(X), R.unit_grid(Y), R.unit_grid(T)
    assert X != Y and not torch.equal(gx[:min(X, Y)], gy[:min(X, Y)])
    A = ops.patchify(dev(x), dev(gx), dev(gy), dev(gt), P)
    assert torch.equal(A.cpu(), R.patchify(R.append_grid(x), P).reshape(-1, K0))
    # and with arbitrary grid vectors, the expected coordinate columns written by hand (append_grid builds its own grids)
    gx, gy, gt = rnd(X, seed=17), rnd(Y, seed=18), rnd(T, seed=19)
    xa = torch.cat([x, gx.view(1, X, 1, 1, 1).expand(B, X, Y, T, 1), gy.view(1, 1, Y, 1, 1).expand(B, X, Y, T, 1),
                    gt.view(1, 1, 1, T, 1).expand(B, X, Y, T, 1)], dim=-1)
    A = ops.patchify(dev(x), dev(gx), dev(gy), dev(gt), P)
    assert torch.equal(A.cpu(), R.patchify(xa, P).reshape(-1, K0))
    dA = rnd(*A.shape, seed=20)
    dx = ops.unpatchify(dev(dA), B, X, Y, T, Cc, P)
    xr = x.clone().requires_grad_(True)
    (R.patchify(R.append_grid(xr), P).reshape(-1, K0) * dA).sum().backward()
    assert torch.equal(dx.cpu(), xr.grad)
