"""CPU half of the activation sweep: the float32 restatement of the device GELU (tests/act_ref.py) against float64 and
against the bounds documented in csrc/common.h, the sample vector the GPU sweep uses, and the float64 references against the
oracle's activation table."""
import re

import numpy as np
import pytest
import torch

import act_ref as AR
from oracle import dpot_ref as R


@pytest.fixture(scope="module")
def grid2m():
    x = np.linspace(-12.0, 12.0, 2_000_001).astype(np.float32)
    return (x,) + AR.reference("gelu", x)


def test_gelu_restatement_meets_the_documented_bounds_on_the_2m_grid(grid2m):
    x, v64, d64 = grid2m
    e_val = np.abs(AR.gelu_fwd(x).astype(np.float64) - v64)
    e_der = np.abs(AR.gelu_bwd(x).astype(np.float64) - d64)
    val2, der2 = AR.gelu_val_der(x)
    e_der2 = np.abs(der2.astype(np.float64) - d64)
    print(f"gelu {e_val.max():.3e} at {x[e_val.argmax()]:.4f}; gelu' {e_der.max():.3e} at {x[e_der.argmax()]:.4f}; "
          f"gelu_val_der' {e_der2.max():.3e} at {x[e_der2.argmax()]:.4f}")
    assert e_val.max() <= AR.DOC_GELU_ERR * 1.02
    assert e_der.max() <= AR.DOC_GELU_DER_ERR
    assert e_der2.max() <= AR.DOC_GELU_DER_ERR
    assert np.array_equal(val2, AR.gelu_fwd(x))                 # the value of gelu_val_der is gelu_fwd's expression


def test_gelu_val_der_equals_gelu_bwd_to_one_ulp_of_exp2(grid2m):
    """gelu_val_der forms phi(x) = exp2(-x^2 log2(e)/2 - log2 sqrt(2 pi)) in one exp2, gelu_bwd forms
    x / sqrt(2 pi) * exp2(-x^2 log2(e)/2): the two derivatives differ by at most |x| phi(x) times the relative error of the
    two float32 exp2 arguments and results.  The argument t (|t| <= 105 on [-12, 12]) carries up to 1.5 ulp32(t) of rounding
    (x*x, the product / fma), i.e. a relative 1.5 ulp32(t) ln 2 on 2^t, plus half an ulp for each rounded exp2, plus the
    products' own half ulps; and one final rounding of each derivative (<= ulp32(1) = 2^-23 together)."""
    x, _, d64 = grid2m
    d1, d2 = AR.gelu_bwd(x).astype(np.float64), AR.gelu_val_der(x)[1].astype(np.float64)
    xd = x.astype(np.float64)
    phi = np.exp(-0.5 * xd * xd) / np.sqrt(2 * np.pi)
    t = 0.5 * xd * xd / np.log(2.0) + 1.3257480647361597
    rel = 2 * (1.5 * AR.ulp32(t) * np.log(2.0)) + 4 * 2.0 ** -24
    bound = np.abs(xd) * phi * rel + 2.0 ** -23
    worst = (np.abs(d1 - d2) / bound).max()
    print(f"max |gelu_bwd - gelu_val_der'| = {np.abs(d1 - d2).max():.3e}, worst ratio to its bound {worst:.3f}")
    assert worst <= 1.0


def test_restatement_uses_the_coefficients_of_common_h():
    """the restatement is only worth something while it restates the device code: the nine coefficients of normal_tail, the
    clamp and the three constants are read from csrc/common.h and must be the same float32 numbers (a change of one float32
    ulp in the header fails here; the 10th printed digit of a coefficient is below float32 resolution and is the same number).
    The comparison is on the header's text (how a coefficient is printed, whole expressions for the clamp and the softplus
    threshold): re-formatting common.h fails this test without any numerical change, and the test is then to be updated with
    it.  The compiled constants themselves are held by the GPU sweep."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dpot_amd", "csrc", "common.h")).read()
    body = src[src.index("float normal_tail(float ax)"):src.index("gelu_clamp_abs(float x)")]
    nums = [float(t) for t in re.findall(r"(-?\d\.\d+e[+-]\d+)f", body)]
    assert len(nums) == 9 and [np.float32(v) for v in nums] == [np.float32(v) for v in AR.TAIL_COEF]
    assert "__builtin_fabsf(x), 6.5f)" in src
    for const in ("0.72134752044448170368f", "0.39894228040143267794f", "1.32574806473615975284f"):
        assert const in src
    assert "case DPOT_ACT_SOFTPLUS: return x > 20.f ? x" in src and "case DPOT_ACT_SOFTPLUS: return x > 20.f ? 1.f" in src


@pytest.mark.parametrize("k", [6, 7, 8])
def test_a_perturbed_tail_coefficient_breaks_the_documented_bound(grid2m, k):
    """what the documented bounds can see: they are dominated by the float32 rounding of the result (half an ulp at 4.5 is
    2.4e-7), so a relative change of 1e-5 in one of the three low-order coefficients breaks them; smaller changes, and changes of
    that size in coefficients 0 to 5 (whose terms are small where the error peaks), are seen only by the equality test above"""
    x, v64, d64 = grid2m
    coef = list(AR.TAIL_COEF)
    coef[k] *= 1.0 + 1e-5
    e = np.abs(AR.gelu_fwd(x, coef).astype(np.float64) - v64).max()
    ed = np.abs(AR.gelu_bwd(x, coef).astype(np.float64) - d64).max()
    assert e > AR.DOC_GELU_ERR * 1.02 and ed > AR.DOC_GELU_DER_ERR


def test_sample_vector_is_deterministic_and_covers_what_the_sweep_claims():
    v = AR.sample_points()
    assert v.dtype == np.float32 and v.shape == (AR.N_POINTS,)
    assert np.array_equal(v.view(np.int32), AR.sample_points().view(np.int32))
    fin = np.isfinite(v)
    nf = AR.nonfinite_positions()
    assert sorted(np.flatnonzero(~fin)) == sorted(nf) and all(p % 16 in (0, 5, 10, 15) for p in nf)
    assert np.isnan(v).sum() >= 4 and np.isposinf(v).sum() >= 4 and np.isneginf(v).sum() >= 4
    for p in nf:                                                  # every float4 with a non-finite lane has finite ones too
        q = p // 4 * 4
        assert fin[q:q + 4].sum() == 3
    have = set(v[fin].view(np.int32).tolist())
    need = []
    for c in AR.CRITICAL:
        c = np.float32(c)
        need += [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    need += [0.0, -0.0, AR.DENORM_MIN, AR.FLT_MIN, -AR.FLT_MIN, AR.FLT_MAX, -AR.FLT_MAX]
    assert all(int(np.float32(c).view(np.int32)) in have for c in need)
    g = np.linspace(-12.0, 12.0, 4096).astype(np.float32)
    assert np.array_equal(v[fin][:4096], g)
    a = np.abs(v[fin])
    assert a[a > 0].min() == np.float32(AR.DENORM_MIN) and (a >= 1e29).sum() >= 2 and ((a > 0) & (a <= 1.01e-30)).sum() >= 2
    # what a site may leave out: non-finite derivative cases (fp32 sites, < 1 %), the bf16-plane restriction (< 5 %)
    assert (~fin).sum() / v.size < 0.01
    assert (~AR.bf16_exact(v)).sum() / v.size < 0.05


@pytest.mark.parametrize("name", sorted(AR.LIP))
def test_slope_and_curvature_constants_of_the_tail_bound(name):
    """AR.LIP = (sup |act'|, sup |act''|), which the out-layer tail's error bound carries errors through: not below what
    float64 autograd gives on the sample points and on a 200 001-point grid over [-12, 12], and not more than 2 % above"""
    pts = AR.sample_points()
    x = np.concatenate([pts[np.isfinite(pts)].astype(np.float64), np.linspace(-12.0, 12.0, 200_001)])
    t = torch.from_numpy(x).requires_grad_(True)
    d1, = torch.autograd.grad(AR._TABLE[name](t).sum(), t, create_graph=True)
    d2, = torch.autograd.grad(d1.sum(), t)
    s1, s2 = d1.abs().max().item(), d2.abs().max().item()
    l1, l2 = AR.LIP[name]
    print(f"{name}: sup |act'| {s1:.5f} <= {l1}, sup |act''| {s2:.5f} <= {l2}")
    assert s1 <= l1 <= 1.02 * s1 and s2 <= l2 <= 1.02 * s2


def test_float64_references_agree_with_the_oracle_table():
    v = AR.sample_points()
    x = torch.from_numpy(v).double()
    for name in AR.NAMES:
        want = R._act(name)(x).numpy()
        got, _ = AR.reference(name, v)
        assert np.array_equal(got, want, equal_nan=True), name
    assert set(AR.NAMES) == {"gelu", "tanh", "sigmoid", "relu", "leaky_relu", "softplus", "ELU", "silu"}


def test_bounds_come_from_the_references_own_error():
    v = AR.sample_points()
    b = AR.Bounds(v)
    print("restatement on the sample points: gelu %.3e, gelu' %.3e" % b.restate_err)
    for row in b.table:
        print("%-10s %-10s torch float32 error %.2f ulp, margin %d, c = %.2f" % row)
    assert b.restate_err[0] <= AR.DOC_GELU_ERR * 1.02 and b.restate_err[1] <= AR.DOC_GELU_DER_ERR
    # the reference's own float32 error, pinned: tanh, sigmoid, ELU and the derivative of softplus are within `a` everywhere
    # (c = the floor), softplus about half an ulp, silu about one, silu' (cancellation in 1 + x (1 - s)) about seven
    err = {(n, k): e for n, k, e, _, _ in b.table}
    for key, e in err.items():
        lo, hi = {("softplus", "value"): (0.2, 0.8), ("silu", "value"): (0.8, 1.5),
                  ("silu", "derivative"): (5.0, 8.0)}.get(key, (0.0, 0.0))
        assert lo <= e <= hi and b.c[key] == max(4.0, 4.0 * e), (key, e)
    # the rule accepts the reference implementation's own float32 results and the restatement, and rejects a ReLU that
    # swallows NaN and a softplus threshold of 2
    for name in AR.NAMES:
        val, der = AR.torch_f32(name, v)
        if name == "gelu":
            val, der = AR.gelu_fwd(v), AR.gelu_bwd(v)
        n, _ = AR.check(name, "value", v, val, b, name)
        nd, _ = AR.check(name, "derivative", v, der, b, name + "'")
        assert n == v.size and nd >= 0.99 * v.size
    with pytest.raises(AssertionError):
        AR.check("relu", "value", v, np.where(v > 0, v, np.float32(0)), b, "relu that swallows NaN")
    with pytest.raises(AssertionError):
        t = torch.from_numpy(v)
        AR.check("softplus", "value", v, torch.nn.functional.softplus(t, threshold=2.0).numpy(), b, "softplus threshold 2")
