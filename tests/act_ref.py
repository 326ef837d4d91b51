"""float64 reference of the eight fused activations (models/dpot.py:19) and their derivatives, the sample points the
activation tests sweep, the point-wise error rule, and a numpy float32 restatement of the device GELU of csrc/common.h
(normal_tail / gelu_fwd / gelu_parts / gelu_bwd / gelu_val_der): same coefficients, every fmaf formed in float64 and rounded
once to float32, every plain product / difference rounded to float32, exp2 exact (float64 exp2, rounded).

The rule (tests/test_gpu_activations.py, tests/test_cpu_activations.py):  |got - ref| <= c * ulp32(ref) + a  element-wise
  gelu           c = 1, a = max error of the restatement against float64 on the test's own points + 2^-24 (one-ulp hardware
                 exp2 at |x| Phi(-|x|) <= 0.17, and the final rounding)
  libm functions c = 4 * (error of torch-CPU float32 in ulp32(ref) on the same points, counted only where it exceeds `a`:
                 an absolute error below `a` is already admitted by `a`, and in ulps of a denormal reference it would be
                 astronomically large and make c meaningless), floor c = 4;  a = 2^-23, and 0 on the unbounded branch
                 x > 20 of a forward function
  relu, leaky    bit-exact against torch-CPU float32
"""
import numpy as np
import torch

NAMES = ("gelu", "tanh", "sigmoid", "relu", "leaky_relu", "softplus", "ELU", "silu")
EXACT = ("relu", "leaky_relu")
LIBM = ("tanh", "sigmoid", "softplus", "ELU", "silu")
UNBOUNDED = ("softplus", "ELU", "silu")
# the derivative at NaN is not asserted for these: torch's own answer there is an artefact of a comparison with NaN
NAN_DER_UNASSERTED = ("relu", "leaky_relu", "ELU")

DOC_GELU_ERR, DOC_GELU_DER_ERR = 2.5e-7, 1.5e-7          # the bounds documented in csrc/common.h over [-12, 12]
F32 = np.float32
FLT_MAX, FLT_MIN, DENORM_MIN = float(np.finfo(F32).max), float(np.finfo(F32).tiny), 2.0 ** -149
BF16_LO, BF16_HI = 2.0 ** -100, 1e4                      # where a 3-way bf16 split of an fp32 value is exact
N_POINTS = 10240
# (sup |act'|, sup |act''|) over the real line, rounded up: what an error is carried through by a second activation
LIP = {"gelu": (1.13, 0.80), "silu": (1.10, 0.50)}

_F = torch.nn.functional
_TABLE = {"gelu": lambda v: _F.gelu(v), "tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu,
          "leaky_relu": lambda v: _F.leaky_relu(v, 0.1), "softplus": lambda v: _F.softplus(v, beta=1.0, threshold=20.0),
          "ELU": _F.elu, "silu": _F.silu}


# ---- the device GELU, restated --------------------------------------------------------------------------------------
TAIL_COEF = (2.275872930e-06, -3.296802970e-05, 1.572788460e-04, 2.024787827e-04, -7.142781746e-03, 5.254643410e-02,
             4.591930509e-01, 1.151106954e+00, 9.999999404e-01)
_LOG2E_HALF = F32(0.72134752044448170368)
_INV_SQRT_2PI = F32(0.39894228040143267794)
_LOG2_SQRT_2PI = F32(1.32574806473615975284)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _exp2(x):
    return np.exp2(np.asarray(x, np.float64)).astype(F32)


def normal_tail(ax, coef=TAIL_COEF):
    c = [F32(v) for v in coef]
    r = _fma(ax, c[0], c[1])
    for k in c[2:]:
        r = _fma(r, ax, k)
    return _exp2(-r)


def _clamp_abs(x):
    return np.minimum(np.abs(x), F32(6.5))               # np.minimum / np.maximum propagate NaN, as v_minimum3 / v_maximum3


def _relu(x):
    return (x - np.minimum(x, F32(0))).astype(F32)           # gelu_relu of common.h: NaN at -inf


def gelu_fwd(x, coef=TAIL_COEF):
    with np.errstate(all="ignore"):
        x = np.asarray(x, F32)
        ax = _clamp_abs(x)
        return _fma(-ax, normal_tail(ax, coef), _relu(x))


def _cdf(x, e):
    return np.where(x >= 0, (F32(1) - e).astype(F32), e).astype(F32)


def gelu_bwd(x, coef=TAIL_COEF):
    with np.errstate(all="ignore"):
        x = np.asarray(x, F32)
        e = normal_tail(_clamp_abs(x), coef)
        gauss = _exp2(((-_LOG2E_HALF * x).astype(F32) * x).astype(F32))
        return _fma((x * _INV_SQRT_2PI).astype(F32), gauss, _cdf(x, e))


def gelu_val_der(x, coef=TAIL_COEF):
    with np.errstate(all="ignore"):
        x = np.asarray(x, F32)
        ax = _clamp_abs(x)
        e = normal_tail(ax, coef)
        phi = _exp2(_fma((x * x).astype(F32), -_LOG2E_HALF, -_LOG2_SQRT_2PI))
        return _fma(-ax, e, _relu(x)), _fma(x, phi, _cdf(x, e))


# ---- float64 reference -----------------------------------------------------------------------------------------------
def reference(name, x32):
    """(act(x), act'(x)) in float64 from the exact float32 points: torch float64 functions, autograd for the derivative"""
    x = torch.from_numpy(np.ascontiguousarray(x32, dtype=F32)).double().requires_grad_(True)
    y = _TABLE[name](x)
    y.sum().backward()
    return y.detach().numpy(), x.grad.numpy()


def torch_f32(name, x32):
    """what torch-CPU float32 gives (the precision the reference implementation trains in)"""
    x = torch.from_numpy(np.ascontiguousarray(x32, dtype=F32)).requires_grad_(True)
    y = _TABLE[name](x)
    y.sum().backward()
    return y.detach().numpy(), x.grad.numpy()


def ulp32(ref):
    """spacing of float32 at |ref| (2^-149 below FLT_MIN), as float64"""
    with np.errstate(all="ignore"):
        a = np.minimum(np.abs(np.asarray(ref, np.float64)), FLT_MAX).astype(F32)
        return np.spacing(a).astype(np.float64)


# ---- sample points ----------------------------------------------------------------------------------------------------
CRITICAL = (0.0, 6.5, -6.5, 20.0, -20.0, 9.02, -9.02, 16.64, -16.64, 17.33, -17.33, 87.34, -87.34, 88.73, -88.73,
            103.98, -103.98, 4.5183, 1.4966, -1.4966)
NONFINITE_BASES = (3, 201, 402, 600)                      # 16-element groups that hold non-finite values at 0, 5, 10, 15
_NF = (float("nan"), float("inf"), float("-inf"))


def nonfinite_positions():
    """{position: value}: NaN, +inf, -inf at positions 0, 5, 10, 15 modulo 16, so that in a row-major operand whose width is a
    multiple of 16 every float4 that holds one also holds finite values"""
    out = {}
    for g, base in enumerate(NONFINITE_BASES):
        for j, off in enumerate((0, 5, 10, 15)):
            out[16 * base + off] = _NF[(g + j) % 3]
    return out


def finite_points():
    grid = np.linspace(-12.0, 12.0, 4096)
    mags = np.logspace(-30.0, 30.0, 512)
    wide = np.concatenate([mags, -mags])
    crit = []
    for c in CRITICAL:
        c = F32(c)
        crit += [np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))]
    edges = [0.0, -0.0, DENORM_MIN, -DENORM_MIN, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX]
    head = np.concatenate([grid, wide, np.asarray(crit, np.float64), np.asarray(edges, np.float64)])
    n_fill = N_POINTS - len(nonfinite_positions()) - head.size
    fill = np.linspace(-6.61, 6.59, n_fill)               # a second, finer grid across both GELU clamps
    return np.concatenate([head, fill]).astype(F32)


def sample_points():
    """the one deterministic vector of N_POINTS float32 sample points, non-finite values included"""
    nf = nonfinite_positions()
    v = np.empty(N_POINTS, F32)
    mask = np.ones(N_POINTS, bool)
    mask[list(nf)] = False
    v[mask] = finite_points()
    for p, val in nf.items():
        v[p] = val
    return v


def bf16_exact(v):
    """points a 3-way bf16 split represents exactly: finite, 2^-100 <= |x| <= 1e4, or +-0"""
    with np.errstate(all="ignore"):
        a = np.abs(v.astype(np.float64))
        return np.isfinite(v) & ((a == 0) | ((a >= BF16_LO) & (a <= BF16_HI)))


# ---- bounds -------------------------------------------------------------------------------------------------------------
def _abs_term(name, x, derivative):
    a = np.full(x.shape, 2.0 ** -23)
    if not derivative and name in UNBOUNDED:
        a[x > 20.0] = 0.0
    return a


class Bounds:
    """per activation: (c, a) for the value and the derivative on the finite points of `x32`, and what they were derived
    from (`table`: rows of name, kind, reference float32 error in ulps, margin, c)"""

    def __init__(self, x32):
        x = np.asarray(x32, F32)
        x = x[np.isfinite(x)]
        self.c, self.a_gelu, self.table = {}, {}, []
        v64, d64 = reference("gelu", x)
        self.restate_err = (float(np.abs(gelu_fwd(x).astype(np.float64) - v64).max()),
                            float(np.abs(gelu_bwd(x).astype(np.float64) - d64).max()))
        self.a_gelu = (self.restate_err[0] + 2.0 ** -24, self.restate_err[1] + 2.0 ** -24)
        for name in LIBM:
            (v64, d64), (v32, d32) = reference(name, x), torch_f32(name, x)
            for kind, r64, r32 in (("value", v64, v32), ("derivative", d64, d32)):
                a = _abs_term(name, x, kind == "derivative")
                with np.errstate(all="ignore"):
                    over = np.maximum(np.abs(r32.astype(np.float64) - r64) - a, 0.0) / ulp32(r64)
                e = float(over.max())
                self.c[(name, kind)] = max(4.0, 4.0 * e)
                self.table.append((name, kind, e, 4, self.c[(name, kind)]))

    def tol(self, name, kind, x, ref):
        """element-wise tolerance for finite references (name not in EXACT)"""
        if name == "gelu":
            return ulp32(ref) + self.a_gelu[kind == "derivative"]
        return self.c[(name, kind)] * ulp32(ref) + _abs_term(name, np.asarray(x, F32), kind == "derivative")


def check(name, kind, x32, got, bounds, what, extra_rel=0.0):
    """hold `got` (float32 array) to the rule at the points x32; returns (number of points compared, largest finite error).
    NaN reference -> NaN; infinite reference -> the same infinity; finite reference -> the bound (bit-exact for relu and
    leaky_relu, against torch float32).  The derivative at NaN of relu / leaky_relu / ELU is not compared.
    extra_rel: a further relative term (the rounding of a result that is stored in a narrower format)."""
    x = np.asarray(x32, F32).reshape(-1)
    got = np.asarray(got, F32).reshape(-1)
    assert got.shape == x.shape, f"{what}: {got.shape} vs {x.shape}"
    v64, d64 = reference(name, x)
    ref = d64 if kind == "derivative" else v64
    use = np.ones(x.shape, bool)
    if kind == "derivative" and name in NAN_DER_UNASSERTED:
        use &= ~np.isnan(x)
    rn, ri = np.isnan(ref) & use, np.isinf(ref) & use
    bad = rn & ~np.isnan(got)
    assert not bad.any(), (f"{what}: {int(bad.sum())} point(s) where the reference is NaN and the kernel is not; first x = "
                           f"{x[bad][0]!r}, got {got[bad][0]!r}")
    bad = ri & ~(got.astype(np.float64) == ref)
    assert not bad.any(), (f"{what}: {int(bad.sum())} point(s) where the reference is infinite and the kernel differs; first "
                           f"x = {x[bad][0]!r}, got {got[bad][0]!r}, reference {ref[bad][0]!r}")
    fin = np.isfinite(ref) & use
    if name in EXACT:
        t32 = torch_f32(name, x)[kind == "derivative"]
        bad = fin & ~(got == t32)
        assert not bad.any(), (f"{what}: {int(bad.sum())} point(s) not bit-exact; first x = {x[bad][0]!r}, got "
                               f"{got[bad][0]!r}, torch float32 {t32[bad][0]!r}")
        return int(use.sum()), 0.0
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(np.float64) - ref)
        tol = bounds.tol(name, kind, x, ref) + extra_rel * np.abs(ref)
        bad = fin & ~(err <= tol)
    if bad.any():
        i = int(np.flatnonzero(bad)[np.argmax((err / tol)[bad])])
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(fin.sum())} finite points out of bound; worst at x = {x[i]!r}: "
                             f"got {got[i]!r}, reference {ref[i]!r}, |d| = {err[i]:.3e}, bound {tol[i]:.3e}")
    return int(use.sum()), float(err[fin].max()) if fin.any() else 0.0
