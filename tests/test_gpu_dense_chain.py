"""GPU tests of functional._dense_fwd / _dense_bwd / _res_bwd - the chain of dense layers every plain stage runs through -
against a float64 torch restatement with autograd, tolerance of tests/helpers.py.  Chains of 1, 2 and 3 layers; widths that
are multiples of 4 but not of 32, and one first layer with K = 512, which ops.small_linear takes below 129 rows; 5 and 132
rows, either side of that limit; with and without a residual table res[R, N] (res_mod = R, res_div = 2); with and without
the first layer's data gradient; the first layer's input always handed over as a callable.

The residual's gradient is a sum over row groups (ops.group_rowsum), defined for M = groups * R * res_div rows only: with
5 rows the table is a constant (output and every other gradient are checked), and 6 rows stand in for the small side where
dres is checked.  Buffers are guarded and NaN-poisoned (tests/guard.py)."""
import functools

import pytest
import torch
import torch.nn.functional as TF

import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close

pytestmark = pytest.mark.gpu

ACT = "gelu"
R, DIV = 3, 2
# layer widths K -> ... -> N_last
WIDTHS = [(8, 12), (8, 12, 4), (8, 12, 20, 4), (512, 12, 8)]
ROWS = [5, 132]
CASES = [(w, M, res, dx) for w in WIDTHS for M in ROWS + [6] for res in (False, True) for dx in (False, True)
         if M != 6 or res]
IDS = ["-".join(map(str, w)) + f"_M{M}" + ("_res" if res else "") + ("_dx" if dx else "") for w, M, res, dx in CASES]


@functools.lru_cache(maxsize=None)
def case(widths, M, res):
    """CPU inputs (fp32) and the float64 expectations of one chain, computed once and shared (never modified)"""
    gen = torch.Generator().manual_seed(7300 + 97 * len(widths) + widths[0] + M)
    x = torch.randn(M, widths[0], generator=gen)
    layers = [(torch.randn(n, k, generator=gen) / k ** 0.5, torch.randn(n, generator=gen) * 0.1)
              for k, n in zip(widths[:-1], widths[1:])]
    table = torch.randn(R, widths[-1], generator=gen) if res else None
    dy = torch.randn(M, widths[-1], generator=gen)
    leaves = [t.double().requires_grad_(True) for t in [x] + [t for l in layers for t in l] + ([table] if res else [])]
    y = leaves[0]
    for i in range(len(layers)):
        y = TF.linear(y, leaves[1 + 2 * i], leaves[2 + 2 * i])
        if i < len(layers) - 1:
            y = TF.gelu(y)
    if res:
        y = y + leaves[-1][(torch.arange(M) // DIV) % R]
    grads = torch.autograd.grad(y, leaves, dy.double())
    return dict(x=x, layers=layers, table=table, dy=dy, y=y.detach(), dx=grads[0],
                dWb=[(grads[1 + 2 * i], grads[2 + 2 * i]) for i in range(len(layers))], dres=grads[-1] if res else None)


def test_small_linear_takes_the_wide_first_layer_below_129_rows():
    """the two rows counts do straddle the route switch of ops.linear_fwd, and only the K = 512 chain reaches small_linear"""
    from dpot_amd import ops
    assert ops.small_linear_supported(5, 12, 512) and not ops.small_linear_supported(132, 12, 512)
    assert not ops.small_linear_supported(5, 12, 8)


@pytest.mark.parametrize("widths,M,res,need_dx", CASES, ids=IDS)
def test_dense_chain_against_float64(widths, M, res, need_dx, guarded):
    from dpot_amd import functional as F
    from dpot_amd import ops
    c = case(widths, M, res)
    act = ops.ACT_IDS[ACT]
    x = guard.wrap(c["x"], "cuda")
    layers = [(guard.wrap(W, "cuda"), guard.wrap(b, "cuda")) for W, b in c["layers"]]
    table = guard.wrap(c["table"], "cuda") if res else None
    dy = guard.wrap(c["dy"], "cuda")
    calls = []

    def first_input():
        calls.append(1)
        return x.clone()

    y, ins, pres = F._dense_fwd(first_input, layers, act, table, DIV if res else 0, R if res else 0)
    assert len(calls) == 1 and ins[0] is first_input and len(ins) == len(layers) and len(pres) == len(layers) - 1
    assert_close(y, c["y"], "y")
    dx, grads = F._dense_bwd(dy, ins, pres, [W for W, _ in layers], act, need_dx)
    assert len(calls) == 2, "the first layer's input is made exactly once in the backward"
    for i, ((dW, db), (rW, rb)) in enumerate(zip(grads, c["dWb"])):
        assert_close(dW, rW, f"dW{i}")
        assert_close(db, rb, f"db{i}")
    if need_dx:
        assert_close(dx, c["dx"], "dx")
    else:
        assert dx is None
    if res and M % (R * DIV) == 0:
        assert_close(F._res_bwd(dy, DIV, R), c["dres"], "dres")
    torch.cuda.synchronize()


def test_res_bwd_of_a_row_by_row_residual_is_dy():
    from dpot_amd import functional as F
    dy = torch.zeros(4, 8)
    assert F._res_bwd(dy, 0, 0) is dy
