"""Case table of the AFNO mixer kernel tests (csrc/afno_mlp.hip: afno_mlp2_kernel<RT, NW, ACTK>, the four-product form, and
afno_mlp3_kernel<RT, BS, ACTK, SPLIT>, the three-product form).

One module, two readers: tests/test_cpu_afno_mixer.py asserts with the library's own selection (dpot_afno_mlp2_plan) that every
case still reaches the instantiation it is here for and that the table reaches every instantiation that exists
(dpot_afno_mlp2_plans); tests/test_gpu_afno_mixer.py runs the kernels on the very same tuples, inputs and float64 references.

A case is (layout, nb, bs, M, act, mode, outputs, ldx_pad, ldo_pad, want_rt, want_form, note):
    layout    0 four-product packs (afno_block_weights), 1 three-product packs (AfnoPacks)
    act       "gelu" (the GELU instantiation), "relu" / "none" / "silu" (the run-time switch)
    mode      0 forward, 1 backward data path
    outputs   which of the optional outputs are asked for: a subset of ("pre", "mid"); Y is always written
    ld*_pad   floats between the rows of X (ldx = nb*N + ldx_pad) and of aux and every output (ldo = nb*N + ldo_pad)
    want_rt   16-row tiles per panel the cost rule picks (pick_rt below restates it; the CPU test holds table, restatement
              and library to one another);  want_form  FOUR / THREE / SPLIT

Shapes.  RT > 1 needs nb * ceil(M / 16) > 256 workgroups, so the table uses many small blocks rather than many rows; _SHAPES holds,
per RT, four (nb, M) with the last panel holding 1 row, 16 RT - 1 rows, exactly one row tile (RT 1: 7 rows) and all its rows.
Every instantiation (form, bs, RT, gelu) gets the forward with `pre` and the backward with `mid` (the product's own calls), the
four shapes rotating over the four launches, so that every (form, bs, RT) meets all four edges.  The other output combinations,
the padded leading dimensions, M < 16, the remainders 1 / 7 / 0 of the chiplet work-item map with an odd block count and the
places where M can end relative to the split form's row-tile partition (RA = (RT + 1) / 2 tiles on waves 4 / 5, RT - RA on waves
6 / 7) follow as sections of their own.

INT cases run on small integer operands (|X| <= 4, |W| <= 2, |b| <= 8, aux a half-integer): every product and partial sum of both
layers stays below 2^24 (partial_sum_bounds, asserted by the CPU test), so fp32 is exact in any summation order and in Gauss's
three-product form alike, and the kernels are held to the float64 result with torch.equal.

REAL cases run on random data against float64 at helpers.assert_close's default and at the norm-wise bound
    ||kernel - float64|| / ||float64||  <=  F[form] * max(e32, 2^-24)
with e32 the same error of torch-CPU float32 evaluating the same formula.  Measured ratios (MI355X, the REAL cases below, both
activations, every output; printed by the GPU test as `afno-mixer-error` lines):
    FOUR    largest 1.441  (pre 0.995-1.391, mid 0.933-1.441, Y 0.945-1.423, dO1pre 0.835-1.384, dS 0.906-1.390)
    THREE   largest 1.428  (pre 1.006-1.418, mid 0.923-1.390, Y 0.982-1.425, dO1pre 0.945-1.409, dS 0.985-1.428)
    SPLIT   largest 1.027  (pre 1.025-1.027, mid 0.961-0.970, Y 1.008-1.015, dO1pre 0.960-1.025, dS 0.988-1.027)
    act(aux), the re-derived activation (no product): 0.43-0.68 in every form
F is twice the largest ratio seen per form.  No ratio comes near 8.  The larger figures, about sqrt(2), are those of bs = 128
(K = 256 per real product sum), where the MFMA chain adds the 256 products of a dot product into one accumulator in order and
torch-CPU's float32 GEMM presumably into several partial sums; at bs = 96, where alone the split form exists, both are level.  On this
data the three-product form is no worse than the four-product form, inside its documented bound of about 2x.  The GELU cases of
the INT table, whose Y is held to the same bound, were measured too: at most 1.41 (FOUR), 1.74 (THREE), 1.42 (SPLIT).
"""
import functools
import math
from collections import namedtuple

import torch

FOUR, THREE, SPLIT, REFUSED = 0, 1, 2, -1
FORM_NAMES = {FOUR: "four", THREE: "three", SPLIT: "split"}
ACT_IDS = {"none": 0, "gelu": 1, "relu": 4, "silu": 8}
NUM_CU = 256

# norm-wise error bound: twice the largest measured ratio of a form (the docstring holds the measurements)
F = {FOUR: 2.89, THREE: 2.86, SPLIT: 2.06}

Case = namedtuple("Case", "layout nb bs M act mode outputs ldx_pad ldo_pad want_rt want_form note")


def case_id(c):
    out = "+".join(c.outputs) or "Y"
    pad = f"-ld{c.ldx_pad}.{c.ldo_pad}" if c.ldx_pad or c.ldo_pad else ""
    return f"L{c.layout}-nb{c.nb}-bs{c.bs}-M{c.M}-{c.act}-{'bwd' if c.mode else 'fwd'}-{out}{pad}"


# ---- the selection, restated ------------------------------------------------------------------------------------------
def pick_rt(M, nb):
    """fewest rounds of nb * panels workgroups over the 256 CUs, a round costing 16 RT + 12 rows' worth; ties to the larger RT"""
    best, best_cost = 5, None
    for rt in (5, 4, 3, 2, 1):
        panels = -(-M // (16 * rt))
        rounds = -(-panels * nb // NUM_CU)
        cost = rounds * (16 * rt + 12)
        if best_cost is None or cost < best_cost:
            best, best_cost = rt, cost
    return best


def form_of(bs, layout, rt):
    if layout == 0:
        return FOUR if bs in (32, 64, 96, 128) else REFUSED
    if layout != 1 or bs not in (64, 96, 128):
        return REFUSED
    return SPLIT if bs == 96 and rt >= 2 else THREE


def plan(M, nb, bs, layout, act):
    """(form, rt, panels, compute waves, gelu) as dpot_afno_mlp2_plan reports them"""
    if M <= 0 or nb <= 0:
        return (REFUSED, 0, 0, 0, False)
    rt = pick_rt(M, nb)
    form = form_of(bs, layout, rt)
    if form == REFUSED:
        return (REFUSED, 0, 0, 0, False)
    return (form, rt, -(-M // (16 * rt)), 8 if form == SPLIT else bs // 16, act == "gelu")


def key(c):
    """the instantiation a case is in the table for: (form, bs, rt, gelu), a tuple of dpot_afno_mlp2_plans"""
    return (c.want_form, c.bs, c.want_rt, c.act == "gelu")


# ---- the table --------------------------------------------------------------------------------------------------------
# per RT: (nb, M, rows of the last panel) - 1 row, 16 RT - 1 rows, one row tile (RT 1: 7 rows), a full panel
_SHAPES = {1: [(3, 17, 1), (3, 31, 15), (3, 23, 7), (3, 32, 16)],
           2: [(96, 33, 1), (65, 63, 31), (7, 592, 16), (3, 1376, 32)],
           3: [(40, 193, 1), (9, 911, 47), (5, 1648, 16), (9, 912, 48)],
           4: [(7, 1729, 1), (96, 127, 63), (7, 1744, 16), (24, 512, 64)],
           5: [(33, 481, 1), (65, 239, 79), (33, 496, 16), (65, 240, 80)]}
_EDGE = {0: "the last panel holds one row", 1: "the last panel holds 16 RT - 1 rows",
         2: "the last panel holds one row tile, the others lie wholly past M (clamped to row M - 1)",
         3: "M a multiple of 16 RT"}
_WIDTHS = [(0, 32), (0, 64), (0, 96), (0, 128), (1, 64), (1, 96), (1, 128)]


def _form(layout, bs, rt):
    return form_of(bs, layout, rt)


INT = []
# ---- every instantiation, forward with `pre` and backward with `mid`, the four edge shapes rotating -------------------------
for _wi, (_layout, _bs) in enumerate(_WIDTHS):
    for _rt in (1, 2, 3, 4, 5):
        _launches = [("gelu", 0, ("pre",)), ("gelu", 1, ("mid",)), ("relu", 0, ("pre",)),
                     ("relu" if _wi % 2 == 0 else "none", 1, ("mid",))]
        for _slot, (_act, _mode, _outs) in enumerate(_launches):
            _e = (_slot + _wi + _rt) % 4
            _nb, _M, _rows = _SHAPES[_rt][_e]
            INT.append(Case(_layout, _nb, _bs, _M, _act, _mode, _outs, 0, 0, _rt, _form(_layout, _bs, _rt), _EDGE[_e]))
# ---- the other output combinations and padded leading dimensions: one RT per form and width ---------------------------------
#   forward {} (inference), {pre, mid}; backward {mid, pre} with GELU (gelu_val_der) and without (act_fwd + act_bwd); then both
#   directions with ldx = nb*N + 4 and ldo = nb*N + 8 in the same launch
_COMBO_RT = [(0, 32, 2), (0, 64, 3), (0, 96, 4), (0, 128, 5), (1, 64, 4), (1, 96, 1), (1, 96, 3), (1, 128, 2)]
for _layout, _bs, _rt in _COMBO_RT:
    _f = _form(_layout, _bs, _rt)
    (_nb1, _M1, _), (_nb2, _M2, _) = _SHAPES[_rt][1], _SHAPES[_rt][2]
    INT += [Case(_layout, _nb1, _bs, _M1, "gelu", 0, (), 0, 0, _rt, _f, "inference: no optional output"),
            Case(_layout, _nb2, _bs, _M2, "none", 0, ("pre", "mid"), 0, 0, _rt, _f, "every forward output, identity activation"),
            Case(_layout, _nb1, _bs, _M1, "gelu", 0, ("pre", "mid"), 0, 0, _rt, _f, "every forward output, GELU"),
            Case(_layout, _nb2, _bs, _M2, "gelu", 1, ("mid", "pre"), 0, 0, _rt, _f, "backward that re-derives act(aux): gelu_val_der"),
            Case(_layout, _nb1, _bs, _M1, "relu", 1, ("mid", "pre"), 0, 0, _rt, _f, "backward that re-derives act(aux): act_fwd, act_bwd"),
            Case(_layout, _nb1, _bs, _M1, "relu", 0, ("pre", "mid"), 4, 8, _rt, _f, "ldx = nb*N + 4, ldo = nb*N + 8"),
            Case(_layout, _nb1, _bs, _M1, "relu", 1, ("mid", "pre"), 4, 8, _rt, _f, "ldx = nb*N + 4, ldo = nb*N + 8 (aux too)"),
            Case(_layout, _nb2, _bs, _M2, "gelu", 1, ("mid",), 4, 8, _rt, _f, "ldx = nb*N + 4, ldo = nb*N + 8, GELU backward")]
# ---- fewer rows than one row tile -------------------------------------------------------------------------------------------
INT += [Case(0, 3, 32, 1, "relu", 0, ("pre",), 0, 0, 1, FOUR, "M = 1"),
        Case(0, 5, 128, 9, "gelu", 1, ("mid",), 0, 0, 1, FOUR, "M = 9 < 16"),
        Case(0, 300, 64, 1, "gelu", 0, ("pre", "mid"), 0, 0, 1, FOUR, "M = 1 on 300 blocks: two rounds of workgroups"),
        Case(1, 3, 64, 1, "gelu", 0, ("pre",), 0, 0, 1, THREE, "M = 1"),
        Case(1, 5, 128, 13, "relu", 1, ("mid", "pre"), 0, 0, 1, THREE, "M = 13 < 16"),
        Case(1, 2, 96, 5, "relu", 0, ("pre", "mid"), 0, 0, 1, THREE, "M = 5 < 16, six column tiles")]
# ---- chiplet work-item map: nb * panels % 8 of 1, 7, 0 with an odd block count ---------------------------------------------
INT += [Case(0, 9, 64, 5, "relu", 0, ("pre",), 0, 0, 1, FOUR, "9 items: remainder 1"),
        Case(0, 9, 32, 453, "gelu", 1, ("mid",), 0, 0, 2, FOUR, "9 x 15 = 135 items: remainder 7"),
        Case(0, 11, 96, 765, "relu", 0, ("pre", "mid"), 0, 0, 3, FOUR, "11 x 16 = 176 items: remainder 0"),
        Case(1, 7, 128, 5, "gelu", 0, ("pre",), 0, 0, 1, THREE, "7 items: remainder 7"),
        Case(1, 5, 64, 1733, "relu", 1, ("mid",), 0, 0, 3, THREE, "5 x 37 = 185 items: remainder 1"),
        Case(1, 9, 128, 485, "relu", 0, ("pre", "mid"), 0, 0, 2, THREE, "9 x 16 = 144 items: remainder 0"),
        Case(1, 17, 96, 261, "relu", 0, ("pre",), 0, 0, 2, SPLIT, "17 x 9 = 153 items: remainder 1"),
        Case(1, 9, 96, 1413, "gelu", 1, ("mid",), 0, 0, 4, SPLIT, "9 x 23 = 207 items: remainder 7"),
        Case(1, 13, 96, 1277, "relu", 1, ("mid", "pre"), 0, 0, 5, SPLIT, "13 x 16 = 208 items: remainder 0")]
# ---- split form: where M ends relative to the partition (RA row tiles on waves 4 / 5, the rest on waves 6 / 7) ---------------
#   RT 2 (RA 1) and the upper edge of RT 3 (RA 2) are the 1 / 16 / 16 RT - 1 row shapes above
INT += [Case(1, 65, 96, 116, "relu", 0, ("pre", "mid"), 0, 0, 3, SPLIT, "RT 3: the last panel ends inside row tile RA - 1 = 1 (20 rows)"),
        Case(1, 11, 96, 752, "relu", 1, ("mid",), 0, 0, 3, SPLIT, "RT 3: ends exactly between tiles RA - 1 and RA (32 rows)"),
        Case(1, 65, 96, 148, "relu", 1, ("mid", "pre"), 0, 0, 4, SPLIT, "RT 4: ends inside row tile RA - 1 = 1 (20 rows)"),
        Case(1, 65, 96, 160, "gelu", 0, ("pre", "mid"), 0, 0, 4, SPLIT, "RT 4: ends exactly between tiles 1 and 2 (32 rows)"),
        Case(1, 96, 96, 104, "relu", 0, ("pre", "mid"), 0, 0, 4, SPLIT, "RT 4: ends inside row tile RA = 2 (40 rows)"),
        Case(1, 9, 96, 1800, "relu", 0, ("pre", "mid"), 0, 0, 5, SPLIT, "RT 5: ends inside row tile RA - 1 = 2 (40 rows)"),
        Case(1, 9, 96, 1808, "gelu", 1, ("mid",), 0, 0, 5, SPLIT, "RT 5: ends exactly between tiles 2 and 3 (48 rows)"),
        Case(1, 13, 96, 1256, "relu", 1, ("mid",), 0, 0, 5, SPLIT, "RT 5: ends inside row tile RA = 3 (56 rows)")]

# ---- real-valued data: each form and width at RT 1, RT 5 and a ragged RT 3; bs = 96 at RT 1 (the only non-split launch) and
# the split form at RT 2, 3 (ragged) and 5; GELU and SiLU; forward with every output and backward with every output --------------
REAL = []
for _layout, _bs in _WIDTHS:
    _shapes = [(3, 32, 1), (65, 240, 5), (9, 911, 3)]
    if (_layout, _bs) == (1, 96):
        _shapes.insert(1, (65, 63, 2))
    for _nb, _M, _rt in _shapes:
        for _act in ("gelu", "silu"):
            REAL.append(Case(_layout, _nb, _bs, _M, _act, 0, ("pre", "mid"), 0, 0, _rt, _form(_layout, _bs, _rt),
                             "forward and backward against float64"))

# same bits on a second call into fresh outputs: one case per form
REPEAT = [Case(0, 9, 96, 911, "gelu", 0, ("pre", "mid"), 0, 0, 3, FOUR, "second call"),
          Case(1, 65, 128, 239, "gelu", 0, ("pre", "mid"), 0, 0, 5, THREE, "second call"),
          Case(1, 96, 96, 127, "gelu", 0, ("pre", "mid"), 0, 0, 4, SPLIT, "second call")]

# three-product Y against four-product Y on the same weights: (nb, bs, M, rt)
CROSS = [(65, 64, 63, 2), (65, 96, 63, 2), (65, 128, 63, 2), (96, 64, 127, 4), (96, 96, 127, 4), (96, 128, 127, 4)]

CASES = INT + REAL + REPEAT


# ---- inputs -------------------------------------------------------------------------------------------------------------
def _gen(c, salt):
    return torch.Generator().manual_seed((((c.layout * 131 + c.nb) * 131 + c.bs) * 4099 + c.M) * 7 + c.mode + 7919 * salt)


def _randint(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def int_inputs(c):
    """float32 CPU tensors holding small integers: X [M, nb*N] (|X| <= 4), w1, w2 [2, nb, bs, bs] (|w| <= 2: every block and both
    parts their own draw), b1, b2 [2, nb, bs] (|b| <= 8), aux [M, nb*N] half-integers in [-3.5, 3.5] (never 0: relu' is 0 or 1)"""
    g = _gen(c, 1)
    N = 2 * c.bs
    return {"X": _randint(g, -4, 4, c.M, c.nb * N), "w1": _randint(g, -2, 2, 2, c.nb, c.bs, c.bs),
            "w2": _randint(g, -2, 2, 2, c.nb, c.bs, c.bs), "b1": _randint(g, -8, 8, 2, c.nb, c.bs),
            "b2": _randint(g, -8, 8, 2, c.nb, c.bs), "aux": _randint(g, -4, 3, c.M, c.nb * N) + 0.5}


def real_inputs(c):
    """the data of test_afno_mlp3_three_product_form: N(0, 1) rows, weights scaled by 1 / sqrt(N), biases by 0.3"""
    g = _gen(c, 2)
    N = 2 * c.bs
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).float()
    return {"X": r(c.M, c.nb * N), "w1": r(2, c.nb, c.bs, c.bs, scale=1 / math.sqrt(N)),
            "w2": r(2, c.nb, c.bs, c.bs, scale=1 / math.sqrt(N)), "b1": r(2, c.nb, c.bs, scale=0.3),
            "b2": r(2, c.nb, c.bs, scale=0.3), "dO2": r(c.M, c.nb * N)}


def wbig(w):
    """[2, nb, bs, bs] complex weight -> the real [nb, N, N] matrix [[Wr, Wi], [-Wi, Wr]] (W[k][n]) of the planar layout"""
    wr, wi = w[0], w[1]
    return torch.cat([torch.cat([wr, wi], dim=2), torch.cat([-wi, wr], dim=2)], dim=1)


def bbig(b):
    return torch.cat([b[0], b[1]], dim=1)                  # [nb, N] = [br | bi]


def partial_sum_bounds(c, t):
    """float64 upper bounds, from the absolute values of a case's integer inputs, of every partial sum either form can hold in
    either layer and either mode: |sum_k x_k w_kn| <= ||x||_1 max|w| per block, the three-product form's (Sr + Si)(Wr + Wi)
    with ||xr||_1 + ||xi||_1 and max(|Wr| + |Wi|); the activations used on integers (relu, none, relu') never enlarge a value"""
    N = 2 * c.bs
    x1 = t["X"].double().abs().view(c.M, c.nb, N).sum(2).max().item()              # ||x||_1 of a block row = re + im parts
    wa, wb = (t["w1"], t["w2"]) if c.mode == 0 else (t["w2"], t["w1"])
    sa = (wa[0].double().abs() + wa[1].double().abs()).max().item()                # max(|Wr| + |Wi|) >= max|W|
    sb = (wb[0].double().abs() + wb[1].double().abs()).max().item()
    ba = t["b1"].abs().max().item() if c.mode == 0 else 0.0
    bb = t["b2"].abs().max().item() if c.mode == 0 else 0.0
    l1 = x1 * sa + ba                                                              # any product sum of layer 1, bias included
    l2 = N * l1 * sb + bb                                                          # ||mid||_1 <= N max|mid| <= N l1
    return l1, l2


# ---- float64 references -------------------------------------------------------------------------------------------------------
def _act64(name, x):
    x = x.clone().requires_grad_(True)
    f = {"gelu": torch.nn.functional.gelu, "silu": torch.nn.functional.silu, "relu": torch.relu, "none": lambda v: v * 1.0}[name]
    y = f(x)
    y.sum().backward()
    return y.detach(), x.grad


def layer(x, W, b=None, transpose=False):
    """[M, nb*N] x [nb, N, N] -> [M, nb*N] per block, in the dtype of the operands; transpose: multiply by W^T"""
    nb, N = W.shape[0], W.shape[1]
    y = torch.einsum("mko,kno->mkn" if transpose else "mkn,kno->mko", x.view(-1, nb, N), W)
    if b is not None:
        y = y + b
    return y.reshape(x.shape[0], nb * N)


def forward_ref(t, act, dtype=torch.float64):
    """{pre, mid, Y} of mode 0 in `dtype` (float64: the reference; float32: the yardstick e32 of the norm-wise bound)"""
    X, W1, W2 = t["X"].to(dtype), wbig(t["w1"]).to(dtype), wbig(t["w2"]).to(dtype)
    pre = layer(X, W1, bbig(t["b1"]).to(dtype))
    mid = _act64(act, pre)[0]
    return {"pre": pre, "mid": mid, "Y": layer(mid, W2, bbig(t["b2"]).to(dtype))}


def backward_ref(t, act, X, aux, dtype=torch.float64):
    """{pre = act(aux), mid = (X W2^T) act'(aux), Y = mid W1^T} of mode 1; aux is float32 data (what the kernel reads)"""
    W1, W2 = wbig(t["w1"]).to(dtype), wbig(t["w2"]).to(dtype)
    a, d = _act64(act, aux.to(dtype))
    mid = layer(X.to(dtype), W2, transpose=True) * d
    return {"pre": a, "mid": mid, "Y": layer(mid, W1, transpose=True)}


@functools.lru_cache(maxsize=2)
def int_reference(c):
    """the float64 result of an INT case (callers must not modify it)"""
    t = int_inputs(c)
    return forward_ref(t, c.act) if c.mode == 0 else backward_ref(t, c.act, t["X"], t["aux"])


def rel_err(got, ref):
    ref = ref.double()
    return ((got.detach().cpu().double() - ref).norm() / ref.norm()).item()
