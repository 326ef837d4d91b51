"""dpot_gemm_bf16p and dpot_gemm_bf16p_pair (csrc/gemm_bf16p.hip, planes == 1) on the MI355X, launch plan by launch plan:
every row of tests/bf16p_cases.py - each kernel form, tile order, super-block shape with and without idle workgroups, split-K
with ragged last splits, ragged M, the packed-output epilogues - against the float64 reference of tests/bf16p_ref.py.

Integer operands: no tolerance, every comparison is torch.equal (bf16p_ref explains why the kernels must give the bits of the
reference).  Before it launches, every row asserts that the library selects the plan the table names (skipped, the numbers
still compared, when DPOT_TUNE moves bf16p_bd or bf16p_shape off their defaults).  Outputs, packs and the split-K workspace
are NaN-poisoned between guards (tests/guard.py); split rows run twice and must repeat bit for bit."""
import pytest
import torch

import bf16p_cases as BC
import bf16p_ref as BR
import guard
from guard import guarded  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

RELU = BR.ACT_RELU


@pytest.fixture(scope="module")
def ops():
    from dpot_amd import ops as _ops
    from dpot_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _ops


def dev(t):
    return guard.wrap(t, "cuda")


def default_tuning(ops):
    return ops.tune("bf16p_bd") == 1 and ops.tune("bf16p_shape") == 1


def pack_operands(ops, A, W):
    """A [M, K] through dpot_bf16_pack_rows (the padded rows of a ragged M are what the library wrote), W [N, K] through a
    bf16 PanelPacks job; returns (A pack, W pack, what must stay alive)"""
    N, K = W.shape
    Wd = dev(W)
    pk = ops.PanelPacks([(Wd, N, K, K, False)], bf16=True)
    pk.refresh()
    return ops.bf16_pack_rows(dev(A)), pk.bufs[0], (pk, Wd)


def hold(got, ref64, what, tile_cols=256, dtype=torch.float32):
    """got == the reference, bit for bit; names the first differing (row, col) and its tile"""
    assert got.dtype == dtype, (what, got.dtype)
    want = ref64.to(dtype).to(got.device)
    msg = BR.first_difference(got.view(want.shape), want, 128, tile_cols)
    assert msg is None, f"{what}: {msg}"


def run_epilogues(ops, r, t, Ap, Wp, tile_cols, sk):
    M, N, K = r.M, r.N, r.K
    bias = dev(t["bias"])
    todo = {"full": ("relu", "res", "dact"), "relu": ("relu",), "res": ("res",)}[r.variant]
    args = {"relu": dict(mode=BR.EPI_ACT, bias=True), "res": dict(mode=BR.EPI_LINEAR, bias=True, res=True),
            "dact": dict(mode=BR.EPI_DACT)}
    refs = {what: BR.reference(t, what=f"{r.cell} [{what}]", **args[what]) for what in todo}     # computed once
    for rep in range(2 if sk > 1 else 1):               # split-K: twice, both equal to the reference (so to each other)
        for what in todo:
            tag = f"{r.cell} [{what}, run {rep}]"
            ref = refs[what]
            if what == "relu":
                C, pre = ops.gemm_bf16p(Ap, Wp, M, N, K, bias=bias, act=RELU, mode=ops.EPI_ACT, save_pre=r.variant == "full",
                                        splitk=sk)
                hold(C, ref["C"], tag + " relu(pre)", tile_cols)
                if r.variant == "full":
                    hold(pre, ref["pre"], tag + " saved pre-activation", tile_cols)
            elif what == "res":
                C, _ = ops.gemm_bf16p(Ap, Wp, M, N, K, bias=bias, res=dev(t["res"]), splitk=sk)
                hold(C, ref["C"], tag + " linear + residual", tile_cols)
            else:
                C, _ = ops.gemm_bf16p(Ap, Wp, M, N, K, act=RELU, mode=ops.EPI_DACT, aux=dev(t["aux"]), splitk=sk)
                hold(C, ref["C"], tag + " product * relu'(aux)", tile_cols)


def hold_packs(pr, pt, cs, ref, M, N, tag, tile_cols):
    bf = ref["C"].bfloat16()
    hold(BR.unpack_rows(pr, M, N), bf.double(), tag + " row pack", tile_cols)
    hold(BR.unpack_rows(pt, N, M).t().contiguous(), bf.double(), tag + " transposed pack", tile_cols)
    hold(cs.view(1, N), ref["colsum"].view(1, N), tag + " column sums", tile_cols)


def run_packed(ops, r, t, Ap, Wp, tile_cols):
    M, N, K = r.M, r.N, r.K
    bias = dev(t["bias"])
    kw = dict(pack_rows=True, pack_trans=True, colsum=True)
    # direct epilogue (in the accumulator layout): bias + relu, every packed output and the act' pack
    tag = f"{r.cell} [direct: relu, act' pack out]"
    ref = BR.reference(t, BR.EPI_ACT, bias=True, colsum=True, what=tag)
    C, D, pr, pt, cs = ops.gemm_bf16p_packed(Ap, Wp, M, N, K, bias=bias, act=RELU, mode=ops.EPI_ACT, save_dact=True, **kw)
    hold(C, ref["C"], tag + " fp32 output", tile_cols)
    hold_packs(pr, pt, cs, ref, M, N, tag, tile_cols)
    dact = BR.dact_of(ref["pre"])
    assert D.dtype == torch.bfloat16
    hold(BR.unpack_frag(D, M, N), dact.double(), tag + " act' pack", tile_cols)
    # direct epilogue: the product times the act' pack it has just written, no fp32 store
    tag = f"{r.cell} [direct: act' pack in, store=False]"
    ref = BR.reference(t, BR.EPI_DACT, dact=dact, colsum=True, what=tag)
    C, _, pr, pt, cs = ops.gemm_bf16p_packed(Ap, Wp, M, N, K, act=RELU, mode=ops.EPI_DACT, dact=D, store=False, **kw)
    assert C is None
    hold_packs(pr, pt, cs, ref, M, N, tag, tile_cols)
    # staged epilogue (epi_fragment_pack): a saved pre-activation and a residual next to the packs
    tag = f"{r.cell} [staged: relu, pre saved, residual]"
    ref = BR.reference(t, BR.EPI_ACT, bias=True, res=True, colsum=True, what=tag)
    C, pre, pr, pt, cs = ops.gemm_bf16p_packed(Ap, Wp, M, N, K, bias=bias, act=RELU, mode=ops.EPI_ACT, save_pre=True,
                                               res=dev(t["res"]), **kw)
    hold(C, ref["C"], tag + " fp32 output", tile_cols)
    hold(pre, ref["pre"], tag + " saved pre-activation", tile_cols)
    hold_packs(pr, pt, cs, ref, M, N, tag, tile_cols)
    # staged epilogue: relu'(aux)
    tag = f"{r.cell} [staged: relu'(aux)]"
    ref = BR.reference(t, BR.EPI_DACT, colsum=True, what=tag)
    C, _, pr, pt, cs = ops.gemm_bf16p_packed(Ap, Wp, M, N, K, act=RELU, mode=ops.EPI_DACT, aux=dev(t["aux"]), **kw)
    hold(C, ref["C"], tag + " fp32 output", tile_cols)
    hold_packs(pr, pt, cs, ref, M, N, tag, tile_cols)


@pytest.mark.parametrize("r", BC.ROWS, ids=BC.row_id)
def test_rows_equal_the_float64_reference(ops, guarded, r):
    packed = r.variant == "packed"
    sk = ops._lib.load().dpot_gemm_bf16p_splitk(r.M, r.N, r.K) if r.splitk is None else r.splitk
    plan = ops.gemm_bf16p_plan(r.M, r.N, r.K, sk, 1, packed)
    if default_tuning(ops):
        assert plan is not None and tuple(plan) == tuple(r.plan), (plan, r.plan)
    want = {"full": ("bias", "res", "aux"), "relu": ("bias",), "res": ("bias", "res"), "packed": ("bias", "res", "aux")}
    t = BR.build(r.M, r.N, r.K, r.vmax, BC.seed_of(r), want[r.variant])
    Ap, Wp, keep = pack_operands(ops, t["A"], t["W"])
    tile_cols = 192 if plan.kind >= 8 else 256
    if packed:
        run_packed(ops, r, t, Ap, Wp, tile_cols)
    else:
        run_epilogues(ops, r, t, Ap, Wp, tile_cols, sk)
    torch.cuda.synchronize()
    del keep


@pytest.mark.parametrize("r", BC.PAIR_ROWS, ids=BC.row_id)
def test_pair_rows_equal_the_float64_reference(ops, guarded, r):
    plan = ops.gemm_bf16p_pair_plan(r.M0, r.N0, r.M1, r.N1, r.K, r.splitk)
    if default_tuning(ops):
        assert plan is not None and tuple(plan) == tuple(r.plan), (plan, r.plan)
    seed = BC.seed_of(r)
    t0 = BR.build(r.M0, r.N0, r.K, r.vmax, seed, ())
    t1 = BR.build(r.M1, r.N1, r.K, r.vmax, seed + 5, ())
    A0, W0, keep0 = pack_operands(ops, t0["A"], t0["W"])
    A1, W1, keep1 = pack_operands(ops, t1["A"], t1["W"])
    ref0 = BR.reference(t0, what=r.cell + " problem 0")["C"]
    ref1 = BR.reference(t1, what=r.cell + " problem 1")["C"]
    tile_cols = 192 if plan.kind >= 8 else 256
    for rep in range(2 if r.splitk > 1 else 1):
        C0, C1 = ops.gemm_bf16p_pair(A0, W0, r.M0, r.N0, A1, W1, r.M1, r.N1, r.K, splitk=r.splitk)
        hold(C0, ref0, f"{r.cell} problem 0, run {rep}", tile_cols)
        hold(C1, ref1, f"{r.cell} problem 1, run {rep}", tile_cols)
    torch.cuda.synchronize()
    del keep0, keep1


def test_refused_launches_raise_and_write_nothing(ops, guarded):
    from dpot_amd._lib import DpotHipError
    pk = dev(torch.zeros(64 * 256, dtype=torch.bfloat16))           # a valid, aligned operand: refused before it is read
    for what, M, N, K, sk, packed in BC.REFUSED:
        out = guard.full_nan((M, N))
        with pytest.raises(DpotHipError):
            ops.gemm_bf16p_packed(pk, pk, M, N, K, out=out, splitk=sk, pack_rows=packed)
        torch.cuda.synchronize()
        assert bool(out.isnan().all()), what
    for what, M0, N0, M1, N1, K, sk in BC.PAIR_REFUSED:
        o0, o1 = guard.full_nan((M0, N0)), guard.full_nan((M1, N1))
        with pytest.raises(DpotHipError):
            ops.gemm_bf16p_pair(pk, pk, M0, N0, pk, pk, M1, N1, K, out0=o0, out1=o1, splitk=sk)
        torch.cuda.synchronize()
        assert bool(o0.isnan().all()) and bool(o1.isnan().all()), what
    # the neighbours that are admitted: the refusals above are the rules', not the harness's
    t = BR.build(64, 256, 160, 4, 1, ())
    A, W, keep = pack_operands(ops, t["A"], t["W"])
    ref = BR.reference(t)["C"]
    hold(ops.gemm_bf16p(A, W, 64, 256, 160, splitk=5)[0], ref, "splitk == slabs")
    C0, C1 = ops.gemm_bf16p_pair(A, W, 64, 256, A, W, 64, 256, 160, splitk=3)
    hold(C0, ref, "pair, 5 slabs in 3 splits")
    hold(C1, ref, "pair, 5 slabs in 3 splits")
