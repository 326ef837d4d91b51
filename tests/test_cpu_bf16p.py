"""The launch plans of the bf16 panel GEMM (dpot_gemm_bf16p_plan, dpot_gemm_bf16p_pair_plan: the selection the launches
themselves read), checked without a GPU against the table of bf16p_cases.py: every row gets the plan it names, the table
reaches every cell the plan can produce under default tuning, the workgroup -> tile map of every tile order in the table is a
bijection, and the integer reference of bf16p_ref.py is exact."""
import itertools

import pytest
import torch

import bf16p_cases as BC
import bf16p_ref as BR


@pytest.fixture(scope="module")
def built_lib():
    from dpot_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def ops(built_lib):
    from dpot_amd import _lib, ops as _ops
    _lib.load()
    assert _ops.tune("bf16p_bd") == 1 and _ops.tune("bf16p_shape") == 1, "the table names the plans of the default tuning"
    return _ops


def splitk_of(ops, r):
    return ops._lib.load().dpot_gemm_bf16p_splitk(r.M, r.N, r.K) if r.splitk is None else r.splitk


def test_cells_are_unique():
    ids = [r.cell for r in BC.ROWS + BC.PAIR_ROWS]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("r", BC.ROWS, ids=BC.row_id)
def test_every_row_gets_the_plan_it_names(ops, r):
    packed = r.variant == "packed"
    sk = splitk_of(ops, r)
    plan = ops.gemm_bf16p_plan(r.M, r.N, r.K, sk, 1, packed)
    assert plan is not None and tuple(plan) == tuple(r.plan), (plan, r.plan)
    assert ops._lib.load().dpot_gemm_bf16p_kernel_kind(r.M, r.N, r.K, sk, 1, int(packed)) == plan.kind
    assert ops.gemm_bf16p_supported(r.M, r.N, r.K)
    # what the label claims, recomputed from the plan
    nslab = r.K // 32
    assert plan.tilesM == -(-r.M // 128) and plan.tilesN * (192 if plan.kind >= 8 else 256) == r.N
    assert packed or ("ragged-M" in r.cell) == (r.M % 128 != 0 and r.M > 1)
    assert plan.slabs_per_split == -(-nslab // plan.splits) and plan.slabs_per_split * (plan.splits - 1) < nslab
    if "ragged-last-split" in r.cell:
        assert nslab % plan.splits != 0
    if r.variant == "packed":
        assert r.M % 32 == 0 and r.M % 128 != 0 and plan.splits == 1
    if plan.super_r > 0:
        assert plan.super_r * plan.super_c == 32 and plan.grid % 256 == 0
        idle = plan.grid - plan.tilesM * plan.tilesN
        assert (f"idle{idle}" in r.cell) if idle else ("no-idle" in r.cell)
    else:
        assert plan.grid == plan.tilesM * plan.tilesN


@pytest.mark.parametrize("r", BC.PAIR_ROWS, ids=BC.row_id)
def test_every_pair_row_gets_the_plan_it_names(ops, r):
    plan = ops.gemm_bf16p_pair_plan(r.M0, r.N0, r.M1, r.N1, r.K, r.splitk)
    assert plan is not None and tuple(plan) == tuple(r.plan), (plan, r.plan)
    assert (r.M0, r.N0) != (r.M1, r.N1) and (r.M0 % 128 or r.M1 % 128)
    w = 192 if plan.kind >= 8 else 256
    assert plan.grid == -(-r.M0 // 128) * (r.N0 // w) + -(-r.M1 // 128) * (r.N1 // w)


def test_plan_queries_refuse_what_the_launches_refuse(ops):
    for what, M, N, K, sk, packed in BC.REFUSED:
        if "packed" in what:
            continue                                  # a rule of the launch's arguments, not of the shape
        assert ops.gemm_bf16p_plan(M, N, K, sk, 1, packed) is None, what
    for what, M0, N0, M1, N1, K, sk in BC.PAIR_REFUSED:
        assert ops.gemm_bf16p_pair_plan(M0, N0, M1, N1, K, sk) is None, what
    assert ops.gemm_bf16p_plan(64, 256, 64, 2) is not None and ops.gemm_bf16p_pair_plan(64, 256, 64, 256, 160, 3) is not None
    assert ops.gemm_bf16p_plan(64, 256, 64, 1, 2) is None                      # planes
    assert ops.gemm_bf16p_plan(64, 256, 64, 1, 3).kind == 4                    # bf16x6: reported, not swept here


# ---- coverage: the table reaches exactly the cells the plan can produce -------------------------------------------------------
def test_table_reaches_exactly_the_cells_of_the_plan(ops):
    """closure: a new kernel form, tile order or threshold in bf16p_plan without a row here, or a row whose cell is gone, fails"""
    reachable = set()
    for tm, tn, K, sk in itertools.product(BC.SWEEP_TILES, BC.SWEEP_TILES, BC.SWEEP_K, BC.SWEEP_SPLITK):
        plan = ops.gemm_bf16p_plan(128 * tm, 256 * tn, K, sk)
        if plan is not None:                          # (None: more splits than the one slab of K = 32)
            reachable |= BC.cells_of(BC.Plan(*plan))
    reached = set()
    for r in BC.ROWS:
        if r.variant != "packed":
            reached |= BC.cells_of(r.plan)
    assert reached == reachable, sorted(reached ^ reachable)
    # the packed-output rows: every kernel form, and one super-block order with idle workgroups
    packed = [r.plan for r in BC.ROWS if r.variant == "packed"]
    assert {p.kind for p in packed} == {k for k, _, _ in reachable} == {0, 8, 2, 10, 3}
    assert any("super-idle" in BC.order_classes(p) for p in packed)


def test_pair_table_reaches_exactly_the_cells_of_the_pair_plan(ops):
    reachable = set()
    T = BC.PAIR_SWEEP_TILES
    for a, b, c, d, K, sk in itertools.product(T, T, T, T, BC.PAIR_SWEEP_K, BC.SWEEP_SPLITK):
        plan = ops.gemm_bf16p_pair_plan(128 * a, 256 * b, 128 * c, 256 * d, K, sk)
        if plan is not None:
            reachable.add(BC.pair_cell_of(plan))
    reached = {BC.pair_cell_of(r.plan) for r in BC.PAIR_ROWS}
    assert reached == reachable, sorted(reached ^ reachable)
    # the mixed rows put the row-major problem first in one row and second in another
    mixed = {(r.plan.row_major0, r.plan.row_major1) for r in BC.PAIR_ROWS if r.plan.row_major0 != r.plan.row_major1}
    assert mixed == {(0, 1), (1, 0)}


# ---- rasterisation: the workgroup -> tile map of the two kernel bodies, restated -----------------------------------------
def tile_of(bid, tilesM, tilesN, super_r, super_c, bdirect):
    """gemm_bf16p_body / gemm_bf16p_bd_body: (tm, tn) of workgroup `bid`, None for a workgroup that returns at once"""
    xcd, slot = bid & 7, bid >> 3
    if super_r > 0:
        sb, inside = slot >> 5, slot & 31
        srows, scols = tilesM // super_r, tilesN // super_c
        g = sb * 8 + xcd
        if g >= srows * scols:
            return None
        srow, scol = g % srows, g // srows
        return srow * super_r + inside % super_r, scol * super_c + inside // super_r
    ntiles = tilesM * tilesN
    q, r = ntiles >> 3, ntiles & 7
    tile = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + slot
    if bdirect and super_c == 1:
        return tile // tilesN, tile % tilesN
    return tile % tilesM, tile // tilesM


def _geometries():
    out = {}
    for r in BC.ROWS:
        p = r.plan
        out[(p.tilesM, p.tilesN, p.super_r, p.super_c, p.grid, (p.kind & 7) != 0)] = r.cell
    for r in BC.PAIR_ROWS:                             # each problem of a pair is rasterised on its own
        w = 192 if r.plan.kind >= 8 else 256
        for M, N, rm in ((r.M0, r.N0, r.plan.row_major0), (r.M1, r.N1, r.plan.row_major1)):
            tm, tn = -(-M // 128), N // w
            out[(tm, tn, 0, rm, tm * tn, (r.plan.kind & 7) != 0)] = r.cell
    return sorted(out.items())


@pytest.mark.parametrize("geo,cell", _geometries(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, map(int, v))))
def test_workgroups_map_one_to_one_onto_the_tiles(geo, cell):
    tilesM, tilesN, super_r, super_c, grid, bdirect = geo
    if super_r > 0:
        assert tilesM % super_r == 0 and tilesN % super_c == 0 and bdirect
    tiles = [tile_of(b, tilesM, tilesN, super_r, super_c, bdirect) for b in range(grid)]
    live = [t for t in tiles if t is not None]
    assert len(live) == tilesM * tilesN == len(set(live)), cell
    assert set(live) == set(itertools.product(range(tilesM), range(tilesN))), cell
    assert len(tiles) - len(live) == grid - tilesM * tilesN


def test_tile_orders_are_what_they_are_called():
    """column-major walks tm fastest, row-major tn fastest, and only the B-direct body reads super_c == 1"""
    assert tile_of(0, 2, 8, 0, 0, True) == (0, 0) and tile_of(8, 2, 8, 0, 0, True) == (1, 0) == tile_of(8, 2, 8, 0, 0, False)
    assert tile_of(0, 16, 2, 0, 1, True) == (0, 0) and tile_of(8, 16, 2, 0, 1, True) == (0, 1)
    assert tile_of(8, 16, 2, 0, 0, True) == (1, 0) == tile_of(8, 16, 2, 0, 1, False)


# ---- bf16p_ref -----------------------------------------------------------------------------------------------------------------
SMALL = [r for r in BC.ROWS if r.M * r.N * r.K <= 1 << 31]


@pytest.mark.parametrize("r", BC.ROWS, ids=BC.row_id)
def test_exactness_bound_holds_for_every_row(r):
    """the bound is a function of the shape and the value ranges: K vmax^2 + 8 (bias) + 8 (residual), times M for the column
    sums of the packed rows - checked for all rows without building the big ones"""
    top = (r.K * r.vmax ** 2 + 16) * (r.M if r.variant == "packed" else 1)
    assert top < BR.LIMIT, (r.cell, top)


@pytest.mark.parametrize("r", BC.PAIR_ROWS, ids=BC.row_id)
def test_exactness_bound_holds_for_every_pair_row(r):
    assert r.K * r.vmax ** 2 < BR.LIMIT


@pytest.mark.parametrize("r", SMALL, ids=BC.row_id)
def test_reference_equals_a_float32_matmul_of_the_same_integers(r):
    t = BR.build(r.M, r.N, r.K, r.vmax, BC.seed_of(r))
    assert t["A"].abs().min() >= 1 and t["A"].abs().max() <= r.vmax and torch.equal(t["A"], t["A"].bfloat16().float())
    assert t["W"].abs().min() >= 1 and t["W"].abs().max() <= r.vmax and torch.equal(t["W"], t["W"].bfloat16().float())
    packed = r.variant == "packed"
    ref = BR.reference(t, BR.EPI_ACT, bias=True, res=True, colsum=packed, what=r.cell)
    assert ref["bound"] <= (r.K * r.vmax ** 2 + 16) * (r.M if packed else 1)
    pre32 = t["A"] @ t["W"].t() + t["bias"]
    assert torch.equal(ref["pre"], pre32.double())
    assert torch.equal(ref["C"], (torch.relu(pre32) + t["res"]).double())
    if packed:
        assert torch.equal(ref["colsum"], ref["C"].float().sum(0).double())
    d = BR.reference(t, BR.EPI_DACT, what=r.cell)
    assert torch.equal(d["C"], ((t["A"] @ t["W"].t()) * (t["aux"] > 0)).double())
    assert torch.equal(BR.reference(t, BR.EPI_DACT, dact=BR.dact_of(ref["pre"]))["C"], d["pre"] * (ref["pre"] > 0))


def test_reference_refuses_operands_beyond_the_bound():
    t = BR.build(4, 256, 32, 4, 1)
    t["A"] = t["A"] * 65536.0
    with pytest.raises(AssertionError, match="2\\^24"):
        BR.reference(t)


@pytest.mark.parametrize("R,K", [(32, 16), (64, 48), (96, 256)])
def test_pack_helpers_round_trip(R, K):
    x = BR.term(R, K, 3) * 37.0                         # integers up to 296: some round in bf16
    pk = BR.pack_rows(x)
    assert pk.dtype == torch.bfloat16 and pk.numel() == R * K
    assert torch.equal(BR.unpack_rows(pk, R, K), x.bfloat16().float())
    # chunk l of block (rt, kb) = (row l & 31, k 8 (l >> 5) .. + 7): include/dpot_hip.h
    rt, kb, l = R // 32 - 1, K // 16 - 1, 37
    chunk = pk.view(R // 32, K // 16, 64, 8)[rt, kb, l].float()
    assert torch.equal(chunk, x.bfloat16().float()[32 * rt + (l & 31), 16 * kb + 8 * (l >> 5):16 * kb + 8 * (l >> 5) + 8])
    if K % 32 == 0:
        pf = BR.pack_frag(x)
        assert torch.equal(BR.unpack_frag(pf, R, K), x.bfloat16().float())
        # lane l = (column l & 31, kh = l >> 5); element j of half s: row (j & 3) + 4 kh + 8 (j >> 2) + 16 s
        lane, s, j = 45, 1, 6
        got = pf.view(R // 32, K // 32, 2, 64, 8)[0, 1, s, lane, j].float()
        assert got == x.bfloat16().float()[(j & 3) + 4 * (lane >> 5) + 8 * (j >> 2) + 16 * s, 32 + (lane & 31)]


def test_first_difference_names_row_col_and_tile():
    ref = torch.zeros(300, 512)
    got = ref.clone()
    assert BR.first_difference(got, ref) is None
    got[200, 300] = 1.0
    msg = BR.first_difference(got, ref)
    assert "(200, 300)" in msg and "(tm, tn) = (1, 1)" in msg
    got[200, 300] = float("nan")
    assert "(200, 300)" in BR.first_difference(got, ref)
