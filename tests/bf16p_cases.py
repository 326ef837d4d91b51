"""The launch-plan table of the bf16 panel GEMM (csrc/gemm_bf16p.hip, planes == 1): one row per cell of bf16p_plan and of the
pair launch's plan - kernel form x tile order x split-K x what is ragged - with the plan the library must select for it.
No GPU, no library call at import: tests/test_cpu_bf16p.py holds every row to the library's own plan query and proves that
the table reaches every cell the plan can produce; tests/test_gpu_bf16p.py runs the rows bit-exactly (tests/bf16p_ref.py).

Kinds: 0 LDS-DMA on 128 x 256 tiles, 8 LDS-DMA on 128 x 192, 2 B-direct with eight waves, 3 B-direct with four waves (two
workgroups per CU), 10 B-direct on 128 x 192.  K = 32 is one slab; the B-direct forms need >= 512 tiles x splits or >= 64
slabs per split (K >= 2048; the pair launch: >= 128 slabs per split, K >= 4096).

Variants (what a row launches):
  full    the small rows: bias + relu with the pre-activation saved, bias + residual, relu'(aux)
  relu    one epilogue only (rows that write 30-76 MB of fp32): bias + relu
  res     one epilogue only: bias + residual
  packed  M % 32 == 0, no split: the packed outputs - row pack, transposed pack, column sums, act' pack out (direct
          epilogue), act' pack in with store=False (direct), and both with a saved pre-activation / residual / aux (the staged
          epilogue epi_fragment_pack).  Both epilogues take any activation (relu here: exact), so no Gaussian cell is needed.
"""
from typing import NamedTuple, Optional, Tuple


class Plan(NamedTuple):          # the fields of dpot_gemm_bf16p_plan, in its order
    kind: int
    tilesM: int
    tilesN: int
    splits: int
    slabs_per_split: int
    super_r: int
    super_c: int
    grid: int


class Row(NamedTuple):
    cell: str
    M: int
    N: int
    K: int
    splitk: Optional[int]        # None: the library's choice (dpot_gemm_bf16p_splitk)
    plan: Plan
    variant: str
    vmax: int = 4                # A and W hold integers of {-vmax..-1, 1..vmax}


class PairPlan(NamedTuple):      # the fields of dpot_gemm_bf16p_pair_plan, in its order
    kind: int
    splits: int
    slabs_per_split: int
    row_major0: int
    row_major1: int
    grid: int


class PairRow(NamedTuple):
    cell: str
    M0: int
    N0: int
    M1: int
    N1: int
    K: int
    splitk: int
    plan: PairPlan
    vmax: int = 4


def _r(cell, M, N, K, splitk, plan, variant, vmax=4):
    return Row(cell, M, N, K, splitk, Plan(*plan), variant, vmax)


ROWS = [
    # ---- LDS-DMA ---------------------------------------------------------------------------------------------------------
    _r("lds256/col/one-tile/M=1", 1, 256, 32, 1, (0, 1, 1, 1, 1, 0, 0, 1), "full"),
    _r("lds256/col/tiles%8!=0/ragged-M", 2300, 3072, 32, 1, (0, 18, 12, 1, 1, 0, 0, 216), "full"),
    _r("lds192/col/M=1", 1, 768, 32, 1, (8, 1, 4, 1, 1, 0, 0, 4), "full"),
    _r("lds192/col/two-rounds", 16384, 768, 32, 1, (8, 128, 4, 1, 1, 0, 0, 512), "relu"),
    _r("lds256/col/split4/ragged-last-split:33,33,33,30", 256, 256, 4128, 4, (0, 2, 1, 4, 33, 0, 0, 2), "full"),
    _r("lds192/col/auto-split8", 256, 1536, 4096, None, (8, 2, 8, 8, 16, 0, 0, 16), "full"),
    # ---- B-direct, eight waves ---------------------------------------------------------------------------------------------
    _r("bd8/row/one-tile/ragged-M", 100, 256, 2048, 1, (2, 1, 1, 1, 64, 0, 1, 1), "full"),
    _r("bd8/row/3-tiles/ragged-M", 300, 256, 2048, 1, (2, 3, 1, 1, 64, 0, 1, 3), "full"),
    _r("bd8/col/21-tiles/ragged-M", 300, 1792, 2048, 1, (2, 3, 7, 1, 64, 0, 0, 21), "full"),
    _r("bd8/row/split2/ragged-last-split:65,64/ragged-M", 300, 256, 4128, 2, (2, 3, 1, 2, 65, 0, 1, 3), "full"),
    _r("bd8/col/split2/ragged-last-split:65,64/ragged-M", 100, 1792, 4128, 2, (2, 1, 7, 2, 65, 0, 0, 7), "full"),
    _r("bd8/super8x4/no-idle/ragged-M", 1000, 8192, 2048, 1, (2, 8, 32, 1, 64, 8, 4, 256), "relu"),
    _r("bd8/super4x8/idle224/ragged-M", 1500, 6144, 2048, 1, (2, 12, 24, 1, 64, 4, 8, 512), "res"),
    _r("bd8/super16x2/idle224/ragged-M", 2000, 4608, 2048, 1, (2, 16, 18, 1, 64, 16, 2, 512), "relu"),
    _r("bd8/super2x16/idle224/ragged-M", 2200, 4096, 2048, 1, (2, 18, 16, 1, 64, 2, 16, 512), "res"),
    _r("bd8/super32x1/idle224/ragged-M", 4000, 2304, 2048, 1, (2, 32, 9, 1, 64, 32, 1, 512), "relu"),
    _r("bd8/super1x32/idle224/ragged-M", 1100, 8192, 2048, 1, (2, 9, 32, 1, 64, 1, 32, 512), "res"),
    # ---- B-direct on 192-wide tiles ----------------------------------------------------------------------------------------
    _r("bd192/row/ragged-M", 100, 768, 2048, 1, (10, 1, 4, 1, 64, 0, 1, 4), "full"),
    _r("bd192/col/28-tiles", 896, 768, 2048, 1, (10, 7, 4, 1, 64, 0, 0, 28), "full"),
    _r("bd192/row/split2/ragged-last-split:65,64/ragged-M", 100, 768, 4128, 2, (10, 1, 4, 2, 65, 0, 1, 4), "full"),
    _r("bd192/col/split2/ragged-last-split:65,64/ragged-M", 100, 1536, 4128, 2, (10, 1, 8, 2, 65, 0, 0, 8), "full"),
    # ---- B-direct, four waves ----------------------------------------------------------------------------------------------
    _r("bd4/col/513-tiles/ragged-M", 3400, 4864, 32, 1, (3, 27, 19, 1, 1, 0, 0, 513), "relu"),
    _r("bd4/row/516-tiles/ragged-M", 16400, 1024, 32, 1, (3, 129, 4, 1, 1, 0, 1, 516), "res"),
    _r("bd4/super8x4/no-idle/ragged-M", 2000, 8192, 32, 1, (3, 16, 32, 1, 1, 8, 4, 512), "relu"),
    _r("bd4/super4x8/idle192/ragged-M", 1500, 12288, 32, 1, (3, 12, 48, 1, 1, 4, 8, 768), "res"),
    _r("bd4/super16x2/idle192", 12288, 1536, 32, 1, (3, 96, 6, 1, 1, 16, 2, 768), "relu"),
    _r("bd4/super2x16/idle224/ragged-M", 4300, 4096, 32, 1, (3, 34, 16, 1, 1, 2, 16, 768), "res"),
    _r("bd4/super32x1/idle224/ragged-M", 69600, 256, 32, 1, (3, 544, 1, 1, 1, 32, 1, 768), "relu"),
    _r("bd4/super1x32/idle224/ragged-M", 2100, 8192, 32, 1, (3, 17, 32, 1, 1, 1, 32, 768), "res"),
    _r("bd4/col/split3/ragged-M", 4000, 4096, 96, 3, (3, 32, 16, 3, 1, 0, 0, 512), "full"),
    _r("bd4/row/split3/ragged-M", 3684, 1536, 96, 3, (3, 29, 6, 3, 1, 0, 1, 174), "full"),
    # ---- packed outputs: one per kernel form and one super-block order with idle workgroups (M % 32 == 0, M % 128 != 0) -----
    _r("packed/lds256/col", 2272, 3072, 32, 1, (0, 18, 12, 1, 1, 0, 0, 216), "packed"),
    _r("packed/lds192/col", 32, 768, 32, 1, (8, 1, 4, 1, 1, 0, 0, 4), "packed"),
    _r("packed/bd8/col", 288, 1792, 2048, 1, (2, 3, 7, 1, 64, 0, 0, 21), "packed"),
    _r("packed/bd192/col", 864, 768, 2048, 1, (10, 7, 4, 1, 64, 0, 0, 28), "packed", 2),
    _r("packed/bd4/col/513-tiles", 3360, 4864, 32, 1, (3, 27, 19, 1, 1, 0, 0, 513), "packed"),
    _r("packed/bd4/super2x16/idle224", 4320, 4096, 32, 1, (3, 34, 16, 1, 1, 2, 16, 768), "packed"),
]


def _p(cell, M0, N0, M1, N1, K, splitk, plan, vmax=4):
    return PairRow(cell, M0, N0, M1, N1, K, splitk, PairPlan(*plan), vmax)


# the two problems of a row are unequal and at least one M is ragged: a tile of problem 1 indexed as problem 0 shows
PAIR_ROWS = [
    _p("pair/lds256", 100, 256, 300, 512, 32, 1, (0, 1, 1, 0, 0, 7)),
    _p("pair/lds192", 100, 768, 300, 1536, 32, 1, (8, 1, 1, 0, 0, 28)),
    _p("pair/lds256/split6/uneven-last-split:7x5,2", 100, 256, 300, 512, 37 * 32, 6, (0, 6, 7, 0, 0, 7)),
    _p("pair/bd8/col+col", 100, 1792, 200, 1024, 4096, 1, (2, 1, 128, 0, 0, 15)),
    _p("pair/bd8/row+col", 100, 256, 70, 1792, 4096, 1, (2, 1, 128, 1, 0, 8)),
    _p("pair/bd8/row+row", 100, 256, 200, 256, 4096, 1, (2, 1, 128, 1, 1, 3)),
    _p("pair/bd8/col+col/split2:129,128", 100, 1792, 200, 1024, 8192 + 32, 2, (2, 2, 129, 0, 0, 15)),
    _p("pair/bd8/col+row/split2:129,128", 100, 1792, 70, 256, 8192 + 32, 2, (2, 2, 129, 0, 1, 8)),
    _p("pair/bd8/row+row/split2:129,128", 100, 512, 70, 256, 8192 + 32, 2, (2, 2, 129, 1, 1, 3)),
    _p("pair/bd192/col+col", 100, 1536, 200, 768, 4096, 1, (10, 1, 128, 0, 0, 16)),
    _p("pair/bd192/row+col", 100, 768, 200, 768, 4096, 1, (10, 1, 128, 1, 0, 12)),
    _p("pair/bd192/row+row", 100, 768, 2000, 768, 4096, 1, (10, 1, 128, 1, 1, 68)),
    _p("pair/bd4/col+col/256+256-tiles", 1000, 8192, 2000, 4096, 32, 1, (3, 1, 1, 0, 0, 512)),
    _p("pair/bd4/col+row/256+256-tiles", 1000, 8192, 4000, 2048, 32, 1, (3, 1, 1, 0, 1, 512)),
    _p("pair/bd4/row+row/256+256-tiles", 4000, 2048, 8100, 1024, 32, 1, (3, 1, 1, 1, 1, 512)),
    _p("pair/bd4/col+col/split3", 300, 2304, 700, 6144, 96, 3, (3, 3, 1, 0, 0, 171)),
    _p("pair/bd4/col+row/split3", 300, 2304, 3000, 1536, 96, 3, (3, 3, 1, 0, 1, 171)),
    _p("pair/bd4/row+row/split3", 100, 768, 3000, 1792, 96, 3, (3, 3, 1, 1, 1, 171)),
]

# what the launches must refuse (the DPOT_REQUIREs of dpot_gemm_bf16p / dpot_gemm_bf16p_pair): (what, M, N, K, splitk, packed)
REFUSED = [
    ("N % 256 != 0", 64, 128, 32, 1, False),
    ("N % 256 != 0 (a multiple of 192)", 64, 192, 32, 1, False),
    ("K % 32 != 0", 64, 256, 48, 1, False),
    ("K < 32", 64, 256, 16, 1, False),
    ("split-K with packed outputs", 64, 256, 128, 2, True),
    ("splitk > slabs", 64, 256, 64, 3, False),
]
# (what, M0, N0, M1, N1, K, splitk)
PAIR_REFUSED = [
    ("pair: N % 256 != 0", 64, 256, 64, 128, 32, 1),
    ("pair: K % 32 != 0", 64, 256, 64, 256, 48, 1),
    ("pair: splitk > slabs", 64, 256, 64, 256, 64, 3),
    ("pair: an empty split (5 slabs in 4 splits of 2)", 64, 256, 64, 256, 160, 4),
]

# the coarse grid of the coverage proof (tests/test_cpu_bf16p.py)
SWEEP_TILES = tuple(range(1, 41)) + (96, 128, 512, 544)
SWEEP_K = (32, 2048, 4128)
SWEEP_SPLITK = (1, 2, 3)
PAIR_SWEEP_TILES = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 40, 96, 128)
PAIR_SWEEP_K = (32, 2048, 4128, 8192 + 32)


def order_classes(plan: Plan) -> Tuple[str, ...]:
    """the tile-order classes a plan is an instance of: column-major, row-major, its super-block shape, and - for a
    super-block grid padded beyond the tiles - the class of idle workgroups"""
    if plan.super_r > 0:
        out = (f"super{plan.super_r}x{plan.super_c}",)
        return out + (("super-idle",) if plan.grid > plan.tilesM * plan.tilesN else ())
    return ("row",) if plan.super_c == 1 else ("col",)


def cells_of(plan: Plan):
    return {(plan.kind, c, plan.splits > 1) for c in order_classes(plan)}


def pair_cell_of(plan: PairPlan):
    """(kind, how many of the two problems run in row-major order, split?)"""
    return (plan.kind, plan.row_major0 + plan.row_major1, plan.splits > 1)


def row_id(r):
    return r.cell


_SEEDS = {r.cell: 9000 + 10 * i for i, r in enumerate(ROWS + PAIR_ROWS)}


def seed_of(r):
    """a fixed seed per row (its position in the table)"""
    return _SEEDS[r.cell]
