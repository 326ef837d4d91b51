"""The route selection of the GroupNorm kernels (dpot_groupnorm_kernel_kind), checked without a GPU against the table of
gn_cases.py: every case reaches the route it is written down for, in the table, in the plain-Python restatement and in the
library; the table reaches every route the library has; boundary pairs part; bad arguments are refused; and the inputs of
the GPU test are such that a kernel which drops the last token or the last channel of a slab cannot pass."""
import itertools

import pytest
import torch

import gn_cases as GC
from helpers import assert_close


@pytest.fixture(scope="module")
def built_lib():
    from dpot_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def ops(built_lib):
    from dpot_amd import _lib, ops as _ops
    _lib.load()
    return _ops


def lib_kinds(ops, c):
    ws = c.form != "fb_noc"
    if c.form == "stats":
        return ops.groupnorm_kernel_kind(c.B, c.T, c.E, c.G, "stats", True, GC.aligned_for(c, "stats")), GC.REFUSED
    bwd = "bwd_packs" if c.form == "packs" else "bwd"
    return (ops.groupnorm_kernel_kind(c.B, c.T, c.E, c.G, "fwd", ws, GC.aligned_for(c, "fwd")),
            ops.groupnorm_kernel_kind(c.B, c.T, c.E, c.G, bwd, ws, GC.aligned_for(c, "bwd")))


def test_case_ids_are_unique():
    ids = [GC.case_id(c) for c in GC.CASES]
    assert len(ids) == len(set(ids))
    assert len(GC.FB) + len(GC.STATS) + len(GC.PACKS) == len(GC.CASES)


def test_the_kind_constants_are_the_librarys(ops):
    assert (ops.GN_SCALAR, ops.GN_VEC4, ops.GN_CACHED4, ops.GN_CACHED8, ops.GN_CHUNKED) == \
        (GC.SCALAR, GC.VEC4, GC.CACHED4, GC.CACHED8, GC.CHUNKED)


@pytest.mark.parametrize("c", GC.CASES, ids=GC.case_id)
def test_every_case_reaches_the_route_it_names(ops, c):
    assert GC.expected_kinds(c) == (c.kind_fwd, c.kind_bwd), "table against the restated selection"
    assert lib_kinds(ops, c) == (c.kind_fwd, c.kind_bwd), "table against the library"
    assert ops.groupnorm_chunks(c.B, c.T, c.E, c.G) == GC.gn_chunking(c.B, c.T, c.E, c.G)
    assert ops.groupnorm_bwd_packs_rows(c.B, c.T, c.E, c.G) == GC.gn_packs_rows(c.B, c.T, c.E, c.G)
    tc, chunks = GC.gn_chunking(c.B, c.T, c.E, c.G)
    assert ops.groupnorm_ws_elems(c.B, c.T, c.E, c.G) == c.B * chunks * 2 * c.E
    if chunks:
        assert chunks >= 2 and tc >= 16 and (chunks - 1) * tc < c.T <= chunks * tc       # no empty chunk
    if c.form == "packs":
        assert GC.gn_packs_rows(c.B, c.T, c.E, c.G) == (chunks if c.kind_bwd == GC.CHUNKED else 1)
    assert c.B * c.T * c.E * 4 <= 26 << 20                                              # the tensors stay small


@pytest.mark.parametrize("direction", ["fwd", "bwd", "bwd_packs", "stats"])
def test_table_reaches_exactly_the_librarys_routes(ops, direction):
    """closure: a route added to the library without a case here, or a case for a route that is gone, fails"""
    have = ops.groupnorm_kernel_kinds(direction)
    assert len(have) == len(set(have)) and all(k >= 0 for k in have)
    if direction == "fwd":
        reached = {c.kind_fwd for c in GC.FB}
    elif direction == "bwd":
        reached = {c.kind_bwd for c in GC.FB}
    elif direction == "bwd_packs":
        reached = {c.kind_bwd for c in GC.PACKS}
    else:
        reached = {c.kind_fwd for c in GC.STATS}
    assert reached == set(have), reached ^ set(have)
    assert set(ops.groupnorm_kernel_kinds("fwd")) == {GC.SCALAR, GC.VEC4, GC.CACHED4, GC.CACHED8, GC.CHUNKED}
    assert set(ops.groupnorm_kernel_kinds("bwd_packs")) == {GC.CACHED4, GC.CACHED8, GC.CHUNKED}
    assert ops.groupnorm_kernel_kinds("stats") == (GC.CHUNKED,)
    assert ops.groupnorm_kernel_kinds("sideways") == ()


def test_every_chunked_case_runs_all_three_ways():
    """with the workspace, without it (forward and backward on the one-workgroup kernels), and statistics only"""
    shape = lambda c: (c.B, c.T, c.E, c.G)
    chunked = {shape(c) for c in GC.FB if c.form == "fb" and not c.off and c.kind_fwd == GC.CHUNKED}
    assert chunked <= {shape(c) for c in GC.FB if c.form == "fb_noc"}
    assert chunked == {shape(c) for c in GC.STATS}
    assert len(chunked) >= 8


def test_misaligned_cases_cover_every_operand_on_both_shapes():
    for shape in ((2, 200, 96, 8), (2, 96, 1024, 8)):
        one = [c.off[0] for c in GC.FB if (c.B, c.T, c.E, c.G) == shape and len(c.off) == 1]
        assert sorted(one) == sorted((k, 1) for k in ("x", "dy", "add", "gamma", "beta", "out"))


def test_boundary_pairs_land_on_different_kinds(ops):
    shapes = {(c.B, c.T, c.E, c.G) for c in GC.FB if c.form == "fb" and not c.off}
    for a, b in GC.PAIRS:
        assert a in shapes and b in shapes
        for direction in ("fwd", "bwd"):
            ka, kb = ops.groupnorm_kernel_kind(*a, direction), ops.groupnorm_kernel_kind(*b, direction)
            assert ka >= 0 and kb >= 0 and ka != kb, (a, b, direction)
            assert (ka, kb) == (GC.gn_select(*a, direction), GC.gn_select(*b, direction))


def test_restated_selection_is_the_librarys_on_a_sweep(ops):
    """every shape of a coarse grid around the thresholds, every direction, workspace and alignment"""
    Bs, Ts, Gs = (1, 23, 24), (1, 31, 32, 63, 64, 65, 96, 256, 257, 1024, 2016, 2048, 2049, 4097, 8193), (1, 4, 8)
    cgs = (1, 4, 6, 8, 12, 32, 64, 96, 128, 192, 256, 260, 512, 1024, 1028)
    for B, T, G, cg in itertools.product(Bs, Ts, Gs, cgs):
        E = G * cg
        assert ops.groupnorm_chunks(B, T, E, G) == GC.gn_chunking(B, T, E, G), (B, T, E, G)
        assert ops.groupnorm_bwd_packs_rows(B, T, E, G) == GC.gn_packs_rows(B, T, E, G), (B, T, E, G)
        for d, ws, al in itertools.product(("fwd", "bwd", "bwd_packs", "stats"), (False, True), (False, True)):
            assert ops.groupnorm_kernel_kind(B, T, E, G, d, ws, al) == GC.gn_select(B, T, E, G, d, ws, al), (B, T, E, G, d, ws, al)
        assert ops.groupnorm_stats_supported(B, T, E, G) == (GC.gn_select(B, T, E, G, "stats") == GC.CHUNKED)


def test_refusals(ops):
    for s in GC.STATS_REFUSED:
        assert ops.groupnorm_kernel_kind(*s, "stats") == GC.REFUSED == GC.gn_select(*s, "stats")
        assert not ops.groupnorm_stats_supported(*s)
        assert ops.groupnorm_kernel_kind(*s, "fwd") >= 0
    for s in GC.PACKS_REFUSED:
        assert ops.groupnorm_bwd_packs_rows(*s) == 0 == GC.gn_packs_rows(*s)
        assert ops.groupnorm_kernel_kind(*s, "bwd_packs") == GC.REFUSED == GC.gn_select(*s, "bwd_packs")
        assert ops.groupnorm_kernel_kind(*s, "bwd") >= 0
    for c in GC.PACKS:
        s = (c.B, c.T, c.E, c.G)
        assert ops.groupnorm_kernel_kind(*s, "bwd_packs", True, False) == GC.REFUSED          # a misaligned pointer
        no_ws = ops.groupnorm_kernel_kind(*s, "bwd_packs", False, True)
        assert no_ws == (GC.REFUSED if c.kind_bwd == GC.CHUNKED else c.kind_bwd)             # chunked needs the workspace


def test_bad_arguments_are_refused(ops):
    for d in ("fwd", "bwd", "bwd_packs", "stats"):
        assert ops.groupnorm_kernel_kind(0, 64, 64, 8, d) == -1
        assert ops.groupnorm_kernel_kind(2, 0, 64, 8, d) == -1
        assert ops.groupnorm_kernel_kind(2, 64, 0, 8, d) == -1
        assert ops.groupnorm_kernel_kind(2, 64, 64, 0, d) == -1
        assert ops.groupnorm_kernel_kind(2, 64, 60, 8, d) == -1          # E % G
        assert ops.groupnorm_kernel_kind(65536, 64, 64, 8, d) == -1      # B is a grid dimension
    assert ops.groupnorm_kernel_kind(2, 64, 64, 8, "sideways") == -1
    assert ops.groupnorm_kernel_kind(2, 64, 64, 8, "fwd") == GC.CACHED4
    assert ops.groupnorm_chunks(0, 64, 64, 8) == (0, 0) and ops.groupnorm_chunks(2, 64, 60, 8) == (0, 0)


# ---- the inputs: a dropped tail cannot pass -----------------------------------------------------------------------------
def failing(got, ref, names):
    """the outputs of `names` on which `got` fails helpers.assert_close against `ref` at the GPU test's tolerance"""
    out = []
    for k in names:
        try:
            assert_close(got[k], ref[k], k, **GC.TOL[k])
        except AssertionError:
            out.append(k)
    return out


SHAPES = sorted({(c.B, c.T, c.E, c.G) for c in GC.CASES})


@pytest.mark.parametrize("B,T,E,G", SHAPES, ids=lambda v: str(v))
def test_reference_and_mutants(B, T, E, G):
    """the float64 reference written as slab sums equals torch's group_norm; the reference with the slab's last token, and
    with the group's last channel, left out of the sums fails the GPU test's comparison in both directions"""
    t = GC.inputs(B, T, E, G)
    ref = GC.reference(B, T, E, G)
    ytorch = torch.nn.functional.group_norm(t["x"].double().transpose(1, 2), G, t["gamma"].double(), t["beta"].double(),
                                            GC.EPS).transpose(1, 2)
    assert_close(ref["y"], ytorch, "restated forward", rtol=1e-12, atol_scale=1e-12)
    closed = GC.backward_ref(t, G, drop_token=False, drop_channel=False)
    assert_close(closed["part"][0].sum(0), ref["dgamma"], "per-sample sums against autograd", rtol=1e-10, atol_scale=1e-10)
    fwd, bwd = ("y", "mean", "rstd"), ("dx", "part", "dgamma", "dbeta")
    assert failing(ref, ref, fwd + bwd) == []
    for drop in ({"drop_token": True}, {"drop_channel": True}):
        if "drop_channel" in drop and E // G == 1:
            continue                                     # one channel per group: there is no last channel to lose
        bad_f = failing(GC.forward_ref(t, G, **drop), ref, fwd)
        bad_b = failing(GC.backward_ref(t, G, **drop), ref, bwd)
        assert "mean" in bad_f, (drop, bad_f)
        assert "part" in bad_b and "dbeta" in bad_b, (drop, bad_b)


@pytest.mark.parametrize("recipe", GC.HARD_RECIPES)
def test_hard_inputs_reach_every_forward_route(ops, recipe):
    kinds = set()
    for B, T, E, G, chunked, kind in GC.HARD_SHAPES:
        assert ops.groupnorm_kernel_kind(B, T, E, G, "fwd", chunked) == kind == GC.gn_select(B, T, E, G, "fwd", chunked)
        kinds.add(kind)
        x = GC.hard_input(recipe, B, T, E, G)
        assert x.shape == (B, T, E) and torch.isfinite(x).all()
    assert kinds == set(ops.groupnorm_kernel_kinds("fwd"))
