"""The kernel selection of the AFNO mixer (dpot_afno_mlp2_plan), checked without a GPU against the table of afno_mixer_cases.py:
every case reaches the instantiation it is written down for, in the table, in the plain-Python restatement and in the library;
the table reaches every instantiation the library has and no other; the restated cost rule is the library's on a sweep that
holds the model shapes; the integer inputs of the GPU test keep every partial sum exact in fp32; and ops.afno_mlp2 refuses the
views its kernels cannot express before anything is launched."""
import pytest
import torch

import afno_mixer_cases as MC


@pytest.fixture(scope="module")
def built_lib():
    from dpot_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def ops(built_lib):
    from dpot_amd import _lib, ops as _ops
    _lib.load()
    return _ops


def lib_plan(ops, M, nb, bs, layout, act):
    p = ops.afno_mlp2_plan(M, nb, bs, layout, MC.ACT_IDS[act])
    return (p.form, p.rt, p.panels, p.waves, p.gelu)


def test_case_ids_are_unique():
    for table in (MC.INT, MC.REAL, MC.REPEAT):
        ids = [MC.case_id(c) for c in table]
        assert len(ids) == len(set(ids))


def test_the_constants_are_the_librarys(ops):
    assert (ops.AFNO_FOUR, ops.AFNO_THREE, ops.AFNO_THREE_SPLIT, ops.AFNO_REFUSED) == (MC.FOUR, MC.THREE, MC.SPLIT, MC.REFUSED)
    assert all(ops.ACT_IDS[k] == v for k, v in MC.ACT_IDS.items())


@pytest.mark.parametrize("c", MC.CASES, ids=[f"{n}-{MC.case_id(c)}" for n, t in (("int", MC.INT), ("real", MC.REAL),
                                                                                ("repeat", MC.REPEAT)) for c in t])
def test_every_case_reaches_the_instantiation_it_names(ops, c):
    want = MC.plan(c.M, c.nb, c.bs, c.layout, c.act)
    assert want[:2] == (c.want_form, c.want_rt), "table against the restated selection"
    assert lib_plan(ops, c.M, c.nb, c.bs, c.layout, c.act) == want, "restated selection against the library"
    N = 2 * c.bs
    assert c.M * (c.nb * N + max(c.ldx_pad, c.ldo_pad)) * 4 <= 21 << 20                  # about 20 MB per tensor
    assert 4 * c.M * c.nb * N * N <= 5.5e9                                              # about 5 GFLOP of float64 reference
    assert set(c.outputs) <= {"pre", "mid"} and c.ldx_pad % 4 == 0 and c.ldo_pad % 4 == 0


def test_cross_cases_reach_rt_2_and_4_in_both_forms(ops):
    for nb, bs, M, rt in MC.CROSS:
        assert lib_plan(ops, M, nb, bs, 1, "gelu")[:2] == (MC.SPLIT if bs == 96 else MC.THREE, rt)
        assert lib_plan(ops, M, nb, bs, 0, "gelu")[:2] == (MC.FOUR, rt)
    assert {(bs, rt) for _, bs, _, rt in MC.CROSS} == {(bs, rt) for bs in (64, 96, 128) for rt in (2, 4)}


def test_table_reaches_exactly_the_librarys_instantiations(ops):
    """closure: an instantiation added to the library without a case here, or a case for one that is gone, fails; and each one
    is launched in both directions with the product's own output combination"""
    have = ops.afno_mlp2_plans()
    assert len(have) == len(set(have)) == 70
    assert {MC.key(c) for c in MC.INT} == set(have), {MC.key(c) for c in MC.INT} ^ set(have)
    fwd = {MC.key(c) for c in MC.INT if c.mode == 0 and c.outputs == ("pre",)}
    bwd = {MC.key(c) for c in MC.INT if c.mode == 1 and c.outputs == ("mid",)}
    assert fwd == set(have) and bwd == set(have)
    # the enumeration is what the plan can return: four widths x five RT x {gelu, switch} and the three-product widths, bs = 96
    # split from RT 2 on and never split at RT 1
    want = {(MC.form_of(bs, layout, rt), bs, rt, g) for layout in (0, 1) for bs in (32, 64, 96, 128) for rt in range(1, 6)
            for g in (True, False) if MC.form_of(bs, layout, rt) != MC.REFUSED}
    assert set(have) == want
    assert not any(f == MC.THREE and bs == 96 and rt > 1 for f, bs, rt, _ in have)


def test_edges_and_combinations_are_in_the_table():
    groups = {}
    for c in MC.INT:
        groups.setdefault((c.want_form, c.bs), []).append(c)
    assert len(groups) == 8
    for (form, bs), cs in groups.items():
        combos = {(c.mode, frozenset(c.outputs)) for c in cs}
        assert combos >= {(0, frozenset()), (0, frozenset({"pre"})), (0, frozenset({"pre", "mid"})), (1, frozenset({"mid"})),
                          (1, frozenset({"mid", "pre"}))}, (form, bs)
        assert {c.mode for c in cs if (c.ldx_pad, c.ldo_pad) == (4, 8)} == {0, 1}, (form, bs)
        for rt in {c.want_rt for c in cs}:
            R = 16 * rt
            last = {(c.M - 1) % R + 1 for c in cs if c.want_rt == rt}
            assert last >= {1, R - 1, R}, (form, bs, rt, last)
            if rt > 1:
                assert 16 in last, (form, bs, rt)
    for form in (MC.FOUR, MC.THREE):
        ms = {c.M for c in MC.INT if c.want_form == form}
        assert 1 in ms and any(1 < m < 16 for m in ms)
    for form in (MC.FOUR, MC.THREE, MC.SPLIT):
        rem = {(c.nb * MC.plan(c.M, c.nb, c.bs, c.layout, c.act)[2]) % 8 for c in MC.INT if c.want_form == form and c.nb % 2}
        assert rem >= {0, 1, 7}, (form, rem)
    for rt in (2, 3, 4, 5):                                   # split: M ends inside tile RA - 1, between, inside tile RA
        ra = (rt + 1) // 2
        last = {(c.M - 1) % (16 * rt) + 1 for c in MC.INT if c.want_form == MC.SPLIT and c.want_rt == rt}
        assert any(16 * (ra - 1) < v < 16 * ra for v in last) and 16 * ra in last and any(16 * ra < v < 16 * (ra + 1) for v in last), \
            (rt, sorted(last))


def test_real_cases_cover_each_form_and_width_at_its_extreme_row_tiles():
    seen = {(c.want_form, c.bs, c.want_rt, c.act) for c in MC.REAL}
    for act in ("gelu", "silu"):
        for bs in (32, 64, 96, 128):
            assert {(MC.FOUR, bs, rt, act) for rt in (1, 3, 5)} <= seen
        for bs in (64, 128):
            assert {(MC.THREE, bs, rt, act) for rt in (1, 3, 5)} <= seen
        assert {(MC.THREE, 96, 1, act), (MC.SPLIT, 96, 2, act), (MC.SPLIT, 96, 5, act)} <= seen
    assert {(c.want_form) for c in MC.REPEAT} == {MC.FOUR, MC.THREE, MC.SPLIT}


def test_restated_cost_rule_is_the_librarys_on_a_sweep(ops):
    """the model shapes (DPOT-Tiny / S / M: 16 x 9 modes, nb 4 or 8, B = 1 .. 32; DPOT-L: 32 x 17 modes, nb 16, B = 1 .. 16) and a
    grid of rows x blocks around every threshold of the rule"""
    shapes = [(B * 16 * 9, nb, 128) for B in range(1, 33) for nb in (4, 8)]
    shapes += [(B * 32 * 17, 16, 96) for B in range(1, 17)]
    Ms = sorted(set(list(range(1, 340)) + [m + d for m in range(352, 2300, 16) for d in (-1, 0, 1)] + [4608, 8704, 18432, 100000]))
    shapes += [(M, nb, bs) for M in Ms for nb, bs in ((1, 128), (3, 32), (4, 128), (5, 64), (8, 128), (9, 96), (16, 96), (33, 64),
                                                     (64, 96), (65, 128), (96, 32), (300, 64))]
    rts = set()
    for M, nb, bs in shapes:
        for layout in (0, 1):
            want = MC.plan(M, nb, bs, layout, "gelu")
            assert lib_plan(ops, M, nb, bs, layout, "gelu") == want, (M, nb, bs, layout)
            rts.add(want[1])
    assert rts >= {1, 2, 3, 4, 5}
    # what the issue names: 1088 rows select RT 2 on 4 blocks and RT 5 on 16
    assert MC.pick_rt(1088, 4) == 2 and MC.pick_rt(1088, 16) == 5


def test_plan_refuses_what_the_launcher_refuses(ops):
    for M, nb, bs, layout in [(0, 4, 128, 0), (-1, 4, 128, 1), (16, 0, 128, 0), (16, 4, 48, 0), (16, 4, 32, 1), (16, 4, 256, 0),
                              (16, 4, 128, 2), (16, 4, 128, -1)]:
        assert lib_plan(ops, M, nb, bs, layout, "gelu") == (MC.REFUSED, 0, 0, 0, False) == MC.plan(M, nb, bs, layout, "gelu")
    assert lib_plan(ops, 16, 4, 128, 0, "relu")[4] is False and lib_plan(ops, 16, 4, 128, 0, "gelu")[4] is True


@pytest.mark.parametrize("c", MC.INT, ids=MC.case_id)
def test_integer_inputs_keep_every_partial_sum_exact(c):
    """a condition of the zero-tolerance comparison, not a measurement: below 2^24 every integer is an fp32 number"""
    t = MC.int_inputs(c)
    for k in ("X", "w1", "w2", "b1", "b2"):
        assert torch.equal(t[k], t[k].round())
    assert torch.equal(t["aux"] * 2, (t["aux"] * 2).round()) and bool((t["aux"] != t["aux"].round()).all())
    l1, l2 = MC.partial_sum_bounds(c, t)
    assert l1 < 2 ** 24 and l2 < 2 ** 24, (l1, l2)
    assert c.act in ("relu", "none", "gelu")                 # gelu: only layer 1 (`pre`) is held to zero tolerance


def test_partial_sum_bound_really_bounds():
    """the bound against the sums themselves on one small case of each form (float64, absolute values)"""
    for c in (MC.INT[0], next(c for c in MC.INT if c.layout == 1 and c.mode == 1 and c.M < 40)):
        t = MC.int_inputs(c)
        l1, l2 = MC.partial_sum_bounds(c, t)
        ta = {k: v.abs() for k, v in t.items()}
        ref = MC.forward_ref(ta, "none") if c.mode == 0 else MC.backward_ref(ta, "none", ta["X"], ta["aux"])
        # with |.| operands [[|Wr|, |Wi|], [|Wi|, |Wr|]] every entry is a full absolute sum (wbig's -Wi block apart)
        assert ref["mid"].abs().max().item() <= l1 and ref["Y"].abs().max().item() <= l2


# ---- ops.afno_mlp2: views ---------------------------------------------------------------------------------------------------
def _call(ops, X, **kw):
    nb, bs = 2, 32
    w = torch.zeros(nb, 64, 64)
    return ops.afno_mlp2(X, w, None, w, None, nb, bs, 1, **kw)


def test_wrapper_refuses_views_the_kernel_cannot_express(ops):
    M, cols = 8, 128
    base = torch.zeros(M, 2 * cols + 8)
    ok = torch.zeros(M, cols)
    with pytest.raises(ValueError, match="inner stride"):
        _call(ops, base[:, :2 * cols:2])
    with pytest.raises(ValueError, match="row stride"):
        _call(ops, torch.zeros(M, cols + 2)[:, :cols])                         # ld = 130: no multiple of 4
    with pytest.raises(ValueError, match="16-byte"):
        _call(ops, torch.zeros(M * (cols + 4) + 4)[1:].as_strided((M, cols), (cols + 4, 1)))   # one float off
    with pytest.raises(ValueError, match="must be float32"):
        _call(ops, ok.double())
    with pytest.raises(ValueError, match="must be float32"):
        _call(ops, torch.zeros(M, cols - 4))                                  # narrower than nb * N
    with pytest.raises(ValueError, match="share one row stride"):
        _call(ops, ok, mode=1, aux=torch.zeros(M, cols + 8)[:, :cols])        # aux stride against fresh outputs
    with pytest.raises(ValueError, match="share one row stride"):
        _call(ops, ok, mode=1, aux=ok, out_Y=torch.zeros(M, cols + 8)[:, :cols])
    with pytest.raises(ValueError, match="share one row stride"):
        _call(ops, ok, out_Y=torch.zeros(M, cols + 8)[:, :cols], out_pre=torch.zeros(M, cols + 4)[:, :cols])
    with pytest.raises(ValueError, match="inner stride"):
        _call(ops, ok, out_Y=base[:, :2 * cols:2])
    with pytest.raises(ValueError, match="16-byte"):
        _call(ops, ok, out_mid=torch.zeros(M * cols + 4)[2:2 + M * cols].view(M, cols))
    with pytest.raises(ValueError, match="must be float32"):
        _call(ops, ok, out_Y=torch.zeros(M + 1, cols))
