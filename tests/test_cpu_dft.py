"""The selection of the 2-D DFT kernels (dpot_dft2_kernel_kind), checked without a GPU against the table of dft_cases.py:
every case reaches the kernel it is written down for, the table reaches every kernel that is compiled, every kernel's LDS
slab fits, and the GroupNorm-on-load predicate agrees with the selection."""
import itertools

import pytest

import dft_cases as DC

LDS_BYTES = 160 * 1024                 # per workgroup on gfx950
GENERIC_BUDGET = 150 * 1024 // 4       # floats the generic kernels allow themselves (csrc/common.h LDS_GENERIC_BUDGET)


@pytest.fixture(scope="module")
def built_lib():
    from dpot_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def ops(built_lib):
    from dpot_amd import _lib, ops as _ops
    _lib.load()
    return _ops


def kinds_of(ops, c, norm=False):
    return (ops.dft2_kernel_kind(c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, False, norm),
            ops.dft2_kernel_kind(c.B, c.h, c.w, c.E, c.nb, c.mx, c.my, True, norm))


def generic_floats(c, inverse):
    """(twiddle floats, floats per channel) of the generic kernels' LDS plan"""
    tw = (2 * c.w + 2 * c.h + 3) & ~3
    per_channel = c.mx * c.my * 2 + c.h * c.my * 2 if inverse else c.h * c.w + c.h * c.my * 2
    return tw, per_channel


def generic_cc(c, inverse):
    """the widest power-of-two chunk <= 64 that divides E and fits the budget; 0: not even one channel fits"""
    tw, per_channel = generic_floats(c, inverse)
    for cc in (64, 32, 16, 8, 4, 2, 1):
        if c.E % cc == 0 and per_channel * cc + tw <= GENERIC_BUDGET:
            return cc
    return 0


def test_case_ids_are_unique():
    ids = [DC.case_id(c) for c in DC.CASES]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("c", DC.CASES, ids=DC.case_id)
def test_every_case_reaches_the_kernel_it_names(ops, c):
    assert kinds_of(ops, c) == (c.kind_fwd, c.kind_inv)


@pytest.mark.parametrize("inverse", [False, True])
def test_table_reaches_exactly_the_compiled_kernels(ops, inverse):
    """closure: a kernel added to the library without a case here, or a case for a kernel that is gone, fails"""
    compiled = ops.dft2_kernel_kinds(inverse)
    assert len(compiled) == len(set(compiled)) and all(k >= 0 for k in compiled)
    reached = {(c.kind_inv if inverse else c.kind_fwd) for c in DC.RUNNABLE}
    assert reached == set(compiled), reached ^ set(compiled)
    assert 32032 in ops.dft2_kernel_kinds(False) and 32032 not in ops.dft2_kernel_kinds(True)   # the one asymmetry
    assert 16016 not in compiled


@pytest.mark.parametrize("inverse", [False, True])
def test_every_register_kind_gets_every_mode_set(ops, inverse):
    """full modes, (1, 1), (h/2 + 1, 3) and (3, w/2) for each register kind, in each direction it exists in (128004 keeps at
    most 36 columns: its widest sets are (128, 36) and (3, 36))"""
    for kind in ops.dft2_kernel_kinds(inverse):
        if kind == 0:
            continue
        n = kind // 1000
        want = set(DC.mode_sets(n, n)) if kind != 128004 else {(128, 36), (1, 1), (65, 3), (3, 36)}
        have = {(d.mx, d.my) for d in DC.RUNNABLE if (d.kind_inv if inverse else d.kind_fwd) == kind}
        assert want <= have, (kind, inverse, want - have)


@pytest.mark.parametrize("c", DC.RUNNABLE, ids=DC.case_id)
def test_lds_of_every_kind_fits(c):
    for inverse, kind in ((False, c.kind_fwd), (True, c.kind_inv)):
        n, cc = kind // 1000, kind % 1000
        if kind == 0:
            tw, per_channel = generic_floats(c, inverse)
            cc = generic_cc(c, inverse)
            assert cc >= 1
            nbytes = 4 * (tw + per_channel * cc)
        elif n == 128:
            nbytes = c.my * 128 * 2 * cc * 4
        else:
            assert (c.h, c.w) == (n, n)
            nbytes = (n // 2 + 1) * n * 2 * cc * 4
        assert c.E % cc == 0
        assert nbytes <= LDS_BYTES, (kind, nbytes)


def test_generic_chunk_widths_are_1_8_64():
    got = {generic_cc(c, inv) for c in DC.RUNNABLE if c.kind_fwd == 0 and (c.h, c.w) in DC.GENERIC_GRIDS
           for inv in (False, True)}
    assert got == {1, 8, 64}


@pytest.mark.parametrize("c", DC.REFUSED, ids=DC.case_id)
def test_refused_cases_do_not_fit_lds(ops, c):
    assert generic_cc(c, False) == 0 and generic_cc(c, True) == 0
    assert kinds_of(ops, c) == (-1, -1)


@pytest.mark.parametrize("c", DC.CASES, ids=DC.case_id)
def test_kind_does_not_depend_on_mx(ops, c):
    """the selection reads (h, w, E, nb, my, B); of a refusal only the generic INVERSE's can lift with fewer rows kept (its
    slab holds the mx * my kept modes), so refused cases are held in the forward direction only"""
    for mx in sorted(m for m in {1, 2, c.h // 2, c.h // 2 + 1, c.h - 1, c.h} if 1 <= m <= c.h):
        d = c._replace(mx=mx)
        kf, ki = kinds_of(ops, d)
        assert kf == c.kind_fwd, mx
        if c.kind_inv >= 0:
            assert ki == c.kind_inv, mx


def test_norm_supported_is_the_selection_with_norm(ops):
    sizes, widths = (8, 16, 24, 32, 48, 64, 96, 128), (8, 16, 24, 32, 96, 512)
    for h, w, E in itertools.product(sizes, sizes, widths):
        for B, inverse in itertools.product((1, 64, 1024), (False, True)):
            kind = ops.dft2_kernel_kind(B, h, w, E, 1, h, w // 2 + 1, inverse, True)
            assert ops.rfft2_norm_supported(h, w, E) == (kind > 0), (h, w, E, B, inverse, kind)
            assert kind > 0 or kind == -1                      # never the generic kernel: it has no norm form
            if kind > 0:
                assert kind == ops.dft2_kernel_kind(B, h, w, E, 1, h, w // 2 + 1, inverse, False)


def test_norm_case_tables(ops):
    for c, G in DC.NORM_CASES:
        assert kinds_of(ops, c, norm=True) == (c.kind_fwd, c.kind_inv) == kinds_of(ops, c)
        assert c.E % G == 0 and (c.E // G) % 4 == 0
    reached = {c.kind_fwd for c, _ in DC.NORM_CASES} | {c.kind_inv for c, _ in DC.NORM_CASES}
    assert reached == {k for k in ops.dft2_kernel_kinds(False) if k // 1000 in (8, 16, 32, 64)}
    for c, G in DC.NORM_REFUSED:
        assert kinds_of(ops, c, norm=True) == (-1, -1)
        assert kinds_of(ops, c) == (c.kind_fwd, c.kind_inv)
        assert not ops.rfft2_norm_supported(c.h, c.w, c.E)


def test_bad_arguments_are_refused(ops):
    assert ops.dft2_kernel_kind(2, 16, 16, 32, 3, 16, 9) == -1       # E % nb
    assert ops.dft2_kernel_kind(2, 16, 16, 32, 1, 17, 9) == -1       # mx > h
    assert ops.dft2_kernel_kind(2, 16, 16, 32, 1, 16, 10) == -1      # my > w / 2 + 1
    assert ops.dft2_kernel_kind(0, 16, 16, 32, 1, 16, 9) == -1
