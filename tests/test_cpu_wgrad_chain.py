"""Chained token ranges of the batched weight gradients (csrc/gemm_tn.hip: tn_chain_node, tn_sum_nodes), host side.

A chain c in {1, 2, 4} gives a workgroup a node of up to c consecutive token ranges; the kernel adds the ranges' tiles in
registers and the finalising launch adds the nodes.  Both are restated here from their definitions and the resulting
expression tree is compared with the tree the library has always added `splits` partials in
    per full group of eight  ((0+1)+(2+3))+((4+5)+(6+7)),  the ranges behind it in pairs,  a last odd range alone,
    v = 0;  v += group, ...;  v += pair, ...;  v += single
as nested tuples (structure) and on random float32 partials (bits).  The node list comes from the library
(dpot_tn_chain_nodes); plus the agreement of header, ctypes table and exported symbols for the new entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_INT = ("dpot_tn_chain_count", "dpot_tn_chain_nodes", "dpot_mlp_wgrad_batch_chain", "dpot_afno_wgrad_batch_chain",
           "dpot_mlp_wgrad_batch", "dpot_afno_wgrad_batch", "dpot_wgrad_batch_finalize")
NEW_I64 = ("dpot_mlp_wgrad_chain_ws_elems", "dpot_afno_wgrad_chain_ws_elems")
SPLITS = range(1, 25)
CHAINS = (1, 2, 4)


@pytest.fixture(scope="module")
def built_lib():
    from dpot_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def ops(built_lib):
    from dpot_amd import _lib, ops as _ops
    _lib.load()
    return _ops


def leaf_tree(leaves, add, zero):
    """tn_sum_nodes at chain 1 (the former tn_sum_splits) over the per-range partials"""
    n, v, s = len(leaves), zero, 0
    while s + 8 <= n:
        a = leaves[s:s + 8]
        v = add(v, add(add(add(a[0], a[1]), add(a[2], a[3])), add(add(a[4], a[5]), add(a[6], a[7]))))
        s += 8
    while s + 2 <= n:
        v = add(v, add(leaves[s], leaves[s + 1]))
        s += 2
    if s < n:
        v = add(v, leaves[s])
    return v


def kernel_node(ranges, add):
    """what a workgroup stores for a node: a single range, a pair (r0 + r1), a quad (r0 + r1) + (r2 + r3)"""
    if len(ranges) == 1:
        return ranges[0]
    if len(ranges) == 2:
        return add(ranges[0], ranges[1])
    assert len(ranges) == 4
    return add(add(ranges[0], ranges[1]), add(ranges[2], ranges[3]))


def node_tree(nodes, splits, chain, add, zero):
    """tn_sum_nodes at chain 2 / 4 over the per-node partials (slot j = node j)"""
    v, s, j = zero, 0, 0
    while s + 8 <= splits:
        if chain == 2:
            v = add(v, add(add(nodes[j], nodes[j + 1]), add(nodes[j + 2], nodes[j + 3])))
            j += 4
        else:
            v = add(v, add(nodes[j], nodes[j + 1]))
            j += 2
        s += 8
    while s < splits:
        v = add(v, nodes[j])
        s += 2
        j += 1
    assert j == len(nodes)
    return v


def chained_tree(leaves, chain, ops, add, zero):
    splits = len(leaves)
    if chain == 1:
        return leaf_tree(leaves, add, zero)
    nodes = [kernel_node(leaves[f:f + c], add) for f, c in ops.tn_chain_nodes(splits, chain)]
    return node_tree(nodes, splits, chain, add, zero)


@pytest.mark.parametrize("chain", CHAINS)
def test_nodes_cover_the_ranges_once_in_order_inside_their_group(ops, chain):
    for splits in SPLITS:
        nodes = ops.tn_chain_nodes(splits, chain)
        assert len(nodes) == ops.tn_chain_count(splits, chain) >= 1
        nxt = 0
        for f, c in nodes:
            assert f == nxt and 1 <= c <= chain, (splits, chain, nodes)
            assert f // 8 == (f + c - 1) // 8, f"node {(f, c)} crosses a group of eight ({splits} ranges)"
            if chain == 1:
                assert c == 1
            elif f >= 8 * (splits // 8):
                assert c <= 2 and f % 2 == 0        # behind the last full group: the tree's pairs, a last odd range
            else:
                assert c == chain and f % chain == 0
            nxt = f + c
        assert nxt == splits
        lengths = [c for _, c in nodes]
        assert lengths == sorted(lengths, reverse=True), "long nodes are dispatched first"
    if chain == 1:
        assert ops.tn_chain_nodes(5, 1) == [(i, 1) for i in range(5)]


def test_bad_arguments_are_refused(ops):
    from dpot_amd import _lib
    lib = _lib.load()
    f, c = C.c_int(0), C.c_int(0)
    assert lib.dpot_tn_chain_count(8, 3) == 0 and lib.dpot_tn_chain_count(0, 2) == 0
    assert lib.dpot_tn_chain_nodes(8, 3, 0, C.byref(f), C.byref(c)) != 0
    assert lib.dpot_tn_chain_nodes(10, 4, 3, C.byref(f), C.byref(c)) != 0       # 10 ranges by 4: nodes 0 .. 2
    assert lib.dpot_tn_chain_nodes(10, 4, 2, C.byref(f), C.byref(c)) == 0 and (f.value, c.value) == (8, 2)


@pytest.mark.parametrize("chain", CHAINS)
def test_same_expression_tree(ops, chain):
    add = lambda a, b: ("+", a, b)
    for splits in SPLITS:
        leaves = [f"r{i}" for i in range(splits)]
        assert chained_tree(leaves, chain, ops, add, "0") == leaf_tree(leaves, add, "0"), (splits, chain)


@pytest.mark.parametrize("chain", CHAINS)
def test_same_bits_on_float32_partials(ops, chain):
    rng = np.random.default_rng(271)
    add = lambda a, b: (a + b).astype(np.float32)
    zero = np.zeros(4096, np.float32)
    for splits in SPLITS:
        # partial sums of different magnitudes and signs: any other association shows in the last bits
        leaves = [(rng.standard_normal(4096) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for _ in range(splits)]
        want = leaf_tree(leaves, add, zero)
        got = chained_tree(leaves, chain, ops, add, zero)
        assert want.dtype == np.float32 and np.array_equal(want.view(np.uint32), got.view(np.uint32)), (splits, chain)
    # the comparison can fail: left-to-right is another sum
    lr = zero
    for x in leaves:
        lr = add(lr, x)
    assert not np.array_equal(lr.view(np.uint32), want.view(np.uint32))


def test_headline_shape(ops):
    """DPOT-Tiny, batch 32: channel MLP split 8 over 128 tiles, AFNO (10, 12) over 32 problems"""
    assert ops.tn_chain_count(8, 4) == 2 and 128 * ops.tn_chain_count(8, 4) == 256
    assert 32 * (2 * ops.tn_chain_count(10, 2) + ops.tn_chain_count(12, 2)) == 512
    assert ops.tn_chain_nodes(10, 4) == [(0, 4), (4, 4), (8, 2)]
    assert ops.tn_chain_nodes(12, 4) == [(0, 4), (4, 4), (8, 2), (10, 2)]
    assert 32 * (2 * ops.tn_chain_count(10, 4) + ops.tn_chain_count(12, 4)) == 320
    assert ops.mlp_wgrad_batch_chain(512, 512, 8, 4) == 4           # the largest chain that leaves a full round of 256
    assert ops.mlp_wgrad_batch_chain(512, 512, 8, 1) == 1           # one block: 32 tiles x 8 ranges is the one round
    assert ops.afno_wgrad_batch_chain(4, 4, 10, 12) in (2, 4)
    assert ops.afno_wgrad_batch_chain(4, 1, 10, 12) == 1
    from dpot_amd import _lib
    lib = _lib.load()
    for c in CHAINS:
        assert lib.dpot_mlp_wgrad_chain_ws_elems(512, 512, 8, c) == lib.dpot_mlp_wgrad2_ws_elems(512, 512, ops.tn_chain_count(8, c))
        assert lib.dpot_afno_wgrad_chain_ws_elems(4, 128, 10, 12, c) == lib.dpot_afno_wgrad2_ws_elems(4, 128, ops.tn_chain_count(12, c))
    # chain 4 is not monotone in the ranges: (6, 8) has 3 nodes for P1 / P2 and 2 for the sum product - the workspace holds 3 slots
    assert ops.tn_chain_count(6, 4) == 3 and ops.tn_chain_count(8, 4) == 2
    assert lib.dpot_afno_wgrad_chain_ws_elems(2, 128, 6, 8, 4) == lib.dpot_afno_wgrad2_ws_elems(2, 128, 3)
    assert lib.dpot_afno_wgrad_chain_ws_elems(3, 128, 13, 16, 4) == lib.dpot_afno_wgrad2_ws_elems(3, 128, 5)
    assert lib.dpot_afno_wgrad_chain_ws_elems(2, 128, 6, 8, 2) == lib.dpot_afno_wgrad2_ws_elems(2, 128, 4)
    with pytest.raises(ValueError):
        with ops.wgrad_chain_scope((3, 1)):
            pass


def _ctype_of(decl: str):
    from dpot_amd import _lib
    decl = " ".join(decl.split())
    if decl.startswith("const float* const*"):
        return C.POINTER(C.c_void_p)
    if decl.startswith("const dpot_wgrad_block*"):
        return C.POINTER(_lib.WgradBlock)
    if decl.startswith("int*"):
        return C.POINTER(_lib.c_i)
    if decl.startswith(("float*", "const float*", "dpot_stream_t")):
        return _lib.c_fp
    if decl.startswith("int "):
        return _lib.c_i
    raise AssertionError(f"unexpected parameter {decl!r}")


def test_chain_symbols_in_header_table_and_library(built_lib):
    from dpot_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dpot_hip.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", built_lib], text=True)
    for name, rtype, res in [(n, "int", _lib.c_i) for n in NEW_INT] + [(n, "int64_t", _lib.c_i64) for n in NEW_I64]:
        m = re.search(r"\b" + rtype + " " + name + r"\(([^)]*)\);", hdr)
        assert m, name
        params = [p for p in m.group(1).split(",") if p.strip() != "void"]
        got_res, args = _lib.SIGNATURES[name]
        assert got_res is res, name
        assert args == [_ctype_of(p) for p in params], name
        assert f" T {name}\n" in exported, name
    names = lambda fn: [re.sub(r".*[ *]", "", " ".join(p.split()))
                        for p in re.search(r"\bint " + fn + r"\(([^)]*)\);", hdr).group(1).split(",")]
    assert names("dpot_mlp_wgrad_batch")[-2:] == ["mlp_chain", "stream"]
    assert names("dpot_afno_wgrad_batch")[-2:] == ["afno_chain", "stream"]
    assert names("dpot_wgrad_batch_finalize")[-3:] == ["mlp_chain", "afno_chain", "stream"]
    assert _lib.load().dpot_version() >= 271
