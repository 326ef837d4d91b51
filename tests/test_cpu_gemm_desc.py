"""The descriptor table of tests/gemm_desc_ref.py, checked without a GPU: the float64 reference against plain torch
expressions, the conditions the table must meet (exactness bound, labels that tell the truth about alignment and strides,
coverage of every axis value and every listed pair), check() against tampered results, and the host-only behaviour of the
library (descriptor validation before any launch, workspace size, split counts of the weight-gradient kernel)."""
import ctypes as C
import os
import re

import pytest
import torch

import gemm_desc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from dpot_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


# ---- the reference against plain torch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", R.TERM_SETS)
def test_reference_equals_the_plain_torch_expression(terms):
    """tight, aligned layouts: the buffers ARE the matrices, so the epilogue can be written down directly"""
    M, N, K, batch = 20, 8, 12, (3 if terms == "bcast" else 1)        # M: the row map (m / 3) % 5 wraps
    c = R.mk("selftest", M, N, K, layout="NN", terms=terms, batch=batch)
    t = R.build(c, 11)
    ref = R.reference(c, t)
    A = t["A"].double().view(-1, M, K)                       # bcast: one A for every batch
    B = t["B"].double().view(batch, K, N)
    v = A @ B
    if terms in ("bias", "bias+preact", "act", "acc+res+bias"):
        v = v + t["bias"].double().view(batch, 1, N)
    if terms in ("bias+preact", "act"):
        assert torch.equal(ref["preact"], v)
    if terms == "act":
        v = torch.relu(v)
    if terms == "dact":
        aux = t["aux"].double().view(batch, M, N).requires_grad_(True)
        torch.relu(aux).sum().backward()
        v = v * aux.grad
    if terms in ("act", "acc+res+bias"):
        v = v + t["res"].double().view(batch, M, N)
    if terms == "rowres":
        v = v + t["res"].double().view(5, N)[(torch.arange(M) // 3) % 5]
    if terms == "bcast":
        v = v + t["res"].double().view(1, M, N)
    if terms in ("acc", "acc+res+bias"):
        v = v + t["C"].double().view(batch, M, N)
    assert torch.equal(ref["C"], v)
    assert R.term_set(c) == terms


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
def test_reference_layouts_and_column_sums(layout):
    M, N, K = 5, 7, 6
    ta, tb = R.LAYOUTS[layout]
    for of in (0, 1, 2):
        if (of == 1 and not ta) or (of == 2 and tb):
            continue
        c = R.mk("selftest", M, N, K, layout=layout, colsum_of=of)
        t = R.build(c, 12)
        ref = R.reference(c, t)
        A = t["A"].double().view(K, M).t() if ta else t["A"].double().view(M, K)
        B = t["B"].double().view(N, K).t() if tb else t["B"].double().view(K, N)
        assert torch.equal(ref["C"][0], A @ B)
        if of:
            assert torch.equal(ref["colsum"].reshape(-1), (A.sum(1) if of == 1 else B.sum(0)))


def test_reference_gelu_terms_equal_torch():
    for terms in ("act", "dact"):
        c = R.mk("selftest", 6, 8, 10, terms=terms, act="gelu", exact=False)
        t = R.build(c, 13)
        ref = R.reference(c, t)
        v = t["A"].double().view(6, 10) @ t["B"].double().view(10, 8)
        if terms == "act":
            want = torch.nn.functional.gelu(v + t["bias"].double()) + t["res"].double().view(6, 8)
        else:
            aux = t["aux"].double().view(6, 8).requires_grad_(True)
            torch.nn.functional.gelu(aux).sum().backward()
            want = v * aux.grad
        torch.testing.assert_close(ref["C"][0], want, rtol=1e-12, atol=1e-12)


def test_constants_are_the_library_s():
    from dpot_amd import ops
    assert R.PREC == {"f32": ops.GEMM_F32, "bf16x6": ops.GEMM_BF16X6, "bf16": ops.GEMM_BF16}
    assert R.MODE == {"linear": ops.EPI_LINEAR, "act": ops.EPI_ACT, "dact": ops.EPI_DACT}
    assert all(R.ACT[k] == ops.ACT_IDS[k] for k in R.ACT)


# ---- conditions on the table -------------------------------------------------------------------------------------------------
def test_labels_are_unique_and_nothing_is_skipped():
    labels = [c.label for c in R.CASES]
    assert len(set(labels)) == len(labels)
    assert all(type(c) is R.Case for c in R.CASES), "a table entry carries a pytest mark"
    assert 200 <= len(R.CASES) <= 450, "a few hundred launches"
    src = open(os.path.join(ROOT, "tests", "test_gpu_gemm_desc.py")).read()
    assert not re.search(r"skip|xfail", src)
    items = R.items()
    ran = [c.label for cases in items.values() for c in cases]
    assert sorted(ran) == sorted(labels)
    assert {c.family for c in R.CASES} == set(R.FAMILIES)
    assert all(len({c.family for c in cases}) == 1 and len(cases) <= 40 for cases in items.values())


def test_every_integer_case_stays_below_2_to_the_24(monkeypatch):
    for c in R.CASES:
        t = R.build(c, R.seed_of(c))
        R.reference(c, t)                                     # asserts the bound for the integer cases
        if c.exact:
            for name in R.INPUTS:
                if c.has(name):
                    v = t[name][c.opnd[name].index(c.batch)]
                    assert torch.equal(v, v.round()) and float(v.abs().max()) <= 8
                    if name in ("A", "B"):
                        assert float(v.abs().min()) >= 1 and float(v.abs().max()) <= 4
    c = R.CASES[0]
    monkeypatch.setattr(R, "LIMIT", 1.0)
    with pytest.raises(AssertionError, match="2\\^24"):
        R.reference(c, R.build(c, 1))


def _label_tokens(label):
    loader = next(p for p in label.split("/") if p == "vec" or p.startswith("vec-off:"))
    epi = next(p for p in label.split("/") if p in ("evec", "reduce") or p.startswith("evec-off:"))
    return (set(loader[8:].split(",")) if loader != "vec" else set(),
            None if epi == "reduce" else set(epi[9:].split(",")) if epi != "evec" else set())


def test_buffers_have_the_property_the_label_names():
    """from the label alone: why the loader / the tile epilogue is scalar; from the built buffers and the geometry: the truth"""
    for c in R.CASES:
        t = R.build(c, R.seed_of(c))
        for name, o in c.opnd.items():
            assert t[name].numel() == o.off + (c.batch - 1) * o.stride + o.rows * o.ld, (c.label, name)
            assert o.ld >= o.cols and 0 <= o.off <= 3
            idx = o.index(c.batch)
            assert int(idx.max()) == t[name].numel() - 1 - (o.ld - o.cols) and int(idx.min()) == o.off
            sent = torch.ones(t[name].numel(), dtype=torch.bool)
            sent[idx.reshape(-1)] = False
            if name in R.OUTPUTS:
                assert bool(t[name][sent].isnan().all())
                assert bool(t[name][~sent].isnan().all()) != (name == "C" and c.accumulate)
            else:
                assert bool((t[name][sent] == R.IN_SENTINEL).all()) and not bool((t[name][~sent] == R.IN_SENTINEL).any())
        said_l, said_e = _label_tokens(c.label)
        true_l, true_e = set(R.loader_reasons(c)), set(R.epilogue_reasons(c))
        # what the label names is true, and "vec" / "evec" are said of exactly the cases that vectorise
        assert said_l <= true_l and bool(said_l) == bool(true_l), (c.label, true_l)
        if c.splitk > 1:
            assert said_e is None, c.label
        else:
            assert said_e <= true_e and bool(said_e) == bool(true_e), (c.label, true_e)
        if c.only:   # the case would vectorise but for the ONE reason it names
            if c.family == "loader":
                assert said_l == true_l and len(true_l) == 1, (c.label, true_l)
            else:
                assert said_e == true_e and len(true_e) == 1, (c.label, true_e)
        if c.family == "handoff":
            assert R.handoff_eligible(c) == c.eligible, c.label
        kw = R.gemm_kwargs(c)
        assert kw["lda"] == c.opnd["A"].ld and kw["ldc"] == c.opnd["C"].ld and kw["splitk"] == c.splitk
        for name, key in (("aux", "ldaux"), ("preact", "ldpre"), ("res", "ldres")):
            assert not c.has(name) or kw[key] >= c.N


def _need(have, want, what):
    missing = sorted(set(want) - set(have), key=str)
    assert not missing, f"{what}: {len(missing)} cell(s) missing from the table: {missing}"


def test_every_axis_value_and_every_listed_pair_occurs():
    cs = R.CASES
    gen = [c for c in cs if c.family != "handoff"]
    _need({c.M for c in gen}, R.MN_VALUES, "M")
    _need({c.N for c in gen}, R.MN_VALUES, "N")
    _need({c.K for c in gen}, R.K_VALUES, "K")
    for p in R.PRECS:                                       # every M, N, K value under every precision
        _need({c.M for c in gen if c.precision == p}, R.MN_VALUES, f"M under {p}")
        _need({c.N for c in gen if c.precision == p}, R.MN_VALUES, f"N under {p}")
        _need({c.K for c in gen if c.precision == p}, R.K_VALUES, f"K under {p}")
    _need({(c.precision, c.tile, R.loader_is_vec(c)) for c in cs},
          [(p, t, v) for p in R.PRECS for t in (64, 128) for v in (True, False)], "precision x tile x loader")
    _need({(c.precision, c.layout) for c in cs}, [(p, l) for p in R.PRECS for l in R.LAYOUTS], "precision x layout")
    # the 16-byte loader of a K-contiguous operand: one float4 in all, whole slabs, and partial slabs of whole float4s
    _need({(c.precision, c.K) for c in gen if R.loader_is_vec(c) and c.layout != "TN"},
          [(p, k) for p in R.PRECS for k in (4, 32, 36, 68, 100)], "16-byte loader x K")
    _need({(R.epilogue_form(c), R.term_set(c), c.precision) for c in cs if c.exact},
          [(f, t, p) for f in R.FORMS for t in R.TERM_SETS for p in R.PRECS], "epilogue form x term set x precision")
    _need({(c.colsum_of, c.precision, c.splitk > 1) for c in cs},
          [(o, p, s) for o in (1, 2) for p in R.PRECS for s in (False, True)], "colsum_of x precision x split-K")
    _need({(c.colsum_of, c.precision, c.tile, c.splitk > 1) for c in cs if c.family == "colsum"},
          [(o, p, t, s) for o in (1, 2) for p in R.PRECS for t in (64, 128) for s in (False, True)], "colsum x tile")
    _need({c.precision for c in cs if c.tag == 1 and c.layout == "NN"}, R.PRECS, "tag = 1 on NN")
    assert all(c.layout == "NN" for c in cs if c.tag == 1)
    # each reason for a scalar loader on its own, per precision; odd extents against both kinds of staging
    _need({(c.precision,) + c.claim_loader for c in cs if c.only and c.family == "loader"},
          [(p, f"{x}:{w}") for p in R.PRECS for x in "AB" for w in ("base+1", "base+2", "base+3", "ld%4", "stride%4")],
          "scalar-loader reasons")
    _need({(c.precision, c.K, c.layout) for c in cs}, [(p, k, l) for p in R.PRECS for k in (1, 31, 77) for l in ("NT", "TN")],
          "odd K x K-contiguous / row-contiguous operands")
    # each reason for a scalar tile epilogue on its own
    want = ["N%4"] + [f"{x}:{w}" for x in ("C", "aux", "preact", "res") for w in ("base+1", "base+2", "base+3", "ld%4", "stride%4")]
    want += [f"bias:{w}" for w in ("base+1", "base+2", "base+3", "stride%4")]
    _need({c.claim_epi[0] for c in cs if c.only and c.family == "epilogue"}, want, "scalar-epilogue reasons")
    # padded but vectorisable: ld = extent + 4 on every operand, under the tile epilogue and the split-K reduce
    padded = [c for c in cs if all(o.ld == o.cols + 4 for n, o in c.opnd.items() if n not in ("bias", "colsum"))]
    _need({(R.epilogue_form(c), c.precision) for c in padded if R.loader_is_vec(c) or c.family == "epilogue"},
          [(f, p) for f in ("vector", "reduce") for p in R.PRECS], "padded leading dimensions")
    assert any(R.loader_is_vec(c) and R.epilogue_form(c) == "vector" and len(c.opnd) >= 6 for c in padded)
    assert any(c.batch > 1 and any(o.stride > o.rows * o.ld for o in c.opnd.values()) for c in cs), "gaps between batches"
    # split-K
    sk = [c for c in cs if c.family == "splitk"]
    _need({(c.precision, c.splitk, c.K) for c in sk}, [(p, s, k) for p in R.PRECS for s in R.SPLITK_VALUES for k in R.SPLITK_KS],
          "splitk x K")
    _need({(c.precision, c.colsum_of) for c in sk}, [(p, o) for p in R.PRECS for o in (0, 1, 2)], "split-K x column sums")
    _need({(c.precision, c.batch) for c in sk}, [(p, b) for p in R.PRECS for b in (1, 3)], "split-K x batch")
    empty = [c for c in sk if -(-(-(-c.K // 32)) // c.splitk) * (c.splitk - 1) >= -(-c.K // 32)]
    _need({(c.precision, c.colsum_of > 0) for c in empty}, [(p, o) for p in R.PRECS for o in (False, True)], "empty splits")
    # hand-off
    ho = [c for c in cs if c.family == "handoff"]
    assert all(c.precision == "f32" and c.layout == "TN" and c.batch == 1 for c in ho)
    el = [c for c in ho if c.eligible]
    _need({c.M for c in el}, R.HANDOFF_M, "hand-off M")
    _need({c.N for c in el}, R.HANDOFF_N, "hand-off N")
    _need({s for c in el for s in R._slabs(c.K, c.splitk)}, (1, 2, 3, 4, 5), "slabs per split")
    assert any(len(set(R._slabs(c.K, c.splitk))) > 1 for c in el), "an uneven last split"
    assert (224, 3) in {(c.K, c.splitk) for c in el}
    _need({(c.K, c.splitk, c.colsum_of, c.opnd["A"].ld > c.M and c.opnd["B"].ld > c.N) for c in el},
          [(k, s, o, w) for k, s in R.HANDOFF_SPLITS for o in (0, 1, 2) for w in (False, True)], "hand-off cells")
    kinds = ("near:K+4", "near:M+4", "near:A+1float", "near:lda%4", "near:splitk>slabs")
    _need({(c.label.split("/")[-1], k) for c in ho if not c.eligible for k, s in R.HANDOFF_SPLITS
           if (c.K - (4 if "K+4" in c.label else 0)) == k}, [(n, k) for n in kinds for k, s in R.HANDOFF_SPLITS], "neighbours")
    _need({c.K for c in ho if c.label.endswith("near:empty-split")}, [k for k, s in R.HANDOFF_SPLITS if k // 32 >= 4],
          "empty-split neighbours")
    # Gaussian
    g = [c for c in cs if not c.exact]
    assert len(g) >= 12 and all(c.act == "gelu" and c.family == "gauss" for c in g)
    _need({(c.mode, R.epilogue_form(c)) for c in g}, [(m, f) for m in ("act", "dact") for f in R.FORMS], "gelu cells")


# ---- check() must see what it is there to see --------------------------------------------------------------------------------
def _faithful(c):
    """buffers after a faithful run: the reference written into the valid regions"""
    before = R.build(c, 5)
    ref = R.reference(c, before)
    after = {k: v.clone() for k, v in before.items()}
    for name in R.OUTPUTS:
        if c.has(name):
            after[name][c.opnd[name].index(c.batch).reshape(-1)] = ref[name].reshape(-1).float()
    return before, after, ref


@pytest.mark.parametrize("exact", [True, False])
def test_check_reports_every_kind_of_damage(exact):
    c = R.mk("selftest", 12, 8, 20, layout="TN", terms="act", act="relu" if exact else "gelu", exact=exact, batch=2, pad=4,
             gap=8, colsum_of=1, dev=("C:base+1", "A:base+2"))
    before, after, ref = _faithful(c)
    R.check(c, before, after, ref)                                  # a faithful result passes

    def tampered(name, pos, value):
        t = {k: v.clone() for k, v in after.items()}
        t[name][pos] = value
        return t
    o = c.opnd["C"]
    last = int(o.index(c.batch)[1, 11, 7])
    with pytest.raises(AssertionError, match=r"C: 1( of |/)192 elements (differ|out of tolerance)"):
        R.check(c, before, tampered("C", last, float(after["C"][last]) + (1.0 if exact else 0.5)), ref)
    with pytest.raises(AssertionError, match=r"preact: 1( of |/)192 elements"):
        R.check(c, before, tampered("preact", 5, float(after["preact"][5]) + 1.0), ref)
    with pytest.raises(AssertionError, match=r"colsum: 1( of |/)24 elements"):
        R.check(c, before, tampered("colsum", 3, 99.0), ref)
    with pytest.raises(AssertionError, match="C: 1 of 192 valid elements are NaN"):
        R.check(c, before, tampered("C", last, float("nan")), ref)
    for pos, what in ((0, "base offset"), (1 + o.cols, "pad column"), (1 + o.rows * o.ld + 2, "batch gap")):
        assert bool(after["C"][pos].isnan()), what
        with pytest.raises(AssertionError, match=f"C: 1 sentinel.*flat position {pos} "):
            R.check(c, before, tampered("C", pos, 0.0), ref)
    with pytest.raises(AssertionError, match="preact: 1 sentinel"):
        R.check(c, before, tampered("preact", c.N, 1.0), ref)
    for name in ("A", "B", "bias", "res"):
        with pytest.raises(AssertionError, match=f"{name}: input changed at 1 position"):
            R.check(c, before, tampered(name, c.opnd[name].off, 77.0), ref)
    with pytest.raises(AssertionError, match="A: input changed"):   # a write into an input's pad
        R.check(c, before, tampered("A", 0, 0.0), ref)


# ---- host-only behaviour of the library ----------------------------------------------------------------------------------------
def _desc(c, **over):
    """the descriptor of a case over made-up non-null pointers, with precision = 99: dpot_gemm_f32 validates the descriptor
    and then refuses the precision - whatever the other fields say, it returns before anything is launched"""
    from dpot_amd._lib import GemmDesc
    kw = R.gemm_kwargs(c)
    d = GemmDesc()
    d.A, d.B, d.C = 0x10000, 0x20000, 0x30000
    d.M, d.N, d.K, d.batch = c.M, c.N, c.K, c.batch
    d.transA, d.transB = int(c.transA), int(c.transB)
    d.lda, d.ldb, d.ldc = kw["lda"], kw["ldb"], kw["ldc"]
    d.act, d.epi_mode = kw["act"], kw["mode"]
    for i, (name, field, ldf) in enumerate((("aux", "aux", "ldaux"), ("preact", "preact", "ldpre"), ("res", "res", "ldres"))):
        if c.has(name):
            setattr(d, field, 0x40000 + 0x10000 * i)
            setattr(d, ldf, kw[ldf])
    d.splitk, d.precision = 1, 99
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_missing_epilogue_leading_dimension_is_rejected_before_any_launch(lib):
    act = R.mk("selftest", 8, 8, 8, terms="act")                    # bias, preact, res
    dact = R.mk("selftest", 8, 8, 8, terms="dact")                  # aux
    for c, field in ((act, "ldpre"), (act, "ldres"), (dact, "ldaux")):
        good = _desc(c)
        assert lib.dpot_gemm_f32(C.byref(good), None) == -1
        assert b"bad precision 99" in lib.dpot_last_error()         # every check before the precision's passed
        assert lib.dpot_gemm_f32(C.byref(_desc(c, **{field: c.N})), None) == -1
        assert b"bad precision 99" in lib.dpot_last_error()         # ld == N is enough
        for bad in (0, c.N - 1):                                    # 0: the field's default in ops.gemm
            assert lib.dpot_gemm_f32(C.byref(_desc(c, **{field: bad})), None) == -1
            msg = lib.dpot_last_error().decode()
            assert f"{field}={bad}" in msg and "too small" in msg, msg
    # the field is free while its pointer is null
    assert lib.dpot_gemm_f32(C.byref(_desc(R.mk("selftest", 8, 8, 8))), None) == -1
    assert b"bad precision 99" in lib.dpot_last_error()


class _Recorder:
    """stands in for libdpot_hip and for the module attribute `torch` of dpot_amd.ops: records the descriptor dpot_gemm_f32
    is handed and the sizes ops.gemm allocates, launches nothing"""

    def __init__(self, real):
        self.real, self.descs, self.allocs = real, [], []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def dpot_gemm_f32(self, dref, stream):
        from dpot_amd._lib import GemmDesc
        self.descs.append(GemmDesc.from_buffer_copy(bytes(dref._obj)))
        return 0


class _TorchRecorder:
    def __init__(self, rec):
        self.rec = rec

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, **kw):
        self.rec.allocs.append(size)
        return torch.empty(*size, **kw)


def test_ops_gemm_builds_the_descriptor_and_the_workspace_the_library_asks_for(lib, monkeypatch):
    from dpot_amd import ops
    rec = _Recorder(lib)
    monkeypatch.setattr(ops._lib, "load", lambda: rec)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "torch", _TorchRecorder(rec))
    n_split = 0
    for c in R.CASES:
        t = R.build(c, 1)
        view = {k: v[c.opnd[k].off:] for k, v in t.items()}
        rec.descs.clear(), rec.allocs.clear()
        ops.gemm(view["A"], view["B"], view["C"], c.M, c.N, c.K, bias=view.get("bias"), aux=view.get("aux"),
                 preact=view.get("preact"), res=view.get("res"), colsum_out=view.get("colsum"), **R.gemm_kwargs(c))
        d, = rec.descs
        assert (d.M, d.N, d.K, d.batch, d.transA, d.transB) == (c.M, c.N, c.K, c.batch, int(c.transA), int(c.transB))
        for name, ptr, ld, stride in (("A", d.A, d.lda, d.strideA), ("B", d.B, d.ldb, d.strideB), ("C", d.C, d.ldc, d.strideC),
                                      ("bias", d.bias, None, d.strideBias), ("aux", d.aux, d.ldaux, d.strideAux),
                                      ("preact", d.preact, d.ldpre, d.stridePre), ("res", d.res, d.ldres, d.strideRes),
                                      ("colsum", d.colsum_out, None, d.strideColsum)):
            if not c.has(name):
                assert not ptr, (c.label, name)
                continue
            o = c.opnd[name]
            assert ptr == t[name].data_ptr() + 4 * o.off and stride == o.stride and ld in (None, o.ld), (c.label, name)
        assert (d.res_div, d.res_mod, d.accumulate, d.tile, d.tag, d.colsum_of) == (
            c.res_div, c.res_mod, int(c.accumulate), c.tile, c.tag, c.colsum_of)
        assert (d.precision, d.act, d.epi_mode) == (R.PREC[c.precision], R.ACT[c.act], R.MODE[c.mode])
        want = lib.dpot_gemm_workspace_bytes(C.byref(d))
        if c.splitk > 1:
            n_split += 1
            L = c.M if c.colsum_of == 1 else c.N if c.colsum_of == 2 else 0
            assert d.splitk == c.splitk and d.workspace and rec.allocs == [(c.splitk * c.batch * (c.M * c.N + L),)], c.label
            assert want == 4 * rec.allocs[0][0], c.label
        else:
            assert d.splitk == 1 and not d.workspace and not rec.allocs and want == 0, c.label
    assert n_split >= 100


def test_tn_splitk_never_names_a_split_count_the_hand_off_refuses(lib):
    on = 0
    for M in R.HANDOFF_M:
        for N in R.HANDOFF_N:
            for nslab in range(1, 97):
                s = lib.dpot_gemm_tn_splitk(M, N, 32 * nslab, 1)
                if s == 0:
                    continue
                on += 1
                sps = -(-nslab // s)
                assert 2 <= s <= nslab and sps * (s - 1) < nslab, (M, N, nslab, s)   # the checks of dpot_gemm_tn_try
            assert lib.dpot_gemm_tn_splitk(M, N, 32 * 8 + 16, 1) == 0                 # K % 32, not K % 16
            assert lib.dpot_gemm_tn_splitk(M + 4, N, 256, 1) == 0 and lib.dpot_gemm_tn_splitk(M, N, 256, 2) == 0
    assert on > 0 or lib.dpot_tune(b"panel", 1) == 0
