"""Every route of the GroupNorm kernels (csrc/norm.hip) against float64, on the cases of gn_cases.py: before each launch the
library's own selection (dpot_groupnorm_kernel_kind) is asserted to name the route the case is in the table for, so a
failure here names the kernel that broke.  Inputs and references are those of gn_cases.py (tests/test_cpu_groupnorm.py
shows that a dropped last token or last channel cannot pass them); every tensor lives in a guarded, poisoned buffer."""
import pytest
import torch

import gn_cases as GC
import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from dpot_amd import ops as _ops
    from dpot_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(autouse=True)
def _guard(guarded):
    """every test of this module runs on guarded, poisoned allocations (tests/guard.py) and checks the guards when it ends"""
    yield guarded


def lib():
    from dpot_amd import _lib
    return _lib.load()


def place(t, off=0):
    """a test input on the GPU inside a guarded buffer, `off` floats past its 512-byte aligned start (NaN in front)"""
    if off == 0:
        return guard.wrap(t, "cuda")
    buf = guard.wrap(torch.cat([torch.full((off,), NAN), t.reshape(-1)]), "cuda")
    v = buf[off:].view(t.shape)
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def slot(shape, off=0, dtype=torch.float32):
    """(buffer, view): a NaN-filled output between guards, the view `off` elements past its aligned start"""
    n = 1
    for s in shape:
        n *= s
    buf = guard.full_nan(n + off, dtype)
    return buf, buf[off:].view(shape)


def upload(c, t):
    off = dict(c.off)
    return {k: place(v, off.get(k, 0)) for k, v in t.items()}


def close(got, ref, name, what):
    assert_close(got, ref, f"{what}: {name}", **GC.TOL[name])


def all_nan(*tensors):
    return all(bool(t.isnan().all()) for t in tensors)


# ---- launches: through ops, or - where the OUTPUT is to be misaligned or has to be seen untouched - the C entry points ---
def run_fwd(ops, c, d):
    chunked, off = c.form != "fb_noc", dict(c.off).get("out", 0)
    if not off:
        return ops.groupnorm_fwd(d["x"], d["gamma"], d["beta"], c.G, GC.EPS, chunked=chunked)
    ybuf, y = slot((c.B, c.T, c.E), off)
    _, mean = slot((c.B, c.G))
    _, rstd = slot((c.B, c.G))
    ws = ops._gn_workspace(c.B, c.T, c.E, c.G, y.device) if chunked else None
    ops.check(lib().dpot_groupnorm_fwd(d["x"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(), y.data_ptr(),
                                       mean.data_ptr(), rstd.data_ptr(), ops._p(ws), c.B, c.T, c.E, c.G, GC.EPS,
                                       ops._stream()), "groupnorm_fwd")
    assert all_nan(ybuf[:off]), "the floats in front of a misaligned y were written"
    return y, mean, rstd


def run_bwd(ops, c, d, mean, rstd, add, defer):
    chunked, off = c.form != "fb_noc", dict(c.off).get("out", 0)
    if not off:
        return ops.groupnorm_bwd(d["dy"], d["x"], mean, rstd, d["gamma"], c.G, add=add, defer=defer, chunked=chunked)
    dxbuf, dx = slot((c.B, c.T, c.E), off)
    _, part = slot((2, c.B, c.E))
    dg = None if defer else slot((c.E,))[1]
    db = None if defer else slot((c.E,))[1]
    ws = ops._gn_workspace(c.B, c.T, c.E, c.G, dx.device) if chunked else None
    ops.check(lib().dpot_groupnorm_bwd(d["dy"].data_ptr(), d["x"].data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                       d["gamma"].data_ptr(), ops._p(add), dx.data_ptr(), ops._p(dg), ops._p(db),
                                       part.data_ptr(), ops._p(ws), c.B, c.T, c.E, c.G, ops._stream()), "groupnorm_bwd")
    assert all_nan(dxbuf[:off]), "the floats in front of a misaligned dx were written"
    return (dx, part) if defer else (dx, dg, db)


def bwd_aligned(c, use_add):
    """the backward looks at `add` only when it is given"""
    return not any(k in GC.BWD_OPERANDS and (k != "add" or use_add) and v % 4 for k, v in c.off)


# ---- forward + backward, every route -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GC.FB, ids=GC.case_id)
def test_forward_and_backward_vs_float64(ops, c):
    what = GC.case_id(c)
    B, T, E, G = c.B, c.T, c.E, c.G
    ws = c.form != "fb_noc"
    t, ref = GC.inputs(B, T, E, G), GC.reference(B, T, E, G)
    d = upload(c, t)
    # forward: y, mean, rstd
    assert ops.groupnorm_kernel_kind(B, T, E, G, "fwd", ws, GC.aligned_for(c, "fwd")) == c.kind_fwd
    if c.kind_fwd == GC.CHUNKED:
        assert ops.groupnorm_chunks(B, T, E, G) == GC.gn_chunking(B, T, E, G) and ops.groupnorm_ws_elems(B, T, E, G) > 0
    y, mean, rstd = run_fwd(ops, c, d)
    for name, got in (("y", y), ("mean", mean), ("rstd", rstd)):
        close(got, ref[name], name, what)
    # backward: add given or not x parameter gradients reduced at once or deferred, each twice
    for use_add in (True, False):
        add = d["add"] if use_add else None
        kind = ops.groupnorm_kernel_kind(B, T, E, G, "bwd", ws, bwd_aligned(c, use_add))
        assert kind == GC.gn_select(B, T, E, G, "bwd", ws, bwd_aligned(c, use_add))
        if use_add:
            assert kind == c.kind_bwd
        dx, dg, db = run_bwd(ops, c, d, mean, rstd, add, defer=False)
        close(dx, ref["dx"] + t["add"].double() if use_add else ref["dx"], "dx", f"{what} add={use_add}")
        close(dg, ref["dgamma"], "dgamma", what)
        close(db, ref["dbeta"], "dbeta", what)
        dx2, dg2, db2 = run_bwd(ops, c, d, mean, rstd, add, defer=False)
        assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2), f"{what}: two runs differ"
        dx3, part = run_bwd(ops, c, d, mean, rstd, add, defer=True)
        dx4, part4 = run_bwd(ops, c, d, mean, rstd, add, defer=True)
        assert torch.equal(dx3, dx4) and torch.equal(part, part4), f"{what}: two deferred runs differ"
        assert torch.equal(dx3, dx), f"{what}: dx differs between defer=True and defer=False"
        close(part, ref["part"], "part", what)
        (dg5, db5), = ops.groupnorm_param_grads([(part, None, None)])
        assert torch.equal(dg5, dg) and torch.equal(db5, db), f"{what}: deferred parameter gradients differ from the immediate ones"


# ---- statistics only -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GC.STATS, ids=GC.case_id)
def test_statistics_only_vs_float64(ops, c):
    what = GC.case_id(c)
    B, T, E, G = c.B, c.T, c.E, c.G
    t, ref = GC.inputs(B, T, E, G), GC.reference(B, T, E, G)
    d = upload(c, t)
    assert ops.groupnorm_kernel_kind(B, T, E, G, "stats") == c.kind_fwd == GC.CHUNKED
    assert ops.groupnorm_stats_supported(B, T, E, G)
    mean, rstd = ops.groupnorm_stats(d["x"], d["gamma"], d["beta"], G, GC.EPS)
    close(mean, ref["mean"], "mean", what)
    close(rstd, ref["rstd"], "rstd", what)
    _, mean1, rstd1 = ops.groupnorm_fwd(d["x"], d["gamma"], d["beta"], G, GC.EPS)
    assert torch.equal(mean, mean1) and torch.equal(rstd, rstd1), f"{what}: statistics differ from the full forward's"


@pytest.mark.parametrize("shape", GC.STATS_REFUSED, ids=str)
def test_statistics_only_refused_launches_nothing(ops, shape):
    """off the chunked route there is no statistics-only form: the call raises, with or without a workspace, and writes nothing"""
    B, T, E, G = shape
    t = GC.inputs(B, T, E, G)
    x, gamma, beta = place(t["x"]), place(t["gamma"]), place(t["beta"])
    assert ops.groupnorm_kernel_kind(B, T, E, G, "stats") == GC.REFUSED and not ops.groupnorm_stats_supported(B, T, E, G)
    with pytest.raises(RuntimeError, match="statistics-only"):
        ops.groupnorm_stats(x, gamma, beta, G, GC.EPS)
    for with_ws in (False, True):
        _, mean = slot((B, G))
        _, rstd = slot((B, G))
        ws = slot((4096,))[1] if with_ws else None
        rc = lib().dpot_groupnorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, mean.data_ptr(), rstd.data_ptr(),
                                      ops._p(ws), B, T, E, G, GC.EPS, ops._stream())
        torch.cuda.synchronize()
        assert rc != 0
        assert all_nan(mean, rstd) and (ws is None or all_nan(ws)), "a refused statistics-only call wrote something"


# ---- the hard statistics inputs on every forward route ------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", GC.HARD_RECIPES)
@pytest.mark.parametrize("B,T,E,G,chunked,kind", GC.HARD_SHAPES, ids=lambda v: str(v))
def test_hard_statistics_on_every_forward_route(ops, recipe, B, T, E, G, chunked, kind):
    """mean >> sigma, outliers, nearly constant data and an offset border (the inputs of
    test_gpu_ops.py::test_groupnorm_chunked_statistics_hard_cases, at its tolerances) through the two-pass kernels as well"""
    assert ops.groupnorm_kernel_kind(B, T, E, G, "fwd", chunked) == kind
    xh = GC.hard_input(recipe, B, T, E, G)
    x, gw, gb = place(xh), place(torch.ones(E)), place(torch.zeros(E))
    y, mean, rstd = ops.groupnorm_fwd(x, gw, gb, G, GC.EPS, chunked=chunked)
    mu, var = GC.stats_ref(xh, G)
    what = f"{recipe} kind {kind}"
    close(mean, mu, "mean", what)
    close(rstd, 1 / torch.sqrt(var + GC.EPS), "rstd", what)
    assert bool(torch.isfinite(y).all())


# ---- pack-writing backward ----------------------------------------------------------------------------------------------------
def pack_ref(ops, dx2d):
    """the two bf16 packs of dx [M, K] from a separate pass"""
    M, K = dx2d.shape
    if ops.bf16_pack_both_supported(M, K):
        pr, pt, _ = ops.bf16_pack_both(dx2d)
        return pr, pt
    return ops.bf16_pack_rows(dx2d, trans=False), ops.bf16_pack_rows(dx2d, trans=True)


def colsum_ref(dx, rows, tc):
    """float64 sums of dx [B, T, E] over the token range of every column-sum row: [B * rows, E]"""
    B, T, E = dx.shape
    dx = dx.double().cpu()
    if rows == 1:
        return dx.sum(1)
    return torch.stack([dx[:, k * tc:(k + 1) * tc].sum(1) for k in range(rows)], dim=1).reshape(B * rows, E)


@pytest.mark.parametrize("c", GC.PACKS, ids=GC.case_id)
def test_pack_writing_backward(ops, c):
    what = GC.case_id(c)
    B, T, E, G = c.B, c.T, c.E, c.G
    t, ref = GC.inputs(B, T, E, G), GC.reference(B, T, E, G)
    d = upload(c, t)
    assert ops.groupnorm_kernel_kind(B, T, E, G, "bwd_packs") == c.kind_bwd
    assert ops.groupnorm_kernel_kind(B, T, E, G, "fwd") == c.kind_fwd
    rows = ops.groupnorm_bwd_packs_rows(B, T, E, G)
    tc, chunks = ops.groupnorm_chunks(B, T, E, G)
    assert rows == (chunks if c.kind_bwd == GC.CHUNKED else 1) and rows > 0
    _, mean, rstd = ops.groupnorm_fwd(d["x"], d["gamma"], d["beta"], G, GC.EPS)
    for use_add in (True, False):
        add = d["add"] if use_add else None
        dx0, part0 = ops.groupnorm_bwd(d["dy"], d["x"], mean, rstd, d["gamma"], G, add=add, defer=True)
        dx, part, pr, pt, cs = ops.groupnorm_bwd_packs(d["dy"], d["x"], mean, rstd, d["gamma"], G, add=add)
        assert torch.equal(dx, dx0) and torch.equal(part, part0), f"{what}: dx / part differ from groupnorm_bwd(defer=True)"
        close(dx, ref["dx"] + t["add"].double() if use_add else ref["dx"], "dx", f"{what} add={use_add}")
        close(part, ref["part"], "part", what)
        pr0, pt0 = pack_ref(ops, dx0.view(B * T, E))
        assert pr.shape == pr0.shape and pt.shape == pt0.shape
        assert torch.equal(pr.view(torch.int16), pr0.view(torch.int16)), f"{what}: row-form pack of dx"
        assert torch.equal(pt.view(torch.int16), pt0.view(torch.int16)), f"{what}: transposed pack of dx"
        assert cs.shape == (B * rows, E)
        close(cs, colsum_ref(dx0, rows, tc), "colsum", what)
        again = ops.groupnorm_bwd_packs(d["dy"], d["x"], mean, rstd, d["gamma"], G, add=add)
        for a, b in zip((dx, part, pr.view(torch.int16), pt.view(torch.int16), cs),
                        (again[0], again[1], again[2].view(torch.int16), again[3].view(torch.int16), again[4])):
            assert torch.equal(a, b), f"{what}: two runs differ"


def raw_packs(ops, d, mean, rstd, shape, add=None, rows_off=0, trans_off=0):
    """dpot_groupnorm_bwd_packs on NaN-filled outputs of its own; returns (rc, outputs)"""
    B, T, E, G = shape
    L = lib()
    _, dx = slot((B, T, E))
    _, part = slot((2, B, E))
    _, pr = slot((L.dpot_bf16_packed_elems(B * T, E, 1),), rows_off, torch.bfloat16)
    _, pt = slot((L.dpot_bf16_packed_elems(E, B * T, 1),), trans_off, torch.bfloat16)
    _, cs = slot((B * 64, E))
    _, ws = slot((max(ops.groupnorm_ws_elems(B, T, E, G), 4096),))
    rc = L.dpot_groupnorm_bwd_packs(d["dy"].data_ptr(), d["x"].data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                    d["gamma"].data_ptr(), ops._p(add), dx.data_ptr(), part.data_ptr(), pr.data_ptr(),
                                    pt.data_ptr(), cs.data_ptr(), ws.data_ptr(), B, T, E, G, ops._stream())
    torch.cuda.synchronize()
    return rc, (dx, part, pr, pt, cs, ws)


@pytest.mark.parametrize("shape", GC.PACKS_REFUSED, ids=str)
def test_pack_writing_backward_refused_shapes_launch_nothing(ops, shape):
    B, T, E, G = shape
    t = GC.inputs(B, T, E, G)
    d = {k: place(v) for k, v in t.items()}
    assert ops.groupnorm_bwd_packs_rows(B, T, E, G) == 0 and not ops.groupnorm_bwd_packs_supported(T, E, G, B=B)
    assert ops.groupnorm_kernel_kind(B, T, E, G, "bwd_packs") == GC.REFUSED
    _, mean, rstd = ops.groupnorm_fwd(d["x"], d["gamma"], d["beta"], G, GC.EPS)
    with pytest.raises(RuntimeError, match="groupnorm_bwd_packs"):
        ops.groupnorm_bwd_packs(d["dy"], d["x"], mean, rstd, d["gamma"], G, add=d["add"])
    rc, outs = raw_packs(ops, d, mean, rstd, shape, add=d["add"])
    assert rc != 0 and all_nan(*outs), "a refused pack-writing backward wrote something"


@pytest.mark.parametrize("shape", [(1, 32, 1024, 8), (1, 2016, 256, 8)], ids=str)      # a cached and a chunked pack case
def test_pack_writing_backward_misaligned_pointers_launch_nothing(ops, shape):
    B, T, E, G = shape
    assert shape in [(c.B, c.T, c.E, c.G) for c in GC.PACKS]
    t = GC.inputs(B, T, E, G)
    d = {k: place(v) for k, v in t.items()}
    bad_add = place(t["add"], 1)
    _, mean, rstd = ops.groupnorm_fwd(d["x"], d["gamma"], d["beta"], G, GC.EPS)
    assert ops.groupnorm_kernel_kind(B, T, E, G, "bwd_packs", True, False) == GC.REFUSED
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.groupnorm_bwd_packs(d["dy"], d["x"], mean, rstd, d["gamma"], G, add=bad_add)
    for kw in (dict(add=bad_add), dict(rows_off=2), dict(trans_off=2)):                 # 2 bf16 = 4 bytes off
        rc, outs = raw_packs(ops, d, mean, rstd, shape, **kw)
        assert rc != 0 and all_nan(*outs), f"a pack-writing backward with {list(kw)} misaligned wrote something"
    rc, outs = raw_packs(ops, d, mean, rstd, shape, add=d["add"])                       # the same call, aligned: it runs
    assert rc == 0 and bool(torch.isfinite(outs[0]).all())


# ---- the parameter-gradient reduction ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", GC.PARAM_GRAD_E)
@pytest.mark.parametrize("B", GC.PARAM_GRAD_B)
def test_param_grads_vs_float64(ops, B, E):
    """the two-at-a-time sample loop with and without a tail (B = 9: one pairwise step, then one more sample), one to four jobs
    in a launch, E below and off the 64-channel block"""
    g = torch.Generator().manual_seed(100 * B + E)
    parts = [torch.randn(2, B, E, generator=g) + 0.25 * (j + 1) for j in range(4)]
    dev = [place(p) for p in parts]
    for njobs in (1, 2, 3, 4):
        outs = ops.groupnorm_param_grads([(dev[j], None, None) for j in range(njobs)])
        again = ops.groupnorm_param_grads([(dev[j], None, None) for j in range(njobs)])
        assert len(outs) == njobs
        for j, ((dg, db), (dg2, db2)) in enumerate(zip(outs, again)):
            assert dg.shape == (E,) and db.shape == (E,)
            close(dg, parts[j][0].double().sum(0), "dgamma", f"B={B} E={E} job {j} of {njobs}")
            close(db, parts[j][1].double().sum(0), "dbeta", f"B={B} E={E} job {j} of {njobs}")
            assert torch.equal(dg, dg2) and torch.equal(db, db2)
