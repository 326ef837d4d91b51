"""Every instantiation of the AFNO mixer kernels (csrc/afno_mlp.hip) on the cases of afno_mixer_cases.py: before each launch the
library's own selection (dpot_afno_mlp2_plan) is asserted to name the instantiation the case is in the table for, so a failure
here names the kernel that broke.  Integer operands are held to the float64 result with torch.equal (tests/test_cpu_afno_mixer.py
shows that every partial sum stays exact in fp32), real-valued data to float64 at assert_close's default and at a norm-wise
bound scaled by torch-CPU float32's own error; every tensor lives in a guarded, poisoned buffer, so rows past M and the pad
columns of a leading dimension can neither be read into a result nor be written."""
import numpy as np
import pytest
import torch

import act_ref as AR
import afno_mixer_cases as MC
import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS24 = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from dpot_amd import ops as _ops
    from dpot_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module")
def bounds():
    return AR.Bounds(AR.sample_points())


@pytest.fixture(autouse=True)
def _guard(guarded):
    """every test of this module runs on guarded, poisoned allocations (tests/guard.py) and checks the guards when it ends"""
    yield guarded


def dev(t):
    return guard.wrap(t, "cuda")


def place(t, pad):
    """a [M, cols] input on the GPU as the first `cols` columns of a guarded [M, cols + pad] buffer whose pad columns hold NaN"""
    if not pad:
        return dev(t)
    buf = dev(torch.cat([t, torch.full((t.shape[0], pad), NAN)], dim=1))
    return buf[:, :t.shape[1]]


def slot(M, cols, pad):
    """(buffer, view): a NaN-filled [M, cols + pad] output between guards and its first `cols` columns"""
    buf = guard.full_nan((M, cols + pad))
    return buf, buf[:, :cols]


def weights(ops, c, t):
    """the packs of a case: {a: (Wa, ba, Wb, bb) of mode 0, b: (Wa, Wb) of mode 1}"""
    if c.layout == 0:                      # Wbig built on the CPU: [[Wr, Wi], [-Wi, Wr]]
        f1, k1 = ops.afno_block_weights(dev(MC.wbig(t["w1"])))
        f2, k2 = ops.afno_block_weights(dev(MC.wbig(t["w2"])))
        b1, b2 = dev(MC.bbig(t["b1"])), dev(MC.bbig(t["b2"]))
    else:
        packs = ops.AfnoPacks([(dev(t["w1"]), dev(t["b1"])), (dev(t["w2"]), dev(t["b2"]))])
        assert packs.layout == 1
        (_, b1, f1, k1), (_, b2, f2, k2) = packs.refresh()
    return {"fwd": (f1, b1, f2, b2), "bwd": (k2, None, k1, None)}


def launch(ops, c, w, X, aux=None, outputs=None, mode=None):
    """one launch of the case (or of its other direction / another output set): asserts the plan, returns {Y, pre, mid} on
    the device; with pads the outputs are views of NaN-filled buffers whose pad columns are asserted to stay bitwise NaN"""
    mode = c.mode if mode is None else mode
    outputs = c.outputs if outputs is None else outputs
    act = MC.ACT_IDS[c.act]
    pl = ops.afno_mlp2_plan(c.M, c.nb, c.bs, c.layout, act)
    assert (pl.form, pl.rt, pl.gelu) == (c.want_form, c.want_rt, c.act == "gelu"), \
        f"{MC.case_id(c)}: the library plans {pl}, the table names {MC.FORM_NAMES[c.want_form]} RT {c.want_rt}"
    assert pl.panels == -(-c.M // (16 * pl.rt)) and pl.waves == (8 if pl.form == MC.SPLIT else c.bs // 16)
    cols = c.nb * 2 * c.bs
    Wa, ba, Wb, bb = w["bwd" if mode else "fwd"]
    kw = dict(mode=mode, aux=place(aux, c.ldo_pad) if mode else None, want_pre="pre" in outputs, want_mid="mid" in outputs,
              layout=c.layout)
    bufs = {}
    if c.ldx_pad or c.ldo_pad:
        for name in ("Y",) + tuple(outputs):
            bufs[name], kw["out_" + name] = slot(c.M, cols, c.ldo_pad)
    Y, pre, mid = ops.afno_mlp2(place(X, c.ldx_pad), Wa, ba, Wb, bb, c.nb, c.bs, act, **kw)
    got = {"Y": Y, "pre": pre, "mid": mid}
    for name, buf in bufs.items():
        assert got[name].data_ptr() == buf.data_ptr() and got[name].stride(0) == cols + c.ldo_pad
        if c.ldo_pad:
            assert bool((buf[:, cols:].view(torch.int32) == -1).all()), f"{MC.case_id(c)}: pad columns of {name} were written"
    for name in ("pre", "mid"):
        assert (got[name] is not None) == (name in outputs)
    return got


def equal(got, ref, what):
    """the float32 output equals the float64 reference as numbers (-0 == +0; a NaN - an unwritten element - fails)"""
    g, r = got.detach().cpu(), ref.float()
    assert torch.equal(r.double(), ref), f"{what}: the reference is no fp32 number"
    if not torch.equal(g, r):
        bad = ~(g == r)
        i = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements differ ({int(g.isnan().sum())} NaN); first at "
                             f"{i}: got {g[i].item()!r}, reference {r[i].item()!r}")


def normwise(got, ref, e32, form, what):
    """||got - ref|| / ||ref|| <= F[form] * max(e32, 2^-24); prints the ratio before it asserts"""
    err = MC.rel_err(got, ref)
    ratio = err / max(e32, EPS24)
    print(f"afno-mixer-error {what}: kernel {err:.3e} float32 {e32:.3e} ratio {ratio:.3f} (F {MC.F[form]})")
    assert ratio <= MC.F[form], f"{what}: relative error {err:.3e} is {ratio:.2f} x max(float32's {e32:.3e}, 2^-24), bound {MC.F[form]}"
    return ratio


def layer2_of_own_mid(c, t, mid_gpu, dtype):
    """mid W + b of the kernel's own `mid` output: mode 0 with the second layer's weights, mode 1 with W1^T"""
    m = mid_gpu.detach().cpu().to(dtype)
    if c.mode == 0:
        return MC.layer(m, MC.wbig(t["w2"]).to(dtype), MC.bbig(t["b2"]).to(dtype))
    return MC.layer(m, MC.wbig(t["w1"]).to(dtype), transpose=True)


# ---- a. integer operands: every instantiation, both directions, zero tolerance ---------------------------------------------
@pytest.mark.parametrize("c", MC.INT, ids=MC.case_id)
def test_exact_on_integer_operands(ops, bounds, c):
    what = f"{MC.case_id(c)} ({MC.FORM_NAMES[c.want_form]} RT {c.want_rt}: {c.note})"
    t, ref = MC.int_inputs(c), MC.int_reference(c)
    w = weights(ops, c, t)
    got = launch(ops, c, w, t["X"], aux=t["aux"])
    if c.act != "gelu":
        for name in ("pre", "mid", "Y"):
            if got[name] is not None:
                equal(got[name], ref[name], f"{what}: {name}")
        return
    # GELU: the integer part stays exact - layer 1 before the activation (mode 0: `pre`) - and the activation is held to the
    # point-wise rule of the fused call sites against act_ref's float32 restatement of the device function
    x = (ref["pre"] if c.mode == 0 else t["aux"]).float().numpy().reshape(-1)
    if c.mode == 0:
        if got["pre"] is not None:
            equal(got["pre"], ref["pre"], f"{what}: pre")
        want_mid = AR.gelu_fwd(x).astype(np.float64)
        tol_mid = bounds.tol("gelu", "value", x, AR.reference("gelu", x)[0])
    else:
        v = MC.layer(t["X"].double(), MC.wbig(t["w2"]).double(), transpose=True).numpy().reshape(-1)     # exact integers
        val, der = AR.gelu_val_der(x) if "pre" in c.outputs else (None, AR.gelu_bwd(x))
        v64, d64 = AR.reference("gelu", x)
        want_mid = (v.astype(np.float32) * der).astype(np.float64)                                       # one fp32 product
        tol_mid = np.abs(v) * bounds.tol("gelu", "derivative", x, d64) + AR.ulp32(v * d64)
        if got["pre"] is not None:                            # act(aux), re-derived
            p = got["pre"].cpu().numpy().reshape(-1).astype(np.float64)
            bad = ~(np.abs(p - val.astype(np.float64)) <= bounds.tol("gelu", "value", x, v64))
            assert not bad.any(), f"{what}: gelu(aux): {int(bad.sum())} points out of bound"
    if got["mid"] is not None:
        m = got["mid"].cpu().numpy().reshape(-1).astype(np.float64)
        bad = ~(np.abs(m - want_mid) <= tol_mid)
        assert not bad.any(), (f"{what}: mid: {int(bad.sum())} of {bad.size} points out of bound; worst |d| "
                               f"{np.nanmax(np.abs(m - want_mid) - tol_mid):.3e} over the bound")
        # layer 2 on the kernel's own mid: an error there cannot hide behind the activation's rounding
        Yref, Y32 = layer2_of_own_mid(c, t, got["mid"], torch.float64), layer2_of_own_mid(c, t, got["mid"], torch.float32)
        assert_close(got["Y"], Yref, f"{what}: Y against float64 of the kernel's mid")
        normwise(got["Y"], Yref, MC.rel_err(Y32, Yref), c.want_form, f"{what}: Y of own mid")
    else:
        assert c.mode == 0, "every backward case of the table asks for mid"
        r32 = MC.forward_ref(t, "gelu", torch.float32)       # no mid to start from: the whole chain, GELU in float64 / float32
        assert_close(got["Y"], ref["Y"], f"{what}: Y")
        normwise(got["Y"], ref["Y"], MC.rel_err(r32["Y"], ref["Y"]), c.want_form, f"{what}: Y")


# ---- b. real-valued data against float64, element-wise and norm-wise -----------------------------------------------------------
@pytest.mark.parametrize("c", MC.REAL, ids=MC.case_id)
def test_real_data_vs_float64(ops, c):
    what = f"{MC.case_id(c)} ({MC.FORM_NAMES[c.want_form]} RT {c.want_rt})"
    t = MC.real_inputs(c)
    w = weights(ops, c, t)
    ref, r32 = MC.forward_ref(t, c.act), MC.forward_ref(t, c.act, torch.float32)
    got = launch(ops, c, w, t["X"], outputs=("pre", "mid"), mode=0)
    for name in ("pre", "mid", "Y"):
        assert_close(got[name], ref[name], f"{what}: {name}")
        normwise(got[name], ref[name], MC.rel_err(r32[name], ref[name]), c.want_form, f"{what}: {name}")
    aux = ref["pre"].float()
    bref, b32 = MC.backward_ref(t, c.act, t["dO2"], aux), MC.backward_ref(t, c.act, t["dO2"], aux, torch.float32)
    for outputs in (("mid",), ("mid", "pre")):
        got = launch(ops, c, w, t["dO2"], aux=aux, outputs=outputs, mode=1)
        tag = "+".join(outputs)
        for name, label in (("mid", "dO1pre"), ("Y", "dS")) + ((("pre", "act(aux)"),) if "pre" in outputs else ()):
            assert_close(got[name], bref[name], f"{what}: {label} [{tag}]")
            normwise(got[name], bref[name], MC.rel_err(b32[name], bref[name]), c.want_form, f"{what}: {label} [{tag}]")


# ---- d. same bits on a second call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", MC.REPEAT, ids=MC.case_id)
def test_second_call_gives_the_same_bits(ops, c):
    t = MC.real_inputs(c)
    w = weights(ops, c, t)
    a = launch(ops, c, w, t["X"], mode=0)
    b = launch(ops, c, w, t["X"], mode=0)
    aux = a["pre"].detach().cpu()
    da = launch(ops, c, w, t["dO2"], aux=aux, outputs=("mid", "pre"), mode=1)
    db = launch(ops, c, w, t["dO2"], aux=aux, outputs=("mid", "pre"), mode=1)
    for x, y in ((a, b), (da, db)):
        for name in ("Y", "pre", "mid"):
            assert x[name].data_ptr() != y[name].data_ptr() and not bool(x[name].isnan().any())
            assert torch.equal(x[name], y[name]), f"{MC.case_id(c)}: {name} differs between two calls"


# ---- e. three-product Y against four-product Y at RT 2 and RT 4 ---------------------------------------------------------------
@pytest.mark.parametrize("nb,bs,M,rt", MC.CROSS)
def test_three_product_vs_four_product(ops, nb, bs, M, rt):
    form = MC.SPLIT if bs == 96 else MC.THREE
    c3 = MC.Case(1, nb, bs, M, "gelu", 0, ("pre", "mid"), 0, 0, rt, form, "against the four-product kernel")
    c4 = c3._replace(layout=0, want_form=MC.FOUR)
    t = MC.real_inputs(c3)
    g3 = launch(ops, c3, weights(ops, c3, t), t["X"])
    g4 = launch(ops, c4, weights(ops, c4, t), t["X"])
    for name in ("pre", "mid", "Y"):
        assert_close(g3[name], g4[name].double(), f"bs {bs} RT {rt}: {name} vs four-product kernel", rtol=2e-5, atol_scale=2e-5)
