"""Every fused nonlinearity against float64, point by point, over its whole domain (tests/act_ref.py: the sample vector, the
references and the rule |got - ref| <= c ulp32(ref) + a).

How a site is driven.  The activation alone is observed through the site's own GEMM: y = act(P @ I + 0) with the sample points
P as the left operand and an identity / selection matrix as the weight (products by 1 and sums with 0 are exact in fp32), and
dx = (dy @ W) * act'(aux) with dy one-hot in column 0 against a weight row of ones, so dy @ W == 1 exactly, and the sample
points in aux.  Where the op returns its pre-activation the test asserts first, with torch.equal, that it IS the sample points.

Non-finite pre-activations.  0 * inf = NaN: a non-finite value in the left operand of a GEMM poisons its whole output row, so
through the product only finite points can be driven.  NaN / +inf / -inf reach a forward epilogue through the BIAS instead
(columns 0, 5, 10, 15 modulo 16: every float4 of the epilogue that holds a non-finite lane holds finite lanes too, and every
row holds both), and reach act' and the recomputing backward kernels directly, in aux, at positions 0, 5, 10, 15 modulo 16 of
the vector.  A bias makes a whole output column non-finite, so for the forward form the finite neighbours of a non-finite
value are those of its float4 and its row; in aux they are those of its float4, row and column.

bf16-plane sites see the points a 3-way bf16 split holds exactly (finite, 2^-100 <= |x| <= 1e4, +-0): the others are
replaced by 0 and not counted.  The one-plane epilogues of the bf16 panel GEMM (saved act', packed act' product) see the
points rounded to bf16, and their own returned pre-activation is asserted to be exactly those.

Each test asserts that it compared at least 95 % of the vector and prints the largest error it saw.
"""
import numpy as np
import pytest
import torch

import act_ref as AR
import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import set_tune

pytestmark = pytest.mark.gpu

V = AR.sample_points()
FIN = np.isfinite(V)
VF = np.where(FIN, V, np.float32(0))                       # for the left operand of a GEMM: finite points only
B16 = AR.bf16_exact(V)
VB = np.where(B16, V, np.float32(0))                       # for a three-plane bf16 operand
ALL8 = list(AR.NAMES)


@pytest.fixture(scope="module")
def ops():
    from dpot_amd import ops as _ops
    from dpot_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module")
def bounds():
    b = AR.Bounds(V)
    assert b.restate_err[0] <= AR.DOC_GELU_ERR * 1.02 and b.restate_err[1] <= AR.DOC_GELU_DER_ERR   # common.h's comment
    return b


@pytest.fixture(autouse=True)
def _guard(guarded):
    yield guarded


def dev(t):
    return guard.wrap(t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)), "cuda")


def host(t):
    return t.detach().float().cpu().numpy()


def chunks(v, rows, cols):
    """the vector as consecutive [rows, cols] operands, the last one padded with zeros: (matrix, number of points in it)"""
    per = rows * cols
    for s in range(0, v.size, per):
        c = v[s:s + per]
        P = np.zeros(per, np.float32)
        P[:c.size] = c
        yield torch.from_numpy(P.reshape(rows, cols)), c.size


def sweep(v, rows, cols, fn):
    """fn(P [rows, cols]) -> tuple of [rows, cols] results; returns each result over the whole vector"""
    outs = None
    for P, n in chunks(v, rows, cols):
        res = [host(r).reshape(-1)[:n] for r in fn(P)]
        outs = [[r] for r in res] if outs is None else [o + [r] for o, r in zip(outs, res)]
    return [np.concatenate(o) for o in outs]


def same_bits(t, want):
    """torch.equal with NaN == NaN (for operands that hold non-finite values on purpose)"""
    return np.array_equal(host(t), np.asarray(want, np.float32), equal_nan=True)


def nf_bias(cols):
    b = np.zeros(cols, np.float32)
    for j in range(cols):
        if j % 16 in (0, 5, 10, 15):
            b[j] = (np.nan, np.inf, -np.inf)[(j // 4) % 3]
    return b


def held(name, kind, x, got, bounds, what, mask=None, floor=0.95, extra_rel=0.0):
    if mask is not None:
        x, got = x[mask], got[mask]
    n, worst = AR.check(name, kind, x, got, bounds, what, extra_rel)
    print(f"{what}: {n} points, max |err| {worst:.3e}")
    assert n >= floor * V.size, f"{what}: compared only {n} of {V.size} points"
    return worst


def forward_with_nonfinite_bias(name, fwd, rows, cols, bounds, what):
    """finite points through the product, NaN / inf through the bias: pre == P + bias exactly, act(pre) to the rule"""
    P, _ = next(chunks(VF, rows, cols))
    b = nf_bias(cols)
    y, pre = fwd(P, b)
    with np.errstate(all="ignore"):
        want = (P.numpy() + b[None, :]).astype(np.float32)
    assert same_bits(pre, want), f"{what}: the pre-activation is not the sample points + bias"
    held(name, "value", want.reshape(-1), host(y).reshape(-1), bounds, what + " (non-finite bias)", floor=0.0)


def one_hot(rows, n):
    dy = torch.zeros(rows, n)
    dy[:, 0] = 1.0
    return dy


def ones_row(n, k):
    w = torch.zeros(n, k)
    w[0, :] = 1.0
    return w


# ---- fp32 GEMM epilogue: vector path (N = K = 64), scalar path (N = K = 63, odd ld) ----------------------------------------
@pytest.mark.parametrize("n", [64, 63])
@pytest.mark.parametrize("name", ALL8)
def test_gemm_f32_epilogue(ops, bounds, name, n):
    a = ops.ACT_IDS[name]
    rows = -(-V.size // n)
    eye, w1 = dev(torch.eye(n)), dev(ones_row(n, n))

    def fwd(P, bias=None):
        b = dev(np.zeros(n, np.float32) if bias is None else bias)
        return ops.linear_fwd(dev(P), eye, b, act=a, save_pre=True)

    (y, pre), = [fwd(P) for P, _ in chunks(VF, rows, n)]
    Pm, _ = next(chunks(VF, rows, n))
    assert torch.equal(pre.cpu(), Pm), "precondition: the saved pre-activation is the sample points"
    held(name, "value", VF, host(y).reshape(-1)[:V.size], bounds, f"gemm n={n} {name}", mask=FIN)
    forward_with_nonfinite_bias(name, fwd, rows, n, bounds, f"gemm n={n} {name}")
    # derivative: dx = (dy @ W) * act'(aux), dy @ W == 1, aux = the whole vector (non-finite values included)
    Pa, _ = next(chunks(V, rows, n))
    dx = ops.linear_bwd_data(dev(one_hot(rows, n)), w1, act=a, aux=dev(Pa))
    held(name, "derivative", V, host(dx).reshape(-1)[:V.size], bounds, f"gemm n={n} {name}'")


# ---- split-K reduce (epi_store) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL8)
def test_gemm_f32_splitk_reduce_epilogue(ops, bounds, name):
    a, n = ops.ACT_IDS[name], 128
    rows = V.size // n
    eye, w1 = dev(torch.eye(n)), dev(ones_row(n, n))

    def fwd(P, bias=None):
        b = dev(np.zeros(n, np.float32) if bias is None else bias)
        y, pre = guard.full_nan((rows, n)), guard.full_nan((rows, n))
        ops.gemm(dev(P), eye, y, rows, n, n, transB=True, lda=n, ldb=n, ldc=n, bias=b, act=a, mode=ops.EPI_ACT,
                 preact=pre, ldpre=n, splitk=2)
        return y, pre

    Pm, _ = next(chunks(VF, rows, n))
    y, pre = fwd(Pm)
    assert torch.equal(pre.cpu(), Pm), "precondition: the saved pre-activation is the sample points"
    held(name, "value", VF, host(y).reshape(-1), bounds, f"split-K {name}", mask=FIN)
    forward_with_nonfinite_bias(name, fwd, rows, n, bounds, f"split-K {name}")
    Pa, _ = next(chunks(V, rows, n))
    dx = guard.full_nan((rows, n))
    ops.gemm(dev(one_hot(rows, n)), w1, dx, rows, n, n, transB=False, lda=n, ldb=n, ldc=n, act=a, mode=ops.EPI_DACT,
             aux=dev(Pa), ldaux=n, splitk=2)
    held(name, "derivative", V, host(dx).reshape(-1), bounds, f"split-K {name}'")


# ---- fp32 panel GEMM ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gelu", "silu"])
def test_gemm_panel_epilogue(ops, bounds, name):
    """(M, N, K) = (65, 64, 64) of test_gemm_panel_static_weight: the smallest N, and the smallest K a 64 x 64 identity fits"""
    a, M, n = ops.ACT_IDS[name], 65, 64
    assert ops.gemm_panel_supported(M, n, n)
    eye, w1 = dev(torch.eye(n)), dev(ones_row(n, n))
    pk = ops.PanelPacks([(eye, n, n, n, False), (w1, n, n, n, True)])
    pk.refresh()

    def fwd(P, bias=None):
        b = dev(np.zeros(n, np.float32) if bias is None else bias)
        return ops.gemm_panel(dev(P), pk.bufs[0], n, bias=b, act=a, mode=ops.EPI_ACT, save_pre=True)

    def fwd_checked(P):
        y, pre = fwd(P)
        assert torch.equal(pre.cpu(), P), "precondition: the saved pre-activation is the sample points"
        return (y,)

    y, = sweep(VF, M, n, fwd_checked)
    held(name, "value", VF, y, bounds, f"panel {name}", mask=FIN)
    forward_with_nonfinite_bias(name, fwd, M, n, bounds, f"panel {name}")
    dy = dev(one_hot(M, n))
    dx, = sweep(V, M, n, lambda P: (ops.gemm_panel(dy, pk.bufs[1], n, act=a, mode=ops.EPI_DACT, aux=dev(P))[0],))
    held(name, "derivative", V, dx, bounds, f"panel {name}'")


# ---- bf16 panel GEMM -----------------------------------------------------------------------------------------------------------
def _unpack_frag(pk, M, N):
    """act' pack in fragment order (csrc/gemm_bf16p.hip epi_fragment_direct) -> [M, N] fp32; as in test_gpu_ops.py"""
    t = pk.view(M // 32, N // 32, 2, 2, 32, 2, 4).float()
    return t.permute(0, 2, 5, 3, 6, 1, 4).reshape(M, N)


@pytest.mark.parametrize("name", ["gelu", "silu"])
def test_gemm_bf16p_three_plane_epilogue(ops, bounds, name):
    """(M, N, K) = (130, 512, 64) of test_gemm_bf16x6_panel_is_fp32_accurate, three planes: out[m, j] = act(P[m, j % 64])"""
    a, M, N, K = ops.ACT_IDS[name], 130, 512, 64
    assert ops.gemm_bf16p_supported(M, N, K)
    sel = torch.zeros(N, K)
    sel[torch.arange(N), torch.arange(N) % K] = 1.0
    pk = ops.PanelPacks([(dev(sel), N, K, K, False)], bf16=True, planes=3)
    pk.refresh()
    zero = dev(torch.zeros(N))

    def fwd(P):
        y, pre = ops.gemm_bf16p(ops.bf16_pack_rows(dev(P), planes=3), pk.bufs[0], M, N, K, bias=zero, act=a,
                                mode=ops.EPI_ACT, save_pre=True, planes=3)
        assert torch.equal(pre.cpu(), P.repeat(1, N // K)), "precondition: the saved pre-activation is the sample points"
        return y[:, :K], y[:, N - K:]

    y0, y7 = sweep(VB, M, K, fwd)
    held(name, "value", VB, y0, bounds, f"bf16p x3 {name}", mask=B16)
    held(name, "value", VB, y7, bounds, f"bf16p x3 {name} (last 64 columns)", mask=B16)
    # act' epilogue of the three-plane kernel: (dY W^T) == 1 exactly, aux (read in fp32) = the whole vector
    col0 = torch.zeros(N, K)
    col0[:, 0] = 1.0
    pk1 = ops.PanelPacks([(dev(col0), N, K, K, False)], bf16=True, planes=3)
    pk1.refresh()
    aux = torch.zeros(M, N)
    aux.view(-1)[:V.size] = torch.from_numpy(V)
    dx, _ = ops.gemm_bf16p(ops.bf16_pack_rows(dev(one_hot(M, K)), planes=3), pk1.bufs[0], M, N, K, act=a, mode=ops.EPI_DACT,
                           aux=dev(aux), planes=3)
    held(name, "derivative", V, host(dx).reshape(-1)[:V.size], bounds, f"bf16p x3 {name}' (aux)")


@pytest.mark.parametrize("name", ["gelu", "silu"])
def test_gemm_bf16p_one_plane_saved_derivative_and_packed_dact(ops, bounds, name):
    """(M, N, K) = (256, 512, 256) of test_gemm_bf16_panel_saved_activation_derivative, one plane: the points rounded to bf16
    pass the product exactly.  The act' pack holds bf16(act'(pre)): the rule, plus half a bf16 ulp for the pack's own rounding
    to nearest: bf16 keeps 8 significant bits, so half an ulp is 2^-9 of the binade's power of two, up to 2^-8 |ref| at the
    binade's lower end.  (The packed epilogues exist for one plane only: dpot_gemm_bf16p requires planes == 1 for them.)
    The act' epilogue reads aux in fp32: the whole vector, non-finite values included."""
    a, M, N, K = ops.ACT_IDS[name], 256, 512, 256
    v16 = torch.from_numpy(VB).bfloat16().float().numpy()
    A = torch.zeros(M, K)
    A.view(-1)[:V.size] = torch.from_numpy(v16)
    sel = torch.zeros(N, K)
    sel[torch.arange(N), torch.arange(N) % K] = 1.0
    col0 = torch.zeros(N, K)
    col0[:, 0] = 1.0
    pk = ops.PanelPacks([(dev(sel), N, K, K, False), (dev(col0), N, K, K, False)], bf16=True)
    pk.refresh()
    zero = dev(torch.zeros(N))
    Ap = ops.bf16_pack_rows(dev(A))
    y, pre = ops.gemm_bf16p(Ap, pk.bufs[0], M, N, K, bias=zero, act=a, mode=ops.EPI_ACT, save_pre=True)
    assert torch.equal(pre.cpu(), A.repeat(1, 2)), "precondition: the saved pre-activation is the bf16-rounded points"
    y2, D, _, _, _ = ops.gemm_bf16p_packed(Ap, pk.bufs[0], M, N, K, bias=zero, act=a, mode=ops.EPI_ACT, save_dact=True,
                                           pack_rows=True)
    assert torch.equal(y, y2)
    rows = V.size // K
    got = host(y)[:rows, :K].reshape(-1)
    held(name, "value", v16, got, bounds, f"bf16p x1 {name}", mask=B16)
    # saved act' (gelu: gelu_val_der): against float64 act' of the kernel's own pre-activation, to the rule + one bf16 ulp
    Dm = _unpack_frag(D, M, N)
    d = host(Dm)[:rows, :K].reshape(-1)
    held(name, "derivative", v16, d, bounds, f"bf16p x1 saved {name}'", mask=B16, extra_rel=2.0 ** -8)
    # act' epilogues: (dY W^T) == 1 exactly (dY one-hot in column 0, W's column 0 all ones)
    dYp = ops.bf16_pack_rows(dev(one_hot(M, K)))
    aux = torch.zeros(M, N)
    aux.view(-1)[:V.size] = torch.from_numpy(V)
    dx, _ = ops.gemm_bf16p(dYp, pk.bufs[1], M, N, K, act=a, mode=ops.EPI_DACT, aux=dev(aux))
    held(name, "derivative", V, host(dx).reshape(-1)[:V.size], bounds, f"bf16p x1 {name}' (aux)")
    out, _, _, _, _ = ops.gemm_bf16p_packed(dYp, pk.bufs[1], M, N, K, act=a, mode=ops.EPI_DACT, dact=D)
    assert torch.equal(out, Dm), "packed act' epilogue: 1 * the stored bf16 derivative, exactly"


# ---- AFNO mixer kernels --------------------------------------------------------------------------------------------------------
def _mixer(ops, bounds, name, nb, bs, M, layout, w_fwd, w_bwd, zero_b, fwd_mask, what):
    """forward: X = the points of fwd_mask (0 elsewhere) in the real half of every complex block (imaginary half 0: the
    three-product forms then add and subtract zeros only), both layers the identity, zero biases -> pre == X, mid = act(pre).
    backward: X = ones, both layers the identity -> (X Wa) == 1; aux = the whole vector (every form reads it in fp32) in
    every column: `pre` = act(aux) and mid = act'(aux) from one evaluation (gelu: gelu_val_der)."""
    a, N = ops.ACT_IDS[name], 2 * bs
    X = torch.zeros(M, nb, 2, bs)
    rows = -(-V.size // (nb * bs))
    assert rows <= M
    flat = torch.zeros(rows * nb * bs)
    pts = np.where(fwd_mask, V, np.float32(0))
    flat[:V.size] = torch.from_numpy(pts)
    X[:rows, :, 0, :] = flat.view(rows, nb, bs)
    X = X.view(M, nb * N)
    Y, pre, mid = ops.afno_mlp2(dev(X), w_fwd, zero_b, w_fwd, zero_b, nb, bs, a, mode=0, want_pre=True, want_mid=True,
                                layout=layout)
    assert torch.equal(pre.cpu(), X), f"{what}: precondition: the layer-1 pre-activation is the sample points"
    got = host(mid).reshape(M, nb, 2, bs)[:rows, :, 0, :].reshape(-1)[:V.size]
    held(name, "value", pts, got, bounds, f"{what} {name}", mask=fwd_mask)
    # backward with recomputation
    aux = torch.zeros(M * nb * N)
    aux[:V.size] = torch.from_numpy(V)
    aux = aux.view(M, nb * N)
    dS, o1, dmid = ops.afno_mlp2(dev(torch.ones(M, nb * N)), w_bwd, None, w_bwd, None, nb, bs, a, mode=1, aux=dev(aux),
                                 want_mid=True, want_pre=True, layout=layout)
    held(name, "value", V, host(o1).reshape(-1)[:V.size], bounds, f"{what} {name} re-derived by the backward")
    held(name, "derivative", V, host(dmid).reshape(-1)[:V.size], bounds, f"{what} {name}' of the backward")
    # forward again with NaN / inf in the first layer's bias (added in fp32 after the products): pre == X + bias exactly
    b = nf_bias(nb * N)
    _, pre, mid = ops.afno_mlp2(dev(X), w_fwd, dev(b.reshape(nb, N)), w_fwd, zero_b, nb, bs, a, mode=0, want_pre=True,
                                want_mid=True, layout=layout)
    with np.errstate(all="ignore"):
        want = (X.numpy() + b[None, :]).astype(np.float32)
    assert same_bits(pre, want), f"{what}: the pre-activation is not the sample points + bias"
    held(name, "value", want.reshape(-1), host(mid).reshape(-1), bounds, f"{what} {name} (non-finite bias)", floor=0.0)


@pytest.mark.parametrize("name", ["gelu", "silu", "relu"])
def test_afno_mixer_two_product(ops, bounds, name):
    nb, bs, M = 2, 64, 100                                   # of test_afno_mlp2_fused_two_layers
    assert ops.afno_mlp2_supported(nb, bs)
    N = 2 * bs
    wf, wb = ops.afno_block_weights(dev(torch.eye(N).repeat(nb, 1, 1)))
    _mixer(ops, bounds, name, nb, bs, M, 0, wf, wb, dev(torch.zeros(nb, N)), FIN, "mixer (four real products)")


def _complex_identity(nb, bs):
    w = torch.zeros(2, nb, bs, bs)
    w[0] = torch.eye(bs)
    return w, torch.zeros(2, nb, bs)


@pytest.mark.parametrize("name", ["gelu", "silu", "relu"])
def test_afno_mixer_three_product(ops, bounds, name):
    nb, bs, M = 2, 128, 333                                  # of test_afno_mlp3_three_product_form
    assert ops.afno_mlp2_supported(nb, bs) and ops.afno_mlp3_supported(nb, bs)
    w, b = _complex_identity(nb, bs)
    packs = ops.AfnoPacks([(dev(w), dev(b)), (dev(w), dev(b))])
    assert packs.layout == 1
    (wb1, bb1, f1, bw1), _ = packs.refresh()
    _mixer(ops, bounds, name, nb, bs, M, 1, f1, bw1, bb1, FIN, "mixer (three products)")


@pytest.mark.parametrize("name", ["gelu", "silu", "relu"])
def test_afno_mixer_bf16x6(ops, bounds, monkeypatch, name):
    nb, bs, M = 2, 128, 333                                  # of test_afno_mlp6_bf16x6_form
    set_tune(monkeypatch, mixer6=2)
    assert ops.afno_mlp6_supported(nb, bs)
    w, b = _complex_identity(nb, bs)
    with ops.precision_scope("auto", None):
        packs = ops.AfnoPacks([(dev(w), dev(b)), (dev(w), dev(b))])
        it1, _ = packs.refresh()
    assert it1.p6 is not None
    _mixer(ops, bounds, name, nb, bs, M, 2, it1.p6[0], it1.p6[1], it1[1], B16, "mixer (bf16x6)")


# ---- few-row linear --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gelu", "relu"])
def test_small_linear_epilogue(ops, bounds, monkeypatch, name):
    a, M, n = ops.ACT_IDS[name], 32, 512                     # (32, 512, 512) of test_small_linear_vs_fp64
    assert ops.small_linear_supported(M, n, n)
    set_tune(monkeypatch, fused_small=1)
    from dpot_amd import _lib
    lib, calls = _lib.load(), []
    entry = lib.dpot_small_linear
    monkeypatch.setattr(lib, "dpot_small_linear", lambda *args: (calls.append(1), entry(*args))[1])
    eye = dev(torch.eye(n))

    def fwd(P, bias=None):
        b = dev(np.zeros(n, np.float32) if bias is None else bias)
        return ops.linear_fwd(dev(P), eye, b, act=a, save_pre=True)

    P, _ = next(chunks(VF, M, n))
    y, pre = fwd(P)
    assert torch.equal(pre.cpu(), P), "precondition: the saved pre-activation is the sample points"
    held(name, "value", VF, host(y).reshape(-1)[:V.size], bounds, f"small_linear {name}", mask=FIN)
    forward_with_nonfinite_bias(name, fwd, M, n, bounds, f"small_linear {name}")
    assert len(calls) == 2, "both launches must have gone through dpot_small_linear, not the GEMM"


# ---- sites that do not expose the activation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("co", [4, 9])
@pytest.mark.parametrize("name", ["gelu", "silu"])
def test_out_tail(ops, bounds, name, co):
    """csrc/tail.hip (GELU template flag on and off): out = act(act(x) W2^T + b2) W4^T + b4 with W2 = I, b2 = 0, W4 = the
    one-hot rows of channels 0 .. co-1, b4 = 0, so out[pixel, c] = act(act(x[pixel, c])).  The site returns no pre-activation:
    route 2.  With u = act(x):  |got - act(act(x))| <= tol(u, act(u)) + sup|act'| tol(x, u)  (the second activation's own bound,
    plus the first one's carried through a function whose slope is at most sup|act'|).  Backward with dout = 1:
    dupre = act'(u) act'(x) for the selected channels, bounded by the product rule with sup|act'|, sup|act''| and one rounding.
    Finite points only in the sweep: the second layer multiplies every channel by W2, and 0 * inf would poison the pixel.
    NaN propagation is held by one more launch: a pixel whose 32 channels are all NaN must come out NaN in every output
    channel and in every selected channel of the backward, and every other pixel (x = 0) must stay exactly 0."""
    a, (B, h, w, P) = ops.ACT_IDS[name], (2, 3, 5, 4)
    npix = B * h * w * P * P
    assert ops.out_tail_supported(32, co, npix)
    l1, l2 = AR.LIP[name]                                      # held to float64 by tests/test_cpu_activations.py
    w2, b2 = dev(torch.eye(32)), dev(torch.zeros(32))
    w4 = torch.zeros(co, 32)
    w4[torch.arange(co), torch.arange(co)] = 1.0
    w4p, b4p = ops.out_tail_pad(dev(w4), dev(torch.zeros(co)), co)
    dout = dev(torch.ones(B, h * P, w * P, co))

    def unshuffle(t):
        return t.view(B, h, P, w, P, co).permute(0, 1, 3, 2, 4, 5).reshape(npix, co)

    def run(Pm):
        x = torch.zeros(npix, 32)
        x[:, :co] = Pm
        xd = dev(x)
        out = ops.out_tail_fwd(xd, w2, b2, w4p, b4p, B, h, w, P, co, a)
        dupre, _ = ops.out_tail_bwd(xd, dout, w2, b2, w4p, B, h, w, P, co, a)
        return unshuffle(out), dupre[:, :co]

    got, dgot = sweep(VF, npix, co, run)
    x = VF[FIN]
    u, du = AR.reference(name, x)
    u32 = u.astype(np.float32)
    ref, d2 = AR.reference(name, u32)                          # act(u), act'(u) at the float32 nearest to u
    t1v, t1d = bounds.tol(name, "value", x, u), bounds.tol(name, "derivative", x, du)
    tol = bounds.tol(name, "value", u32, ref) + l1 * (t1v + AR.ulp32(u))
    err = np.abs(got[FIN].astype(np.float64) - ref)
    print(f"tail co={co} {name}({name}): {x.size} points, max |err| {err.max():.3e}, worst ratio {(err / tol).max():.3f}")
    assert (err <= tol).all(), f"tail fwd: x = {x[np.argmax(err / tol)]!r}: {(err / tol).max():.3f} of the bound"
    dref = d2 * du
    dtol = l1 * (bounds.tol(name, "derivative", u32, d2) + l2 * (t1v + AR.ulp32(u))) + l1 * t1d + AR.ulp32(dref)
    derr = np.abs(dgot[FIN].astype(np.float64) - dref)
    print(f"tail co={co} {name}'({name}) {name}': max |err| {derr.max():.3e}, worst ratio {(derr / dtol).max():.3f}")
    assert (derr <= dtol).all(), f"tail bwd: x = {x[np.argmax(derr / dtol)]!r}: {(derr / dtol).max():.3f} of the bound"
    assert x.size >= 0.95 * V.size
    xn = torch.zeros(npix, 32)
    xn[7, :] = float("nan")
    xd = dev(xn)
    on = host(unshuffle(ops.out_tail_fwd(xd, w2, b2, w4p, b4p, B, h, w, P, co, a)))
    dn = host(ops.out_tail_bwd(xd, dout, w2, b2, w4p, B, h, w, P, co, a)[0])[:, :co]
    assert np.isnan(on[7]).all() and np.isnan(dn[7]).all(), "tail: a NaN pixel must give NaN"
    others = np.arange(npix) != 7
    assert (on[others] == 0).all() and np.isfinite(dn[others]).all(), "tail: a NaN pixel leaked into another pixel"


@pytest.mark.parametrize("name", ["gelu", "silu"])
def test_implicit_patch_embed(ops, bounds, name):
    """csrc/embed.hip at (B, X, Y, T, hid) = (2, 32, 32, 10, 35) of test_implicit_patch_embed_matches_patch_matrix_path (gelu: the
    float4 branch): x = 0, so the patch product is exactly 0 and Hpre is the bias table, which holds the sample points, NaN
    and inf included.  Route 1: the site returns Hpre; it is asserted to be the table, bit for bit, and Hh is held to the rule."""
    from dpot_amd import functional as F
    a, (B, X, Y, T, hid), Cc, P = ops.ACT_IDS[name], (2, 32, 32, 10, 35), 4, 8
    assert ops.embed_supported(Cc, P, T, hid, Y // P)
    hidp = (hid + 3) // 4 * 4
    g = torch.Generator().manual_seed(2)
    w0 = dev(torch.randn(hid, Cc + 3, P, P, generator=g) * 0.06)
    wfrag = ops.embed_pack_w0(w0)
    x = dev(torch.zeros(B, X, Y, T, Cc))
    rows = F.embed_grid_matrix(dev(torch.linspace(0, 1, X)), dev(torch.linspace(0, 1, Y)), dev(torch.linspace(0, 1, T)),
                               X, Y, T, Cc, P).shape[0]

    def run(Pm):
        bt = torch.zeros(rows, hidp)
        bt[:, :hid] = Pm
        Hh, Hpre = ops.embed_fwd(x, wfrag, dev(bt), hidp, a)
        assert same_bits(Hpre[:rows], bt.numpy()) and same_bits(Hpre[rows:2 * rows], bt.numpy()), \
            "precondition: the returned pre-activation is the bias table"
        return (Hh[rows:2 * rows, :hid],)

    got, = sweep(V, rows, hid, run)
    held(name, "value", V, got, bounds, f"embed {name}")


def test_afno_layer_one_launch(ops, bounds, monkeypatch):
    """csrc/afno_fused.hip (its own `ACTK == DPOT_ACT_GELU ? gelu_fwd : act_fwd`) at (E, nb, B) = (512, 4, 2) without the norms,
    the norm-free case of test_afno_layer_one_launch_vs_three_launches: y1 = irfft2(W2 act(W1 rfft2(x) + 0) + 0) + x with both
    layers the complex identity.  The pre-activation passes through the kernel's own fp32 DFT, so it is not exact.  Route 1:
    the site returns it, and y1 is compared with the float64 composition irfft2(act(pre)) + x of the RETURNED pre.

    What is driven.  Every (sample, channel) carries ONE sample point p, alone in the real or the imaginary part of one mode
    (kx, ky), 0 < ky < 8 (those columns have no conjugate partner inside the half spectrum): x = irfft2 of that spectrum in
    float64, a cosine of amplitude p / 8.  The returned pre at that mode is asserted to be p to the DFT's round-off
    (64 u |p|, u = 2^-24: the bound on the inverse transform below, twice, for the float64 -> float32 rounding of x and the
    forward transform), so the sweep does cover the vector; what the other 287 entries of that channel's spectrum hold
    (round-off of the order u |p|) is taken from the returned pre as well.  y1 then shows act(p) / 8 in every pixel.
    Finite |p| <= 1e36 (the DFTs sum 256 terms before they scale by 1 / 16); NaN and inf would fill the whole image.

    The bound, per (sample, channel), for every pixel, with m = 1 for ky in {0, 8} and 2 otherwise:
        sum over modes of m / 16 * [tol(act, pre_re) + tol(act, pre_im) + (2 + 32) u (|act re| + |act im|)] + ulp32(y1)
    - tol is the rule's bound of each activated entry (each reaches a pixel with weight at most m / 16);
    - 2 u: the identity second layer in three-product form returns re exactly and im = ((re + im) - re), two roundings;
    - 32 u: an entry reaches a pixel through log2(256) = 8 radix-2 levels of butterflies, each at most a complex twiddle
      product (3 u with the constant's own rounding) and a sum (u); the scale 1 / 16 is exact;
    - ulp32(y1): the sum with x and the store."""
    name = "gelu"
    set_tune(monkeypatch, afno_layer=1)
    a, (E, nb, B, h, wf) = ops.ACT_IDS[name], (512, 4, 2, 16, 9)
    bs, u = E // nb, 2.0 ** -24
    assert ops.afno_fused_supported(h, h, E, nb, h, wf, G=0)
    wI, bI = _complex_identity(nb, bs)
    packs = ops.AfnoPacks([(dev(wI), dev(bI)), (dev(wI), dev(bI))])
    assert packs.layout == 1
    l1, l2 = packs.refresh()
    use = FIN & (np.abs(VF) <= 1e36)
    pts = V[use]
    bi, ci = np.meshgrid(np.arange(B), np.arange(E), indexing="ij")
    kx, ky, imag = ci % 16, 1 + (ci // 16) % 7, (bi + ci) % 2 == 1
    mult = np.full(wf, 2.0)
    mult[0] = mult[-1] = 1.0
    n, worst, worst12 = 0, 0.0, 0.0
    for s in range(0, pts.size, B * E):
        c = pts[s:s + B * E]
        p = np.zeros(B * E, np.float32)
        p[:c.size] = c
        p = p.reshape(B, E)
        Z = np.zeros((B, h, wf, E), np.complex128)
        Z[bi, kx, ky, ci] = np.where(imag, 1j, 1.0) * p.astype(np.float64)
        x = torch.fft.irfft2(torch.from_numpy(Z), s=(h, h), dim=(1, 2), norm="ortho").reshape(B, h * h, E).float()
        _, pre, y1, *_ = ops.afno_fused_fwd(dev(x), None, None, l1[2], l1[1], l2[2], l2[1], None, None, h, h, nb, h, wf, a)
        pre = host(pre).reshape(B, h, wf, nb, 2, bs)
        pr, pi = pre[:, :, :, :, 0, :].reshape(B, h, wf, E), pre[:, :, :, :, 1, :].reshape(B, h, wf, E)
        seen = np.where(imag, pi[bi, kx, ky, ci], pr[bi, kx, ky, ci]).astype(np.float64)
        off = np.abs(seen - p) - (64 * u * np.abs(p.astype(np.float64)) + 16 * AR.FLT_MIN)
        assert (off <= 0).all(), f"one-launch layer: precondition: the returned pre-activation is not the points ({off.max():.3e})"
        mr = AR.reference(name, pr.reshape(-1))[0].reshape(pr.shape)
        mi = AR.reference(name, pi.reshape(-1))[0].reshape(pi.shape)
        te = (bounds.tol(name, "value", pr, mr) + bounds.tol(name, "value", pi, mi) + 34 * u * (np.abs(mr) + np.abs(mi)))
        T = (te * mult[None, None, :, None]).sum(axis=(1, 2)) / 16.0                       # [B, E]
        o2 = torch.complex(torch.from_numpy(mr), torch.from_numpy(mi))
        yref = torch.fft.irfft2(o2, s=(h, h), dim=(1, 2), norm="ortho").reshape(B, h * h, E) + x.double()
        yref = yref.numpy()
        tol = T[:, None, :] + AR.ulp32(yref)
        err = np.abs(host(y1).astype(np.float64) - yref)
        ratio = err / tol
        if not (ratio <= 1.0).all():
            b_, t_, c_ = np.unravel_index(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio)), ratio.shape)
            raise AssertionError(f"one-launch layer: point {p[b_, c_]!r} (sample {b_}, channel {c_}, pixel {t_}): got "
                                 f"{host(y1)[b_, t_, c_]!r}, float64 composition {yref[b_, t_, c_]!r}, bound {tol[b_, t_, c_]:.3e}")
        worst = max(worst, float(ratio.max()))
        small = np.abs(p) <= 12
        worst12 = max(worst12, float((err * small[:, None, :]).max()))
        n += c.size
    print(f"one-launch layer {name}: {n} points, worst ratio to the bound {worst:.3f}, max |y1 err| for |p| <= 12 {worst12:.3e}")
    assert n >= 0.95 * V.size
