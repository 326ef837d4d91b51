"""The weight gradients of several DPOT blocks per launch (csrc/gemm_tn.hip: dpot_mlp_wgrad_batch, dpot_afno_wgrad_batch,
dpot_wgrad_batch_finalize; functional.WgradBatch): the batched entry points against float64 on the host under the guarded,
NaN-poisoned allocator (an unwritten partial slot or a stray write fails), bit-reproducibility, and a three-block model
whose backward takes the batched path against the per-block schedule (DPOT_TUNE fused_small=2) and the CPU oracle."""
import os
import subprocess
import sys
from collections import OrderedDict

import pytest
import torch

import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close, set_tune
from oracle import dpot_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def dev(t):
    return guard.wrap(t, "cuda")


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).float()


# ------------------------------------------------------------------------------------------------------
# T = 224: 7 slabs, ragged over 2 (4 + 3) and 3 (3 + 3 + 1) token ranges; n = 3: an odd number of blocks (6 sets over 8 XCDs);
# n = 17: more blocks than one problem table holds (two launches of the GEMM kernel and of the finalising kernel)
@pytest.mark.parametrize("n,T,E,mh,splits", [(3, 224, 128, 256, 2), (3, 224, 128, 256, 3), (1, 64, 128, 256, 0),
                                             (1, 64, 128, 256, 2), (17, 64, 128, 128, 0)])
def test_mlp_wgrad_batch_vs_float64(ops, n, T, E, mh, splits):
    """dpot_mlp_wgrad_batch + dpot_wgrad_batch_finalize: dW2 = do2^T Hh, db2, dW1 = dHpre^T xn2, db1 of n blocks; the
    tolerance of tests/test_gpu_ops.py::test_mlp_wgrad2_both_layers_one_launch"""
    sk = splits or ops.mlp_wgrad_batch_splitk(T, E, mh, n)
    assert sk >= 1
    host = [(rnd(T, E, seed=10 * i + 1), rnd(T, mh, seed=10 * i + 2), rnd(T, E, seed=10 * i + 3), rnd(T, mh, seed=10 * i + 4))
            for i in range(n)]
    on_dev = [tuple(dev(t) for t in blk) for blk in host]

    def run():
        outs = [(guard.full_nan((E, mh)), guard.full_nan((E,)), guard.full_nan((mh, E)), guard.full_nan((mh,)))
                for _ in range(n)]
        ws = ops.mlp_wgrad_batch(*[[blk[k] for blk in on_dev] for k in range(4)], sk)
        ops.wgrad_batch_finalize(None, (ws, sk, E, mh, outs), [[] for _ in range(n)])
        return outs

    outs = run()
    for i, ((do2, Hh, xn2, dH), (dW2, db2, dW1, db1)) in enumerate(zip(host, outs)):
        assert_close(dW2, do2.double().t() @ Hh.double(), f"block {i} dW2", rtol=2e-5, atol_scale=2e-6)
        assert_close(dW1, dH.double().t() @ xn2.double(), f"block {i} dW1", rtol=2e-5, atol_scale=2e-6)
        assert_close(db2, do2.double().sum(0), f"block {i} db2", rtol=2e-5, atol_scale=2e-6)
        assert_close(db1, dH.double().sum(0), f"block {i} db1", rtol=2e-5, atol_scale=2e-6)
    # again on fresh NaN-poisoned workspaces and outputs: the same bits (fixed summation order, no state between calls)
    for a, b in zip(run(), outs):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# Mm = 288 (9 slabs: the smallest 128-channel case of test_afno_wgrad2_both_layers_one_launch; token-limited split (1, 2),
# ranges of 5 + 4 slabs) and 928 (29 slabs: 5 ranges of 6 for P1 / P2 (6 + 6 + 6 + 6 + 5), 6 of 5 for the sum product
# (5 x 5 + 4)); per_launch 2: the three blocks cut into launches of 2 + 1
@pytest.mark.parametrize("Mm,per_launch", [(288, 0), (928, 0), (928, 2)])
def test_afno_wgrad_batch_vs_float64(ops, Mm, per_launch):
    """dpot_afno_wgrad_batch (three-product form) + dpot_wgrad_batch_finalize for n = 3 blocks, nb = 2, bs = 128, against
    float64 complex arithmetic; the tolerance of tests/test_gpu_ops.py::test_afno_wgrad2_both_layers_one_launch"""
    n, nb, bs = 3, 2, 128
    N = 2 * bs
    per, s12, sk = ops.afno_wgrad_batch_plan(Mm, nb, bs, n)
    assert per == 3 and 1 <= s12 <= sk and 2 * n * nb * (2 * s12 + sk) <= 256, (per, s12, sk)
    per = per_launch or per
    host = [tuple(rnd(Mm, nb * N, seed=10 * i + k) for k in (1, 2, 3, 4)) for i in range(n)]
    on_dev = [tuple(dev(t) for t in blk) for blk in host]

    def run():
        outs = [(guard.full_nan((2, nb, bs, bs)), guard.full_nan((2, nb, bs)), guard.full_nan((2, nb, bs, bs)),
                 guard.full_nan((2, nb, bs))) for _ in range(n)]
        ws = ops.afno_wgrad_batch(*[[blk[k] for blk in on_dev] for k in range(4)], nb, bs, per, s12, sk)
        ops.wgrad_batch_finalize((ws, s12, sk, nb, bs, outs), None, [[] for _ in range(n)])
        return outs

    def ref(A, Bm):
        Ac = A.double().view(Mm, nb, 2, bs)
        Bc = Bm.double().view(Mm, nb, 2, bs)
        Ar, Ai, Br, Bi = Ac[:, :, 0], Ac[:, :, 1], Bc[:, :, 0], Bc[:, :, 1]
        e = lambda x, y: torch.einsum("mki,mko->kio", x, y)
        return torch.stack([e(Ar, Br) + e(Ai, Bi), e(Ar, Bi) - e(Ai, Br)]), torch.stack([Br.sum(0), Bi.sum(0)])

    outs = run()
    for i, ((S, dO1, O1, dO2), (dw1, db1, dw2, db2)) in enumerate(zip(host, outs)):
        for dw, db, A, Bm, nm in ((dw1, db1, S, dO1, "layer 1"), (dw2, db2, O1, dO2, "layer 2")):
            rw, rb = ref(A, Bm)
            assert_close(dw, rw, f"block {i} dw {nm}", rtol=2e-5, atol_scale=2e-6)
            assert_close(db, rb, f"block {i} db {nm}", rtol=2e-5, atol_scale=2e-6)
    for a, b in zip(run(), outs):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------
# the smallest model whose blocks take the batched path: 128 channels per AFNO block (embed 256 / 2), a 16 x 16 latent grid
# (Mm = 2 * 16 * 9 = 288 spectral tokens, 512 tokens), three blocks, batch 2
MODEL_KW = dict(R.TINY, embed_dim=256, n_blocks=2, depth=3)
MODEL_B = 2


def _model_inputs(T_ar, kw=None):
    cfg = R.DPOTConfig(**(kw or MODEL_KW))
    S = cfg.img_size
    xx = R.recipe_input((MODEL_B, S, S, cfg.in_timesteps, cfg.in_channels), salt=81)
    yy = R.recipe_input((MODEL_B, S, S, T_ar, cfg.out_channels), salt=82)
    msk = torch.ones(MODEL_B, S, S, 1, cfg.out_channels)
    return cfg, xx, yy, msk


_ORACLE = {}


def _oracle_grads(T_ar):
    """the CPU oracle's rollout loss and every parameter gradient: computed once per T_ar, shared, left unchanged"""
    if T_ar not in _ORACLE:
        cfg, xx, yy, msk = _model_inputs(T_ar)
        sd = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in R.recipe_state_dict(cfg, salt=6).items())
        loss, _ = R.rollout_loss(sd, xx, yy, msk, cfg)
        loss.backward()
        _ORACLE[T_ar] = (loss.item(), OrderedDict((k, v.grad) for k, v in sd.items()))
    return _ORACLE[T_ar]


def _gpu_grads(monkeypatch, T_ar, fused_small, recompute=False, hook=False, kw=None):
    """one rollout + backward on flat-bound parameters; returns (loss, {name: grad}, finalising launches of the batched /
    of the per-block kind)"""
    from dpot_amd import DPOTNet, ops
    from dpot_amd.train import FlatParams, rollout
    set_tune(monkeypatch, fused_small=fused_small)
    kw = kw or MODEL_KW
    cfg, xx, yy, msk = _model_inputs(T_ar, kw)
    m = DPOTNet(**kw)
    m.load_state_dict(R.recipe_state_dict(cfg, salt=6))
    m.cuda()
    m.recompute_blocks = recompute
    if hook:
        m._boundary_hook = lambda b, lat: lat
    fp = FlatParams(m)
    fp.zero_grad()
    calls = {"batch": 0, "block": 0}
    real_b, real_f = ops.wgrad_batch_finalize, ops.block_finalize
    monkeypatch.setattr(ops, "wgrad_batch_finalize", lambda *a: (calls.__setitem__("batch", calls["batch"] + 1), real_b(*a))[1])
    monkeypatch.setattr(ops, "block_finalize", lambda *a: (calls.__setitem__("block", calls["block"] + 1), real_f(*a))[1])
    loss, _ = rollout(m, xx.cuda(), yy.cuda(), msk.cuda())
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "wgrad_batch_finalize", real_b)
    monkeypatch.setattr(ops, "block_finalize", real_f)
    left = [k for k, p in zip(fp.names, fp.pending) if p != 0 and not k.startswith("cls_head.")]
    assert not left, f"gradient sinks never delivered: {left}"
    grads = OrderedDict((k, p.grad.clone()) for k, p in m.named_parameters() if not k.startswith("cls_head."))
    return loss.item(), grads, calls


def _batch_expected():
    """does this process's library batch at all?  (DPOT_TUNE wgrad_gauss=0 / panel=0, read once by the C side, turn the
    batched plan off: the per-block path runs)"""
    from dpot_amd import _lib
    lib = _lib.load()
    return lib.dpot_tune(b"wgrad_gauss", 1) != 0 and lib.dpot_tune(b"panel", 1) != 0


@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("T_ar", [1, 2])
def test_model_batched_vs_per_block_and_oracle(monkeypatch, T_ar, mode):
    """every parameter gradient after one backward: batched schedule (fused_small=1: the per-block token ranges; 3: the
    one-round rules) against the per-block one (fused_small=2) and both against the CPU oracle, at the model-level tolerance
    of tests/test_gpu_sizes.py (rtol 1e-4); T_ar = 2: one batch per pass, the second one accumulates into the slots"""
    depth = MODEL_KW["depth"]
    la, ga, ca = _gpu_grads(monkeypatch, T_ar, mode)
    lb, gb, cb = _gpu_grads(monkeypatch, T_ar, 2)
    if _batch_expected():
        assert ca == {"batch": T_ar, "block": 0}, ca           # ONE finalising launch per pass through the blocks
    else:
        assert ca == {"batch": 0, "block": T_ar * depth}, ca
    assert cb == {"batch": 0, "block": T_ar * depth}, cb
    l_ref, g_ref = _oracle_grads(T_ar)
    assert abs(la - l_ref) <= 1e-4 * abs(l_ref) and abs(lb - l_ref) <= 1e-4 * abs(l_ref)
    for k in ga:
        assert_close(ga[k], gb[k], f"T_ar={T_ar} d{k}: batched vs per-block")
        assert_close(ga[k], g_ref[k], f"T_ar={T_ar} d{k}: batched vs oracle")
        assert_close(gb[k], g_ref[k], f"T_ar={T_ar} d{k}: per-block vs oracle")
        if mode == 1:
            assert torch.equal(ga[k], gb[k]), f"T_ar={T_ar} d{k}: the default batch must not change a bit"


def test_default_batch_is_bit_identical_where_the_one_round_rule_is_not(monkeypatch):
    """DPOT-Tiny's blocks (embed 512, nb = 4) at batch 2, T_ar = 2: the one-round rule cuts the channel-MLP tokens into 2
    ranges where a per-block launch cuts them into 4 - fused_small=3 differs from the per-block schedule in the last bits
    (and stays within the model-level tolerance), the default batch (several rounds, per-block ranges) in none"""
    _, g_blk, _ = _gpu_grads(monkeypatch, 2, 2, kw=R.TINY)
    _, g_def, c_def = _gpu_grads(monkeypatch, 2, 1, kw=R.TINY)
    _, g_one, c_one = _gpu_grads(monkeypatch, 2, 3, kw=R.TINY)
    if _batch_expected():
        assert c_def == {"batch": 2, "block": 0} and c_one == {"batch": 2, "block": 0}, (c_def, c_one)
        assert any(not torch.equal(g_one[k], g_blk[k]) for k in g_blk if ".mlp." in k)
    for k in g_blk:
        assert torch.equal(g_def[k], g_blk[k]), k
        assert_close(g_one[k], g_blk[k], f"d{k}: one-round batch vs per-block")


@pytest.mark.parametrize("mode", [1, 3])
def test_model_batched_backward_is_reproducible(monkeypatch, mode):
    _, ga, _ = _gpu_grads(monkeypatch, 1, mode)
    _, gb, _ = _gpu_grads(monkeypatch, 1, mode)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def test_no_batch_with_boundary_hook_or_recompute(monkeypatch):
    """the segmented data-parallel step (a _boundary_hook is set) and activation recomputation keep the per-block schedule"""
    depth = MODEL_KW["depth"]
    _, g0, _ = _gpu_grads(monkeypatch, 1, 2)
    for kw in (dict(hook=True), dict(recompute=True)):
        for mode in (1, 3):
            _, g, calls = _gpu_grads(monkeypatch, 1, mode, **kw)
            assert calls == {"batch": 0, "block": depth}, (kw, mode, calls)
            for k in g:
                assert torch.equal(g[k], g0[k]), (kw, mode, k)


def test_model_falls_back_per_block_without_the_three_product_form():
    """DPOT_TUNE=wgrad_gauss=0 (read once per process by the C library: a child process): the batched launches cover nothing,
    the model-level test above must pass on the per-block path"""
    env = dict(os.environ)
    cur = [kv for kv in env.get("DPOT_TUNE", "").split(",") if kv and not kv.startswith("wgrad_gauss=")]
    env["DPOT_TUNE"] = ",".join(cur + ["wgrad_gauss=0"])
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_wgrad_batch.py",
           "-k", "test_model_batched_vs_per_block_and_oracle and 1-1"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:]
