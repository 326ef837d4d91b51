"""Chained token ranges in the batched weight gradients (csrc/gemm_tn.hip gemm_tn_chain_kernel, tn_sum_nodes): a workgroup
walks 2 or 4 consecutive token ranges, restarts its accumulators at every range boundary and adds the ranges' tiles in the
association of the finalising launch's summation tree.  Nothing may change a bit: every comparison of a chain against chain 1
is torch.equal; chain 1 itself is held to float64.  All of it on the guarded, NaN-poisoned allocator (tests/guard.py): a
workspace slot that is read without having been written, or a store outside the node-sized workspace, fails the test.

Shapes: ragged in every way the node cutting can be - a last range shorter than the others, a last node of one range, a pair
behind a full group of eight, P1 / P2 and the sum product cut differently (10 and 12 ranges: nodes of 4, 4, 2 and 4, 4, 2, 2)."""
import pytest
import torch

import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close, set_tune
from oracle import dpot_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dpot_amd import _lib
    from dpot_amd import ops as _ops
    lib = _lib.load()
    assert torch.cuda.is_available()
    if lib.dpot_tune(b"wgrad_gauss", 1) == 0 or lib.dpot_tune(b"panel", 1) == 0:
        pytest.fail("this process's DPOT_TUNE turns the batched weight gradients off: nothing to chain")
    return _ops


@pytest.fixture(autouse=True)
def _guard(guarded):
    yield guarded


def dev(t):
    return guard.wrap(t, "cuda")


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).float()


def _ranges(ops, T, splits):
    from dpot_amd import _lib
    import ctypes as C
    f, n = C.c_int(0), C.c_int(0)
    out = []
    for i in range(splits):
        assert _lib.load().dpot_tn_split_range(T, splits, i, C.byref(f), C.byref(n)) == 0
        out.append(n.value // 32)
    return out


# ------------------------------------------------------------------------------------------------------
# T = 480: 15 slabs over 8 ranges (seven of 2 slabs, a last one of 1): one full group - pairs / quads, the last node ragged
# T = 352: 11 slabs over 3 ranges (4 + 4 + 3): no full group - a pair and an odd single, at chain 2 and at chain 4
MLP_CASES = [(480, 8), (352, 3)]


def _mlp_run(ops, on_dev, n, E, mh, sk, chain):
    outs = [(guard.full_nan((E, mh)), guard.full_nan((E,)), guard.full_nan((mh, E)), guard.full_nan((mh,))) for _ in range(n)]
    ws = ops.mlp_wgrad_batch(*[[blk[k] for blk in on_dev] for k in range(4)], sk, chain)
    assert ws.shape[1] * 4 == ops.tn_chain_count(sk, chain) * 2 * (E * mh + max(E, mh)) * 4
    ops.wgrad_batch_finalize(None, (ws, sk, E, mh, outs), [[] for _ in range(n)], chain, 1)
    return outs


@pytest.mark.parametrize("T,sk", MLP_CASES)
def test_mlp_chain_is_bit_identical(ops, T, sk):
    n, E, mh = 3, 128, 256
    assert _ranges(ops, T, sk) == ([2] * 7 + [1] if T == 480 else [4, 4, 3])
    host = [(rnd(T, E, seed=10 * i + 1), rnd(T, mh, seed=10 * i + 2), rnd(T, E, seed=10 * i + 3), rnd(T, mh, seed=10 * i + 4))
            for i in range(n)]
    on_dev = [tuple(dev(t) for t in blk) for blk in host]
    base = _mlp_run(ops, on_dev, n, E, mh, sk, 1)
    # chain 1 against float64, the tolerance of test_gpu_wgrad_batch.py::test_mlp_wgrad_batch_vs_float64
    for i, ((do2, Hh, xn2, dH), (dW2, db2, dW1, db1)) in enumerate(zip(host, base)):
        assert_close(dW2, do2.double().t() @ Hh.double(), f"block {i} dW2", rtol=2e-5, atol_scale=2e-6)
        assert_close(dW1, dH.double().t() @ xn2.double(), f"block {i} dW1", rtol=2e-5, atol_scale=2e-6)
        assert_close(db2, do2.double().sum(0), f"block {i} db2", rtol=2e-5, atol_scale=2e-6)
        assert_close(db1, dH.double().sum(0), f"block {i} db1", rtol=2e-5, atol_scale=2e-6)
    for chain in (1, 2, 4):
        for rep in range(2):                        # twice: fresh poisoned workspaces and outputs, the same bits
            got = _mlp_run(ops, on_dev, n, E, mh, sk, chain)
            for i, (a, b) in enumerate(zip(got, base)):
                for x, y, nm in zip(a, b, ("dW2", "db2", "dW1", "db1")):
                    assert torch.equal(x, y), f"chain {chain} run {rep} block {i} {nm}: {(x != y).sum().item()} elements differ"


# ------------------------------------------------------------------------------------------------------
# Mm = 1856: 58 slabs; P1 / P2 in 10 ranges (nine of 6, one of 4), the sum product in 12 (eleven of 5, one of 3): a full group
# plus one / two pairs.  Mm = 928: 29 slabs at the planned (5, 6) - no full group, pairs and an odd single
# Mm = 1024: 32 slabs at (6, 8) - what the per-block rule gives 8 sum-product ranges.  At chain 4 the six P1 / P2 ranges are THREE
# pairs, the eight sum-product ranges TWO quads: more nodes for fewer ranges, the workspace must go by the larger count
AFNO_CASES = [(1856, 10, 12), (928, 5, 6), (1024, 6, 8)]


def _afno_run(ops, on_dev, n, nb, bs, per, s12, sk, chain):
    outs = [(guard.full_nan((2, nb, bs, bs)), guard.full_nan((2, nb, bs)), guard.full_nan((2, nb, bs, bs)),
             guard.full_nan((2, nb, bs))) for _ in range(n)]
    ws = ops.afno_wgrad_batch(*[[blk[k] for blk in on_dev] for k in range(4)], nb, bs, per, s12, sk, chain)
    slots = max(ops.tn_chain_count(sk, chain), ops.tn_chain_count(s12, chain))
    assert ws.shape[1] == slots * 2 * nb * (3 * bs * bs + 2 * bs)
    ops.wgrad_batch_finalize((ws, s12, sk, nb, bs, outs), None, [[] for _ in range(n)], 1, chain)
    return outs


@pytest.mark.parametrize("Mm,s12,sk", AFNO_CASES)
def test_afno_chain_is_bit_identical(ops, Mm, s12, sk):
    n, nb, bs = 3, 2, 128
    N = 2 * bs
    if Mm == 1856:
        assert _ranges(ops, Mm, s12) == [6] * 9 + [4] and _ranges(ops, Mm, sk) == [5] * 11 + [3]
    elif Mm == 928:
        assert ops.afno_wgrad_batch_plan(Mm, nb, bs, n)[1:] == (s12, sk)
    else:
        assert _ranges(ops, Mm, s12) == [6] * 5 + [2] and _ranges(ops, Mm, sk) == [4] * 8
        assert ops.afno_wgrad2_splits12(Mm, bs, sk) == s12
        assert ops.tn_chain_count(s12, 4) == 3 > ops.tn_chain_count(sk, 4) == 2
    host = [tuple(rnd(Mm, nb * N, seed=10 * i + k) for k in (1, 2, 3, 4)) for i in range(n)]
    on_dev = [tuple(dev(t) for t in blk) for blk in host]
    base = _afno_run(ops, on_dev, n, nb, bs, 1, s12, sk, 1)
    # chain 1 against float64 (test_gpu_wgrad_batch.py::test_afno_wgrad_batch_vs_float64): the chains are compared with THIS
    S, dO1 = host[0][0].double().view(Mm, nb, 2, bs), host[0][1].double().view(Mm, nb, 2, bs)
    e = lambda x, y: torch.einsum("mki,mko->kio", x, y)
    assert_close(base[0][0], torch.stack([e(S[:, :, 0], dO1[:, :, 0]) + e(S[:, :, 1], dO1[:, :, 1]),
                                          e(S[:, :, 0], dO1[:, :, 1]) - e(S[:, :, 1], dO1[:, :, 0])]), "dw1, block 0",
                 rtol=2e-5, atol_scale=2e-6)
    assert_close(base[0][1], torch.stack([dO1[:, :, 0].sum(0), dO1[:, :, 1].sum(0)]), "db1, block 0", rtol=2e-5, atol_scale=2e-6)
    for per in (1, 2):
        for chain in (1, 2, 4):
            for rep in range(2):
                got = _afno_run(ops, on_dev, n, nb, bs, per, s12, sk, chain)
                for i, (a, b) in enumerate(zip(got, base)):
                    for x, y, nm in zip(a, b, ("dw1", "db1", "dw2", "db2")):
                        assert torch.equal(x, y), (f"chain {chain}, {per} per launch, run {rep}, block {i} {nm}: "
                                                   f"{(x != y).sum().item()} elements differ")


def test_entry_points_refuse_other_chains(ops):
    """by return code only: nothing is launched"""
    from dpot_amd import _lib
    lib = _lib.load()
    t = dev(rnd(64, 128))
    arr = ops._ptr_array([t])
    for chain in (0, 3, 8):
        assert lib.dpot_mlp_wgrad_batch(arr, arr, arr, arr, 1, 64, 128, 128, t.data_ptr(), 1, chain, None) != 0
        assert lib.dpot_afno_wgrad_batch(arr, arr, arr, arr, 1, 256, 64, 1, 128, t.data_ptr(), 1, 1, 1, chain, None) != 0
        blocks = (_lib.WgradBlock * 1)()
        assert lib.dpot_wgrad_batch_finalize(blocks, 1, 1, 1, 1, 128, 1, 128, 128, 0, 0, 0, chain, 1, None) != 0
        assert lib.dpot_wgrad_batch_finalize(blocks, 1, 1, 1, 1, 128, 1, 128, 128, 0, 0, 0, 1, chain, None) != 0


# ------------------------------------------------------------------------------------------------------
# the three-block model of test_gpu_wgrad_batch.py: 128 channels per AFNO block (embed 256 / 2), 16 x 16 latent grid, batch 2
MODEL_KW = dict(R.TINY, embed_dim=256, n_blocks=2, depth=3)
MODEL_B = 2
SCOPES = [None] + [(m, a) for m in (1, 2, 4) for a in (1, 2, 4)]


def _fresh():
    from dpot_amd import DPOTNet
    from dpot_amd.train import FlatParams, FusedAdam
    cfg = R.DPOTConfig(**MODEL_KW)
    S = cfg.img_size
    xx = R.recipe_input((MODEL_B, S, S, cfg.in_timesteps, cfg.in_channels), salt=81).cuda()
    yy = R.recipe_input((MODEL_B, S, S, 1, cfg.out_channels), salt=82).cuda()
    msk = torch.ones(MODEL_B, S, S, 1, cfg.out_channels).cuda()
    m = DPOTNet(**MODEL_KW)
    m.load_state_dict(R.recipe_state_dict(cfg, salt=6))
    m.cuda()
    opt = FusedAdam(FlatParams(m), lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
    return m, opt, xx, yy, msk


def _grads(ops, lane, scope):
    from dpot_amd.train import _forward_backward as fb, rollout_total
    m, opt, xx, yy, msk = _fresh()
    with ops.wgrad_lane_scope(lane), ops.wgrad_chain_scope(scope):
        loss, _ = fb(opt, lambda: rollout_total(m, xx, yy, msk))
    torch.cuda.synchronize()
    assert ops.wgrad_lane_pending() == 0
    return loss.clone(), opt.fp.grad.clone()


def test_model_every_chain_setting_against_the_per_block_schedule(ops, monkeypatch):
    """loss and the whole flat gradient buffer: every chain setting, on the lane and on the step's stream, against the
    per-block schedule (DPOT_TUNE fused_small=2)"""
    from dpot_amd import functional as F
    set_tune(monkeypatch, fused_small=2)
    want_loss, want = _grads(ops, False, None)
    assert torch.isfinite(want).all() and want.abs().max() > 0
    set_tune(monkeypatch, fused_small=4)
    used = []
    real = F.WgradBatch.chains
    monkeypatch.setattr(F.WgradBatch, "chains", staticmethod(lambda *a: (used.append(real(*a)), used[-1])[1]))
    for scope in SCOPES:
        for lane in (True, False):
            loss, grad = _grads(ops, lane, scope)
            assert torch.equal(loss, want_loss), (scope, lane)
            assert torch.equal(grad, want), f"chains {scope}, lane {lane}: {(grad != want).sum().item()} gradient elements differ"
            assert used and (scope is None or used[-1] == scope), (scope, used[-1:])
    assert all(c in (1, 2, 4) for pair in used for c in pair)


@pytest.mark.parametrize("scope", [None, (4, 2)])
def test_captured_step_matches_the_eager_one(ops, scope):
    """one optimisation step: the replay of the step captured at the default (no chain) and at chains (4, 2) leaves the
    loss and the parameters of the eager, unchained step"""
    from dpot_amd.train import GraphedTrainStep, train_step
    m, opt, xx, yy, msk = _fresh()
    start = opt.fp.flat.clone()
    eager_loss, _ = train_step(m, opt, xx, yy, msk, lr=1e-3)
    torch.cuda.synchronize()
    eager, eager_loss = opt.fp.flat.clone(), eager_loss.clone()
    m, opt, xx, yy, msk = _fresh()
    with ops.wgrad_chain_scope(scope):
        step = GraphedTrainStep(m, opt, xx, yy, msk, warmup=1)    # the warm-up step is undone (train.trial_state)
    assert torch.equal(opt.fp.flat, start)
    loss = step.replay(1e-3)
    torch.cuda.synchronize()
    assert torch.isfinite(eager).all() and not torch.equal(eager, start)
    assert torch.equal(loss, eager_loss)
    assert torch.equal(opt.fp.flat, eager), f"{(opt.fp.flat != eager).sum().item()} parameters differ"
