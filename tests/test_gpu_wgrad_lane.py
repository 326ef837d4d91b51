"""The weight-gradient lane (lane 0 of csrc/lane.hip; ops.wgrad_flush_async / ops.wgrad_lane_join; functional.WgradBatch._flush_group): the
batched weight gradients on the library's own stream beside the embed backward.  No kernel, split factor or summation order
changes, so every comparison here is bit for bit against the synchronous schedule: an eager step, a captured step (an unjoined
lane would end the capture with an error), the pending count between the flush and the end of the backward, the cases that
must stay synchronous, and a first use inside a capture (no lane may be created there).

The model is the smallest that takes the batched route: 16 x 16 latent grid, embed 128 = one channel block of 128, mlp_ratio 1,
depth 2, batch 2 - 512 tokens and 2 * 16 * 9 = 288 spectrum rows, both multiples of the 32-token slab."""
import pytest
import torch

from oracle import dpot_ref as R

pytestmark = pytest.mark.gpu

KW = dict(R.TINY, embed_dim=128, n_blocks=1, depth=2)
B = 2


@pytest.fixture(scope="module")
def ops():
    from dpot_amd import _lib
    from dpot_amd import ops as _ops
    lib = _lib.load()
    assert torch.cuda.is_available()
    if lib.dpot_tune(b"wgrad_gauss", 1) == 0 or lib.dpot_tune(b"panel", 1) == 0 or _ops.tune("fused_small") in (0, 2):
        pytest.fail("this process's DPOT_TUNE turns the batched weight gradients off: the lane has nothing to carry")
    return _ops


def _inputs(T_ar):
    cfg = R.DPOTConfig(**KW)
    S = cfg.img_size
    xx = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=91)
    yy = R.recipe_input((B, S, S, T_ar, cfg.out_channels), salt=92)
    return cfg, xx.cuda(), yy.cuda(), torch.ones(B, S, S, 1, cfg.out_channels).cuda()


def _fresh(T_ar=1):
    from dpot_amd import DPOTNet
    from dpot_amd.train import FlatParams, FusedAdam
    cfg, xx, yy, msk = _inputs(T_ar)
    m = DPOTNet(**KW)
    m.load_state_dict(R.recipe_state_dict(cfg, salt=9))
    m.cuda()
    opt = FusedAdam(FlatParams(m), lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
    return m, opt, xx, yy, msk


def _forward_backward(ops, m, opt, xx, yy, msk, lane):
    from dpot_amd.train import _forward_backward as fb, rollout_total
    with ops.wgrad_lane_scope(lane):
        return fb(opt, lambda: rollout_total(m, xx, yy, msk))


class _Probe:
    """counts the asynchronous flushes and samples the lane's pending count where EmbedFn.backward starts - after the flush
    (block 0's backward delivers the last job), before the end of the backward"""

    def __init__(self, monkeypatch, ops):
        from dpot_amd import functional as F
        self.flushes, self.pending = 0, []
        real_flush, real_bwd = ops.wgrad_flush_async, F.EmbedFn.backward

        def flush(*a):
            self.flushes += 1
            return real_flush(*a)

        def bwd(ctx, *g):
            self.pending.append(ops.wgrad_lane_pending())
            return real_bwd(ctx, *g)

        monkeypatch.setattr(ops, "wgrad_flush_async", flush)
        monkeypatch.setattr(F.EmbedFn, "backward", staticmethod(bwd))


_SYNC = {}


def _sync_grads(ops, T_ar):
    """loss and flat gradient buffer of one backward on the synchronous schedule: once per T_ar, shared, left unchanged"""
    if T_ar not in _SYNC:
        m, opt, xx, yy, msk = _fresh(T_ar)
        loss, _ = _forward_backward(ops, m, opt, xx, yy, msk, False)
        torch.cuda.synchronize()
        _SYNC[T_ar] = (loss.clone(), opt.fp.grad.clone())
    return _SYNC[T_ar]


def test_model_takes_the_batched_route(ops):
    from dpot_amd.functional import WgradBatch
    cfg = R.DPOTConfig(**KW)
    tok = (cfg.img_size // cfg.patch_size) ** 2
    assert tok == 256 and B * tok % 32 == 0 and (B * 16 * 9) % 32 == 0
    s = WgradBatch.splits(KW["depth"], B * tok, 128, 128, ops.effective_mlp_precision(), B * 16 * 9, 1, 128)
    assert all(s), s


def test_eager_step_is_bit_identical(ops, monkeypatch):
    """one eager optimisation step with the lane and without it, same seed: loss, every gradient, every updated parameter"""
    from dpot_amd.train import train_step
    probe = _Probe(monkeypatch, ops)
    got = []
    for lane in (True, False):
        m, opt, xx, yy, msk = _fresh()
        with ops.wgrad_lane_scope(lane):
            loss, pred = train_step(m, opt, xx, yy, msk)
        torch.cuda.synchronize()
        assert ops.wgrad_lane_pending() == 0
        got.append((loss.clone(), pred.clone(), opt.fp.grad.clone(), opt.fp.flat.clone(), opt.sumsq.clone()))
    assert probe.flushes == 1 and probe.pending == [1, 0], (probe.flushes, probe.pending)
    assert ops.wgrad_lane_ready()
    assert torch.isfinite(got[0][2]).all() and got[0][2].abs().max() > 0
    for a, b, what in zip(got[0], got[1], ("loss", "pred", "gradients", "parameters", "||g||^2")):
        assert torch.equal(a, b), what
    assert torch.equal(got[0][2], _sync_grads(ops, 1)[1])


def test_captured_step_is_bit_identical(ops, monkeypatch):
    """GraphedTrainStep with the lane: the capture succeeds (the lane is forked from and joined back into the capturing stream)
    and three replays leave the parameters of three replays of the synchronous capture"""
    from dpot_amd.train import GraphedTrainStep
    probe = _Probe(monkeypatch, ops)
    flat = []
    for lane in (True, False):
        m, opt, xx, yy, msk = _fresh()
        with ops.wgrad_lane_scope(lane):
            step = GraphedTrainStep(m, opt, xx, yy, msk, warmup=1)
        assert ops.wgrad_lane_pending() == 0
        per_replay = []
        for _ in range(3):
            step.replay(1e-3)
            per_replay.append(opt.fp.flat.clone())
        torch.cuda.synchronize()
        flat.append(per_replay)
    assert probe.flushes == 2 and probe.pending == [1, 1, 0, 0], (probe.flushes, probe.pending)   # warm-up + capture, each
    for k, (a, b) in enumerate(zip(*flat)):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), f"parameters after replay {k}"
    assert not torch.equal(flat[0][0], flat[0][2])


def test_pending_count(ops, monkeypatch):
    """1 between the flush and the end of the backward, 0 when backward() has returned and before the optimiser launches"""
    probe = _Probe(monkeypatch, ops)
    m, opt, xx, yy, msk = _fresh()
    assert ops.wgrad_lane_pending() == 0
    _forward_backward(ops, m, opt, xx, yy, msk, True)
    assert probe.pending == [1] and probe.flushes == 1
    assert ops.wgrad_lane_pending() == 0
    ops.wgrad_lane_join()                          # safe to call again: nothing pending
    assert ops.wgrad_lane_pending() == 0
    opt.step(1e-3)
    torch.cuda.synchronize()
    assert ops.wgrad_lane_pending() == 0
    assert torch.equal(opt.fp.grad, _sync_grads(ops, 1)[1])


def test_gradient_callbacks_keep_the_synchronous_flush(ops, monkeypatch):
    """a callback in fp.callbacks (a data-parallel reducer, gradient-ready hooks) may read a gradient the moment it is
    reported final: it copies it on the current stream, and the copies are the synchronous schedule's"""
    probe = _Probe(monkeypatch, ops)
    m, opt, xx, yy, msk = _fresh()
    fp, seen, copies = opt.fp, [], {}

    def on_ready(i):
        seen.append(ops.wgrad_lane_pending())
        copies[i] = fp.grad_views[i].clone()

    fp.callbacks.append(on_ready)
    _forward_backward(ops, m, opt, xx, yy, msk, True)
    torch.cuda.synchronize()
    assert probe.flushes == 0 and probe.pending == [0] and seen and not any(seen)
    want = _sync_grads(ops, 1)[1]
    blocks = [i for i, n in enumerate(fp.names) if n.startswith("blocks.")]
    assert blocks and all(i in copies for i in blocks)
    for i, c in copies.items():
        o = fp.offsets[i]
        assert torch.equal(c.reshape(-1), want[o:o + c.numel()]), fp.names[i]
    assert torch.equal(fp.grad, want)


def test_rollout_keeps_the_synchronous_flush(ops, monkeypatch):
    """T_ar = 2: the second pass through the blocks adds to the slots on the step's stream, so neither pass may leave its
    gradients to the lane"""
    probe = _Probe(monkeypatch, ops)
    m, opt, xx, yy, msk = _fresh(2)
    loss, _ = _forward_backward(ops, m, opt, xx, yy, msk, True)
    torch.cuda.synchronize()
    assert probe.flushes == 0 and probe.pending == [0, 0]
    want_loss, want = _sync_grads(ops, 2)
    assert torch.equal(loss, want_loss) and torch.equal(opt.fp.grad, want)


def test_first_use_inside_a_capture_runs_on_the_callers_stream(ops, monkeypatch):
    """no lane exists when the first asynchronous flush is captured: none is created (stream creation is no capturable call),
    the launches go to the capturing stream, the capture ends well and its replay gives the synchronous gradients"""
    probe = _Probe(monkeypatch, ops)
    m, opt, xx, yy, msk = _fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _forward_backward(ops, m, opt, xx, yy, msk, False)          # allocator and lazy initialisations, off the lane
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ops.wgrad_lane_shutdown()
    assert not ops.wgrad_lane_ready()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        loss, _ = _forward_backward(ops, m, opt, xx, yy, msk, True)
    assert probe.flushes == 1 and probe.pending == [0, 0]
    assert not ops.wgrad_lane_ready() and ops.wgrad_lane_pending() == 0
    opt.fp.grad.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    want_loss, want = _sync_grads(ops, 1)
    assert torch.equal(loss, want_loss) and torch.equal(opt.fp.grad, want)
