"""The side lane (csrc/lane.hip dpot_lane_fork / dpot_lane_join, lane 1; ops.side_lane): the step's latency-bound side chains
- the weight-only prologue (`weights`) and the first conv's gradients (`patch`) - on a library-owned stream beside independent work
of the step's stream.  (The classification head, `cls`, failed its ablation and has no call site: profiles/side_lane_ab.txt.)
No kernel, split factor, launch argument or summation order changes, so every comparison here is torch.equal against
`side_lane_scope(())`, the schedule with every site off.

The model is that of tests/test_gpu_wgrad_lane.py: 16 x 16 latent grid, embed 128, depth 2, batch 2."""
import pytest
import torch

from oracle import dpot_ref as R

pytestmark = pytest.mark.gpu

KW = dict(R.TINY, embed_dim=128, n_blocks=1, depth=2)
KW3 = dict(KW, in_channels=3, out_channels=3)          # no implicit-GEMM patch embedding: the explicit patch-matrix route
B = 2
ALL = ("weights", "patch")
WHAT = ("loss", "pred", "cls_pred", "gradients", "parameters", "||g||^2")


@pytest.fixture(scope="module")
def ops():
    from dpot_amd import ops as _ops
    assert torch.cuda.is_available()
    if _ops.tune("fused_small") == 0:
        pytest.fail("this process's DPOT_TUNE turns the merged layout launch off: the `weights` site has nothing to fork behind")
    return _ops


def _inputs(kw, T_ar):
    cfg = R.DPOTConfig(**kw)
    S = cfg.img_size
    xx = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=91)
    yy = R.recipe_input((B, S, S, T_ar, cfg.out_channels), salt=92)
    return cfg, xx.cuda(), yy.cuda(), torch.ones(B, S, S, 1, cfg.out_channels).cuda()


def _fresh(kw=KW, T_ar=1, update_tail=False):
    from dpot_amd import DPOTNet
    from dpot_amd.train import FlatParams, FusedAdam
    cfg, xx, yy, msk = _inputs(kw, T_ar)
    m = DPOTNet(**kw)
    m.load_state_dict(R.recipe_state_dict(cfg, salt=9))
    m.cuda()
    opt = FusedAdam(FlatParams(m), lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0, update_tail=update_tail)
    return m, opt, xx, yy, msk


def _step(ops, sites, kw=KW, T_ar=1, cls_weight=0.0):
    """a no_grad forward (for cls_pred) and one eager optimisation step under `sites` -> the tensors of WHAT"""
    from dpot_amd.train import train_step
    m, opt, xx, yy, msk = _fresh(kw, T_ar, update_tail=cls_weight != 0.0)
    labels = torch.tensor([1, 3], device="cuda") if cls_weight != 0.0 else None
    with ops.side_lane_scope(sites):
        with torch.no_grad():
            _, cls_pred = m(xx)
        loss, pred = train_step(m, opt, xx, yy, msk, cls=labels, cls_weight=cls_weight)
    torch.cuda.synchronize()
    assert ops.side_lane_pending() == 0 and ops.wgrad_lane_pending() == 0
    return loss.clone(), pred.clone(), cls_pred.clone(), opt.fp.grad.clone(), opt.fp.flat.clone(), opt.sumsq.clone()


_REF = {}


def _ref(ops, kw=KW, T_ar=1, cls_weight=0.0):
    """the step with every site off: once per configuration, shared, left unchanged"""
    key = (kw["in_channels"], T_ar, cls_weight)
    if key not in _REF:
        _REF[key] = _step(ops, (), kw, T_ar, cls_weight)
    return _REF[key]


def _same(got, want):
    assert torch.isfinite(got[3]).all() and got[3].abs().max() > 0
    for a, b, what in zip(got, want, WHAT):
        assert torch.equal(a, b), what


class _Probe:
    """counts the forks per site (`ops.side_lane` with the site on) and samples the side lane's pending count before and after
    every `ops.side_lane_join`, and the weight-gradient lane's where EmbedFn.backward starts"""

    def __init__(self, monkeypatch, ops):
        from dpot_amd import functional as F
        self.forks, self.joins, self.wgrad = [], [], []
        real_lane, real_join, real_bwd = ops.side_lane, ops.side_lane_join, F.EmbedFn.backward

        def lane(site, on=None, join=True):
            if ops.side_lane_enabled(site) if on is None else on:
                self.forks.append(site)
            return real_lane(site, on, join)

        def join():
            before = ops.side_lane_pending()
            real_join()
            self.joins.append((before, ops.side_lane_pending()))

        def bwd(ctx, *g):
            self.wgrad.append(ops.wgrad_lane_pending())
            return real_bwd(ctx, *g)

        monkeypatch.setattr(ops, "side_lane", lane)
        monkeypatch.setattr(ops, "side_lane_join", join)
        monkeypatch.setattr(F.EmbedFn, "backward", staticmethod(bwd))

    def effective(self):
        return [j for j in self.joins if j[0] != 0]


@pytest.mark.parametrize("sites", [("weights",), ("patch",), ALL], ids="+".join)
def test_eager_step_is_bit_identical(ops, sites):
    _same(_step(ops, sites), _ref(ops))
    assert ops.side_lane_ready()


def test_captured_step_is_bit_identical(ops):
    """GraphedTrainStep with every site: the capture succeeds - an unjoined lane would end it with an error - and two replays
    leave the parameters of two replays of the capture without the side lane"""
    from dpot_amd.train import GraphedTrainStep
    flat = []
    for sites in (ALL, ()):
        m, opt, xx, yy, msk = _fresh()
        with ops.side_lane_scope(sites):
            step = GraphedTrainStep(m, opt, xx, yy, msk, warmup=1)
        assert ops.side_lane_pending() == 0 and ops.wgrad_lane_pending() == 0
        per_replay = []
        for _ in range(2):
            step.replay(1e-3)
            per_replay.append(opt.fp.flat.clone())
        torch.cuda.synchronize()
        flat.append(per_replay)
    for k, (a, b) in enumerate(zip(*flat)):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), f"parameters after replay {k}"
    assert not torch.equal(flat[0][0], flat[0][1])


def test_first_use_inside_a_capture_runs_on_the_callers_stream(ops, monkeypatch):
    """no side lane exists when its first fork is captured: none is created, the side chains go to the capturing stream, the
    capture ends well and its replay gives the gradients of the schedule without the lane"""
    from dpot_amd.train import _forward_backward as fb, rollout_total
    probe = _Probe(monkeypatch, ops)
    m, opt, xx, yy, msk = _fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), ops.side_lane_scope(()):
        fb(opt, lambda: rollout_total(m, xx, yy, msk))              # allocator and lazy initialisations, off the lane
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ops.side_lane_shutdown()
    assert not ops.side_lane_ready()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"), ops.side_lane_scope(ALL):
        loss, _ = fb(opt, lambda: rollout_total(m, xx, yy, msk))
    assert probe.forks[-2:] == ["weights", "patch"] and not probe.effective()
    assert not ops.side_lane_ready() and ops.side_lane_pending() == 0
    opt.fp.grad.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    want = _ref(ops)
    assert torch.equal(loss, want[0]) and torch.equal(opt.fp.grad, want[3])


def test_pending_counts(ops, monkeypatch):
    """one fork per site and step; the side lane's count is 1 inside each window (at the join that closes it) and 0 after it;
    the weight-gradient lane still counts its one flush where EmbedFn.backward starts"""
    from dpot_amd.train import _forward_backward as fb, rollout_total
    probe = _Probe(monkeypatch, ops)
    m, opt, xx, yy, msk = _fresh()
    assert ops.side_lane_pending() == 0
    with ops.side_lane_scope(ALL), ops.wgrad_lane_scope(True):
        fb(opt, lambda: rollout_total(m, xx, yy, msk))
    assert probe.forks == ["weights", "patch"]
    assert probe.effective() == [(1, 0)] * 2 and all(j[1] == 0 for j in probe.joins)
    assert probe.wgrad == [1]
    assert ops.side_lane_pending() == 0 and ops.wgrad_lane_pending() == 0
    ops.side_lane_join()                           # safe to call again: nothing pending
    assert ops.side_lane_pending() == 0
    torch.cuda.synchronize()
    assert torch.equal(opt.fp.grad, _ref(ops)[3])


def test_rollout_forks_and_joins_once(ops, monkeypatch):
    """T_ar = 2 under weights_scope: the prologue is forked once, where the scope opens; the first pass's EmbedFn.forward is the
    one effective join and the second pass finds nothing pending"""
    from dpot_amd.train import _forward_backward as fb, rollout_total
    probe = _Probe(monkeypatch, ops)
    m, opt, xx, yy, msk = _fresh(T_ar=2)
    with ops.side_lane_scope(("weights",)):
        loss, _ = fb(opt, lambda: rollout_total(m, xx, yy, msk))
    torch.cuda.synchronize()
    assert probe.forks == ["weights"] and probe.effective() == [(1, 0)], (probe.forks, probe.joins)
    assert len(probe.joins) > 2
    want = _ref(ops, T_ar=2)
    assert torch.equal(loss, want[0]) and torch.equal(opt.fp.grad, want[3])


def test_rollout_with_every_site(ops):
    _same(_step(ops, ALL, T_ar=2), _ref(ops, T_ar=2))


def test_derive_called_directly_leaves_nothing_pending(ops):
    m, _, _, _, _ = _fresh()
    with ops.side_lane_scope(("weights",)):
        got = m.packs.derive(m)
        assert ops.side_lane_pending() == 0
    with ops.side_lane_scope(()):
        emb = [t.clone() for t in got[0] if t is not None]         # (the persistent buffers are rewritten below)
        want = m.packs.derive(m)
    torch.cuda.synchronize()
    assert len(emb) == len([t for t in want[0] if t is not None]) >= 8
    for a, b in zip(emb, [t for t in want[0] if t is not None]):
        assert torch.equal(a, b)


def test_no_grad_forward(ops):
    m, _, xx, _, _ = _fresh()
    out = []
    for sites in (ALL, ()):
        with ops.side_lane_scope(sites), torch.no_grad():
            out.append(m(xx))
        assert ops.side_lane_pending() == 0
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.isfinite(out[0][1]).all() and out[0][1].abs().max() > 0


def test_cls_backward(ops):
    """cls_weight != 0: the classification head's backward runs, and its gradients reach the embed backward's `patch` window
    (the default, where cls_pred is unused, is every other test here)"""
    _same(_step(ops, ALL, cls_weight=0.5), _ref(ops, cls_weight=0.5))
    assert not torch.equal(_ref(ops, cls_weight=0.5)[3], _ref(ops)[3])


def test_three_input_channels_take_the_patch_matrix_route(ops):
    from dpot_amd import functional as F
    cfg = R.DPOTConfig(**KW3)
    hid = cfg.out_channels * cfg.patch_size + 3
    assert not ops.embed_supported(cfg.in_channels, cfg.patch_size, cfg.in_timesteps, hid, cfg.img_size // cfg.patch_size)
    assert F._pad4(hid) != hid                     # colsum + linear_bwd_weight + copy2d_pad on the lane
    _same(_step(ops, ALL, KW3), _ref(ops, KW3))
    _same(_step(ops, ("patch",), KW3), _ref(ops, KW3))


def test_gradient_ready_callback_sees_finished_first_conv_gradients(ops):
    """a callback in fp.callbacks copies a gradient on the step's stream the moment it is reported final: the first conv's
    gradients come from the lane, and the copies are those of the schedule without it"""
    from dpot_amd.train import _forward_backward as fb, rollout_total
    m, opt, xx, yy, msk = _fresh()
    fp, copies, pending = opt.fp, {}, {}

    def on_ready(i):
        pending[i] = ops.side_lane_pending()
        copies[i] = fp.grad_views[i].clone()

    fp.callbacks.append(on_ready)
    with ops.side_lane_scope(ALL):
        fb(opt, lambda: rollout_total(m, xx, yy, msk))
    torch.cuda.synchronize()
    want = _ref(ops)[3]
    conv = [i for i, n in enumerate(fp.names) if n.startswith("patch_embed.proj.0.")]
    assert len(conv) == 2 and all(i in copies for i in conv)
    # (the weight-only chain's gradients are produced on the step's stream and may be reported inside the window)
    assert all(pending[i] == 0 for i in conv), pending          # told after the join
    for i, c in copies.items():
        o = fp.offsets[i]
        assert torch.equal(c.reshape(-1), want[o:o + c.numel()]), fp.names[i]
    assert torch.equal(fp.grad, want)


@pytest.mark.parametrize("site,op", [("weights", "colsum"), ("patch", "group_rowsum")])
def test_an_op_that_raises_leaves_nothing_pending(ops, monkeypatch, site, op):
    """an exception between fork and join: the join sits in a finally, and the next step is the reference's"""
    from dpot_amd.train import _forward_backward as fb, rollout_total
    m, opt, xx, yy, msk = _fresh()
    real, seen = getattr(ops, op), []

    def boom(*a, **k):
        seen.append(ops.side_lane_pending())
        raise RuntimeError("boom")

    with ops.side_lane_scope((site,)):
        monkeypatch.setattr(ops, op, boom)
        with pytest.raises(RuntimeError, match="boom"):
            fb(opt, lambda: rollout_total(m, xx, yy, msk))
        monkeypatch.setattr(ops, op, real)
        assert seen == [1], seen                   # raised inside the window
        assert ops.side_lane_pending() == 0
        ops.wgrad_lane_join()
        torch.cuda.synchronize()
    _same(_step(ops, (site,)), _ref(ops))
