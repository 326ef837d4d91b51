"""GPU tests of the training metrics (csrc/metrics.hip, ops.cls_ce_* / rel_l2_combine / metrics_accum, functional.ClsCEFn,
train.StepMetrics and the cls / cls_weight / metrics arguments of the steps).  Oracles: torch.nn.functional.cross_entropy in
float64 on the CPU, the existing rel_l2 kernel on the concatenated rollout, oracle/dpot_ref.py.  The op-level tests run on the
guarded NaN-poisoned allocator (tests/guard.py)."""
import os
import socket
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import RTOL, assert_close
from oracle import dpot_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- cross-entropy, op level ------------------------------------------------------------------------------------------
def _logits(B, n_cls, seed):
    """random logits scaled to +-80 (exp(80) overflows fp32: only the max-subtracted form survives) whose row maximum is
    unique by a margin > 1e-3, so that an exact accuracy count is a fair demand"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, n_cls, generator=g)
    x = x / x.abs().max() * 80.0
    if n_cls > 1:
        top = x.double().topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) > 1e-3
    labels = torch.randint(0, n_cls, (B,), generator=g)
    labels[: B // 2] = x[: B // 2].argmax(1)                    # about half the rows are classified correctly
    return x, labels


@pytest.mark.parametrize("B,n_cls", [(32, 12), (1, 1), (7, 3), (4096, 12), (16, 1000), (5, 64), (9, 65)])
def test_cls_ce_fwd_bwd_vs_float64_torch(B, n_cls, guarded):
    from dpot_amd import cls_ce_loss, ops
    x, labels = _logits(B, n_cls, seed=B * 1009 + n_cls)
    xr = x.double().requires_grad_(True)
    ref = F.cross_entropy(xr, labels, reduction="sum")
    (0.7 * ref).backward()
    want_correct = int((x.argmax(1) == labels).sum())
    xd = guard.wrap(x.cuda()).requires_grad_(True)
    ld = guard.wrap(labels.cuda())
    loss, correct = cls_ce_loss(xd, ld)
    (0.7 * loss).backward()
    torch.cuda.synchronize()
    print(f"cls_ce ({B},{n_cls}): loss {loss.item():.6f} ref {ref.item():.6f} correct {int(correct)} / {want_correct}")
    assert loss.dtype == torch.float32 and loss.dim() == 0 and correct.dtype == torch.int64
    assert_close(loss, ref.detach(), f"cls_ce loss ({B},{n_cls})")
    assert_close(xd.grad, xr.grad, f"cls_ce dlogits ({B},{n_cls})")
    assert int(correct) == want_correct
    # the raw op: out words {loss, correct, valid, invalid}, row statistics, and run-to-run determinism (bit-identical)
    o1, s1 = ops.cls_ce_fwd(xd.detach(), ld)
    o2, s2 = ops.cls_ce_fwd(xd.detach(), ld)
    assert o1.tolist()[1:] == [want_correct, B, 0] and torch.equal(o1, o2) and torch.equal(s1, s2)
    assert_close(s1[:, 0], x.max(1).values, "row max")
    assert_close(s1[:, 1], torch.logsumexp(x.double(), 1), "row lse")
    g = guard.wrap(torch.tensor([0.7], device="cuda"))
    d1, d2 = ops.cls_ce_bwd(xd.detach(), ld, s1, g), ops.cls_ce_bwd(xd.detach(), ld, s1, g)
    assert torch.equal(d1, d2) and torch.equal(d1, xd.grad)
    guard.check()


def test_cls_ce_ties_take_the_first_maximal_index(guarded):
    """torch.argmax returns the FIRST maximal index; exact ties inside one lane group, across lanes and across trips"""
    from dpot_amd import cls_ce_loss
    small = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, 5.0, 1.0, 5.0], [7.0, 7.0, -1.0, 7.0]])
    lab_s = torch.tensor([1, 0, 3, 1])                           # first maxima: 1, 0, 1, 0 -> rows 0 and 1 are correct
    wide = torch.zeros(4, 130)
    wide[0, [3, 70]] = 4.0                                       # lanes 3 and 6 (second trip): first is 3
    wide[1, [69, 5]] = 2.5                                       # the same lane on two trips: first is 5
    wide[2, [129, 64, 0]] = 1.0                                  # first is 0
    wide[3, 128] = 9.0
    lab_w = torch.tensor([3, 69, 0, 128])                        # correct: rows 0, 2, 3
    for x, labels, want in ((small, lab_s, 2), (wide, lab_w, 3)):
        assert int((x.argmax(1) == labels).sum()) == want        # the CPU's own rule
        loss, correct = cls_ce_loss(guard.wrap(x.cuda()), guard.wrap(labels.cuda()))
        assert int(correct) == want
        assert_close(loss, F.cross_entropy(x.double(), labels, reduction="sum"), "ties loss")


def test_cls_ce_labels_outside_the_classes_index_nothing(guarded):
    """labels -1 and n_cls: their rows add nothing to loss / correct / valid, are counted in `invalid`, get a zero gradient -
    and every guard around logits, labels, row statistics, out and dlogits is intact"""
    from dpot_amd import ops
    B, n_cls = 9, 12
    x, labels = _logits(B, n_cls, seed=77)
    labels[0], labels[4], labels[8] = -1, n_cls, 1 << 40
    ok = (labels >= 0) & (labels < n_cls)
    xr = x.double().requires_grad_(True)
    ref = F.cross_entropy(xr[ok], labels[ok], reduction="sum")
    ref.backward()
    xd, ld = guard.wrap(x.cuda()), guard.wrap(labels.cuda())
    out, stats = ops.cls_ce_fwd(xd, ld)
    dl = ops.cls_ce_bwd(xd, ld, stats, guard.wrap(torch.ones(1, device="cuda")))
    torch.cuda.synchronize()
    assert out.tolist()[1:] == [int((x.argmax(1) == labels)[ok].sum()), int(ok.sum()), 3]
    assert_close(ops.cls_out_loss(out), ref.detach(), "loss over the valid rows")
    assert_close(dl, xr.grad, "dlogits")
    assert float(dl[~ok.cuda()].abs().max()) == 0.0
    guard.check()


# ---- full-rollout relative L2 from the step statistics ----------------------------------------------------------------
def _mask(kind, B, X, C, seed):
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(B, X, X, 1, C, generator=g) > 0.3).float()
    if kind == "channel":                                        # whole channels of some samples masked out: nch_b differs
        m[0, ..., 1] = 0.0
        m[2, ..., 0] = 0.0
        m[2, ..., 2] = 0.0
    return m


@pytest.mark.parametrize("n_steps", [1, 3, 20])
@pytest.mark.parametrize("kind", ["none", "random", "channel"])
def test_rel_l2_combine_vs_two_pass_and_oracle(n_steps, kind, guarded):
    from dpot_amd import ops
    from dpot_amd.functional import rel_l2_loss
    B, X, C = 5, 16, 3
    g = torch.Generator().manual_seed(100 + n_steps)
    yy = torch.randn(B, X, X, n_steps, C, generator=g)
    preds = [yy[..., t:t + 1, :] + 0.3 * (t + 1) * torch.randn(B, X, X, 1, C, generator=g) for t in range(n_steps)]
    msk = _mask(kind, B, X, C, seed=9)
    md = msk.cuda() if msk is not None else None
    n = ops.rel_l2_stats_elems(B, X * X, C)
    slots = guard.full_nan((n_steps, n))
    separate = []
    steps = []
    for t in range(n_steps):
        y = yy[..., t:t + 1, :].contiguous().cuda()
        steps.append(rel_l2_loss(preds[t].contiguous().cuda(), y, md, slots[t]))
        l2, st = ops.rel_l2_fwd(preds[t].contiguous().cuda(), y, md, B, X * X, C, 1)
        assert torch.equal(l2.view(()), steps[-1])               # the slot changes nothing
        separate.append(st.view(-1))
    full = ops.rel_l2_combine(slots, B, C)
    again = ops.rel_l2_combine(slots, B, C, out=guard.full_nan(1))
    table = ops.rel_l2_combine(ops.StatsTable(separate), B, C)
    two_pass = rel_l2_loss(torch.cat(preds, dim=-2).contiguous().cuda(), yy.cuda(), md)
    oracle = R.rel_l2_loss(torch.cat(preds, dim=-2).double(), yy.double(), msk.double() if msk is not None else None)
    torch.cuda.synchronize()
    print(f"rel_l2_combine n={n_steps} {kind}: {full.item():.7f} two-pass {two_pass.item():.7f} oracle {oracle.item():.7f}")
    assert torch.equal(full, again) and torch.equal(full, table)             # deterministic; table == strided
    assert_close(full.view(()), two_pass, "combine vs two-pass")
    assert_close(full.view(()), oracle, "combine vs oracle")
    if n_steps == 1:
        assert_close(full.view(()), steps[0], "one step: the full loss is the step loss")
    guard.check()


def test_metrics_accum_op(guarded):
    """two accumulate launches: sums, the last-step copy, the grad norm from sumsq, a NaN step counted"""
    from dpot_amd import ops
    acc = guard.wrap(torch.zeros(2, ops.METRICS_WORDS, dtype=torch.int64, device="cuda"))
    cls = torch.zeros(2, ops.CLS_OUT_WORDS, dtype=torch.int64)
    cls[:, 0] = torch.tensor([1.5, 2.25], dtype=torch.float32).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    cls[:, 1:] = torch.tensor([[3, 4, 0], [2, 3, 1]])
    cls = guard.wrap(cls.cuda())
    l2s, l2f = guard.wrap(torch.tensor([6.0], device="cuda")), guard.wrap(torch.tensor([2.5], device="cuda"))
    ss = guard.wrap(torch.tensor([16.0], device="cuda"))
    ops.metrics_accum(acc, l2s, l2f, cls, 2, ss, 0.5, 4, 2, 1)
    bad = guard.wrap(torch.tensor([float("nan")], device="cuda"))
    ops.metrics_accum(acc, bad, l2f, None, 0, None, 1.0, 4, 2, 1)
    a = acc.cpu()
    run, last = a[0], a[1]
    f = run[:4].view(torch.float64).tolist()
    assert np.isnan(f[0]) and f[1:] == [5.0, 3.75, 2.0]
    assert run[4:11].tolist() == [5, 7, 1, 8, 4, 2, 1]
    lf = last[:4].view(torch.float64).tolist()
    assert np.isnan(lf[0]) and lf[1:] == [2.5, 0.0, 0.0] and last[4:11].tolist() == [0, 0, 0, 4, 2, 1, 1]
    guard.check()


# ---- step level -------------------------------------------------------------------------------------------------------
def _state(cfg, salt):
    """the recipe weights with the last cls_head layer scaled by 30: the recipe's logits differ by ~1e-2 between classes,
    too close to demand an exact accuracy count from two implementations; x30 gives every row a clear maximum (each test
    that counts still asserts the margin)"""
    sd = R.recipe_state_dict(cfg, salt=salt)
    sd["cls_head.4.weight"] = sd["cls_head.4.weight"] * 30.0
    sd["cls_head.4.bias"] = sd["cls_head.4.bias"] * 30.0
    return sd


def build(kw, salt):
    from dpot_amd import DPOTNet
    cfg = R.DPOTConfig(**kw)
    m = DPOTNet(**kw)
    m.load_state_dict(_state(cfg, salt))
    return m.cuda(), cfg


def _batch(cfg, B, T_ar=1, salt=1):
    S = cfg.img_size
    xx = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=salt).cuda()
    yy = R.recipe_input((B, S, S, T_ar, cfg.out_channels), salt=salt + 1).cuda()
    msk = torch.ones(B, S, S, 1, cfg.out_channels, device="cuda")
    cls = (torch.arange(B, device="cuda") % cfg.n_cls).view(B, 1)
    return xx, yy, msk, cls


def _opt(m, **kw):
    from dpot_amd.train import FlatParams, FusedAdam
    args = dict(lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
    args.update(kw)
    return FusedAdam(FlatParams(m), **args)


def _oracle_logits(sd, xx, pred, k, cfg):
    """cls logits of AR step k in float64 on the CPU: the window is the input slid by the first k predictions"""
    win = torch.cat((xx[..., k:, :], pred[..., :k, :]), dim=-2).double().cpu()
    return R.dpot_forward(OrderedDict((n, v.double()) for n, v in sd.items()), win, cfg)[1]


@pytest.mark.parametrize("T_ar", [1, 3])
@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_metrics_observe_without_changing_the_step_and_sum_up(T_ar, mode):
    """(a) observer property: a step with metrics + cls attached and cls_weight = 0 produces loss, prediction and flat
    parameter buffer BIT-identical to one without, over 3 steps from the same start; (b) read() then equals the sums of the
    per-step values computed from the returned predictions: l2_step / l2_full with the existing kernel on the predictions,
    the cross-entropy in float64 on the CPU from the oracle's logits, accuracy and counters exactly; (c) cls_head did not
    move (update_tail=False) and the warm-up of the graph is not logged"""
    from dpot_amd import StepMetrics
    from dpot_amd.functional import rel_l2_loss
    from dpot_amd.train import GraphedTrainStep, train_step
    N, B = 3, 4
    runs = []
    for attach in (False, True):
        m, cfg = build(R.MINI, salt=31)
        xx, yy, msk, cls = _batch(cfg, B, T_ar)
        opt = _opt(m)
        met = StepMetrics("cuda", T_ar) if attach else None
        kw = dict(cls=cls, cls_weight=0.0, metrics=met) if attach else {}
        step = GraphedTrainStep(m, opt, xx, yy, msk, warmup=2, **kw) if mode == "graph" else None
        if attach:
            z = met.read()
            assert z["opt_steps"] == 0 and z["samples"] == 0 and z["l2_step"] == 0.0       # warm-up is not logged
        rec = []
        for _ in range(N):
            sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
            if step is not None:
                loss, pred = step.replay(1e-3), step.pred
            else:
                loss, pred = train_step(m, opt, xx, yy, msk, lr=1e-3, **kw)
            rec.append((loss.clone(), pred.clone(), opt.fp.flat.clone(), sd, float(opt.grad_norm().item())))
        runs.append((rec, met, m, cfg, xx, yy, msk, cls))
    (plain, _, _, _, _, _, _, _), (seen, met, m, cfg, xx, yy, msk, cls) = runs
    for k in range(N):
        for a, b, what in zip(plain[k][:3], seen[k][:3], ("loss", "pred", "flat")):
            assert torch.equal(a, b), f"step {k}: {what} changed by attaching the metrics"
    head0 = _state(cfg, 31)
    for n, p in m.named_parameters():
        if n.startswith("cls_head."):
            assert torch.equal(p.detach().cpu(), head0[n]), n
    # (b) sums
    want = dict(l2_step=0.0, l2_full=0.0, cls_loss=0.0, grad_norm=0.0, correct=0)
    labels = cls.view(-1).cpu()
    for loss, pred, _, sd, gn in seen:
        want["l2_step"] += sum(float(rel_l2_loss(pred[..., t:t + 1, :].contiguous(), yy[..., t:t + 1, :].contiguous(), msk))
                               for t in range(T_ar))
        want["l2_full"] += float(rel_l2_loss(pred.contiguous(), yy, msk))
        want["grad_norm"] += gn
        for k in range(T_ar):
            lg = _oracle_logits(sd, xx, pred, k, cfg)
            top = lg.topk(2, dim=1).values
            assert float((top[:, 0] - top[:, 1]).min()) > 1e-3           # a unique maximum: exact accuracy is a fair demand
            want["cls_loss"] += float(F.cross_entropy(lg, labels, reduction="sum"))
            want["correct"] += int((lg.argmax(1) == labels).sum())
    d = met.read()
    print(f"metrics T_ar={T_ar} {mode}: got { {k: d[k] for k in ('l2_step', 'l2_full', 'cls_loss', 'grad_norm', 'cls_correct')} } "
          f"want {want}")
    for key in ("l2_step", "l2_full", "cls_loss", "grad_norm"):
        assert_close(torch.tensor(d[key]), torch.tensor(want[key]), key)
    assert d["cls_correct"] == want["correct"]
    assert (d["cls_total"], d["cls_invalid"], d["samples"], d["ar_steps"], d["opt_steps"], d["nonfinite_steps"]) == \
        (N * T_ar * B, 0, N * B, N * T_ar, N, 0)
    assert_close(torch.tensor(d["train_l2_step_avg"]), torch.tensor(want["l2_step"] / (N * B) / T_ar), "train_l2_step_avg")
    last = met.last()
    assert_close(last["l2_step"], seen[-1][0].double(), "last l2_step")
    assert int(last["samples"]) == B and int(last["opt_steps"]) == 1
    met.reset()
    assert met.read()["opt_steps"] == 0


@pytest.mark.parametrize("T_ar", [1, 3])
def test_weighted_cls_loss_gradient_reaches_the_whole_model(T_ar):
    """cls_weight = 1, update_tail=True: the loss and EVERY parameter gradient of one step against torch autograd on the CPU
    over the oracle's forward + rel_l2_loss + cross_entropy(reduction='sum'), at the tolerance of the g6 rollout golden test
    (loss 1e-4 relative; per-tensor gradient norm 1e-4 relative + 1e-7) and element-wise at the parity tolerance; the
    cls_head gradients are non-zero and its parameters move"""
    from dpot_amd import StepMetrics
    from dpot_amd.train import train_step
    B = 2
    m, cfg = build(R.MINI, salt=12)
    xx, yy, msk, cls = _batch(cfg, B, T_ar)
    sd = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in _state(cfg, 12).items())
    labels = cls.view(-1).cpu()
    l2_ref, ce_ref, win = 0.0, 0.0, xx.cpu()
    for t in range(T_ar):
        im, lg = R.dpot_forward(sd, win, cfg)
        l2_ref = l2_ref + R.rel_l2_loss(im, yy.cpu()[..., t:t + 1, :], msk.cpu())
        ce_ref = ce_ref + F.cross_entropy(lg, labels, reduction="sum")
        win = torch.cat((win[..., 1:, :], im), dim=-2)
    (l2_ref + 1.0 * ce_ref).backward()
    opt = _opt(m, update_tail=True)
    met = StepMetrics("cuda", T_ar)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    loss, _ = train_step(m, opt, xx, yy, msk, cls=cls, cls_weight=1.0, metrics=met)
    torch.cuda.synchronize()
    d = met.read()
    print(f"weighted cls T_ar={T_ar}: l2 {loss.item():.6f} ref {l2_ref.item():.6f}; ce {d['cls_loss']:.6f} ref {ce_ref.item():.6f}")
    assert abs(loss.item() - l2_ref.item()) <= 1e-4 * abs(l2_ref.item())          # the returned loss stays the L2 loss
    assert abs(d["cls_loss"] - ce_ref.item()) <= 1e-4 * abs(ce_ref.item())
    assert abs((d["l2_step"] + d["cls_loss"]) - (l2_ref + ce_ref).item()) <= 1e-4 * abs((l2_ref + ce_ref).item())
    for n, p in m.named_parameters():
        ref = sd[n].grad
        assert ref is not None, n
        gn = ref.norm().item()
        assert abs(p.grad.norm().item() - gn) <= 1e-4 * gn + 1e-7, n
        assert_close(p.grad, ref, "weighted cls d" + n)
        if n.startswith("cls_head."):
            assert float(p.grad.abs().max()) > 0.0, n
            assert not torch.equal(p.detach(), before[n]), f"{n} did not move"


def test_graph_replay_uses_the_staged_labels():
    """the labels live in a static buffer next to xx / yy / msk: a replay after stage(cls=new) scores the new labels"""
    from dpot_amd import StepMetrics
    from dpot_amd.train import GraphedTrainStep
    B = 4
    m, cfg = build(R.MINI, salt=8)
    xx, yy, msk, cls = _batch(cfg, B)
    opt = _opt(m, lr=0.0)                                        # lr 0: the parameters, hence the logits, stay put
    met = StepMetrics("cuda", 1)
    with torch.no_grad():
        logits = m(xx)[1].double().cpu()
    new = ((cls + 2) % cfg.n_cls).contiguous()
    step = GraphedTrainStep(m, opt, xx, yy, msk, warmup=1, cls=cls, metrics=met)
    flat0 = opt.fp.flat.clone()
    got = []
    for lab in (cls, new):
        step.stage(xx, yy, msk, cls=lab)
        step.replay(0.0)
        last = met.last()
        got.append((float(last["cls_loss"]), int(last["cls_correct"])))
    assert torch.equal(opt.fp.flat, flat0)
    for (ce, correct), lab in zip(got, (cls, new)):
        lab = lab.view(-1).cpu()
        assert_close(torch.tensor(ce), F.cross_entropy(logits, lab, reduction="sum"), "cls_loss of the staged labels")
        assert correct == int((logits.argmax(1) == lab).sum())
    assert abs(got[0][0] - got[1][0]) > 1e-3                     # the two label sets do score differently
    with pytest.raises(ValueError, match="without labels"):
        GraphedTrainStep(m, opt, xx, yy, msk, warmup=1).stage(xx, yy, msk, cls=cls)


def test_rollout_eval_accumulates_the_test_metrics():
    """infer.rollout_eval(metrics=...): test_l2_step / test_l2_full accumulate over two rollouts; the returned full loss
    (from the step statistics) agrees with the two-pass value of the call without metrics"""
    from dpot_amd import StepMetrics
    from dpot_amd.infer import GraphedRollout, rollout_eval
    B, T_ar = 3, 4
    m, cfg = build(R.MINI, salt=4)
    xx, yy, msk, _ = _batch(cfg, B, T_ar)
    m.eval()
    pred0, steps0, full0 = rollout_eval(m, xx, yy, msk)
    met = StepMetrics("cuda", T_ar)
    pred1, steps1, full1 = rollout_eval(m, xx, yy, msk, metrics=met)
    pred2, steps2, full2 = GraphedRollout(m, xx)(xx, yy, msk, metrics=met)
    assert torch.equal(pred0, pred1) and torch.equal(steps0, steps1)
    assert_close(full1, full0, "full loss: statistics vs second pass")
    assert_close(full2, full0, "graphed rollout")
    d = met.read()
    assert_close(torch.tensor(d["l2_step"]), (steps1 + steps2).double(), "test_l2_step")
    assert_close(torch.tensor(d["l2_full"]), (full1 + full2).double(), "test_l2_full")
    assert (d["samples"], d["ar_steps"], d["opt_steps"], d["cls_total"]) == (2 * B, 2 * T_ar, 2, 0)
    assert_close(torch.tensor(d["test_l2_full_avg"]), (full1 + full2).double() / (2 * B), "test_l2_full_avg")


# ---- data parallel ----------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, out_dir, backend):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from dpot_amd import DPOTNet, StepMetrics
    from dpot_amd.dp import BucketedGradReducer
    from dpot_amd.train import FlatParams, FusedAdam, make_dp_step
    cfg = R.DPOTConfig(**R.MINI)
    model = DPOTNet(**R.MINI)
    model.load_state_dict(R.recipe_state_dict(cfg, salt=17))
    model.cuda()
    fp = FlatParams(model)
    red = BucketedGradReducer(fp, n_buckets=3, overlap=True)
    red.single_rank_collective = backend == "nccl"
    red.broadcast_parameters(0)
    B = 4
    xx = R.recipe_input((B, cfg.img_size, cfg.img_size, cfg.in_timesteps, cfg.in_channels), salt=81)
    yy = R.recipe_input((B, cfg.img_size, cfg.img_size, 1, cfg.out_channels), salt=82)
    sl = slice(2 * rank, 2 * rank + 2) if world > 1 else slice(0, B)
    xs, ys = xx[sl].cuda(), yy[sl].cuda()
    ms = torch.ones_like(ys)
    cls = (torch.arange(B)[sl] % cfg.n_cls).view(-1, 1).cuda()
    opt = FusedAdam(fp, lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=1e4, update_tail=True)
    met = StepMetrics("cuda", 1)
    step, info = make_dp_step(model, opt, red, xs, ys, ms, warmup=1, cls=cls, cls_weight=0.0, metrics=met)
    torch.cuda.synchronize()
    assert met.read()["opt_steps"] == 0                          # neither the warm-up nor the trial steps are logged
    tail_launches = []
    real = red._launch

    def spy(k):
        if k == red.tail_bucket:
            tail_launches.append(k)
        return real(k)

    red._launch = spy
    for _ in range(2):
        step.replay(1e-3)
    torch.cuda.synchronize()
    red._launch = real
    local, summed = met.read(), met.read(red)
    torch.save(dict(local=local, summed=summed, mode=info["mode"], tail=len(tail_launches), n=int(xs.shape[0])),
               os.path.join(out_dir, f"{backend}_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_read_group_sums_over_the_ranks_and_the_zero_tail_shortcut_stays(tmp_path):
    """(a) one-rank RCCL communicator: the one-graph step captures with the metrics launches inside, read(reducer) equals
    the local read; (b) two ranks over gloo (segmented chain): read(reducer) is the sum over the ranks, and with
    cls_weight = 0 the cls_head tail bucket launches no collective"""
    import torch.multiprocessing as mp
    mp.spawn(_dp_worker, args=(1, _free_port(), str(tmp_path), "nccl"), nprocs=1, join=True)
    a = torch.load(os.path.join(str(tmp_path), "nccl_0.pt"))
    assert a["mode"] == "one-graph" and a["summed"] == a["local"]
    assert (a["local"]["opt_steps"], a["local"]["samples"], a["local"]["cls_total"]) == (2, 8, 8)
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path), "gloo"), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(str(tmp_path), f"gloo_{r}.pt")) for r in (0, 1))
    assert r0["mode"] == "segmented" and r0["tail"] == 0 and r1["tail"] == 0
    assert r0["summed"] == r1["summed"]
    s = r0["summed"]
    for key in ("l2_step", "l2_full", "cls_loss", "grad_norm"):
        assert s[key] == r0["local"][key] + r1["local"][key], key      # one float64 sum of two terms: exact either way
    for key in ("cls_correct", "cls_total", "samples", "ar_steps", "opt_steps"):
        assert s[key] == r0["local"][key] + r1["local"][key], key
    assert (s["samples"], s["opt_steps"], s["cls_total"]) == (8, 4, 8)
    assert np.isfinite(s["l2_step"]) and s["l2_step"] > 0 and s["cls_loss"] > 0
