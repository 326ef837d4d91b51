"""GPU tests of the CDPOT model: the anti-aliased activation kernels (csrc/aa_act.hip, ops.aa_lrelu / aa_lrelu_bwd,
functional.AALReLUFn) against the float64 restatement (tests/cdpot_ref.py) and the reference's records (g21_cdpot), and
CDPOTNet through the training step, the captured step and the rollouts.  The operator tests run on the guarded, poisoned
allocator (tests/guard.py)."""
import functools
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import cdpot_ref as CR
import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close, load
from oracle import dpot_ref as R
from resize_ref import resize_ref

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24          # unit roundoff of float32


def _ids(c):
    N, h, w, C, Cb, out, _ = c
    return f"n{N}_{h}x{w}_c{C}_b{Cb}_" + ("none" if out is None else f"{out[0]}x{out[1]}")


def _run_op(x, g, bias, out):
    from dpot_amd.functional import AALReLUFn
    xd = guard.wrap(x, "cuda").requires_grad_(True)
    bd = guard.wrap(bias, "cuda").requires_grad_(True)
    y = AALReLUFn.apply(xd, bd, out, CR.SLOPE)
    y.backward(guard.wrap(g, "cuda"))
    torch.cuda.synchronize()
    return y.detach(), xd.grad, bd.grad


@pytest.mark.parametrize("case", CR.GPU_OP_CASES, ids=_ids)
def test_operator_vs_restatement(case, guarded):
    N, h, w, C, Cb, out, _ = case
    x, g, bias = CR.gpu_op_inputs(case)
    y, dx, db = _run_op(x, g, bias, out)
    y64, dx64, db64 = CR.run_op_ref(x, g, bias, out)
    assert tuple(y.shape) == (N,) + (out or (h, w)) + (C,)
    assert_close(y, y64, f"aa_lrelu {_ids(case)} y")
    assert_close(dx, dx64, f"aa_lrelu {_ids(case)} dx")
    assert_close(db, db64, f"aa_lrelu {_ids(case)} dbias")


def _nerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("name", list(CR.OP_CASES))
def test_operator_vs_reference_fixture_and_its_float32_error(name, guarded):
    """Against the reference's float64 record, and norm-wise beside the reference's own float32 figure.  The allowed factor over
    that figure is the ratio of the lengths of the longest chains of rounded operations behind one element (worst-case error
    bounds grow linearly with them), from the tap counts; a figure below the unit roundoff 2^-24 is raised to it (no float32
    result is better than its own rounding):
      y   kernel: 4 (the 2 x 2 taps of an up-sampled value) + 16 (the 4 x 4 taps of D, one fma each) + 4 (V) + 1 (bias) = 25;
          reference, separable: (2 + 2) + (4 + 4) + (2 + 2) + 1 = 17.  25 / 17 < 2.
      dx  with r = ceil(H / h), V^T has at most 2 r + 1 taps per axis.  kernel: 2 (2 r + 1) (V^T, rows then columns) + 4 (D^T)
          + 16 (U^T); reference: 2 (2 r + 1) + (2 + 2) + (4 + 4).  (20 + t) / (12 + t) < 2.
      db  kernel: the chain of one g value, then per sample and channel at most npix / 8 + 64 sequential additions (256 / CHW
          >= 8 sub-sums of npix * CHW / 256 pixels each, then the sub-sums), then the N * C / Cb rows of colsum; reference: a
          pairwise sum of N * H * W terms, ceil(log2) + 1 levels.  The factor is that ratio, computed below."""
    fx = load("g21_cdpot")
    N, h, C, out = CR.OP_CASES[name]
    x, g, bias = CR.op_inputs(name)
    y, dx, db = _run_op(x, g, bias, out)
    H = out or h
    r = math.ceil(H / h)
    t = 2 * (2 * r + 1) if out else 0
    factor = {"y": 2.0, "dx": 2.0,
              "db": max(2.0, (t + h * h / 8 + 64 + N) / (math.ceil(math.log2(N * H * H)) + 1))}
    got = {"y": y, "dx": dx, "db": db}
    for k in ("y", "dx", "db"):
        ref = fx[f"op.{name}.{k}64"]
        e_ref, e_got = float(fx[f"op.{name}.e32.{k}"]), _nerr(got[k].cpu().numpy(), ref)
        print(f"aa-error {name}.{k}: kernel {e_got:.3e}  reference-fp32 {e_ref:.3e}  allowed {factor[k]:.2f} x "
              f"max(reference, 2^-24)")
    for k in ("y", "dx", "db"):
        ref = fx[f"op.{name}.{k}64"]
        assert_close(got[k], ref, f"op.{name}.{k} vs reference")
        e_ref, e_got = float(fx[f"op.{name}.e32.{k}"]), _nerr(got[k].cpu().numpy(), ref)
        assert e_got <= factor[k] * max(e_ref, U32), (name, k, e_got, e_ref)


@pytest.mark.parametrize("shape,out", [((2, 5, 7, 3), None), ((1, 8, 8, 36), (32, 32)), ((3, 2, 2, 35), (10, 10))])
def test_zero_input_gradient_is_slope_times_the_linear_operator(shape, out, guarded):
    """at exactly 0 the derivative is the slope: dx = slope * U^T D^T V^T dy V D U"""
    from dpot_amd import ops
    N, h, w, C = shape
    H, W = out or (h, w)
    x = torch.zeros(shape)
    g = CR.hash_input((N, H, W, C), 77)
    bias = ((R.recipe_tensor("aa_bias", (C,), 77) - 0.5) * 0.4).float()
    y, dx, db = _run_op(x, g, bias, out)
    assert torch.equal(y.cpu(), bias.expand(N, H, W, C))
    mats = [torch.from_numpy(ops.aa_resize_matrix(*p)) for p in ((h, 2 * h), (2 * h, h), (h, H), (w, 2 * w), (2 * w, w), (w, W))]
    Lh, Lw = mats[2] @ mats[1] @ mats[0], mats[5] @ mats[4] @ mats[3]               # V D U per axis
    want = CR.SLOPE * torch.einsum("Ip,nIJc,Jq->npqc", Lh, g.double(), Lw)
    assert_close(dx, want, "dx at x = 0")
    assert_close(dx, CR.run_op_ref(x, g, bias, out)[1], "dx at x = 0 vs restatement")
    assert_close(db, g.double().sum((0, 1, 2)), "dbias")


@pytest.mark.parametrize("case", [(2, 5, 7, 35, 7, None), (2, 16, 16, 36, 36, (80, 80)), (3, 7, 7, 3, 3, (30, 30)),
                                  (1, 64, 64, 8, 8, None), (2, 32, 32, 40, 4, (64, 64))], ids=lambda c: _ids(c + (0,)))
def test_operator_is_deterministic_and_stays_inside_its_output(case, guarded):
    """two launches give identical bits, forward and backward; out= into a guarded NaN slot is written completely and nothing
    around it is touched"""
    from dpot_amd import ops
    N, h, w, C, Cb, out = case
    H, W = out or (h, w)
    x0 = CR.hash_input((N, h, w, C), 91)
    x = guard.wrap(x0, "cuda")
    g0 = CR.hash_input((N, H, W, C), 92)
    g = guard.wrap(g0, "cuda")
    b0 = ((R.recipe_tensor("aa_bias", (Cb,), 91) - 0.5) * 0.4).float()
    bias = guard.wrap(b0, "cuda")
    out1, out2 = guard.full_nan((N, H, W, C)), guard.full_nan((N, H, W, C))
    r1 = ops.aa_lrelu(x, bias, out, CR.SLOPE, out=out1)
    r2 = ops.aa_lrelu(x, bias, out, CR.SLOPE, out=out2)
    dx1, db1 = ops.aa_lrelu_bwd(x, g, Cb, CR.SLOPE)
    dx2, db2 = ops.aa_lrelu_bwd(x, g, Cb, CR.SLOPE)
    torch.cuda.synchronize()
    assert r1 is out1 and r2 is out2
    assert torch.equal(out1.view(torch.int32), out2.view(torch.int32))
    assert torch.equal(dx1.view(torch.int32), dx2.view(torch.int32)) and torch.equal(db1.view(torch.int32), db2.view(torch.int32))
    assert_close(out1, CR.aa_lrelu_ref(x0.double(), b0.double(), out), f"aa_lrelu {case} into out=")
    guard.check()


def test_operator_argument_checks():
    from dpot_amd import _lib, ops
    err = (ValueError, _lib.DpotHipError)
    x = torch.zeros(2, 8, 8, 6, device="cuda")
    b = torch.zeros(6, device="cuda")
    with pytest.raises(err):
        ops.aa_lrelu(torch.zeros(1, 65, 8, 2, device="cuda"), torch.zeros(2, device="cuda"))      # latent size beyond 64
    with pytest.raises(err):
        ops.aa_lrelu(x, b, (4, 16))                                                                # output below the input
    with pytest.raises(err):
        ops.aa_lrelu(x, b, (8, 2048))                                                              # output beyond the limit
    with pytest.raises(err):
        ops.aa_lrelu(x, torch.zeros(4, device="cuda"))                                             # 6 % 4 != 0
    with pytest.raises(err):
        ops.aa_lrelu(x.double(), b.double())
    with pytest.raises(err):
        ops.aa_lrelu(x.permute(0, 2, 1, 3)[:, ::2], b)
    with pytest.raises(err):
        ops.aa_lrelu(x, b, out=x)
    with pytest.raises(err):
        ops.aa_lrelu(x, b, 16, out=torch.zeros(2, 16, 8, 6, device="cuda"))
    with pytest.raises(err):
        ops.aa_lrelu_bwd(x, torch.zeros(2, 8, 8, 6, device="cuda").double(), 6)
    lib = _lib.load()                                       # the C entry points: DPOT_EUNSUP with the size named, nothing launched
    s = torch.cuda.current_stream().cuda_stream
    d = torch.zeros(4, device="cuda")
    t = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert lib.dpot_aa_lrelu_fwd(d.data_ptr(), None, x.data_ptr(), t.data_ptr(), 1, 65, 4, 1, 1, 0.01, s) == -2
    assert b"65x4" in lib.dpot_last_error()
    assert lib.dpot_aa_lrelu_bwd(d.data_ptr(), d.data_ptr(), x.data_ptr(), b.data_ptr(), t.data_ptr(), 1, 4, 65, 1, 0.01, s) == -2
    assert lib.dpot_aa_up_fwd(d.data_ptr(), None, x.data_ptr(), t.data_ptr(), 1, 2, 2, 1, 2, 1, 1, s) == -2
    assert b"1x2" in lib.dpot_last_error()
    assert lib.dpot_aa_up_adj(d.data_ptr(), x.data_ptr(), t.data_ptr(), 1, 2, 2, 2, 2000, 1, s) == -2
    torch.cuda.synchronize()
    assert not d.any()


@pytest.mark.parametrize("out", [None, (40, 40)])
def test_operator_under_graph_capture_replays_to_the_eager_bits(out):
    from dpot_amd import _lib, ops
    x = CR.hash_input((3, 8, 8, 35), 11).cuda()
    bias = CR.hash_input((7,), 12).cuda()
    g = CR.hash_input((3,) + (out or (8, 8)) + (35,), 13).cuda()
    eager = ops.aa_lrelu(x, bias, out)                      # builds the plan outside the capture
    edx, edb = ops.aa_lrelu_bwd(x, g, 7)
    static_out = torch.full_like(eager, float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.aa_lrelu(x, bias, out, out=static_out)
        dx, db = ops.aa_lrelu_bwd(x, g, 7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out.view(torch.int32), eager.view(torch.int32))
    assert torch.equal(dx.view(torch.int32), edx.view(torch.int32)) and torch.equal(db.view(torch.int32), edb.view(torch.int32))
    x.copy_(CR.hash_input((3, 8, 8, 35), 14))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out.view(torch.int32), ops.aa_lrelu(x, bias, out).view(torch.int32))
    assert torch.equal(dx.view(torch.int32), ops.aa_lrelu_bwd(x, g, 7)[0].view(torch.int32))


def test_plan_under_capture_is_an_error(monkeypatch):
    """a size tuple first seen while the stream captures: an error that says what to do, before anything is uploaded (the
    capture state is stubbed: aborting a real capture is not something a test should leave behind)"""
    from dpot_amd import _lib, ops
    x = torch.zeros(1, 3, 9, 4, device="cuda")              # a size tuple no other test uses
    bias = torch.zeros(4, device="cuda")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.DpotHipError, match="before capturing"):
        ops.aa_lrelu(x, bias)
    monkeypatch.undo()
    assert tuple(ops.aa_lrelu(x, bias).shape) == (1, 3, 9, 4)


# ---- the model -----------------------------------------------------------------------------------------------------------
def build(cfg, salt):
    from dpot_amd import CDPOTNet
    m = CDPOTNet(**cfg)
    sd = CR.recipe_sd(OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items()), cfg, salt)
    m.load_state_dict(sd, strict=True)
    return m.cuda(), sd


@pytest.mark.parametrize("tag", list(CR.MODELS))
def test_mini_model_vs_reference(tag):
    from dpot_amd.functional import rel_l2_loss
    fx = load("g21_cdpot")
    cfg, salt = CR.MODELS[tag]
    m, _ = build(cfg, salt)
    x, y, msk, gc = (t.cuda() for t in CR.model_inputs(tag))
    x.requires_grad_(True)
    pred, cls_pred = m(x)
    (rel_l2_loss(pred, y, msk) + (cls_pred * gc).sum()).backward()
    torch.cuda.synchronize()
    for k, t in (("pred", pred), ("cls_pred", cls_pred)):
        ref = torch.from_numpy(fx[f"{tag}.{k}"]).double()
        print(f"{tag}.{k}: kernels {(t.detach().double().cpu() - ref).abs().max().item() / ref.abs().max().item():.2e}  "
              f"reference-fp32 {float(fx[f'{tag}.err32.{k}']):.2e} (max|d| / max|float64|)")
    assert_close(pred, fx[f"{tag}.pred"], f"{tag}.pred")
    assert_close(cls_pred, fx[f"{tag}.cls_pred"], f"{tag}.cls_pred")
    assert_close(x.grad.reshape(-1)[::CR.DX_STRIDE], fx[f"{tag}.dx"], f"{tag}.dx")
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert sorted(grads) == sorted(str(n) for n in fx[f"{tag}.gnames"])
    for k, g in grads.items():
        assert g is not None, k
        assert_close(g, fx[f"{tag}.g.{k}"], f"{tag}.g.{k}")


def _per_tensor(model, names, flat_of):
    """[(name, every STEP_STRIDE-th element of the concatenation that falls into this tensor)] as the fixture stores them"""
    params = dict(model.named_parameters())
    flat = torch.cat([flat_of(params[n]).detach().reshape(-1) for n in names]).cpu()
    owner = torch.cat([torch.full((params[n].numel(),), i, dtype=torch.int64) for i, n in enumerate(names)])
    return flat[::CR.STEP_STRIDE], owner[::CR.STEP_STRIDE]


def _step_batch():
    return tuple(t.cuda() for t in CR.step_inputs())


def _opt(m, update_tail=False):
    from dpot_amd.train import FlatParams, FusedAdam
    st = CR.STEP
    return FusedAdam(FlatParams(m), lr=st["lr"], betas=st["betas"], weight_decay=st["weight_decay"], max_norm=st["max_norm"],
                     update_tail=update_tail)


def test_two_ar_step_train_step_vs_reference():
    """train_temporal.py's loop, two AR steps, noise off: loss, gradient before the clip, its norm, parameters after Adam.

    Gradient: per tensor at the contract, tol_g = 1e-4 |g| + 1e-4 max|g|.  Parameters: per tensor at the contract PLUS what
    Adam's first step makes of a gradient that differs within tol_g.  That step moves a parameter by lr u(g'), u(x) = x / (|x| + eps),
    g' = c g + wd p (c the clip coefficient): a step of size lr whatever |g'| is, so where |g'| is not far above eps = 1e-8 the
    size of the move depends on the gradient's last bits - the reference's own float32 gradient is rounding noise there.
    u' = eps / (|x| + eps)^2 falls with |x|, so two gradients within c tol_g of each other give moves within
        lr min(2, c tol_g eps / (max(0, |g'| - c tol_g) + eps)^2)
    of each other.  For |g'| >= 1e-5 that is below 1e-7 lr; it only matters for the few elements whose gradient nearly vanishes
    (21 of the 5895 recorded elements get more than 1e-3 lr; seen: one element of pos_embed, gradient 5e-8 against a largest one of
    0.026, off by 0.0065 lr)."""
    from dpot_amd.train import train_step
    fx = load("g21_cdpot")
    st = CR.STEP
    m, sd0 = build(CR.MINI1, st["salt"])
    xx, yy, msk = _step_batch()
    opt = _opt(m)
    cls_before = [p.detach().clone() for p in m.cls_head.parameters()]
    loss, pred = train_step(m, opt, xx, yy, msk, lr=st["lr"])
    torch.cuda.synchronize()
    assert tuple(pred.shape) == tuple(yy.shape)
    assert_close(loss, fx["step.loss"], "step loss")
    gnorm = float(fx["step.grad_norm"])
    assert abs(opt.grad_norm().item() - gnorm) <= 1e-4 * gnorm
    names = [str(n) for n in fx["step.names"]]
    assert names == [n for n, _ in m.named_parameters() if not n.startswith("cls_head.")]
    assert [str(n) for n in fx["step.nograd"]] == [n for n, _ in m.named_parameters() if n.startswith("cls_head.")]
    got_g, owner = _per_tensor(m, names, lambda p: p.grad)
    got_p, _ = _per_tensor(m, names, lambda p: p)
    ref_g, ref_p = torch.from_numpy(fx["step.grad"]).double(), torch.from_numpy(fx["step.params"]).double()
    p0 = torch.cat([sd0[n].reshape(-1) for n in names])[::CR.STEP_STRIDE].double()
    assert got_g.shape == ref_g.shape and got_p.shape == ref_p.shape
    c = min(1.0, st["max_norm"] / (gnorm + 1e-6))
    eps = 1e-8
    for i, n in enumerate(names):
        sel = owner == i
        if not sel.any():
            continue
        assert_close(got_g[sel], ref_g[sel], f"step gradient {n}")
        g, p = ref_g[sel], ref_p[sel]
        tol_g = c * (1e-4 * g.abs() + 1e-4 * g.abs().max())
        geff = (c * g + st["weight_decay"] * p0[sel]).abs()
        move = st["lr"] * torch.clamp(tol_g * eps / ((geff - tol_g).clamp(min=0.0) + eps) ** 2, max=2.0)
        err = (got_p[sel].double() - p).abs()
        tol = 1e-4 * p.abs() + 1e-4 * p.abs().max() + move
        assert torch.isfinite(got_p[sel]).all() and (err <= tol).all(), \
            (f"step parameters {n}: {int((err > tol).sum())}/{err.numel()} out of tolerance, worst {float((err - tol).max()):.3e} "
             f"over it; {int((move > 1e-3 * st['lr']).sum())} elements carry an Adam allowance above 1e-3 lr")
    for p, q in zip(m.cls_head.parameters(), cls_before):                          # no gradient: untouched, as the reference
        assert torch.equal(p.detach(), q)


@pytest.mark.parametrize("with_cls", [False, True], ids=["plain", "cls_metrics"])
def test_graphed_train_step_vs_eager(with_cls):
    from dpot_amd import StepMetrics
    from dpot_amd.train import GraphedTrainStep, train_step
    st = CR.STEP
    xx, yy, msk = _step_batch()
    cls = torch.tensor([2, 0], device="cuda")
    runs = []
    for graphed in (False, True):
        m, _ = build(CR.MINI1, st["salt"])
        opt = _opt(m, update_tail=with_cls)          # a weighted classification loss trains cls_head
        met = StepMetrics("cuda", st["T_ar"]) if with_cls else None
        kw = dict(cls=cls, cls_weight=0.3, metrics=met) if with_cls else {}
        if graphed:
            step = GraphedTrainStep(m, opt, xx, yy, msk, warmup=1, **kw)
            snap = opt.snapshot()
            msnap = met.snapshot() if met is not None else None
            loss, pred = step.replay(st["lr"]).clone(), step.pred.clone()
            flat = opt.fp.flat.clone()
            opt.restore(snap)
            if met is not None:
                met.restore(msnap)
            loss2, pred2 = step.replay(st["lr"]).clone(), step.pred.clone()
            torch.cuda.synchronize()
            assert torch.equal(loss, loss2) and torch.equal(pred, pred2) and torch.equal(flat, opt.fp.flat)   # bit for bit
        else:
            loss, pred = train_step(m, opt, xx, yy, msk, lr=st["lr"], **kw)
        torch.cuda.synchronize()
        runs.append((loss.clone(), pred.clone(), {n: p.detach().clone() for n, p in m.named_parameters()},
                     met.read() if met is not None else None))
    (l0, p0, w0, d0), (l1, p1, w1, d1) = runs
    assert_close(l1, l0, "graphed loss")
    assert_close(p1, p0, "graphed pred")
    for n in w0:
        assert_close(w1[n], w0[n], f"graphed parameters {n}")
    if with_cls:
        moved = [n for n in w0 if n.startswith("cls_head.")]
        m0, _ = build(CR.MINI1, st["salt"])
        start = dict(m0.named_parameters())
        assert all(not torch.equal(w0[n], start[n].detach()) for n in moved)       # cls_weight != 0: the head trains
        for k in ("l2_step", "l2_full", "cls_loss", "grad_norm"):
            assert_close(torch.tensor(d1[k]), torch.tensor(d0[k]), f"metrics {k}")
        for k in ("cls_correct", "cls_total", "samples", "ar_steps", "opt_steps"):
            assert d1[k] == d0[k], k
        assert d0["opt_steps"] == 1 and d0["cls_total"] == 2 * st["T_ar"]


@functools.lru_cache(maxsize=None)
def _rollout_model():
    m, sd = build(CR.MINI1, 450)
    return m.eval(), {k: v.double() for k, v in sd.items()}


def _ref_rollout(sd, xx, yy, msk, model_res=None):
    """evaluate.py / evaluate_varyingres.py with the float64 restatement of the model and of the Fourier resize"""
    data_res = tuple(xx.shape[1:3])
    xx, yy, msk = xx.double(), yy.double(), msk.double()
    loss, preds = 0.0, []
    for t in range(yy.shape[-2]):
        inp = torch.from_numpy(resize_ref(xx.numpy(), model_res)) if model_res is not None else xx
        im, _ = CR.cdpot_forward(sd, inp, CR.MINI1)
        if model_res is not None:
            im = torch.from_numpy(resize_ref(im.numpy(), data_res))
        loss = loss + R.rel_l2_loss(im, yy[..., t:t + 1, :], msk)
        preds.append(im)
        xx = torch.cat((xx[..., 1:, :], im), dim=-2)
    pred = torch.cat(preds, dim=-2)
    return pred, loss, R.rel_l2_loss(pred, yy, msk)


@pytest.mark.parametrize("res", [None, 13], ids=["model_resolution", "data13_model20"])
def test_rollout_eval_and_graphed_rollout(res):
    from dpot_amd.infer import GraphedRollout, refill_mask, rollout_eval
    m, sd = _rollout_model()
    cfg = CR.MINI1
    B, T_ar, S = 2, 3, cfg["img_size"]
    D = res or S
    xx = CR.hash_input((B, D, D, cfg["in_timesteps"], cfg["in_channels"]), 451)
    yy = CR.hash_input((B, D, D, T_ar, cfg["out_channels"]), 452)
    msk0 = torch.ones(B, S, S, 1, cfg["out_channels"])
    msk0[1, :, :, :, 2] = 0.0
    msk = refill_mask(msk0.cuda(), D) if res else msk0.cuda()
    kw = dict(model_res=S) if res else {}
    with torch.no_grad():
        pred_ref, steps_ref, full_ref = _ref_rollout(sd, xx, yy, msk.cpu(), (S, S) if res else None)
    pred, l_steps, l_full = rollout_eval(m, xx.cuda(), yy.cuda(), msk, **kw)
    assert tuple(pred.shape) == (B, D, D, T_ar, cfg["out_channels"])
    assert_close(pred, pred_ref, "rollout pred")
    assert_close(l_steps, steps_ref, "sum of step losses")
    assert_close(l_full, full_ref, "full-trajectory loss")
    g = GraphedRollout(m, torch.zeros(B, S, S, cfg["in_timesteps"], cfg["in_channels"], device="cuda"))
    pred_g, l_steps_g, l_full_g = g(xx.cuda(), yy.cuda(), msk, **kw)
    torch.cuda.synchronize()
    assert torch.equal(pred_g, pred) and torch.equal(l_steps_g, l_steps) and torch.equal(l_full_g, l_full)


def test_rollout_evaluator_and_checkpoint_loader():
    from dpot_amd import CDPOTNet, RolloutEvaluator
    from dpot_amd.infer import GraphedRollout, load_model_from_checkpoint, rollout_eval
    m, _ = _rollout_model()
    cfg = CR.MINI1
    B, T_ar, S = 2, 2, cfg["img_size"]
    xx = CR.hash_input((B, S, S, cfg["in_timesteps"], cfg["in_channels"]), 461).cuda()
    yy = CR.hash_input((B, S, S, T_ar, cfg["out_channels"]), 462).cuda()
    msk = torch.ones(B, S, S, 1, cfg["out_channels"], device="cuda")
    m2 = CDPOTNet(**cfg)
    load_model_from_checkpoint(m2, {"model": OrderedDict(("module." + k, v.cpu()) for k, v in m.state_dict().items())})
    m2 = m2.cuda().eval()
    ev1, ev2 = (RolloutEvaluator("cuda", cfg["out_channels"], T_ar, ilow=2, ihigh=6) for _ in range(2))
    p1, _, _ = rollout_eval(m, xx, yy, msk, evaluator=ev1)
    p2, _, _ = GraphedRollout(m2, xx)(xx, yy, msk, evaluator=ev2)
    torch.cuda.synchronize()
    assert torch.equal(p1, p2)
    r1, r2 = ev1.read(), ev2.read()
    assert set(r1) == set(r2)
    for k in r1:
        assert np.array_equal(np.asarray(r1[k]), np.asarray(r2[k])), k
