"""GPU tests of dpot_amd.UNet on the width-2 fixture (tests/golden/g24_unet.npz, written from the reference's own UNet): forward
and gradients in both windows, two training steps with the BatchNorm buffers, the captured step (warm-up leaves no trace in
parameters OR buffers), and the rollouts in eval mode."""
import functools

import pytest
import torch

import unet_ref as UR
from helpers import assert_close, load

pytestmark = pytest.mark.gpu

CFG = UR.CFG


def build(in_shape=(32, 32), sd=None):
    from dpot_amd import UNet
    m = UNet(2, **dict(CFG, in_shape=in_shape))
    m.load_state_dict(sd if sd is not None else UR.fixture_sd(load("g24_unet")), strict=True)
    return m.cuda()


def _opt(m):
    from dpot_amd.train import FlatParams, FusedAdam
    st = UR.STEP
    return FusedAdam(FlatParams(m), lr=st["lr"], betas=st["betas"], weight_decay=st["weight_decay"], max_norm=st["max_norm"])


def _buffers(m):
    return {n: b.detach().clone() for n, b in m.named_buffers()}


def _params(m):
    return {n: p.detach().clone() for n, p in m.named_parameters()}


def _same(a, b):
    assert list(a) == list(b)
    for n in a:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("tag", list(UR.WINDOWS))
def test_forward_and_gradients_vs_the_reference(tag):
    """the 1e-4 contract against the fixture, and per tensor the error against the reference's float64 record beside the
    reference's own float32 error against it: at most 4 times that (both are fp32 sums of the same lengths in another order;
    4 is the scatter between seeds of the reference's own float32 run on the same kind of tensor, 1.0e-5 to 3.2e-5), or 2e-6 of
    the tensor's maximum, whichever is larger.  Prediction: norm-wise; gradients: max|d| / max|float64|, as the fixture records
    them (a tensor of more than 2048 elements on every third element).
    Measured on MI355X: see the README's section "The UNet baseline"."""
    from dpot_amd.functional import rel_l2_loss
    fx = load("g24_unet")
    B, in_shape = UR.WINDOWS[tag]
    m = build(in_shape).train()
    x, y = (t.cuda() for t in UR.window_inputs(tag))
    pred, cls = m(x)
    assert tuple(pred.shape) == tuple(y.shape) and tuple(cls.shape) == (B, CFG["n_cls"])
    assert not cls.requires_grad and not bool(cls.any())
    rel_l2_loss(pred, y, None).backward()
    torch.cuda.synchronize()
    p64 = torch.from_numpy(fx[f"{tag}.pred64"])
    assert_close(pred, p64, f"{tag}.pred")
    e, e_ref = UR.nerr(pred.detach().cpu().numpy(), p64.numpy()), float(fx[f"{tag}.err32.pred"])
    print(f"unet-error {tag}.pred: kernels {e:.3e}  reference-fp32 {e_ref:.3e}  ratio {e / e_ref:.2f}")
    assert e <= max(4 * e_ref, 2e-6), (tag, "pred", e, e_ref)
    layout = UR.param_layout(fx)
    grads = dict(m.named_parameters())
    assert [n for n, _ in layout] == list(grads)
    pieces = UR.unpack(torch.from_numpy(fx[f"{tag}.g64"]), [s for _, s in layout])
    worst = 0.0
    failed = []
    for i, ((name, shape), rec) in enumerate(zip(layout, pieces)):
        g = grads[name].grad
        assert g is not None and tuple(g.shape) == shape, name
        got = UR.sub(g.detach().cpu()).reshape(-1)
        assert_close(got, rec, f"{tag}.g.{name}")
        e = float((got.double() - rec).abs().max() / rec.abs().max())
        e_ref = float(fx[f"{tag}.err32.g"][i])
        worst = max(worst, e / max(e_ref, 1e-30))
        print(f"unet-error {tag}.g.{name}: kernels {e:.3e}  reference-fp32 {e_ref:.3e}  ratio {e / max(e_ref, 1e-30):.2f}")
        if e > max(4 * e_ref, 2e-6):
            failed.append((name, e, e_ref))
    print(f"unet-error {tag}: worst gradient ratio {worst:.2f}")
    assert not failed, failed


def test_one_value_per_channel_raises_in_training_mode():
    m = build((16, 16)).train()
    x = torch.zeros(1, 16, 16, CFG["in_timesteps"], CFG["in_channels"], device="cuda")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(x)
    m.eval()
    with torch.no_grad():
        assert tuple(m(x)[0].shape) == (1, 16, 16, 1, CFG["out_channels"])


@functools.lru_cache(maxsize=None)
def _step1_gradients():
    """float64 gradients of the first step, all elements, from the restatement (held to the reference's float64 records by
    tests/test_cpu_unet.py): the clip coefficient and Adam's sensitivity below need every element"""
    fx = load("g24_unet")
    x, y = UR.window_inputs("a")
    ref = UR.Model(UR.fixture_sd(fx), (32, 32), CFG["out_timesteps"], CFG["out_channels"], CFG["act"])
    pred = ref.forward(x.double(), train=True)
    return ref.backward(UR.rel_l2(pred, y.double())[1])


def test_two_training_steps_vs_the_reference():
    """two eager train_steps (FusedAdam, noise off) against the reference's loop: the losses, the buffers after each step, the
    parameters after both, the eval-mode prediction afterwards.  Parameters: the contract plus what two Adam steps (each a move
    of size lr whatever |g| is) make of a gradient that differs within the gradient tolerance - the allowance of
    tests/test_gpu_fno.py's step test, lr min(2, c tol_g eps / (max(0, |g'| - c tol_g) + eps)^2) with g' = c g + wd p and c the
    clip coefficient, taken twice with the first step's gradient."""
    from dpot_amd.train import train_step
    fx = load("g24_unet")
    st = UR.STEP
    m = build().train()
    opt = _opt(m)
    x, y = (t.cuda() for t in UR.window_inputs("a"))
    blayout, players = UR.buffer_layout(fx), UR.param_layout(fx)
    for k in (1, 2):
        loss, pred = train_step(m, opt, x, y, None, lr=st["lr"])
        torch.cuda.synchronize()
        assert_close(loss, fx["step.loss"][k - 1], f"loss of step {k}")
        bufs = dict(m.named_buffers())
        assert list(bufs) == [n for n, _ in blayout]
        for (name, shape), rec in zip(blayout, UR.unpack(torch.from_numpy(fx[f"step.buf{k}"]), [s for _, s in blayout])):
            if name.endswith("num_batches_tracked"):
                assert int(bufs[name]) == k == int(rec), name
            else:
                assert_close(bufs[name].reshape(-1), rec, f"step {k} {name}")
    g1 = _step1_gradients()
    gnorm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g1.values())))
    c, eps = min(1.0, st["max_norm"] / (gnorm + 1e-6)), 1e-8
    sd0 = UR.fixture_sd(fx)
    params = dict(m.named_parameters())
    for (name, shape), rec in zip(players, UR.unpack(torch.from_numpy(fx["step.p"]), [s for _, s in players])):
        got, g, p0 = (UR.sub(t.detach().cpu()).reshape(-1).double() for t in (params[name], g1[name], sd0[name]))
        rec = rec.double()
        tol_g = c * (1e-4 * g.abs() + 1e-4 * g.abs().max())
        geff = (c * g + st["weight_decay"] * p0).abs()
        move = 2 * st["lr"] * torch.clamp(tol_g * eps / ((geff - tol_g).clamp(min=0.0) + eps) ** 2, max=2.0)
        tol = 1e-4 * rec.abs() + 1e-4 * rec.abs().max() + move
        err = (got - rec).abs()
        assert torch.isfinite(got).all() and (err <= tol).all(), \
            f"parameters {name}: {int((err > tol).sum())}/{err.numel()} out of tolerance, worst {float((err - tol).max()):.3e} over it"
    m.eval()
    with torch.no_grad():
        pred = m(x)[0]
    torch.cuda.synchronize()
    assert_close(pred, fx["step.eval_pred"], "eval-mode prediction after two steps")
    assert not m.training


def test_graphed_train_step_leaves_no_trace_and_replays_the_eager_step():
    """directly after construction parameters AND buffers hold the bits they held before (the warm-up steps are no training
    steps: train.trial_state puts the model's persistent buffers back too); two replays equal two eager steps bit for bit"""
    from dpot_amd.train import GraphedTrainStep, train_step
    st = UR.STEP
    x, y = (t.cuda() for t in UR.window_inputs("a"))
    eager = build().train()
    opt_e = _opt(eager)
    for _ in range(2):
        train_step(eager, opt_e, x, y, None, lr=st["lr"])
    torch.cuda.synchronize()

    m = build().train()
    opt = _opt(m)
    p0, b0 = _params(m), _buffers(m)
    step = GraphedTrainStep(m, opt, x, y, None, warmup=2)
    torch.cuda.synchronize()
    _same(_params(m), p0)
    _same(_buffers(m), b0)
    assert int(m.bottleneck.bottlenecknorm1.num_batches_tracked) == 0
    for _ in range(2):
        step.replay(st["lr"])
    torch.cuda.synchronize()
    _same(_params(m), _params(eager))
    _same(_buffers(m), _buffers(eager))
    assert int(m.decoder1.dec1norm2.num_batches_tracked) == 2


@pytest.mark.parametrize("training", [True, False], ids=["train_mode_before", "eval_mode_before"])
def test_rollouts_run_in_eval_mode_and_leave_the_model_as_found(training):
    from dpot_amd import RolloutEvaluator, StepMetrics
    from dpot_amd.infer import GraphedRollout, rollout_eval
    fx = load("g24_unet")
    sd = UR.fixture_sd(fx)
    for k in sd:                                      # running statistics that are neither 0 nor 1
        if k.endswith("running_mean"):
            sd[k] = UR.hash_input(tuple(sd[k].shape), 801) * 0.1
        elif k.endswith("running_var"):
            sd[k] = UR.hash_input(tuple(sd[k].shape), 802).abs() + 0.5
    m = build(sd=sd).train(training)
    B, T_ar = 2, 3
    xx = UR.hash_input((B, 32, 32, CFG["in_timesteps"], CFG["in_channels"]), 803).cuda()
    yy = UR.hash_input((B, 32, 32, T_ar, CFG["out_channels"]), 804).cuda()
    b0 = _buffers(m)
    pred, l_steps, l_full = rollout_eval(m, xx, yy, None)
    assert m.training is training
    g = GraphedRollout(m, torch.zeros_like(xx))
    assert m.training is training
    pred_g, l_steps_g, l_full_g = g(xx, yy, None)
    torch.cuda.synchronize()
    assert tuple(pred.shape) == (B, 32, 32, T_ar, CFG["out_channels"])
    assert torch.equal(pred_g, pred) and torch.equal(l_steps_g, l_steps) and torch.equal(l_full_g, l_full)
    _same(_buffers(m), b0)
    # the first AR step against the float64 restatement in eval mode
    ref = UR.Model(sd, (32, 32), CFG["out_timesteps"], CFG["out_channels"], CFG["act"])
    assert_close(pred[..., :1, :], ref.forward(xx.cpu().double(), train=False), "first AR step, eval mode")
    ev, met = RolloutEvaluator("cuda", CFG["out_channels"], T_ar), StepMetrics("cuda", T_ar)
    pred_e, _, _ = rollout_eval(m, xx, yy, None, evaluator=ev, metrics=met)
    pred_ge, _, _ = g(xx, yy, None, evaluator=ev, metrics=met)
    torch.cuda.synchronize()
    assert torch.equal(pred_e, pred) and torch.equal(pred_ge, pred)
    assert ev.read()["samples"] == 2 * B and m.training is training
    _same(_buffers(m), b0)
