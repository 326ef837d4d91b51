"""GPU tests of the 3-D fine-tuning step: train.rollout_total / train_step / GraphedTrainStep / StepMetrics and
infer.rollout_eval with DPOTNet3D against the reference's own loop (finetune3d.py:206-230, recorded in g18_finetune3d by
scripts/make_golden_finetune3d.py), the 3-D noise rule on every path of the noise kernels, the one-graph step against the eager
step, and what PatchEmbed3DFn keeps for its backward.  Default fp32 precision, B = 2, guarded allocator where the test owns
the buffers' lifetime (not around a graph capture)."""
import math

import pytest
import torch

import afno3d_ref as A3
import finetune3d_ref as F3
import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close, assert_sub, load

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def build(tag):
    from dpot_amd import DPOTNet3D, load_3d_components_from_2d
    m = DPOTNet3D(**F3.CASES[tag]["cfg"])
    sd3, sd2 = F3.recipe_weights(tag, m)
    m.load_state_dict(sd3)
    load_3d_components_from_2d(m, sd2, ["blocks", "time_agg"])
    return m.cuda()


def _rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double()
    return (a.reshape(-1) - b.reshape(-1)).abs().max().item() / (b.abs().max().item() + 1e-300)


# ---- reference parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(F3.CASES))
def test_step_vs_reference_loop(tag, guarded):
    from dpot_amd import ops, train
    fx = load("g18_finetune3d")
    c = F3.CASES[tag]
    m = build(tag)
    xx, yy, msk, eps = F3.inputs(tag)
    xx, yy, msk = guard.wrap(xx, "cuda"), guard.wrap(yy, "cuda"), guard.wrap(msk, "cuda")
    eps = [guard.wrap(e, "cuda") for e in eps]
    n_steps = len(eps)
    opt = train.FusedAdam(train.FlatParams(m), lr=F3.OPT["lr"], betas=F3.OPT["betas"], weight_decay=F3.OPT["weight_decay"],
                          max_norm=F3.OPT["max_norm"])
    metrics = train.StepMetrics("cuda", n_steps)
    cls_before = [p.detach().clone() for p in m.cls_head.parameters()]

    assert_sub(ops.noise_inject(xx, eps[0], F3.NOISE_SCALE), fx, f"{tag}.noisy.0", f"{tag}.noisy.0", rtol=RTOL)

    opt.zero_grad()
    loss, pred, total = train.rollout_total(m, xx, yy, msk, c["T_bundle"], F3.NOISE_SCALE, noise=eps, metrics=metrics)
    assert total is loss and tuple(pred.shape) == tuple(yy.shape)
    total.backward()
    grads = {n: g.clone() for n, g in zip(opt.fp.names, opt.fp.grad_views)}
    opt.step()
    metrics.accumulate(opt)
    torch.cuda.synchronize()
    got = metrics.read()
    assert got["ar_steps"] == n_steps and got["samples"] == F3.B and got["cls_total"] == 0
    for name, val in (("loss", loss.item()), ("l2_step", got["l2_step"]), ("l2_full", got["l2_full"]),
                      ("grad_norm", got["grad_norm"]), ("grad_norm (opt)", opt.grad_norm().item())):
        key = {"l2_step": "loss", "grad_norm (opt)": "grad_norm"}.get(name, name)
        want = float(fx[f"{tag}.{key}"])
        print(f"{tag}.{name}: {val:.8f} reference {want:.8f} rel {abs(val - want) / want:.2e} "
              f"(reference fp32 vs its float64 {float(fx[f'{tag}.err32.{key}']):.2e})")
    for name, val in (("loss", loss.item()), ("loss", got["l2_step"]), ("l2_full", got["l2_full"]),
                      ("grad_norm", got["grad_norm"]), ("grad_norm", opt.grad_norm().item())):
        want = float(fx[f"{tag}.{name}"])
        assert abs(val - want) <= RTOL * want, (name, val, want)
    names = [str(n) for n in fx[f"{tag}.names"]]
    assert sorted(names) == sorted(n for n in grads if not n.startswith("cls_head."))
    for n in names:
        key = f"{tag}.g.{n}"
        if key + ".sub" in fx.files:
            print(f"{key}: kernels {_rel(grads[n].reshape(-1)[::int(fx[key + '.stride'])], fx[key + '.sub']):.2e}  "
                  f"reference-fp32 {float(fx[f'{tag}.err32.g.{n}']):.2e}")
            assert_sub(grads[n], fx, key, key)
        else:
            print(f"{key}: kernels {_rel(grads[n], fx[key]):.2e}  reference-fp32 {float(fx[f'{tag}.err32.g.{n}']):.2e}")
            assert_close(grads[n], fx[key], key)
    sd = m.state_dict()
    for n in names:
        stride = int(fx[f"{tag}.p.{n}.stride"])
        after = sd[n].detach().cpu().reshape(-1)[::stride]
        assert (after - torch.from_numpy(fx[f"{tag}.p.{n}.sub"])).abs().max().item() <= 0.05 * F3.OPT["lr"], n
    for n in grads:
        if n.startswith("cls_head."):
            assert not grads[n].any(), n
    for p, q in zip(m.cls_head.parameters(), cls_before):
        assert torch.equal(p.detach(), q)


def test_noisy_input_of_the_second_ar_step_vs_reference(guarded):
    """the window after one slide, with its noise: prediction, slide and the per-(b, t, c) norm of a window whose last frame is
    the model's output"""
    from dpot_amd import ops
    fx = load("g18_finetune3d")
    for tag in F3.CASES:
        c = F3.CASES[tag]
        m = build(tag)
        xx, _, _, eps = F3.inputs(tag)
        with torch.no_grad():
            x0 = ops.noise_inject(guard.wrap(xx, "cuda"), guard.wrap(eps[0], "cuda"), F3.NOISE_SCALE)
            x1 = ops.noise_inject(ops.window_slide(x0, m(x0).contiguous()), guard.wrap(eps[1], "cuda"), F3.NOISE_SCALE)
        torch.cuda.synchronize()
        assert x1.shape[-2] == c["cfg"]["in_timesteps"]
        assert_sub(x1, fx, f"{tag}.noisy.1", f"{tag}.noisy.1", rtol=RTOL)


# ---- the noise rule --------------------------------------------------------------------------------------------------------
def _noise_case(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=gen) for _ in range(3)]


def test_noise_6d_explicit_eps_vs_float64(guarded):
    from dpot_amd import ops
    xx, eps, _ = _noise_case((2, 4, 4, 4, 3, 2), 51)
    got, norms = ops.noise_inject(guard.wrap(xx, "cuda"), guard.wrap(eps, "cuda"), 0.05, return_norms=True)
    torch.cuda.synchronize()
    assert_close(got, F3.noise3d(xx.double(), 0.05, eps.double()), "noise_inject 6-D")
    assert_close(norms[:2 * 3 * 2].view(2, 3, 2), (xx.double() ** 2).sum(dim=(1, 2, 3)).sqrt(), "norms per (b, t, c)")
    # and the 5-D rule is untouched: the same numbers as a [B, X, Y*Z, T, C] window reduce over the time axis as well
    got5 = ops.noise_inject(guard.wrap(xx.view(2, 4, 16, 3, 2), "cuda"), guard.wrap(eps.view(2, 4, 16, 3, 2), "cuda"), 0.05)
    torch.cuda.synchronize()
    assert_close(got5.view(xx.shape), F3.noise2d_rule(xx.double(), 0.05, eps.double()), "noise_inject 5-D")


def test_noise_6d_backward_vs_float64_autograd(guarded):
    from dpot_amd import train
    xx, eps, g = _noise_case((2, 4, 4, 4, 3, 2), 52)
    x = guard.wrap(xx, "cuda").requires_grad_(True)
    out = train._NoiseFn.apply(x, guard.wrap(eps, "cuda"), 0.05)
    out.backward(guard.wrap(g, "cuda"))
    torch.cuda.synchronize()
    x64 = xx.double().requires_grad_(True)
    F3.noise3d(x64, 0.05, eps.double()).backward(g.double())
    assert_close(out, F3.noise3d(xx.double(), 0.05, eps.double()), "_NoiseFn 6-D forward")
    assert_close(x.grad, x64.grad, "_NoiseFn 6-D backward")


def test_noise_6d_generator_statistics_and_redraw(guarded):
    """the in-kernel generator under the 3-D rule: (out - xx) / (scale * ||xx||_(b,t,c)) is N(0, 1) - under the 2-D reduction
    its variance would be T = 4 - and the backward re-draws the very same noise"""
    from dpot_amd import ops, train
    shape, scale = (2, 16, 16, 16, 4, 4), 0.01
    xx, _, g = _noise_case(shape, 53)
    norm = (xx.double() ** 2).sum(dim=(1, 2, 3), keepdim=True).sqrt()
    x = guard.wrap(xx, "cuda")
    out = ops.noise_inject(x, None, scale)                                  # the first-step shortcut of the rollout
    torch.cuda.synchronize()
    z = (out.double().cpu() - xx.double()) / (scale * norm)
    n = z.numel()
    mean, var = z.mean().item(), z.var().item()
    print(f"generator under the 3-D rule: n = {n}, mean {mean:.4e} (5 se = {5 / math.sqrt(n):.4e}), "
          f"var - 1 = {var - 1:.4e} (5 se = {5 * math.sqrt(2 / n):.4e})")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1.0) <= 5 * math.sqrt(2.0 / n)

    xr = guard.wrap(xx, "cuda").requires_grad_(True)
    out2 = train._NoiseFn.apply(xr, None, scale)
    out2.backward(guard.wrap(g, "cuda"))
    torch.cuda.synchronize()
    eps_rec = ((out2.detach().double().cpu() - xx.double()) / (scale * norm)).float()
    _, norms = ops.noise_inject(x, guard.wrap(eps_rec, "cuda"), scale, return_norms=True)
    want = ops.noise_inject_bwd(x, guard.wrap(eps_rec, "cuda"), None, guard.wrap(g, "cuda"), norms, scale)
    torch.cuda.synchronize()
    assert not torch.equal(out2.detach(), out)                              # a second draw, not a replay of the first
    assert_close(xr.grad, want, "backward re-draw", rtol=1e-5, atol_scale=1e-5)


# ---- graph against eager ---------------------------------------------------------------------------------------------------
def _batch(tag, T_ar):
    xx, yy, msk, _ = F3.inputs(tag)
    return xx.cuda(), yy[..., :T_ar, :].contiguous().cuda(), msk.cuda()


def test_graphed_step_bit_identical_to_eager():
    from dpot_amd.train import FlatParams, FusedAdam, GraphedTrainStep, StepMetrics, train_step
    m = build("ft")
    xx, yy, msk = _batch("ft", 2)
    opt = FusedAdam(FlatParams(m), lr=1e-3, weight_decay=1e-6, max_norm=1.0)
    metrics = StepMetrics("cuda", 2)
    cls_before = [p.detach().clone() for p in m.cls_head.parameters()]
    lrs = (1e-3, 3e-3, 2e-3)
    g = GraphedTrainStep(m, opt, xx, yy, msk, T_bundle=1, warmup=1, metrics=metrics)
    snap = opt.snapshot()
    graph_losses = [g.replay(lr).item() for lr in lrs]
    torch.cuda.synchronize()
    graph = [t.clone() for t in opt._state_tensors()]
    graph_metrics = metrics.read()
    opt.restore(snap)
    metrics.reset()
    eager_losses = [train_step(m, opt, xx, yy, msk, lr=lr, metrics=metrics)[0].item() for lr in lrs]
    torch.cuda.synchronize()
    assert graph_losses == eager_losses
    for a, b in zip(graph, opt._state_tensors()):
        assert torch.equal(a, b)
    assert int(opt.step_dev.item()) == len(lrs)
    eager_metrics = metrics.read()
    assert graph_metrics["opt_steps"] == 3 and graph_metrics["ar_steps"] == 6
    for k in ("l2_step", "l2_full", "grad_norm"):
        assert graph_metrics[k] == eager_metrics[k], k
    for p, q in zip(m.cls_head.parameters(), cls_before):
        assert torch.equal(p.detach(), q)


@pytest.mark.parametrize("optimiser", ["adam", "lamb"])
def test_graphed_step_with_noise_trains(optimiser):
    from dpot_amd.train import FlatParams, FusedAdam, FusedLamb, GraphedTrainStep
    m = build("ft")
    xx, yy, msk = _batch("ft", 2)
    cls = FusedAdam if optimiser == "adam" else FusedLamb
    opt = cls(FlatParams(m), lr=1e-3, max_norm=5.0)
    g = GraphedTrainStep(m, opt, xx, yy, msk, T_bundle=1, noise_scale=0.01, warmup=1)
    losses = [g.replay(1e-3).item() for _ in range(6)]
    torch.cuda.synchronize()
    print(f"{optimiser}: losses of six replays {['%.5f' % l for l in losses]}")
    assert all(math.isfinite(l) for l in losses)
    assert losses[-1] < losses[0]
    assert torch.isfinite(opt.fp.flat).all()


# ---- memory ----------------------------------------------------------------------------------------------------------------
def test_patch_embed_keeps_the_window_not_the_patch_matrix(guarded):
    from dpot_amd import ops
    from dpot_amd.functional import PatchEmbed3DFn
    m = build("ft")
    cfg = F3.CASES["ft"]["cfg"]
    S, P, T, C, E = cfg["img_size"], cfg["patch_size"], cfg["in_timesteps"], cfg["in_channels"], cfg["embed_dim"]
    h = S // P
    tok, K = h ** 3, (C + 4) * P ** 3
    x = guard.wrap(F3.inputs("ft")[0], "cuda").requires_grad_(True)
    pe = m.patch_embed.proj
    hid = pe[0].weight.shape[0]
    z = PatchEmbed3DFn.apply(x, m._gs, m._gt, pe[0].weight.view(hid, K), pe[0].bias, pe[2].weight.view(E, hid), pe[2].bias,
                             m.pos_embed.view(E, tok).t(), P, ops.ACT_IDS["gelu"])
    saved = [t for t in z.grad_fn.saved_tensors if torch.is_tensor(t)]
    assert any(t.data_ptr() == x.data_ptr() for t in saved)                 # the window itself
    for t in saved:
        assert tuple(t.shape) != (F3.B * T * tok, K) and t.numel() != F3.B * T * tok * K, tuple(t.shape)
    # ... and the backward still delivers everything, dx through unpatchify3
    z.backward(torch.ones_like(z))
    torch.cuda.synchronize()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    assert pe[0].weight.grad is not None and m.pos_embed.grad is not None


# ---- evaluation ------------------------------------------------------------------------------------------------------------
def test_rollout_eval_equals_the_hand_loop(guarded):
    from dpot_amd import infer
    from dpot_amd.functional import rel_l2_loss
    from dpot_amd.train import StepMetrics
    tag = "ftb"
    c = F3.CASES[tag]
    m = build(tag).eval()
    xx, yy, msk, _ = F3.inputs(tag)
    xx, yy, msk = guard.wrap(xx, "cuda"), guard.wrap(yy, "cuda"), guard.wrap(msk, "cuda")
    Tb = c["T_bundle"]
    with torch.no_grad():
        pred, l_step, l_full = infer.rollout_eval(m, xx, yy, msk, T_bundle=Tb)
        metrics = StepMetrics("cuda", 2)
        pred_m, _, l_full_m = infer.rollout_eval(m, xx, yy, msk, T_bundle=Tb, metrics=metrics)
        w, loss, preds = xx, 0., []
        for t in range(0, c["T_ar"], Tb):                                   # finetune3d.py:263-273
            im = m(w)
            loss = loss + rel_l2_loss(im, yy[..., t:t + Tb, :].contiguous(), msk)
            preds.append(im)
            w = torch.cat((w[..., Tb:, :], im), dim=-2)
        hand = torch.cat(preds, dim=-2)
        full = rel_l2_loss(hand, yy, msk)
    torch.cuda.synchronize()
    assert torch.equal(pred, hand) and torch.equal(pred_m, hand)
    assert l_step.item() == loss.item() and l_full.item() == full.item()
    assert abs(l_full_m.item() - full.item()) <= RTOL * full.item()
    got = metrics.read()
    assert got["samples"] == F3.B and abs(got["l2_full"] - full.item()) <= RTOL * full.item()
    with pytest.raises(ValueError):
        infer.rollout_eval(m, xx, yy, msk, T_bundle=Tb, model_res=8)
