"""GPU tests of the step machinery added in round 2: device-side Adam step counter (no host staging buffer), optimiser
checkpoint format, the HIP noise-injection backward and window slide, the segmented (bucket-overlapped) data-parallel
graph step, and the data-parallel path driven by the HIP backward in two processes sharing the one GPU."""
import os
import socket
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import RTOL, assert_close, load, set_tune
from oracle import dpot_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(kw, salt):
    from dpot_amd import DPOTNet
    cfg = R.DPOTConfig(**kw)
    m = DPOTNet(**kw)
    m.load_state_dict(R.recipe_state_dict(cfg, salt=salt))
    return m.cuda(), cfg


def _batch(cfg, B, T_ar=1, salt=1):
    S = cfg.img_size
    xx = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=salt).cuda()
    yy = R.recipe_input((B, S, S, T_ar, cfg.out_channels), salt=salt + 1).cuda()
    msk = torch.ones(B, S, S, 1, cfg.out_channels, device="cuda")
    return xx, yy, msk


def _opt(m, **kw):
    from dpot_amd.train import FlatParams, FusedAdam
    args = dict(lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
    args.update(kw)
    return FusedAdam(FlatParams(m), **args)


# ------------------------------------------------------------------------------------------------------
def test_replays_without_host_sync_match_synced_run():
    """lr / bias corrections of step k must not be overwritten by the host staging step k+n.
    Replaying N steps back to back WITHOUT any synchronisation must give exactly the parameters of a run that
    synchronises after every step (different lr every step, fast-changing bias corrections in the first steps)."""
    from dpot_amd.train import GraphedTrainStep
    lrs = [1e-3 * (1 + 3 * (i % 5)) for i in range(24)]
    outs = []
    for sync in (True, False):
        m, cfg = build(R.MINI, salt=5)
        xx, yy, msk = _batch(cfg, 2)
        opt = _opt(m)
        g = GraphedTrainStep(m, opt, xx, yy, msk, warmup=1)
        for lr in lrs:
            g.replay(lr)
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        assert int(opt.step_dev.item()) == len(lrs) == opt.step_count
        outs.append(opt.fp.flat.clone())
    assert torch.equal(outs[0], outs[1])


def test_graph_warmup_does_not_train():
    """the eager warm-up iterations of GraphedTrainStep leave parameters, moments and the step
    counter untouched"""
    from dpot_amd.train import GraphedTrainStep
    m, cfg = build(R.MINI, salt=5)
    xx, yy, msk = _batch(cfg, 2)
    opt = _opt(m)
    before = opt.fp.flat.clone()
    GraphedTrainStep(m, opt, xx, yy, msk, warmup=3)
    assert torch.equal(opt.fp.flat, before) and int(opt.step_dev.item()) == 0 and opt.step_count == 0
    assert float(opt.exp_avg.abs().max()) == 0.0


def test_optimizer_state_dict_roundtrip_and_reference_layout():
    """FusedAdam.state_dict has the layout of the reference's torch-style Adam (utils/optimizer.py:101-164) and
    resuming from it continues the run bit for bit"""
    from dpot_amd.train import train_step
    m, cfg = build(R.MINI, salt=8)
    xx, yy, msk = _batch(cfg, 2)
    opt = _opt(m)
    for _ in range(3):
        train_step(m, opt, xx, yy, msk, lr=2e-3)
    sd_opt = opt.state_dict(m)
    sd_model = OrderedDict((k, v.clone()) for k, v in m.state_dict().items())
    names = [n for n, _ in m.named_parameters()]
    assert sd_opt["param_groups"][0]["params"] == list(range(len(names)))
    for i, n in enumerate(names):
        if n.startswith("cls_head."):
            assert i not in sd_opt["state"]                  # never updated in single-GPU training
        else:
            st = sd_opt["state"][i]
            assert st["step"] == 3 and st["exp_avg"].shape == dict(m.named_parameters())[n].shape
    train_step(m, opt, xx, yy, msk, lr=2e-3)
    want = opt.fp.flat.clone()
    m2, _ = build(R.MINI, salt=8)
    m2.load_state_dict(sd_model)
    opt2 = _opt(m2)
    opt2.load_state_dict(sd_opt, m2)
    train_step(m2, opt2, xx, yy, msk, lr=2e-3)
    assert torch.equal(opt2.fp.flat, want)


def test_grad_norm_without_clipping():
    from dpot_amd.train import train_step
    m, cfg = build(R.MINI, salt=8)
    xx, yy, msk = _batch(cfg, 2)
    opt = _opt(m, max_norm=None)
    train_step(m, opt, xx, yy, msk)
    n = opt.fp.n_head
    assert abs(opt.grad_norm().item() - opt.fp.grad[:n].double().norm().item()) <= 1e-5 * opt.grad_norm().item()


# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 8, 8, 4, 3), (3, 16, 16, 10, 4)])
def test_noise_backward_and_window_slide_vs_autograd(shape, guarded):
    from dpot_amd import ops
    from dpot_amd.train import _NoiseFn, _SlideFn
    g = torch.Generator().manual_seed(3)
    xx = guard.wrap(torch.randn(*shape, generator=g), "cuda")
    eps = guard.wrap(torch.randn(*shape, generator=g), "cuda")
    up = guard.wrap(torch.randn(*shape, generator=g), "cuda")
    s = 0.3
    # explicit eps: against torch autograd of the reference expression (train_temporal.py:205)
    a = guard.wrap(xx).requires_grad_(True)
    (_NoiseFn.apply(a, eps, s) * up).sum().backward()
    b = xx.clone().requires_grad_(True)
    ref = b + s * torch.sum(b ** 2, dim=(1, 2, 3), keepdim=True) ** 0.5 * eps
    (ref * up).sum().backward()
    assert_close(a.grad, b.grad, "noise bwd (eps given)")
    # in-kernel generator: the backward re-draws the forward's noise from the saved generator state
    if xx.numel() % 4 == 0:
        c = guard.wrap(xx).requires_grad_(True)
        out = _NoiseFn.apply(c, None, s)
        (out * up).sum().backward()
        n = torch.sum(xx ** 2, dim=(1, 2, 3), keepdim=True) ** 0.5
        eps_used = (out.detach() - xx) / (s * n)
        want = up + s * xx / n * torch.sum(up * eps_used, dim=(1, 2, 3), keepdim=True)
        assert_close(c.grad, want, "noise bwd (in-kernel generator)", rtol=1e-3, atol_scale=1e-3)
    # window slide
    Tb = 2 if shape[3] > 2 else 1
    im = guard.wrap(torch.randn(*shape[:3], Tb, shape[4], generator=g), "cuda")
    a, ai = guard.wrap(xx).requires_grad_(True), guard.wrap(im).requires_grad_(True)
    o = _SlideFn.apply(a, ai)
    (o * up).sum().backward()
    b, bi = xx.clone().requires_grad_(True), im.clone().requires_grad_(True)
    o_ref = torch.cat((b[..., Tb:, :], bi), dim=-2)
    (o_ref * up).sum().backward()
    assert torch.equal(o, o_ref) and torch.equal(a.grad, b.grad) and torch.equal(ai.grad, bi.grad)


def test_rollout_with_noise_gradient_vs_oracle():
    """T_ar=3 rollout with explicit noise tensors: loss and every gradient vs the oracle (which differentiates through
    the noise norm exactly as the reference's autograd does)"""
    from dpot_amd.train import rollout
    m, cfg = build(R.MINI, salt=12)
    xx, yy, msk = _batch(cfg, 2, T_ar=3)
    g = torch.Generator().manual_seed(5)
    noise = [torch.randn(*xx.shape, generator=g) for _ in range(3)]
    sd = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in R.recipe_state_dict(cfg, salt=12).items())
    l_ref, _ = R.rollout_loss(sd, xx.cpu(), yy.cpu(), msk.cpu(), cfg, noise_scale=0.05, noise=noise)
    l_ref.backward()
    loss, _ = rollout(m, xx, yy, msk, noise_scale=0.05, noise=[n.cuda() for n in noise])
    loss.backward()
    assert abs(loss.item() - l_ref.item()) <= RTOL * abs(l_ref.item())
    for k, p in m.named_parameters():
        if sd[k].grad is not None:
            assert_close(p.grad, sd[k].grad, "noise rollout d" + k)


# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_ar", [1, 3])
def test_segmented_graph_step_equals_eager_step(T_ar):
    """the bucket-segmented hipGraph chain (train.SegmentedTrainStep) reproduces the eager step bit for bit (world 1:
    the collectives are no-ops, the graph cuts / leaf hand-over / shared pool are what is tested); T_ar = 3: the cuts sit
    in the FIRST auto-regressive step's backward only (train_temporal_parallel.py:214-244 under DDP)"""
    from dpot_amd.dp import BucketedGradReducer
    from dpot_amd.train import SegmentedTrainStep, train_step
    kw = dict(R.MINI, depth=4)
    m1, cfg = build(kw, salt=3)
    xx, yy, msk = _batch(cfg, 2, T_ar=T_ar)
    opt1 = _opt(m1, update_tail=True)
    for lr in (1e-3, 2e-3, 5e-4):
        l_e, _ = train_step(m1, opt1, xx, yy, msk, lr=lr)
    m2, _ = build(kw, salt=3)
    opt2 = _opt(m2, update_tail=True)
    red = BucketedGradReducer(opt2.fp, n_buckets=8, overlap=True)
    assert red.n_buckets >= 3
    seg = SegmentedTrainStep(m2, opt2, red, xx, yy, msk, warmup=1)
    assert len(seg.graphs) == red.n_buckets - 1 and len(seg.graphs) >= 2       # really cut into several graphs
    for lr in (1e-3, 2e-3, 5e-4):
        l_s = seg.replay(lr)
    assert l_s.item() == l_e.item()
    assert torch.equal(opt1.fp.flat, opt2.fp.flat)


def test_segmented_graph_step_equals_eager_step_bf16_small(monkeypatch):
    """the same at DPOT-Small with the bf16 channel MLP (batch 4): the graph cuts sit between Blocks whose backwards hand the
    gradient on TOGETHER with its bf16 packs (functional._GRAD_PACKS, round 5) and run the one-launch AFNO layer forward with
    its pack outputs; the Block behind a cut does not hand packs on (its gradient goes to a leaf): the chain must reproduce the
    eager step - same loss, parameters to fp32 rounding"""
    from dpot_amd.dp import BucketedGradReducer
    from dpot_amd.train import SegmentedTrainStep, train_step
    set_tune(monkeypatch, afno_layer=1)                      # (batch 4 is below the `auto` threshold of the one-launch layer)
    m1, cfg = build(R.SMALL, salt=3)
    m1.mlp_precision = "bf16"
    xx, yy, msk = _batch(cfg, 4, T_ar=1)
    opt1 = _opt(m1, update_tail=True)
    eager = []
    for lr in (1e-3, 2e-3):
        l_e, _ = train_step(m1, opt1, xx, yy, msk, lr=lr)
        eager.append(l_e.item())
    m2, _ = build(R.SMALL, salt=3)
    m2.mlp_precision = "bf16"
    opt2 = _opt(m2, update_tail=True)
    red = BucketedGradReducer(opt2.fp, n_buckets=4, overlap=True)
    seg = SegmentedTrainStep(m2, opt2, red, xx, yy, msk, warmup=1)
    assert len(seg.graphs) >= 2
    losses = [seg.replay(lr).item() for lr in (1e-3, 2e-3)]
    # the SECOND step's loss is a function of the first step's parameters, which differ in the last bit of six bias gradients
    # (below): equal to fp32 rounding, not bit for bit (2e-7 relative observed)
    assert losses[0] == eager[0]                                       # same parameters, same forward: same bits
    assert abs(losses[1] - eager[1]) <= 1e-6 * abs(eager[1]), (losses, eager)
    # (not bit for bit here: the Block behind a cut packs its incoming gradient itself, and that pass forms the fc2 bias
    # column sums per 64 tokens where the GroupNorm backward of the un-cut chain forms them per sample - fp32 rounding of
    # six bias gradients; everything else is the same arithmetic)
    d = (opt1.fp.flat - opt2.fp.flat).double().norm() / opt1.fp.flat.double().norm()
    assert d.item() <= 1e-5, d.item()      # (Adam turns a last-bit difference of a near-zero gradient into +-lr on that element)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, out_dir, segmented, T_ar=1):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)                                 # both ranks share the one GPU of the test box
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dpot_amd import DPOTNet
    from dpot_amd.dp import BucketedGradReducer
    from dpot_amd.train import FlatParams, FusedAdam, SegmentedTrainStep, rollout
    cfg = R.DPOTConfig(**R.MINI)
    sd = R.recipe_state_dict(cfg, salt=17)
    model = DPOTNet(**R.MINI)
    if rank == 0:
        model.load_state_dict(sd)
    model.cuda()
    fp = FlatParams(model)
    red = BucketedGradReducer(fp, n_buckets=3, overlap=True)
    red.broadcast_parameters(0)
    B = 4
    xx = R.recipe_input((B, cfg.img_size, cfg.img_size, cfg.in_timesteps, cfg.in_channels), salt=81)
    yy = R.recipe_input((B, cfg.img_size, cfg.img_size, T_ar, cfg.out_channels), salt=82)
    msk = torch.ones(B, cfg.img_size, cfg.img_size, 1, cfg.out_channels)
    sl = slice(2 * rank, 2 * rank + 2)
    xs, ys, ms = xx[sl].cuda(), yy[sl].cuda(), msk[sl].cuda()
    if segmented:
        opt = FusedAdam(fp, lr=0.0, betas=(0.9, 0.9), weight_decay=0.0, max_norm=1e4, update_tail=True)
        seg = SegmentedTrainStep(model, opt, red, xs, ys, ms, warmup=1)
        seg.replay(0.0)                                      # lr 0: weights stay, the flat gradient is what we check
        launched = len(seg.graphs)
    else:
        fp.zero_grad()
        red.begin_step()
        loss, _ = rollout(model, xs, ys, ms)
        loss.backward()                                      # HIP backward -> _Sink -> FlatParams.fire -> reducer
        launched = sum(red._launched)
        red.finish()
    torch.cuda.synchronize()
    g = (fp.grad * red.grad_scale).cpu()
    if rank == 0:
        np.savez(os.path.join(out_dir, f"dp_{int(segmented)}.npz"), flat=g.numpy(),
                 gnorm=np.float64(torch.sqrt((g.double() ** 2).sum()).item()), names=np.array(fp.names),
                 norms=np.array([g[o:o + p.numel()].norm().item() for p, o in zip(fp.params, fp.offsets)]),
                 launched=launched, n_buckets=red.n_buckets)
    ref = g.clone()
    dist.broadcast(ref, src=0)
    assert torch.equal(ref, g)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("segmented", [False, True])
def test_two_process_dp_hip_backward_vs_golden(tmp_path, segmented):
    """two processes on the one GPU, gloo collectives: the HIP backward's gradient-ready notifications drive the
    bucketed reducer (eager), resp. the segmented graph chain launches the buckets between replays; the averaged
    gradients match the golden numbers generated from the reference under DDP semantics (g8)"""
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path), segmented), nprocs=2, join=True)
    got = np.load(os.path.join(str(tmp_path), f"dp_{int(segmented)}.npz"))
    fx = load("g8_dp")
    assert abs(float(got["gnorm"]) - float(fx["grad_norm"])) <= RTOL * float(fx["grad_norm"])
    want = dict(zip([str(n) for n in fx["names"]], fx["grad_norms"]))
    for n, v in zip(got["names"], got["norms"]):
        assert abs(v - want[str(n)]) <= RTOL * want[str(n)] + 1e-7, n
    if not segmented:
        assert int(got["launched"]) >= int(got["n_buckets"]) - 1     # buckets went out DURING the backward


@pytest.mark.timeout(600)
def test_two_process_dp_segmented_rollout_vs_oracle(tmp_path):
    """T_ar = 3 under data parallelism (train_temporal_parallel.py:214-244): two processes on the one GPU, gloo
    collectives; the segmented graph chain (cuts in the first AR step's backward) and the eager hook-driven path must give
    the SAME averaged flat gradient bit for bit, and that gradient must match the oracle's rollout gradient of the full
    batch divided by the world size (sum-loss + DDP mean)"""
    import torch.multiprocessing as mp
    T_ar = 3
    res = {}
    for segmented in (False, True):
        mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path), segmented, T_ar), nprocs=2, join=True)
        res[segmented] = np.load(os.path.join(str(tmp_path), f"dp_{int(segmented)}.npz"))
    assert np.array_equal(res[True]["flat"], res[False]["flat"])
    assert int(res[True]["launched"]) >= 2                       # the chain really is several graphs
    cfg = R.DPOTConfig(**R.MINI)
    sd = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in R.recipe_state_dict(cfg, salt=17).items())
    B = 4
    xx = R.recipe_input((B, cfg.img_size, cfg.img_size, cfg.in_timesteps, cfg.in_channels), salt=81)
    yy = R.recipe_input((B, cfg.img_size, cfg.img_size, T_ar, cfg.out_channels), salt=82)
    msk = torch.ones(B, cfg.img_size, cfg.img_size, 1, cfg.out_channels)
    loss, _ = R.rollout_loss(sd, xx, yy, msk, cfg)
    loss.backward()
    got = dict(zip([str(n) for n in res[True]["names"]], res[True]["norms"]))
    for k, v in sd.items():
        if v.grad is None:
            continue
        want = v.grad.double().norm().item() / 2
        assert abs(got[k] - want) <= RTOL * want + 1e-7, k


def _rccl_worker(rank, port, out_dir):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    from dpot_amd import DPOTNet
    from dpot_amd.dp import BucketedGradReducer
    from dpot_amd.train import FlatParams, FusedAdam, GraphedTrainStep, SegmentedTrainStep, rollout
    cfg = R.DPOTConfig(**R.MINI)
    sd = R.recipe_state_dict(cfg, salt=17)
    B, T_ar = 4, 2
    xs = R.recipe_input((B, cfg.img_size, cfg.img_size, cfg.in_timesteps, cfg.in_channels), salt=81).cuda()
    ys = R.recipe_input((B, cfg.img_size, cfg.img_size, T_ar, cfg.out_channels), salt=82).cuda()
    ms = torch.ones(B, cfg.img_size, cfg.img_size, 1, cfg.out_channels).cuda()
    out = {}
    for kind in ("plain", "eager", "segmented", "onegraph"):
        model = DPOTNet(**R.MINI)
        model.load_state_dict(sd)
        model.cuda()
        fp = FlatParams(model)
        if kind == "plain":                                  # no reducer at all: the single-GPU gradient
            fp.zero_grad()
            loss, _ = rollout(model, xs, ys, ms)
            loss.backward()
            launched = 0
        else:
            red = BucketedGradReducer(fp, n_buckets=3, overlap=True)
            red.single_rank_collective = True                # real dist.all_reduce calls (nccl backend) on the side stream
            red.broadcast_parameters(0)
            if kind == "segmented":
                opt = FusedAdam(fp, lr=0.0, betas=(0.9, 0.9), weight_decay=0.0, max_norm=1e4, update_tail=True)
                seg = SegmentedTrainStep(model, opt, red, xs, ys, ms, warmup=1)
                for _ in range(3):                           # replays queue behind each other without host syncs
                    seg.replay(0.0)
                launched = len(seg.graphs)
            elif kind == "onegraph":                         # opt-in: the collectives captured INSIDE the one graph
                opt = FusedAdam(fp, lr=0.0, betas=(0.9, 0.9), weight_decay=0.0, max_norm=1e4, update_tail=True)
                try:
                    g1 = GraphedTrainStep(model, opt, xs, ys, ms, warmup=1, reducer=red, capture_collectives=True)
                    for _ in range(3):
                        g1.replay(0.0)
                    launched = sum(red._launched)
                except Exception as e:                       # RCCL build without graph capture: recorded, not a failure
                    launched = -1
                    out["onegraph_error"] = np.array(f"{type(e).__name__}: {e}"[:300])
            else:
                fp.zero_grad()
                red.begin_step()
                loss, _ = rollout(model, xs, ys, ms)
                loss.backward()
                launched = sum(red._launched)
                red.finish()
        torch.cuda.synchronize()
        out[kind] = fp.grad.cpu().numpy().copy()
        out[kind + "_launched"] = launched
    out["backend"] = np.array(dist.get_backend())
    np.savez(os.path.join(out_dir, "rccl1.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_one_rank_rccl_collectives_leave_the_gradient_unchanged(tmp_path):
    """the N > 1 code path with the REAL RCCL library on the one GPU of the test box: a one-rank nccl process group, the
    bucket all-reduces issued through torch's nccl backend on the side stream (hook-driven during an eager backward, between
    the replays of the segmented hipGraph chain - three steps queued back to back - and, opt-in mode, captured inside ONE
    graph).  SUM over one rank is the identity (RCCL enqueues no device work for it), so the flat gradient must equal the
    plain single-GPU gradient BIT FOR BIT: communicator set-up, the host path and the stream hand-offs are what this covers
    - a collective's data path needs a second GPU"""
    import torch.multiprocessing as mp
    mp.spawn(_rccl_worker, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    got = np.load(os.path.join(str(tmp_path), "rccl1.npz"))
    assert str(got["backend"]) == "nccl"
    assert np.abs(got["plain"]).max() > 0
    assert np.array_equal(got["eager"], got["plain"])
    assert np.array_equal(got["segmented"], got["plain"])
    assert int(got["eager_launched"]) >= 2 and int(got["segmented_launched"]) >= 2
    if int(got["onegraph_launched"]) >= 0:                   # collectives captured inside the one graph (opt-in mode)
        assert int(got["onegraph_launched"]) >= 2
        assert np.array_equal(got["onegraph"], got["plain"])
    else:
        print("one-graph capture of the collectives not available here:", str(got["onegraph_error"]))


def _select_worker(rank, world, port, out_dir, backend):
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
    from dpot_amd import DPOTNet
    from dpot_amd.dp import BucketedGradReducer
    from dpot_amd.train import FlatParams, FusedAdam, GraphedTrainStep, SegmentedTrainStep, make_dp_step
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
    opt = FusedAdam(fp, lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=1e4, update_tail=True)
    before = (fp.flat.clone(), opt.exp_avg.clone(), int(opt.step_dev.item()))
    step, info = make_dp_step(model, opt, red, xs, ys, ms, noise_scale=5e-4, warmup=1)
    torch.cuda.synchronize()
    # the selection leaves parameters / optimiser state as found
    assert torch.equal(fp.flat, before[0]) and torch.equal(opt.exp_avg, before[1]) and int(opt.step_dev.item()) == before[2]
    losses = [float(step.replay(1e-3).item()) for _ in range(3)]
    torch.cuda.synchronize()
    ref = fp.flat.clone()
    dist.broadcast(ref, src=0)                               # (a device tensor: the nccl backend has no CPU path)
    assert torch.equal(ref, fp.flat)                         # replicas stay identical
    flat = fp.flat.cpu()
    if rank == 0:
        np.savez(os.path.join(out_dir, f"select_{backend}.npz"), mode=np.array(info["mode"]), why=np.array(info["why"]),
                 kind=np.array(type(step).__name__), losses=np.array(losses), flat=flat.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_dp_step_selection_one_rank_rccl_and_two_rank_gloo(tmp_path):
    """round 6: train.make_dp_step builds the segmented chain AND the one-graph step, runs one trial step in
    each from the same snapshot and keeps the one-graph step only if the reduced gradient is bit-identical between the modes
    and across the ranks.  (a) one-rank RCCL communicator (the real library on the one GPU): the collectives capture, the
    trial agrees -> one-graph SELECTED; (b) two ranks over gloo: a gloo collective cannot sit inside a stream capture (it
    synchronises the stream from the host) -> the selection FALLS BACK to the chain and says so; training continues either way and the
    replicas stay bit-identical."""
    import torch.multiprocessing as mp
    mp.spawn(_select_worker, args=(1, _free_port(), str(tmp_path), "nccl"), nprocs=1, join=True)
    a = np.load(os.path.join(str(tmp_path), "select_nccl.npz"))
    assert str(a["mode"]) == "one-graph" and str(a["kind"]) == "GraphedTrainStep", (str(a["mode"]), str(a["why"]))
    mp.spawn(_select_worker, args=(2, _free_port(), str(tmp_path), "gloo"), nprocs=2, join=True)
    b = np.load(os.path.join(str(tmp_path), "select_gloo.npz"))
    assert str(b["mode"]) == "segmented" and str(b["kind"]) == "SegmentedTrainStep"
    assert "capture failed" in str(b["why"]), str(b["why"])
    assert np.isfinite(a["losses"]).all() and np.isfinite(b["losses"]).all()


def test_backward_after_optimiser_step_raises():
    """the derived weight packs are persistent buffers; a backward that runs AFTER the optimiser changed the
    parameters would silently use overwritten packs - it must raise instead"""
    from dpot_amd.train import rollout
    m, cfg = build(R.MINI, salt=3)
    xx, yy, msk = _batch(cfg, 2)
    opt = _opt(m)
    opt.zero_grad()
    loss_a, _ = rollout(m, xx, yy, msk)
    opt.step(1e-3)                                            # parameters change between forward(A) and backward(A)
    with pytest.raises(RuntimeError, match="parameters were updated"):
        loss_a.backward()
    opt.zero_grad()                                           # a fresh forward / backward pair is fine again
    loss_b, _ = rollout(m, xx, yy, msk)
    loss_b.backward()
    assert torch.isfinite(opt.grad_norm()).item()


def test_backward_after_graph_replay_raises():
    """a hipGraph replay runs the captured Adam and rewrites the persistent weight packs just like the eager
    optimiser: an eager forward -> replay -> eager backward sequence must raise, not use overwritten packs"""
    from dpot_amd.train import GraphedTrainStep, rollout
    m, cfg = build(R.MINI, salt=3)
    xx, yy, msk = _batch(cfg, 2)
    opt = _opt(m)
    g = GraphedTrainStep(m, opt, xx, yy, msk, warmup=1)
    loss_a, _ = rollout(m, xx, yy, msk)                       # eager forward A
    g.replay(1e-3)                                            # parameters + packs change under it
    with pytest.raises(RuntimeError, match="parameters were updated"):
        loss_a.backward()
    loss_b, _ = rollout(m, xx, yy, msk)
    loss_b.backward()
    assert torch.isfinite(opt.grad_norm()).item()


def test_window_slide_rejects_mismatched_prediction(guarded):
    from dpot_amd import _lib, ops
    xx = guard.wrap(torch.zeros(2, 8, 8, 4, 3, device="cuda"))
    with pytest.raises(_lib.DpotHipError):
        ops.window_slide(xx, torch.zeros(2, 8, 8, 1, 4, device="cuda"))      # out_channels != in_channels
    with pytest.raises(_lib.DpotHipError):
        ops.window_slide(xx, torch.zeros(2, 8, 4, 1, 3, device="cuda"))      # other spatial extent


def test_adam_writes_the_weight_packs(monkeypatch):
    """round 6: with the plain-bf16 channel MLP the fused Adam launch ALSO writes the two bf16 packs of every
    channel-MLP weight (dpot_adam_step_packs: 64 x 256 tiles of the weight through LDS) and the next forward skips its pack
    launch.  (a) parameters, moments and losses are BIT-identical to the separate Adam + pack launches (DPOT_TUNE packs=0),
    eagerly and under hipGraph replay; (b) the packs Adam wrote equal a forced refresh from the parameters; (c) anything else
    that moves the parameters (load_state_dict, optimiser restore) makes the forward pack again."""
    from dpot_amd.train import GraphedTrainStep, train_step
    kw = dict(R.MINI, embed_dim=256, n_blocks=2, depth=2, mlp_ratio=2)
    runs = {}
    for packs in ("0", "1"):
        set_tune(monkeypatch, packs=packs)
        m, cfg = build(kw, salt=7)
        m.mlp_precision = "bf16"
        xx, yy, msk = _batch(cfg, 4)
        opt = _opt(m)
        losses = [train_step(m, opt, xx, yy, msk, lr=lr)[0].item() for lr in (1e-3, 2e-3, 5e-4)]
        pp = m.packs.get("bf16")
        plan = m.packs.adam_plan(opt.fp.flat, opt.n_active)
        if packs == "1":
            assert plan is not None and plan.ntiles == 2 * 2 * (512 // 64) * (256 // 256) and opt.wrote is pp
            assert m.packs.is_fresh(pp)
            mine = [b.clone() for b in pp.bufs]
            pp.refresh()
            assert all(torch.equal(a, b) for a, b in zip(mine, pp.bufs)), "packs written by Adam != packs of the parameters"
            # (c) load_state_dict bumps the tensor versions: the packs are no longer trusted
            m.load_state_dict(m.state_dict())
            assert not m.packs.is_fresh(pp)
            snap = opt.snapshot()
            opt.restore(snap)                      # re-packs eagerly and trusts them again (graph warm-up relies on it)
            assert m.packs.is_fresh(pp)
        else:
            assert plan is None and opt.wrote is None and not m.packs.is_fresh(pp)
        g = GraphedTrainStep(m, opt, xx, yy, msk, warmup=1)
        assert g.owned is (pp if packs == "1" else None)
        losses += [g.replay(lr).item() for lr in (1e-3, 3e-3, 1e-3)]
        if packs == "1":
            mine = [b.clone() for b in pp.bufs]
            pp.refresh()
            assert all(torch.equal(a, b) for a, b in zip(mine, pp.bufs)), "packs after graph replays"
        runs[packs] = (losses, opt.fp.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())
    assert runs["0"][0] == runs["1"][0], (runs["0"][0], runs["1"][0])
    for a, b in zip(runs["0"][1:], runs["1"][1:]):
        assert torch.equal(a, b)


_BF16_KW = dict(R.MINI, embed_dim=256, n_blocks=2, depth=2, mlp_ratio=2)     # (channel MLP on the bf16 packs Adam writes)


def _bf16_model(salt=7, mlp="bf16"):
    m, cfg = build(_BF16_KW, salt=salt)
    m.mlp_precision = mlp
    return m, cfg


@pytest.mark.parametrize("kind", ["graphed", "segmented"])
def test_replay_after_load_state_dict_equals_eager_step(kind):
    """a captured step whose Adam writes the bf16 packs holds no pack launch; after load_state_dict (the documented resume
    path) its next replay must run on packs of the NEW parameters - as the eager step from the same state does"""
    from dpot_amd.dp import BucketedGradReducer
    from dpot_amd.train import GraphedTrainStep, SegmentedTrainStep, train_step
    m, cfg = _bf16_model()
    xx, yy, msk = _batch(cfg, 4)
    opt = _opt(m)
    if kind == "graphed":
        step = GraphedTrainStep(m, opt, xx, yy, msk, warmup=1)
    else:
        step = SegmentedTrainStep(m, opt, BucketedGradReducer(opt.fp, n_buckets=4, overlap=True), xx, yy, msk, warmup=1)
    step.replay(1e-3)
    m.load_state_dict(R.recipe_state_dict(cfg, salt=11))
    snap = opt.snapshot()
    loss = step.replay(2e-3).item()
    m2, _ = _bf16_model()
    opt2 = _opt(m2)
    opt2.restore(snap)                                         # same parameters, moments and step counter
    assert loss == train_step(m2, opt2, xx, yy, msk, lr=2e-3)[0].item()
    if kind == "graphed":
        assert torch.equal(opt.fp.flat, opt2.fp.flat)
    else:                                                      # (tolerance of the segmented-vs-eager test above)
        d = (opt.fp.flat - opt2.fp.flat).double().norm() / opt2.fp.flat.double().norm()
        assert d.item() <= 1e-5, d.item()


def test_replay_marks_fresh_only_the_packs_its_adam_wrote():
    """captured with the f32 channel MLP, the graph's Adam writes no bf16 packs: a bf16 forward after a replay must re-pack,
    not trust packs the replay never wrote"""
    from dpot_amd.train import GraphedTrainStep
    m, cfg = _bf16_model(mlp="f32")
    xx, yy, msk = _batch(cfg, 4)
    g = GraphedTrainStep(m, _opt(m), xx, yy, msk, warmup=1)
    assert g.owned is None
    m.mlp_precision = "bf16"
    with torch.no_grad():
        m(xx)                                                  # makes the bf16 packs
        g.replay(1e-3)
        after_replay = m(xx)[0]
        m.packs.get("bf16").refresh()
        after_refresh = m(xx)[0]
    assert torch.equal(after_replay, after_refresh)


def test_touch_after_a_flat_write_repacks():
    """writes through fp.flat change no tensor version: FlatParams.touch() declares them, and the next forward re-packs"""
    from dpot_amd.train import train_step
    m, cfg = _bf16_model()
    xx, yy, msk = _batch(cfg, 4)
    opt = _opt(m)
    train_step(m, opt, xx, yy, msk, lr=1e-3)                  # Adam wrote the packs: they are fresh
    m2, _ = _bf16_model(salt=11)
    fp2 = _opt(m2).fp                                          # (the same flat layout as the model under test)
    with torch.no_grad():
        opt.fp.flat[:] = fp2.flat
        opt.fp.touch()
        assert torch.equal(m(xx)[0], m2(xx)[0])


@pytest.mark.parametrize("E,mh,depth", [(1024, 4096, 3), (1536, 6144, 2)])
def test_adam_step_packs_at_model_sizes(E, mh, depth):
    """dpot_adam_step_packs at the weight shapes of DPOT-M / DPOT-L (a flat buffer laid out like the model's: small tensors between
    the channel-MLP weights, a > 2^20-element stretch, a tail the optimiser does not touch): parameters and both moments
    bit-identical to dpot_adam_step over the same buffers, both packs of every weight bit-identical to dpot_bf16_pack_jobs of
    the updated parameters; with and without the clip coefficient"""
    from dpot_amd import ops
    torch.manual_seed(E)
    sizes = []
    for _ in range(depth):
        sizes += [2 * E, 4 * E * 96, mh * E, mh, E * mh, E]          # norms | AFNO-ish | W1 | b1 | W2 | b2
    sizes = [(1 << 20) + 12345 * 4] + sizes + [4096]
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (n + 3) // 4 * 4
    n_active = offs[-1]
    p0 = torch.randn(off, device="cuda") * 0.05
    g = torch.randn(off, device="cuda") * 0.01
    m0, v0 = torch.randn(off, device="cuda") * 0.01, torch.rand(off, device="cuda") * 1e-4
    hyper = torch.zeros(8, device="cuda")
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.adam_stage(hyper, step, 1e-3, 0.9, 0.9, 1e-8, 1e-6, 0.5, 3)
    part, ss = torch.zeros(1024, device="cuda"), torch.zeros(1, device="cuda")
    ops.sumsq(g[:n_active], ss, part)

    def weights(p):
        ws = []
        for d in range(depth):
            i = 1 + 6 * d
            ws += [p[offs[i + 2]:offs[i + 2] + mh * E].view(mh, E), p[offs[i + 4]:offs[i + 4] + E * mh].view(E, mh)]
        return ws

    def jobs(p):
        out = []
        for w in weights(p):
            R_, K = w.shape
            out += [(w, R_, K, K, False), (w, K, R_, K, True)]
        return out

    for clip in (None, ss):
        pa, ma, va = p0.clone(), m0.clone(), v0.clone()
        ops.adam_step(pa[:n_active], g[:n_active], ma[:n_active], va[:n_active], hyper, clip, 0.5)
        ref = ops.PanelPacks(jobs(pa), bf16=True)
        ref.refresh()
        pb, mb, vb = p0.clone(), m0.clone(), v0.clone()
        pk = ops.PanelPacks(jobs(pb), bf16=True)
        for b in pk.bufs:
            b.zero_()
        plan = ops.AdamPackPlan.build(pb, n_active, pk)
        assert plan is not None and plan.ntiles == depth * 2 * (mh // 64) * (E // 256) and plan.max_range <= 1 << 20
        ops.adam_step_packs(plan, pb, g, mb, vb, hyper, clip, 0.5)
        torch.cuda.synchronize()
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
        assert torch.equal(pb[n_active:], p0[n_active:])                      # the tail is not touched
        for a, b in zip(ref.bufs, pk.bufs):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_adam_step_packs_at_the_smallest_weight(guarded):
    """dpot_adam_step_packs at the smallest weight dpot_adam_pack_supported admits (rows = 64, K = 256: ONE 64 x 256 tile)
    between small tensors, on guarded buffers (tests/guard.py): parameters and moments bit-identical to dpot_adam_step and
    within the neighbouring test's bound of the float64 update rule; both packs, NaN before the launch, bit-identical to the
    packs of the updated weight; the tail beyond n_active and every guard untouched"""
    from dpot_amd import ops
    rows, K = 64, 256
    assert ops._lib.load().dpot_adam_pack_supported(rows, K) and not ops._lib.load().dpot_adam_pack_supported(rows - 32, K)
    sizes = [100, rows * K, 36, 64]
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (n + 3) // 4 * 4
    n_active = offs[-1]
    gen = torch.Generator().manual_seed(64)
    p0, g = torch.randn(off, generator=gen) * 0.05, torch.randn(off, generator=gen) * 0.01
    m0, v0 = torch.randn(off, generator=gen) * 0.01, torch.rand(off, generator=gen) * 1e-4
    lr, b1, b2, eps, wd, gscale = 1e-3, 0.9, 0.9, 1e-8, 1e-6, 0.5
    hyper = guard.wrap(torch.zeros(8), "cuda")
    step = guard.wrap(torch.zeros(1, dtype=torch.int64), "cuda")
    ops.adam_stage(hyper, step, lr, b1, b2, eps, wd, 1e9, 1)
    gd = guard.wrap(g, "cuda")
    weight = lambda p: p[offs[1]:offs[1] + rows * K].view(rows, K)
    jobs = lambda p: [(weight(p), rows, K, K, False), (weight(p), K, rows, K, True)]
    pa, ma, va = (guard.wrap(t, "cuda") for t in (p0, m0, v0))
    ops.adam_step(pa[:n_active], gd[:n_active], ma[:n_active], va[:n_active], hyper, None, gscale)
    ref = ops.PanelPacks(jobs(pa), bf16=True)
    ref.refresh()
    pb, mb, vb = (guard.wrap(t, "cuda") for t in (p0, m0, v0))
    pk = ops.PanelPacks(jobs(pb), bf16=True)
    for b in pk.bufs:
        b.fill_(float("nan"))
    plan = ops.AdamPackPlan.build(pb, n_active, pk)
    assert plan is not None and plan.ntiles == 1
    ops.adam_step_packs(plan, pb, gd, mb, vb, hyper, None, gscale)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert torch.equal(pb[n_active:].cpu(), p0[n_active:]) and torch.equal(mb[n_active:].cpu(), m0[n_active:])
    for a, b in zip(ref.bufs, pk.bufs):
        assert torch.isfinite(b.float()).all() and torch.equal(a.view(torch.int16), b.view(torch.int16))
    pr, mr, vr = p0[:n_active].clone().double(), m0[:n_active].clone().double(), v0[:n_active].clone().double()
    R.adam_update(pr, g[:n_active].double() * gscale, mr, vr, 1, lr, b1, b2, eps, wd)
    assert (pb[:n_active].cpu().double() - pr).abs().max().item() <= 2e-3 * lr
    assert_close(mb[:n_active], mr, "exp_avg")
    assert_close(vb[:n_active], vr, "exp_avg_sq")


# ------------------------------------------------------------------------------------------------------
def _shared_step_run(kind):
    """mini model, batch 2, two AR steps (every parameter gradient accumulated once), clip on, metrics attached, the weighted
    classification loss training cls_head.  max_norm = 0.5 lies below the gradient norm of these steps
    (3.3 and 1.6 for the relative-L2 part alone in oracle.dpot_ref.train_step): the clip rescales"""
    from dpot_amd import StepMetrics
    from dpot_amd.train import FlatParams, FusedAdam, FusedLamb
    m, cfg = build(R.MINI, salt=5)
    xx, yy, msk = _batch(cfg, 2, T_ar=2)
    cls = (torch.arange(2, device="cuda") % cfg.n_cls).view(2, 1)
    args = dict(lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=0.5, update_tail=True)
    opt = FusedAdam(FlatParams(m), **args) if kind == "adam" else FusedLamb(FlatParams(m), debias=True, **args)
    met = StepMetrics("cuda", 2)
    return m, opt, met, (xx, yy, msk), dict(cls=cls, cls_weight=0.5, metrics=met)


def _shared_step_state(opt, met):
    torch.cuda.synchronize()
    st = {"flat": opt.fp.flat, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq, "step_dev": opt.step_dev, "acc": met.acc[0]}
    if hasattr(opt, "norms"):
        st["norms"] = opt.norms
    return {k: v.clone() for k, v in st.items()}, opt.step_count, opt.lr


@pytest.mark.parametrize("kind", ["adam", "lamb"])
def test_eager_and_replayed_steps_share_one_body_and_warm_up_is_undone(kind):
    """train_step, the warm-up of GraphedTrainStep and its captured graph run ONE step body (train._forward_backward +
    train._optimise), and warm-up steps sit inside train.trial_state.  (a) two eager steps and two replays from the same seeded
    start leave parameters, moments, the step counter, LAMB's norms and the metrics accumulator bit-identical; (b) building a
    graph step with warmup=2 on the TRAINED state (non-zero moments, step 2, a filled accumulator) leaves all of them as they
    were.  Cells other tests hold already: Adam's warm-up from the zero state (test_graph_warmup_does_not_train), an unlogged
    warm-up with cls_weight = 0 (test_gpu_metrics.test_metrics_observe_without_changing_the_step_and_sum_up), LAMB replay
    against eager at T_ar = 1 without metrics (test_gpu_lamb.test_graph_replay_bit_identical_to_eager)."""
    from dpot_amd.train import GraphedTrainStep, train_step
    lrs = (1e-3, 2e-3)
    m, opt, met, batch, kw = _shared_step_run(kind)
    for lr in lrs:
        train_step(m, opt, *batch, lr=lr, **kw)
    eager = _shared_step_state(opt, met)
    assert float(opt.grad_norm()) > opt.max_norm, "the clip must be active, or sumsq reaches the update unused"
    GraphedTrainStep(m, opt, *batch, warmup=2, **kw)                     # (b)
    after = _shared_step_state(opt, met)
    assert after[1:] == eager[1:] == (2, lrs[-1])
    for k, v in eager[0].items():
        assert torch.equal(v, after[0][k]), f"{k} changed by building a graph step"
    assert int(eager[0]["step_dev"]) == 2 and float(eager[0]["exp_avg"].abs().max()) > 0.0

    m2, opt2, met2, batch2, kw2 = _shared_step_run(kind)                 # (a)
    g = GraphedTrainStep(m2, opt2, *batch2, warmup=2, **kw2)
    for lr in lrs:
        g.replay(lr)
    replayed = _shared_step_state(opt2, met2)
    assert replayed[1:] == eager[1:]
    for k, v in eager[0].items():
        assert torch.equal(v, replayed[0][k]), f"{k}: replayed steps differ from eager steps"
    assert met2.read()["opt_steps"] == 2 and met2.read()["ar_steps"] == 4


_COLD_GRAPH_CHILD = """
import sys
sys.path.insert(0, {root!r})
import torch
from dpot_amd import DPOTNet
from dpot_amd.train import FlatParams, FusedAdam, GraphedTrainStep, train_step
from oracle import dpot_ref as R
cfg = R.DPOTConfig(**R.MINI)
S, B = cfg.img_size, 2
xx = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=1).cuda()
yy = R.recipe_input((B, S, S, 2, cfg.out_channels), salt=2).cuda()
msk = torch.ones(B, S, S, 1, cfg.out_channels, device="cuda")
def fresh():
    m = DPOTNet(**R.MINI)
    m.load_state_dict(R.recipe_state_dict(cfg, salt=5))
    m.cuda()
    return m, FusedAdam(FlatParams(m), lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
m, opt = fresh()
g = GraphedTrainStep(m, opt, xx, yy, msk, warmup=1)        # the first kernel launches of this process
for lr in (1e-3, 2e-3):
    loss = g.replay(lr)
m2, opt2 = fresh()
for lr in (1e-3, 2e-3):
    loss2, _ = train_step(m2, opt2, xx, yy, msk, lr=lr)
torch.cuda.synchronize()
assert loss.item() == loss2.item(), (loss.item(), loss2.item())
assert torch.equal(opt.fp.flat, opt2.fp.flat) and torch.equal(opt.exp_avg, opt2.exp_avg)
print("cold graph step ok")
"""


def test_graph_step_captured_in_a_cold_process_equals_the_eager_step():
    """a fresh process whose first launches are GraphedTrainStep's warm-up: the warm-up is what lifts every kernel's dynamic-LDS
    cap (csrc/common.h raise_dynamic_lds, once per kernel and device), inside the capture behind it the helper only reads the
    current device, and the replays leave the parameters and moments of the eager steps, bit for bit (those run after them in the
    same child)"""
    import subprocess
    code = _COLD_GRAPH_CHILD.format(root=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0 and "cold graph step ok" in r.stdout, r.stdout[-3000:]
