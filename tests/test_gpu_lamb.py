"""GPU tests of the fused LAMB optimiser (csrc/loss_opt.hip lamb_*, ops.lamb_step, train.FusedLamb): the reference's Lamb
(g14_lamb) and the float64 restatement (tests/lamb_ref.py) at op level in the three configurations of the fixture, the
chunked per-tensor reduction on a DPOT-M-like flat buffer, FusedLamb on a model, graph replay, checkpoints and data
parallelism."""
import os
import sys

import numpy as np
import pytest
import torch

import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import load
from lamb_ref import LambState, config, lamb_step
from oracle import dpot_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM_KEYS = ("weight_norm", "adam_norm", "trust_ratio")


def _check_update(du, du_ref, p_ref, what, rel_tol=1e-4):
    """an optimiser UPDATE p_new - p_old against a reference update: norm-wise in float64, then element-wise with the fp32
    rounding of p on top (a small update hides in p)"""
    du, du_ref, p_ref = (np.asarray(x, dtype=np.float64) for x in (du, du_ref, p_ref))
    # the fp32 result rounds each p_new to 2^-24 of itself: allow that on top of rel_tol (p ~ 1e3 next to updates ~ 1e-3)
    err = np.linalg.norm(du - du_ref)
    assert err <= rel_tol * np.linalg.norm(du_ref) + 2.0 ** -23 * np.linalg.norm(p_ref), (what, err, np.linalg.norm(du_ref))
    tol = 1e-3 * np.abs(du_ref) + 1e-4 * np.abs(du_ref).max() + 2.0 ** -23 * max(np.abs(p_ref).max(), 1e-30)
    err = np.abs(du - du_ref)
    assert (err <= tol).all(), (what, int((err > tol).sum()), err.max())


def _layout(numels, pad_to=4):
    offs, off = [], 0
    for n in numels:
        offs.append(off)
        off += (n + pad_to - 1) // pad_to * pad_to
    return offs, off


# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ["a", "b", "c"])
def test_op_level_lamb_vs_reference_and_restatement(c, guarded):
    """ops.lamb_stage + ops.lamb_step on a flat buffer holding the g14 tensors (and an untouched tail), grad_scale 0.5: the
    per-step updates, the per-tensor norms and the final moments equal the reference's Lamb and the restatement.  Every
    buffer the kernels see sits between guards (tests/guard.py): the chunk tables of the plan, the flat buffers, the slots"""
    from dpot_amd import ops
    fx = load("g14_lamb")
    kw = config(fx, c)
    names = [str(n) for n in fx["names"]]
    shapes = [fx[f"p0.{n}"].shape for n in names]
    numels = [int(np.prod(s)) for s in shapes]
    offs, n_act = _layout(numels)
    total = n_act + 64                                           # a tail outside the optimiser's range
    dev = "cuda"
    p = torch.randn(total, device=dev)
    for n, o, k in zip(names, offs, numels):
        p[o:o + k] = torch.from_numpy(fx[f"p0.{n}"].reshape(-1)).to(dev)
    p = guard.wrap(p)
    g = guard.wrap(torch.zeros(total, device=dev))
    m, v = guard.wrap(torch.zeros(total, device=dev)), guard.wrap(torch.zeros(total, device=dev))
    hyper = guard.wrap(torch.zeros(16, device=dev))
    step = guard.wrap(torch.zeros(1, dtype=torch.int64, device=dev))
    sumsq, part = guard.wrap(torch.zeros(1, device=dev)), guard.wrap(torch.zeros(1024, device=dev))
    plan = ops.LambPlan(offs, numels, n_act, dev)
    nt = len(names)
    norms = guard.wrap(torch.zeros(3 * nt, device=dev))
    s = 0.5
    tail0 = p[n_act:].clone()
    params = [fx[f"p0.{n}"].astype(np.float64) for n in names]
    st = LambState(params)
    for k in range(int(fx["steps"])):
        grads = [fx[f"g{k}.{n}"] for n in names]
        for o, kk, gr in zip(offs, numels, grads):
            g[o:o + kk] = torch.from_numpy(gr.reshape(-1) / s).to(dev)
        before = p.clone()
        ops.lamb_stage(hyper, step, kw["lr"], kw["betas"][0], kw["betas"][1], kw["eps"], kw["weight_decay"],
                       kw["max_norm"] or 0.0, kw["clamp_value"], kw["debias"])
        if kw["max_norm"] is not None:
            ops.sumsq(g[:n_act], sumsq, part)
        ops.lamb_step(plan, p, g, m, v, hyper, sumsq if kw["max_norm"] is not None else None, norms, grad_scale=s,
                      adam=kw["adam"])
        torch.cuda.synchronize()
        restate_prev = [x.copy() for x in params]
        params = lamb_step(params, [gr / s for gr in grads], st, grad_scale=s, **kw)
        got_n = norms.cpu().double().numpy().reshape(3, nt)
        for i, (n, o, kk) in enumerate(zip(names, offs, numels)):
            du = (p[o:o + kk] - before[o:o + kk]).double().cpu().numpy()
            ref_prev = fx[f"p0.{n}"] if k == 0 else fx[f"{c}.p{k}.{n}"]
            ref = fx[f"{c}.p{k + 1}.{n}"].reshape(-1)
            _check_update(du, ref.astype(np.float64) - ref_prev.reshape(-1), ref, f"{c} step {k + 1} {n} vs reference")
            _check_update(du, (params[i] - restate_prev[i]).reshape(-1), ref, f"{c} step {k + 1} {n} vs restatement")
            for j, key in enumerate(NORM_KEYS):
                want = float(fx[f"{c}.{key}{k + 1}.{n}"])
                assert abs(got_n[j, i] - want) <= 2e-5 * abs(want) + 1e-12, (c, k + 1, n, key, got_n[j, i], want)
                mine = (st.weight_norm, st.adam_norm, st.trust_ratio)[j][i]
                assert abs(got_n[j, i] - mine) <= 2e-5 * abs(mine) + 1e-12, (c, k + 1, n, key, got_n[j, i], mine)
    assert int(step.item()) == int(fx["steps"])
    for i, (n, o, kk) in enumerate(zip(names, offs, numels)):
        for buf, key in ((m, "exp_avg"), (v, "exp_avg_sq")):
            got = buf[o:o + kk].double().cpu().numpy()
            want = fx[f"{c}.{key}.{n}"].reshape(-1).astype(np.float64)
            assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max() + 1e-30, (c, key, n)
    assert torch.equal(p[n_act:], tail0)


def _dpot_m_like_sizes():
    """DPOT-M's parameter sizes in FlatParams order (cls_head last) plus runs of tiny and odd-sized tensors"""
    from dpot_amd.model import DPOTNet
    with torch.device("meta"):
        net = DPOTNet(**R.MEDIUM)
    named = [(n, p.numel()) for n, p in net.named_parameters()]
    head = [k for n, k in named if not n.startswith("cls_head.")]
    tail = [k for n, k in named if n.startswith("cls_head.")]
    head += [3, 5, 1, 7, 2, 8191, 8193, 8192, 16385, 6]
    return head, tail


def test_chunk_table_edge_cases_on_dpot_m_layout(guarded):
    """per-tensor norms over the chunk table of a DPOT-M-sized buffer (a 10.5 M-element tensor, tiny neighbours, sizes that
    are not multiples of 4, a tail outside n_active) equal float64 norms of the true ranges; the padding slots and the tail
    stay untouched bit for bit; a second run reproduces every bit; nothing is written outside the buffers (tests/guard.py)"""
    from dpot_amd import ops
    head, tail = _dpot_m_like_sizes()
    assert max(head) > 1 << 20
    sizes = head + tail
    offs, total = _layout(sizes)
    n_act = offs[len(head)]
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(14)
    p0 = torch.randn(total, device=dev, generator=gen) * 0.05
    g = guard.wrap(torch.randn(total, device=dev, generator=gen))
    m0 = torch.randn(total, device=dev, generator=gen) * 0.01
    v0 = torch.rand(total, device=dev, generator=gen) * 1e-3
    p0[offs[1]:offs[1] + sizes[1]] = 0.0                         # one all-zero tensor
    plan = ops.LambPlan(offs[:len(head)], head, n_act, dev)
    assert plan.ntensors == len(head) and plan.nchunks > plan.ntensors
    covered = torch.zeros(total, dtype=torch.bool, device=dev)
    for o, k in zip(offs[:len(head)], head):
        covered[o:o + k] = True
    wd, eps, clamp = 1e-4, 1e-6, 10.0
    runs = []
    for _ in range(2):
        p, m, v = guard.wrap(p0), guard.wrap(m0), guard.wrap(v0)
        hyper = guard.wrap(torch.zeros(16, device=dev))
        step = guard.wrap(torch.zeros(1, dtype=torch.int64, device=dev))
        norms = guard.wrap(torch.zeros(3 * len(head), device=dev))
        ops.lamb_stage(hyper, step, 1e-3, 0.9, 0.999, eps, wd, 0.0, clamp, True)
        ops.lamb_step(plan, p, g, m, v, hyper, None, norms, adam=False)
        torch.cuda.synchronize()
        runs.append((p, m, v, norms))
    p, m, v, norms = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    for new, old in ((p, p0), (m, m0), (v, v0)):
        assert torch.equal(new[~covered], old[~covered])        # padding + tail, bit for bit
    nt = len(head)
    got = norms.double().view(3, nt).cpu()
    for i, (o, k) in enumerate(zip(offs[:nt], head)):
        pd = p0[o:o + k].double()
        r = m[o:o + k].double() / (v[o:o + k].double().sqrt() + eps) + wd * pd
        wn = min(pd.norm().item(), clamp)
        an = r.norm().item()
        assert abs(got[0, i].item() - wn) <= 2e-6 * wn + 1e-30, (i, k, got[0, i].item(), wn)
        assert abs(got[1, i].item() - an) <= 2e-6 * an + 1e-30, (i, k, got[1, i].item(), an)
        tr = 1.0 if wn == 0 or an == 0 else wn / an
        assert abs(got[2, i].item() - tr) <= 5e-6 * tr, (i, k, got[2, i].item(), tr)
    assert got[2, 1].item() == 1.0 and got[0, 1].item() == 0.0


# ------------------------------------------------------------------------------------------------------
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


MODES = {"a": dict(adam=True, debias=False, weight_decay=1e-4, betas=(0.9, 0.9)),
         "b": dict(adam=False, debias=True, weight_decay=1e-4)}


def _lamb(m, mode, **kw):
    from dpot_amd.train import FlatParams, FusedLamb
    args = dict(MODES[mode], lr=1e-3, max_norm=1e4)
    args.update(kw)
    return FusedLamb(FlatParams(m), **args)


@pytest.mark.parametrize("mode", ["a", "b"])
def test_model_steps_equal_restatement(mode):
    """three eager train steps on the mini model: each step's update equals the restatement applied to that step's
    gradient (copied from fp.grad), tensor by tensor; the per-tensor norms match"""
    from dpot_amd.train import train_step
    m, cfg = build(R.MINI, salt=8)
    xx, yy, msk = _batch(cfg, 2)
    opt = _lamb(m, mode)
    fp = opt.fp
    mem = opt.members
    params = [fp.flat[fp.offsets[k]:fp.offsets[k] + fp.params[k].numel()].double().cpu().numpy() for k in mem]
    st = LambState(params)
    kw = dict(MODES[mode], lr=2e-3, eps=1e-6, clamp_value=10.0, max_norm=1e4)
    for _ in range(3):
        before = fp.flat.clone()
        train_step(m, opt, xx, yy, msk, lr=2e-3)
        torch.cuda.synchronize()
        gr = [fp.grad[fp.offsets[k]:fp.offsets[k] + fp.params[k].numel()].double().cpu().numpy() for k in mem]
        old = [before[fp.offsets[k]:fp.offsets[k] + fp.params[k].numel()].double().cpu().numpy() for k in mem]
        new = lamb_step(list(old), gr, st, **kw)
        for j, k in enumerate(mem):
            o, n = fp.offsets[k], fp.params[k].numel()
            du = (fp.flat[o:o + n] - before[o:o + n]).double().cpu().numpy()
            _check_update(du, new[j] - old[j], old[j], f"{mode} {fp.names[k]}")
        got = opt.norms.double().view(3, -1).cpu().numpy()
        for q, want in enumerate((st.weight_norm, st.adam_norm, st.trust_ratio)):
            assert np.allclose(got[q], want, rtol=2e-5, atol=1e-12), (mode, NORM_KEYS[q])
    assert opt.wrote is None and opt.step_count == 3 and int(opt.step_dev.item()) == 3


def _state(opt):
    return [opt.fp.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.norms.clone()]


@pytest.mark.parametrize("case", ["a", "b", "b_bf16"])
def test_graph_replay_bit_identical_to_eager(case):
    """GraphedTrainStep with FusedLamb replays bit-identically to eager train_step from the same snapshot: parameters,
    moments, per-tensor norms.  b_bf16: the bf16 channel MLP - LAMB writes no packs, so the graph owns none and its
    forward re-derives them"""
    from dpot_amd.train import GraphedTrainStep, train_step
    mode = case[0]
    if case == "b_bf16":
        m, cfg = build(dict(R.MINI, embed_dim=256, n_blocks=2, depth=2, mlp_ratio=2), salt=7)
        m.mlp_precision = "bf16"
    else:
        m, cfg = build(R.MINI, salt=5)
    xx, yy, msk = _batch(cfg, 2)
    opt = _lamb(m, mode)
    lrs = (1e-3, 3e-3, 2e-3)
    g = GraphedTrainStep(m, opt, xx, yy, msk, warmup=1)
    assert g.owned is None
    snap = opt.snapshot()
    graph_losses = [g.replay(lr).item() for lr in lrs]
    torch.cuda.synchronize()
    graph = _state(opt)
    opt.restore(snap)
    eager_losses = [train_step(m, opt, xx, yy, msk, lr=lr)[0].item() for lr in lrs]
    torch.cuda.synchronize()
    assert graph_losses == eager_losses
    for a, b in zip(graph, _state(opt)):
        assert torch.equal(a, b)
    assert int(opt.step_dev.item()) == len(lrs)


def test_state_dict_roundtrip_and_reference_layout():
    """FusedLamb.state_dict has the key layout of the reference's Lamb (g14) and resuming from it continues bit for bit;
    a reference checkpoint's plain-number trust_ratio loads"""
    from dpot_amd.train import train_step
    fx = load("g14_lamb")
    m, cfg = build(R.MINI, salt=8)
    xx, yy, msk = _batch(cfg, 2)
    opt = _lamb(m, "b")
    for _ in range(3):
        train_step(m, opt, xx, yy, msk, lr=2e-3)
    sd = opt.state_dict(m)
    norms3 = opt.norms.clone()
    sd_model = {k: v.clone() for k, v in m.state_dict().items()}
    names = [n for n, _ in m.named_parameters()]
    assert sorted(sd["param_groups"][0].keys()) == [str(k) for k in fx["b.group_keys"]]
    for i, n in enumerate(names):
        if n.startswith("cls_head."):
            assert i not in sd["state"]
            continue
        st = sd["state"][i]
        assert sorted(st.keys()) == [str(k) for k in fx["b.state_keys"]]
        assert st["step"] == 3 and all(st[k].dim() == 0 for k in NORM_KEYS)
    train_step(m, opt, xx, yy, msk, lr=2e-3)
    want = _state(opt)
    m2, _ = build(R.MINI, salt=8)
    m2.load_state_dict(sd_model)
    opt2 = _lamb(m2, "b")
    opt2.load_state_dict(sd, m2)
    assert torch.equal(opt2.norms, norms3) and opt2.step_count == 3
    train_step(m2, opt2, xx, yy, msk, lr=2e-3)
    for a, b in zip(want, _state(opt2)):
        assert torch.equal(a, b)
    # the reference keeps trust_ratio = 1 (a Python number) where a norm was zero
    first = min(sd["state"])
    sd["state"][first]["trust_ratio"] = 1
    opt2.load_state_dict(sd, m2)
    j = [i for i, k in enumerate(opt2.members) if opt2.fp.params[k] is list(m2.parameters())[first]][0]
    assert float(opt2.trust_ratio[j]) == 1.0


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_lamb_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)                                 # both ranks share the one GPU of the test box
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dpot_amd import DPOTNet
    from dpot_amd.dp import BucketedGradReducer
    from dpot_amd.train import FlatParams, FusedLamb, make_dp_step
    cfg = R.DPOTConfig(**R.MINI)
    model = DPOTNet(**R.MINI)
    if rank == 0:
        model.load_state_dict(R.recipe_state_dict(cfg, salt=17))
    model.cuda()
    fp = FlatParams(model)
    red = BucketedGradReducer(fp, n_buckets=3, overlap=True)
    red.broadcast_parameters(0)
    B = 4
    xx = R.recipe_input((B, cfg.img_size, cfg.img_size, cfg.in_timesteps, cfg.in_channels), salt=81)
    yy = R.recipe_input((B, cfg.img_size, cfg.img_size, 1, cfg.out_channels), salt=82)
    sl = slice(2 * rank, 2 * rank + 2)
    xs, ys = xx[sl].cuda(), yy[sl].cuda()
    ms = torch.ones_like(ys)
    opt = FusedLamb(fp, lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-4, adam=False, debias=True, max_norm=1e4,
                    update_tail=True)
    before = fp.flat.clone()
    step, info = make_dp_step(model, opt, red, xs, ys, ms, warmup=1)
    losses = [float(step.replay(1e-3).item()) for _ in range(2)]
    torch.cuda.synchronize()
    state = torch.cat([fp.flat, opt.exp_avg, opt.exp_avg_sq, opt.norms]).cpu()
    ref = state.clone()
    dist.broadcast(ref, src=0)
    same = bool(torch.equal(ref, state))
    moved = bool((fp.flat != before).any().item())
    if rank == 0:
        np.savez(os.path.join(out_dir, "dp_lamb.npz"), mode=np.array(info["mode"]), losses=np.array(losses))
    np.savez(os.path.join(out_dir, f"dp_lamb_rank{rank}.npz"), same=same, moved=moved, steps=int(opt.step_dev.item()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_process_dp_lamb_ranks_stay_bit_identical(tmp_path):
    """make_dp_step with FusedLamb(update_tail=True), two gloo ranks on the one GPU, two steps: parameters, moments and
    per-tensor norms are bit-identical on both ranks (the norms are reduced in a fixed order on each rank)"""
    import torch.multiprocessing as mp
    mp.spawn(_dp_lamb_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        got = np.load(os.path.join(str(tmp_path), f"dp_lamb_rank{r}.npz"))
        assert bool(got["same"]) and bool(got["moved"]) and int(got["steps"]) == 2
    assert np.isfinite(np.load(os.path.join(str(tmp_path), "dp_lamb.npz"))["losses"]).all()
