"""What train.FlatOptimizer implements for FusedAdam and FusedLamb alike, pinned without a kernel: the checkpoint layout
(state and group key sets, no entry beyond n_active or before the first step), the load / save round trip, the one-step-count
rule, and snapshot / restore.  The optimisers are built over a CPU FlatParams of the mini model and their buffers are filled
by hand."""
import pytest
import torch

from oracle import dpot_ref as R

NORMS = ("weight_norm", "adam_norm", "trust_ratio")
STATE_KEYS = {"adam": {"step", "exp_avg", "exp_avg_sq"}, "lamb": {"step", "exp_avg", "exp_avg_sq", *NORMS}}
GROUP_KEYS = {"adam": {"lr", "betas", "eps", "weight_decay", "amsgrad", "params"},
              "lamb": {"lr", "betas", "eps", "weight_decay", "params"}}


def _make(kind, **kw):
    from dpot_amd import DPOTNet
    from dpot_amd.train import FlatParams, FusedAdam, FusedLamb
    model = DPOTNet(**R.MINI)
    return model, (FusedAdam if kind == "adam" else FusedLamb)(FlatParams(model), **kw)


def _buffers(opt):
    return [opt.exp_avg, opt.exp_avg_sq, opt.step_dev] + ([opt.norms] if hasattr(opt, "norms") else [])


def _fill(opt, step):
    """what `step` steps leave behind, by hand: moments inside the updated tensors only (padding and the tensors beyond
    n_active stay zero, as the kernels leave them), the device step counter, LAMB's norms"""
    g = torch.Generator().manual_seed(7)
    for p, off in zip(opt.fp.params, opt.fp.offsets):
        if off < opt.n_active:
            n = p.numel()
            opt.exp_avg[off:off + n] = torch.randn(n, generator=g)
            opt.exp_avg_sq[off:off + n] = torch.rand(n, generator=g)
    opt.step_dev.fill_(step)
    opt.step_count = step
    if hasattr(opt, "norms"):
        opt.norms.copy_(torch.rand(opt.norms.shape, generator=g) + 0.5)


@pytest.mark.parametrize("update_tail", [False, True])
@pytest.mark.parametrize("kind", ["adam", "lamb"])
def test_checkpoint_layout_and_round_trip(kind, update_tail):
    model, opt = _make(kind, lr=2e-3, betas=(0.8, 0.95), eps=1e-5, weight_decay=1e-3, update_tail=update_tail)
    names = [n for n, _ in model.named_parameters()]
    # before the first step: no state at all, the group is complete
    sd = opt.state_dict(model)
    assert sd["state"] == {} and len(sd["param_groups"]) == 1
    group = sd["param_groups"][0]
    assert set(group) == GROUP_KEYS[kind] and group["params"] == list(range(len(names)))
    assert (group["lr"], group["betas"], group["eps"], group["weight_decay"]) == (2e-3, (0.8, 0.95), 1e-5, 1e-3)
    assert kind != "adam" or group["amsgrad"] is False
    # after five: one entry per UPDATED tensor, keyed by its index in model.parameters()
    _fill(opt, 5)
    sd = opt.state_dict(model)
    updated = [i for i, n in enumerate(names) if update_tail or not n.startswith("cls_head.")]
    assert len(updated) < len(names) or update_tail                      # the mini model has a tail to leave out
    assert sorted(sd["state"]) == updated
    where = {id(p): (j, off) for j, (p, off) in enumerate(zip(opt.fp.params, opt.fp.offsets))}
    for i, p in enumerate(model.parameters()):
        if i not in sd["state"]:
            assert where[id(p)][1] >= opt.n_active
            continue
        st, (j, off) = sd["state"][i], where[id(p)]
        assert set(st) == STATE_KEYS[kind] and st["step"] == 5
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert torch.equal(st["exp_avg"].reshape(-1), opt.exp_avg[off:off + p.numel()])
        assert torch.equal(st["exp_avg_sq"].reshape(-1), opt.exp_avg_sq[off:off + p.numel()])
        assert st["exp_avg"].data_ptr() != opt.exp_avg[off:].data_ptr()                      # a copy, not a view
        if kind == "lamb":
            assert all(st[k].dim() == 0 and float(st[k]) == float(getattr(opt, k)[j]) for k in NORMS)
    # a fresh instance with other hyper-parameters takes over every buffer and the group's values
    model2, opt2 = _make(kind, update_tail=update_tail)
    opt2.exp_avg.fill_(3.0)                                  # (stale contents must not survive the load)
    opt2.load_state_dict(sd, model2)
    for a, b in zip(_buffers(opt), _buffers(opt2)):
        assert torch.equal(a, b)
    assert opt2.step_count == 5
    assert (opt2.lr, opt2.betas, opt2.eps, opt2.weight_decay) == (2e-3, (0.8, 0.95), 1e-5, 1e-3)
    assert opt2.param_groups[0]["lr"] == 2e-3
    # an empty checkpoint resets to step 0
    opt2.load_state_dict({"state": {}}, model2)
    assert int(opt2.step_dev) == 0 and opt2.step_count == 0 and float(opt2.exp_avg.abs().max()) == 0.0 and opt2.lr == 2e-3
    # one step counter for the whole buffer
    sd["state"][updated[1]]["step"] = 6
    with pytest.raises(ValueError, match=r"per-parameter step counts differ \(\[5, 6\]\)"):
        opt2.load_state_dict(sd, model2)


@pytest.mark.parametrize("kind", ["adam", "lamb"])
def test_tail_entries_loaded_into_an_optimiser_that_leaves_the_tail_alone(kind):
    """a checkpoint written with update_tail=True, read with update_tail=False.  Adam takes the tail's moments as well and
    holds its step to the one-count rule; LAMB, whose per-tensor state has no slot for the tail, reads neither"""
    model, opt = _make(kind, update_tail=True)
    _fill(opt, 3)
    sd = opt.state_dict(model)
    model2, opt2 = _make(kind, update_tail=False)
    opt2.load_state_dict(sd, model2)
    n = opt2.n_active
    assert n < opt2.fp.total and int(opt2.step_dev) == 3
    assert torch.equal(opt2.exp_avg[:n], opt.exp_avg[:n]) and torch.equal(opt2.exp_avg_sq[:n], opt.exp_avg_sq[:n])
    tail = [i for i, p in enumerate(model2.parameters()) if any(p is q for q, off in zip(opt2.fp.params, opt2.fp.offsets)
                                                                 if off >= n)]
    assert tail
    sd["state"][tail[0]]["step"] = 4
    if kind == "adam":
        assert torch.equal(opt2.exp_avg[n:], opt.exp_avg[n:]) and float(opt2.exp_avg[n:].abs().max()) > 0.0
        with pytest.raises(ValueError, match=r"per-parameter step counts differ \(\[3, 4\]\)"):
            opt2.load_state_dict(sd, model2)
    else:
        nt = len(opt2.members)
        assert float(opt2.exp_avg[n:].abs().max()) == 0.0 and float(opt2.exp_avg_sq[n:].abs().max()) == 0.0
        assert all(torch.equal(getattr(opt2, k), getattr(opt, k)[:nt]) for k in NORMS)
        opt2.load_state_dict(sd, model2)                     # the tail's step is not looked at
        assert int(opt2.step_dev) == 3


def test_lamb_reads_the_reference_plain_number_trust_ratio():
    model, opt = _make("lamb")
    _fill(opt, 2)
    sd = opt.state_dict(model)
    first = min(sd["state"])
    sd["state"][first]["trust_ratio"] = 1
    model2, opt2 = _make("lamb")
    opt2.load_state_dict(sd, model2)
    j = [k for k, p in enumerate(opt2.fp.params) if p is list(model2.parameters())[first]][0]
    want = opt.trust_ratio.clone()
    want[j] = 1.0
    assert torch.equal(opt2.trust_ratio, want) and torch.equal(opt2.weight_norm, opt.weight_norm)


@pytest.mark.parametrize("kind", ["adam", "lamb"])
def test_snapshot_restore(kind):
    """restore brings back parameters, moments, counters and lr, declares the parameters changed, and marks no weight pack
    fresh (Adam does so only for a pack set it writes itself; a CPU model has none)"""
    model, opt = _make(kind, lr=1e-3)
    _fill(opt, 4)
    before = [t.clone() for t in [opt.fp.flat] + _buffers(opt)]
    snap = opt.snapshot()
    for t in [opt.fp.flat] + _buffers(opt):
        t.add_(1)
    opt.step_count, opt.lr, opt.param_groups[0]["lr"] = 9, 5e-2, 5e-2
    epoch = opt.fp.epoch
    opt.restore(snap)
    for a, b in zip(before, [opt.fp.flat] + _buffers(opt)):
        assert torch.equal(a, b)
    assert (opt.step_count, opt.lr, opt.param_groups[0]["lr"]) == (4, 1e-3, 1e-3)
    assert opt.fp.epoch > epoch and opt.packs.fresh is None and opt.wrote is None
    opt.fp.flat.add_(1)                                      # the snapshot holds copies: it restores a second time
    opt.restore(snap)
    assert torch.equal(opt.fp.flat, before[0])
