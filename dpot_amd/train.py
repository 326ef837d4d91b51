"""Rollout driver of the DPOT pre-training step (reference: train_temporal.py:189-230), MI355X style:

  * the auto-regressive rollout, the masked relative-L2 loss, backward, global-norm clip and Adam are all
    enqueued on one HIP stream with NO host synchronisation (the reference does three ``.item()`` per step);
  * parameters, gradients and Adam moments live in flat fp32 buffers: one fused kernel does clip + Adam for the
    whole model (the reference loops over 61 tensors in Python, utils/optimizer.py:26-52), and the flat gradient
    buffer is what the data-parallel reducer all-reduces in buckets (dp.py);
  * learning rate / bias corrections are read from device memory, so a fixed-shape step can be captured in a
    hipGraph and replayed (``GraphedTrainStep``).
"""
from __future__ import annotations

import contextlib
import functools
import math
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import ops
from .functional import clear_grad_packs, cls_ce_loss, rel_l2_loss

Tensor = torch.Tensor


# ------------------------------------------------------------------------------------------------------
class FlatParams:
    """Re-homes the parameters of ``model`` into one flat fp32 buffer (and their .grad into another).

    ``order`` puts parameters whose names start with one of ``tail_prefixes`` (cls_head: it gets no gradient in
    single-GPU training, train_temporal.py:226) at the end, so the optimiser can address 'everything with a
    gradient' as one contiguous prefix."""

    # forward execution order of DPOTNet's sub-modules (registration order puts time_agg_layer after the blocks):
    # gradients then become final from the END of the buffer towards its start, so contiguous buckets can be
    # all-reduced while the rest of the backward still runs (dp.py)
    EXEC_ORDER = ("patch_embed.", "pos_embed", "time_agg_layer.", "scale_feats_", "blocks.", "out_layer.")

    @classmethod
    def _exec_rank(cls, name: str):
        for i, pre in enumerate(cls.EXEC_ORDER):
            if name.startswith(pre):
                return (i, int(name.split(".")[1])) if pre == "blocks." else (i, 0)
        return (len(cls.EXEC_ORDER), 0)

    def __init__(self, model: nn.Module, tail_prefixes: Sequence[str] = ("cls_head.",)):
        self.model = model
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        head = [(n, p) for n, p in named if not any(n.startswith(t) for t in tail_prefixes)]
        head.sort(key=lambda np_: self._exec_rank(np_[0]))                     # stable: registration order within a module
        tail = [(n, p) for n, p in named if any(n.startswith(t) for t in tail_prefixes)]
        self.names = [n for n, _ in head + tail]
        self.params = [p for _, p in head + tail]
        dev, dt = self.params[0].device, torch.float32
        # every tensor starts on a 4-float boundary so float4 kernels and bucket slices stay aligned
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + 3) // 4 * 4
        self.total = off
        self.n_head = self.offsets[len(head)] if tail else off
        self.flat = torch.zeros(self.total, dtype=dt, device=dev)
        self.grad = torch.zeros(self.total, dtype=dt, device=dev)
        self.grad_views: List[Tensor] = []
        n_p = len(self.params)
        self.filled: List[bool] = [False] * n_p      # slot already holds a gradient contribution this step
        self.pending: List[int] = [0] * n_p          # forward uses whose backward has not delivered yet
        self.callbacks: List[Callable[[int], None]] = []   # fired with the parameter index when its grad is final
        self.epoch = 0                               # advanced by touch() whenever the parameters change
        with torch.no_grad():
            for i, (p, o) in enumerate(zip(self.params, self.offsets)):
                n = p.numel()
                self.flat[o:o + n].copy_(p.detach().reshape(-1))
                p.data = self.flat[o:o + n].view(p.shape)
                self.grad_views.append(self.grad[o:o + n].view(p.shape))
                p.grad = self.grad_views[i]
                # The stage backwards (functional._Sink) write parameter gradients STRAIGHT into these slots (first
                # contribution of a step: the kernel's output buffer is the slot; later ones - AR rollout, the model
                # runs T_ar times - are added in place) and return None to autograd, so there is no per-parameter
                # accumulate kernel.  p.grad stays bound to the slot, so foreign autograd graphs still accumulate
                # into the flat buffer the ordinary way.
                p._dpot_grad_slot = (self, i)

    def zero_grad(self) -> None:
        self.grad.zero_()
        for i, p in enumerate(self.params):
            self.filled[i] = False
            self.pending[i] = 0
            if p.grad is None or p.grad.data_ptr() != self.grad_views[i].data_ptr():
                p.grad = self.grad_views[i]

    def fire(self, i: int) -> None:
        for cb in self.callbacks:
            cb(i)

    def touch(self) -> None:
        """Declare the parameters changed.  The optimiser, a graph replay and the reducer's broadcast call it; call it yourself
        after writing parameters in a way their tensor versions do not see (through ``p.data`` or ``fp.flat``).  Every
        weight-derived copy of the model is then re-derived by the next forward (packs.ModelPacks), and the backward of a
        forward that ran before raises instead of reading overwritten copies (functional._check_epoch)."""
        self.epoch += 1


def complex_pair_ranges(flat: FlatParams, n_active: int):
    """[(name, (lo, hi))] of the updated tensors of ``flat`` whose parameter is marked ``_dpot_complex_pairs`` (a complex tensor
    stored as its view_as_real: FNO3d's spectral weights): float ranges of the flat buffer.  Tensors start on 4-float
    boundaries and hold whole pairs, so no pair straddles a tensor"""
    return [(n, (off, off + p.numel())) for n, p, off in zip(flat.names, flat.params, flat.offsets)
            if getattr(p, "_dpot_complex_pairs", False) and off < n_active]


class FlatOptimizer:
    """The fused optimisers over a FlatParams buffer: everything but the update rule.  Moments, the device-side step counter,
    the global-norm clip, snapshot / restore and the reference's torch.optim checkpoint layout live here.  A subclass sets
    ``HYPER`` and implements ``_stage(max_norm, advance)`` (its ``ops.*_stage`` call) and ``_update(plan, sumsq, grad_scale)``
    (its update launch); it may set ``STATE``, ``PER_TENSOR`` and ``GROUP_EXTRA`` and override ``_pack_plan``.

    Host/device protocol of a step: ``stage_hyper(lr)`` enqueues a one-thread kernel that receives lr / betas / eps /
    weight decay / max_norm BY VALUE, advances the DEVICE-side step counter and derives the bias corrections from
    it; ``launch()`` (capturable) enqueues ||g||^2 + the update kernels, which read those values from device
    memory.  There is no host staging buffer, so a host that runs many (graph-replayed) steps ahead of the GPU
    cannot disturb a step that is still queued."""
    HYPER = 0                                 # floats of the ``hyper`` block its stage kernel fills
    STATE: Tuple[str, ...] = ()               # attributes: further tensors of a snapshot
    PER_TENSOR: Tuple[str, ...] = ()          # attributes: one float per updated tensor, a 0-d tensor each in the checkpoint
    GROUP_EXTRA: Dict[str, object] = {}       # further param_groups keys of the checkpoint

    def __init__(self, flat: FlatParams, lr: float, betas: Tuple[float, float], eps: float, weight_decay: float,
                 max_norm: Optional[float], update_tail: bool):
        self.fp = flat
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.max_norm = max_norm
        self.update_tail = update_tail
        dev = flat.flat.device
        self.exp_avg = torch.zeros_like(flat.flat)
        self.exp_avg_sq = torch.zeros_like(flat.flat)
        self.hyper = torch.zeros(self.HYPER, dtype=torch.float32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)     # the step counter the kernels use
        self.sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self._part = torch.zeros(1024, dtype=torch.float32, device=dev)
        self.step_count = 0                       # host mirror of step_dev (number of steps ENQUEUED)
        self.param_groups = [{"lr": lr}]          # minimal torch.optim surface for LR schedulers / logging
        # the model's packs.ModelPacks, or None for a module that is none of the three models.  Only a DPOTNet's ever holds the
        # "bf16" table `adam_plan` asks for: for DPOTNet3D and CDPOTNet the plan stays None and nothing is marked fresh
        self.packs = getattr(flat.model, "packs", None)
        self.wrote = None                         # the pack set the last launch() wrote along with the parameters, or None

    @property
    def n_active(self) -> int:
        return self.fp.total if self.update_tail else self.fp.n_head

    def zero_grad(self) -> None:
        self.fp.zero_grad()

    def step(self, lr: Optional[float] = None, grad_scale: float = 1.0) -> None:
        self.stage_hyper(lr)
        self.launch(grad_scale)

    def stage_hyper(self, lr: Optional[float] = None, advance: int = 1) -> None:
        """host side of a step (NOT capturable by design: call it right before a graph replay)"""
        if lr is not None:
            self.lr = lr
            self.param_groups[0]["lr"] = lr
        self.step_count += advance
        self._stage(self.max_norm if self.max_norm is not None else 0.0, advance)

    def launch(self, grad_scale: float = 1.0) -> None:
        """device side of a step (capturable): ||g||^2 (with clipping), then the update launches"""
        use_clip = self.max_norm is not None
        ops.wgrad_lane_join()         # the backward has joined the weight-gradient lane already; this costs a list lookup
        if use_clip:
            ops.sumsq(self.fp.grad[:self.n_active], self.sumsq, self._part)
        plan = self._pack_plan()
        self._update(plan, self.sumsq if use_clip else None, grad_scale)
        self.fp.touch()               # parameters changed: a backward of an EARLIER forward must not run any more
        self.wrote = plan.pp if plan is not None else None
        if plan is not None:
            self.packs.mark_fresh(plan.pp, self.fp)

    def _pack_plan(self):
        """tables of the weight packs ``_update`` writes along with the parameters (their pack set is ``.pp``), or None"""
        return None

    def grad_norm(self, grad_scale: float = 1.0) -> Tensor:
        """global norm of the gradients currently in the flat buffer (device tensor; reading it synchronises):
        after a step, the value its clip used (train_temporal.py:228 returns it from clip_grad_norm_)"""
        out = torch.empty_like(self.sumsq)
        ops.sumsq(self.fp.grad[:self.n_active], out, self._part)
        return out.sqrt() * grad_scale

    # -- snapshot / restore (graph warm-up, tests) --------------------------------------------------------
    def _state_tensors(self) -> List[Tensor]:
        return [self.fp.flat, self.exp_avg, self.exp_avg_sq, self.step_dev] + [getattr(self, k) for k in self.STATE]

    def snapshot(self):
        return [t.clone() for t in self._state_tensors()], self.step_count, self.lr

    def restore(self, snap) -> None:
        saved, self.step_count, self.lr = snap
        for t, s in zip(self._state_tensors(), saved):
            t.copy_(s)
        self.param_groups[0]["lr"] = self.lr
        self.fp.touch()                          # parameters changed behind the packs' back ...
        plan = self._pack_plan()
        if plan is not None:                     # ... so bring the optimiser-owned weight packs back in line right away: a graph
            plan.pp.refresh()                    # captured after this (graph-step warm-up) must not capture their pack launch
            self.packs.mark_fresh(plan.pp, self.fp)

    # -- checkpoint format of the reference: torch.optim state_dict (train_temporal.py:244,281) ------------
    def state_dict(self, model: nn.Module) -> dict:
        """{'state': {i: {'step', 'exp_avg', 'exp_avg_sq', ...}}, 'param_groups': [...]} with i = index of the parameter
        in ``model.parameters()`` order - what ``torch.save({'optimizer': optimizer.state_dict()})`` of the
        reference's optimisers (utils/optimizer.py) holds.  Parameters the optimiser never updates (cls_head in
        single-GPU training) have no state entry, as in the reference, and before the first step nothing has.  The updated
        tensors are a prefix of ``fp.params``, so tensor j of FlatParams is entry j of a ``PER_TENSOR`` attribute."""
        order = {id(p): i for i, p in enumerate(model.parameters())}
        n_act = self.n_active
        state = {}
        step = int(self.step_dev.item())
        for j, (p, off) in enumerate(zip(self.fp.params, self.fp.offsets)):
            if off >= n_act or step == 0:
                continue
            n = p.numel()
            state[order[id(p)]] = {"step": step,
                                   "exp_avg": self.exp_avg[off:off + n].view(p.shape).clone(),
                                   "exp_avg_sq": self.exp_avg_sq[off:off + n].view(p.shape).clone(),
                                   **{k: getattr(self, k)[j].clone() for k in self.PER_TENSOR}}
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay,
                 **self.GROUP_EXTRA, "params": list(range(len(order)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd: dict, model: nn.Module) -> None:
        """a ``PER_TENSOR`` entry may be a plain number (the reference's Lamb keeps trust_ratio = 1 that way where a norm was 0).
        Entries of tensors beyond ``n_active`` (a checkpoint written with update_tail=True): Adam keeps their moments and
        holds their step to the one-count rule, an optimiser with per-tensor state (LAMB) has no slot for them and reads none"""
        order = {id(p): i for i, p in enumerate(model.parameters())}
        n_act = self.n_active
        steps = set()
        per = {k: torch.zeros(getattr(self, k).shape) for k in self.PER_TENSOR}
        with torch.no_grad():
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            for j, (p, off) in enumerate(zip(self.fp.params, self.fp.offsets)):
                st = sd["state"].get(order[id(p)])
                if st is None or (self.PER_TENSOR and off >= n_act):
                    continue
                n = p.numel()
                self.exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
                for k, vals in per.items():
                    if k in st:
                        vals[j] = float(st[k])
                steps.add(int(st["step"]))
            for k, vals in per.items():
                getattr(self, k).copy_(vals)
        if len(steps) > 1:
            raise ValueError(f"per-parameter step counts differ ({sorted(steps)}): the fused optimiser keeps one")
        step = steps.pop() if steps else 0
        self.step_dev.fill_(step)
        self.step_count = step
        g = sd.get("param_groups", [{}])[0]
        self.lr = g.get("lr", self.lr)
        self.betas = tuple(g.get("betas", self.betas))
        self.eps = g.get("eps", self.eps)
        self.weight_decay = g.get("weight_decay", self.weight_decay)
        self.param_groups[0]["lr"] = self.lr


class FusedAdam(FlatOptimizer):
    """Adam with L2 weight decay folded into the gradient (utils/optimizer.py:9-52 semantics) + global-norm clip
    (train_temporal.py:228), as ONE kernel over the flat buffer.  ``update_tail=False`` reproduces the single-GPU
    reference where cls_head has no gradient and is therefore skipped by the optimiser.  Checkpoint state per tensor:
    'step', 'exp_avg', 'exp_avg_sq' (utils/optimizer.py:101-164).  Parameters marked ``_dpot_complex_pairs`` (FNO3d's spectral
    weights) get ONE second moment per (re, im) pair, the reference's rule for complex parameters - still one launch
    (ops.adam_step_pairs); their moments are kept, and saved, as real pairs."""
    HYPER = 8
    GROUP_EXTRA = {"amsgrad": False}

    def __init__(self, flat: FlatParams, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.0, max_norm: Optional[float] = None,
                 update_tail: bool = False):
        super().__init__(flat, lr, betas, eps, weight_decay, max_norm, update_tail)
        # complex parameters stored as (re, im) pairs (FNO3d's spectral weights): one second moment per pair, as the reference's
        # Adam forms it (utils/optimizer.py:41).  The table is built once; without such a tensor nothing changes
        pairs = complex_pair_ranges(flat, self.n_active)
        self.pair_ranges = ops.adam_pair_ranges([r for _, r in pairs], flat.flat.device) if pairs else None

    def _stage(self, max_norm: float, advance: int) -> None:
        ops.adam_stage(self.hyper, self.step_dev, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                       max_norm, advance)

    def _pack_plan(self):
        if self.pair_ranges is not None:
            return None
        return self.packs.adam_plan(self.fp.flat, self.n_active) if self.packs is not None else None

    def _update(self, plan, sumsq: Optional[Tensor], grad_scale: float) -> None:
        if self.pair_ranges is not None:
            n = self.n_active
            ops.adam_step_pairs(self.fp.flat[:n], self.fp.grad[:n], self.exp_avg[:n], self.exp_avg_sq[:n], self.hyper, sumsq,
                                self.pair_ranges, grad_scale)
        elif plan is not None:
            # round 6: the channel-MLP weights leave the optimiser ALSO as their two bf16 packs - the next forward's pack
            # launch (a second read of every weight written here) disappears (the owner sees them fresh)
            ops.adam_step_packs(plan, self.fp.flat, self.fp.grad, self.exp_avg, self.exp_avg_sq, self.hyper, sumsq,
                                grad_scale)
        else:
            n = self.n_active
            ops.adam_step(self.fp.flat[:n], self.fp.grad[:n], self.exp_avg[:n], self.exp_avg_sq[:n], self.hyper, sumsq,
                          grad_scale)


class FusedLamb(FlatOptimizer):
    """LAMB (utils/optimizer.py:359-499, the reference's ``--opt lamb``) + global-norm clip (train_temporal.py:228) over the
    flat buffer, per parameter tensor: the trust ratio min(||p||, clamp_value) / ||r|| of every tensor is reduced on the
    device (csrc/loss_opt.hip lamb_*: fixed-order chunked reduction, no atomics), so a step is capturable and bit-for-bit
    reproducible.  Weight decay is added to the step r, not to the gradient (unlike Adam).  ``adam=True`` (what the
    reference's scripts pass) does not apply the trust ratio but still records weight_norm / adam_norm / trust_ratio, as
    the reference's state does: they join 'step', 'exp_avg', 'exp_avg_sq' in the checkpoint as 0-d tensors.

    LAMB writes no derived weight packs: ``wrote`` stays None and ``restore`` marks nothing fresh, so a model with the bf16
    channel MLP re-derives its packs in the next forward (inside a captured graph too)."""
    HYPER = 16
    STATE = ("norms",)
    PER_TENSOR = ("weight_norm", "adam_norm", "trust_ratio")

    def __init__(self, flat: FlatParams, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-6, weight_decay: float = 0.0, clamp_value: float = 10.0, adam: bool = False,
                 debias: bool = False, max_norm: Optional[float] = None, update_tail: bool = False):
        if lr <= 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if weight_decay < 0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if clamp_value < 0.0:
            raise ValueError(f"Invalid clamp value: {clamp_value}")
        super().__init__(flat, lr, tuple(betas), eps, weight_decay, max_norm, update_tail)
        pairs = complex_pair_ranges(flat, self.n_active)
        if pairs:
            raise ValueError(f"FusedLamb: parameter {pairs[0][0]!r} holds complex numbers as (re, im) pairs ({len(pairs)} such "
                             "tensors); LAMB's per-pair second moment and complex norms are not built - use FusedAdam")
        self.clamp_value, self.adam, self.debias = clamp_value, adam, debias
        n_act, dev = self.n_active, flat.flat.device
        # the tensors the optimiser updates (FlatParams.offsets are ordered; the tail starts at n_head): a prefix of flat.params
        self.members = [k for k, off in enumerate(flat.offsets) if off < n_act]
        self.plan = ops.LambPlan([flat.offsets[k] for k in self.members],
                                 [flat.params[k].numel() for k in self.members], n_act, dev)
        nt = len(self.members)
        assert self.members == list(range(nt)), "state_dict / load_state_dict index the norms by position in flat.params"
        self.norms = torch.zeros(3 * nt, dtype=torch.float32, device=dev)
        self.weight_norm, self.adam_norm, self.trust_ratio = self.norms[:nt], self.norms[nt:2 * nt], self.norms[2 * nt:]

    def _stage(self, max_norm: float, advance: int) -> None:
        ops.lamb_stage(self.hyper, self.step_dev, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                       max_norm, self.clamp_value, self.debias, advance)

    def _update(self, plan, sumsq: Optional[Tensor], grad_scale: float) -> None:
        ops.lamb_step(self.plan, self.fp.flat, self.fp.grad, self.exp_avg, self.exp_avg_sq, self.hyper, sumsq, self.norms,
                      grad_scale, self.adam)


# ------------------------------------------------------------------------------------------------------
def one_cycle_lr(step: int, total_steps: int, max_lr: float, pct_start: float = 0.3, div_factor: float = 1e4,
                 final_div_factor: float = 1e4) -> float:
    """torch.optim.lr_scheduler.OneCycleLR (cos annealing, two phases) as a pure function of the step index;
    train_temporal.py:140 uses div_factor=1e4, final_div_factor=1e4, pct_start=warmup_epochs/epochs."""
    initial = max_lr / div_factor
    min_lr = initial / final_div_factor
    up_end = float(pct_start * total_steps) - 1.0
    down_end = float(total_steps) - 1.0

    def cos(a, b, pct):
        return b + (a - b) / 2.0 * (math.cos(math.pi * pct) + 1.0)

    if step <= up_end:
        return cos(initial, max_lr, step / up_end if up_end > 0 else 1.0)
    return cos(max_lr, min_lr, (step - up_end) / (down_end - up_end))


# ------------------------------------------------------------------------------------------------------
class StepMetrics:
    """What the reference's loop logs (train_temporal.py:221-223, 232-237; the test loop :252-281), kept on the DEVICE: a
    persistent accumulator that ONE small launch per step folds the step's scalars into - inside the captured graph, after
    the optimiser - and a copy of the last step's values.  Nothing here synchronises except ``read()``.

    Pass it as ``metrics=`` to rollout / train_step / GraphedTrainStep / SegmentedTrainStep / make_dp_step /
    infer.rollout_eval.  It owns the per-AR-step slots the step's kernels write: the relative-L2 statistics of every AR step
    (``ops.rel_l2_combine`` forms the full-rollout loss from them: no second pass over the fields) and the cross-entropy
    results.  ``T_ar_steps_max``: the largest number of AR steps (T_ar / T_bundle) of a rollout it will see.

    Accumulated (``read()``; sums over the steps since ``reset()``): l2_step, l2_full, cls_loss, grad_norm (the norm the
    optimiser's clip used; 0 for an optimiser without max_norm), cls_correct, cls_total (rows with a label inside
    [0, n_cls)), cls_invalid (rows outside: they contribute to nothing else), samples, ar_steps, opt_steps and
    nonfinite_steps (steps whose loss was NaN / inf: counted, never acted on)."""

    def __init__(self, device, T_ar_steps_max: int = 1):
        if T_ar_steps_max < 1:
            raise ValueError(f"StepMetrics: T_ar_steps_max must be >= 1, got {T_ar_steps_max}")
        self.device = torch.device(device)
        self.T_max = int(T_ar_steps_max)
        self.acc = torch.zeros(2, ops.METRICS_WORDS, dtype=torch.int64, device=self.device)     # [running, last step]
        self.cls_out = torch.zeros(self.T_max, ops.CLS_OUT_WORDS, dtype=torch.int64, device=self.device)
        self.l2_full = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.l2_stats: Optional[Tensor] = None          # [T_max, stats floats of one AR step], sized by the first rollout
        self._pending = None

    # -- slots the rollout hands to its kernels ------------------------------------------------------------
    def _check_steps(self, n_steps: int) -> None:
        if n_steps > self.T_max:
            raise ValueError(f"StepMetrics was built for <= {self.T_max} AR steps per rollout, this one has {n_steps}")

    def stats_slot(self, k: int, B: int, S: int, Cc: int) -> Tensor:
        n = ops.rel_l2_stats_elems(B, S, Cc)
        if self.l2_stats is None or self.l2_stats.shape[1] != n:
            self.l2_stats = torch.zeros(self.T_max, n, dtype=torch.float32, device=self.device)
        return self.l2_stats[k]

    def cls_slot(self, k: int) -> Tensor:
        return self.cls_out[k]

    def end_rollout(self, l2_step: Tensor, n_steps: int, B: int, Cc: int, n_cls_out: int) -> None:
        """after the last AR step: one launch forms the full-rollout loss from the step statistics; the values wait for
        ``accumulate``"""
        ops.rel_l2_combine(self.l2_stats, B, Cc, n_steps, out=self.l2_full)
        self._pending = (l2_step.detach().view(1), n_steps, B, n_cls_out)

    def accumulate(self, opt=None, grad_scale: float = 1.0) -> None:
        """fold the rollout that just ended into the accumulator (ONE launch, capturable).  The step classes call it after
        the optimiser launch; call it yourself after a bare ``rollout(..., metrics=m)``."""
        if self._pending is None:
            raise RuntimeError("StepMetrics.accumulate: no rollout has run with this object since the last accumulate")
        l2_step, n_steps, B, n_cls_out = self._pending
        self._pending = None
        sumsq = opt.sumsq if (opt is not None and getattr(opt, "max_norm", None) is not None) else None
        ops.metrics_accum(self.acc, l2_step, self.l2_full, self.cls_out, n_cls_out, sumsq, grad_scale, B, n_steps, 1)

    # -- reading -------------------------------------------------------------------------------------------
    def reset(self) -> None:
        """zero the accumulator by a launch (capturable; the epoch boundary).  No synchronisation."""
        self.acc.zero_()

    def snapshot(self) -> Tensor:
        return self.acc.clone()

    def restore(self, snap: Tensor) -> None:
        self.acc.copy_(snap)

    def last(self) -> Dict[str, Tensor]:
        """the LAST step's values as 0-d device tensors (views: no launch, no synchronisation) - what the reference hands
        to its writer per iteration (train_temporal.py:236-237)"""
        row = self.acc[1]
        d = {k: row[i:i + 1].view(torch.float64)[0] for i, k in enumerate(ops.METRICS_FLOATS)}
        d.update({k: row[len(ops.METRICS_FLOATS) + i] for i, k in enumerate(ops.METRICS_INTS)})
        return d

    def read(self, group=None) -> Dict[str, float]:
        """the ONLY call that synchronises: the accumulator as a plain dict, plus the reference's normalisations
        train_l2_step_avg = l2_step / samples / ar_steps_per_sample, train_l2_full_avg = l2_full / samples,
        cls_acc = cls_correct / cls_total (and the same two averages under the test loop's names).  ``group``: a
        dp.BucketedGradReducer or a process group - the accumulator is then summed over the ranks with ONE all-reduce,
        here at read time and never per step."""
        nf = len(ops.METRICS_FLOATS)
        row = self.acc[0]
        vals = torch.cat([row[:nf].view(torch.float64), row[nf:nf + len(ops.METRICS_INTS)].to(torch.float64)])
        if group is not None:
            import torch.distributed as dist
            pg = getattr(group, "pg", group) if not isinstance(group, bool) else None
            if dist.is_available() and dist.is_initialized():
                dist.all_reduce(vals, op=dist.ReduceOp.SUM, group=pg)
        return self.normalise(vals.cpu().tolist())

    @staticmethod
    def normalise(vals: Sequence[float]) -> Dict[str, float]:
        """the dict of ``read()`` from the 11 accumulated numbers (METRICS_FLOATS then METRICS_INTS order)"""
        nf = len(ops.METRICS_FLOATS)
        d: Dict[str, float] = {k: float(v) for k, v in zip(ops.METRICS_FLOATS, vals[:nf])}
        d.update({k: int(round(v)) for k, v in zip(ops.METRICS_INTS, vals[nf:])})
        nan = float("nan")
        per = d["ar_steps"] / d["opt_steps"] if d["opt_steps"] else nan
        d["ar_steps_per_sample"] = per
        d["train_l2_step_avg"] = d["l2_step"] / d["samples"] / per if d["samples"] and d["opt_steps"] else nan
        d["train_l2_full_avg"] = d["l2_full"] / d["samples"] if d["samples"] else nan
        d["test_l2_step_avg"], d["test_l2_full_avg"] = d["train_l2_step_avg"], d["train_l2_full_avg"]
        d["cls_acc"] = d["cls_correct"] / d["cls_total"] if d["cls_total"] else nan
        d["cls_loss_avg"] = d["cls_loss"] / d["cls_total"] if d["cls_total"] else nan
        d["grad_norm_avg"] = d["grad_norm"] / d["opt_steps"] if d["opt_steps"] else nan
        return d


def check_cls_args(opt, cls: Optional[Tensor], cls_weight: float) -> None:
    """a weighted classification loss needs labels, and an optimiser that updates cls_head: with ``update_tail=False`` the
    head would receive gradients and silently never move"""
    if cls_weight != 0.0:
        if cls is None:
            raise ValueError(f"cls_weight = {cls_weight} needs the dataset labels (cls=...)")
        if opt is not None and not getattr(opt, "update_tail", False):
            raise ValueError(f"cls_weight = {cls_weight} trains cls_head, but the optimiser was built with update_tail=False "
                             "and would leave it frozen; build it with update_tail=True")


_NO_CLS = ("{} returns one tensor and no cls_pred (the 3-D fine-tuning model: finetune3d.py has no classification branch), so "
           "cls_weight = {} has nothing to weigh; pass cls_weight=0")
_CONST_CLS = ("{} returns a constant cls_pred (zeros, as the reference's UNet does: no classification head and no gradient path), "
              "so cls_weight = {} has nothing to weigh; pass cls_weight=0")


def rollout(model: nn.Module, xx: Tensor, yy: Tensor, msk: Optional[Tensor], T_bundle: int = 1,
            noise_scale: float = 0.0, noise: Optional[List[Tensor]] = None, cls: Optional[Tensor] = None,
            cls_weight: float = 0.0, metrics: Optional[StepMetrics] = None) -> Tuple[Tensor, Tensor]:
    """auto-regressive rollout with summed per-step loss (train_temporal.py:201-219; with a DPOTNet3D and 6-D windows
    [B,X,Y,Z,T,C] the loop of finetune3d.py:206-222 with its own noise rule, ops.noise_dims).  Returns (loss, pred); ``loss``
    is the relative-L2 rollout loss whatever ``cls_weight`` is - ``rollout_total`` also returns the loss to differentiate."""
    return rollout_total(model, xx, yy, msk, T_bundle, noise_scale, noise, cls, cls_weight, metrics)[:2]


def rollout_total(model: nn.Module, xx: Tensor, yy: Tensor, msk: Optional[Tensor], T_bundle: int = 1,
                  noise_scale: float = 0.0, noise: Optional[List[Tensor]] = None, cls: Optional[Tensor] = None,
                  cls_weight: float = 0.0, metrics: Optional[StepMetrics] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """``rollout`` with the dataset-classification branch of train_temporal.py:209-213: cls = the int64 dataset index per
    sample ([B] or [B, 1], as data.DeviceBatcher delivers idx_cls).  Returns (loss, pred, total) with
    total = loss + cls_weight * sum over the AR steps of CrossEntropyLoss(reduction='sum')(cls_pred, cls) when
    cls_weight != 0, else total IS loss: the cross-entropy then runs forward-only for ``metrics`` and cls_head receives no
    gradient.  metrics: a StepMetrics that collects the rollout's scalars (call its ``accumulate`` afterwards).
    A model whose forward returns ONE tensor (DPOTNet3D) has no classification branch: ``cls`` is ignored, and
    cls_weight != 0 raises a ValueError."""
    check_cls_args(None, cls, cls_weight)
    if cls_weight != 0.0 and not getattr(model, "cls_output", True):
        raise ValueError(_NO_CLS.format(type(model).__name__, cls_weight))
    if cls_weight != 0.0 and not getattr(model, "cls_trainable", True):
        raise ValueError(_CONST_CLS.format(type(model).__name__, cls_weight))
    scope = model.weights_scope() if hasattr(model, "weights_scope") else contextlib.nullcontext()
    with scope:
        return _rollout(model, xx, yy, msk, T_bundle, noise_scale, noise, cls, cls_weight, metrics)


def _rollout(model, xx, yy, msk, T_bundle, noise_scale, noise, cls=None, cls_weight=0.0, metrics=None):
    loss = None
    cls_loss = None
    preds = []
    T_ar = yy.shape[-2]
    xx = ops._req(xx.contiguous(), "xx")
    n_steps = len(range(0, T_ar, T_bundle))
    tell = hasattr(model, "_ar_pos")
    want_cls = cls is not None and (cls_weight != 0.0 or metrics is not None)
    if metrics is not None:
        metrics._check_steps(n_steps)
    if want_cls:
        cls = cls.contiguous().view(-1)
    for k, t in enumerate(range(0, T_ar, T_bundle)):
        if tell:
            model._ar_pos = (k, n_steps)            # DPOTNet.recompute_keep_last: which AR steps keep their activations
        y = yy[..., t:t + T_bundle, :]
        if noise_scale != 0.0:
            if noise is None and not xx.requires_grad and xx.numel() % 4 == 0:
                # first AR step of training: nothing to differentiate -> draw the noise inside the kernel
                xx = ops.noise_inject(xx, None, noise_scale)
            else:
                xx = _NoiseFn.apply(xx, noise[k] if noise is not None else None, noise_scale)
        try:
            out = model(xx)
        finally:
            if tell:
                model._ar_pos = None                # (never left behind: a later plain forward must not see a stale position)
        if torch.is_tensor(out):                    # a model without the classification output (DPOTNet3D): labels are ignored
            if cls_weight != 0.0:
                raise ValueError(_NO_CLS.format(type(model).__name__, cls_weight))
            im, cls_pred, want_cls = out, None, False
        else:
            im, cls_pred = out
        if metrics is not None:
            B, Cc = im.shape[0], im.shape[-1]
            l = rel_l2_loss(im, y, msk, metrics.stats_slot(k, B, im.numel() // (B * Cc), Cc))
        else:
            l = rel_l2_loss(im, y, msk)
        loss = l if loss is None else loss + l
        if want_cls:
            slot = metrics.cls_slot(k) if metrics is not None else None
            if cls_weight != 0.0:
                cl, _ = cls_ce_loss(cls_pred, cls, slot)
                cls_loss = cl if cls_loss is None else cls_loss + cl
            else:                                   # an observer: no graph, so HeadFn.backward sees no dcls
                with torch.no_grad():
                    cls_ce_loss(cls_pred.detach(), cls, slot)
        preds.append(im)
        if t + T_bundle < T_ar:
            xx = _SlideFn.apply(xx, im)
    pred = preds[0] if len(preds) == 1 else torch.cat(preds, dim=-2)
    total = loss if cls_loss is None else loss + cls_weight * cls_loss
    if metrics is not None:
        metrics.end_rollout(loss, n_steps, pred.shape[0], pred.shape[-1], n_steps if want_cls else 0)
    return loss, pred, total


class _NoiseFn(torch.autograd.Function):
    """xx + noise_scale * ||xx|| * eps (train_temporal.py:205) for AR steps whose input carries a gradient.  Like
    the reference's autograd, the backward differentiates through the norm as well:
    d/dxx = g + s * xx / ||xx|| * sum(g * eps)  (csrc/loss_opt.hip noise_bwd_*).  eps=None: drawn by the in-kernel
    generator in forward and RE-drawn in backward from a 16-byte copy of the generator state (no eps tensor)."""

    @staticmethod
    def forward(ctx, xx, eps, noise_scale):
        xx = xx.contiguous()
        rng = None
        if eps is None and xx.numel() % 4 != 0:
            eps = torch.randn_like(xx)                      # shapes the in-kernel generator does not cover
        if eps is not None:
            eps = eps.contiguous()
        out, norms = ops.noise_inject(xx, eps, noise_scale, return_norms=True)
        if eps is None:
            rng = ops.rng_state(xx.device).clone()         # {seed, offset} this call drew from
        ctx.save_for_backward(xx, eps if eps is not None else xx.new_empty(0), norms,
                              rng if rng is not None else xx.new_empty(0))
        ctx.noise_scale, ctx.has_eps = noise_scale, eps is not None
        return out

    @staticmethod
    def backward(ctx, g):
        xx, eps, norms, rng = ctx.saved_tensors
        dx = ops.noise_inject_bwd(xx, eps if ctx.has_eps else None, None if ctx.has_eps else rng, g.contiguous(),
                                  norms, ctx.noise_scale)
        return dx, None, None


class _SlideFn(torch.autograd.Function):
    """xx <- cat(xx[..., T_bundle:, :], im) (train_temporal.py:219) as one kernel each way"""

    @staticmethod
    def forward(ctx, xx, im):
        ctx.Tb = im.shape[-2]
        return ops.window_slide(ops._req(xx.contiguous(), "xx"), ops._req(im.contiguous(), "im"))

    @staticmethod
    def backward(ctx, dout):
        dxx, dim = ops.window_slide_bwd(dout.contiguous(), ctx.Tb, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dxx, dim


def train_step(model: nn.Module, opt: FlatOptimizer, xx: Tensor, yy: Tensor, msk: Optional[Tensor], T_bundle: int = 1,
               noise_scale: float = 0.0, lr: Optional[float] = None, reducer=None,
               grad_scale: float = 1.0, cls: Optional[Tensor] = None, cls_weight: float = 0.0,
               metrics: Optional[StepMetrics] = None) -> Tuple[Tensor, Tensor]:
    """one optimisation step; returns (loss, pred) as device tensors - no host sync.  cls / cls_weight / metrics: see
    ``rollout_total`` and ``StepMetrics``; the returned loss stays the relative-L2 rollout loss."""
    check_cls_args(opt, cls, cls_weight)

    def run():
        return rollout_total(model, xx, yy, msk, T_bundle, noise_scale, None, cls, cls_weight, metrics)

    out = _forward_backward(opt, run, reducer)
    _optimise(opt, functools.partial(opt.step, lr), grad_scale, metrics)
    return out


def _forward_backward(opt: FlatOptimizer, run: Callable[[], Tuple[Tensor, Tensor, Tensor]], reducer=None):
    """first half of THE training step, eager or under capture: gradients of ``run()``'s (loss, pred, total) into the zeroed
    flat buffer, reduced over the ranks by a hook-driven ``reducer``; returns (loss, pred) detached"""
    opt.zero_grad()
    if reducer is not None:
        reducer.begin_step()
    loss, pred, total = run()
    total.backward()
    clear_grad_packs()
    if reducer is not None:
        reducer.finish()
    return loss.detach(), pred.detach()


def _optimise(opt: FlatOptimizer, update: Callable[[float], None], grad_scale: float,
              metrics: Optional[StepMetrics]) -> None:
    """second half: the optimiser, then the step's scalars join the device accumulator (the last launch of a step).
    ``update(grad_scale)`` is the optimiser call: ``opt.step`` bound to its lr (stages, then launches) in an eager step,
    ``opt.launch`` where ``opt.stage_hyper`` has run already because it is no part of a capture"""
    update(grad_scale)
    if metrics is not None:
        metrics.accumulate(opt, grad_scale)


@contextlib.contextmanager
def trial_state(opt: FlatOptimizer, metrics: Optional[StepMetrics] = None, rng_device=None, model: Optional[nn.Module] = None):
    """The steps taken inside are NOT training steps (graph warm-up, the trial steps of ``make_dp_step``): parameters,
    optimiser state and the metrics accumulator are put back when the block ends, with ``rng_device`` the in-kernel noise
    generator of that device as well, and with ``model`` the persistent buffers a training-mode forward writes (BatchNorm's
    running_mean / running_var / num_batches_tracked of a UNet); a model without persistent buffers enqueues nothing more.
    A block that raises restores nothing: what raises here is a failed stream capture, and
    the restoring launches must not go to streams that ``_end_stray_captures`` has yet to take out of capture mode."""
    snap = opt.snapshot()
    msnap = metrics.snapshot() if metrics is not None else None
    rng = ops.rng_state(rng_device).clone() if rng_device is not None else None
    bufs = [(b, b.clone()) for b in _persistent_buffers(model)] if model is not None else []
    yield
    opt.restore(snap)
    if msnap is not None:
        metrics.restore(msnap)
    if rng is not None:
        ops.rng_state(rng_device).copy_(rng)
    for b, saved in bufs:
        b.copy_(saved)


def _persistent_buffers(model: nn.Module) -> List[Tensor]:
    """the buffers of ``model`` that are part of its state_dict (a non-persistent one is a constant table, never written)"""
    out = []
    for mod in model.modules():
        out += [b for name, b in mod._buffers.items() if b is not None and name not in mod._non_persistent_buffers_set]
    return out


# ------------------------------------------------------------------------------------------------------
def _retire_collective_watchdog_work(seconds: float = 0.4) -> None:
    """Before a capture that will contain collectives: let the process group's watchdog thread retire the work items of the
    LIVE collectives issued so far (the eager warm-up).  torch's nccl backend keeps every eager collective on a list that its
    watchdog polls (hipEventQuery on the collective's end event, every ~100 ms) until the event has completed; the capture then
    pulls the backend's internal communication stream into capture mode, and HIP refuses a query of an event on a capturing
    stream (hipErrorCapturedEvent) - the watchdog thread throws and the PROCESS aborts.  Seen once in ~10 runs of the one-rank
    RCCL test (round 6).  With the device idle the watchdog needs one of its periods to drop the finished items; there is no
    API to ask it, so: synchronise, then sleep a few periods.  (Inside the capture torch does not enqueue work items at all.)"""
    import time
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return
    torch.cuda.synchronize()
    time.sleep(seconds)


class _GraphStep:
    """What the captured train steps share: static batch buffers, the eager warm-up before the capture, and the replay protocol
    of the weight packs their captured Adam launch writes (``owned``: FusedAdam.wrote at the capture, or None)."""
    owned = None
    cls = None                    # static label buffer (int64, next to xx / yy / msk), or None
    cls_weight = 0.0
    metrics = None

    def _static_batch(self, xx: Tensor, yy: Tensor, msk: Optional[Tensor], cls: Optional[Tensor] = None,
                      cls_weight: float = 0.0, metrics: Optional[StepMetrics] = None) -> None:
        check_cls_args(self.opt, cls, cls_weight)
        self.xx, self.yy = xx.clone(), yy.clone()
        self.msk = msk.clone() if msk is not None else None
        self.cls = cls.clone() if cls is not None else None
        self.cls_weight, self.metrics = cls_weight, metrics

    def stage(self, xx: Tensor, yy: Tensor, msk: Optional[Tensor] = None, cls: Optional[Tensor] = None) -> None:
        self.xx.copy_(xx, non_blocking=True)
        self.yy.copy_(yy, non_blocking=True)
        if msk is not None and self.msk is not None:
            self.msk.copy_(msk, non_blocking=True)
        if cls is not None:
            if self.cls is None:
                raise ValueError("stage(cls=...): this step was built without labels (pass cls= to its constructor)")
            self.cls.copy_(cls.view(self.cls.shape), non_blocking=True)

    def _rollout(self):
        return rollout_total(self.model, self.xx, self.yy, self.msk, self.T_bundle, self.noise_scale, None, self.cls,
                             self.cls_weight, self.metrics)

    def _warm_up(self, n: int, body: Callable[[], None], settle: bool = False) -> None:
        """eager warm-up on a side stream (allocator + lazy inits): ``n`` times what a replay does, stage_hyper then ``body``.
        The warm-up iterations are NOT training steps (a fine-tune of a pretrained checkpoint must not receive unscheduled
        full-lr updates before its first replay), and they are not logged either"""
        with trial_state(self.opt, self.metrics, model=self.model):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(n):
                    self.opt.stage_hyper(self.opt.lr)
                    body()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            if settle:
                _retire_collective_watchdog_work()

    def _replay(self, lr: Optional[float], run: Callable[[], None]) -> Tensor:
        """the graphs hold no pack launch for the set their Adam writes (it was fresh at the capture): refresh it first if
        anything moved the parameters since (load_state_dict, touch()); after the replay its Adam has written it"""
        opt = self.opt
        opt.stage_hyper(lr)
        if self.owned is not None:
            opt.packs.ensure_fresh(self.owned)
        run()
        opt.fp.touch()
        if self.owned is not None:
            opt.packs.mark_fresh(self.owned, opt.fp)
        return self.loss


class GraphedTrainStep(_GraphStep):
    """Captures forward + loss + backward + clip + Adam of a fixed-shape batch into one hipGraph.

    ``stage(xx, yy, msk)`` copies a batch into the static input buffers, ``replay(lr)`` runs the step.  The
    ~500 kernel launches of a DPOT-Tiny step then cost one graph launch instead of ~3 ms of Python/HIP launch
    overhead (the GPU work itself is ~4 ms at B=32)."""

    def __init__(self, model: nn.Module, opt: FlatOptimizer, xx: Tensor, yy: Tensor, msk: Optional[Tensor],
                 T_bundle: int = 1, noise_scale: float = 0.0, warmup: int = 2, reducer=None,
                 grad_scale: float = 1.0, capture_collectives: bool = False, cls: Optional[Tensor] = None,
                 cls_weight: float = 0.0, metrics: Optional[StepMetrics] = None):
        self.model, self.opt = model, opt
        self._static_batch(xx, yy, msk, cls, cls_weight, metrics)
        if reducer is not None and getattr(reducer, "world", 1) > 1 and not capture_collectives:
            raise ValueError("GraphedTrainStep captures the WHOLE step into one graph; pass capture_collectives=True to "
                             "capture the bucket all-reduces with it, or use SegmentedTrainStep (collectives between graphs)")
        # capture_collectives (opt-in): the hook-driven bucket all-reduces are issued INSIDE the capture - the reducer's side
        # stream forks from / joins the capturing stream, RCCL's kernels become nodes of the one graph; no cut in the
        # autograd graph, no graph launches between the buckets
        self.reducer = reducer if capture_collectives else None
        if self.reducer is not None:
            if grad_scale != 1.0 and grad_scale != self.reducer.grad_scale:
                raise ValueError(f"GraphedTrainStep(capture_collectives=True) scales the gradient by the reducer's 1 / world = "
                                 f"{self.reducer.grad_scale}; a different grad_scale ({grad_scale}) was passed")
            grad_scale = self.reducer.grad_scale
            # the capture bakes in WHICH buckets are all-reduced: always include the cls_head tail (a zero slice when the loss
            # ignores it - the SUM of zeros - so the replayed graph stays right if the head starts to receive gradients later)
            self.reducer.skip_zero_tail = False
        self.grad_scale = grad_scale
        self.T_bundle, self.noise_scale = T_bundle, noise_scale
        self._warm_up(warmup, self._body, settle=self.reducer is not None)
        self.graph = torch.cuda.CUDAGraph()
        opt.zero_grad()
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.loss, self.pred = self._body()
        self.owned = opt.wrote
        self.warmup_steps = warmup

    def _body(self):
        out = _forward_backward(self.opt, self._rollout, self.reducer)
        _optimise(self.opt, self.opt.launch, self.grad_scale, self.metrics)
        return out

    def replay(self, lr: Optional[float] = None) -> Tensor:
        return self._replay(lr, self.graph.replay)


class SegmentedTrainStep(_GraphStep):
    """The data-parallel train step (any T_ar, as train_temporal_parallel.py:214-244 runs it under DDP) as a CHAIN of
    hipGraphs, cut where a gradient bucket becomes final, so that the RCCL all-reduce of bucket k runs on the reducer's side stream while the compute stream
    replays the backward of the earlier stages - the overlap torch-DDP gets from autograd hooks
    (train_temporal_parallel.py:244), without a collective inside a capture and without eager launch overhead.

        segment 0      zero_grad, forward, loss, backward of [out layer .. first stage of the LAST bucket]
        segment j      backward of the stages of the j-th bucket from the end
        optimiser      ||g||^2 + fused clip + Adam          (after the compute stream has joined the side stream)

    The autograd graph is cut at the bucket boundaries (``DPOTNet._boundary_hook``): each cut replaces the latent by a
    detached leaf; the next segment continues with ``out.backward(leaf.grad)``.  All segments share one memory pool
    and are always replayed in capture order.

    Auto-regressive rollouts (T_ar > T_bundle): every AR step adds to every parameter gradient, and the backward visits
    the AR steps last to first - a bucket is final only once the backward of the FIRST AR step has passed it.  The cuts
    are therefore made in the first forward call only; segment 0 holds the whole rollout forward, the loss, the complete
    backward of AR steps T-1 .. 1 and the backward of AR step 0 down to its last cut."""

    def __init__(self, model: nn.Module, opt: FlatOptimizer, reducer, xx: Tensor, yy: Tensor, msk: Optional[Tensor],
                 noise_scale: float = 0.0, warmup: int = 2, T_bundle: int = 1, cls: Optional[Tensor] = None,
                 cls_weight: float = 0.0, metrics: Optional[StepMetrics] = None):
        self.T_bundle = T_bundle
        self.model, self.opt, self.reducer = model, opt, reducer
        self._static_batch(xx, yy, msk, cls, cls_weight, metrics)
        self.noise_scale = noise_scale
        self.grad_scale = reducer.grad_scale
        depth = len(model.blocks)
        norm = lambda st: depth + 1 if st == 10 ** 6 else st          # stage number -> boundary index
        # buckets in backward order (tail excluded); a bucket whose first stage is b > 0 needs a cut at boundary b
        self.bwd_buckets = [k for k in range(reducer.n_buckets - 1, -1, -1) if k != reducer.tail_bucket]
        self.cut_at = sorted({norm(reducer.first_stage_of_bucket(k)) for k in self.bwd_buckets} - {0})

        def eager_step():
            for fn in self._segment_fns():
                fn()
            _optimise(opt, opt.launch, self.grad_scale, metrics)

        reducer.detach()
        try:
            self._warm_up(warmup, eager_step)
            self.graphs: List[torch.cuda.CUDAGraph] = []
            pool = torch.cuda.graph_pool_handle()
            for fn in self._segment_fns():
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
                    fn()
                self.graphs.append(g)
            self.opt_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.opt_graph, pool=pool, capture_error_mode="thread_local"):
                _optimise(opt, opt.launch, self.grad_scale, metrics)          # the last segment
            self.owned = opt.wrote
        finally:
            reducer.attach()
            model._boundary_hook = None
        self.tail_has_grad = reducer.tail_bucket >= 0 and any(opt.fp.filled[i]
                                                              for i in reducer.members[reducer.tail_bucket])
        assert len(self.graphs) == len(self.bwd_buckets), (len(self.graphs), self.bwd_buckets)

    def _segment_fns(self):
        """generator of the segment bodies; segment j+1 may only be built after segment j has run"""
        cuts = []
        cut_at = set(self.cut_at)
        calls = [0]                                  # forward calls of this rollout seen so far (hook(1, .) opens one)

        def hook(b, lat):
            if b == 1:
                calls[0] += 1
            if calls[0] == 1 and b in cut_at and lat.requires_grad:
                leaf = lat.detach().requires_grad_(True)
                cuts.append((lat, leaf))
                return leaf
            return lat

        def cut_rollout():
            self.model._boundary_hook = hook
            calls[0] = 0
            try:
                out = self._rollout()
            finally:
                self.model._boundary_hook = None
            assert len(cuts) == len(self.cut_at), f"expected {len(self.cut_at)} graph cuts, the forward made {len(cuts)}"
            return out

        def first():
            self.loss, self.pred = _forward_backward(self.opt, cut_rollout)

        yield first
        # one further segment per cut, from the last cut to the first
        n = len(self.cut_at)
        for j in range(n - 1, -1, -1):
            def seg(j=j):
                out, leaf = cuts[j]
                out.backward(leaf.grad)
                clear_grad_packs()
                leaf.grad = None
            yield seg

    def replay(self, lr: Optional[float] = None) -> Tensor:
        return self._replay(lr, self._run)

    def _run(self) -> None:
        red = self.reducer
        red.begin_step()
        for g, k in zip(self.graphs, self.bwd_buckets):
            g.replay()
            red.reduce_bucket(k)              # side stream waits for the compute stream, then all-reduces bucket k
        if self.tail_has_grad:
            red.reduce_bucket(red.tail_bucket)
        elif red.tail_bucket >= 0:
            red._launched[red.tail_bucket] = True
        red.finish()                          # compute stream joins the side stream
        self.opt_graph.replay()


# ------------------------------------------------------------------------------------------------------
def _grad_checksum(g: Tensor) -> Tensor:
    """order-independent 64-bit checksum of the BIT patterns of a flat fp32 buffer (int64[2]: sum and sum of squares of the
    words mod 2^64) - equal buffers give equal checksums; used across ranks (after an all-reduce every rank must hold the same
    gradient bit for bit)"""
    w = g.view(torch.int32).to(torch.int64)
    return torch.stack([w.sum(), (w * w).sum()])


def _end_stray_captures(streams) -> None:
    """best effort after a FAILED stream capture: a stream that joined the capture (the reducer's side stream) can be left in
    capture mode when the capture is torn down by an exception; end it through the HIP runtime and clear the sticky error"""
    import ctypes
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        return
    for st in streams:
        if st is None:
            continue
        g = ctypes.c_void_p()
        hip.hipStreamEndCapture(ctypes.c_void_p(st.cuda_stream), ctypes.byref(g))
        if g.value:
            hip.hipGraphDestroy(g)
    hip.hipGetLastError()
    try:
        torch.cuda.synchronize()
    except Exception:                                          # pragma: no cover
        pass


def make_dp_step(model: nn.Module, opt: FlatOptimizer, reducer, xx: Tensor, yy: Tensor, msk: Optional[Tensor],
                 noise_scale: float = 0.0, warmup: int = 2, T_bundle: int = 1, try_one_graph: bool = True,
                 cls: Optional[Tensor] = None, cls_weight: float = 0.0, metrics: Optional[StepMetrics] = None):
    """The N > 1 train step with the FAST mode chosen by verification (round 6): returns (step, info).

    Fast mode = ``GraphedTrainStep(capture_collectives=True)``: the whole step, bucket all-reduces included, as ONE hipGraph
    (+0.4 % over the single-GPU graph at DPOT-Tiny against +4 % for the chain).  Fallback = ``SegmentedTrainStep`` (graph
    segments, the all-reduces issued between them: collectives never sit inside a capture).  Whether the communication
    library's kernels replay correctly as graph nodes across ranks cannot be known in advance, so the one-graph step is
    captured and ONE trial step is run twice from the same snapshot (parameters, Adam state, noise generator): eagerly with the
    hook-driven reducer (``train_step`` - the same kernels in the same order, collectives issued live) and as a replay of the
    graph.  The reduced flat gradient must agree BIT FOR BIT between the two and across the ranks (checksums through the process
    group); only then is the one-graph step returned, otherwise the segmented chain is built and ``info`` says why.  (The chain
    itself is not the reference of the comparison: with the bf16 channel MLP its graph cuts change which kernel packs a
    Block's incoming gradient, and six bias gradients differ in the last bit - tests/test_gpu_train2.py.)  Parameters,
    optimiser state and the noise generator are left exactly as found.  Mirrors train_temporal_parallel.py:102,185,243-244."""
    import torch.distributed as dist

    def chain(why):
        reducer.skip_zero_tail = tail_flag
        seg = SegmentedTrainStep(model, opt, reducer, xx, yy, msk, noise_scale=noise_scale, warmup=warmup, T_bundle=T_bundle,
                                 cls=cls, cls_weight=cls_weight, metrics=metrics)
        return seg, {"mode": "segmented", "why": why}

    tail_flag = reducer.skip_zero_tail
    if not try_one_graph:
        return chain("one-graph mode not tried")
    multi = dist.is_available() and dist.is_initialized()
    backend = dist.get_backend(reducer.pg) if multi else "none"
    if multi and backend != "nccl":
        # only RCCL's collectives are device work that a stream capture can record; a gloo collective synchronises the stream
        # from the host - attempting the capture would leave the streams that joined it in a broken capture state
        return chain(f"one-graph capture failed: backend '{backend}' collectives cannot be recorded in a hipGraph (RCCL only)")
    one, err = None, None
    try:
        with trial_state(opt, metrics, xx.device):
            one = GraphedTrainStep(model, opt, xx, yy, msk, T_bundle=T_bundle, noise_scale=noise_scale,
                                   warmup=max(1, warmup), reducer=reducer, capture_collectives=True, cls=cls,
                                   cls_weight=cls_weight, metrics=metrics)
    except Exception as e:                                    # an RCCL build / driver that cannot capture its collectives
        err = f"{type(e).__name__}: {e}"[:160]
        _end_stray_captures([torch.cuda.current_stream(), reducer.stream])
    # every rank must take the same branch: agree on whether the capture worked everywhere
    ok = torch.tensor([1 if one is not None else 0], device=xx.device, dtype=torch.int64)
    if multi:
        dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=reducer.pg)
    if int(ok.item()) == 0:
        del one
        return chain("one-graph capture failed" + (f" here ({err})" if err else " on another rank"))
    grads = []
    for mode in ("eager", "graph"):
        with trial_state(opt, metrics, xx.device):            # both from the same state, which is left as found
            reducer.skip_zero_tail = False                    # (as the capture: the cls_head tail is always reduced)
            if mode == "eager":
                train_step(model, opt, one.xx, one.yy, one.msk, T_bundle=T_bundle, noise_scale=noise_scale, lr=opt.lr,
                           reducer=reducer, grad_scale=reducer.grad_scale, cls=one.cls, cls_weight=cls_weight, metrics=metrics)
            else:
                one.replay(opt.lr)
            torch.cuda.synchronize()
            grads.append(opt.fp.grad[:opt.n_active].clone())
    same_modes = bool(torch.equal(grads[0], grads[1]))
    cs = _grad_checksum(grads[1])
    verdict = torch.tensor([1 if same_modes else 0], device=xx.device, dtype=torch.int64)
    same_ranks = True
    if multi:
        lo, hi = cs.clone(), cs.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=reducer.pg)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=reducer.pg)
        same_ranks = bool(torch.equal(lo, hi))
        dist.all_reduce(verdict, op=dist.ReduceOp.MIN, group=reducer.pg)
    if int(verdict.item()) == 1 and same_ranks:
        return one, {"mode": "one-graph", "why": "reduced gradient of a trial step bit-identical to the eager hook-driven step's "
                                                  "and across the ranks"}
    del one
    return chain("one-graph trial step " + ("differs from the eager step's gradient" if int(verdict.item()) == 0 else
                                            "gave different gradients on different ranks"))
