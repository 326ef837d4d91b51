"""Checkpoint loading and auto-regressive inference for the MI355X DPOTNet.

* ``load_model_from_checkpoint`` / ``load_components_from_pretrained`` - the contracts of the reference's
  utils/utilities.py:99-166 (``module.`` prefix of DDP checkpoints stripped; fine-tuning may take only some
  components from a pretrained state_dict), written against the same sub-module names, so a pretrained ``.pth``
  (``torch.load(path)['model']``, README.md:30) loads unchanged.
* ``load_3d_components_from_2d`` - utils/utilities.py:170-207: the blocks and the time aggregator of a pretrained 2-D
  checkpoint into a ``DPOTNet3D`` (the 3-D fine-tuning path of finetune3d.py).
* ``rollout_eval`` / ``GraphedRollout`` - the no-grad rollout of evaluate.py:183-222: the model's own prediction is
  appended to the input window step after step; returns the prediction, the per-step loss sum and the loss of the
  whole trajectory (both SimpleLpLoss(size_average=False)).  With fixed shapes the single forward step is one
  hipGraph that is replayed T_ar / T_bundle times (the window slide writes into the graph's static input).
* ``refill_mask`` and ``model_res=`` - the resolution-generalisation rollout of evaluate_varyingres.py:198-248: data on
  a res x res grid runs through a model built for another resolution; every AR step Fourier-resizes the window up to the
  model's resolution (ops.spectral_resize, one launch) and the prediction back down.
* ``RolloutEvaluator`` - the reference's second evaluation tool, utils/criterion.py:189-239 ``Evaluator(temporal=True,
  griddata=True, component='all')``: per-channel and per-step normalised errors, the boundary error and the error spectrum
  in three wavenumber bands, accumulated on the device (csrc/evalmetrics.hip); ``evaluator=`` hands every rollout to it.
  3-D rollouts [B, X, Y, Z, T, C] take the same keys, column c being ``Evaluator(..., component=c)`` (csrc/evalmetrics3d.hip).
* ``Resized3D`` - the resolution-generalisation rollout in 3-D: a wrapper that Fourier-resizes a 6-D window up to the wrapped
  model's resolution (ops.spectral_resize3), runs the model there and resizes the prediction back, so that ``rollout_eval``
  and ``GraphedRollout`` take it as any 3-D model.  ``model_res=`` itself stays a keyword of 2-D windows.
"""
from __future__ import annotations

import contextlib
import warnings
from collections import OrderedDict
from typing import Dict, Iterable, Mapping, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import _lib, ops
from .functional import rel_l2_loss

Tensor = torch.Tensor
COMPONENTS = ("patch_embed", "pos", "blocks", "time_agg", "cls_head", "scale_feats", "out")


def _plain_state_dict(sd: Union[str, Mapping]) -> "OrderedDict[str, Tensor]":
    """accepts a path, a checkpoint dict with a 'model' entry, or a state_dict; strips DDP's 'module.' prefix"""
    if isinstance(sd, (str, bytes)):
        sd = torch.load(sd, map_location="cpu", weights_only=False)
    if "model" in sd and isinstance(sd["model"], Mapping) and not isinstance(sd["model"], Tensor):
        sd = sd["model"]
    if len(sd) and next(iter(sd.keys())).startswith("module."):
        sd = OrderedDict((k.replace("module.", ""), v) for k, v in sd.items())
    return OrderedDict(sd)


def load_model_from_checkpoint(model: nn.Module, model_state_dict: Union[str, Mapping]) -> None:
    """utils/utilities.py:99-109"""
    model.load_state_dict(_plain_state_dict(model_state_dict))


def _sub(sd: Mapping[str, Tensor], prefix: str) -> "OrderedDict[str, Tensor]":
    return OrderedDict((k[len(prefix):], v) for k, v in sd.items() if k.startswith(prefix))


def load_components_from_pretrained(model: nn.Module, state_dict: Union[str, Mapping],
                                    components: Union[str, Iterable[str]] = "all") -> None:
    """utils/utilities.py:112-166: components = 'all' or a subset of COMPONENTS.  Must run BEFORE the optimiser's
    FlatParams is built (the reference replaces the pos_embed Parameter object; here its data is copied in place so
    that even an existing flat binding stays valid)."""
    sd = _plain_state_dict(state_dict)
    if components == "all" or "all" in components:
        model.load_state_dict(sd)
        return
    for name in components:
        if name == "patch_embed" and hasattr(model, "patch_embed"):
            model.patch_embed.load_state_dict(_sub(sd, "patch_embed."))
        elif name == "pos" and hasattr(model, "pos_embed"):
            with torch.no_grad():
                src = sd["pos_embed"]
                if tuple(src.shape) != tuple(model.pos_embed.shape):
                    raise RuntimeError(f"pos_embed shape {tuple(src.shape)} != {tuple(model.pos_embed.shape)}")
                model.pos_embed.copy_(src)
        elif name == "blocks" and hasattr(model, "blocks"):
            for i, block in enumerate(model.blocks):
                block.load_state_dict(_sub(sd, f"blocks.{i}."))
        elif name == "scale_feats" and hasattr(model, "scale_feats_mu"):
            model.scale_feats_mu.load_state_dict(_sub(sd, "scale_feats_mu."))
            model.scale_feats_sigma.load_state_dict(_sub(sd, "scale_feats_sigma."))
        elif name == "cls_head" and hasattr(model, "cls_head"):
            model.cls_head.load_state_dict(_sub(sd, "cls_head."))
        elif name == "time_agg" and hasattr(model, "time_agg_layer"):
            model.time_agg_layer.load_state_dict(_sub(sd, "time_agg_layer."))
        elif name == "out" and hasattr(model, "out_layer"):
            model.out_layer.load_state_dict(_sub(sd, "out_layer."))
        elif name in COMPONENTS:
            # utils/utilities.py:163 prints 'Submodule does not exists' and carries on: fine-tune configs list e.g.
            # 'scale_feats' for models built with normalize=False
            warnings.warn(f"load_components_from_pretrained: this model has no {name!r} component - skipped")
        else:
            raise KeyError(f"unknown component {name!r} (known: {COMPONENTS})")


def load_3d_components_from_2d(model: nn.Module, state_dict: Union[str, Mapping],
                               components: Union[str, Iterable[str]] = "all") -> None:
    """utils/utilities.py:170-207: a DPOTNet3D takes components of a pretrained 2-D checkpoint.  'all' loads the whole state
    dict (it must then be a 3-D one), 'blocks' copies every block - the 1 x 1 Conv2d weights of the channel MLP (keys holding
    both 'mlp' and 'weight') gain a trailing axis and become Conv3d weights - and 'time_agg' the time aggregator; any other
    name is reported and skipped, as the reference prints 'Submodule does not exists' and carries on.  Values are copied in
    place (load_state_dict), so an existing FlatParams binding stays valid."""
    sd = _plain_state_dict(state_dict)
    if components == "all" or "all" in components:
        model.load_state_dict(sd)
        return
    for name in components:
        if name == "blocks" and hasattr(model, "blocks"):
            for i, block in enumerate(model.blocks):
                bsd = _sub(sd, f"blocks.{i}.")
                for k, v in bsd.items():
                    if "mlp" in k and "weight" in k:
                        bsd[k] = v.unsqueeze(-1)                  # Conv2d [o, i, 1, 1] -> Conv3d [o, i, 1, 1, 1]
                block.load_state_dict(bsd)
        elif name == "time_agg" and hasattr(model, "time_agg_layer"):
            model.time_agg_layer.load_state_dict(_sub(sd, "time_agg_layer."))
        else:
            warnings.warn(f"load_3d_components_from_2d: component {name!r} is not one a 3-D model takes from a 2-D checkpoint "
                          "('blocks', 'time_agg') or this model does not have it - skipped")


# ------------------------------------------------------------------------------------------------------
def _size2(res) -> Tuple[int, int]:
    return ops.size_tuple(res, 2)


def refill_mask(msk: Tensor, res) -> Tensor:
    """evaluate_varyingres.py:198-201: the mask of resized data [B, res, res, 1, C] - a channel of a sample is 1 everywhere
    if the original mask has any non-zero entry in it, else 0.  `res` is one int or (res_x, res_y)."""
    rx, ry = _size2(res)
    nonzero = (msk.sum(dim=(1, 2, 3)) > 0)[:, None, None, None, :]
    return nonzero.to(torch.float32).expand(msk.shape[0], rx, ry, 1, msk.shape[-1]).contiguous()


class RolloutEvaluator:
    """The metric set of the reference's ``Evaluator(temporal=True, griddata=True, component='all')`` (utils/criterion.py:
    189-239 and compute_fourier_error, :246-360), kept on the DEVICE and accumulated over batches.  ``update(pred, target)``
    enqueues two launches and never synchronises; ``read()`` is the only call that does.  After ``update`` on the batches
    B1, B2, ... ``read()`` equals the reference's Evaluator called once on their concatenation: every metric is a mean over
    the samples of a per-sample value (or, for the spectrum, the root of such a mean), so the accumulator holds sums over
    the samples and the sample count.

    What is computed, with e = pred - target formed in fp32 (also BEFORE the transform: the DFT is linear, and the
    difference of two nearly equal spectra cancels in fp32 where the spectrum of the difference does not):

    * ``nmae, nmse, nmxe`` [1, C]: per sample and channel, over all of X*Y*T: sum|e| / sum|target|,
      sqrt(sum e^2 / sum target^2), max|e| / max|target|; then the mean over the samples.
    * ``nmae_t, nmse_t, nmxe_t`` [1, T, C]: the same per time step, over X*Y.
    * ``bdmse`` **[C, T]**: e^2 summed over the rows x = 0, nx-1 (all y) and the columns y = 0, ny-1 (all x) - the four
      corners counted twice - divided by 2 nx + 2 ny, root, mean over the samples.  An absolute error (no target norm), and
      the one key the reference returns channel-major (untransposed); kept so.
    * ``fmse_low, fmse_mid, fmse_high`` [T, C]: |DFT2(e)|^2 (unnormalised forward transform) over the positive quadrant
      0 <= i < nx//2, 0 <= j < ny//2 only, summed over the shells floor(sqrt(i^2 + j^2)) < K = min(nx//2, ny//2) (larger
      shells are dropped); per shell sqrt(mean over the samples) / (nx ny); then the mean over the shells [0, ilow),
      [ilow, ihigh), [ihigh, K).  An empty band (K <= ihigh, e.g. 16 x 16 with the defaults) is NaN, as in the reference.
    * ``samples``: the number of samples seen.

    A channel whose target is identically zero divides by a zero norm: inf or NaN, as IEEE arithmetic and the reference give;
    nothing is counted specially.  There is no mask, no normalizer and no single-component mode.  All batches between two
    ``reset()`` share X, Y, T, C (T <= T_max, C == n_channels); the batch size may change.  X <= 1024, Y <= 304 (the LDS
    intermediate of a workgroup).  ``update`` is capturable in a hipGraph once a shape has been seen.

    3-D fields: ``update`` also takes a pair [B, X, Y, Z, T, C] (csrc/evalmetrics3d.hip); ops takes the rank from the shape.  The
    reference's Evaluator cannot run ``component='all'`` on such a field; column c of every key is its
    ``Evaluator(temporal=True, griddata=True, component=c)(pred[..., c], target)``, in the shapes above: the ratios over all of
    X*Y*Z*T and, per step, over X*Y*Z; ``bdmse`` is e^2 summed over the six faces x = 0, X-1, y = 0, Y-1, z = 0, Z-1 (an edge
    counted twice, a corner three times) over 2 XY + 2 YZ + 2 ZX; ``fmse_*`` is |DFT3(e)|^2 over the positive octant summed
    over the shells floor(sqrt(i^2 + j^2 + k^2)) < K = min(X//2, Y//2, Z//2), per shell sqrt(mean over the samples) / (X Y Z).
    X, Y, Z <= 512 each.  The batches between two ``reset()`` share the rank as well as the shape."""

    def __init__(self, device, n_channels: int, T_max: int, ilow: int = 4, ihigh: int = 12):
        if n_channels < 1 or T_max < 1:
            raise ValueError(f"RolloutEvaluator: n_channels and T_max must be >= 1, got {n_channels}, {T_max}")
        if not 0 <= ilow <= ihigh:
            raise ValueError(f"RolloutEvaluator: need 0 <= ilow <= ihigh, got {ilow}, {ihigh}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DpotHipError(f"RolloutEvaluator must live on the MI355X (got device {self.device}): dpot_amd has no "
                                    "CPU path")
        self.C, self.T_max, self.ilow, self.ihigh = int(n_channels), int(T_max), int(ilow), int(ihigh)
        self.shape: Optional[Tuple[int, ...]] = None                   # (X, Y[, Z], T, C) of the batches since reset()
        self.acc: Optional[Tensor] = None
        self._accs: Dict[Tuple[int, ...], Tensor] = {}                  # one accumulator per shape ever seen: no re-allocation

    def update(self, pred: Tensor, target: Tensor) -> None:
        """fold one batch in: pred, target [B, X, Y, T, C] or [B, X, Y, Z, T, C] fp32 contiguous on the GPU.  No
        synchronisation."""
        if pred.dim() not in (5, 6) or pred.shape != target.shape:
            raise _lib.DpotHipError(f"RolloutEvaluator.update: pred and target must be [B, X, Y, T, C] or [B, X, Y, Z, T, C] "
                                    f"of one shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
        shape = tuple(int(s) for s in pred.shape[1:])
        if shape[-1] != self.C or shape[-2] > self.T_max:
            raise _lib.DpotHipError(f"RolloutEvaluator was built for {self.C} channels and T <= {self.T_max}, got "
                                    f"{tuple(pred.shape)}")
        if self.shape is not None and shape != self.shape:
            raise _lib.DpotHipError(f"RolloutEvaluator: the batches between two reset() must share X, Y, T, C (and the rank): "
                                    f"{self.shape} so far, now {shape}")
        if not (pred.is_cuda and target.is_cuda):
            raise _lib.DpotHipError(f"RolloutEvaluator.update: pred and target must live on the MI355X (got {pred.device}, "
                                    f"{target.device}): dpot_amd has no CPU path")
        if self.shape is None:
            acc = self._accs.get(shape)
            if acc is None:
                if torch.cuda.is_current_stream_capturing():
                    raise _lib.DpotHipError("RolloutEvaluator: the accumulator of a shape is allocated when it is first seen - "
                                            "run one update (and reset) before capturing")
                acc = self._accs[shape] = ops.eval_acc_alloc(*shape, self.device)
            self.acc = acc
        ops.eval_metrics_update(pred, target, self.acc)
        self.shape = shape

    def reset(self) -> None:
        """zero the accumulator by a launch (no synchronisation); the next update may bring another shape"""
        if self.acc is not None:
            self.acc.zero_()
        self.shape = None

    def read(self, group=None) -> Dict[str, object]:
        """the ONLY call that synchronises: the reference's ten keys as float32 numpy arrays in the reference's shapes (see
        the class docstring; ``bdmse`` is [C, T]) plus ``samples``.  The accumulator is left as it is.  ``group``: a
        dp.BucketedGradReducer or a process group - the sums are added over the ranks with ONE all-reduce first."""
        if self.shape is None:
            raise _lib.DpotHipError("RolloutEvaluator.read: no update since the last reset")
        vals = torch.cat([self.acc[:1].to(torch.float64), self.acc[1:].view(torch.float64)])
        if group is not None:
            import torch.distributed as dist
            pg = getattr(group, "pg", group) if not isinstance(group, bool) else None
            if dist.is_available() and dist.is_initialized():
                dist.all_reduce(vals, op=dist.ReduceOp.SUM, group=pg)
        vals = vals.cpu().numpy()
        return ops.eval_finish(vals, int(round(vals[0])), *self.shape, self.ilow, self.ihigh)


@contextlib.contextmanager
def _eval_mode(model: nn.Module):
    """THE place the evaluation paths (rollout_eval, GraphedRollout's capture) switch the model to eval mode - a UNet's BatchNorm
    then reads its running statistics and writes nothing - and put its mode back as they found it, also when the block raises"""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


@torch.no_grad()
def rollout_eval(model: nn.Module, xx: Tensor, yy: Tensor, msk: Optional[Tensor], T_bundle: int = 1,
                 step=None, metrics=None, model_res=None, evaluator=None) -> Tuple[Tensor, Tensor, Tensor]:
    """evaluate.py:193-213; with a DPOTNet3D and 6-D windows [B,X,Y,Z,T,C] the test loop of finetune3d.py:252-278.
    Returns (pred [B,X,Y,T_ar,C], sum of the per-step losses, loss of the whole rollout).
    `step(xx) -> im` defaults to the model's forward (a GraphedRollout passes its graph replay).
    metrics: a train.StepMetrics - the test loop's test_l2_step / test_l2_full (train_temporal.py:252-281) are accumulated
    on the device (one launch per rollout, no synchronisation; `metrics.read()` at the end of the loop), and the loss of the
    whole rollout is formed from the statistics the per-step losses left (ops.rel_l2_combine) instead of a second pass over
    the concatenated fields - equal to the two-pass value at the parity tolerance (tests/test_gpu_metrics.py), not bit for
    bit: without `metrics` the returned value stays on the two-pass path.
    model_res (an int or (res_x, res_y)): evaluate_varyingres.py:228-248 - xx, yy and msk live at the DATA resolution; every
    step Fourier-resizes the window to model_res, runs the model there and resizes the prediction back; loss, metrics and
    the window slide stay at the data resolution.  As in the reference the two resizes also run when model_res equals the
    data resolution (every frequency is kept then: the identity up to rounding).  None: no resize is enqueued.
    evaluator: a RolloutEvaluator - `evaluator.update(pred, yy)` runs on the assembled prediction at the DATA resolution, on
    the same stream, without a synchronisation; the returned values are untouched by it.  None: nothing is enqueued.
    6-D windows take `evaluator=` as well - a RolloutEvaluator, anything else is a ValueError before the rollout starts;
    `model_res=` does not exist for them: a 3-D model is evaluated at another data resolution by wrapping it, Resized3D."""
    # weight-only products (packed AFNO weights, folded embed matrices, ...) once per rollout, not once per AR step
    scope = model.weights_scope() if (step is None and hasattr(model, "weights_scope")) else contextlib.nullcontext()
    def forward(x):                      # DPOTNet returns (pred, cls_pred), DPOTNet3D the prediction alone
        out = model(x)
        return out if torch.is_tensor(out) else out[0]

    step = step or forward
    if xx.dim() == 6 and model_res is not None:
        # the test loop of finetune3d.py:252-278 has no resize; model_res= drives the 2-D kernel, Resized3D wraps a 3-D model
        raise ValueError(f"rollout_eval: model_res= exists for 2-D windows [B,X,Y,T,C] only, got a 6-D window "
                         f"{tuple(xx.shape)}")
    if xx.dim() == 6 and evaluator is not None and not isinstance(evaluator, RolloutEvaluator):
        # a 6-D prediction goes to RolloutEvaluator's 3-D kernels; any other object with an update() was written for
        # [B,X,Y,T,C], and failing before the rollout beats failing (or mis-reading the rank) after it
        raise ValueError(f"rollout_eval: a 6-D window {tuple(xx.shape)} needs a RolloutEvaluator as evaluator=; "
                         f"a {type(evaluator).__name__} is taken for 2-D windows [B,X,Y,T,C] only")
    T_ar = yy.shape[-2]
    loss_steps = None
    preds = []
    xx = xx.contiguous()
    n_steps = len(range(0, T_ar, T_bundle))
    if metrics is not None:
        metrics._check_steps(n_steps)
    if model_res is not None:
        model_res, data_res = _size2(model_res), (xx.shape[1], xx.shape[2])
    with scope, _eval_mode(model):
        for k, t in enumerate(range(0, T_ar, T_bundle)):
            y = yy[..., t:t + T_bundle, :]
            if model_res is None:
                im = step(xx)
            else:
                im = ops.spectral_resize(step(ops.spectral_resize(xx, model_res)).contiguous(), data_res)
            slot = None
            if metrics is not None:
                B, Cc = im.shape[0], im.shape[-1]
                slot = metrics.stats_slot(k, B, im.numel() // (B * Cc), Cc)
            l = rel_l2_loss(im, y.contiguous(), msk, slot)
            loss_steps = l if loss_steps is None else loss_steps + l
            preds.append(im)
            if t + T_bundle < T_ar:
                xx = ops.window_slide(xx, im.contiguous())               # xx[..., T_bundle:, :] ++ im, one kernel
    pred = preds[0] if len(preds) == 1 else torch.cat(preds, dim=-2)
    if evaluator is not None:
        evaluator.update(pred.contiguous(), yy.contiguous())
    if metrics is not None:
        metrics.end_rollout(loss_steps, n_steps, pred.shape[0], pred.shape[-1], 0)
        metrics.accumulate()
        return pred, loss_steps, metrics.l2_full.clone().view(())
    loss_full = rel_l2_loss(pred.contiguous(), yy.contiguous(), msk)
    return pred, loss_steps, loss_full


class Resized3D(nn.Module):
    """A 3-D model evaluated at any data resolution: forward on a window [B, X, Y, Z, T, C] is ops.spectral_resize3 up (or
    down) to `model_res`, the wrapped model, and ops.spectral_resize3 of its prediction back to (X, Y, Z) - the 3-D form of
    the loop body of evaluate_varyingres.py:228-248.  Returns one tensor, as DPOTNet3D and FNO3d do.  No parameters of its own.
    rollout_eval and GraphedRollout take it as any 3-D model (metrics= and evaluator= included), so loss, metrics and the
    window slide run at the DATA resolution; a GraphedRollout of it is captured at the data resolution with both resizes
    inside the graph, and its warm-up builds the two resize plans.  As in the reference's 2-D loop, `model_res` equal to the
    data resolution still resizes (the identity up to rounding).  model_res: one int or (res_x, res_y, res_z)."""

    def __init__(self, model: nn.Module, model_res):
        super().__init__()
        self.model = model
        self.model_res = ops.size_tuple(model_res, 3, strict=True)
        if self.model_res is None:
            raise ValueError(f"Resized3D: model_res must be one int or (res_x, res_y, res_z), got {model_res!r}")

    def weights_scope(self):
        """the wrapped model's weight-only products once per rollout (rollout_eval), where it has them"""
        return self.model.weights_scope() if hasattr(self.model, "weights_scope") else contextlib.nullcontext()

    def forward(self, xx: Tensor) -> Tensor:
        if xx.dim() != 6:
            raise ValueError(f"Resized3D: needs a 6-D window [B, X, Y, Z, T, C], got {tuple(xx.shape)}")
        data_res = tuple(xx.shape[1:4])
        out = self.model(ops.spectral_resize3(xx.contiguous(), self.model_res))
        out = out if torch.is_tensor(out) else out[0]
        return ops.spectral_resize3(out.contiguous(), data_res)


class GraphedRollout:
    """One hipGraph of the forward step for a fixed input shape, replayed for every AR step.  The model's forward returns
    (pred, cls_pred) as DPOTNet does, or the prediction alone as DPOTNet3D does (`cls` is then None)."""

    def __init__(self, model: nn.Module, example_xx: Tensor):
        self.model = model
        self.x = example_xx.detach().clone().contiguous()
        with torch.no_grad(), _eval_mode(model):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    model(self.x)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                out = model(self.x)
        self.im, self.cls = (out, None) if torch.is_tensor(out) else (out[0], out[1])

    def step(self, xx: Tensor) -> Tensor:
        self.x.copy_(xx)
        self.graph.replay()
        return self.im.clone()          # the graph's output buffer is overwritten by the next replay

    def __call__(self, xx: Tensor, yy: Tensor, msk: Optional[Tensor], T_bundle: int = 1, metrics=None, model_res=None,
                 evaluator=None):
        """model_res: the graph's own resolution - xx, yy, msk may then live at any data resolution; the two resizes of an
        AR step run outside the captured graph, on the same stream (rollout_eval).  evaluator: as in rollout_eval.  A graph
        captured for 6-D windows [B, X, Y, Z, T, C] takes metrics= and evaluator=, not model_res= (wrap the model in
        Resized3D and capture at the data resolution instead: both resizes are then inside the graph)"""
        want = tuple(self.x.shape)
        if model_res is not None:
            if xx.dim() != 5:
                raise ValueError(f"GraphedRollout: model_res= needs an input [B, X, Y, T, C], got {tuple(xx.shape)}")
            if _size2(model_res) != want[1:3]:
                raise ValueError(f"GraphedRollout captured at resolution {want[1:3]}, model_res is {_size2(model_res)}")
            want = want[:1] + tuple(xx.shape[1:3]) + want[3:]
        if tuple(xx.shape) != want:
            raise ValueError(f"GraphedRollout captured for input {tuple(self.x.shape)}, got {tuple(xx.shape)}"
                             + ("" if model_res is None else f" (model_res {_size2(model_res)})"))
        return rollout_eval(self.model, xx, yy, msk, T_bundle, step=self.step, metrics=metrics, model_res=model_res,
                            evaluator=evaluator)
