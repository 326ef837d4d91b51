"""Checkpoint loading and auto-regressive inference for the MI355X DPOTNet.

* ``load_model_from_checkpoint`` / ``load_components_from_pretrained`` - the contracts of the reference's
  utils/utilities.py:99-166 (``module.`` prefix of DDP checkpoints stripped; fine-tuning may take only some
  components from a pretrained state_dict), written against the same sub-module names, so a pretrained ``.pth``
  (``torch.load(path)['model']``, README.md:30) loads unchanged.
* ``rollout_eval`` / ``GraphedRollout`` - the no-grad rollout of evaluate.py:183-222: the model's own prediction is
  appended to the input window step after step; returns the prediction, the per-step loss sum and the loss of the
  whole trajectory (both SimpleLpLoss(size_average=False)).  With fixed shapes the single forward step is one
  hipGraph that is replayed T_ar / T_bundle times (the window slide writes into the graph's static input).
* ``refill_mask`` and ``model_res=`` - the resolution-generalisation rollout of evaluate_varyingres.py:198-248: data on
  a res x res grid runs through a model built for another resolution; every AR step Fourier-resizes the window up to the
  model's resolution (ops.spectral_resize, one launch) and the prediction back down.
"""
from __future__ import annotations

import contextlib
import warnings
from collections import OrderedDict
from typing import Dict, Iterable, Mapping, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import ops
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


# ------------------------------------------------------------------------------------------------------
def _size2(res) -> Tuple[int, int]:
    return (int(res), int(res)) if isinstance(res, int) else (int(res[0]), int(res[1]))


def refill_mask(msk: Tensor, res) -> Tensor:
    """evaluate_varyingres.py:198-201: the mask of resized data [B, res, res, 1, C] - a channel of a sample is 1 everywhere
    if the original mask has any non-zero entry in it, else 0.  `res` is one int or (res_x, res_y)."""
    rx, ry = _size2(res)
    nonzero = (msk.sum(dim=(1, 2, 3)) > 0)[:, None, None, None, :]
    return nonzero.to(torch.float32).expand(msk.shape[0], rx, ry, 1, msk.shape[-1]).contiguous()


@torch.no_grad()
def rollout_eval(model: nn.Module, xx: Tensor, yy: Tensor, msk: Optional[Tensor], T_bundle: int = 1,
                 step=None, metrics=None, model_res=None) -> Tuple[Tensor, Tensor, Tensor]:
    """evaluate.py:193-213.  Returns (pred [B,X,Y,T_ar,C], sum of the per-step losses, loss of the whole rollout).
    `step(xx) -> im` defaults to the model's forward (a GraphedRollout passes its graph replay).
    metrics: a train.StepMetrics - the test loop's test_l2_step / test_l2_full (train_temporal.py:252-281) are accumulated
    on the device (one launch per rollout, no synchronisation; `metrics.read()` at the end of the loop), and the loss of the
    whole rollout is formed from the statistics the per-step losses left (ops.rel_l2_combine) instead of a second pass over
    the concatenated fields - equal to the two-pass value at the parity tolerance (tests/test_gpu_metrics.py), not bit for
    bit: without `metrics` the returned value stays on the two-pass path.
    model_res (an int or (res_x, res_y)): evaluate_varyingres.py:228-248 - xx, yy and msk live at the DATA resolution; every
    step Fourier-resizes the window to model_res, runs the model there and resizes the prediction back; loss, metrics and
    the window slide stay at the data resolution.  As in the reference the two resizes also run when model_res equals the
    data resolution (every frequency is kept then: the identity up to rounding).  None: no resize is enqueued."""
    # weight-only products (packed AFNO weights, folded embed matrices, ...) once per rollout, not once per AR step
    scope = model.weights_scope() if (step is None and hasattr(model, "weights_scope")) else contextlib.nullcontext()
    step = step or (lambda x: model(x)[0])
    T_ar = yy.shape[-2]
    loss_steps = None
    preds = []
    xx = xx.contiguous()
    n_steps = len(range(0, T_ar, T_bundle))
    if metrics is not None:
        metrics._check_steps(n_steps)
    if model_res is not None:
        model_res, data_res = _size2(model_res), (xx.shape[1], xx.shape[2])
    with scope:
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
    if metrics is not None:
        metrics.end_rollout(loss_steps, n_steps, pred.shape[0], pred.shape[-1], 0)
        metrics.accumulate()
        return pred, loss_steps, metrics.l2_full.clone().view(())
    loss_full = rel_l2_loss(pred.contiguous(), yy.contiguous(), msk)
    return pred, loss_steps, loss_full


class GraphedRollout:
    """One hipGraph of the forward step for a fixed input shape, replayed for every AR step."""

    def __init__(self, model: nn.Module, example_xx: Tensor):
        self.model = model
        self.x = example_xx.detach().clone().contiguous()
        was_training = model.training
        model.eval()
        with torch.no_grad():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    model(self.x)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.im, self.cls = model(self.x)
        model.train(was_training)

    def step(self, xx: Tensor) -> Tensor:
        self.x.copy_(xx)
        self.graph.replay()
        return self.im.clone()          # the graph's output buffer is overwritten by the next replay

    def __call__(self, xx: Tensor, yy: Tensor, msk: Optional[Tensor], T_bundle: int = 1, metrics=None, model_res=None):
        """model_res: the graph's own resolution - xx, yy, msk may then live at any data resolution; the two resizes of an
        AR step run outside the captured graph, on the same stream (rollout_eval)"""
        want = tuple(self.x.shape)
        if model_res is not None:
            if xx.dim() != 5:
                raise ValueError(f"GraphedRollout: input must be [B, X, Y, T, C], got {tuple(xx.shape)}")
            if _size2(model_res) != want[1:3]:
                raise ValueError(f"GraphedRollout captured at resolution {want[1:3]}, model_res is {_size2(model_res)}")
            want = want[:1] + tuple(xx.shape[1:3]) + want[3:]
        if tuple(xx.shape) != want:
            raise ValueError(f"GraphedRollout captured for input {tuple(self.x.shape)}, got {tuple(xx.shape)}"
                             + ("" if model_res is None else f" (model_res {_size2(model_res)})"))
        return rollout_eval(self.model, xx, yy, msk, T_bundle, step=self.step, metrics=metrics, model_res=model_res)
