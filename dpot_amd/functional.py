"""Autograd functions of the DPOT step, one per stage, each with a hand-written backward that calls the HIP
kernels directly (no autograd tracing inside a stage, no eager-PyTorch math):

  EmbedFn   patch embed (8x8/8 conv as GEMM + act) -> folded [1x1 conv + pos + TimeAggregator] GEMM  models/dpot.py:373-384
  BlockFn   GroupNorm -> AFNO mixer -> GroupNorm -> channel MLP -> +residual                        models/dpot.py:165-180
  HeadFn    out_layer (ConvTranspose as GEMM + pixel tail) and cls_head                             models/dpot.py:394-398
  RelL2Fn   masked relative L2 loss                                                                 utils/criterion.py:38-59
  AFNO3DFn, GroupNormFn, Mlp2Fn, TimeAggFn, Head3DFn, block3d   the 3-D model's stages          models/dpot3d.py
  AALReLUFn, PatchConvFn, LinearFn, ClsHeadFn, TokenMeanFn      the CDPOT model's stages        models/dpot_res.py

Every chain of Linear layers in the plain stages (Mlp2Fn, LinearFn, ClsHeadFn, PatchConvFn, PatchEmbed3DFn, the pointwise layers of
Head3DFn, HeadFn's cls_head and unfused tail) runs through _dense_fwd / _dense_bwd: one place where a dense layer is differentiated.

Internal activation layout: channels-last tokens [B, h*w, E] (row-major [B*h*w, E]).

Parameter gradients: when the parameters live in a train.FlatParams buffer, the backward kernels write them straight
into their slot of the flat gradient buffer (see _Sink) and autograd receives None - no per-parameter accumulate
kernels, and the data-parallel reducer is notified the moment a parameter's gradient is final.
"""
from __future__ import annotations

import os
from collections import OrderedDict, namedtuple
from typing import NamedTuple, Optional

import torch

from . import ops
from .ops import EPI_ACT, EPI_DACT

Tensor = torch.Tensor


def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


class _Sink:
    """Where the gradient of one parameter goes.

    forward:  ``_Sink(param, needed)`` registers one pending use if ``param`` is bound to a FlatParams slot.
    backward: ``out()`` is the buffer the producing kernel should write (the slot itself for the first contribution of
              a step, None = "allocate a temporary" otherwise); ``done(t)`` finalises: returns ``t`` for plain
              autograd, or adds/marks the slot, notifies the owner when the last pending use has delivered, and
              returns None (autograd then has nothing to accumulate)."""
    __slots__ = ("fp", "i")

    def __init__(self, param: Optional[Tensor], needed: bool):
        s = getattr(param, "_dpot_grad_slot", None) if (needed and param is not None) else None
        self.fp, self.i = s if s is not None else (None, -1)
        if self.fp is not None:
            self.fp.pending[self.i] += 1

    def out(self) -> Optional[Tensor]:
        if self.fp is None or self.fp.filled[self.i]:
            return None
        return self.fp.grad_views[self.i]

    def done(self, t: Optional[Tensor]) -> Optional[Tensor]:
        if self.fp is None or t is None:
            return t
        fp, i = self.fp, self.i
        view = fp.grad_views[i]
        if t.data_ptr() != view.data_ptr():
            view.add_(t.reshape(view.shape))          # produced elsewhere (or a further use in this step): accumulate
        fp.filled[i] = True
        fp.pending[i] -= 1
        if fp.pending[i] == 0:
            fp.fire(i)
        return None

    def skip(self) -> None:
        """this use delivers no gradient (its branch of the backward did not run): release the pending count so the
        parameter can still be reported final (data-parallel bucket accounting)"""
        if self.fp is None:
            return
        fp, i = self.fp, self.i
        fp.pending[i] -= 1
        if fp.pending[i] == 0 and fp.filled[i]:
            fp.fire(i)


_AFNO_PARAMS = ("w1", "b1", "w2", "b2")
_MLP_PARAMS = ("f2w", "f2b", "f1w", "f1b")                # in the order of the weight-gradient launches' outputs
_GN_PARAMS = (("n1w", "n1b"), ("n2w", "n2b"))
_BLOCK_PARAMS = _GN_PARAMS[0] + _AFNO_PARAMS + _GN_PARAMS[1] + ("f1w", "f1b", "f2w", "f2b")          # BlockFn's order
# a Block's entry in its forward pass's WgradBatch: key = (M, E, mh, mp, (Mm, nb, bs), shape of a GroupNorm partial),
# mlp = (do2, Hh, xn2, dHpre), afno = (S, dO1pre, O1, dO2), gn = the partials of norm1, norm2, sinks = {parameter name: _Sink}
WgradJob = namedtuple("WgradJob", "key mlp afno gn sinks")


class WgradBatch:
    """The weight gradients of all Blocks of ONE forward pass, computed when the last of them has run its backward.

    No data gradient reads a weight gradient - only the optimiser does - so a Block's backward need not launch its own small
    weight-gradient problems (split deeply along the tokens to fill the chip) and its own finalising launch: it leaves its
    operands and sinks here, and the flush runs the channel-MLP problems of all Blocks in one launch, the AFNO ones in as many
    launches as `ops.afno_wgrad_batch_plan` balances, and ONE finalising launch (csrc/gemm_tn.hip).  DPOTNet creates one per
    forward (an auto-regressive rollout: one per pass) and hands it to its Blocks; a Block registers in its forward when all
    its parameters are bound to FlatParams slots (a gradient returned to autograd would have to exist when the Block's
    backward returns).  Blocks are counted, not ordered.  The deferred operands are the Block's saved activations and
    gradients its backward allocated; nothing writes them again, and the jobs keep them alive until the flush.

    By default the batched launches cut the tokens exactly as the per-block launches do (several rounds of workgroups in one
    launch): every partial and every sum is the same, the gradients are bit-identical to the per-block schedule's.
    DPOT_TUNE fused_small=3 selects the one-round rules instead (fewer, longer token ranges: less partial traffic, another
    summation order).  The default batch can CHAIN its token ranges (`chains`, `ops.wgrad_chain_scope`): a workgroup walks 2 or 4
    consecutive ranges, restarts its accumulators at every range boundary and adds the ranges' tiles in registers in the
    association of the finalising launch's summation tree - the one-round rules' traffic and launch shape, every rounding still
    the per-block schedule's.  The default is NO chain: alone the three launches gain 27 us at DPOT-Tiny (490 -> 463 us), but
    beside the embed backward the long one-round workgroups keep its launches off the CUs and the step LOSES 20 - 40 us at
    every chain setting (profiles/wgrad_chain_ab.txt).

    The flush is the last thing block 0's backward does; the embed backward that follows is a chain of small launches that reads
    none of its results.  By default (DPOT_TUNE fused_small=4 or 5, `ops.wgrad_lane_scope`) the three launch sets therefore go to the
    library's weight-gradient lane (lane 0 of csrc/lane.hip), a stream of its own that is forked from this one and joined back
    when the backward ends (`_lane_ok`, ops.wgrad_flush_async).  Same launches, same results."""

    def __init__(self):
        self.expected = self.delivered = 0
        self.jobs = []
        self.lane = ops.wgrad_lane_enabled()     # read in the forward: the flush runs on the autograd engine's thread
        self.chain = ops.wgrad_chain_override()

    def register(self) -> None:
        self.expected += 1

    def withdraw(self) -> None:
        """a registered Block whose backward took the per-block route after all"""
        self.delivered += 1
        self._maybe_flush()

    def deliver(self, job: WgradJob) -> None:
        self.jobs.append(job)
        self.delivered += 1
        self._maybe_flush()

    def _maybe_flush(self) -> None:
        if self.delivered < self.expected:
            return
        jobs, self.jobs, self.delivered = self.jobs, [], 0
        groups = {}
        for j in jobs:
            groups.setdefault(j.key, []).append(j)
        for g in groups.values():
            self._flush_group(g)

    @staticmethod
    def splits(n, M, E, mh, mp, Mm, nb, bs):
        """(channel-MLP splits, AFNO blocks per launch, splits12, splits) of a batch of n Blocks; a zero: not covered"""
        if ops.wgrad_batch_one_round():
            per, s12, sk = ops.afno_wgrad_batch_plan(Mm, nb, bs, n)
            return ops.mlp_wgrad_batch_splitk(M, E, mh, n, mp), (per if per >= 2 else 0), s12, sk
        covered = ops.afno_wgrad_batch_plan(Mm, nb, bs, 1)[0] >= 1          # the three-product form at 128 channels per block
        sk = ops.afno_wgrad2_splitk(Mm, nb, bs) if covered else 0
        s12 = ops.afno_wgrad2_splits12(Mm, bs, sk) if sk else 0
        return ops.mlp_wgrad2_splitk(M, E, mh, mp), min(n, ops.wgrad_batch_max_blocks()), s12, sk

    @staticmethod
    def chains(splits, override=None):
        """(mlp_chain, afno_chain) of the batch the 4-tuple `splits` describes: (1, 1) - no chain, the measured optimum of the step - or
        the `override` of `ops.wgrad_chain_scope` for the default batch (the largest chains that leave a full round of
        workgroups are `ops.mlp_wgrad_batch_chain` / `ops.afno_wgrad_batch_chain`); always (1, 1) under the one-round rules,
        whose ranges are already one round long"""
        if ops.wgrad_batch_one_round() or not all(splits) or override is None:
            return 1, 1
        return override

    @staticmethod
    def _lane_ok(g) -> bool:
        """The flush may run beside the rest of the backward (ops.wgrad_flush_async) when nobody looks at its gradients before
        the backward ends - no gradient-ready callbacks (a data-parallel reducer, hooks) - and every sink is the ONLY outstanding
        use of its parameter and writes its slot directly: no temporary to add on the step's stream now, none by a later
        contribution of this backward (a rollout's further passes).  The join (ops.wgrad_lane_join) is the autograd engine's
        end-of-backward callback; outside a backward there is none to queue."""
        for j in g:
            for sk in j.sinks.values():
                if sk.fp.callbacks or sk.fp.pending[sk.i] != 1 or sk.out() is None:
                    return False
        try:
            torch.autograd.Variable._execution_engine.queue_callback(ops.wgrad_lane_join)
        except RuntimeError:
            return False
        return True

    def _flush_group(self, g) -> None:
        M, E, mh, mp, adims, _ = g[0].key
        dev = g[0].mlp[0].device
        skm, per, s12, sk = WgradBatch.splits(len(g), M, E, mh, mp, *adims)
        cm, ca = WgradBatch.chains((skm, per, s12, sk), self.chain)
        lane = self.lane and self._lane_ok(g)
        if not lane:
            ops.wgrad_lane_join()        # nothing pending in a backward of one schedule; a mixed one adds on this stream below
        mops, aops = [[j.mlp[k] for j in g] for k in range(4)], [[j.afno[k] for j in g] for k in range(4)]
        def outs(j, names, shapes):      # the gradient slots where this is the step's first contribution, else temporaries
            return tuple(ops._out(j.sinks[nm].out(), shp, dev) for nm, shp in zip(names, shapes))
        mouts = [outs(j, _MLP_PARAMS, ((E, mh), (E,), (mh, E), (mh,))) for j in g]
        Mm, nb, bs = adims
        aouts = [outs(j, _AFNO_PARAMS, ((2, nb, bs, bs), (2, nb, bs)) * 2) for j in g]
        gn = [[(part,) + outs(j, names, ((E,), (E,))) for part, names in zip(j.gn, _GN_PARAMS)] for j in g]
        if lane:
            ops.wgrad_flush_async(mops, skm, mouts, aops, nb, bs, per, s12, sk, aouts, gn, cm, ca)
        else:
            mws = ops.mlp_wgrad_batch(*mops, skm, cm)
            aws = ops.afno_wgrad_batch(*aops, nb, bs, per, s12, sk, ca)
            ops.wgrad_batch_finalize((aws, s12, sk, nb, bs, aouts), (mws, skm, E, mh, mouts), gn, cm, ca)
        for i, j in enumerate(g):
            dW2, db2, dW1, db1 = mouts[i]
            (_, dg1, db1n), (_, dg2, db2n) = gn[i]
            final = (dW2.view(E, mh, 1, 1), db2, dW1.view(mh, E, 1, 1), db1) + aouts[i] + (dg1, db1n, dg2, db2n)
            for nm, t in zip(_MLP_PARAMS + _AFNO_PARAMS + _GN_PARAMS[0] + _GN_PARAMS[1], final):
                j.sinks[nm].done(t)


def _epoch_of(sinks):
    """(FlatParams, its weights epoch) of the first flat-bound parameter, or None.  DPOTNet keeps its derived weights
    (AFNO packs, panel packs, the de-embed matrix) in PERSISTENT buffers that every forward outside a weights_scope
    rewrites in place, and the stage backwards read them again without autograd version tracking; FlatParams.touch()
    advances the epoch whenever the parameters change.  (Parameters changed by other means are the caller's
    responsibility: run backward before modifying them.)"""
    for sk in sinks:
        if sk.fp is not None:
            return sk.fp, sk.fp.epoch
    return None


def _check_epoch(ctx, what: str) -> None:
    rec = ctx.weights_epoch
    if rec is not None and rec[0].epoch != rec[1]:
        raise RuntimeError(f"{what}.backward: the parameters were updated (optimiser step) after this forward ran; its "
                           "packed weights have been overwritten.  Run backward before the step, or re-run the forward.")


def _sinks(ctx, params, first_index: int):
    return [_Sink(p, ctx.needs_input_grad[first_index + k]) for k, p in enumerate(params)]


# ======================================================================================================
# a chain of dense layers (Linear / 1x1 convolution / k = s = P convolution on a patch matrix): every plain stage below
# ======================================================================================================
def _dense_fwd(x, layers, act: int, res=None, res_div: int = 0, res_mod: int = 0):
    """rows x[M, K] through `layers` = [(W[N, K], b), ...]: y = x W^T + b per layer, `act` after every layer but the last,
    `res` added by the last (ops.linear_fwd: res[M, N] row by row, or res[R, N] with res_mod = R as res[(m // res_div) % R]).
    x may be a callable that makes the rows (a patch matrix): they are dropped as soon as the first layer has read them.
    -> (y, the input of every layer - the callable for such a first one -, the pre-activation of every layer but the last):
    what _dense_bwd takes"""
    ins, pres = [], []
    last = len(layers) - 1
    for i, (W, b) in enumerate(layers):
        ins.append(x)
        xin = x() if callable(x) else x
        if i < last:
            x, pre = ops.linear_fwd(xin, W, b, act=act, save_pre=True)
            pres.append(pre)
        else:
            x, _ = ops.linear_fwd(xin, W, b, res=res, res_div=res_div, res_mod=res_mod)
        del xin
    return x, ins, pres


def _dense_bwd(dy, ins, pres, weights, act: int, need_dx: bool = True, pre0=None, sinks=None):
    """backward of _dense_fwd from dy[M, N_last] (contiguous), last layer to first; per layer the data gradient - times
    act'(pre-activation of the layer before) -, then (dW, db) in one launch (ops.linear_bwd_wb).  The first layer's data
    gradient runs only if need_dx, times act'(pre0) if the chain's input was an activation of pre0.  ins[0] may be a callable
    that makes the first layer's input: it is called once, right before that layer's weight gradient, and the result dropped
    right after.  sinks: per layer (_Sink of W, _Sink of b, shape of the parameter W) - where HeadFn delivers.
    -> (dx | None, [(dW, db) per layer])"""
    grads = [None] * len(weights)
    for i in reversed(range(len(weights))):
        aux = pres[i - 1] if i else pre0
        d_in = ops.linear_bwd_data(dy, weights[i], act=act if aux is not None else 0, aux=aux) if i or need_dx else None
        xin = ins[i]() if callable(ins[i]) else ins[i]
        if sinks is None:
            grads[i] = ops.linear_bwd_wb(dy, xin)
        else:
            s_w, s_b, shape = sinks[i]
            dW, db = ops.linear_bwd_wb(dy, xin, s_w.out(), s_b.out())
            grads[i] = s_w.done(dW.view(shape)), s_b.done(db)
        del xin
        dy = d_in
    return dy, grads


def _res_bwd(dy, res_div: int, res_mod: int):
    """gradient of the residual _dense_fwd added: dy itself, or its sum over the rows that share a row of the table"""
    if not res_mod:
        return dy
    M, N = dy.shape
    res_div = max(res_div, 1)
    return ops.group_rowsum(dy, M // (res_mod * res_div), res_mod, res_div, N)


# ======================================================================================================
def embed_grid_matrix(gx, gy, gt, X: int, Y: int, T: int, Cc: int, P: int):
    """[tok*T, 3*P*P]: the unit-grid columns of the patch matrix (input channels C..C+2 = x, y, t coordinates,
    models/dpot.py:356-357) - batch independent, constant for a model"""
    z = torch.zeros(1, X, Y, T, Cc, dtype=torch.float32, device=gx.device)
    return ops.patchify(z, gx, gy, gt, P)[:, Cc * P * P:].contiguous()


def embed_layout_jobs(pos, w0, b0, w2, b2):
    """the layout pieces of embed_derived as ops.LayoutJobs entries, in the order (w0p, b0p, w2p, posb)"""
    hid, E = w0.shape[0], w2.shape[0]
    K0 = w0[0].numel()
    hidp = _pad4(hid)
    tok = pos.shape[2] * pos.shape[3]
    return [(w0, None, (1, hidp, K0), (1, hid, K0), (0, K0, 1)),               # zero rows hid..hidp
            (b0, None, (1, 1, hidp), (1, 1, hid), (0, 0, 1)),
            (w2, None, (1, E, hidp), (1, E, hid), (0, hid, 1)),                # zero cols hid..hidp
            (pos, b2, (1, tok, E), (1, tok, E), (0, 1, tok))]                  # pos^T [tok, E] + conv bias


def embed_implicit_tables(w0, w0p, b0p, grid):
    """(wfrag, bt) of the implicit-GEMM patch embedding (csrc/embed.hip): data-channel weights in fragment order, and the
    unit-grid channels folded into a bias table  bt[(tok,t), n] = b0[n] + sum_{c>=C,i,j} grid[(tok,t),(c,i,j)] w0[n,c,i,j].
    With the layout pieces, all of the weight-only products that `embed_fwd` reads."""
    hidp, K0 = w0p.shape
    kg = grid.shape[1]
    wfrag = ops.embed_pack_w0(w0)
    bt = torch.empty(grid.shape[0], hidp, dtype=torch.float32, device=grid.device)
    ops.gemm(grid, w0p[:, K0 - kg:], bt, grid.shape[0], hidp, kg, transB=True, lda=kg, ldb=K0, ldc=hidp, bias=b0p)
    return wfrag, bt


def embed_derived(pos, w0, b0, w2, b2, taw, tagamma, tt, T: int, grid=None, layouts=None, implicit_tables: bool = True):
    """weight-only products of the embed stage (they depend on no activation, so a T_ar-step rollout computes them
    once per optimiser step, see DPOTNet.weights_scope): padded conv weights, pos+bias, the cos-scaled aggregation
    weights and the folded [1x1 conv -> TimeAggregator] matrices V / c described in EmbedFn.forward.  layouts: the four
    tensors of `embed_layout_jobs`, already refreshed (DPOTNet: one launch for all layout pieces of the model).
    implicit_tables=False leaves wfrag and bt None: the caller adds `embed_implicit_tables` (packs.ModelPacks.derive runs the rest
    on the side lane)"""
    hid, E = w0.shape[0], w2.shape[0]
    K0 = w0[0].numel()
    hidp = _pad4(hid)
    tok = pos.shape[2] * pos.shape[3]
    dev = pos.device
    if layouts is not None:
        w0p, b0p, w2p, posb = layouts[0].view(hidp, K0), layouts[1].view(hidp), layouts[2].view(E, hidp), layouts[3].view(tok, E)
    else:
        w0p = ops.copy2d_pad(w0, hid, K0, hidp, K0)                                # zero rows hid..hidp
        b0p = ops.copy2d_pad(b0, 1, hid, 1, hidp).view(hidp)
        w2p = ops.copy2d_pad(w2, E, hid, E, hidp)                                  # zero cols hid..hidp
        posT = ops.transpose2d(pos, 1, E, tok).view(tok, E)                        # [tok, E]
        posb = ops.bias_add(posT, b2)                                              # pos + conv bias
    ws = ops.timeagg_scale_w(taw, tagamma, tt) if tagamma is not None else taw
    V = torch.empty(T * hidp, E, dtype=torch.float32, device=dev)
    ops.gemm(w2p, ws, V, hidp, E, E, transA=True, lda=hidp, ldb=E, ldc=E, batch=T, strideA=0, strideB=E * E,
             strideC=hidp * E)
    wsum = ops.colsum(ws, T, E * E).view(E, E)
    cc = torch.empty(tok, E, dtype=torch.float32, device=dev)
    ops.gemm(posb, wsum, cc, tok, E, E, lda=E, ldb=E, ldc=E)
    wfrag = bt = None
    if grid is not None and implicit_tables:
        wfrag, bt = embed_implicit_tables(w0, w0p, b0p, grid)
    return w0p, b0p, w2p, posb, ws, V, wsum, cc, wfrag, bt, grid


class EmbedFn(torch.autograd.Function):
    """x[B,X,Y,T,C] -> latent [B, h*w, E]"""

    @staticmethod
    def forward(ctx, x, pos, w0, b0, w2, b2, taw, tagamma, gx, gy, gt, tt, P: int, act: int, derived=None):
        ops.capture_precision(ctx)       # re-applied around backward (ops.with_ctx_precision)
        x = x.contiguous()
        B, X, Y, T, Cc = x.shape
        h, w = X // P, Y // P
        tok = h * w
        hid, E = w0.shape[0], w2.shape[0]
        K0 = (Cc + 3) * P * P
        hidp = _pad4(hid)
        dev = x.device
        M = B * tok

        implicit = derived is not None and derived[8] is not None
        A0 = None if implicit else ops.patchify(x, gx, gy, gt, P)               # [M0, K0], rows (b,px,py,t)
        if derived is None:
            derived = embed_derived(pos, w0, b0, w2, b2, taw, tagamma, tt, T)
        w0p, b0p, w2p, posb, ws, V, wsum, cc, wfrag, bt, grid = derived
        if implicit:   # rows gathered from x inside the kernel; grid channels + bias come from the table bt
            Hh, Hpre = ops.embed_fwd(x, wfrag, bt, hidp, act)
        else:
            Hh, Hpre = ops.linear_fwd(A0, w0p, b0p, act=act, save_pre=True)    # [M0, hidp]
        ops.side_lane_join()             # V and cc of `derived` (packs.ModelPacks.derive: side-lane site `weights`)
        # Everything after the activation is LINEAR (1x1 conv hid->E, + pos_embed, TimeAggregator), and the hidden
        # width is only hid = out_channels*P+3 (35).  Instead of materialising z[M0, E] (168 MB at B=32) and
        # contracting it with ws[T*E, E] (K = 5120), the 1x1 conv is folded INTO the aggregation weights every step:
        #     V[t,h,j]  = sum_i w2[i,h] * ws[t,i,j]                         (T small GEMMs, 0.2 GFLOP)
        #     c[tok,j]  = sum_i (pos[tok,i] + b2[i]) * sum_t ws[t,i,j]       (token-dependent constant)
        #     y[m,j]    = sum_{t,h} H[m,(t,h)] * V[(t,h),j] + c[tok(m),j]    (K = T*hidp = 360 instead of 5120)
        # Same result up to fp32 re-association; 15x fewer FLOPs for this stage, and its backward.
        Yl = torch.empty(M, E, dtype=torch.float32, device=dev)
        ops.gemm(Hh, V, Yl, M, E, T * hidp, lda=T * hidp, ldb=E, ldc=E, res=cc, ldres=E, res_mod=tok)
        ctx.implicit = implicit
        ctx.save_for_backward(x if implicit else A0, Hpre, Hh, w0p, w2p, ws, V, wsum, posb, taw, tagamma, tt,
                              grid if implicit else x.new_empty(0))
        ctx.dims = (B, X, Y, T, Cc, P, h, w, hid, hidp, E, K0, act)
        ctx.sinks = _sinks(ctx, (pos, w0, b0, w2, b2, taw, tagamma), 1)
        ctx.weights_epoch = _epoch_of(ctx.sinks)
        ctx.side = ops.side_lane_enabled("patch")        # read in the forward: the backward runs on the autograd engine's thread
        return Yl.view(B, tok, E)

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dY):
        _check_epoch(ctx, "EmbedFn")
        A0, Hpre, Hh, w0p, w2p, ws, V, wsum, posb, taw, tagamma, tt, grid = ctx.saved_tensors
        B, X, Y, T, Cc, P, h, w, hid, hidp, E, K0, act = ctx.dims
        s_pos, s_w0, s_b0, s_w2, s_b2, s_taw, s_gamma = ctx.sinks
        tok = h * w
        M, M0 = B * tok, B * tok * T
        dev = dY.device
        dY = dY.contiguous().view(M, E)
        # y = H V + c  ->  dH = dY V^T (times act'), dV = H^T dY, dc = sum_b dY
        dHpre = torch.empty(M0, hidp, dtype=torch.float32, device=dev)         # viewed [M, T*hidp]
        ops.gemm(dY, V, dHpre, M, T * hidp, E, transB=True, lda=E, ldb=E, ldc=T * hidp, act=act, mode=EPI_DACT,
                 aux=Hpre, ldaux=T * hidp)
        def first_conv():
            """(dw0, db0) of the first (PxP / stride P) conv, before their sinks: they need only dHpre"""
            if ctx.implicit:
                # data channels: implicit weight-gradient GEMM over x (A0 holds x here); unit-grid channels: the grid matrix
                # is batch independent -> contract it with the batch-summed dHpre; both land in the gradient slot itself
                db0 = ops.colsum(dHpre, M0, hid, ld=hidp, out=s_b0.out())
                dw0 = ops._out(s_w0.out(), (hid, K0), dev)
                ops.embed_wgrad(A0, dHpre, dw0, hid)
                dHs = ops._scratch(ops.group_rowsum(dHpre, B, tok * T, 1, hidp))   # [tok*T, hidp]
                kg = grid.shape[1]
                ops.gemm(dHs, grid, dw0[:, K0 - kg:], hid, kg, tok * T, transA=True, lda=hidp, ldb=kg, ldc=K0)
                return dw0.view(hid, Cc + 3, P, P), db0
            if hid == hidp:
                dw0p, db0 = ops.linear_bwd_wb(dHpre, A0, None, s_b0.out())      # [hidp, K0] (padded: 16-byte loads)
            else:
                db0 = ops.colsum(dHpre, M0, hid, ld=hidp, out=s_b0.out())
                dw0p = ops.linear_bwd_weight(dHpre, A0)
            return ops.copy2d_pad(ops._scratch(dw0p), hidp, K0, hid, K0, out=s_w0.out()).view(hid, Cc + 3, P, P), db0

        # Side-lane site `patch` (ops.side_lane): the first conv's gradients are a chain of their own beside the weight-only chain
        # below; their sinks are told after the join - a gradient-ready callback must never see an unfinished slot
        try:
            if ctx.side:
                with ops.side_lane("patch", on=True, join=False):
                    dw0, db0 = first_conv()
            dV = torch.empty(T * hidp, E, dtype=torch.float32, device=dev)
            ops.gemm(Hh, dY, dV, T * hidp, E, M, transA=True, lda=T * hidp, ldb=E, ldc=E,
                     splitk=ops.auto_splitk(T * hidp, E, M, tn=True))
            dc = ops.group_rowsum(dY, B, tok, 1, E)                                # [tok, E]
            # c = posb wsum  ->  dwsum = posb^T dc, dposb = dc wsum^T
            dwsum = torch.empty(E, E, dtype=torch.float32, device=dev)
            ops.gemm(posb, dc, dwsum, E, E, tok, transA=True, lda=E, ldb=E, ldc=E, splitk=ops.auto_splitk(E, E, tok, tn=True))
            dposb = torch.empty(tok, E, dtype=torch.float32, device=dev)
            ops.gemm(dc, wsum, dposb, tok, E, E, transB=True, lda=E, ldb=E, ldc=E)
            dpos = s_pos.done(ops.transpose2d(dposb, 1, tok, E, out=s_pos.out()).view(1, E, h, w))
            db2 = s_b2.done(ops.colsum(dposb, tok, E, out=s_b2.out()))
            # V_t = w2^T ws_t  ->  dw2 = sum_t ws_t dV_t^T,  dws_t = w2 dV_t (+ dwsum for every t)
            dw2_t = torch.empty(T, E, hidp, dtype=torch.float32, device=dev)
            ops.gemm(ws, dV, dw2_t, E, hidp, E, transB=True, lda=E, ldb=E, ldc=hidp, batch=T, strideA=E * E,
                     strideB=hidp * E, strideC=E * hidp)
            dw2p = ops.colsum(dw2_t, T, E * hidp).view(E, hidp)
            dw2 = s_w2.done(ops.copy2d_pad(dw2p, E, hidp, E, hid, out=s_w2.out()).view(E, hid, 1, 1))
            dws = s_taw.out() if tagamma is None else None
            dws = ops._out(dws, (T, E, E), dev)
            ops.gemm(w2p, dV, dws, E, E, hidp, lda=hidp, ldb=E, ldc=E, batch=T, strideA=0, strideB=hidp * E,
                     strideC=E * E, res=dwsum, ldres=E, strideRes=0)
            if tagamma is not None:
                dtaw, dgamma = ops.timeagg_scale_w_bwd(dws, taw, tagamma, tt, out_dw=s_taw.out(),
                                                       out_dgamma=s_gamma.out())
                dtaw, dgamma = s_taw.done(dtaw), s_gamma.done(dgamma)
            else:
                dtaw, dgamma = s_taw.done(dws), None
            if not ctx.side:
                dw0, db0 = first_conv()
            dx = None
            if ctx.needs_input_grad[0]:
                dA0 = ops.linear_bwd_data(dHpre, w0p)                              # [M0, K0]
                dx = ops.unpatchify(dA0, B, X, Y, T, Cc, P)
        finally:
            ops.side_lane_join()
        db0 = s_b0.done(db0)
        dw0 = s_w0.done(dw0)
        return dx, dpos, dw0, db0, dw2, db2, dtaw, dgamma, None, None, None, None, None, None, None


# ======================================================================================================
def mlp_pack_kind(E: int, mh: int, M: Optional[int] = None) -> Optional[str]:
    """which pre-packed-weight kernel family the channel MLP of a model uses under the current precision settings:
    'bf16' (opt-in reduced precision), 'bf16x6' (fp32-accurate operand split; precision 'bf16x6', or 'auto' for GEMMs of
    >= 3 GFLOP), 'f32' (csrc/gemm_panel.hip) or None (generic kernels)"""
    eff = ops.effective_mlp_precision()
    Mq = 128 if M is None else M          # M = None: the model deriving its packs before it has seen a batch
    bf_ok = ops.gemm_bf16p_supported(Mq, mh, E) and ops.gemm_bf16p_supported(Mq, E, mh)
    if bf_ok and eff == ops.GEMM_BF16:
        return "bf16"
    # (The fp32-accurate modes do NOT take the three-plane panel kernel: it reaches 154-190 TFLOP/s fp32-equivalent against
    # 147-178 for the register-staged split kernel (gemm_split.h) but needs a 10 B/element pack pass per activation operand that
    # costs more than it gains - profiles/r02_bf16x6p_bench.txt; the opt-in of rounds 2-5 is gone, ops.gemm_bf16p(planes=3) stays.)
    if eff == ops.GEMM_F32 and ops.panel_enabled() and ops.gemm_panel_supported(Mq, mh, E) \
            and ops.gemm_panel_supported(Mq, E, mh):
        return "f32"
    return None


def _mlp_panel_mode(mlp_pk, M, E, mh, mp) -> int:
    """which pre-packed-weight kernel the channel MLP runs on: 0 = none (generic split GEMM), 1 = fp32 panel
    (csrc/gemm_panel.hip), 2 = bf16 panel (csrc/gemm_bf16p.hip; plain bf16 or the fp32-accurate bf16x6 split, by the
    packs' kind).  The packs were made for the precision that was current when the weights were derived; a different
    precision at call time falls back to the generic kernels."""
    if mlp_pk is None:
        return 0
    kind = getattr(mlp_pk, "kind", "f32")
    if kind != mlp_pack_kind(E, mh, M):
        return 0
    if kind == "f32":
        return 1
    ok = ops.gemm_bf16p_supported(E, mh, M) and ops.gemm_bf16p_supported(mh, E, M)     # weight-gradient shapes
    return 2 if ok else 0


class MixerWeights(NamedTuple):
    """One filter's two packed layers (a pair of ops.AfnoItem) resolved ONCE per forward, under the precision in effect, into the
    operands each launch takes.  The packs are epoch-checked persistent buffers: the ctx keeps the view (`for_backward`)."""
    fused: bool               # both layers in one launch (ops.afno_mlp2, csrc/afno_mlp.hip); else the generic batched GEMM
    fwd: Optional[tuple]      # (w1T, b1, w2T, b2) of the forward: fragment packs (fused) or the plain Wbig / bbig (generic)
    layout: int               # of fwd's and bwd's packs: 0 fragment-block-major Wbig, 1 (Wr, Wi) fragments, 2 bf16x6
    bwd: tuple                # (w1, w2) the backward data path multiplies by: packs of W^T (fused) or the plain Wbig
    base: Optional[tuple]     # (w1T, b1, w2T, b2) for the one-launch AFNO layer (ops.afno_fused_fwd): never the bf16x6 packs
    base_layout: int

    @classmethod
    def of(cls, packed) -> "MixerWeights":
        a, b = packed
        if a.fwd is None:
            return cls(False, (a.wbig, a.bbig, b.wbig, b.bbig), 0, (a.wbig, b.wbig), None, 0)
        base = (a.fwd, a.bbig, b.fwd, b.bbig)
        if a.p6 is not None and b.p6 is not None and ops.afno_mlp6_wanted():
            # fp32-accurate on the bf16 matrix cores (gemm_precision 'auto' / 'bf16x6', csrc/afno_mlp6.hip): same contract
            return cls(True, (a.p6[0], a.bbig, b.p6[0], b.bbig), 2, (a.p6[1], b.p6[1]), base, a.layout)
        return cls(True, base, a.layout, (a.bwd, b.bwd), base, a.layout)

    def for_backward(self, recompute: bool) -> "MixerWeights":
        """what the ctx keeps: all of it when the backward runs the forward again, else the backward-data operands only"""
        return self if recompute else self._replace(fwd=None, base=None)


class BlockDims(NamedTuple("BlockDims", [(n, int) for n in "B tok E h w nb mx my mh act".split()])):
    """shapes of one Block: x [B, tok = h*w, E], nb diagonal blocks of E // nb channels, mx x my kept modes, hidden width mh"""
    M = property(lambda d: d.B * d.tok)               # token rows of the channel MLP
    Mm = property(lambda d: d.B * d.mx * d.my)        # kept-mode rows of the spectrum


class _WgradRoute:
    """Where the parameter gradients of ONE backward are delivered; the route is decided once, here:
      at once    every producer finalises its gradients itself (`put`): AFNO2DFn / AFNO3DFn, and DPOT_TUNE fused_small=0;
      `defer`    the fused weight-gradient launches leave their split-K partials, and ONE launch per block (csrc/gemm_tn.hip
                 block_finalize_kernel) reduces them together with the GroupNorm partials;
      `batch`    only operands are recorded: the forward pass's WgradBatch computes them with those of the other Blocks.
    The producers' generic split-K fallbacks `put` at once on every route.  `finish()` -> the gradients in the sinks' order."""

    def __init__(self, names, sinks):
        self.sinks = dict(zip(names, sinks))
        self.grads = dict.fromkeys(names)
        self.defer, self.batch = False, None
        self.afno_job = self.mlp_job = self.gn_parts = None
        self.mp = self.mlp_ops = self.afno_ops = self.afno_dims = None       # the batch route's record (of_block, mlp, afno)
        self.cs_jobs, self.late = (), []  # late: (name, tensor) final once the block's finalising launch has run

    @classmethod
    def of_block(cls, ctx, do2, Hh, xn2, S, bf16p: bool) -> "_WgradRoute":
        self = cls(_BLOCK_PARAMS, ctx.sinks)
        d, self.mp = ctx.dims, ctx.mlp_precision
        self.defer = ops.block_finalize_enabled()
        batch = ctx.wgrad_batch      # only the native fp32 two-layer weight-gradient launches, three-product AFNO form
        if batch is not None:
            bs = d.E // d.nb
            if (self.defer and not bf16p and do2.is_contiguous() and Hh.is_contiguous() and xn2.is_contiguous()
                    and ops.mlp_wgrad2_splitk(d.M, d.E, d.mh, self.mp) and ctx.mixer.fused and S.stride(0) == 2 * d.E
                    and ops.afno_wgrad2_splitk(d.Mm, d.nb, bs)
                    and all(WgradBatch.splits(batch.expected, d.M, d.E, d.mh, self.mp, d.Mm, d.nb, bs))):
                self.batch = batch
            else:
                batch.withdraw()
        return self

    def out(self, name: str, shape, dev) -> Tensor:
        return ops._out(self.sinks[name].out(), shape, dev)

    def put(self, name: str, t: Optional[Tensor]) -> None:
        self.grads[name] = self.sinks[name].done(t)

    def _launched(self, names, outs, job):
        if job is None:
            for n, t in zip(names, outs):
                self.put(n, t)
        else:
            self.late += zip(names, outs)
        return job

    def afno(self, S, dO1pre, O1, dO2, nb: int, bs: int, sk2: int) -> None:
        """both weight gradients of the mixer in ONE launch (csrc/gemm_tn.hip, dpot_afno_wgrad2)"""
        if self.batch is not None:
            self.afno_ops, self.afno_dims = (S, dO1pre, O1, dO2), (S.shape[0], nb, bs)
            return
        outs = [self.out(n, shp, S.device) for n, shp in zip(_AFNO_PARAMS, ((2, nb, bs, bs), (2, nb, bs)) * 2)]
        self.afno_job = self._launched(_AFNO_PARAMS, outs,
                                       ops.afno_wgrad2(S, dO1pre, O1, dO2, nb, bs, *outs, sk2, defer=self.defer))

    def mlp(self, do2, Hh, xn2, dHpre, skm: int) -> None:
        """both weight gradients of the channel MLP in ONE launch (csrc/gemm_tn.hip, dpot_mlp_wgrad2)"""
        if self.batch is not None:
            self.mlp_ops = (do2, Hh, xn2, dHpre)
            return
        (M, E), mh, dev = do2.shape, Hh.shape[1], do2.device
        df2w, df2b = self.out("f2w", (E, mh), dev), self.out("f2b", (E,), dev)
        df1w, df1b = self.out("f1w", (mh, E), dev), self.out("f1b", (mh,), dev)
        self.mlp_job = self._launched(_MLP_PARAMS, (df2w.view(E, mh, 1, 1), df2b, df1w.view(mh, E, 1, 1), df1b),
                                      ops.mlp_wgrad2(do2, Hh, xn2, dHpre, df2w, df2b, df1w, df1b, skm, defer=self.defer))

    def bias_colsums(self, df2b, df1b) -> None:
        """pack-both path: finished column sums, or with `defer` the pack passes' jobs (partials, rows, n, out)"""
        if self.defer:
            self.cs_jobs = [df2b, df1b]
            self.late += [("f2b", df2b[3]), ("f1b", df1b[3])]
        else:
            self.put("f2b", df2b), self.put("f1b", df1b)

    def groupnorm(self, gn1_part, gn2_part) -> None:
        self.gn_parts = (gn1_part, gn2_part)

    def finish(self) -> tuple:
        s = self.sinks
        if self.batch is not None:
            (M, E), mh = self.mlp_ops[0].shape, self.mlp_ops[1].shape[1]
            self.batch.deliver(WgradJob((M, E, mh, self.mp, self.afno_dims, tuple(self.gn_parts[0].shape)),
                                        self.mlp_ops, self.afno_ops, self.gn_parts, s))
        elif self.gn_parts is not None:
            gn_jobs = [(part, s[g].out(), s[b].out()) for part, (g, b) in zip(self.gn_parts, _GN_PARAMS)]
            if self.afno_job is not None or self.mlp_job is not None or self.cs_jobs:
                outs = ops.block_finalize(self.afno_job, self.mlp_job, gn_jobs, self.cs_jobs)
                for n, t in self.late:
                    self.put(n, t)
            else:
                outs = ops.groupnorm_param_grads(gn_jobs)
            for (g, b), (dg, db) in zip(_GN_PARAMS, outs):
                self.put(g, dg), self.put(b, db)
        return tuple(self.grads.values())


def _mixer_core(S, mw: MixerWeights, nb: int, act: int):
    """the block-diagonal complex 2-layer MLP on the kept modes (models/dpot.py:72-94): spectrum S [Mm, 2E] -> (O2, O1pre, O1)"""
    Mm, E, bs = S.shape[0], S.shape[1] // 2, S.shape[1] // 2 // nb
    w1, b1, w2, b2 = mw.fwd
    if mw.fused:
        # both layers of the block-diagonal complex MLP in ONE launch; the activated spectrum never leaves the CU
        # except as the copy saved for the backward (csrc/afno_mlp.hip)
        # only the pre-activation is saved: the activated layer-1 output (operand of the layer-2 weight gradient) is
        # re-derived by the backward launch from it (O1 = None here; one spectrum-sized store and 18.9 MB per block less)
        return ops.afno_mlp2(S, w1, b1, w2, b2, nb, bs, act, mode=0, want_pre=True, want_mid=False, layout=mw.layout)
    O1 = torch.empty(Mm, 2 * E, dtype=torch.float32, device=S.device)
    O1pre = torch.empty_like(O1)
    kw = dict(lda=2 * E, ldb=2 * bs, ldc=2 * E, batch=nb, strideA=2 * bs, strideB=4 * bs * bs, strideC=2 * bs,
              strideBias=2 * bs, tag=1)
    ops.gemm(S, w1, O1, Mm, 2 * bs, 2 * bs, bias=b1, act=act, mode=EPI_ACT, preact=O1pre, ldpre=2 * E,
             stridePre=2 * bs, **kw)
    O2 = torch.empty_like(O1)
    ops.gemm(O1, w2, O2, Mm, 2 * bs, 2 * bs, bias=b2, **kw)
    return O2, O1pre, O1


def _mixer_one_launch(x, mw: MixerWeights, d: BlockDims):
    """the whole mixer in ONE launch (csrc/afno_fused.hip), spectrum and hidden layer on chip; None: not covered"""
    if not (mw.fused and ops.afno_fused_supported(d.h, d.w, d.E, d.nb, d.mx, d.my, G=0, B=d.B, layout=mw.base_layout)):
        return None
    S, O1pre, y1 = ops.afno_fused_fwd(x, None, None, *mw.base, None, None, d.h, d.w, d.nb, d.mx, d.my, d.act)[:3]
    return y1, S, O1pre, None


def _mixer_fwd(xn1, mw: MixerWeights, d: BlockDims, norm=None):
    """AFNO2D.forward on [B, tok, E] (models/dpot.py:51-110): rfft2 -> _mixer_core -> irfft2 + x_orig -> (y1, S, O1pre, O1).
    norm = (mean, rstd, gamma, beta): xn1 is the UN-normalised block input and both DFT kernels apply GroupNorm1 on their
    loads (the transform's input and the residual) - the normalised field is never written"""
    one = _mixer_one_launch(xn1, mw, d) if norm is None else None
    if one is not None:
        return one
    S = ops.rfft2(xn1, d.h, d.w, d.nb, d.mx, d.my, 0, norm=norm)                     # [Mm, 2E]
    O2, O1pre, O1 = _mixer_core(S, mw, d.nb, d.act)
    y1 = ops.irfft2(O2, d.B, d.h, d.w, d.E, d.nb, d.mx, d.my, 1, res=xn1, res_norm=norm)  # + x_orig (the normalised input)
    return y1, S, O1pre, O1


def _mixer_core_bwd(dO2, S, O1pre, O1, mw: MixerWeights, nb: int, act: int, wg: _WgradRoute):
    """backward of _mixer_core: dO2 [Mm, 2E] -> dS; the four weight gradients go to `wg`"""
    Mm, E, bs, dev = dO2.shape[0], dO2.shape[1] // 2, dO2.shape[1] // 2 // nb, dO2.device
    wb1, wb2 = mw.bwd
    kw = dict(lda=2 * E, ldb=2 * bs, ldc=2 * E, batch=nb, strideA=2 * bs, strideB=4 * bs * bs, strideC=2 * bs)
    sk = max(2, ops.auto_splitk(2 * bs, 2 * bs, Mm, nb, tn=True))
    wkw = dict(transA=True, lda=2 * E, ldb=2 * E, ldc=2 * bs, batch=nb, strideA=2 * bs, strideB=2 * bs,
               strideC=4 * bs * bs, splitk=sk, mode=ops.EPI_AFNO_WGRAD)

    def wgrad(a, dy, w: str, b: str):
        # wgrad of Wbig; its split-K reduction writes dw / db in the parameters' own [2, nb, bs, ...] layout
        dw, db = wg.out(w, (2, nb, bs, bs), dev), wg.out(b, (2, nb, bs), dev)
        ops.gemm(a, dy, dw, 2 * bs, 2 * bs, Mm, colsum_out=db, colsum_of=2, **wkw)
        wg.put(w, dw), wg.put(b, db)

    sk2 = ops.afno_wgrad2_splitk(Mm, nb, bs) if mw.fused and S.stride(0) == 2 * E else 0
    if mw.fused:
        # data path of both layers in one launch: dO1pre = (dO2 W2^T) * act'(O1pre), dS = dO1pre W1^T; the same launch
        # re-derives O1 = act(O1pre) when the forward did not keep it
        dS, O1r, dO1pre = ops.afno_mlp2(dO2, wb2, None, wb1, None, nb, bs, act, mode=1, aux=O1pre, want_mid=True,
                                        want_pre=O1 is None, layout=mw.layout)
        O1 = O1r if O1 is None else O1
    if not sk2:
        wgrad(O1, dO2, "w2", "b2")
    if not mw.fused:
        dO1pre = torch.empty(Mm, 2 * E, dtype=torch.float32, device=dev)
        ops.gemm(dO2, wb2, dO1pre, Mm, 2 * bs, 2 * bs, transB=True, act=act, mode=EPI_DACT, aux=O1pre,
                 ldaux=2 * E, strideAux=2 * bs, **kw)
    if sk2:
        wg.afno(S, dO1pre, O1, dO2, nb, bs, sk2)
    else:
        wgrad(S, dO1pre, "w1", "b1")
    if not mw.fused:
        dS = torch.empty(Mm, 2 * E, dtype=torch.float32, device=dev)
        ops.gemm(dO1pre, wb1, dS, Mm, 2 * bs, 2 * bs, transB=True, **kw)
    return dS


def _afno_forward(ctx, x, weights, packed, nb: int, act: int, rfft, irfft, one_launch=None):
    """AFNO2DFn / AFNO3DFn: transform -> _mixer_core -> inverse transform + x.  rfft(t, col_weights) and
    irfft(spec, col_weights, res) are the pair of transform calls (kept for the backward: they hold shapes only)"""
    if packed is None:
        packed = tuple(ops.AfnoPacks([weights[:2], weights[2:]]).refresh())
    mw = MixerWeights.of(packed)
    out = one_launch(mw) if one_launch is not None else None
    if out is None:
        S = rfft(x, 0)                                                       # [Mm, 2E]
        O2, O1pre, O1 = _mixer_core(S, mw, nb, act)
        out = irfft(O2, 1, x), S, O1pre, O1                                  # + x_orig
    y, *saved = out
    ctx.save_for_backward(*saved)
    ctx.mixer, ctx.mixer_args, ctx.transforms = mw.for_backward(False), (nb, act), (rfft, irfft)
    ctx.sinks = _sinks(ctx, weights, 1)
    ctx.weights_epoch = _epoch_of(ctx.sinks)
    return y


def _afno_backward(ctx, dy, what: str):
    """adjoint of _afno_forward: (dx, dw1, db1, dw2, db2)"""
    _check_epoch(ctx, what)
    rfft, irfft = ctx.transforms
    dy = dy.contiguous()
    wg = _WgradRoute(_AFNO_PARAMS, ctx.sinks)
    dO2 = rfft(dy, 1)                                                        # adjoint of the inverse transform
    dS = _mixer_core_bwd(dO2, *ctx.saved_tensors, ctx.mixer, *ctx.mixer_args, wg)
    return (irfft(dS, 0, dy),) + wg.finish()                                 # adjoint of the transform, + skip path


class AFNO2DFn(torch.autograd.Function):
    """The AFNO mixer alone, as the reference's ``AFNO2D`` module computes it (models/dpot.py:51-110) on a channels-last
    field: x[B, h*w, E] -> irfft2(MLP(rfft2(x))) + x.  The very kernel sequence BlockFn runs (same helpers): the per-op
    golden vectors g1_afno_* drive the product mixer through this entry."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, h: int, w: int, nb: int, modes: int, act: int, packed=None):
        ops.capture_precision(ctx)       # re-applied around backward (ops.with_ctx_precision)
        x = x.contiguous()
        B, tok, E = x.shape
        d = BlockDims(B, tok, E, h, w, nb, min(modes, h), min(modes, w // 2 + 1), 0, act)
        return _afno_forward(ctx, x, (w1, b1, w2, b2), packed, nb, act,
                             lambda t, cw: ops.rfft2(t, h, w, nb, d.mx, d.my, cw),
                             lambda s, cw, res: ops.irfft2(s, B, h, w, E, nb, d.mx, d.my, cw, res=res),
                             lambda mw: _mixer_one_launch(x, mw, d))

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dy):
        return _afno_backward(ctx, dy, "AFNO2DFn") + (None,) * 6


# every intermediate of a Block's forward that its backward reads.  xn2 / Hh are the fp32 GroupNorm2 output and hidden layer,
# or on the pack-both bf16 path their TRANSPOSED bf16 packs (Hpre then: act'(pre-activation) as a bf16 pack)
_Parts = namedtuple("_Parts", "mean1 rstd1 S O1pre O1 y1 mean2 rstd2 xn2 Hpre Hh")


def _norms_mixer_fwd(x, n1w, n1b, n2w, n2b, mw: MixerWeights, d: BlockDims, pack_norm: bool, save: bool):
    """norm1 -> AFNO mixer -> norm2 by the fewest launches the shape allows: the first nine fields of _Parts, and fused_xp.
    pack_norm (the channel MLP's pack pass applies norm2 on its load): xn2 = None, or the one-launch layer wrote fused_xp"""
    B, tok, E, h, w, nb, mx, my = d[:8]
    fused_xp = None
    if mw.fused and ops.afno_fused_supported(h, w, E, nb, mx, my, B=B, layout=mw.base_layout):
        # the whole AFNO layer - norm1, rfft2, both MLP layers, irfft2, + x_orig, norm2 - in ONE launch (csrc/afno_fused.hip,
        # SURVEY 8 f4): spectrum and hidden layer stay on chip; save=False (nothing will run a backward on these
        # intermediates: inference, or a forward whose Block recomputes): S / O1pre are not even written
        # (round 5: with the bf16 channel MLP the same launch also writes GroupNorm2(y1) as the two bf16 operand packs -
        # DPOT_TUNE packs=0: the separate pack pass over y1 instead)
        fused_packs = pack_norm and ops.tune("packs") != 0
        w1T, b1, w2T, b2 = mw.base
        res = ops.afno_fused_fwd(
            x, n1w, n1b, w1T, b1, w2T, b2, n2w, n2b, h, w, nb, mx, my, d.act, save=save,
            want_y1=save or (pack_norm and not fused_packs), want_xn2=not pack_norm, want_packs=fused_packs,
            packs_trans=save)
        S, O1pre, y1, xn2, mean1, rstd1, mean2, rstd2 = res[:8]
        O1, fused_xp = None, (res[8:] if fused_packs else None)
    elif ops.gn_dft_supported(h, w, E):
        # GroupNorm fused with the neighbouring DFT (csrc/gn_dft.hip): norm1 + rfft2, and irfft2 + x_orig + norm2 -
        # two launches around the mixer instead of four, GroupNorm1(x) never written
        S, mean1, rstd1 = ops.gn_rfft2(x, n1w, n1b, h, w, nb, mx, my)
        O2, O1pre, O1 = _mixer_core(S, mw, nb, d.act)
        y1, xn2, mean2, rstd2 = ops.irfft2_gn(O2, x, mean1, rstd1, n1w, n1b, n2w, n2b, h, w, nb, mx, my,
                                              want_xn2=not pack_norm)
    else:
        # norm1 inside both DFT kernels where they are not fused with the statistics anyway (32x32 latent grid:
        # statistics-only GroupNorm launches, no normalised tensor)
        stats = ops.tune("gn_fuse") != 0 and ops.groupnorm_stats_supported(B, tok, E)
        if stats and ops.rfft2_norm_supported(h, w, E):
            mean1, rstd1 = ops.groupnorm_stats(x, n1w, n1b)
            y1, S, O1pre, O1 = _mixer_fwd(x, mw, d, norm=(mean1, rstd1, n1w, n1b))
        else:
            xn1, mean1, rstd1 = ops.groupnorm_fwd(x, n1w, n1b)
            y1, S, O1pre, O1 = _mixer_fwd(xn1, mw, d)
            del xn1
        if pack_norm and stats:
            xn2 = None
            mean2, rstd2 = ops.groupnorm_stats(y1, n2w, n2b)
        else:
            xn2, mean2, rstd2 = ops.groupnorm_fwd(y1, n2w, n2b)
    return mean1, rstd1, S, O1pre, O1, y1, mean2, rstd2, xn2, fused_xp


def _mlp_fwd(x, front: list, n2w, n2b, f1w, f1b, f2w, f2b, mlp_pk, panel: int, both: bool, d: BlockDims, mp, need_out: bool):
    """the channel MLP + outer residual on kernel family `panel` (_mlp_panel_mode): (out | None, xn2, Hpre, Hh) as _Parts
    keeps them.  Takes xn2 and fused_xp OUT of `front` (what _norms_mixer_fwd returned), so that the fp32 xn2 can be dropped
    here; xn2 = None (only with `both`): the pack pass applies GroupNorm2 on its load, or fused_xp exists"""
    M, E, mh, act = d.M, d.E, d.mh, d.act
    fused_xp, xn2 = front.pop(), front.pop()
    y1, mean2, rstd2 = front[5:]
    npl = mlp_pk.planes if panel == 2 else 0
    out = None
    if both:
        # plain-bf16 channel MLP, one pack pass per activation: the pass that packs xn2 / Hh as the A operand of the
        # next GEMM also writes the TRANSPOSED pack the weight gradient will need - that (bf16, half the bytes) is what
        # the backward keeps; the fp32 xn2 / Hh are dropped right here
        if fused_xp is not None:
            xp, xpT = fused_xp                      # written by the one-launch AFNO layer itself
        elif xn2 is None:
            xp, xpT, _ = ops.bf16_pack_both(y1.view(M, E), norm=(mean2, rstd2, n2w, n2b, d.tok))
        else:
            xp, xpT, _ = ops.bf16_pack_both(xn2.view(M, E))
        del xn2
        # fc1: the epilogue emits the activated hidden layer directly in its packed forms (no fp32 copy of it exists)
        # (Hpre here = act'(pre-activation) as a bf16 pack: all the backward needs of it, at half the bytes of the fp32
        # pre-activation and without a second activation evaluation)
        _, Hpre, hp, hpT, _ = ops.gemm_bf16p_packed(xp, mlp_pk[0], M, mh, E, bias=f1b, act=act, mode=EPI_ACT,
                                                    save_dact=True, pack_rows=need_out, pack_trans=True, store=False)
        if need_out:
            out, _ = ops.gemm_bf16p(hp, mlp_pk[2], M, E, mh, bias=f2b, res=x.view(M, E))
        return out, xpT, Hpre, hpT
    if panel == 2:   # bf16 matrix cores: weights pre-packed bf16 once per step, activations packed in one pass each
        Hh, Hpre = ops.gemm_bf16p(ops.bf16_pack_rows(xn2.view(M, E), planes=npl), mlp_pk[0], M, mh, E, bias=f1b, act=act,
                                  mode=EPI_ACT, save_pre=True, planes=npl)
    elif panel:    # static-weight panel GEMM (csrc/gemm_panel.hip): weights pre-packed once per optimiser step
        Hh, Hpre = ops.gemm_panel(xn2.view(M, E), mlp_pk[0], mh, bias=f1b, act=act, mode=EPI_ACT, save_pre=True)
    else:
        Hh, Hpre = ops.linear_fwd(xn2.view(M, E), f1w, f1b, act=act, save_pre=True, precision=mp)
    if need_out:
        if panel == 2:
            out, _ = ops.gemm_bf16p(ops.bf16_pack_rows(Hh, planes=npl), mlp_pk[2], M, E, mh, bias=f2b, res=x.view(M, E),
                                    planes=npl)
        elif panel:
            out, _ = ops.gemm_panel(Hh, mlp_pk[2], E, bias=f2b, res=x.view(M, E))
        else:
            out, _ = ops.linear_fwd(Hh, f2w, f2b, res=x.view(M, E), precision=mp)
    return out, xn2, Hpre, Hh


def _block_parts(x, n1w, n1b, n2w, n2b, f1w, f1b, mw: MixerWeights, d: BlockDims, mp, need_out, f2w=None, f2b=None,
                 mlp_pk=None, save=True):
    """forward of one Block up to (and optionally including) the second channel-MLP GEMM; returns (out | None, _Parts).
    Called by BlockFn.forward, and again by BlockFn.backward when activations are recomputed."""
    # GroupNorm2 applied ON THE LOAD of its consumer (DPOT_TUNE gn_fuse=0 disables): inside the pack pass of the bf16
    # channel MLP (the fp32 GroupNorm2(y1) is never written)
    panel = _mlp_panel_mode(mlp_pk, d.M, d.E, d.mh, mp)
    both = (panel == 2 and mlp_pk.planes == 1 and ops.tune("pack_both") != 0
            and ops.bf16_pack_both_supported(d.M, d.E) and ops.bf16_pack_both_supported(d.M, d.mh))
    pack_norm = both and ops.tune("gn_fuse") != 0 and d.tok % 64 == 0 and (d.E // 8) % 4 == 0
    front = list(_norms_mixer_fwd(x, n1w, n1b, n2w, n2b, mw, d, pack_norm, save))
    out, *back = _mlp_fwd(x, front, n2w, n2b, f1w, f1b, f2w, f2b, mlp_pk, panel, both, d, mp, need_out)
    return out, _Parts(*front, *back)


# The gradient a Block's backward returns (dx) is the `dout` of the PREVIOUS Block's backward, whose bf16 channel MLP first packs
# it (row form, transposed form, bias column sums: one more pass over it).  Round 5: the GroupNorm1-backward kernel that produces
# dx writes those packs itself (ops.groupnorm_bwd_packs); they travel beside the autograd gradient in this side table, keyed by
# the gradient's address.  An entry HOLDS dx, so its memory cannot be handed to another tensor while the entry lives (a stale
# key can never alias a different gradient); the consumer pops its entry, at most two entries are kept.
_GRAD_PACKS: "OrderedDict[int, tuple]" = OrderedDict()


def _stash_grad_packs(dx: Tensor, dop: Tensor, dopT: Tensor, cs: Tensor) -> None:
    _GRAD_PACKS[dx.data_ptr()] = (dx, dx._version, dop, dopT, cs)
    while len(_GRAD_PACKS) > 2:
        _GRAD_PACKS.popitem(last=False)


def clear_grad_packs() -> None:
    """drop the side table (the step classes call this after every backward: an entry nobody took - frozen prefix, a tensor
    hook that replaced the gradient - would otherwise pin dx and both packs until two later stashes evict it)"""
    _GRAD_PACKS.clear()


def _take_grad_packs(do2: Tensor):
    e = _GRAD_PACKS.pop(do2.data_ptr(), None)
    if e is None:
        return None
    dx, ver, dop, dopT, cs = e
    if dx.numel() != do2.numel() or dx._version != ver:       # another tensor / modified in place since: pack it afresh
        return None
    return dop, dopT, cs


class BlockFn(torch.autograd.Function):
    """x[B,tok,E] -> x + MLP(GN2(GN1(x) + irfft2(Mix(rfft2(GN1(x))))))

    ``recompute=True`` (activation recomputation, for long auto-regressive rollouts at 256^2: SURVEY 7 risk "T_ar>1
    backward"): only the block INPUT is kept; the backward re-runs the forward kernels (everything but the last GEMM)
    to rebuild the 11 intermediates.  Same kernels, same order -> bit-identical gradients, ~1/20 of the memory."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, w1, b1, w2, b2, n2w, n2b, f1w, f1b, f2w, f2b, h: int, w: int, nb: int, modes: int,
                act: int, packed=None, recompute: bool = False, mlp_pk=None, grad_enabled: bool = True,
                emit_grad_packs: bool = False, wgrad_batch: Optional[WgradBatch] = None):
        x = x.contiguous()
        (B, tok, E), mh = x.shape, f1w.shape[0]
        if packed is None:      # normally packed by the model (packs.DerivedWeights)
            packed = (ops.afno_pack3(w1, b1), ops.afno_pack3(w2, b2))
        mw = MixerWeights.of(packed)
        d = BlockDims(B, tok, E, h, w, nb, min(modes, h), min(modes, w // 2 + 1), mh, act)
        mp = ops.mlp_precision()                                               # channel-MLP GEMM precision override
        # (no input needs a gradient or the caller runs under no_grad - inference - or the Block recomputes: the
        # intermediates are dropped right below.  grad_enabled comes from the CALLER: inside forward() autograd is always off,
        # and needs_input_grad mirrors requires_grad of the inputs whatever the grad mode)
        keep = grad_enabled and any(ctx.needs_input_grad) and not recompute
        out, parts = _block_parts(x, n1w, n1b, n2w, n2b, f1w, f1b, mw, d, mp, True, f2w, f2b, mlp_pk, save=keep)
        ctx.mlp_pk = mlp_pk if _mlp_panel_mode(mlp_pk, d.M, E, mh, mp) else None
        ctx.mixer = mw.for_backward(recompute)
        if recompute:
            ctx.save_for_backward(x, n1w, n1b, n2w, n2b, f1w, f1b, f2w)
        else:
            ctx.save_for_backward(x, *parts, n1w, n2w, f1w, f2w)
        ctx.recompute, ctx.dims = recompute, d
        ctx.emit_grad_packs = emit_grad_packs     # a Block precedes this one: its bf16 channel-MLP backward wants dx packed
        ctx.mlp_precision = ops.effective_mlp_precision()    # a concrete code: the backward reproduces the forward's mode
        ctx.gemm_precision = ops._cur_gemm()
        ctx.sinks = _sinks(ctx, (n1w, n1b, w1, b1, w2, b2, n2w, n2b, f1w, f1b, f2w, f2b), 1)
        ctx.weights_epoch = _epoch_of(ctx.sinks)
        # deferred weight gradients (WgradBatch): every parameter gradient must have a FlatParams slot to land in later
        ctx.wgrad_batch = None
        if wgrad_batch is not None and keep and all(sk.fp is not None for sk in ctx.sinks):
            wgrad_batch.register()
            ctx.wgrad_batch = wgrad_batch
        return out.view(B, tok, E)

    @staticmethod
    def backward(ctx, dout):
        # the modes the forward ran in (per-model attributes), whatever thread autograd runs this on
        with ops.precision_scope(getattr(ctx, "gemm_precision", None), ctx.mlp_precision):
            _check_epoch(ctx, "BlockFn")
            d, mp, mlp_pk = ctx.dims, ctx.mlp_precision, ctx.mlp_pk
            if ctx.recompute:
                x, n1w, n1b, n2w, n2b, f1w, f1b, f2w = ctx.saved_tensors
                with torch.no_grad():
                    _, p = _block_parts(x, n1w, n1b, n2w, n2b, f1w, f1b, ctx.mixer, d, mp, False, mlp_pk=mlp_pk)
            else:
                x, *parts, n1w, n2w, f1w, f2w = ctx.saved_tensors
                p = _Parts(*parts)
            dout = dout.contiguous()
            do2 = dout.view(d.M, d.E)
            bf16p = mlp_pk is not None and mlp_pk.kind != "f32"
            both = bf16p and p.xn2.dtype == torch.bfloat16       # pack-both path: xn2 / Hh ARE the transposed bf16 packs
            wg = _WgradRoute.of_block(ctx, do2, p.Hh, p.xn2, p.S, bf16p)
            dxn2 = _mlp_bwd_packed(do2, p, mlp_pk, d, wg) if both else _mlp_bwd(do2, p, f1w, f2w, mlp_pk, d, mp, wg)
            pack_dx = both and ctx.emit_grad_packs and ctx.needs_input_grad[0]      # the previous Block wants dx packed as well
            dx = _norms_mixer_bwd(dout, dxn2, x, p, n1w, n2w, ctx.mixer, d, pack_dx, wg)
            return (dx,) + wg.finish() + (None,) * 11


def _mlp_bwd_packed(do2, p: _Parts, mlp_pk, d: BlockDims, wg: _WgradRoute):
    """channel-MLP backward on the pack-both bf16 path (see _mlp_fwd) -> dxn2 [M, E]: each gradient is packed once, in both forms,
    and its bias column sums come out of the same pass (with wg.defer: partials now, summed by the block's finalising launch)"""
    M, E, mh = d.M, d.E, d.mh
    s_f2b, s_f1b = wg.sinks["f2b"], wg.sinks["f1b"]
    taken = _take_grad_packs(do2)
    if taken is not None:              # packed by the kernel that produced this gradient (the next Block's backward)
        dop, dopT, cs_b = taken             # cs_b: [B * token ranges, E] partial column sums
        df2b = ((cs_b, cs_b.shape[0], E, wg.out("f2b", (E,), do2.device)) if wg.defer
                else ops.colsum(cs_b, cs_b.shape[0], E, out=s_f2b.out()))
    else:
        dop, dopT, df2b = ops.bf16_pack_both(do2, want_colsum=True, colsum_out=s_f2b.out(), defer_colsum=wg.defer)
    # both weight gradients in ONE launch once dHpre's pack exists, when each alone would need split-K
    pair = ops.gemm_bf16p_pair_wanted(E, mh, mh, E, M)
    if not pair:
        df2w, _ = ops.gemm_bf16p(dopT, p.Hh, E, mh, M, out=wg.sinks["f2w"].out())
    # dHpre = (do2 W2) * act'(Hpre) leaves the GEMM as its packs + bias column sums only
    _, _, dhp, dhpT, df1b = ops.gemm_bf16p_packed(dop, mlp_pk[3], M, mh, E, act=d.act, mode=EPI_DACT, dact=p.Hpre,
                                                  pack_rows=True, pack_trans=True, colsum=True,
                                                  colsum_out=s_f1b.out(), store=False, defer_colsum=wg.defer)
    if pair:
        df2w, df1w = ops.gemm_bf16p_pair(dopT, p.Hh, E, mh, dhpT, p.xn2, mh, E, M, out0=wg.sinks["f2w"].out(),
                                         out1=wg.sinks["f1w"].out())
    else:
        df1w, _ = ops.gemm_bf16p(dhpT, p.xn2, mh, E, M, out=wg.sinks["f1w"].out())
    del dop, dopT
    wg.put("f2w", df2w.view(E, mh, 1, 1)), wg.put("f1w", df1w.view(mh, E, 1, 1))
    wg.bias_colsums(df2b, df1b)
    return ops.gemm_bf16p(dhp, mlp_pk[1], M, E, mh)[0]


def _mlp_bwd(do2, p: _Parts, f1w, f2w, mlp_pk, d: BlockDims, mp, wg: _WgradRoute):
    """channel-MLP backward with fp32 activations -> dxn2 [M, E]: generic GEMMs, fp32 panels, or bf16 / bf16x6 panels"""
    M, E, mh, act = d.M, d.E, d.mh, d.act
    xn2 = p.xn2.view(M, E)
    bf16p = mlp_pk is not None and mlp_pk.kind != "f32"
    npl = mlp_pk.planes if bf16p else 0

    def wgrad(dy, xin, w: str, b: str, shape):
        n, k = dy.shape[1], xin.shape[1]
        if bf16p:   # dW[n, k] = dy^T xin on the bf16 matrix cores: both operands packed transposed (k-dim = tokens),
            #         split-K over the tokens with a fixed-order reduction; the bias gradient is a column sum
            dw, _ = ops.gemm_bf16p(ops.bf16_pack_rows(dy, trans=True, planes=npl),
                                   ops.bf16_pack_rows(xin, trans=True, planes=npl), n, k, M, out=wg.sinks[w].out(),
                                   planes=npl)
            db = ops.colsum(dy, M, n, out=wg.sinks[b].out())
        else:
            dw, db = ops.linear_bwd_wb(dy, xin, wg.sinks[w].out(), wg.sinks[b].out(), precision=mp)
        wg.put(w, dw.view(shape)), wg.put(b, db)

    # native fp32: both weight gradients in ONE launch once dHpre exists (csrc/gemm_tn.hip, dpot_mlp_wgrad2)
    skm = 0 if bf16p else ops.mlp_wgrad2_splitk(M, E, mh, mp)
    if skm and not (do2.is_contiguous() and p.Hh.is_contiguous() and p.xn2.is_contiguous()):
        skm = 0
    if not skm:
        wgrad(do2, p.Hh, "f2w", "f2b", (E, mh, 1, 1))
    if bf16p:
        dHpre, _ = ops.gemm_bf16p(ops.bf16_pack_rows(do2, planes=npl), mlp_pk[3], M, mh, E, act=act, mode=EPI_DACT,
                                  aux=p.Hpre, planes=npl)
    elif mlp_pk is not None:
        dHpre, _ = ops.gemm_panel(do2, mlp_pk[3], mh, act=act, mode=EPI_DACT, aux=p.Hpre)       # do2 W2, * act'(Hpre)
    else:
        dHpre = ops.linear_bwd_data(do2, f2w, act=act, aux=p.Hpre, precision=mp)  # [M, mh]
    if skm:
        wg.mlp(do2, p.Hh, xn2, dHpre, skm)
    else:
        wgrad(dHpre, xn2, "f1w", "f1b", (mh, E, 1, 1))
    if bf16p:
        return ops.gemm_bf16p(ops.bf16_pack_rows(dHpre, planes=npl), mlp_pk[1], M, E, mh, planes=npl)[0]
    if mlp_pk is not None:
        return ops.gemm_panel(dHpre, mlp_pk[1], E)[0]                      # dHpre W1
    return ops.linear_bwd_data(dHpre, f1w, precision=mp)                   # [M, E]


def _norms_mixer_bwd(dout, dxn2, x, p: _Parts, n1w, n2w, mw: MixerWeights, d: BlockDims, pack_dx: bool, wg: _WgradRoute):
    """norm2 backward, mixer backward, norm1 backward + outer skip: dxn2 [M, E] -> dx; both norms' partials go to `wg`"""
    B, tok, E, h, w, nb, mx, my = d[:8]
    if ops.gn_dft_supported(h, w, E):
        # norm2 backward + rfft2 (adjoint of the forward irfft2), then irfft2 (adjoint) + skip + norm1 backward + outer
        # skip: two launches around the mixer's backward (csrc/gn_dft.hip)
        dy1, gn2_part, dO2 = ops.gn_bwd_rfft2(dxn2.view(B, tok, E), p.y1, p.mean2, p.rstd2, n2w, h, w, nb, mx, my,
                                              col_weights=1)
        dS = _mixer_core_bwd(dO2, p.S, p.O1pre, p.O1, mw, nb, d.act, wg)
        if E // 8 <= 64:
            dx, gn1_part = ops.irfft2_gn_bwd(dS, dy1, x, p.mean1, p.rstd1, n1w, h, w, nb, mx, my, add=dout,
                                             col_weights=0)
        else:
            # 128 channels per group (DPOT-S / -M): this pair reads four fields with 4-byte accesses and runs at 64.7 us
            # against 20.0 + 24.6 us for the separate kernels (profiles/r03_step_census_M_bf16_v1.txt) - not fused
            dxn1 = ops.irfft2(dS, B, h, w, E, nb, mx, my, 0, res=dy1)
            if pack_dx and ops.groupnorm_bwd_packs_supported(tok, E, B=B) and ops.tune("packs") != 0:
                # dx goes to the previous Block's bf16 channel-MLP backward: written here in its packed forms as well
                dx, gn1_part, gp_r, gp_t, gp_cs = ops.groupnorm_bwd_packs(dxn1, x, p.mean1, p.rstd1, n1w, add=dout)
                _stash_grad_packs(dx, gp_r, gp_t, gp_cs)
            else:
                dx, gn1_part = ops.groupnorm_bwd(dxn1, x, p.mean1, p.rstd1, n1w, add=dout, defer=True)
    else:
        dy1, gn2_part = ops.groupnorm_bwd(dxn2.view(B, tok, E), p.y1, p.mean2, p.rstd2, n2w, defer=True)
        dO2 = ops.rfft2(dy1, h, w, nb, mx, my, 1)                              # adjoint of irfft2
        dS = _mixer_core_bwd(dO2, p.S, p.O1pre, p.O1, mw, nb, d.act, wg)
        dxn1 = ops.irfft2(dS, B, h, w, E, nb, mx, my, 0, res=dy1)              # adjoint of rfft2, + skip path
        # (DPOT-L: the CHUNKED GroupNorm backward could write the gradient's packs too - see the 128-channel branch above - but
        # there the staging + two barriers per 32-token sub-tile cost what the saved pack pass did: DPOT-L 91.2 -> 90.9 ms,
        # L20 2.185 -> 2.211 s, profiles/r05_grad_packs_step_ab_L.txt; the opt-in of round 5 is gone)
        dx, gn1_part = ops.groupnorm_bwd(dxn1, x, p.mean1, p.rstd1, n1w, add=dout, defer=True)
    wg.groupnorm(gn1_part, gn2_part)
    return dx


# ======================================================================================================
def head_layout_jobs(o0b, o4w, o4b, P: int, old: int):
    """the small layout pieces of head_derived as ops.LayoutJobs entries, in the order (bexp, [w4p, b4p])"""
    co = o4w.shape[0]
    PP = P * P
    jobs = [(o0b, None, (1, PP, old), (1, PP, old), (0, 0, 1))]                # bias repeated per pixel of the patch
    if old == 32 and 0 < co <= 32:
        jobs += [(o4w, None, (1, 32, 32), (1, co, 32), (0, 32, 1)), (o4b, None, (1, 1, 32), (1, 1, co), (0, 0, 1))]
    return jobs


def head_derived(o0w, o0b, o4w, o4b, P: int, wt_out=None, layouts=None):
    """weight-only layouts of the de-embed stage: ConvTranspose2d(k=s=P) weight as the GEMM matrix whose columns are
    ordered (i, j, o) - the GEMM result IS the pixel-major [pixels, old] matrix -, its bias repeated per pixel, and
    the zero-padded last 1x1 conv of the fused tail (None when the fused tail does not apply).  layouts: the tensors of
    `head_layout_jobs`, already refreshed"""
    E, old = o0w.shape[0], o0w.shape[1]
    co = o4w.shape[0]
    PP = P * P
    wt = ops.transpose2d(o0w, E, old, PP, out=wt_out).view(E, PP * old)
    w4p = b4p = None
    if layouts is not None:
        bexp = layouts[0].view(PP * old)
        if len(layouts) > 1:
            w4p, b4p = layouts[1].view(32, 32), layouts[2].view(32)
        return wt, bexp, w4p, b4p
    bexp = ops.tile_vec(o0b, PP)
    if old == 32 and 0 < co <= 32:
        w4p, b4p = ops.out_tail_pad(o4w, o4b, co)
    return wt, bexp, w4p, b4p


class HeadFn(torch.autograd.Function):
    """x[B,tok,E] -> (pred [B,X,Y,T_out*C_out], cls_pred [B,n_cls])"""

    @staticmethod
    def forward(ctx, x, o0w, o0b, o2w, o2b, o4w, o4b, c0w, c0b, c2w, c2b, c4w, c4b, h: int, w: int, P: int, act: int,
                derived=None):
        ops.capture_precision(ctx)       # re-applied around backward (ops.with_ctx_precision)
        ctx.set_materialize_grads(False)      # an unused output (cls_pred in train_temporal.py:226) costs nothing
        x = x.contiguous()
        B, tok, E = x.shape
        old, co = o0w.shape[1], o4w.shape[0]
        PP = P * P
        M, Mp = B * tok, B * tok * PP
        dev = x.device
        fused = ops.out_tail_supported(old, co, Mp)
        if derived is None:
            derived = head_derived(o0w, o0b, o4w, o4b, P)
        wt, bexp, w4p, b4p = derived[:4]
        head_pk = derived[4] if len(derived) > 4 else None
        if head_pk is not None and not (ops.panel_enabled() and ops.gemm_panel_supported(M, PP * old, E)
                                        and ops.gemm_panel_supported(M, E, PP * old)):
            head_pk = None
        ctx.head_pk = head_pk
        if fused:
            # GEMM writes only the pre-activation; the whole per-pixel tail (act, 1x1, act, 1x1, pixel shuffle) is one
            # kernel that reads it once (csrc/tail.hip)
            U = V = Vpre = None
            Upre = torch.empty(M, PP * old, dtype=torch.float32, device=dev)
            if head_pk is not None:
                Upre, _ = ops.gemm_panel(x.view(M, E), head_pk[0], PP * old, bias=bexp)
            else:
                ops.gemm(x, wt, Upre, M, PP * old, E, lda=E, ldb=PP * old, ldc=PP * old, bias=bexp)
            pred = ops.out_tail_fwd(Upre, o2w, o2b, w4p, b4p, B, h, w, P, co, act)  # [B, X, Y, co]
            V = w4p                                                            # (saved slot reused: padded W4)
        else:
            if head_pk is not None:
                U, Upre = ops.gemm_panel(x.view(M, E), head_pk[0], PP * old, bias=bexp, act=act, mode=EPI_ACT,
                                         save_pre=True)
            else:
                U = torch.empty(M, PP * old, dtype=torch.float32, device=dev)
                Upre = torch.empty_like(U)
                ops.gemm(x, wt, U, M, PP * old, E, lda=E, ldb=PP * old, ldc=PP * old, bias=bexp, act=act,
                         mode=EPI_ACT, preact=Upre, ldpre=PP * old)
            Z, (_, V), (Vpre,) = _dense_fwd(U.view(Mp, old), [(o2w, o2b), (o4w, o4b)], act)     # [Mp, co]
            pred = ops.pixel_shuffle(Z, B, h, w, P, co)                        # [B, X, Y, co]
        # classification head
        cls, (cm, c1, c2), (c1pre, c2pre) = _dense_fwd(ops.token_mean(x), [(c0w, c0b), (c2w, c2b), (c4w, c4b)], act)
        ctx.save_for_backward(x, wt, U, Upre, V, Vpre, o2w, o2b, o4w, cm, c1, c1pre, c2, c2pre, c0w, c2w, c4w)
        ctx.dims = (B, tok, E, h, w, P, old, co, act)
        ctx.fused = fused
        # the cls_head sinks are registered lazily in backward: whether that branch runs is only known there
        ctx.sinks = _sinks(ctx, (o0w, o0b, o2w, o2b, o4w, o4b), 1)
        ctx.cls_params = (c0w, c0b, c2w, c2b, c4w, c4b)
        ctx.cls_needed = tuple(ctx.needs_input_grad[7:13])
        ctx.weights_epoch = _epoch_of(ctx.sinks)
        return pred, cls

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dpred, dcls):
        _check_epoch(ctx, "HeadFn")
        x, wt, U, Upre, V, Vpre, o2w, o2b, o4w, cm, c1, c1pre, c2, c2pre, c0w, c2w, c4w = ctx.saved_tensors
        B, tok, E, h, w, P, old, co, act = ctx.dims
        s_o0w, s_o0b, s_o2w, s_o2b, s_o4w, s_o4b = ctx.sinks
        PP = P * P
        M, Mp = B * tok, B * tok * PP
        dev = x.device
        do0w = do0b = do2w = do2b = do4w = do4b = dx_out = None
        dc0w = dc0b = dc2w = dc2b = dc4w = dc4b = None
        if dpred is not None:
            # ---- out layer
            if ctx.fused:
                # the five small parameter gradients leave the partial-row reduction straight into their slots
                dUpre, (g2w, g4w, g2b, g0b, g4b) = ops.out_tail_bwd(
                    Upre, dpred.contiguous(), o2w, o2b, V, B, h, w, P, co, act,
                    outs=(s_o2w.out(), s_o4w.out(), s_o2b.out(), s_o0b.out(), s_o4b.out()))
                do2w = s_o2w.done(g2w.view(old, old, 1, 1))
                do4w = s_o4w.done(g4w.view(co, old, 1, 1))
                do2b, do0b, do4b = s_o2b.done(g2b), s_o0b.done(g0b), s_o4b.done(g4b)
            else:
                dZ = ops.pixel_shuffle(dpred.contiguous(), B, h, w, P, co, inverse=True)  # [Mp, co]
                dUpre, ((do2w, do2b), (do4w, do4b)) = _dense_bwd(
                    dZ, [U.view(Mp, old), V], [Vpre], [o2w.view(old, old), o4w.view(co, old)], act, pre0=Upre.view(Mp, old),
                    sinks=[(s_o2w, s_o2b, o2w.shape), (s_o4w, s_o4b, o4w.shape)])          # [Mp, old]
                do0b = s_o0b.done(ops.colsum(dUpre, Mp, old, out=s_o0b.out()))
            dU2 = dUpre.view(M, PP * old)
            if ctx.head_pk is not None:
                dx_out, _ = ops.gemm_panel(dU2, ctx.head_pk[1], E)
            else:
                dx_out = torch.empty(M, E, dtype=torch.float32, device=dev)
                ops.gemm(dU2, wt, dx_out, M, E, PP * old, transB=True, lda=PP * old, ldb=PP * old, ldc=E)
            dwt = torch.empty(E, PP * old, dtype=torch.float32, device=dev)
            ops.gemm(x, dU2, dwt, E, PP * old, M, transA=True, lda=E, ldb=PP * old, ldc=PP * old,
                     splitk=ops.auto_splitk(E, PP * old, M, tn=True))
            do0w = s_o0w.done(ops.transpose2d(dwt, E, PP, old, out=s_o0w.out()).view(E, old, P, P))
            dx_out = dx_out.view(B, tok, E)
        else:
            for sk in ctx.sinks:
                sk.skip()
        dx = dx_out
        if dcls is not None:
            # ---- cls head
            cs = [_Sink(p, n) for p, n in zip(ctx.cls_params, ctx.cls_needed)]
            dcm, ((dc0w, dc0b), (dc2w, dc2b), (dc4w, dc4b)) = _dense_bwd(
                dcls.contiguous(), [cm, c1, c2], [c1pre, c2pre], [c0w, c2w, c4w], act,
                sinks=[(cs[2 * i], cs[2 * i + 1], W.shape) for i, W in enumerate((c0w, c2w, c4w))])
            dx = ops.token_mean_bwd(dcm, tok, add=dx_out)
        return (dx, do0w, do0b, do2w, do2b, do4w, do4b, dc0w, dc0b, dc2w, dc2b, dc4w, dc4b, None, None, None, None,
                None)


# ======================================================================================================
class RelL2Fn(torch.autograd.Function):
    """sum_b sum_c ||(x-y) m||_2 / (||y m||_2 + 1e-8) / n_channels_b   (SimpleLpLoss(size_average=False))"""

    @staticmethod
    def forward(ctx, x, y, mask: Optional[Tensor], stats_out: Optional[Tensor] = None):
        x, y = ops._req(x.contiguous(), "pred"), ops._req(y.contiguous(), "target")
        B, Cc = x.shape[0], x.shape[-1]
        Tt = x.shape[-2] if x.dim() >= 3 else 1
        S = x.numel() // (B * Cc)
        if mask is not None:
            mask = mask.contiguous()
            if mask.numel() == x.numel():
                Tt_m = 1
            elif mask.numel() * Tt == x.numel():
                Tt_m = Tt
            else:
                raise ValueError(f"mask shape {tuple(mask.shape)} does not broadcast over {tuple(x.shape)}")
        else:
            Tt_m = 1
        # stats_out: a caller-owned slot the statistics are left in (and the backward reads them from): the per-step slots of
        # train.StepMetrics, from which ops.rel_l2_combine forms the full-rollout loss.  Same kernels, same result.
        loss, stats = ops.rel_l2_fwd(x, y, mask, B, S, Cc, Tt_m, stats=stats_out)
        ctx.save_for_backward(x, y, mask if mask is not None else x.new_empty(0), stats)
        ctx.meta = (B, S, Cc, Tt_m, mask is not None)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        x, y, mask, stats = ctx.saved_tensors
        B, S, Cc, Tt_m, has_mask = ctx.meta
        dx = ops.rel_l2_bwd(x, y, mask if has_mask else None, stats, g.contiguous().view(1), B, S, Cc, Tt_m)
        return dx, None, None, None


class ClsCEFn(torch.autograd.Function):
    """CrossEntropyLoss(reduction='sum')(logits, labels) and the number of rows whose argmax equals the label
    (train_temporal.py:209-213), both from one launch; backward: gloss * (softmax - onehot), one launch.
    Returns (loss 0-d float32, correct 0-d int64), both views of the 4-word dpot_cls_ce_out slot (ops.cls_ce_fwd);
    `slot` = None, or a 1-element list holding a caller-owned slot (a list, so that autograd does not see it as an input)."""

    @staticmethod
    def forward(ctx, logits, labels, slot=None):
        logits = ops._req(logits.contiguous(), "logits")
        labels = labels.contiguous().view(-1)
        out, row_stats = ops.cls_ce_fwd(logits, labels, slot[0] if slot else None)
        ctx.save_for_backward(logits, labels, row_stats)
        correct = out[1]
        ctx.mark_non_differentiable(correct)
        return ops.cls_out_loss(out), correct

    @staticmethod
    def backward(ctx, g, _gc):
        logits, labels, row_stats = ctx.saved_tensors
        return ops.cls_ce_bwd(logits, labels, row_stats, g.contiguous().view(1)), None, None


class AdaINFn(torch.autograd.Function):
    """lat * scale[b,:] + shift[b,:]   (models/dpot.py:386-387, the normalize=True branch)"""

    @staticmethod
    def forward(ctx, lat, scale, shift):
        lat, scale, shift = lat.contiguous(), scale.contiguous(), shift.contiguous()
        ctx.save_for_backward(lat, scale)
        return ops.scale_shift(lat, scale, shift)

    @staticmethod
    def backward(ctx, g):
        lat, scale = ctx.saved_tensors
        return ops.scale_shift_bwd(g.contiguous(), lat, scale)


def rel_l2_loss(x: Tensor, y: Tensor, mask: Optional[Tensor] = None, stats_out: Optional[Tensor] = None) -> Tensor:
    return RelL2Fn.apply(x, y, mask, stats_out)


def cls_ce_loss(logits: Tensor, labels: Tensor, out: Optional[Tensor] = None):
    """-> (loss, correct): the summed cross-entropy of logits [B, n_cls] against int64 labels [B] / [B, 1] (differentiable in
    the logits) and the count of rows whose first maximal logit is the label.  Rows with a label outside [0, n_cls) add
    nothing to either and get a zero gradient; `out` (optional 4-word int64 slot) then holds their count in word 3."""
    return ClsCEFn.apply(logits, labels, [out] if out is not None else None)


# ======================================================================================================
# 3-D model (models/dpot3d.py): AFNO3D on the kernels of csrc/dft3.hip, and the plain stages of DPOTNet3D
# ======================================================================================================
class AFNO3DFn(torch.autograd.Function):
    """The reference's ``AFNO3D`` (models/dpot3d.py:46-97) on a channels-last field x[B, X*Y*Z, E] (z fastest):
    irfftn(MLP(rfftn(x)[:modes, :modes, :8])) + x.  The 3-D twin of AFNO2DFn: rfft3 -> _mixer_core -> irfft3 (+ x); backward
    rfft3(dy, w(kz)) -> _mixer_core_bwd -> irfft3(dS, w = 1) + dy."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, dims3, nb: int, modes: int, act: int, packed=None):
        ops.capture_precision(ctx)
        x = x.contiguous()
        B, tok, E = x.shape
        dims3 = tuple(int(d) for d in dims3)
        assert tok == dims3[0] * dims3[1] * dims3[2], f"{tok} tokens are not a {dims3} grid"
        m3 = ops.kept_modes3(dims3, modes)
        return _afno_forward(ctx, x, (w1, b1, w2, b2), packed, nb, act,
                             lambda t, cw: ops.rfft3(t, dims3, nb, m3, cw),
                             lambda s, cw, res: ops.irfft3(s, B, dims3, E, nb, m3, cw, res=res))

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dy):
        return _afno_backward(ctx, dy, "AFNO3DFn") + (None,) * 5


class GroupNormFn(torch.autograd.Function):
    """GroupNorm(G, E) of a channels-last field x[B, tokens, E] (any number of spatial axes flattened into the tokens)"""

    @staticmethod
    def forward(ctx, x, gamma, beta, G: int = 8):
        x = x.contiguous()
        y, mean, rstd = ops.groupnorm_fwd(x, gamma, beta, G)
        ctx.save_for_backward(x, mean, rstd, gamma)
        ctx.G = G
        ctx.sinks = _sinks(ctx, (gamma, beta), 1)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, gamma = ctx.saved_tensors
        s_g, s_b = ctx.sinks
        dx, dg, db = ops.groupnorm_bwd(dy.contiguous(), x, mean, rstd, gamma, ctx.G, out_dgamma=s_g.out(),
                                       out_dbeta=s_b.out())
        return dx, s_g.done(dg), s_b.done(db), None


class Mlp2Fn(torch.autograd.Function):
    """y[M, N] = act(x[M, K] W1[H, K]^T + b1) W2[N, H]^T + b2 (+ res): two 1x1 convolutions / Linears with the activation in
    the first GEMM's epilogue.  res [M, N] is added row by row; res [R, N] with res_mod = R is added to row m as res[m % R]
    (a per-token table under a batch).  Weights are 2-D views of the parameters."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, act: int, res=None, res_mod: int = 0):
        ops.capture_precision(ctx)
        x, W1, W2 = x.contiguous(), W1.contiguous(), W2.contiguous()
        res = res.contiguous() if res is not None else None
        y, ins, pres = _dense_fwd(x, [(W1, b1), (W2, b2)], act, res, 0, res_mod)
        ctx.save_for_backward(*ins, *pres, W1, W2)
        ctx.act, ctx.res_mod, ctx.has_res = act, res_mod, res is not None
        return y

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dy):
        x, Hh, Hpre, W1, W2 = ctx.saved_tensors
        dy = dy.contiguous()
        dx, ((dW1, db1), (dW2, db2)) = _dense_bwd(dy, [x, Hh], [Hpre], [W1, W2], ctx.act, ctx.needs_input_grad[0])
        dres = _res_bwd(dy, 1, ctx.res_mod) if ctx.has_res and ctx.needs_input_grad[6] else None
        return dx, dW1, db1, dW2, db2, None, dres, None


class PatchEmbed3DFn(torch.autograd.Function):
    """PatchEmbed of DPOTNet3D (models/dpot3d.py:100-140) on the raw window x[B,S,S,S,T,C]: ops.patchify3 (the four coordinate
    channels come from the tables gs[S], gt[T]), then the two GEMMs of Mlp2Fn - k = s = P convolution, act, 1x1 convolution,
    + the pos_embed table ``pos`` [tok, E] - giving rows ((b, t), token).  The patch matrix ((C+4)/C times the window, per AR
    step) is NOT kept for the backward: x is, and the backward gathers the matrix again for the weight gradient and frees it.
    dx (an AR step whose input carries a gradient) comes from ops.unpatchify3."""

    @staticmethod
    def forward(ctx, x, gs, gt, W1, b1, W2, b2, pos, P: int, act: int):
        ops.capture_precision(ctx)
        x, W1, W2, pos = x.contiguous(), W1.contiguous(), W2.contiguous(), pos.contiguous()
        y, (_, Hh), (Hpre,) = _dense_fwd(lambda: ops.patchify3(x, gs, gt, P), [(W1, b1), (W2, b2)], act, pos, 0, pos.shape[0])
        ctx.save_for_backward(x, gs, gt, Hh, Hpre, W1, W2)
        ctx.P, ctx.act, ctx.tok = P, act, pos.shape[0]
        return y

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dy):
        x, gs, gt, Hh, Hpre, W1, W2 = ctx.saved_tensors
        dy = dy.contiguous()
        dA0, ((dW1, db1), (dW2, db2)) = _dense_bwd(dy, [lambda: ops.patchify3(x, gs, gt, ctx.P), Hh], [Hpre], [W1, W2], ctx.act,
                                                   ctx.needs_input_grad[0])
        dx = None
        if dA0 is not None:
            B, S, _, _, T, C = x.shape
            dx = ops.unpatchify3(dA0, B, S, T, C, ctx.P)
        dpos = _res_bwd(dy, 1, ctx.tok) if ctx.needs_input_grad[7] else None
        return dx, None, None, dW1, db1, dW2, db2, dpos, None, None


class TimeAggFn(torch.autograd.Function):
    """TimeAggregator (models/dpot3d.py:143-151) on rows A[M, T*E] (columns (t, i)): y[m, j] = sum_{t,i} A[m, (t,i)] ws[t,i,j]
    with ws = w (time_agg 'mlp') or w * cos(t gamma_i) ('exp_mlp': gamma given)"""

    @staticmethod
    def forward(ctx, A, w, gamma, tt):
        ops.capture_precision(ctx)
        A = A.contiguous()
        T, E, _ = w.shape
        M = A.shape[0]
        ws = ops.timeagg_scale_w(w, gamma, tt) if gamma is not None else w
        y = torch.empty(M, E, dtype=torch.float32, device=A.device)
        ops.gemm(A, ws, y, M, E, T * E, lda=T * E, ldb=E, ldc=E)
        ctx.save_for_backward(A, ws, w, gamma, tt)
        ctx.sinks = _sinks(ctx, (w, gamma), 1)
        ctx.weights_epoch = _epoch_of(ctx.sinks)
        return y

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dy):
        A, ws, w, gamma, tt = ctx.saved_tensors
        s_w, s_g = ctx.sinks
        T, E, _ = w.shape
        M = A.shape[0]
        dy = dy.contiguous()
        dev = dy.device
        dA = None
        if ctx.needs_input_grad[0]:
            dA = torch.empty(M, T * E, dtype=torch.float32, device=dev)
            ops.gemm(dy, ws, dA, M, T * E, E, transB=True, lda=E, ldb=E, ldc=T * E)
        dws = ops._out(s_w.out() if gamma is None else None, (T, E, E), dev)
        ops.gemm(A, dy, dws, T * E, E, M, transA=True, lda=T * E, ldb=E, ldc=E,
                 splitk=ops.auto_splitk(T * E, E, M, tn=True))
        if gamma is not None:
            dw, dgamma = ops.timeagg_scale_w_bwd(dws, w, gamma, tt, out_dw=s_w.out(), out_dgamma=s_g.out())
            dw, dgamma = s_w.done(dw), s_g.done(dgamma)
        else:
            dw, dgamma = s_w.done(dws), None
        return dA, dw, dgamma, None


def _unfold3(t: Tensor, B: int, h: int, P: int, old: int) -> Tensor:
    """(the torch statement of ops.fold3, kept as the yardstick of its tests and timings)
    [B*h^3, old*P^3] (rows (b, hx, hy, hz), columns (o, i, j, k)) -> [B*(hP)^3, old] (rows (b, x, y, z)): the scatter of a
    k = s = P transposed convolution"""
    return t.view(B, h, h, h, old, P, P, P).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(B * (h * P) ** 3, old)


def _fold3(t: Tensor, B: int, h: int, P: int, old: int) -> Tensor:
    """inverse of _unfold3"""
    return t.view(B, h, P, h, P, h, P, old).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(B * h ** 3, old * P ** 3)


class Head3DFn(torch.autograd.Function):
    """out_layer of DPOTNet3D (models/dpot3d.py:301-307): ConvTranspose3d(E -> old, k = s = P), act, Conv3d(old -> old, 1), act,
    Conv3d(old -> Co, 1) on latent rows x[B*h^3, E] -> [B*(hP)^3, Co] (rows (b, x, y, z)).  W0 [E, old*P^3] is the transposed
    convolution's weight viewed 2-D, b0e its bias repeated over the P^3 taps (column order (o, i, j, k))."""

    @staticmethod
    def forward(ctx, x, W0, b0e, W2, b2, W4, b4, B: int, h: int, P: int, act: int):
        ops.capture_precision(ctx)
        x, W0, W2, W4 = x.contiguous(), W0.contiguous(), W2.contiguous(), W4.contiguous()
        M, E = x.shape
        old = W2.shape[0]
        N0 = old * P ** 3
        H1 = torch.empty(M, N0, dtype=torch.float32, device=x.device)
        H1pre = torch.empty_like(H1)
        ops.gemm(x, W0, H1, M, N0, E, lda=E, ldb=N0, ldc=N0, bias=b0e.contiguous(), act=act, mode=EPI_ACT, preact=H1pre,
                 ldpre=N0)
        H1p = ops.fold3(H1, B, h, P, old)                                   # rows (b, x, y, z)
        del H1
        H1pre_p = ops.fold3(H1pre, B, h, P, old)
        del H1pre
        out, (_, H2), (H2pre,) = _dense_fwd(H1p, [(W2, b2), (W4, b4)], act)
        ctx.save_for_backward(x, W0, W2, W4, H1p, H1pre_p, H2, H2pre)
        ctx.dims = (B, h, P, old, act)
        return out

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dout):
        x, W0, W2, W4, H1p, H1pre_p, H2, H2pre = ctx.saved_tensors
        B, h, P, old, act = ctx.dims
        M, E = x.shape
        N0 = old * P ** 3
        dev = x.device
        dout = dout.contiguous()
        dH1pre_p, ((dW2, db2), (dW4, db4)) = _dense_bwd(dout, [H1p, H2], [H2pre], [W2, W4], act, pre0=H1pre_p)
        dH1pre = ops.fold3(dH1pre_p, B, h, P, old, inverse=True)             # [M, old*P^3]
        dW0 = torch.empty(E, N0, dtype=torch.float32, device=dev)
        ops.gemm(x, dH1pre, dW0, E, N0, M, transA=True, lda=E, ldb=N0, ldc=N0, splitk=ops.auto_splitk(E, N0, M, tn=True))
        db0e = ops.colsum(dH1pre, M, N0)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, E, dtype=torch.float32, device=dev)
            ops.gemm(dH1pre, W0, dx, M, E, N0, transB=True, lda=N0, ldb=N0, ldc=E)
        return dx, dW0, db0e, dW2, db2, dW4, db4, None, None, None, None


def block3d(x, n1w, n1b, w1, b1, w2, b2, n2w, n2b, f1w, f1b, f2w, f2b, dims3, nb: int, modes: int, act: int, packed=None):
    """``Block`` of models/dpot3d.py:208-225 (double_skip=False) on x[B, X*Y*Z, E]:  MLP(GN2(AFNO3D(GN1(x)))) + x"""
    B, tok, E = x.shape
    mh = f1w.shape[0]
    xn1 = GroupNormFn.apply(x, n1w, n1b, 8)
    y1 = AFNO3DFn.apply(xn1, w1, b1, w2, b2, dims3, nb, modes, act, packed)
    xn2 = GroupNormFn.apply(y1, n2w, n2b, 8)
    out = Mlp2Fn.apply(xn2.view(B * tok, E), f1w.view(mh, E), f1b, f2w.view(E, mh), f2b, act, x.reshape(B * tok, E), 0)
    return out.view(B, tok, E)


# ======================================================================================================
# CDPOT model (models/dpot_res.py): the anti-aliased activation and the plain stages around it
# ======================================================================================================
class AALReLUFn(torch.autograd.Function):
    """ops.aa_lrelu on a channels-last field x[N, h, w, C] with bias [Cb], C % Cb == 0: bilinear up by 2, LeakyReLU,
    anti-aliased bilinear down by 2, optionally bilinear up to out_size, + bias (the reference's LReLu_torch).  Keeps x and
    nothing of the up-sampled size: the backward recomputes the up-sampled field inside its kernel."""

    @staticmethod
    def forward(ctx, x, bias, out_size=None, slope: float = 0.01):
        x, bias = x.contiguous(), bias.contiguous()
        ctx.save_for_backward(x)
        ctx.Cb, ctx.slope = bias.shape[0], float(slope)
        return ops.aa_lrelu(x, bias, out_size, slope)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dx, dbias = ops.aa_lrelu_bwd(x, dy.contiguous(), ctx.Cb, ctx.slope)
        return dx, dbias, None, None


class LinearFn(torch.autograd.Function):
    """y[M, N] = x[M, K] W[N, K]^T + b (+ res): one Linear / 1x1 convolution.  res [R, N] with res_mod = R is added to row m as
    res[(m // res_div) % R] (a per-token table under rows (b, token, t): res_div = T)."""

    @staticmethod
    def forward(ctx, x, W, b, res=None, res_div: int = 0, res_mod: int = 0):
        ops.capture_precision(ctx)
        x, W = x.contiguous(), W.contiguous()
        res = res.contiguous() if res is not None else None
        y, _, _ = _dense_fwd(x, [(W, b)], 0, res, res_div, res_mod)
        ctx.save_for_backward(x, W)
        ctx.res_div, ctx.res_mod, ctx.has_res = res_div, res_mod, res is not None
        return y

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dy = dy.contiguous()
        dx, ((dW, db),) = _dense_bwd(dy, [x], [], [W], 0, ctx.needs_input_grad[0])
        dres = _res_bwd(dy, ctx.res_div, ctx.res_mod) if ctx.has_res and ctx.needs_input_grad[3] else None
        return dx, dW, db, dres, None, None


class ClsHeadFn(torch.autograd.Function):
    """cls_head on the token mean cm[B, E]: Linear, act, Linear, act, Linear (models/dpot_res.py:467-473)"""

    @staticmethod
    def forward(ctx, cm, c0w, c0b, c2w, c2b, c4w, c4b, act: int):
        ops.capture_precision(ctx)
        cls, ins, pres = _dense_fwd(cm.contiguous(), [(c0w, c0b), (c2w, c2b), (c4w, c4b)], act)
        ctx.save_for_backward(*ins, *pres, c0w, c2w, c4w)
        ctx.act = act
        return cls

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dcls):
        t = ctx.saved_tensors
        dcm, grads = _dense_bwd(dcls.contiguous(), t[0:3], t[3:5], t[5:8], ctx.act, ctx.needs_input_grad[0])
        return (dcm,) + sum(grads, ()) + (None,)


class PatchConvFn(torch.autograd.Function):
    """The k = s = P convolution of the 2-D patch embedding WITHOUT an activation, on the raw window x[B, X, Y, T, C]:
    ops.patchify (the three coordinate channels come from the tables gx, gy, gt) and one GEMM -> rows (b, hx, hy, t), hid
    columns.  x is kept, not the patch matrix: the backward gathers it again for the weight gradient."""

    @staticmethod
    def forward(ctx, x, gx, gy, gt, W, b, P: int):
        ops.capture_precision(ctx)
        x, W = x.contiguous(), W.contiguous()
        y, _, _ = _dense_fwd(lambda: ops.patchify(x, gx, gy, gt, P), [(W, b)], 0)
        ctx.save_for_backward(x, gx, gy, gt, W)
        ctx.P = P
        return y

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dy):
        x, gx, gy, gt, W = ctx.saved_tensors
        dA0, ((dW, db),) = _dense_bwd(dy.contiguous(), [lambda: ops.patchify(x, gx, gy, gt, ctx.P)], [], [W], 0,
                                      ctx.needs_input_grad[0])
        dx = None
        if dA0 is not None:
            B, X, Y, T, C = x.shape
            dx = ops.unpatchify(dA0, B, X, Y, T, C, ctx.P)
        return dx, None, None, None, dW, db, None


class TokenMeanFn(torch.autograd.Function):
    """x[B, tokens, E] -> the mean over the tokens [B, E]"""

    @staticmethod
    def forward(ctx, x):
        ctx.tok = x.shape[1]
        return ops.token_mean(x.contiguous())

    @staticmethod
    def backward(ctx, dy):
        return ops.token_mean_bwd(dy.contiguous(), ctx.tok)


# ======================================================================================================
# the FNO baselines (models/fno.py): csrc/fno.hip through ops.fno_*, csrc/fno3.hip through ops.fno3_*.  One forward and one
# backward serve both ranks and both forms (the spectral convolution alone, the whole layer); a rank is its four operators
# (rfft, irfft, mix, wgrad), looked up on `ops` when a pass runs, and its weight tuple
# ======================================================================================================
def _fno2_ops():
    return (ops.fno_rfft2, ops.fno_irfft2, lambda X, ws, adjoint=False: ops.fno_mix(X, *ws, adjoint),
            lambda X, dO, outs, acc: ops.fno_mix_wgrad(X, dO, *(outs or (None, None)), acc))


def _fno3_ops():
    return ops.fno3_rfft3, ops.fno3_irfft3, ops.fno3_mix, ops.fno3_mix_wgrad


def _fno_sizes(ws):
    """(Cout, modes) of two planar weights [2, Cin, Cout, m1, m2] or four real-pair weights [Cin, Cout, m1, m2, m3, 2]"""
    Cout, *modes = ws[0].shape[2:] if len(ws) == 2 else ws[0].shape[1:5]
    return Cout, modes


def _fno_wgrad(X, dO, sinks, wgrad, need: bool = True):
    """the spectral weights' gradients delivered: straight into the flat gradient slots where this is the step's first
    contribution, ADDED there by the kernel itself in a further pass of a rollout (every slot filled), else as temporaries;
    need=False (no weight takes a gradient, frozen spectral weights): nothing is launched"""
    if not need:
        for s in sinks:
            s.skip()
        return (None,) * len(sinks)
    outs, acc = [s.out() for s in sinks], False
    if any(o is None for o in outs):
        outs = None
        if all(s.fp is not None and s.fp.filled[s.i] for s in sinks):
            outs, acc = [s.fp.grad_views[s.i] for s in sinks], True
    return tuple(s.done(d) for s, d in zip(sinks, wgrad(X, dO, outs, acc)))


def _fno_forward(ctx, x, ws, fno_ops, cw=None, cb=None, act: int = 0):
    """SpectralConv2dFn / SpectralConv3dFn: irfft(mix(rfft(x))) on a channels-last field; with the 1x1 convolution (cw, cb),
    FNOLayerFn / FNO3dLayerFn: act(that + conv(x)) - the convolution is one GEMM whose result rides into the inverse
    transform's epilogue (add, activation).  Keeps the kept spectrum X; the layer keeps x and the pre-activation too."""
    rfft, irfft, mix, _ = fno_ops
    x, ws = x.contiguous(), tuple(w.contiguous() for w in ws)
    B, *dims, Cin = x.shape
    Cout, modes = _fno_sizes(ws)
    conv = None
    if cw is not None:
        cw = cw.contiguous()
        conv = ops.linear_fwd(x.view(-1, Cin), cw, cb)[0].view(B, *dims, Cout)
    X = rfft(x, *modes)
    y, pre = irfft(mix(X, ws), *dims, add=conv, act=act, save_pre=cw is not None)
    if cw is None:
        ctx.save_for_backward(X, *ws)
        ctx.sinks = _sinks(ctx, ws, 1)
    else:
        ctx.save_for_backward(X, *ws, x, pre, cw)
        ctx.sinks = _sinks(ctx, ws + (cw, cb), 1)
    ctx.act, ctx.n_weights = act, len(ws)
    return y


def _fno_backward(ctx, dy, fno_ops):
    """adjoint of _fno_forward: (dx, the spectral weights' gradients) and, for a layer, (dcw, dcb): dpre = dy act'(pre) is
    formed once, and the convolution's data gradient rides into the adjoint transform as its result rode into the forward's"""
    rfft, irfft, mix, wgrad = fno_ops
    X, *rest = ctx.saved_tensors
    n = ctx.n_weights
    ws, layer = tuple(rest[:n]), rest[n:]
    Cout, modes = _fno_sizes(ws)
    g = dy.contiguous()
    if layer:
        x, pre, cw = layer
        g = ops.act_bwd_mul(g, pre, ctx.act)
    dO = rfft(g, *modes, adjoint=True)
    dx = None
    if ctx.needs_input_grad[0]:
        dxc = ops.linear_bwd_data(g.view(-1, Cout), cw).view(x.shape) if layer else None
        dx, _ = irfft(mix(dO, ws, adjoint=True), *g.shape[1:-1], add=dxc, adjoint=True)
    grads = (dx,) + _fno_wgrad(X, dO, ctx.sinks[:n], wgrad, any(ctx.needs_input_grad[1:1 + n]))
    if layer:
        s_cw, s_cb = ctx.sinks[n:]
        dcw, dcb = ops.linear_bwd_wb(g.view(-1, Cout), x.view(-1, x.shape[-1]), s_cw.out(), s_cb.out())
        grads += (s_cw.done(dcw.view(cw.shape)), s_cb.done(dcb))
    return grads


class SpectralConv2dFn(torch.autograd.Function):
    """SpectralConv2d_fast (models/fno.py:14-53) on a channels-last field x[B, H, W, Cin] -> [B, H, W, Cout]: truncated rfft2,
    per-mode mixing with weights1 / weights2 [2, Cin, Cout, m1, m2], irfft2.  Keeps the kept spectrum X, not the field."""

    @staticmethod
    def forward(ctx, x, w1, w2):
        return _fno_forward(ctx, x, (w1, w2), _fno2_ops())

    @staticmethod
    def backward(ctx, dy):
        return _fno_backward(ctx, dy, _fno2_ops())


class FNOLayerFn(torch.autograd.Function):
    """One layer of FNO2d (models/fno.py:192-196): act(SpectralConv2d_fast(x) + Conv2d 1x1(x)) on x[B, H, W, Cin]."""

    @staticmethod
    def forward(ctx, x, w1, w2, cw, cb, act: int):
        ops.capture_precision(ctx)
        return _fno_forward(ctx, x, (w1, w2), _fno2_ops(), cw, cb, act)

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dy):
        return _fno_backward(ctx, dy, _fno2_ops()) + (None,)


class FNOEmbedFn(torch.autograd.Function):
    """PatchEmbed of FNO2d (models/fno.py:57-82) on x[B, X, Y, 1, K] (K = the T * C input planes; ops.patchify appends the
    coordinate channels): k = s = P convolution, act, 1x1 convolution, + res[b] (scale_feats, one row per sample) -> rows
    (b, hx, hy).  W0 [hid, (K + 3) P P] carries a zero column block for the third coordinate channel, which FNO2d lacks."""

    @staticmethod
    def forward(ctx, x, gx, gy, gt, W0, b0, W2, b2, res, P: int, act: int):
        ops.capture_precision(ctx)
        x, W0, W2 = x.contiguous(), W0.contiguous(), W2.contiguous()
        B, X, Y = x.shape[:3]
        tok = (X // P) * (Y // P)
        res = res.contiguous() if res is not None else None
        y, ins, pres = _dense_fwd(lambda: ops.patchify(x, gx, gy, gt, P), [(W0, b0), (W2, b2)], act, res, tok,
                                  B if res is not None else 0)
        ctx.save_for_backward(x, gx, gy, gt, ins[1], pres[0], W0, W2)
        ctx.P, ctx.act, ctx.tok, ctx.has_res = P, act, tok, res is not None
        return y

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dy):
        x, gx, gy, gt, Hh, Hpre, W0, W2 = ctx.saved_tensors
        dy = dy.contiguous()
        B, X, Y, T, K = x.shape
        dA0, ((dW0, db0), (dW2, db2)) = _dense_bwd(dy, [lambda: ops.patchify(x, gx, gy, gt, ctx.P), Hh], [Hpre], [W0, W2],
                                                   ctx.act, ctx.needs_input_grad[0])
        dx = ops.unpatchify(dA0, B, X, Y, T, K, ctx.P) if dA0 is not None else None
        dres = _res_bwd(dy, ctx.tok, B) if ctx.has_res and ctx.needs_input_grad[8] else None
        return dx, None, None, None, dW0, db0, dW2, db2, dres, None, None


class SpectralConv3dFn(torch.autograd.Function):
    """SpectralConv3d (models/fno.py:290-342) on a channels-last field x[B, X, Y, Z, Cin] -> [B, X, Y, Z, Cout]: truncated
    rfftn, per-mode mixing with the four corner weights [Cin, Cout, m1, m2, m3, 2] (real pairs), irfftn.  Keeps the kept
    spectrum, not the field."""

    @staticmethod
    def forward(ctx, x, w1, w2, w3, w4):
        return _fno_forward(ctx, x, (w1, w2, w3, w4), _fno3_ops())

    @staticmethod
    def backward(ctx, dy):
        return _fno_backward(ctx, dy, _fno3_ops())


class FNO3dLayerFn(torch.autograd.Function):
    """One layer of FNO3d (models/fno.py:407-411): act(SpectralConv3d(x) + Conv3d 1x1x1(x)) on x[B, X, Y, Z, Cin]."""

    @staticmethod
    def forward(ctx, x, w1, w2, w3, w4, cw, cb, act: int):
        ops.capture_precision(ctx)
        return _fno_forward(ctx, x, (w1, w2, w3, w4), _fno3_ops(), cw, cb, act)

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dy):
        return _fno_backward(ctx, dy, _fno3_ops()) + (None,)


# ======================================================================================================
# the UNet baseline (models/unet.py): csrc/unet.hip through ops.conv3x3 / bn_stats / bn_act / conv3x3_wgrad
# ======================================================================================================
def _deliver(sink, make):
    """a weight gradient delivered as _fno_wgrad delivers the spectral ones: `make(out, accumulate)` writes the flat slot where
    this is the step's first contribution, ADDS to it in a further pass of a rollout, else makes a temporary"""
    out, acc = sink.out(), False
    if out is None and sink.fp is not None and sink.fp.filled[sink.i]:
        out, acc = sink.fp.grad_views[sink.i], True
    return sink.done(make(out, acc))


class ConvBNActFn(torch.autograd.Function):
    """conv3x3 (no bias) -> BatchNorm2d -> act on a channels-last field x [B, H, W, Cin], one third of a UNet block
    (models/unet.py:534-564); pool=True returns (y, max_pool2d(y, 2, 2)), the encoder's last layer and the pooling after it.

    training=True: the batch statistics come out of the convolution's epilogue, and the same launch that merges them updates
    running_mean / running_var / num_batches_tracked in place (momentum 0.1, the unbiased variance).  Keeps x, z (the
    convolution's output), mean and invstd - not the normalised field, not y and no pooling indices: the backward recomputes
    them.  training=False: normalises with the running buffers and writes none of them; its backward raises."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, running_mean, running_var, num_batches_tracked, act: int, pool: bool, training: bool):
        x, w = x.contiguous(), w.contiguous()
        B, H, W, _ = x.shape
        ctx.training, ctx.act, ctx.pool = training, act, pool
        ctx.set_materialize_grads(False)
        if training:
            z, part = ops.conv3x3(x, w, stats=True)
            mean, invstd = ops.bn_stats(part, B * H * W, w.shape[0], running_mean, running_var, num_batches_tracked)
            del part
            ctx.save_for_backward(x, z, mean, invstd, w, gamma, beta)
            ctx.sinks = _sinks(ctx, (w, gamma, beta), 1)
            return ops.bn_act(z, mean, invstd, gamma, beta, act, pool)
        z = ops.conv3x3(x, w)
        return ops.bn_act(z, running_mean, running_var, gamma, beta, act, pool, stat_is_var=True)

    @staticmethod
    def backward(ctx, dy, dpool=None):
        if not ctx.training:
            raise RuntimeError("ConvBNActFn.backward: the forward ran in eval mode (running statistics); a backward through it "
                               "is not built - call model.train() before a step that differentiates")
        x, z, mean, invstd, w, gamma, beta = ctx.saved_tensors
        s_w, s_g, s_b = ctx.sinks
        if dy is None and dpool is None:
            for s in ctx.sinks:
                s.skip()
            return (None,) * 10
        dy = dy.contiguous() if dy is not None else None
        dpool = dpool.contiguous() if dpool is not None else None
        o_g, o_b = s_g.out(), s_b.out()
        dz, dgamma, dbeta = ops.bn_act_bwd(dy, dpool, z, mean, invstd, gamma, beta, ctx.act, out_dgamma=o_g, out_dbeta=o_b)
        dgamma, dbeta = s_g.done(dgamma), s_b.done(dbeta)
        dw = None
        if ctx.needs_input_grad[1]:
            dw = _deliver(s_w, lambda out, acc: ops.conv3x3_wgrad(x, dz, out, acc))
        else:
            s_w.skip()
        dx = ops.conv3x3_bwd_data(dz, w) if ctx.needs_input_grad[0] else None
        return dx, dw, dgamma, dbeta, None, None, None, None, None, None


class UpConv2Fn(torch.autograd.Function):
    """ConvTranspose2d(k = s = 2) on a channels-last field x [B, h, w, Cin] -> [B, 2 h, 2 w, Cout]: one GEMM of the pixel rows
    with the parameter W [Cin, Cout, 2, 2] read in place as a [Cin, 4 Cout] matrix, then ops.unet_upshuffle (+ bias)."""

    @staticmethod
    def forward(ctx, x, W, b):
        ops.capture_precision(ctx)
        x, W = x.contiguous(), W.contiguous()
        B, h, w, Cin = x.shape
        Cout = W.shape[1]
        Z = ops.linear_bwd_data(x.view(-1, Cin), W.view(Cin, 4 * Cout))                  # [B h w, 4 Cout] = x @ W
        ctx.save_for_backward(x, W)
        ctx.sinks = _sinks(ctx, (W, b), 1)
        return ops.unet_upshuffle(Z, B, h, w, Cout, bias=b)

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        B, h, w, Cin = x.shape
        Cout = W.shape[1]
        s_w, s_b = ctx.sinks
        dy = dy.contiguous()
        db = s_b.done(ops.colsum(dy.view(-1, Cout), B * h * w * 4, Cout, out=s_b.out()))
        dZ = ops.unet_upshuffle(dy, B, h, w, Cout, inverse=True)                         # [B h w, 4 Cout]
        dW = ops.linear_bwd_weight(x.view(-1, Cin), dZ, out=s_w.out())                   # [Cin, 4 Cout] = x^T dZ
        dW = s_w.done(dW.view(W.shape))
        dx = ops.linear_fwd(dZ, W.view(Cin, 4 * Cout), None)[0].view(x.shape) if ctx.needs_input_grad[0] else None
        return dx, dW, db
