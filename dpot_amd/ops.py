"""Tensor-level wrappers over the C ABI (include/dpot_hip.h).

PyTorch is used here only as the owner of device memory and of the HIP stream: every function takes
contiguous fp32 CUDA tensors, passes ``data_ptr()`` / sizes / the current stream to libdpot_hip.so and returns
tensors.  There is deliberately no CPU or eager-PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import contextlib
import functools
import math
import threading
import os
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import GemmDesc, check

Tensor = torch.Tensor

ACT_IDS = {None: 0, "none": 0, "gelu": 1, "tanh": 2, "sigmoid": 3, "relu": 4, "leaky_relu": 5, "softplus": 6,
           "ELU": 7, "silu": 8}
EPI_LINEAR, EPI_ACT, EPI_DACT, EPI_AFNO_WGRAD = 0, 1, 2, 3
GEMM_F32, GEMM_BF16X6, GEMM_AUTO, GEMM_BF16 = 0, 1, 2, 3
_PRECISIONS = {"f32": GEMM_F32, "bf16x6": GEMM_BF16X6, "auto": GEMM_AUTO, "bf16": GEMM_BF16}
# how every GEMM forms its fp32 products (include/dpot_hip.h: dpot_gemm_desc.precision);
# DPOT_GEMM_PRECISION = f32 | bf16x6 | auto
_gemm_precision = _PRECISIONS[os.environ.get("DPOT_GEMM_PRECISION", "f32")]


def set_gemm_precision(name: str) -> None:
    """'f32' = native fp32 MFMA, 'bf16x6' = fp32 emulated by 3-way bf16 operand splitting (fp32-level accuracy),
    'auto' = per shape, whichever of the two is faster (the library's rule)"""
    global _gemm_precision
    _gemm_precision = _PRECISIONS[name]


def gemm_precision() -> str:
    return {v: k for k, v in _PRECISIONS.items()}[_cur_gemm()]


# precision of the channel-MLP GEMMs only (Block.mlp, models/dpot.py:157-161); None = follow the global setting.
# BASELINE.json configs[2] asks for a "bf16 channel-MLP on MFMA": 'bf16x6' here puts exactly those GEMMs on the bf16
# matrix cores at fp32 accuracy; 'bf16' is the plain reduced-precision form (operands rounded to bf16, fp32
# accumulation - NOT within the 1e-4 parity tolerance, opt-in only).   DPOT_MLP_PRECISION = f32 | bf16x6 | auto | bf16
_mlp_precision = _PRECISIONS[os.environ["DPOT_MLP_PRECISION"]] if os.environ.get("DPOT_MLP_PRECISION") else None


def set_mlp_precision(name: Optional[str]) -> None:
    global _mlp_precision
    _mlp_precision = None if name is None else _PRECISIONS[name]


# per-THREAD overrides of the two process defaults above, set by the scopes below (round 5; ADVICE r4: the per-model
# precision used to be a temporary write to the process-global, visible to a backward of another model running on autograd's
# device thread at the same time).  A model applies its attributes around its own forward / weight derivation; every autograd
# Function captures the effective values in its context and re-applies them around its backward, whatever thread runs it.
_tls = threading.local()
_UNSET = object()


def _cur_gemm() -> int:
    v = getattr(_tls, "gemm", None)
    return _gemm_precision if v is None else v


def _cur_mlp() -> Optional[int]:
    v = getattr(_tls, "mlp", _UNSET)
    return _mlp_precision if v is _UNSET else v


def _code(prec) -> int:
    return _PRECISIONS[prec] if isinstance(prec, str) else int(prec)


@contextlib.contextmanager
def mlp_precision_scope(prec):
    """the channel-MLP precision of ONE model while its kernels are being enqueued: `DPOTNet.mlp_precision` (a
    per-model attribute: 'f32' | 'bf16x6' | 'auto' | 'bf16' | None = the process default above) is applied around the
    model's forward, its weight derivation and - through the value captured in the autograd context - its backward, so two
    models of one process can run different modes and nothing leaks to the next caller or to another thread.  prec: a name,
    a precision code or None (= leave the current setting)."""
    if prec is None:
        yield
        return
    prev = getattr(_tls, "mlp", _UNSET)
    _tls.mlp = _code(prec)
    try:
        yield
    finally:
        if prev is _UNSET:
            del _tls.mlp
        else:
            _tls.mlp = prev


@contextlib.contextmanager
def gemm_precision_scope(prec):
    """the same for the GEMM precision of everything OUTSIDE the channel MLP (`DPOTNet.gemm_precision`: 'f32' | 'bf16x6' |
    'auto' | None = the process default of set_gemm_precision / DPOT_GEMM_PRECISION)"""
    if prec is None:
        yield
        return
    prev = getattr(_tls, "gemm", None)
    _tls.gemm = _code(prec)
    try:
        yield
    finally:
        _tls.gemm = prev


@contextlib.contextmanager
def precision_scope(gemm=None, mlp=None):
    with gemm_precision_scope(gemm), mlp_precision_scope(mlp):
        yield


def with_ctx_precision(backward):
    """decorator for torch.autograd.Function.backward: re-apply the precisions the forward captured in ctx.gemm_precision /
    ctx.mlp_precision (see capture_precision) - autograd runs backward on its own thread, long after the model's scope"""
    @functools.wraps(backward)
    def wrapper(ctx, *grads):
        with precision_scope(getattr(ctx, "gemm_precision", None), getattr(ctx, "mlp_precision", None)):
            return backward(ctx, *grads)
    return wrapper


def capture_precision(ctx) -> None:
    """store the precisions in effect on this thread in an autograd context (forward side of with_ctx_precision)"""
    ctx.gemm_precision = _cur_gemm()
    # the EFFECTIVE channel-MLP precision as a concrete code: an unset override (None = "follow the GEMM precision")
    # would make the backward's scope a no-op and let it read whatever the autograd thread's default is by then
    ctx.mlp_precision = effective_mlp_precision()


def effective_mlp_precision() -> int:
    """precision the channel-MLP GEMMs run in: the override if set, else the GEMM precision in effect"""
    m = _cur_mlp()
    return m if m is not None else _cur_gemm()


def mlp_precision() -> Optional[int]:
    return _cur_mlp()


# ---- DPOT_TUNE: the ONE switchboard of the fallback-path selectors (round 6; rounds 1-5 grew 43 separate DPOT_* variables) ------
# DPOT_TUNE="key=val,key=val" (integers).  Every key selects a PREVIOUS-GENERATION path that stays under the GPU test gate
# (tests/test_gpu_optout.py runs parity subsets under them); the defaults are what measured fastest.  The C side reads the same
# variable once per process (csrc/core.hip dpot::tune); this side looks at it per call and parses it when it has changed.
# Besides DPOT_TUNE the package reads only DPOT_HIP_LIB (library path), DPOT_GEMM_PRECISION and DPOT_MLP_PRECISION (process
# defaults of the precision modes).
TUNE_KEYS = {
    "mixer": (3, "AFNO mixer MLP: 3 = three-product fused kernel (afno_mlp3), 4 = four-product fused kernel (afno_mlp2), "
                 "0 = two generic GEMM launches"),
    "afno_layer": (-1, "one-launch AFNO layer forward (afno_fused_fwd): -1 = where it measured faster (>= 80 % full last "
                       "round of (sample, block) workgroups), 0 = never, 1 = wherever supported"),
    "gn_fuse": (1, "0 = GroupNorm as its own kernels: not fused with the mixer's DFTs, never applied on the load of its consumer"),
    "panel": (1, "0 = generic GEMM kernels instead of the pre-packed-weight panel GEMM, the token-contraction weight-gradient "
                 "kernels (gemm_tn) and their two-layer launches"),
    "wgrad_gauss": (1, "0 = four-product AFNO weight gradients instead of the three-product forms"),
    "bf16p_bd": (1, "0 = the LDS-DMA bf16 GEMM kernels of rounds 2-3 for every launch instead of the B-direct kernels"),
    "bf16p_shape": (1, "0 = none of the bf16 GEMM shape heuristics: 128 x 256 tiles only, column-major tile order, eight waves, "
                       "un-paired weight gradients"),
    "packs": (1, "0 = bf16 packs by separate pack passes only: none from the one-launch AFNO layer, the GroupNorm backward or Adam"),
    "pack_both": (1, "0 = bf16 channel MLP without the pack-both path (one pack pass per operand form, fp32 pre-activation saved)"),
    "fused_small": (5, "0 = separate small launches: per-block reduce launches, eight layout launches, torch ops for the cls head; "
                       "2 = as 1, but the blocks' weight gradients and their finalising launch per block instead of batched; "
                       "3 = as 1 with the batched launches cut by the one-round rules (another summation order); "
                       "4 = as 1 with the batched launches on the library's own stream beside the embed backward "
                       "(ops.wgrad_flush_async); 5 = as 4 with the step's latency-bound side chains on the library's side lane "
                       "(ops.side_lane: the weight-only prologue beside the embed forward, the first conv's gradients beside the "
                       "weight-only chain of the embed backward); 1 = the batched launches on the step's stream, one after the other"),
    "embed_implicit": (1, "0 = explicit patch matrix + GEMM instead of the implicit-GEMM patch embedding"),
    "mixer6": (1, "bf16x6 mixer kernel afno_mlp6 under gemm_precision 'auto' / 'bf16x6': 1 = where it measured faster (96 channels "
                  "per block: DPOT-L), 2 = wherever supported (also 128), 0 = never (the fp32 matrix-core kernels)"),
}


# (the DPOT_TUNE string, its parse): re-parsed only when the variable's string changes.  The dict IS the cache: read it only
_tune_parsed = ("", {})


def _parse_tune():
    global _tune_parsed
    env = os.environ.get("DPOT_TUNE", "")
    if env == _tune_parsed[0]:
        return _tune_parsed[1]
    out = {}
    for kv in env.split(","):
        kv = kv.strip()
        if not kv:
            continue
        k, _, v = kv.partition("=")
        if k not in TUNE_KEYS:
            raise ValueError(f"DPOT_TUNE: unknown key {k!r} (known: {', '.join(TUNE_KEYS)})")
        out[k] = int(v)
    _tune_parsed = (env, out)
    return out


def tune(key: str, default: Optional[int] = None) -> int:
    """value of `key` in DPOT_TUNE, else its default (TUNE_KEYS)"""
    d = TUNE_KEYS[key][0] if default is None else default
    return _parse_tune().get(key, d)


def _step_stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _stream() -> int:
    """the stream every launch of this module goes to: torch's current stream, or - inside a lane block of this thread
    (`_Lane.block`) - that lane of the library"""
    cur = getattr(_tls, "lane", None)
    return _step_stream() if cur is None else cur[1]


def _hold(*tensors) -> None:
    """inside a lane block of this thread: keep `tensors` referenced until the lane's join has been issued"""
    cur = getattr(_tls, "lane", None)
    if cur is not None:
        with _lane_lock:
            cur[0].held.extend(tensors)


def _scratch(t: Tensor) -> Tensor:
    """a workspace that its op drops when it returns.  On the step's stream the allocator may hand it out again at once (stream
    order protects it); inside a lane block it stays referenced until the join has been issued."""
    _hold(t)
    return t


def _req(t: Tensor, name: str = "tensor") -> Tensor:
    if not t.is_cuda:
        raise _lib.DpotHipError(f"{name} must live on the MI355X (got a {t.device} tensor): dpot_amd has no CPU path")
    if t.dtype != torch.float32:
        raise _lib.DpotHipError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.DpotHipError(f"{name} must be contiguous")
    return t


def _p(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------------
def auto_splitk(M: int, N: int, K: int, batch: int = 1, precision: Optional[int] = None, tn: bool = False) -> int:
    """split-K factor for a GEMM; tn: a weight gradient (transA, not transB) - in native fp32 those run on the kernel
    of csrc/gemm_tn.hip, which wants one 128x128 workgroup per CU"""
    lib = _lib.load()
    prec = _cur_gemm() if precision is None else precision
    if tn and prec == GEMM_F32:
        s = lib.dpot_gemm_tn_splitk(M, N, K, batch)
        if s > 0:
            return s
    return lib.dpot_gemm_auto_splitk2(M, N, K, batch, prec)


def gemm(A: Tensor, B: Tensor, C_: Tensor, M: int, N: int, K: int, *, transA: bool = False, transB: bool = False,
         lda: int, ldb: int, ldc: int, batch: int = 1, strideA: int = 0, strideB: int = 0, strideC: int = 0,
         bias: Optional[Tensor] = None, strideBias: int = 0, act: int = 0, mode: int = EPI_LINEAR,
         aux: Optional[Tensor] = None, ldaux: int = 0, strideAux: int = 0,
         preact: Optional[Tensor] = None, ldpre: int = 0, stridePre: int = 0,
         res: Optional[Tensor] = None, ldres: int = 0, res_div: int = 0, res_mod: int = 0, strideRes: int = 0,
         accumulate: bool = False, splitk: Optional[int] = None, tile: int = 0, tag: int = 0,
         colsum_out: Optional[Tensor] = None, colsum_of: int = 0, strideColsum: int = 0,
         precision: Optional[int] = None) -> Tensor:
    """C = epilogue(A @ B) on the matrix cores; see include/dpot_hip.h for the exact semantics."""
    lib = _lib.load()
    d = GemmDesc()
    d.A, d.B, d.C = A.data_ptr(), B.data_ptr(), C_.data_ptr()
    d.M, d.N, d.K, d.batch = M, N, K, batch
    d.transA, d.transB = int(transA), int(transB)
    d.lda, d.ldb, d.ldc = lda, ldb, ldc
    d.strideA, d.strideB, d.strideC = strideA, strideB, strideC
    d.bias, d.strideBias = _p(bias), strideBias
    d.act, d.epi_mode = act, mode
    d.aux, d.ldaux, d.strideAux = _p(aux), ldaux, strideAux
    d.preact, d.ldpre, d.stridePre = _p(preact), ldpre, stridePre
    d.res, d.ldres, d.res_div, d.res_mod, d.strideRes = _p(res), ldres, res_div, res_mod, strideRes
    d.accumulate = int(accumulate)
    d.tile = tile
    d.tag = tag
    d.precision = _cur_gemm() if precision is None else precision
    if splitk is None:
        # launches that cannot fill the chip (<= 128 output tiles: the embed fold's T small products, the cls head,
        # pos-embed terms) are latency bound - spread their K over more workgroups; big grids stay un-split
        small = ((M + 63) // 64) * ((N + 63) // 64) * batch <= 128
        splitk = auto_splitk(M, N, K, batch, precision=d.precision) if small else 1
    d.colsum_out, d.colsum_of, d.strideColsum = _p(colsum_out), (colsum_of if colsum_out is not None else 0), strideColsum
    ws = None
    if splitk > 1:
        L = M if d.colsum_of == 1 else N if d.colsum_of == 2 else 0
        ws = _scratch(torch.empty(splitk * batch * (M * N + L), dtype=torch.float32, device=A.device))
        d.splitk, d.workspace = splitk, ws.data_ptr()
    else:
        d.splitk, d.workspace = 1, None
    check(lib.dpot_gemm_f32(C.byref(d), _stream()), "gemm_f32")
    return C_


# ------------------------------------------------------------------------------------------------------
# panel GEMM with pre-packed static weights (csrc/gemm_panel.hip)
# ------------------------------------------------------------------------------------------------------
def panel_enabled() -> bool:
    """the panel kernel is an fp32 kernel: used while the global GEMM precision is 'f32' (the channel-MLP override of
    set_mlp_precision is checked where it applies, functional._mlp_panel_ok)"""
    return tune("panel") != 0 and _cur_gemm() == GEMM_F32


def gemm_panel_supported(M: int, N: int, K: int) -> bool:
    return bool(_lib.load().dpot_gemm_panel_supported(M, N, K))


def _device_table(struct, entries, dev) -> Tensor:
    """job table of a one-launch kernel: one ctypes `struct` per entry (a tuple of its fields in _lib's order), as raw bytes
    in device memory"""
    import numpy as np
    arr = (struct * len(entries))(*(struct(*e) for e in entries))
    return torch.from_numpy(np.frombuffer(bytearray(arr), dtype=np.uint8)).to(dev)


class PanelPacks:
    """Fragment-block-major copies of a set of static weights, refreshed by ONE launch (dpot_panel_pack_weights) from a
    job table that lives in device memory.  jobs = [(src tensor, rows, K, ld, trans)]; the destination buffers are
    allocated once, so the table stays valid while the sources do not move.  refresh() always launches: whether a set
    is still fresh is decided by its owner (packs.ModelPacks)."""

    def __init__(self, jobs, bf16: bool = False, planes: int = 1):
        dev = jobs[0][0].device
        self.bf16 = bf16
        self.planes = planes if bf16 else 0       # 1: plain bf16, 3: bf16x6 split (fp32-accurate)
        if bf16:       # csrc/gemm_bf16p.hip: rows padded to 32, bf16 elements, `planes` planes per 16-k block
            lib = _lib.load()
            self.bufs = [torch.empty(lib.dpot_bf16_packed_elems(rows, K, planes), dtype=torch.bfloat16, device=dev)
                         for _, rows, K, _, _ in jobs]
        else:
            self.bufs = [torch.empty(rows * K, dtype=torch.float32, device=dev) for _, rows, K, _, _ in jobs]
        self.table = _device_table(_lib.PackJob, [(src.data_ptr(), dst.data_ptr(), rows, K, ld, int(trans))
                                                  for (src, rows, K, ld, trans), dst in zip(jobs, self.bufs)], dev)
        self.n = len(jobs)
        self.max_elems = max(rows * K for _, rows, K, _, _ in jobs)
        self.jobs = list(jobs)                    # (the table holds raw pointers: this also keeps the sources alive)

    def refresh(self) -> None:
        lib = _lib.load()
        if self.bf16:
            check(lib.dpot_bf16_pack_jobs(self.table.data_ptr(), self.n, self.max_elems, self.planes, _stream()),
                  "bf16_pack_jobs")
        else:
            check(lib.dpot_panel_pack_weights(self.table.data_ptr(), self.n, self.max_elems, _stream()), "pack_weights")


class LayoutJobs:
    """Small weight-only layout products (zero-padded copies, small transposes, bias broadcasts, "+ bias") refreshed by ONE
    launch (dpot_layout_jobs) from a device-resident table.  jobs = [(src, add | None, (d0, d1, d2), (v0, v1, v2),
    (s0, s1, s2))]: out[i0, i1, i2] = (inside v ? src.flat[i0 s0 + i1 s1 + i2 s2] : 0) + (add[i2] if add is not None).
    self.out[i]: persistent [d0, d1, d2] tensors (the table stays valid while the sources do not move)."""

    def __init__(self, jobs):
        dev = jobs[0][0].device
        self.out = [torch.empty(d, dtype=torch.float32, device=dev) for _, _, d, _, _ in jobs]
        self.sources = [(j[0], j[1]) for j in jobs]        # the table holds raw pointers: keep the tensors alive
        self.table = _device_table(_lib.LayoutJob, [(src.data_ptr(), _p(add), dst.data_ptr(), *d, *v, *st)
                                                    for (src, add, d, v, st), dst in zip(jobs, self.out)], dev)
        self.n = len(jobs)
        self.max_elems = max(d[0] * d[1] * d[2] for _, _, d, _, _ in jobs)

    def refresh(self):
        check(_lib.load().dpot_layout_jobs(self.table.data_ptr(), self.n, self.max_elems, _stream()), "layout_jobs")
        return self.out


def gemm_panel(A: Tensor, Wpacked: Tensor, N: int, *, bias: Optional[Tensor] = None, act: int = 0,
               mode: int = EPI_LINEAR, aux: Optional[Tensor] = None, res: Optional[Tensor] = None,
               save_pre: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """C[M,N] = epilogue(A[M,K] @ Wt^T), Wt packed by PanelPacks (rows = N).  Returns (C, pre | None)."""
    M, K = A.shape
    out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    pre = torch.empty_like(out) if save_pre else None
    check(_lib.load().dpot_gemm_panel(A.data_ptr(), A.stride(0), Wpacked.data_ptr(), _p(bias), _p(aux),
                                      aux.stride(0) if aux is not None else 0, _p(res),
                                      res.stride(0) if res is not None else 0, _p(pre), N, out.data_ptr(), N, M, N, K,
                                      act, mode, _stream()), "gemm_panel")
    return out, pre


def gemm_bf16p_supported(M: int, N: int, K: int) -> bool:
    return bool(_lib.load().dpot_gemm_bf16p_supported(M, N, K))


class MlpPacks(tuple):
    """(W1, W1^T, W2, W2^T) packed for one of the pre-packed-weight GEMM kernels; kind = 'f32' (csrc/gemm_panel.hip),
    'bf16' (csrc/gemm_bf16p.hip, 1 plane: reduced precision) or 'bf16x6' (3 planes: fp32-accurate)"""

    def __new__(cls, bufs, kind: str):
        self = super().__new__(cls, bufs)
        self.kind = kind
        return self

    @property
    def planes(self) -> int:
        return {"f32": 0, "bf16": 1, "bf16x6": 3}[self.kind]


def bf16_pack_rows(x: Tensor, trans: bool = False, planes: int = 1) -> Tensor:
    """fp32 [M, K] -> bf16 fragment-block-major operand of gemm_bf16p (one pass; rows padded to 32 with zeros).
    trans: pack x^T instead (x stored [K, rows]: weight gradients - rows = features, k = tokens);
    planes = 3: the three-plane bf16x6 split"""
    lib = _lib.load()
    if trans:
        K, M = x.shape
    else:
        M, K = x.shape
    out = torch.empty(lib.dpot_bf16_packed_elems(M, K, planes), dtype=torch.bfloat16, device=x.device)
    check(lib.dpot_bf16_pack_rows(x.data_ptr(), x.stride(0), M, K, int(trans), planes, out.data_ptr(), _stream()),
          "bf16_pack_rows")
    return out


def bf16_pack_both_supported(rows: int, K: int) -> bool:
    return bool(_lib.load().dpot_bf16_pack_both_supported(rows, K))


def bf16_pack_both(x: Tensor, want_rows: bool = True, want_trans: bool = True, colsum_out: Optional[Tensor] = None,
                   want_colsum: bool = False, norm=None, defer_colsum: bool = False):
    """one pass over x [M, K] fp32 -> (row-form pack | None, transposed pack | None, column sums | None): the two operand
    forms the bf16 channel MLP needs of an activation (data GEMM and weight gradient) and its bias gradient.
    norm = (mean [B,G], rstd [B,G], gamma [K], beta [K], rows_per_sample): the packs of GroupNorm(x) with those statistics
    (rows_per_sample % 64 == 0), applied on the load - no column sums in that form"""
    lib = _lib.load()
    M, K = x.shape
    pr = torch.empty(lib.dpot_bf16_packed_elems(M, K, 1), dtype=torch.bfloat16, device=x.device) if want_rows else None
    pt = torch.empty(lib.dpot_bf16_packed_elems(K, M, 1), dtype=torch.bfloat16, device=x.device) if want_trans else None
    if norm is not None:
        mean, rstd, gamma, beta, rps = norm
        assert not want_colsum
        check(lib.dpot_bf16_pack_both_norm(x.data_ptr(), x.stride(0), M, K, mean.data_ptr(), rstd.data_ptr(),
                                           gamma.data_ptr(), beta.data_ptr(), rps, mean.shape[1], _p(pr), _p(pt), _stream()),
              "bf16_pack_both_norm")
        return pr, pt, None
    part = torch.empty(M // 64, K, dtype=torch.float32, device=x.device) if want_colsum else None
    check(lib.dpot_bf16_pack_both(x.data_ptr(), x.stride(0), M, K, _p(pr), _p(pt), _p(part), _stream()), "bf16_pack_both")
    if want_colsum and defer_colsum:      # the column sums are left as partials: (part, rows, N, out) for `block_finalize`
        return pr, pt, (part, M // 64, K, _out(colsum_out, (K,), x.device))
    cs = colsum(part, M // 64, K, out=colsum_out) if want_colsum else None
    return pr, pt, cs


def gemm_bf16p(Ap: Tensor, Wp: Tensor, M: int, N: int, K: int, *, bias: Optional[Tensor] = None, act: int = 0,
               mode: int = EPI_LINEAR, aux: Optional[Tensor] = None, res: Optional[Tensor] = None,
               save_pre: bool = False, out: Optional[Tensor] = None, splitk: Optional[int] = None,
               planes: int = 1) -> Tuple[Tensor, Optional[Tensor]]:
    """C[M,N] fp32 = epilogue(A @ Wt^T) on the bf16 matrix cores; Ap / Wp: packed bf16 operands (bf16_pack_rows, or a
    bf16 PanelPacks buffer) with the same number of planes (1: plain bf16, 3: bf16x6 = fp32-accurate).
    splitk=None: the library's choice (weight gradients use split-K).  Returns (C, pre | None)."""
    C_, pre, _, _, _ = gemm_bf16p_packed(Ap, Wp, M, N, K, bias=bias, act=act, mode=mode, aux=aux, res=res,
                                         save_pre=save_pre, out=out, splitk=splitk, planes=planes)
    return C_, pre


def gemm_bf16p_pair_wanted(M0: int, N0: int, M1: int, N1: int, K: int) -> bool:
    return bool(_lib.load().dpot_gemm_bf16p_pair_wanted(M0, N0, M1, N1, K))


BF16P_KERNEL_KINDS = {0: "dpot::gemm_bf16p_kernel (8 compute + 4 loader waves, LDS-DMA)",
                      1: "dpot::gemm_bf16p_duo_kernel (two 8-wave workgroups per CU)",
                      2: "dpot::gemm_bf16p_bd_kernel<8,1,3> (B-direct: W fragments straight from global memory into registers, "
                         "only the A panel through LDS; eight 128 x 32 waves)",
                      3: "dpot::gemm_bf16p_bd_kernel<8,2,3> (B-direct: W fragments straight from global memory into registers, "
                         "only the A panel through LDS; four 128 x 64 waves, two workgroups per CU)",
                      4: "dpot::gemm_bf16x6p_kernel (fp32-accurate three-plane split)"}


def gemm_bf16p_kernel_name(M: int, N: int, K: int, splitk: int = 1, planes: int = 1, packed_outputs: bool = False) -> str:
    """the kernel dpot_gemm_bf16p runs for this shape, from the library's own selection (dpot_gemm_bf16p_kernel_kind)"""
    k = _lib.load().dpot_gemm_bf16p_kernel_kind(M, N, K, splitk, planes, int(packed_outputs))
    return BF16P_KERNEL_KINDS.get(k & 7, f"kind {k}") + (" on 128 x 192 tiles" if k >= 8 else "")


class Bf16pPlan(NamedTuple):
    """launch plan of dpot_gemm_bf16p (include/dpot_hip.h, dpot_gemm_bf16p_plan)"""
    kind: int              # 0 LDS-DMA, 2 B-direct eight waves, 3 B-direct four waves, 4 bf16x6; + 8 on 128 x 192 tiles
    tilesM: int
    tilesN: int            # of 192 columns when kind >= 8
    splits: int
    slabs_per_split: int
    super_r: int           # > 0: super-blocks of super_r x super_c tiles, grid padded to rounds of 256 workgroups
    super_c: int           # with super_r == 0: 1 = row-major XCD-contiguous order, 0 = column-major
    grid: int


class Bf16pPairPlan(NamedTuple):
    """launch plan of dpot_gemm_bf16p_pair (dpot_gemm_bf16p_pair_plan)"""
    kind: int              # 0, 2 or 3 as above; + 8 on 128 x 192 tiles
    splits: int
    slabs_per_split: int
    row_major0: int
    row_major1: int
    grid: int


def gemm_bf16p_plan(M: int, N: int, K: int, splitk: int = 1, planes: int = 1,
                    packed_outputs: bool = False) -> Optional[Bf16pPlan]:
    """the plan dpot_gemm_bf16p launches with, from the library's own selection (host only); None: the launch refuses"""
    buf = (C.c_int * 8)()
    n = _lib.load().dpot_gemm_bf16p_plan(M, N, K, splitk, planes, int(packed_outputs), buf, 8)
    return Bf16pPlan(*buf[:8]) if n == 8 else None


def gemm_bf16p_pair_plan(M0: int, N0: int, M1: int, N1: int, K: int, splitk: int = 1) -> Optional[Bf16pPairPlan]:
    """the plan dpot_gemm_bf16p_pair launches with for an explicit splitk (host only); None: the launch refuses"""
    buf = (C.c_int * 6)()
    n = _lib.load().dpot_gemm_bf16p_pair_plan(M0, N0, M1, N1, K, splitk, buf, 6)
    return Bf16pPairPlan(*buf[:6]) if n == 6 else None


def gemm_bf16p_pair(A0: Tensor, W0: Tensor, M0: int, N0: int, A1: Tensor, W1: Tensor, M1: int, N1: int, K: int,
                    out0: Optional[Tensor] = None, out1: Optional[Tensor] = None,
                    splitk: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """(A0 W0^T [M0,N0], A1 W1^T [M1,N1]) on the bf16 matrix cores in ONE launch (packed plain-bf16 operands, common K,
    one common split-K factor - None: the library's choice): the two channel-MLP weight gradients of a block."""
    lib = _lib.load()
    C0 = _out(out0, (M0, N0), A0.device)
    C1 = _out(out1, (M1, N1), A1.device)
    sk = max(1, lib.dpot_gemm_bf16p_pair_splitk(M0, N0, M1, N1, K)) if splitk is None else splitk
    ws = torch.empty(sk * (M0 * N0 + M1 * N1), dtype=torch.float32, device=A0.device) if sk > 1 else None
    check(lib.dpot_gemm_bf16p_pair(A0.data_ptr(), W0.data_ptr(), C0.data_ptr(), N0, M0, N0, A1.data_ptr(), W1.data_ptr(),
                                   C1.data_ptr(), N1, M1, N1, K, sk, _p(ws), _stream()), "gemm_bf16p_pair")
    return C0, C1


def gemm_bf16p_packed(Ap: Tensor, Wp: Tensor, M: int, N: int, K: int, *, bias: Optional[Tensor] = None, act: int = 0,
                      mode: int = EPI_LINEAR, aux: Optional[Tensor] = None, res: Optional[Tensor] = None,
                      save_pre: bool = False, out: Optional[Tensor] = None, splitk: Optional[int] = None,
                      planes: int = 1, pack_rows: bool = False, pack_trans: bool = False, colsum: bool = False,
                      colsum_out: Optional[Tensor] = None, store: bool = True, save_dact: bool = False,
                      dact: Optional[Tensor] = None, defer_colsum: bool = False):
    """gemm_bf16p whose epilogue can ALSO emit the packed forms of the output and its column sums
    (pack_rows / pack_trans / colsum: planes == 1, M % 32 == 0, no split-K); store=False skips the fp32 output.
    save_dact (EPI_ACT): instead of the fp32 pre-activation, the second return value is act'(pre) as a packed bf16
    tensor - pass it as `dact` to the EPI_DACT launch of the backward (replaces aux).
    Always returns (C | None, pre or act' pack | None, row pack | None, transposed pack | None, column sums | None)."""
    lib = _lib.load()
    packs = pack_rows or pack_trans or colsum or save_dact or dact is not None
    C_ = _out(out, (M, N), Ap.device) if (store or not packs) else None
    pre = torch.empty(M, N, dtype=torch.float32, device=Ap.device) if save_pre else None
    if splitk is None:
        splitk = 1 if packs else lib.dpot_gemm_bf16p_splitk(M, N, K)
    ws = torch.empty(splitk * M * N, dtype=torch.float32, device=Ap.device) if splitk > 1 else None
    pr = torch.empty(lib.dpot_bf16_packed_elems(M, N, 1), dtype=torch.bfloat16, device=Ap.device) if pack_rows else None
    pt = torch.empty(lib.dpot_bf16_packed_elems(N, M, 1), dtype=torch.bfloat16, device=Ap.device) if pack_trans else None
    part = torch.empty(M // 32, N, dtype=torch.float32, device=Ap.device) if colsum else None
    dout = torch.empty(lib.dpot_bf16_packed_elems(M, N, 1), dtype=torch.bfloat16, device=Ap.device) if save_dact else None
    check(lib.dpot_gemm_bf16p(Ap.data_ptr(), Wp.data_ptr(), _p(bias), _p(aux),
                              aux.stride(0) if aux is not None else 0, _p(res),
                              res.stride(0) if res is not None else 0, _p(pre), N, _p(C_), N, M, N, K,
                              act, mode, planes, splitk, _p(ws), _p(pr), _p(pt), _p(part), _p(dout), _p(dact),
                              _stream()), "gemm_bf16p")
    if colsum and defer_colsum:           # (part, rows, N, out) for `block_finalize`
        cs = (part, M // 32, N, _out(colsum_out, (N,), Ap.device))
    else:
        cs = globals()["colsum"](part, M // 32, N, out=colsum_out) if colsum else None
    return C_, (dout if save_dact else pre), pr, pt, cs


def small_linear_supported(M: int, N: int, K: int) -> bool:
    return bool(_lib.load().dpot_small_linear_supported(M, N, K))


def linear_fwd(x: Tensor, W: Tensor, bias: Optional[Tensor], act: int = 0, save_pre: bool = False,
               res: Optional[Tensor] = None, res_div: int = 0, res_mod: int = 0,
               ldw: Optional[int] = None, precision: Optional[int] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """y[M,N] = act(x[M,K] @ W[N,K]^T + bias) (+ res)   -  nn.Linear / 1x1-conv semantics."""
    M, K = x.shape
    N = W.shape[0]
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    pre = torch.empty_like(y) if save_pre else None
    lib = _lib.load()
    prec = _cur_gemm() if precision is None else precision
    if (res is None and M <= 128 and prec != GEMM_BF16 and lib.dpot_small_linear_supported(M, N, K)
            and tune("fused_small") != 0):
        # a handful of rows (the cls_head on the token mean): one pass over W, no split-K / reduce pair; exact fp32
        # (not under the opt-in bf16 operand rounding: that mode keeps its rounding at every batch size)
        check(lib.dpot_small_linear(x.data_ptr(), x.stride(0), W.data_ptr(), ldw or W.stride(0), _p(bias), y.data_ptr(),
                                    _p(pre), N, M, N, K, act, _stream()), "small_linear")
        return y, pre
    gemm(x, W, y, M, N, K, transB=True, lda=x.stride(0), ldb=ldw or W.stride(0), ldc=N, bias=bias, act=act,
         mode=EPI_ACT if act else EPI_LINEAR, preact=pre, ldpre=N, res=res, ldres=N, res_div=res_div,
         res_mod=res_mod, precision=precision)
    return y, pre


def linear_bwd_data(dy: Tensor, W: Tensor, act: int = 0, aux: Optional[Tensor] = None,
                    precision: Optional[int] = None) -> Tensor:
    """dx[M,K] = dy[M,N] @ W[N,K]  (optionally times act'(aux[M,K]))."""
    M, N = dy.shape
    K = W.shape[1]
    dx = torch.empty(M, K, dtype=torch.float32, device=dy.device)
    gemm(dy, W, dx, M, K, N, transB=False, lda=dy.stride(0), ldb=W.stride(0), ldc=K, act=act,
         mode=EPI_DACT if aux is not None else EPI_LINEAR, aux=aux, ldaux=K, precision=precision)
    return dx


def _out(out: Optional[Tensor], shape, device) -> Tensor:
    """`out` (a gradient slot inside the flat gradient buffer, see train.FlatParams) or a fresh tensor"""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    return out.view(shape)


def linear_bwd_weight(dy: Tensor, x: Tensor, out: Optional[Tensor] = None, n_rows: Optional[int] = None,
                      bias_out: Optional[Tensor] = None, precision: Optional[int] = None) -> Tensor:
    """dW[N,K] = dy[M,N]^T @ x[M,K]   (split-K over the token dimension); n_rows < N computes only dW[:n_rows].
    bias_out [N]: also db = colsum(dy), produced by the same kernel from the dy tiles it stages anyway."""
    M, N = dy.shape
    N = n_rows or N
    K = x.shape[1]
    dW = _out(out, (N, K), dy.device)
    gemm(dy, x, dW, N, K, M, transA=True, transB=False, lda=dy.stride(0), ldb=x.stride(0), ldc=K,
         splitk=auto_splitk(N, K, M, precision=precision, tn=True), colsum_out=bias_out, colsum_of=1,
         precision=precision)
    return dW


def linear_bwd_wb(dy: Tensor, x: Tensor, out_w: Optional[Tensor] = None, out_b: Optional[Tensor] = None,
                  precision: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """(dW, db) of y = x W^T + b in one launch (+ the split-K reduction): db rides on the dy tiles of the wgrad GEMM"""
    db = _out(out_b, (dy.shape[1],), dy.device)
    return linear_bwd_weight(dy, x, out=out_w, bias_out=db, precision=precision), db


# ------------------------------------------------------------------------------------------------------
# spectral ops
# ------------------------------------------------------------------------------------------------------
def rfft2_norm_supported(h: int, w: int, E: int) -> bool:
    return bool(_lib.load().dpot_rfft2_norm_supported(h, w, E))


def dft2_kernel_kind(B: int, h: int, w: int, E: int, nb: int, mx: int, my: int, inverse: bool = False,
                     norm: bool = False) -> int:
    """the kernel rfft2 / irfft2 (inverse) run for this call, norm: their GroupNorm-on-load forms - from the library's own
    selection (dpot_dft2_kernel_kind): H * 1000 + CC for a register FFT with CC-channel chunks, 0 for the generic direct-sum
    kernel, -1 where the call is refused"""
    return _lib.load().dpot_dft2_kernel_kind(B, h, w, E, nb, mx, my, int(inverse), int(norm))


def dft2_kernel_kinds(inverse: bool = False) -> Tuple[int, ...]:
    """every kind dft2_kernel_kind can return >= 0 for this direction: the kernels that are compiled"""
    buf = (C.c_int * 64)()
    n = _lib.load().dpot_dft2_kernel_kinds(int(inverse), buf, 64)
    assert n <= 64
    return tuple(buf[:n])


def rfft2(x: Tensor, h: int, w: int, nb: int, mx: int, my: int, col_weights: int = 0, norm=None) -> Tensor:
    """x[B,h*w,E] -> spec[B*mx*my, 2E] (planar per channel block).
    norm = (mean [B,G], rstd [B,G], gamma [E], beta [E]): the transform of GroupNorm(x) with those statistics, applied on
    the load (rfft2_norm_supported grids)"""
    B, E = x.shape[0], x.shape[-1]
    spec = torch.empty(B * mx * my, 2 * E, dtype=torch.float32, device=x.device)
    if norm is not None:
        mean, rstd, gamma, beta = norm
        check(_lib.load().dpot_rfft2_norm(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                          mean.shape[1], spec.data_ptr(), B, h, w, E, nb, mx, my, col_weights, _stream()),
              "rfft2_norm")
        return spec
    check(_lib.load().dpot_rfft2(x.data_ptr(), spec.data_ptr(), B, h, w, E, nb, mx, my, col_weights, _stream()),
          "rfft2")
    return spec


def irfft2(spec: Tensor, B: int, h: int, w: int, E: int, nb: int, mx: int, my: int, col_weights: int = 1,
           res: Optional[Tensor] = None, res_norm=None) -> Tensor:
    """res_norm = (mean, rstd, gamma, beta): the residual added is GroupNorm(res) with those statistics"""
    y = torch.empty(B, h * w, E, dtype=torch.float32, device=spec.device)
    if res_norm is not None:
        mean, rstd, gamma, beta = res_norm
        check(_lib.load().dpot_irfft2_norm(spec.data_ptr(), res.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                           gamma.data_ptr(), beta.data_ptr(), mean.shape[1], y.data_ptr(), B, h, w, E, nb,
                                           mx, my, col_weights, _stream()), "irfft2_norm")
        return y
    check(_lib.load().dpot_irfft2(spec.data_ptr(), _p(res), y.data_ptr(), B, h, w, E, nb, mx, my, col_weights,
                                  _stream()), "irfft2")
    return y


def kept_modes3(dims, modes: int, temporal_modes: int = 8) -> Tuple[int, int, int]:
    """the box AFNO3D keeps of rfftn's half spectrum (models/dpot3d.py:64): [:modes, :modes, :temporal_modes]"""
    X, Y, Z = dims
    return min(modes, X), min(modes, Y), min(temporal_modes, Z // 2 + 1)


def dft3_supported(dims, E: int, modes3) -> bool:
    """whether one sample's channel slab of an X x Y x Z latent cube fits the LDS (host only, no GPU needed)"""
    X, Y, Z = dims
    mx, my, mz = modes3
    return bool(_lib.load().dpot_dft3_supported(X, Y, Z, E, mx, my, mz))


def rfft3(x: Tensor, dims, nb: int, modes3, col_weights: int = 0) -> Tensor:
    """x[B, X*Y*Z, E] -> spec[B*mx*my*mz, 2E] (rows (b, kx, ky, kz), planar per channel block): w(kz) * rfftn(x, ortho) on
    the kept box; col_weights = 1: the adjoint of irfft3"""
    X, Y, Z = dims
    mx, my, mz = modes3
    B, E = x.shape[0], x.shape[-1]
    if not dft3_supported(dims, E, modes3):
        raise ValueError(f"rfft3: the latent grid {X}x{Y}x{Z} (kept modes {mx}x{my}x{mz}, {E} channels) is not supported: "
                         "one sample's channel slab does not fit the LDS")
    spec = torch.empty(B * mx * my * mz, 2 * E, dtype=torch.float32, device=x.device)
    check(_lib.load().dpot_rfft3(_req(x, "x").data_ptr(), spec.data_ptr(), B, X, Y, Z, E, nb, mx, my, mz, col_weights,
                                 _stream()), "rfft3")
    return spec


def irfft3(spec: Tensor, B: int, dims, E: int, nb: int, modes3, col_weights: int = 1,
           res: Optional[Tensor] = None) -> Tensor:
    """spec[B*mx*my*mz, 2E] -> y[B, X*Y*Z, E]: what irfftn(s=(X, Y, Z), ortho) gives for the zero-padded box, also for a
    spectrum that is not Hermitian (col_weights = 1); col_weights = 0: the adjoint of rfft3.  `res` is added"""
    X, Y, Z = dims
    mx, my, mz = modes3
    if not dft3_supported(dims, E, modes3):
        raise ValueError(f"irfft3: the latent grid {X}x{Y}x{Z} (kept modes {mx}x{my}x{mz}, {E} channels) is not supported: "
                         "one sample's channel slab does not fit the LDS")
    y = torch.empty(B, X * Y * Z, E, dtype=torch.float32, device=spec.device)
    check(_lib.load().dpot_irfft3(_req(spec, "spec").data_ptr(), _p(res), y.data_ptr(), B, X, Y, Z, E, nb, mx, my, mz,
                                  col_weights, _stream()), "irfft3")
    return y


def afno_pack(w: Tensor, b: Tensor) -> Tuple[Tensor, Tensor]:
    _, nb, bs, _ = w.shape
    wbig = torch.empty(nb, 2 * bs, 2 * bs, dtype=torch.float32, device=w.device)
    bbig = torch.empty(nb, 2 * bs, dtype=torch.float32, device=w.device)
    check(_lib.load().dpot_afno_pack(w.data_ptr(), b.data_ptr(), wbig.data_ptr(), bbig.data_ptr(), nb, bs,
                                     _stream()), "afno_pack")
    return wbig, bbig


class AfnoItem(tuple):
    """(Wbig, bbig, fwd pack | None, bwd pack | None) of one AFNO layer + the layout of the packs (0: fragment-block-major
    Wbig for afno_mlp2's four-product kernel, 1: (Wr, Wi) fragments for the three-product kernel)"""

    def __new__(cls, items, layout: int = 0, p6=None):
        self = super().__new__(cls, items)
        self.layout = layout
        self.p6 = p6          # (fwd6, bwd6): the bf16x6 packs of csrc/afno_mlp6.hip (layout 2 of afno_mlp2), or None
        return self

    wbig, bbig, fwd, bwd = (property(lambda self, i=i: self[i]) for i in range(4))


def afno_pack3(w: Tensor, b: Tensor) -> AfnoItem:
    """one layer packed on its own: (Wbig, bbig, blocked W | None, blocked W^T | None), layout 0"""
    _, nb, bs, _ = w.shape
    wbig, bbig = afno_pack(w, b)
    wf, wb = afno_block_weights(wbig) if afno_mlp2_supported(nb, bs) else (None, None)
    return AfnoItem((wbig, bbig, wf, wb))


class AfnoPacks:
    """Packed forms of ALL AFNO layers of a model, refreshed by ONE launch (dpot_afno_pack_all) from a device-resident
    job table: persistent output buffers, so the table is built once per parameter placement.
    pairs = [(w [2,nb,bs,bs], b [2,nb,bs]), ...];  self.items[i] = (wbig, bbig, fwd | None, bwd | None)"""

    def __init__(self, pairs):
        n = len(pairs)
        _, nb, bs, _ = pairs[0][0].shape
        dev = pairs[0][0].device
        N = 2 * bs
        self.nb, self.bs, self.n = nb, bs, n
        fused = afno_mlp2_supported(nb, bs)
        self.layout = 1 if fused and afno_mlp3_supported(nb, bs) else 0      # three-product (Wr, Wi) fragment packs
        wbig = torch.empty(n, nb, N, N, dtype=torch.float32, device=dev)
        bbig = torch.empty(n, nb, N, dtype=torch.float32, device=dev)
        fwd = torch.empty_like(wbig) if fused else None
        bwd = torch.empty_like(wbig) if fused else None
        self.table = _device_table(_lib.AfnoPackJob, [
            (_req(w, "w").data_ptr(), _req(b, "b").data_ptr(), wbig[i].data_ptr(), bbig[i].data_ptr(),
             fwd[i].data_ptr() if fused else None, bwd[i].data_ptr() if fused else None) for i, (w, b) in enumerate(pairs)], dev)
        # bf16x6 packs (csrc/afno_mlp6.hip): items alternate (first-layer weight, second-layer weight) - pairs of a filter
        self.wbig = wbig
        self.fwd6 = self.bwd6 = None               # allocated by the first refresh that wants them (3 bytes per weight element
        self._p6_ok = fused and n % 2 == 0 and afno_mlp6_supported(nb, bs)   # each: nothing for a model that stays in 'f32')
        self._base = [(wbig[i], bbig[i], fwd[i] if fused else None, bwd[i] if fused else None) for i in range(n)]
        self.items = [AfnoItem(t, self.layout, None) for t in self._base]

    def refresh(self):
        lib = _lib.load()
        check(lib.dpot_afno_pack_all(self.table.data_ptr(), self.n, self.nb, self.bs, self.layout, _stream()),
              "afno_pack_all")
        if self._p6_ok and afno_mlp6_wanted():
            if self.fwd6 is None:
                ne = int(lib.dpot_afno_pack6_elems(self.nb, self.bs))
                dev = self.wbig.device
                self.fwd6 = torch.empty(self.n, ne, dtype=torch.int16, device=dev)
                self.bwd6 = torch.empty(self.n, ne, dtype=torch.int16, device=dev)
                self.items = [AfnoItem(t, self.layout, (self.fwd6[i], self.bwd6[i])) for i, t in enumerate(self._base)]
            check(lib.dpot_afno_pack6(self.wbig.data_ptr(), self.fwd6.data_ptr(), self.bwd6.data_ptr(), self.n, self.nb,
                                      self.bs, _stream()), "afno_pack6")
        return self.items


def afno_block_weights(wbig: Tensor) -> Tuple[Tensor, Tensor]:
    """wbig [J, N, N] (W[k][n]) -> (fwd, bwd): fragment-block-major W and W^T (dpot_afno_block_weights)"""
    J, N, _ = wbig.shape
    fwd, bwd = torch.empty_like(wbig), torch.empty_like(wbig)
    check(_lib.load().dpot_afno_block_weights(wbig.data_ptr(), fwd.data_ptr(), bwd.data_ptr(), J, N, _stream()),
          "afno_block_weights")
    return fwd, bwd


def mlp_wgrad2_splitk(T: int, E: int, mh: int, precision: Optional[int] = None) -> int:
    """split factor of the fused fc1 + fc2 weight gradient (0: not covered / not worthwhile -> two separate GEMMs)"""
    prec = _cur_gemm() if precision is None else precision
    return _lib.load().dpot_mlp_wgrad2_splitk(T, E, mh) if prec == GEMM_F32 else 0


def mlp_wgrad2(do2: Tensor, Hh: Tensor, xn2: Tensor, dHpre: Tensor, dW2: Tensor, db2: Tensor, dW1: Tensor, db1: Tensor,
               splitk: int, defer: bool = False):
    """both weight gradients of a channel MLP, one launch + one reduce.  defer=True: the launch writes its split-K partials
    only and the job (for `block_finalize`, which reduces it together with the block's other partials) is returned"""
    lib = _lib.load()
    T, E = do2.shape
    mh = Hh.shape[1]
    ws = torch.empty(lib.dpot_mlp_wgrad2_ws_elems(E, mh, splitk), dtype=torch.float32, device=do2.device)
    outs = (None,) * 4 if defer else (dW2.data_ptr(), db2.data_ptr(), dW1.data_ptr(), db1.data_ptr())
    check(lib.dpot_mlp_wgrad2(do2.data_ptr(), Hh.data_ptr(), xn2.data_ptr(), dHpre.data_ptr(), T, E, mh, *outs,
                              ws.data_ptr(), splitk, _stream()), "mlp_wgrad2")
    return (ws, splitk, E, mh, dW2, db2, dW1, db1) if defer else None


def afno_wgrad2_splitk(Mm: int, nb: int, bs: int) -> int:
    """split factor of the fused two-layer AFNO weight gradient (0: shape not covered -> two generic GEMM launches)"""
    return _lib.load().dpot_afno_wgrad2_splitk(Mm, nb, bs) if _cur_gemm() in (GEMM_F32, GEMM_AUTO) else 0


def afno_wgrad2(S: Tensor, dO1pre: Tensor, O1: Tensor, dO2: Tensor, nb: int, bs: int, dw1: Tensor, db1: Tensor,
                dw2: Tensor, db2: Tensor, splitk: int, defer: bool = False):
    """dw1 / db1 (from S, dO1pre) and dw2 / db2 (from O1, dO2) of an AFNO block's complex MLP: one launch + one reduce.
    defer=True: partials only; returns the job for `block_finalize`"""
    lib = _lib.load()
    Mm, ld = S.shape
    ws = torch.empty(lib.dpot_afno_wgrad2_ws_elems(nb, bs, splitk), dtype=torch.float32, device=S.device)
    outs = (None,) * 4 if defer else (dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr())
    check(lib.dpot_afno_wgrad2(S.data_ptr(), dO1pre.data_ptr(), O1.data_ptr(), dO2.data_ptr(), ld, Mm, nb, bs, *outs,
                               ws.data_ptr(), splitk, _stream()), "afno_wgrad2")
    return (ws, splitk, nb, bs, dw1, db1, dw2, db2) if defer else None


def block_finalize(afno_job, mlp_job, gn_jobs, cs_jobs=()):
    """ONE launch for the reductions that end a DPOT block's backward (csrc/gemm_tn.hip block_finalize_kernel): the deferred
    split-K partials of `afno_wgrad2` and / or `mlp_wgrad2` (jobs as those return them, or None) and the GroupNorm
    parameter-gradient partials gn_jobs = [(part [2,B,E], out_dgamma | None, out_dbeta | None)] (<= 2), and the deferred
    column sums cs_jobs of `bf16_pack_both` / `gemm_bf16p_packed` (defer_colsum=True; <= 2).  Returns the GroupNorm outputs
    [(dgamma, dbeta)]; the other outputs are the tensors handed to / returned by the deferred calls."""
    null = None
    a = afno_job if afno_job is not None else (None, 0, 0, 0, None, None, None, None)
    m = mlp_job if mlp_job is not None else (None, 0, 0, 0, None, None, None, None)
    n = len(gn_jobs)
    outs, B, E = [], 0, 0
    parts = dgs = dbs = null
    if n:
        _, B, E = gn_jobs[0][0].shape
        outs = [(_out(og, (E,), p.device), _out(ob, (E,), p.device)) for p, og, ob in gn_jobs]
        parts = (C.c_void_p * n)(*[p.data_ptr() for p, _, _ in gn_jobs])
        dgs = (C.c_void_p * n)(*[g.data_ptr() for g, _ in outs])
        dbs = (C.c_void_p * n)(*[b.data_ptr() for _, b in outs])
    nc = len(cs_jobs)                              # [(part [rows, N], rows, N, out [N])] (<= 2): deferred column sums
    cparts = couts = crows = ccols = null
    if nc:
        cparts = (C.c_void_p * nc)(*[j[0].data_ptr() for j in cs_jobs])
        couts = (C.c_void_p * nc)(*[j[3].data_ptr() for j in cs_jobs])
        crows = (C.c_int * nc)(*[j[1] for j in cs_jobs])
        ccols = (C.c_int * nc)(*[j[2] for j in cs_jobs])
    check(_lib.load().dpot_block_finalize(_p(a[0]), a[1], a[2], a[3], _p(a[4]), _p(a[5]), _p(a[6]), _p(a[7]),
                                          _p(m[0]), m[1], m[2], m[3], _p(m[4]), _p(m[5]), _p(m[6]), _p(m[7]),
                                          parts, dgs, dbs, n, B, E, cparts, couts, crows, ccols, nc, _stream()),
          "block_finalize")
    return outs


def block_finalize_enabled() -> bool:
    return tune("fused_small") != 0


def wgrad_batch_enabled() -> bool:
    """the weight gradients of all blocks in batched launches + one finalising launch (DPOT_TUNE fused_small=2: per block;
    4 and 5, the default: the batched launches on the weight-gradient lane, `wgrad_lane_enabled`)"""
    return tune("fused_small") in (1, 3, 4, 5)


def wgrad_batch_one_round() -> bool:
    """DPOT_TUNE fused_small=3: the batched launches cut the tokens by the one-round rules (`mlp_wgrad_batch_splitk`,
    `afno_wgrad_batch_plan`) - another summation order than the per-block launches; default: the per-block split factors,
    bit-identical gradients"""
    return tune("fused_small") == 3


@contextlib.contextmanager
def wgrad_lane_scope(on: Optional[bool]):
    """whether the forward passes run on this thread inside hand their batched weight gradients to the library's lane
    (functional.WgradBatch reads it when DPOTNet creates it, so the backward may run anywhere later): True / False, or None =
    DPOT_TUNE fused_small (4 and 5, the default: the lane).  For one process that runs both schedules."""
    prev = getattr(_tls, "wgrad_lane", None)
    _tls.wgrad_lane = on
    try:
        yield
    finally:
        _tls.wgrad_lane = prev


@contextlib.contextmanager
def wgrad_chain_scope(chains):
    """the chains (mlp_chain, afno_chain) - each 1, 2 or 4 - that the default batch of the forward passes run on this thread
    inside gives its two launches (functional.WgradBatch reads it when DPOTNet creates it), or None = the default, no chain.
    For tests and A/B runs in one process; the results do not depend on it."""
    if chains is not None:
        chains = (int(chains[0]), int(chains[1]))
        if not all(c in (1, 2, 4) for c in chains):
            raise ValueError(f"wgrad_chain_scope: chains {chains} must be 1, 2 or 4")
    prev = getattr(_tls, "wgrad_chain", None)
    _tls.wgrad_chain = chains
    try:
        yield
    finally:
        _tls.wgrad_chain = prev


def wgrad_chain_override():
    """(mlp_chain, afno_chain) of the enclosing `wgrad_chain_scope`, or None"""
    return getattr(_tls, "wgrad_chain", None)


def tn_chain_count(splits: int, chain: int) -> int:
    """workspace slots (nodes) of `splits` token ranges chained by `chain`; 0: bad arguments"""
    return _lib.load().dpot_tn_chain_count(splits, chain)


def tn_chain_nodes(splits: int, chain: int):
    """[(first range, ranges)] of every node, in dispatch order (csrc/gemm_tn.hip tn_chain_node)"""
    lib, out = _lib.load(), []
    f, c = C.c_int(0), C.c_int(0)
    for i in range(lib.dpot_tn_chain_count(splits, chain)):
        check(lib.dpot_tn_chain_nodes(splits, chain, i, C.byref(f), C.byref(c)), "tn_chain_nodes")
        out.append((f.value, c.value))
    return out


def mlp_wgrad_batch_chain(E: int, mh: int, splitk: int, n: int) -> int:
    """the largest chain of `mlp_wgrad_batch` over n blocks that leaves a full round of 256 workgroups (fastest for the launch
    alone; not the model's default, see functional.WgradBatch)"""
    return _lib.load().dpot_mlp_wgrad_batch_chain(E, mh, splitk, n)


def afno_wgrad_batch_chain(nb: int, per_launch: int, splits12: int, splitk: int) -> int:
    """the same for `afno_wgrad_batch` at `per_launch` blocks per launch, at most 2 (4 leaves unequal workgroups: slower)"""
    return _lib.load().dpot_afno_wgrad_batch_chain(nb, per_launch, splits12, splitk)


def wgrad_lane_enabled() -> bool:
    v = getattr(_tls, "wgrad_lane", None)
    return tune("fused_small") in (4, 5) if v is None else bool(v)


# ---- the library's lanes (csrc/lane.hip) -------------------------------------------------------------------------------------
_lane_lock = threading.Lock()


class _Lane:
    """One lane of the library as this module drives it: a library-owned stream beside the step's.  `block` forks it behind
    torch's current stream and sends this thread's launches to it, `join` orders the streams that forked behind it.
    index: the library's lane; forks: forks not joined yet, as this module counts them; streams: the streams that forked;
    held: what the queued launches touch - allocated on the step's stream and referenced from here until the join has been
    ISSUED, so whatever the allocator hands out again afterwards is ordered behind the lane.  (`_tls.lane` says which lane, if
    any, this thread's launches go to.)
    Known limit: ONE thread and ONE stream per device drive a lane between fork and join.  The library clears its pending count
    at the first join, so after forks from two streams (or two threads at once) the second stream's join is a no-op."""

    def __init__(self, index: int):
        self.index, self.forks, self.streams, self.held = index, 0, [], []

    def init(self) -> None:
        """create the current device's lane now (never legal while a stream of the device is capturing)"""
        check(_lib.load().dpot_lane_init(self.index), "lane_init")

    def ready(self) -> bool:
        return bool(_lib.load().dpot_lane_ready(self.index))

    def pending(self) -> int:
        """forks of the current device's lane since the last join (tests, assertions)"""
        return _lib.load().dpot_lane_pending(self.index)

    def shutdown(self) -> None:
        check(_lib.load().dpot_lane_shutdown(self.index), "lane_shutdown")

    def join(self) -> None:
        """order every stream that forked the lane behind it (dpot_lane_join) and release what the lane's launches use.  The
        streams are those recorded at the fork, not torch's current one: lane 0 is joined from the autograd engine's
        end-of-backward callback.  Nothing - no library call - when nothing is forked; may be repeated."""
        with _lane_lock:
            if self.forks == 0:
                return
            streams, held = self.streams, self.held        # `held` lives until the joins below have been issued
            self.forks, self.streams, self.held = 0, [], []
        for stream in dict.fromkeys(streams):
            check(_lib.load().dpot_lane_join(self.index, stream), "lane_join")

    @contextlib.contextmanager
    def block(self, join: bool = True, joiner=None):
        """Fork the lane behind torch's current stream and send every launch of this module made inside the block, on this
        thread, to the lane (`_stream`).  torch's current stream stays the step's: allocations belong to it, and NO torch op
        may run inside the block - allocate what one would, or let the ops of this module allocate, before any further work
        goes to the step's stream.  Nested in another lane block nothing is forked: the launches stay where they were going.
        join=False leaves the lane forked when the block ends normally - the caller joins before anything reads the block's
        results; an exception inside always joins.  joiner: what joins (default `self.join`)."""
        if getattr(_tls, "lane", None) is not None:
            yield
            return
        step = _step_stream()
        handle = C.c_void_p()
        check(_lib.load().dpot_lane_fork(self.index, step, C.byref(handle)), "lane_fork")
        with _lane_lock:
            self.forks += 1
            self.streams.append(step)
        _tls.lane = (self, handle.value or 0)
        ok = False
        try:
            yield
            ok = True
        finally:
            _tls.lane = None
            if join or not ok:
                (joiner or self.join)()


SIDE_LANE = 1
_WGRAD, _SIDE = _Lane(0), _Lane(SIDE_LANE)

# Lane 0, the weight-gradient lane (`wgrad_flush_async`).  wgrad_lane_join: the end-of-backward callback of functional.WgradBatch
# and FlatOptimizer.launch call it.
wgrad_lane_init, wgrad_lane_ready, wgrad_lane_pending, wgrad_lane_join = _WGRAD.init, _WGRAD.ready, _WGRAD.pending, _WGRAD.join


def wgrad_lane_shutdown() -> None:
    wgrad_lane_join()
    _WGRAD.shutdown()


# Lane 1, the side lane: short chains of latency-bound launches that run beside independent work of the step's stream (DESIGN.md
# section 5):
#   weights  packs.ModelPacks.derive: everything `embed_fwd` does not read, joined by EmbedFn.forward before the fold GEMM
#   patch    EmbedFn.backward: the first conv's gradients beside the weight-only chain
# Same launches, same arguments, same results; DPOT_TUNE fused_small=5 (the default) switches on the sites of SIDE_SITES_DEFAULT.
# (A third site, the classification head beside the de-embed GEMM, measured 11 us against a spread of 9 us and was taken out
# again: profiles/side_lane_ab.txt, section 2.)
SIDE_SITES = ("weights", "patch")
SIDE_SITES_DEFAULT = SIDE_SITES
side_lane_ready, side_lane_pending, side_lane_join = _SIDE.ready, _SIDE.pending, _SIDE.join


@contextlib.contextmanager
def side_lane_scope(sites):
    """the side-lane sites (a subset of SIDE_SITES) of the forward passes run on this thread inside, and of their backward
    passes wherever those run; None = DPOT_TUNE fused_small.  For the ablation and the tests."""
    if sites is not None:
        sites = tuple(sites)
        if any(s not in SIDE_SITES for s in sites):
            raise ValueError(f"side_lane_scope: sites {sites} not among {SIDE_SITES}")
    prev = getattr(_tls, "side_sites", None)
    _tls.side_sites = sites
    try:
        yield
    finally:
        _tls.side_sites = prev


def side_lane_enabled(site: str) -> bool:
    v = getattr(_tls, "side_sites", None)
    if v is None:
        v = SIDE_SITES_DEFAULT if tune("fused_small") == 5 else ()
    return site in v


def side_lane_shutdown() -> None:
    side_lane_join()
    _SIDE.shutdown()


@contextlib.contextmanager
def side_lane(site: str, on: Optional[bool] = None, join: bool = True):
    """a `_Lane.block` of the side lane when the site takes the lane (on; None = `side_lane_enabled(site)`), else nothing: the
    launches stay where they were going.  join=False: the caller joins (`side_lane_join`)."""
    if on is None:
        on = side_lane_enabled(site)
    with _SIDE.block(join, lambda: side_lane_join()) if on else contextlib.nullcontext():
        yield


def wgrad_batch_max_blocks() -> int:
    return _lib.load().dpot_wgrad_batch_max_blocks()


def afno_wgrad2_splits12(Mm: int, bs: int, splitk: int) -> int:
    """token ranges of P1 / P2 in `afno_wgrad2` at `splitk`; 0 if one of them would be empty (TN_TOK = 32 tokens per slab)"""
    s12 = _lib.load().dpot_afno_wgrad2_splits12(bs, splitk)
    nslab = Mm // 32
    return s12 if s12 >= 1 and -(-nslab // s12) * (s12 - 1) < nslab else 0


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def mlp_wgrad_batch_splitk(T: int, E: int, mh: int, n: int, precision: Optional[int] = None) -> int:
    """split factor of the channel-MLP weight gradients of n blocks in one launch (0: not covered)"""
    prec = _cur_gemm() if precision is None else precision
    return _lib.load().dpot_mlp_wgrad_batch_splitk(T, E, mh, n) if prec == GEMM_F32 else 0


def mlp_wgrad_batch(do2, Hh, xn2, dHpre, splitk: int, chain: int = 1) -> Tensor:
    """partials of both channel-MLP weight gradients of len(do2) blocks (lists of per-block operands, as `mlp_wgrad2`):
    returns the workspace [n, elems] - row i in the layout `mlp_wgrad2(defer=True)` leaves, for `wgrad_batch_finalize`.
    chain 2 / 4: a workgroup walks up to that many consecutive token ranges and stores one partial per node of the
    finalising launch's summation tree (same bits; give `wgrad_batch_finalize` the same chain)"""
    n = len(do2)
    T, E = do2[0].shape
    mh = Hh[0].shape[1]
    for a, b, c, d in zip(do2, Hh, xn2, dHpre):
        assert a.shape == (T, E) and c.shape == (T, E) and b.shape == (T, mh) and d.shape == (T, mh)
        assert a.is_contiguous() and b.is_contiguous() and c.is_contiguous() and d.is_contiguous()
    ws = torch.empty(n, _lib.load().dpot_mlp_wgrad_chain_ws_elems(E, mh, splitk, chain), dtype=torch.float32,
                     device=do2[0].device)
    check(_lib.load().dpot_mlp_wgrad_batch(_ptr_array(do2), _ptr_array(Hh), _ptr_array(xn2), _ptr_array(dHpre), n, T, E, mh,
                                           ws.data_ptr(), splitk, chain, _stream()), "mlp_wgrad_batch")
    return ws


def afno_wgrad_batch_plan(Mm: int, nb: int, bs: int, n: int) -> Tuple[int, int, int]:
    """(blocks per launch, splits12, splits) of the batched three-product AFNO weight gradient; blocks per launch 0: the
    shape is not covered (per-block launches)"""
    if _cur_gemm() not in (GEMM_F32, GEMM_AUTO):
        return 0, 0, 0
    s12, s = C.c_int(0), C.c_int(0)
    per = _lib.load().dpot_afno_wgrad_batch_plan(Mm, nb, bs, n, C.byref(s12), C.byref(s))
    return per, s12.value, s.value


def afno_wgrad_batch(S, dO1pre, O1, dO2, nb: int, bs: int, per_launch: int, splits12: int, splitk: int,
                     chain: int = 1) -> Tensor:
    """partials of both AFNO weight gradients of len(S) blocks (lists of per-block operands, as `afno_wgrad2`), `per_launch`
    blocks per launch: returns the workspace [n, elems], row i in the layout of `afno_wgrad2(defer=True)`; chain: as
    `mlp_wgrad_batch`"""
    n = len(S)
    Mm, ld = S[0].shape
    for ts in (S, dO1pre, O1, dO2):
        for t in ts:
            assert t.shape == (Mm, ld) and t.is_contiguous()
    ws = torch.empty(n, _lib.load().dpot_afno_wgrad_chain_ws_elems(nb, bs, splits12, splitk, chain), dtype=torch.float32,
                     device=S[0].device)
    check(_lib.load().dpot_afno_wgrad_batch(_ptr_array(S), _ptr_array(dO1pre), _ptr_array(O1), _ptr_array(dO2), n, ld, Mm, nb,
                                            bs, ws.data_ptr(), per_launch, splits12, splitk, chain, _stream()), "afno_wgrad_batch")
    return ws


def wgrad_batch_finalize(afno, mlp, gn, mlp_chain: int = 1, afno_chain: int = 1):
    """ONE launch that finalises n blocks (csrc/gemm_tn.hip wgrad_batch_finalize_kernel); mlp_chain / afno_chain: the chains
    the workspaces were written with.
    afno: None | (ws [n, .], splits12, splitk, nb, bs, [(dw1, db1, dw2, db2)] * n);
    mlp:  None | (ws [n, .], splitk, E, mh, [(dW2, db2, dW1, db1)] * n);
    gn:   [[(part [2, B, E], dgamma, dbeta)] * jobs] * n  (jobs <= 2, outputs allocated by the caller)"""
    n = len(gn)
    blocks = (_lib.WgradBlock * n)()
    jobs, B, Eg = len(gn[0]), 0, 0
    for i in range(n):
        w = blocks[i]
        if afno is not None:
            w.afno_ws = afno[0][i].data_ptr()
            w.dw1, w.db1, w.dw2, w.db2 = (t.data_ptr() for t in afno[5][i])
        if mlp is not None:
            w.mlp_ws = mlp[0][i].data_ptr()
            w.dW2, w.dfb2, w.dW1, w.dfb1 = (t.data_ptr() for t in mlp[4][i])
        assert len(gn[i]) == jobs
        for j, (part, dg, db) in enumerate(gn[i]):
            _, B, Eg = part.shape
            w.gn_part[j], w.gn_dgamma[j], w.gn_dbeta[j] = part.data_ptr(), dg.data_ptr(), db.data_ptr()
    a = afno if afno is not None else (None, 0, 0, 0, 0)
    m = mlp if mlp is not None else (None, 0, 0, 0)
    check(_lib.load().dpot_wgrad_batch_finalize(blocks, n, a[1], a[2], a[3], a[4], m[1], m[2], m[3], jobs, B, Eg, mlp_chain,
                                                afno_chain, _stream()), "wgrad_batch_finalize")


def wgrad_flush_async(mlp_ops, skm: int, mouts, afno_ops, nb: int, bs: int, per_launch: int, splits12: int, splitk: int,
                      aouts, gn, mlp_chain: int = 1, afno_chain: int = 1) -> None:
    """`afno_wgrad_batch`, `mlp_wgrad_batch` and `wgrad_batch_finalize` of one group of blocks on the library's lane 0, forked
    behind the current stream and left forked.  mlp_ops / afno_ops: the four operand lists of the two launches; mouts, aouts,
    gn: the outputs per block as `wgrad_batch_finalize` takes them.  Everything the launches touch stays referenced until
    `wgrad_lane_join` has ordered the stream behind the lane."""
    with _WGRAD.block(join=False):
        # The AFNO launch goes FIRST.  The embed backward beside the lane opens with its two MFMA-bound fold GEMMs (768 and 528
        # workgroups) and goes on with short latency-bound launches.  Beside the channel-MLP launch the first fold GEMM took
        # 124 us (38 us alone) - and 334 us beside a chained, one-round MLP launch, whose 256 workgroups hold every CU for
        # 300 us; beside the AFNO launch (shorter workgroups, a third of them the VALU-heavy sum-product tiles) the fold GEMMs
        # get through, and the long MLP launch then runs beside the short launches.  Independent workspaces: no result depends
        # on the order.  DPOT-Tiny step 2.9275 -> 2.8859 ms against the parent commit (profiles/wgrad_chain_ab.txt, section 4)
        aws = afno_wgrad_batch(*afno_ops, nb, bs, per_launch, splits12, splitk, afno_chain)
        mws = mlp_wgrad_batch(*mlp_ops, skm, mlp_chain)
        _hold(mlp_ops, afno_ops, aws, mws, mouts, aouts, gn)
        E, mh = mlp_ops[0][0].shape[1], mlp_ops[1][0].shape[1]
        wgrad_batch_finalize((aws, splits12, splitk, nb, bs, aouts), (mws, skm, E, mh, mouts), gn, mlp_chain, afno_chain)


def afno_mlp2_supported(nb: int, bs: int) -> bool:
    return bool(_lib.load().dpot_afno_mlp2_supported(nb, bs)) and tune("mixer") != 0


def afno_mlp3_supported(nb: int, bs: int) -> bool:
    """the three-product (Gauss / Karatsuba) form of the fused mixer kernel: bs == 128; DPOT_TUNE mixer=4 / mixer=0 select
    the other forms"""
    return bool(_lib.load().dpot_afno_mlp3_supported(nb, bs)) and tune("mixer") == 3


def afno_mlp6_supported(nb: int, bs: int) -> bool:
    """the bf16x6 (fp32-accurate, bf16 matrix cores) form of the fused mixer kernel, csrc/afno_mlp6.hip: bs in {96, 128}"""
    return bool(_lib.load().dpot_afno_mlp6_supported(nb, bs)) and tune("mixer") != 0 and (tune("mixer6") == 2 or (tune("mixer6") == 1 and bs == 96))


def afno_mlp6_wanted() -> bool:
    """the mixer follows the GEMM precision in effect: 'auto' / 'bf16x6' -> the bf16x6 kernel (both are fp32-accurate, the
    choice is speed); 'f32' -> the native fp32 matrix-core kernels"""
    return _cur_gemm() in (GEMM_AUTO, GEMM_BF16X6)


AFNO_FOUR, AFNO_THREE, AFNO_THREE_SPLIT, AFNO_REFUSED = 0, 1, 2, -1


class AfnoPlan(NamedTuple):
    """what dpot_afno_mlp2_plan reports: form (AFNO_FOUR / AFNO_THREE / AFNO_THREE_SPLIT / AFNO_REFUSED), 16-row tiles per
    panel, panels per block (the grid is nb * panels), compute waves, GELU instantiation (else the run-time switch)"""
    form: int
    rt: int
    panels: int
    waves: int
    gelu: bool


def afno_mlp2_plan(M: int, nb: int, bs: int, layout: int = 0, act: int = 1) -> AfnoPlan:
    """the kernel instantiation afno_mlp2 (layout 0 / 1) launches for this call, from the library's own selection
    (dpot_afno_mlp2_plan); form AFNO_REFUSED where the call is refused"""
    buf = (C.c_int * 5)()
    _lib.load().dpot_afno_mlp2_plan(M, nb, bs, layout, act, buf)
    return AfnoPlan(buf[0], buf[1], buf[2], buf[3], bool(buf[4]))


def afno_mlp2_plans() -> Tuple[Tuple[int, int, int, bool], ...]:
    """every instantiation afno_mlp2_plan can name, as (form, bs, rt, gelu)"""
    cap = 128
    buf = (C.c_int * (4 * cap))()
    n = _lib.load().dpot_afno_mlp2_plans(buf, cap)
    assert n <= cap
    return tuple((buf[4 * i], buf[4 * i + 1], buf[4 * i + 2], bool(buf[4 * i + 3])) for i in range(n))


def _afno_ld(t: Tensor, name: str, M: int, cols: int) -> int:
    """the leading dimension of a [M, >= cols] operand of afno_mlp2 (its row stride), or a ValueError for what the kernels
    cannot express: they read and write rows of unit-stride floats in 16-byte pieces"""
    if t.dim() != 2 or t.shape[0] != M or t.shape[1] < cols or t.dtype != torch.float32:
        raise ValueError(f"afno_mlp2: {name} must be float32 [{M}, >= {cols}], got {t.dtype} {tuple(t.shape)}")
    if t.stride(1) != 1:
        raise ValueError(f"afno_mlp2: {name} has inner stride {t.stride(1)}: the rows must be contiguous")
    ld = t.stride(0) if M > 1 else t.shape[1]            # a single row has no row stride
    if ld < cols or ld % 4:
        raise ValueError(f"afno_mlp2: {name} has row stride {ld}: it must be a multiple of 4 and at least {cols}")
    if t.data_ptr() % 16:
        raise ValueError(f"afno_mlp2: {name} does not start on a 16-byte boundary")
    return ld


def afno_mlp2(X: Tensor, WaT: Tensor, ba: Optional[Tensor], WbT: Tensor, bb: Optional[Tensor], nb: int, bs: int,
              act: int, mode: int = 0, aux: Optional[Tensor] = None, want_pre: bool = False, want_mid: bool = False,
              layout: int = 0, out_Y: Optional[Tensor] = None, out_pre: Optional[Tensor] = None,
              out_mid: Optional[Tensor] = None):
    """both layers of the AFNO block-diagonal complex MLP in one launch (csrc/afno_mlp.hip).
    mode 0: pre = X Wa + ba, mid = act(pre), Y = mid Wb + bb;  mode 1: mid = (X Wa) * act'(aux), Y = mid Wb, and with
    want_pre the `pre` output is act(aux) (the forward's activated layer-1 output, re-derived for the weight gradient).
    X / outputs: [M, nb*2*bs]; WaT / WbT: [nb, 2bs, 2bs] fragment-block-major weights from afno_block_weights (`fwd`
    to multiply by W, `bwd` to multiply by W^T).  Returns (Y, pre | None, mid | None).
    X may be a view with a row stride of its own (ldx); the outputs are fresh contiguous tensors, or out_Y / out_pre / out_mid
    (an out_pre / out_mid implies want_pre / want_mid), whose common row stride is ldo - aux, which the kernels address with
    ldo as well, must have it too.  Anything else (an inner stride, a row stride that is no multiple of 4, a base off a
    16-byte boundary, strides that differ) is a ValueError before anything is launched."""
    M, cols = X.shape[0], nb * 2 * bs
    ldx = _afno_ld(X, "X", M, cols)
    given = [(n, t) for n, t in (("out_Y", out_Y), ("out_pre", out_pre), ("out_mid", out_mid), ("aux", aux)) if t is not None]
    lds = {n: _afno_ld(t, n, M, cols) for n, t in given}
    ldo = lds.get("out_Y", lds.get("out_pre", lds.get("out_mid", X.shape[1])))
    if M > 1 and any(v != ldo for v in lds.values()):
        raise ValueError(f"afno_mlp2: aux and the outputs share one row stride, got {lds} against {ldo}"
                         + ("" if out_Y is not None else " of the fresh outputs"))
    if ldo < cols or ldo % 4:
        raise ValueError(f"afno_mlp2: output row stride {ldo}: it must be a multiple of 4 and at least {cols}")

    def fresh():
        t = torch.empty((M, ldo), dtype=torch.float32, device=X.device)
        return t if ldo == X.shape[1] else t[:, :X.shape[1]]

    Y = out_Y if out_Y is not None else fresh()
    pre = out_pre if out_pre is not None else fresh() if want_pre else None
    mid = out_mid if out_mid is not None else fresh() if want_mid else None
    if layout == 2:      # WaT / WbT: the bf16x6 packs of AfnoPacks (item.p6), csrc/afno_mlp6.hip
        check(_lib.load().dpot_afno_mlp6(X.data_ptr(), WaT.data_ptr(), _p(ba), WbT.data_ptr(), _p(bb), _p(aux), _p(pre),
                                         _p(mid), Y.data_ptr(), M, nb, bs, ldx, ldo, act, mode, _stream()), "afno_mlp6")
        return Y, pre, mid
    check(_lib.load().dpot_afno_mlp2(X.data_ptr(), WaT.data_ptr(), _p(ba), WbT.data_ptr(), _p(bb), _p(aux), _p(pre),
                                     _p(mid), Y.data_ptr(), M, nb, bs, ldx, ldo, act, mode, layout, _stream()),
          "afno_mlp2")
    return Y, pre, mid


def afno_unpack_grad(dwbig: Tensor, dbbig: Tensor, nb: int, bs: int, out_dw: Optional[Tensor] = None,
                     out_db: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    dw = _out(out_dw, (2, nb, bs, bs), dwbig.device)
    db = _out(out_db, (2, nb, bs), dwbig.device)
    check(_lib.load().dpot_afno_unpack_grad(dwbig.data_ptr(), dbbig.data_ptr(), dw.data_ptr(), db.data_ptr(), nb, bs,
                                            _stream()), "afno_unpack_grad")
    return dw, db


# ------------------------------------------------------------------------------------------------------
# GroupNorm
# ------------------------------------------------------------------------------------------------------
def _gn_workspace(B: int, T: int, E: int, G: int, device) -> Optional[Tensor]:
    """scratch for the chunked GroupNorm kernels (few, large (sample, group) slabs: DPOT-L at 256^2), or None"""
    n = _lib.load().dpot_groupnorm_ws_elems(B, T, E, G)
    return torch.empty(n, dtype=torch.float32, device=device) if n > 0 else None


def groupnorm_ws_elems(B: int, T: int, E: int, G: int) -> int:
    return int(_lib.load().dpot_groupnorm_ws_elems(B, T, E, G))


GN_DIRECTIONS = {"fwd": 0, "bwd": 1, "bwd_packs": 2, "stats": 3}
GN_SCALAR, GN_VEC4, GN_CACHED4, GN_CACHED8, GN_CHUNKED = 0, 1, 4, 8, 16


def groupnorm_kernel_kind(B: int, T: int, E: int, G: int = 8, direction: str = "fwd", has_workspace: bool = True,
                          aligned: bool = True) -> int:
    """the kernel route groupnorm_fwd / groupnorm_bwd / groupnorm_bwd_packs / groupnorm_stats (direction "fwd", "bwd",
    "bwd_packs", "stats") take for this call, from the library's own selection (dpot_groupnorm_kernel_kind): GN_SCALAR,
    GN_VEC4 (generic kernels), GN_CACHED4 / GN_CACHED8 (register-cached, 4 / 8 items), GN_CHUNKED, or -1 where the call is
    refused.  has_workspace: chunked=True; aligned: every tensor of the call starts on a 16-byte boundary"""
    return _lib.load().dpot_groupnorm_kernel_kind(B, T, E, G, GN_DIRECTIONS.get(direction, -1), int(has_workspace),
                                                  int(aligned))


def groupnorm_kernel_kinds(direction: str = "fwd") -> Tuple[int, ...]:
    """every kind groupnorm_kernel_kind can return >= 0 for this direction"""
    buf = (C.c_int * 16)()
    n = _lib.load().dpot_groupnorm_kernel_kinds(GN_DIRECTIONS.get(direction, -1), buf, 16)
    assert n <= 16
    return tuple(buf[:n])


def groupnorm_chunks(B: int, T: int, E: int, G: int = 8) -> Tuple[int, int]:
    """(tokens per chunk, chunks per (sample, group) slab) of the chunked kernels; (0, 0): the shape is never chunked"""
    tc, ch = C.c_int(0), C.c_int(0)
    _lib.load().dpot_groupnorm_chunks(B, T, E, G, C.byref(tc), C.byref(ch))
    return tc.value, ch.value


def groupnorm_fwd(x: Tensor, gamma: Tensor, beta: Tensor, G: int = 8, eps: float = 1e-5, chunked: bool = True):
    """chunked=False: never the chunked kernels (no workspace is passed)"""
    B, T, E = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(B, G, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B, G, dtype=torch.float32, device=x.device)
    ws = _gn_workspace(B, T, E, G, x.device) if chunked else None
    check(_lib.load().dpot_groupnorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                         mean.data_ptr(), rstd.data_ptr(), _p(ws), B, T, E, G, eps, _stream()),
          "groupnorm_fwd")
    return y, mean, rstd


def groupnorm_stats_supported(B: int, T: int, E: int, G: int = 8) -> bool:
    """statistics-only GroupNorm (groupnorm_stats): the chunked kernels (few, large (sample, group) slabs - DPOT-L)"""
    return _lib.load().dpot_groupnorm_ws_elems(B, T, E, G) > 0


def groupnorm_stats(x: Tensor, gamma: Tensor, beta: Tensor, G: int = 8, eps: float = 1e-5):
    """(mean, rstd) [B, G] of GroupNorm(G, E) over x [B, T, E] without writing the normalised tensor - the consumer applies
    the affine map on its load (rfft2(norm=...), bf16_pack_both(norm=...)); needs groupnorm_stats_supported"""
    B, T, E = x.shape
    mean = torch.empty(B, G, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B, G, dtype=torch.float32, device=x.device)
    ws = _gn_workspace(B, T, E, G, x.device)
    check(_lib.load().dpot_groupnorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, mean.data_ptr(),
                                         rstd.data_ptr(), _p(ws), B, T, E, G, eps, _stream()), "groupnorm_fwd (statistics)")
    return mean, rstd


def groupnorm_bwd(dy: Tensor, x: Tensor, mean: Tensor, rstd: Tensor, gamma: Tensor, G: int = 8,
                  add: Optional[Tensor] = None, out_dgamma: Optional[Tensor] = None,
                  out_dbeta: Optional[Tensor] = None, defer: bool = False, chunked: bool = True):
    """defer=False: returns (dx, dgamma, dbeta).  defer=True: returns (dx, part) - the per-sample partials [2,B,E] of the
    parameter gradients, to be reduced later by groupnorm_param_grads (several layers in one launch).
    chunked=False: never the chunked kernels (no workspace is passed)"""
    B, T, E = x.shape
    dx = torch.empty_like(x)
    part = torch.empty(2, B, E, dtype=torch.float32, device=x.device)
    dgamma = None if defer else _out(out_dgamma, (E,), x.device)
    dbeta = None if defer else _out(out_dbeta, (E,), x.device)
    ws = _gn_workspace(B, T, E, G, x.device) if chunked else None
    check(_lib.load().dpot_groupnorm_bwd(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                         gamma.data_ptr(), _p(add), dx.data_ptr(), _p(dgamma), _p(dbeta),
                                         part.data_ptr(), _p(ws), B, T, E, G, _stream()), "groupnorm_bwd")
    return (dx, part) if defer else (dx, dgamma, dbeta)


def groupnorm_bwd_packs_rows(B: int, T: int, E: int, G: int = 8) -> int:
    """column-sum partial rows per sample groupnorm_bwd_packs writes for this shape (0: not supported)"""
    return int(_lib.load().dpot_groupnorm_bwd_packs_rows(B, T, E, G))


def groupnorm_bwd_packs_supported(T: int, E: int, G: int = 8, B: int = 1) -> bool:
    return groupnorm_bwd_packs_rows(B, T, E, G) > 0


def groupnorm_bwd_packs(dy: Tensor, x: Tensor, mean: Tensor, rstd: Tensor, gamma: Tensor, G: int = 8,
                        add: Optional[Tensor] = None):
    """groupnorm_bwd(defer=True) that also writes dx as the bf16 operand packs of the previous block's channel-MLP backward:
    returns (dx, part [2,B,E], dx row-form pack, dx transposed pack, column sums of dx [B * rows, E] over `rows` token ranges
    per sample) - the last three are what bf16_pack_both(dx, want_colsum=True) would produce from a second pass over dx"""
    B, T, E = x.shape
    lib = _lib.load()
    rows = lib.dpot_groupnorm_bwd_packs_rows(B, T, E, G)
    dx = torch.empty_like(x)
    part = torch.empty(2, B, E, dtype=torch.float32, device=x.device)
    pr = torch.empty(lib.dpot_bf16_packed_elems(B * T, E, 1), dtype=torch.bfloat16, device=x.device)
    pt = torch.empty(lib.dpot_bf16_packed_elems(E, B * T, 1), dtype=torch.bfloat16, device=x.device)
    cs = torch.empty(B * max(rows, 1), E, dtype=torch.float32, device=x.device)
    ws = _gn_workspace(B, T, E, G, x.device)
    check(lib.dpot_groupnorm_bwd_packs(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                       _p(add), dx.data_ptr(), part.data_ptr(), pr.data_ptr(), pt.data_ptr(), cs.data_ptr(),
                                       _p(ws), B, T, E, G, _stream()), "groupnorm_bwd_packs")
    return dx, part, pr, pt, cs


def groupnorm_param_grads(jobs):
    """jobs = [(part [2,B,E], out_dgamma | None, out_dbeta | None)] (<= 4) -> [(dgamma, dbeta)], one launch"""
    n = len(jobs)
    _, B, E = jobs[0][0].shape
    outs = [(_out(og, (E,), p.device), _out(ob, (E,), p.device)) for p, og, ob in jobs]
    parts = (C.c_void_p * n)(*[p.data_ptr() for p, _, _ in jobs])
    dgs = (C.c_void_p * n)(*[g.data_ptr() for g, _ in outs])
    dbs = (C.c_void_p * n)(*[b.data_ptr() for _, b in outs])
    check(_lib.load().dpot_groupnorm_param_grads(parts, dgs, dbs, n, B, E, _stream()), "groupnorm_param_grads")
    return outs


# ------------------------------------------------------------------------------------------------------
# GroupNorm fused with the mixer's DFTs (csrc/gn_dft.hip)
# ------------------------------------------------------------------------------------------------------
def gn_dft_supported(h: int, w: int, E: int, G: int = 8) -> bool:
    """16x16 latent grid and 64 / 128 channels per group (DPOT-Tiny / -Small / -Medium at 128^2); DPOT_TUNE gn_fuse=0 disables"""
    return bool(_lib.load().dpot_gn_dft_supported(h, w, E, G))


def gn_rfft2(x: Tensor, gamma: Tensor, beta: Tensor, h: int, w: int, nb: int, mx: int, my: int, G: int = 8,
             eps: float = 1e-5):
    """(spec [B*mx*my, 2E] = rfft2(GroupNorm(x)), mean [B,G], rstd [B,G]) in one launch; GroupNorm(x) is not written"""
    B, _, E = x.shape
    spec = torch.empty(B * mx * my, 2 * E, dtype=torch.float32, device=x.device)
    mean = torch.empty(B, G, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B, G, dtype=torch.float32, device=x.device)
    check(_lib.load().dpot_gn_rfft2(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), spec.data_ptr(), mean.data_ptr(),
                                    rstd.data_ptr(), B, h, w, E, G, nb, mx, my, eps, _stream()), "gn_rfft2")
    return spec, mean, rstd


def irfft2_gn(spec: Tensor, x: Tensor, mean1: Tensor, rstd1: Tensor, g1: Tensor, b1: Tensor, g2: Tensor, b2: Tensor,
              h: int, w: int, nb: int, mx: int, my: int, G: int = 8, eps: float = 1e-5, col_weights: int = 1,
              want_xn2: bool = True):
    """(y1 = irfft2(spec) + GroupNorm1(x), xn2 = GroupNorm2(y1), mean2, rstd2) in one launch; want_xn2=False: statistics
    only (xn2 = None: the bf16 channel MLP packs GroupNorm2(y1) itself, bf16_pack_both(norm=...))"""
    B, _, E = x.shape
    y1, xn2 = torch.empty_like(x), (torch.empty_like(x) if want_xn2 else None)
    mean2 = torch.empty(B, G, dtype=torch.float32, device=x.device)
    rstd2 = torch.empty(B, G, dtype=torch.float32, device=x.device)
    check(_lib.load().dpot_irfft2_gn(spec.data_ptr(), x.data_ptr(), mean1.data_ptr(), rstd1.data_ptr(), g1.data_ptr(),
                                     b1.data_ptr(), g2.data_ptr(), b2.data_ptr(), y1.data_ptr(), _p(xn2),
                                     mean2.data_ptr(), rstd2.data_ptr(), B, h, w, E, G, nb, mx, my, col_weights, eps,
                                     _stream()), "irfft2_gn")
    return y1, xn2, mean2, rstd2


def afno_layer_mode() -> int:
    """DPOT_TUNE afno_layer: 0 = never the one-launch AFNO layer (csrc/afno_fused.hip), 1 = wherever it is supported, -1
    (default) = where it measured faster than the three-launch form (afno_layer_wins)"""
    return tune("afno_layer")


def afno_layer_wins(B: int, nb: int) -> bool:
    """one (sample, channel block) workgroup per CU and round: the one-launch layer costs ~100 us per round of 256
    workgroups whatever their number, the three launches ~125 us per 256 (profiles/r05_f4_fused_vs_3launch.txt: 128
    workgroups 84 vs 72 us - DPOT-Tiny at batch 32 stays on three launches -, 256: 98 vs 124, 512: 196 vs 240) - so it
    is selected where the last round is at least 80 % full"""
    n = B * nb
    rounds = (n + 255) // 256
    return n >= 0.8 * 256 * rounds


def afno_fused_supported(h: int, w: int, E: int, nb: int, mx: int, my: int, G: int = 8, B: Optional[int] = None,
                         layout: int = 1) -> bool:
    """one-launch AFNO layer forward: 16x16 latent grid, 128 channels per block, all modes kept, three-product packs"""
    mode = afno_layer_mode()
    if mode == 0 or layout != 1 or not _lib.load().dpot_afno_fused_supported(h, w, E, G, nb, mx, my):
        return False
    return mode == 1 or (B is not None and afno_layer_wins(B, nb))


def afno_fused_fwd(x: Tensor, g1: Optional[Tensor], b1: Optional[Tensor], WaT: Tensor, ba: Tensor, WbT: Tensor, bb: Tensor,
                   g2: Optional[Tensor], b2: Optional[Tensor], h: int, w: int, nb: int, mx: int, my: int, act: int,
                   G: int = 8, eps: float = 1e-5, save: bool = True, want_y1: bool = True, want_xn2: bool = True,
                   want_packs: bool = False, packs_trans: bool = True):
    """[GroupNorm1] -> rfft2 -> 2-layer complex MLP -> irfft2 + x_orig -> [GroupNorm2] in ONE launch (csrc/afno_fused.hip).
    Returns (S, O1pre, y1, xn2, mean1, rstd1, mean2, rstd2) - the tensors gn_rfft2 / afno_mlp2 / irfft2_gn return, same
    layouts; save=False (inference): S = O1pre = None; entries that do not apply are None.
    want_packs (with g2): two more entries (xp, xpT) = GroupNorm2(y1) as the bf16 operand packs of the channel MLP (what
    bf16_pack_both(y1, norm=...) returns), written by the same launch; packs_trans=False: xpT = None (inference: only the
    weight gradient reads the transposed form)"""
    B, tok, E = x.shape
    dev = x.device
    Mm = B * mx * my
    S = torch.empty(Mm, 2 * E, dtype=torch.float32, device=dev) if save else None
    pre = torch.empty(Mm, 2 * E, dtype=torch.float32, device=dev) if save else None
    want_xn2 = want_xn2 and g2 is not None
    want_packs = want_packs and g2 is not None
    y1 = torch.empty_like(x) if (want_y1 or not (want_xn2 or want_packs)) else None
    xn2 = torch.empty_like(x) if want_xn2 else None
    st = [torch.empty(B, G, dtype=torch.float32, device=dev) if g is not None else None for g in (g1, g1, g2, g2)]
    lib = _lib.load()
    xp = xpT = None
    if want_packs:
        n = lib.dpot_bf16_packed_elems(B * tok, E, 1)
        xp = torch.empty(n, dtype=torch.bfloat16, device=dev)
        xpT = torch.empty(lib.dpot_bf16_packed_elems(E, B * tok, 1), dtype=torch.bfloat16, device=dev) if packs_trans else None
    check(lib.dpot_afno_fused_fwd(x.data_ptr(), _p(g1), _p(b1), WaT.data_ptr(), _p(ba), WbT.data_ptr(), _p(bb),
                                  _p(g2), _p(b2), _p(S), _p(pre), _p(y1), _p(xn2), _p(st[0]), _p(st[1]),
                                  _p(st[2]), _p(st[3]), _p(xp), _p(xpT), B, h, w, E, G, nb, mx, my, act, eps, _stream()),
          "afno_fused_fwd")
    if want_packs:
        return S, pre, y1, xn2, st[0], st[1], st[2], st[3], xp, xpT
    return S, pre, y1, xn2, st[0], st[1], st[2], st[3]


def gn_bwd_rfft2(dy: Tensor, xin: Tensor, mean: Tensor, rstd: Tensor, gamma: Tensor, h: int, w: int, nb: int, mx: int,
                 my: int, G: int = 8, col_weights: int = 1):
    """(dx = GroupNorm backward of dy, part [2,B,E], spec = rfft2(dx; col_weights)) in one launch"""
    B, _, E = xin.shape
    dx = torch.empty_like(xin)
    part = torch.empty(2, B, E, dtype=torch.float32, device=xin.device)
    spec = torch.empty(B * mx * my, 2 * E, dtype=torch.float32, device=xin.device)
    check(_lib.load().dpot_gn_bwd_rfft2(dy.data_ptr(), xin.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                        dx.data_ptr(), part.data_ptr(), spec.data_ptr(), B, h, w, E, G, nb, mx, my,
                                        col_weights, _stream()), "gn_bwd_rfft2")
    return dx, part, spec


def irfft2_gn_bwd(spec: Tensor, res: Tensor, xin: Tensor, mean: Tensor, rstd: Tensor, gamma: Tensor, h: int, w: int,
                  nb: int, mx: int, my: int, add: Optional[Tensor] = None, G: int = 8, col_weights: int = 0):
    """(dx = GroupNorm backward of (irfft2(spec; col_weights) + res) (+ add), part [2,B,E]) in one launch"""
    B, _, E = xin.shape
    dx = torch.empty_like(xin)
    part = torch.empty(2, B, E, dtype=torch.float32, device=xin.device)
    check(_lib.load().dpot_irfft2_gn_bwd(spec.data_ptr(), res.data_ptr(), xin.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                         gamma.data_ptr(), _p(add), dx.data_ptr(), part.data_ptr(), B, h, w, E, G, nb, mx,
                                         my, col_weights, _stream()), "irfft2_gn_bwd")
    return dx, part


# ------------------------------------------------------------------------------------------------------
# data movement / small ops
# ------------------------------------------------------------------------------------------------------
def patchify(x: Tensor, gx: Tensor, gy: Tensor, gt: Tensor, P: int) -> Tensor:
    B, X, Y, T, Cc = x.shape
    K0 = (Cc + 3) * P * P
    A = torch.empty(B * (X // P) * (Y // P) * T, K0, dtype=torch.float32, device=x.device)
    check(_lib.load().dpot_patchify(x.data_ptr(), gx.data_ptr(), gy.data_ptr(), gt.data_ptr(), A.data_ptr(), B, X, Y,
                                    T, Cc, P, _stream()), "patchify")
    return A


def embed_supported(Cc: int, P: int, T: int, hid: int, w: int) -> bool:
    """shapes the implicit-GEMM patch embedding covers (csrc/embed.hip); DPOT_TUNE embed_implicit=0 disables it"""
    return (tune("embed_implicit") != 0
            and bool(_lib.load().dpot_embed_supported(Cc, P, T, hid, w)))


def embed_pack_w0(w0: Tensor) -> Tensor:
    lib = _lib.load()
    wf = torch.empty(lib.dpot_embed_wfrag_elems(), dtype=torch.float32, device=w0.device)
    check(lib.dpot_embed_pack_w0(w0.data_ptr(), w0.shape[0], wf.data_ptr(), _stream()), "embed_pack_w0")
    return wf


def embed_fwd(x: Tensor, wfrag: Tensor, btab: Tensor, hidp: int, act: int) -> Tuple[Tensor, Tensor]:
    """(Hh, Hpre) [B*tok*T, hidp] of the patch convolution, gathered from x[B,X,Y,T,4] (no patch matrix)"""
    B, X, Y, T, _ = x.shape
    M0 = B * (X // 8) * (Y // 8) * T
    hpre = torch.empty(M0, hidp, dtype=torch.float32, device=x.device)
    hh = torch.empty_like(hpre)
    check(_lib.load().dpot_embed_fwd(x.data_ptr(), wfrag.data_ptr(), btab.data_ptr(), hpre.data_ptr(), hh.data_ptr(),
                                     B, X, Y, T, hidp, act, _stream()), "embed_fwd")
    return hh, hpre


def embed_wgrad(x: Tensor, dhpre: Tensor, dw0: Tensor, hid: int) -> Tensor:
    """data-channel columns of the patch-conv weight gradient: dw0[hid, K0][:, :4*64] (deterministic two-launch sum)"""
    lib = _lib.load()
    B, X, Y, T, _ = x.shape
    ws = _scratch(torch.empty(lib.dpot_embed_wgrad_ws_elems(B, X, Y), dtype=torch.float32, device=x.device))
    check(lib.dpot_embed_wgrad(x.data_ptr(), dhpre.data_ptr(), ws.data_ptr(), dw0.data_ptr(), dw0.stride(0), hid, B, X,
                               Y, T, dhpre.shape[1], _stream()), "embed_wgrad")
    return dw0


def unpatchify(dA: Tensor, B: int, X: int, Y: int, T: int, Cc: int, P: int) -> Tensor:
    dx = torch.empty(B, X, Y, T, Cc, dtype=torch.float32, device=dA.device)
    check(_lib.load().dpot_unpatchify(dA.data_ptr(), dx.data_ptr(), B, X, Y, T, Cc, P, _stream()), "unpatchify")
    return dx


def pixel_shuffle(z: Tensor, B: int, h: int, w: int, P: int, Cc: int, inverse: bool = False) -> Tensor:
    """inverse=False: z[(b,px,py,i,j),Cc] -> out[b,px*P+i,py*P+j,Cc];  inverse=True: the other way."""
    out = torch.empty(B * h * w * P * P, Cc, dtype=torch.float32, device=z.device)
    if not inverse:
        out = out.view(B, h * P, w * P, Cc)
        check(_lib.load().dpot_pixel_shuffle(z.data_ptr(), out.data_ptr(), B, h, w, P, Cc, 0, _stream()),
              "pixel_shuffle")
    else:
        check(_lib.load().dpot_pixel_shuffle(z.data_ptr(), out.data_ptr(), B, h, w, P, Cc, 1, _stream()),
              "pixel_shuffle")
    return out


def _patch3_dims(what: str, S: int, P: int) -> int:
    if P < 1 or S < 1 or S % P != 0:
        raise _lib.DpotHipError(f"{what}: the grid size {S} is not a multiple of the patch size {P}")
    return S // P


def patchify3(x: Tensor, gs: Tensor, gt: Tensor, P: int) -> Tensor:
    """x[B,S,S,S,T,C] -> the patch matrix A[(b,t,hx,hy,hz), (c,i,j,k)] of DPOTNet3D's k = s = P patch convolution, with the four
    coordinate channels C..C+3 = gs[x], gs[y], gs[z], gt[t] written from the tables gs[S], gt[T] (csrc/patch3d.hip)"""
    if x.dim() != 6 or not (x.shape[1] == x.shape[2] == x.shape[3]):
        raise _lib.DpotHipError(f"patchify3: expected x[B,S,S,S,T,C], got {tuple(x.shape)}")
    B, S, _, _, T, Cc = x.shape
    h = _patch3_dims("patchify3", S, P)
    _req(x, "x"), _req(gs, "gs"), _req(gt, "gt")
    if gs.numel() != S or gt.numel() != T:
        raise _lib.DpotHipError(f"patchify3: coordinate tables of {gs.numel()} / {gt.numel()} entries for S = {S}, T = {T}")
    A = torch.empty(B * T * h ** 3, (Cc + 4) * P ** 3, dtype=torch.float32, device=x.device)
    check(_lib.load().dpot_patchify3(x.data_ptr(), gs.data_ptr(), gt.data_ptr(), A.data_ptr(), B, S, T, Cc, P, _stream()),
          "patchify3")
    return A


def unpatchify3(dA: Tensor, B: int, S: int, T: int, Cc: int, P: int) -> Tensor:
    """adjoint of patchify3 w.r.t. x: dA[B*T*h^3, (Cc+4)*P^3] -> dx[B,S,S,S,T,Cc] (the coordinate columns are dropped)"""
    h = _patch3_dims("unpatchify3", S, P)
    _req(dA, "dA")
    if tuple(dA.shape) != (B * T * h ** 3, (Cc + 4) * P ** 3):
        raise _lib.DpotHipError(f"unpatchify3: dA {tuple(dA.shape)} is not [{B * T * h ** 3}, {(Cc + 4) * P ** 3}]")
    dx = torch.empty(B, S, S, S, T, Cc, dtype=torch.float32, device=dA.device)
    check(_lib.load().dpot_unpatchify3(dA.data_ptr(), dx.data_ptr(), B, S, T, Cc, P, _stream()), "unpatchify3")
    return dx


def fold3(t: Tensor, B: int, h: int, P: int, old: int, inverse: bool = False) -> Tensor:
    """inverse=False: t[B*h^3, old*P^3] (columns (o,i,j,k)) -> [B*(hP)^3, old] (rows (b,x,y,z)), the scatter of a k = s = P
    transposed 3-D convolution;  inverse=True: the other way"""
    if h < 1 or P < 1:
        raise _lib.DpotHipError(f"fold3: bad grid h = {h}, P = {P}")
    _req(t, "t")
    rows, cols = (B * h ** 3, old * P ** 3), (B * (h * P) ** 3, old)
    want, out = (cols, rows) if inverse else (rows, cols)
    if tuple(t.shape) != want:
        raise _lib.DpotHipError(f"fold3: got {tuple(t.shape)}, expected {want}")
    dst = torch.empty(out, dtype=torch.float32, device=t.device)
    check(_lib.load().dpot_fold3(t.data_ptr(), dst.data_ptr(), B, h, P, old, int(inverse), _stream()), "fold3")
    return dst


def copy2d_pad(src: Tensor, sR: int, sC: int, dR: int, dC: int, out: Optional[Tensor] = None) -> Tensor:
    dst = _out(out, (dR, dC), src.device)
    check(_lib.load().dpot_copy2d_pad(src.data_ptr(), sR, sC, dst.data_ptr(), dR, dC, _stream()), "copy2d_pad")
    return dst


def transpose2d(src: Tensor, nbatch: int, R: int, Cn: int, out: Optional[Tensor] = None) -> Tensor:
    dst = _out(out, (nbatch, Cn, R), src.device)
    check(_lib.load().dpot_transpose2d(src.data_ptr(), dst.data_ptr(), nbatch, R, Cn, _stream()), "transpose2d")
    return dst


def colsum(X: Tensor, M: int, N: int, ld: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    lib = _lib.load()
    out = _out(out, (N,), X.device)
    part = _scratch(torch.empty(lib.dpot_colsum_parts(M), N, dtype=torch.float32, device=X.device))
    check(lib.dpot_colsum(X.data_ptr(), M, N, ld or N, out.data_ptr(), part.data_ptr(), _stream()), "colsum")
    return out


def group_rowsum(X: Tensor, B: int, R: int, T: int, N: int) -> Tensor:
    out = torch.empty(R, N, dtype=torch.float32, device=X.device)
    check(_lib.load().dpot_group_rowsum(X.data_ptr(), out.data_ptr(), B, R, T, N, _stream()), "group_rowsum")
    return out


def token_mean(x: Tensor) -> Tensor:
    B, T, E = x.shape
    y = torch.empty(B, E, dtype=torch.float32, device=x.device)
    check(_lib.load().dpot_token_mean(x.data_ptr(), y.data_ptr(), B, T, E, _stream()), "token_mean")
    return y


def token_mean_bwd(dy: Tensor, T: int, add: Optional[Tensor] = None) -> Tensor:
    B, E = dy.shape
    dx = torch.empty(B, T, E, dtype=torch.float32, device=dy.device)
    check(_lib.load().dpot_token_mean_bwd(dy.data_ptr(), _p(add), dx.data_ptr(), B, T, E, _stream()),
          "token_mean_bwd")
    return dx


def bias_add(x: Tensor, v: Tensor) -> Tensor:
    """y[r, n] = x[r, n] + v[n]"""
    R, N = x.shape
    y = torch.empty_like(x)
    check(_lib.load().dpot_bias_add(x.data_ptr(), v.data_ptr(), y.data_ptr(), R, N, _stream()), "bias_add")
    return y


def tile_vec(v: Tensor, reps: int) -> Tensor:
    """v [N] repeated `reps` times -> [reps * N]"""
    N = v.numel()
    y = torch.empty(reps * N, dtype=torch.float32, device=v.device)
    check(_lib.load().dpot_bias_add(None, v.data_ptr(), y.data_ptr(), reps, N, _stream()), "tile_vec")
    return y


def scale_shift(x: Tensor, scale: Tensor, shift: Tensor) -> Tensor:
    B, T, E = x.shape
    y = torch.empty_like(x)
    check(_lib.load().dpot_scale_shift(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), B, T, E,
                                       _stream()), "scale_shift")
    return y


def scale_shift_bwd(dy: Tensor, x: Tensor, scale: Tensor):
    B, T, E = x.shape
    dx = torch.empty_like(x)
    dscale = torch.empty(B, E, dtype=torch.float32, device=x.device)
    dshift = torch.empty_like(dscale)
    check(_lib.load().dpot_scale_shift_bwd(dy.data_ptr(), x.data_ptr(), scale.data_ptr(), dx.data_ptr(),
                                           dscale.data_ptr(), dshift.data_ptr(), B, T, E, _stream()), "scale_shift_bwd")
    return dx, dscale, dshift


def timeagg_scale_w(w: Tensor, gamma: Tensor, tt: Tensor) -> Tensor:
    T, E, _ = w.shape
    ws = torch.empty_like(w)
    check(_lib.load().dpot_timeagg_scale_w(w.data_ptr(), gamma.data_ptr(), tt.data_ptr(), ws.data_ptr(), T, E,
                                           _stream()), "timeagg_scale_w")
    return ws


def timeagg_scale_w_bwd(dws: Tensor, w: Tensor, gamma: Tensor, tt: Tensor, out_dw: Optional[Tensor] = None,
                        out_dgamma: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    T, E, _ = w.shape
    dw = _out(out_dw, (T, E, E), w.device)
    dgamma = _out(out_dgamma, (1, E), w.device)
    check(_lib.load().dpot_timeagg_scale_w_bwd(dws.data_ptr(), w.data_ptr(), gamma.data_ptr(), tt.data_ptr(),
                                               dw.data_ptr(), dgamma.data_ptr(), T, E, _stream()),
          "timeagg_scale_w_bwd")
    return dw, dgamma


def out_tail_supported(old: int, co: int, n_pixels: int) -> bool:
    return old == 32 and 0 < co <= 32 and n_pixels % 32 == 0


def out_tail_pad(w4: Tensor, b4: Tensor, co: int) -> Tuple[Tensor, Tensor]:
    """W4 [co,32] -> [32,32], b4 [co] -> [32], zero padded (the tail kernels load them unconditionally)"""
    return copy2d_pad(w4, co, 32, 32, 32), copy2d_pad(b4, 1, co, 1, 32).view(32)


def out_tail_fwd(upre: Tensor, w2: Tensor, b2: Tensor, w4p: Tensor, b4p: Tensor, B: int, h: int, w: int, P: int,
                 co: int, act: int) -> Tensor:
    out = torch.empty(B, h * P, w * P, co, dtype=torch.float32, device=upre.device)
    check(_lib.load().dpot_out_tail_fwd(upre.data_ptr(), w2.data_ptr(), b2.data_ptr(), w4p.data_ptr(),
                                        b4p.data_ptr(), out.data_ptr(), B, h, w, P, co, act, _stream()), "out_tail_fwd")
    return out


def colsum_scatter(X: Tensor, M: int, N: int, segments) -> None:
    """column sums of X[M,N]; segments = [(first column, tensor)]: each tensor receives its columns (one launch pair)"""
    lib = _lib.load()
    n = len(segments)
    starts = (C.c_int * n)(*[s for s, _ in segments])
    lens = (C.c_int * n)(*[t.numel() for _, t in segments])
    dsts = (C.c_void_p * n)(*[t.data_ptr() for _, t in segments])
    part = torch.empty(lib.dpot_colsum_parts(M) * N, dtype=torch.float32, device=X.device)
    check(lib.dpot_colsum_scatter(X.data_ptr(), M, N, N, part.data_ptr(), n, starts, lens, dsts, _stream()),
          "colsum_scatter")


def out_tail_bwd(upre: Tensor, dout: Tensor, w2: Tensor, b2: Tensor, w4p: Tensor, B: int, h: int, w: int, P: int,
                 co: int, act: int, outs=None):
    """returns (dupre [pixels,32], (dW2 [32,32], dW4 [co,32], db2 [32], colsum(dupre) [32], db4 [co])); `outs`: the five
    destination tensors (gradient slots) or None entries for fresh ones - all written by one reduction"""
    lib = _lib.load()
    rows, cols = lib.dpot_out_tail_partial_rows(B, h, w, P), lib.dpot_out_tail_partial_cols()
    dupre = torch.empty_like(upre)
    part = torch.empty(rows, cols, dtype=torch.float32, device=upre.device)
    check(lib.dpot_out_tail_bwd(upre.data_ptr(), dout.data_ptr(), w2.data_ptr(), b2.data_ptr(), w4p.data_ptr(),
                                dupre.data_ptr(), part.data_ptr(), B, h, w, P, co, act, _stream()), "out_tail_bwd")
    shapes = ((32, 32), (co, 32), (32,), (32,), (co,))
    starts = (0, 1024, 2048, 2080, 2112)
    outs = list(outs) if outs is not None else [None] * 5
    res = [_out(o, shp, upre.device) for o, shp in zip(outs, shapes)]
    colsum_scatter(part, rows, cols, list(zip(starts, res)))
    return dupre, tuple(res)


# ------------------------------------------------------------------------------------------------------
# loss / optimiser
# ------------------------------------------------------------------------------------------------------
def rel_l2_fwd(x: Tensor, y: Tensor, mask: Optional[Tensor], B: int, S: int, Cc: int, Tt: int,
               stats: Optional[Tensor] = None):
    """stats: a caller-owned buffer of >= rel_l2_stats_elems(B, S, Cc) floats to use instead of a fresh one (the per-step
    slot of train.StepMetrics: rel_l2_combine then reads every step's statistics from one strided buffer)"""
    nch = _lib.load().dpot_rel_l2_chunks(S, Cc)
    if stats is None:
        stats = torch.empty(1 + nch, B, Cc, 4, dtype=torch.float32, device=x.device)
    else:
        _req(stats, "stats")
        if stats.numel() < (1 + nch) * B * Cc * 4 or stats.data_ptr() % 16:
            raise _lib.DpotHipError(f"rel_l2_fwd: the stats slot needs {(1 + nch) * B * Cc * 4} floats, 16-byte aligned")
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    check(_lib.load().dpot_rel_l2_fwd(x.data_ptr(), y.data_ptr(), _p(mask), stats.data_ptr(), loss.data_ptr(), B, S,
                                      Cc, Tt, _stream()), "rel_l2_fwd")
    return loss, stats


def rel_l2_bwd(x: Tensor, y: Tensor, mask: Optional[Tensor], stats: Tensor, gloss: Tensor, B: int, S: int, Cc: int,
               Tt: int) -> Tensor:
    dx = torch.empty_like(x)
    check(_lib.load().dpot_rel_l2_bwd(x.data_ptr(), y.data_ptr(), _p(mask), stats.data_ptr(), gloss.data_ptr(),
                                      dx.data_ptr(), B, S, Cc, Tt, _stream()), "rel_l2_bwd")
    return dx


# ---- training metrics (csrc/metrics.hip) ------------------------------------------------------------------------------
CLS_OUT_WORDS = 4        # struct dpot_cls_ce_out as int64 words: {float loss + pad, correct, valid, invalid}
METRICS_WORDS = 12       # struct dpot_metrics as 8-byte words: 4 doubles, then 8 int64
METRICS_FLOATS = ("l2_step", "l2_full", "cls_loss", "grad_norm")
METRICS_INTS = ("cls_correct", "cls_total", "cls_invalid", "samples", "ar_steps", "opt_steps", "nonfinite_steps")


def _req_labels(labels: Tensor, B: int) -> Tensor:
    if not labels.is_cuda:
        raise _lib.DpotHipError(f"labels must live on the MI355X (got a {labels.device} tensor): dpot_amd has no CPU path")
    if labels.dtype != torch.int64 or not labels.is_contiguous() or labels.numel() != B:
        raise _lib.DpotHipError(f"labels must be {B} contiguous int64 values, got {tuple(labels.shape)} {labels.dtype}")
    return labels


def cls_ce_fwd(logits: Tensor, labels: Tensor, out: Optional[Tensor] = None):
    """CrossEntropyLoss(reduction='sum') + argmax accuracy of logits [B, n_cls] against int64 labels [B] (or [B, 1]), one
    launch.  Returns (out, row_stats): `out` = 4 int64 words holding struct dpot_cls_ce_out - word 0 is the float32 loss
    (`cls_out_loss(out)`), then correct, valid, invalid; row_stats [B, 2] = {row max, log-sum-exp} for `cls_ce_bwd`.
    A label outside [0, n_cls) reads no memory: its row adds nothing to the loss or the counts and is counted in `invalid`
    (nothing aborts - check `invalid` where the labels are not trusted).  `out`: a caller-owned slot (StepMetrics)."""
    _req(logits, "logits")
    if logits.dim() != 2:
        raise _lib.DpotHipError(f"logits must be [B, n_cls], got {tuple(logits.shape)}")
    B, n_cls = logits.shape
    _req_labels(labels, B)
    if out is None:
        out = torch.empty(CLS_OUT_WORDS, dtype=torch.int64, device=logits.device)
    elif out.dtype != torch.int64 or out.numel() != CLS_OUT_WORDS or not out.is_contiguous() or out.device != logits.device:
        raise _lib.DpotHipError(f"cls_ce_fwd: out must be {CLS_OUT_WORDS} contiguous int64 words on {logits.device}")
    row_stats = torch.empty(B, 2, dtype=torch.float32, device=logits.device)
    check(_lib.load().dpot_cls_ce_fwd(logits.data_ptr(), labels.data_ptr(), row_stats.data_ptr(), out.data_ptr(), B, n_cls,
                                      _stream()), "cls_ce_fwd")
    return out, row_stats


def cls_out_loss(out: Tensor) -> Tensor:
    """the float32 loss of a dpot_cls_ce_out slot, as a 0-d view (no launch)"""
    return out.view(torch.float32)[0]


def cls_ce_bwd(logits: Tensor, labels: Tensor, row_stats: Tensor, gloss: Tensor) -> Tensor:
    """gloss[0] * (softmax(logits) - onehot(labels)); zeros for the rows whose label is outside [0, n_cls)"""
    _req(logits, "logits")
    _req(row_stats, "row_stats")
    _req(gloss, "gloss")
    B, n_cls = logits.shape
    _req_labels(labels, B)
    dl = torch.empty_like(logits)
    check(_lib.load().dpot_cls_ce_bwd(logits.data_ptr(), labels.data_ptr(), row_stats.data_ptr(), gloss.data_ptr(),
                                      dl.data_ptr(), B, n_cls, _stream()), "cls_ce_bwd")
    return dl


def rel_l2_stats_elems(B: int, S: int, Cc: int) -> int:
    """floats of the `stats` buffer of one rel_l2_fwd call (its first B*Cc*4 are what rel_l2_combine reads)"""
    return (1 + _lib.load().dpot_rel_l2_chunks(S, Cc)) * B * Cc * 4


class StatsTable:
    """DEVICE table of the per-step `stats` pointers for `rel_l2_combine` when the steps' buffers are separate tensors.
    Built once (one host-to-device copy); valid while the tensors it names live - it keeps them alive."""

    def __init__(self, stats):
        self.stats = [_req(s, "stats") for s in stats]
        if not self.stats:
            raise ValueError("StatsTable: need at least one step")
        if any(s.data_ptr() % 16 for s in self.stats):
            raise _lib.DpotHipError("StatsTable: every stats buffer must be 16-byte aligned")
        self.n_steps = len(self.stats)
        self.table = torch.tensor([s.data_ptr() for s in self.stats], dtype=torch.int64).to(self.stats[0].device)


def rel_l2_combine(stats, B: int, Cc: int, n_steps: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """relative L2 of the WHOLE rollout (SimpleLpLoss of the predictions concatenated along time) from the statistics the
    per-step rel_l2_fwd calls left - no second pass over the fields.  stats: a StatsTable, or ONE contiguous tensor
    [n_steps, >= B*Cc*4] whose row t is step t's stats buffer.  Returns a 1-element float32 tensor."""
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=(stats.table if isinstance(stats, StatsTable) else stats).device)
    if isinstance(stats, StatsTable):
        n = stats.n_steps if n_steps is None else n_steps
        if not 0 < n <= stats.n_steps or any(s.numel() < B * Cc * 4 for s in stats.stats[:n]):
            raise _lib.DpotHipError("rel_l2_combine: the table does not hold n_steps buffers of >= B*C*4 floats")
        args = (stats.table.data_ptr(), None, 0)
    else:
        _req(stats, "stats")
        if stats.dim() != 2 or stats.shape[1] < B * Cc * 4:
            raise _lib.DpotHipError(f"rel_l2_combine: stats must be [n_steps, >= {B * Cc * 4}], got {tuple(stats.shape)}")
        n = stats.shape[0] if n_steps is None else n_steps
        if not 0 < n <= stats.shape[0]:
            raise _lib.DpotHipError(f"rel_l2_combine: n_steps {n} outside (0, {stats.shape[0]}]")
        args = (None, stats.data_ptr(), stats.stride(0))
    check(_lib.load().dpot_rel_l2_combine(*args, n, B, Cc, out.data_ptr(), _stream()), "rel_l2_combine")
    return out


def metrics_accum(acc: Tensor, l2_step: Optional[Tensor], l2_full: Optional[Tensor], cls_out: Optional[Tensor], n_cls_out: int,
                  sumsq_: Optional[Tensor], grad_scale: float, samples: int, ar_steps: int, opt_steps: int) -> None:
    """acc (int64 [2, METRICS_WORDS] = two struct dpot_metrics): acc[0] += this step's values, acc[1] = them; one launch"""
    if not acc.is_cuda:
        raise _lib.DpotHipError(f"the metrics accumulator must live on the MI355X (got a {acc.device} tensor): no CPU path")
    if acc.dtype != torch.int64 or acc.numel() != 2 * METRICS_WORDS or not acc.is_contiguous():
        raise _lib.DpotHipError(f"metrics_accum: acc must be {2 * METRICS_WORDS} contiguous int64 words")
    if n_cls_out and (cls_out is None or cls_out.numel() < n_cls_out * CLS_OUT_WORDS):
        raise _lib.DpotHipError("metrics_accum: cls_out holds fewer than n_cls_out results")
    check(_lib.load().dpot_metrics_accum(acc.data_ptr(), _p(l2_step), _p(l2_full), _p(cls_out) if n_cls_out else None,
                                         n_cls_out, _p(sumsq_), grad_scale, samples, ar_steps, opt_steps, _stream()),
          "metrics_accum")


def sumsq(g: Tensor, out: Tensor, part: Tensor, accumulate: bool = False) -> Tensor:
    check(_lib.load().dpot_sumsq(g.data_ptr(), g.numel(), out.data_ptr(), part.data_ptr(), int(accumulate),
                                 _stream()), "sumsq")
    return out


def adam_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, hyper: Tensor, sumsq_: Optional[Tensor],
              grad_scale: float = 1.0) -> None:
    check(_lib.load().dpot_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                                     hyper.data_ptr(), _p(sumsq_), grad_scale, _stream()), "adam_step")


def adam_pair_ranges(ranges, device) -> Tensor:
    """the device table of dpot_adam_step_pairs: int64 [n, 2] of the [lo, hi) float ranges of a flat buffer that hold complex
    numbers as (re, im) pairs; ascending, disjoint, even bounds"""
    ranges = sorted((int(lo), int(hi)) for lo, hi in ranges)
    if not ranges or any(lo % 2 or hi % 2 or hi <= lo for lo, hi in ranges) \
            or any(a[1] > b[0] for a, b in zip(ranges, ranges[1:])):
        raise ValueError(f"adam_pair_ranges: non-empty, disjoint [lo, hi) ranges with even bounds, got {ranges}")
    return torch.tensor(ranges, dtype=torch.int64).to(device)


def adam_step_pairs(p: Tensor, g: Tensor, m: Tensor, v: Tensor, hyper: Tensor, sumsq_: Optional[Tensor], ranges_dev: Tensor,
                    grad_scale: float = 1.0) -> None:
    """dpot_adam_step with ONE second moment per (re, im) pair inside `ranges_dev` (adam_pair_ranges), the reference's Adam on
    complex parameters (utils/optimizer.py:41)"""
    check(_lib.load().dpot_adam_step_pairs(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), hyper.data_ptr(),
                                           _p(sumsq_), grad_scale, ranges_dev.data_ptr(), ranges_dev.shape[0], _stream()),
          "adam_step_pairs")


class AdamPackPlan:
    """Device tables of dpot_adam_step_packs for one (flat parameter buffer, PanelPacks of 1-plane bf16 weight packs): every
    weight W [R, K] (row-major inside the flat buffer) that the pack set holds as the pair (W, R, K, K, False) / (W, K, R, K,
    True) becomes a job whose 64 x 256 tiles run Adam AND write both packs; the rest of [0, n_active) becomes plain ranges of
    <= 2^20 elements.  None (`AdamPackPlan.build` returns None) when any weight of the set does not qualify."""
    MAX_RANGE = 1 << 20

    @staticmethod
    def build(flat: Tensor, n_active: int, pp: "PanelPacks"):
        lib = _lib.load()
        if not pp.bf16 or pp.planes != 1 or pp.n % 2:
            return None
        base, jobs = flat.data_ptr(), []
        for j in range(0, pp.n, 2):
            (w, rows, K, ld, tr), (w2, rows2, K2, ld2, tr2) = pp.jobs[j], pp.jobs[j + 1]
            off = (w.data_ptr() - base) // 4
            if (w2.data_ptr() != w.data_ptr() or tr or not tr2 or ld != K or ld2 != K or rows2 != K or K2 != rows
                    or (w.data_ptr() - base) % 16 or off < 0 or off + rows * K > n_active or not w.is_contiguous()
                    or w.numel() != rows * K or not lib.dpot_adam_pack_supported(rows, K)):
                return None
            jobs.append((off, rows, K, pp.bufs[j], pp.bufs[j + 1]))
        jobs.sort(key=lambda t: t[0])
        self = AdamPackPlan()
        self.pp = pp
        dev = flat.device
        ntiles, tile_job, tab = 0, [], []
        ranges, pos = [], 0
        for i, (off, R, K, drow, dtr) in enumerate(jobs):
            if off < pos:
                return None                                   # overlapping weights: not a layout this plan understands
            tab.append((off, drow.data_ptr(), dtr.data_ptr(), R, K, ntiles))
            nt = (R // 64) * (K // 256)
            tile_job += [i] * nt
            ntiles += nt
            ranges.append((pos, off - pos))
            pos = off + R * K
        ranges.append((pos, n_active - pos))
        split = []
        for st, ln in ranges:
            while ln > 0:
                c = min(ln, AdamPackPlan.MAX_RANGE)
                split.append((st, c))
                st, ln = st + c, ln - c
        self.ntiles, self.nranges = ntiles, len(split)
        self.max_range = max((c for _, c in split), default=0)
        self.jobs_dev = _device_table(_lib.AdamPackJob, tab, dev)
        self.tile_job_dev = torch.tensor(tile_job, dtype=torch.int32, device=dev)
        self.ranges_dev = torch.tensor(split, dtype=torch.int64).view(-1, 2).to(dev)
        return self


def adam_step_packs(plan: AdamPackPlan, p: Tensor, g: Tensor, m: Tensor, v: Tensor, hyper: Tensor, sumsq_: Optional[Tensor],
                    grad_scale: float = 1.0) -> None:
    """dpot_adam_step over the flat buffers whose channel-MLP weights ALSO leave as their two bf16 packs (plan.pp's buffers)"""
    check(_lib.load().dpot_adam_step_packs(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), hyper.data_ptr(), _p(sumsq_),
                                           grad_scale, plan.jobs_dev.data_ptr(), plan.tile_job_dev.data_ptr(), plan.ntiles,
                                           plan.ranges_dev.data_ptr() if plan.nranges else None, plan.nranges, plan.max_range,
                                           _stream()), "adam_step_packs")


def adam_stage(hyper: Tensor, step: Tensor, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
               max_norm: float, advance: int = 1) -> None:
    """step[0] += advance; hyper <- {lr, betas, eps, wd, bias corrections(step), max_norm}; every value travels by
    value in the launch packet (no host buffer that a later step could overwrite)"""
    check(_lib.load().dpot_adam_stage(hyper.data_ptr(), step.data_ptr(), lr, beta1, beta2, eps, weight_decay,
                                      max_norm, advance, _stream()), "adam_stage")


class LambPlan:
    """Device tables of dpot_lamb_step for one flat buffer: tensor k = the `numels[k]` elements at element offset
    `offsets[k]` (a multiple of 4; padding between tensors belongs to no chunk and is never read or written), cut into
    chunks of <= dpot_lamb_chunk_elems() elements that each lie in one tensor.  `part` is the per-chunk scratch of the
    norm reduction.  Built once on the host; the tables stay valid while the buffer does not move."""

    def __init__(self, offsets, numels, size: int, device):
        lib = _lib.load()
        ce = lib.dpot_lamb_chunk_elems()
        if not offsets or len(offsets) != len(numels):
            raise ValueError("LambPlan: need one offset per tensor and at least one tensor")
        chunks, tensors, end = [], [], 0
        for k, (off, n) in enumerate(zip(offsets, numels)):
            off, n = int(off), int(n)
            if off % 4 or n <= 0 or off < end or off + n > size:
                raise ValueError(f"LambPlan: tensor {k} at [{off}, {off + n}) is not a 4-aligned, ordered range of the "
                                 f"{size}-element buffer")
            tensors.append((len(chunks), (n + ce - 1) // ce))
            chunks += [(off + s, min(ce, n - s), k) for s in range(0, n, ce)]
            end = off + n
        self.size, self.nchunks, self.ntensors, self.chunk_elems = size, len(chunks), len(tensors), ce
        self.chunks_dev = _device_table(_lib.LambChunk, chunks, device)
        self.tensors_dev = _device_table(_lib.LambTensor, tensors, device)
        self.part = torch.zeros(2 * len(chunks), dtype=torch.float64, device=device)


def lamb_step(plan: LambPlan, p: Tensor, g: Tensor, m: Tensor, v: Tensor, hyper: Tensor, sumsq_: Optional[Tensor],
              norms: Tensor, grad_scale: float = 1.0, adam: bool = False) -> None:
    """one LAMB step over the tensors of `plan` (include/dpot_hip.h dpot_lamb_step); norms (3 * plan.ntensors floats)
    receives weight_norm, adam_norm and trust_ratio per tensor"""
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _req(t, name)
        if t.numel() < plan.size:
            raise _lib.DpotHipError(f"lamb_step: {name} has {t.numel()} elements, the plan addresses {plan.size}")
    if norms.dtype != torch.float32 or norms.numel() < 3 * plan.ntensors or not norms.is_contiguous():
        raise _lib.DpotHipError(f"lamb_step: norms must be >= {3 * plan.ntensors} contiguous float32")
    check(_lib.load().dpot_lamb_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), hyper.data_ptr(), _p(sumsq_),
                                     grad_scale, plan.chunks_dev.data_ptr(), plan.nchunks, plan.tensors_dev.data_ptr(),
                                     plan.ntensors, plan.part.data_ptr(), norms.data_ptr(), int(bool(adam)), _stream()),
          "lamb_step")


def lamb_stage(hyper: Tensor, step: Tensor, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
               max_norm: float, clamp_value: float, debias: bool, advance: int = 1) -> None:
    """step[0] += advance; hyper <- {betas, 1 - betas, eps, wd, max_norm, lr * bias correction(step), clamp_value} (>= 9
    floats), by value in the launch packet as adam_stage"""
    if hyper.numel() < 9:
        raise _lib.DpotHipError("lamb_stage: hyper needs >= 9 floats")
    check(_lib.load().dpot_lamb_stage(hyper.data_ptr(), step.data_ptr(), lr, beta1, beta2, eps, weight_decay, max_norm,
                                      clamp_value, int(bool(debias)), advance, _stream()), "lamb_stage")


_rng_states = {}


def rng_state(device) -> Tensor:
    """{seed, offset} of the in-kernel noise generator of `device` (int64[2]); seeded from torch.initial_seed()"""
    key = torch.device(device).index or 0
    if key not in _rng_states:
        _rng_states[key] = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64,
                                        device=device)
    return _rng_states[key]


def noise_dims(xx: Tensor) -> Tuple[int, int, int]:
    """(B, S, C') of the [B, S, C'] field the noise kernels see - one norm per (b, c') over S - chosen by the window's rank,
    for the forward and the backward alike:
      5-D [B,X,Y,T,C]    one norm per (b, c) over X*Y*T     (train_temporal.py:205):  S = X*Y*T, C' = C
      6-D [B,X,Y,Z,T,C]  one norm per (b, t, c) over X*Y*Z  (finetune3d.py:210):      S = X*Y*Z, C' = T*C
    (the kernels refuse C' > 256: the channel sum gives every channel a lane of a 256-thread block)"""
    if xx.dim() not in (5, 6):
        raise _lib.DpotHipError(f"noise_inject: expected a window [B,X,Y,T,C] or [B,X,Y,Z,T,C], got {tuple(xx.shape)}")
    B = xx.shape[0]
    Cc = xx.shape[-1] * (xx.shape[-2] if xx.dim() == 6 else 1)
    return B, xx.numel() // (B * Cc), Cc


def noise_inject(xx: Tensor, eps: Optional[Tensor], noise_scale: float, return_norms: bool = False):
    """xx + noise_scale * ||xx|| * eps with the norm of ``noise_dims`` (over X,Y,T per (b,c) for a 5-D window; over X,Y,Z per
    (b,t,c) for a 6-D one);  eps=None: eps ~ N(0,1) is drawn inside the kernel.
    return_norms: also return the scratch tensor whose first B*C' floats are the norms (for the backward)"""
    B, S, Cc = noise_dims(xx)
    out = torch.empty_like(xx)
    lib = _lib.load()
    norms = torch.empty(B * Cc * (1 + lib.dpot_noise_chunks(S, Cc)), dtype=torch.float32, device=xx.device)
    if eps is None:
        check(lib.dpot_noise_inject_rng(xx.data_ptr(), out.data_ptr(), norms.data_ptr(), rng_state(xx.device).data_ptr(),
                                        noise_scale, B, S, Cc, _stream()), "noise_inject_rng")
    else:
        check(lib.dpot_noise_inject(xx.data_ptr(), eps.data_ptr(), out.data_ptr(), norms.data_ptr(), noise_scale,
                                    B, S, Cc, _stream()), "noise_inject")
    return (out, norms) if return_norms else out


def noise_inject_bwd(xx: Tensor, eps: Optional[Tensor], rng_snapshot: Optional[Tensor], g: Tensor, norms: Tensor,
                     noise_scale: float) -> Tensor:
    """d/dxx of noise_inject: g + noise_scale * xx / ||xx|| * sum(g * eps); eps given, or re-drawn from the
    generator state the forward used (rng_snapshot = clone of rng_state() taken right after the forward call)"""
    B, S, Cc = noise_dims(xx)
    lib = _lib.load()
    dx = torch.empty_like(xx)
    part = torch.empty(B * Cc * lib.dpot_noise_chunks(S, Cc), dtype=torch.float32, device=xx.device)
    check(lib.dpot_noise_inject_bwd(xx.data_ptr(), _p(eps), _p(rng_snapshot), g.data_ptr(), norms.data_ptr(),
                                    dx.data_ptr(), part.data_ptr(), noise_scale, B, S, Cc, _stream()),
          "noise_inject_bwd")
    return dx


def window_slide(xx: Tensor, im: Tensor) -> Tensor:
    """cat(xx[..., Tb:, :], im) along the time axis of [B,X,Y,T,C] (train_temporal.py:219)"""
    T, Cc = xx.shape[-2], xx.shape[-1]
    Tb = im.shape[-2]
    # the reference's torch.cat raises when the prediction does not continue the window (out_channels != in_channels,
    # other leading dims); the kernel would read `im` with the wrong stride instead
    if im.shape[:-2] != xx.shape[:-2] or im.shape[-1] != Cc or Tb > T:
        raise _lib.DpotHipError(f"window_slide: prediction {tuple(im.shape)} does not continue the window {tuple(xx.shape)} "
                                f"(needs equal leading dims and channel count, T_bundle <= T_in)")
    rows = xx.numel() // (T * Cc)
    out = torch.empty_like(xx)
    check(_lib.load().dpot_window_slide(xx.data_ptr(), im.data_ptr(), out.data_ptr(), rows, T, Tb, Cc, _stream()),
          "window_slide")
    return out


def window_slide_bwd(dout: Tensor, Tb: int, need_xx: bool, need_im: bool):
    T, Cc = dout.shape[-2], dout.shape[-1]
    if not 0 < Tb <= T:
        raise _lib.DpotHipError(f"window_slide_bwd: T_bundle {Tb} outside (0, {T}]")
    rows = dout.numel() // (T * Cc)
    dxx = torch.empty_like(dout) if need_xx else None
    dim = torch.empty(dout.shape[:-2] + (Tb, Cc), dtype=torch.float32, device=dout.device) if need_im else None
    check(_lib.load().dpot_window_slide_bwd(dout.data_ptr(), _p(dxx), _p(dim), rows, T, Tb, Cc, _stream()),
          "window_slide_bwd")
    return dxx, dim


# ------------------------------------------------------------------------------------------------------
# Table plans: what the table-driven operators below (spectral resize, rollout metrics, anti-aliased activation, FNO transforms)
# share on the host - how a plan is built, guarded and cached, the output buffer check and the size parser
# ------------------------------------------------------------------------------------------------------
class _TablePlan:
    """The device-resident tables of one operator for one size tuple.  A subclass gives its `words` for the messages (class
    name, accessor, what the tables are called, what a size tuple is called, what else builds the plan), checks its sizes
    against the library (`_check`) and computes its tables on the host (`_host(*sizes)`: an ordered dict name -> numpy array or
    None; where a class has a public host function, that is it).
    The constructor does the rest, always in this order: `sizes`, the checks, the refusal to build while the stream is capturing
    (an upload is no graph node), the upload into `dev` - int32 tables as they are, every other one rounded once to fp32 on the
    host, None kept, in the host dict's order.  Plans are made through `_plan`, which caches them."""

    def __init__(self, sizes, device):
        self.sizes = tuple(sizes)
        self._check()
        if torch.cuda.is_current_stream_capturing():
            name, entry, tables, noun, instead = self.words
            raise _lib.DpotHipError(f"{name} {self.sizes}: the {tables} are uploaded when a {noun} is first used - call "
                                    f"ops.{entry}(...) {instead} before capturing")
        self.dev = {}
        for key, a in self._host(*self.sizes).items():
            if a is not None:
                h = torch.from_numpy(a if a.dtype == "int32" else a.astype("float32"))
                a = torch.empty(h.shape, dtype=h.dtype, device=device).copy_(h)
            self.dev[key] = a

    def _check_pads(self, pad, output_rows, sizes=None) -> None:
        """the class's pads() must be what the library's `pad` entry point answers for each size and its output_rows flag"""
        want = tuple(pad(n, rows) for n, rows in zip(sizes or self.sizes, output_rows))
        if want != self.pads(*self.sizes):
            raise _lib.DpotHipError(f"{self.words[0]}: the library pads {self.sizes} to {want}, this module to "
                                    f"{self.pads(*self.sizes)}")


_plans = {}


def _plan(cls, sizes, device, check=None):
    """the cached plan of (class, sizes, device): `cuda` without an index is the current device, the sizes are plain ints;
    built - after `check(sizes)` - when the key is first seen, and kept only if the constructor returns"""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (cls, *(int(n) for n in sizes), device)
    plan = _plans.get(key)
    if plan is None:
        if check is not None:
            check(key[1:-1])
        plan = _plans[key] = cls(*key[1:])
    return plan


def _out_buf(t: Optional[Tensor], what: str, name: str, shape, device, exc=_lib.DpotHipError,
             x: Optional[Tensor] = None) -> Tensor:
    """`t`, checked to be a kernel-ready tensor of `shape` on `device` that does not start where `x` does; a fresh one when it is
    None.  `exc`: the caller's exception type"""
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if tuple(_req(t, f"{what}: {name}").shape) != tuple(shape) or t.device != device:
        raise exc(f"{what}: {name} must be {tuple(shape)} on {device}, got {tuple(t.shape)} on {t.device}")
    if x is not None and t.data_ptr() == x.data_ptr():
        raise exc(f"{what}: {name} must not alias x")
    return t


def size_tuple(size, rank: int, strict: bool = False):
    """`size` as `rank` ints: one int for every axis, or a sequence whose first `rank` entries are taken.  strict: None for a
    sequence of another length (the caller words the refusal)"""
    if isinstance(size, int):
        return (int(size),) * rank
    if strict and len(size) != rank:
        return None
    return tuple(int(size[k]) for k in range(rank))


def padded(a, shape):
    """`a` rounded to fp32 in the low corner of a zero array of `shape`"""
    import numpy as np
    out = np.zeros(shape, dtype=np.float32)
    out[tuple(slice(0, s) for s in a.shape)] = a.astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------------
# Fourier ("spectral") resize: utils/utilities.py:277-305 as dense products (csrc/resize.hip)
# ------------------------------------------------------------------------------------------------------
def _resize_freqs(n: int, m: int, axis: int):
    """(frequencies k, weights c_k) the resize keeps along one axis of length n -> m.  axis 0 is the full-spectrum axis
    (the reference's top and bottom row blocks), axis 1 the half-spectrum axis of rfft2 / irfft2"""
    import numpy as np
    if axis == 0:
        t1, b1 = min((n + 1) // 2, (m + 1) // 2), min(n // 2, m // 2)
        k = np.concatenate([np.arange(t1), np.arange(-b1, 0)])
        return k, np.ones(len(k))
    k = np.arange(min(n // 2 + 1, m // 2 + 1))
    # a complex-to-real inverse of length m counts every column twice but the DC one and (m even) the Nyquist one
    return k, np.where((k == 0) | (2 * k == m), 1.0, 2.0)


def spectral_resize_matrices(n: int, m: int, axis: int):
    """float64 (Re D, Im D), each [m, n], of one axis of the Fourier resize n -> m:
    D[j', j] = sum_k c_k exp(2 pi i k (j'/m - j/n)).  A plane resizes as
    out = (Re Dx (x) Re Dy - Im Dx (x) Im Dy) in / (n_x n_y), i.e. Re Dx @ in @ Re Dy.T - Im Dx @ in @ Im Dy.T, scaled.
    Pure host mathematics (numpy): the CPU tests check it without a GPU."""
    import numpy as np
    if n < 2 or m < 2 or axis not in (0, 1):
        raise ValueError(f"spectral_resize_matrices: sizes must be >= 2 and axis 0 or 1 (got {n} -> {m}, axis {axis})")
    k, c = _resize_freqs(n, m, axis)
    # the phase as an exact integer over the common denominator n m, reduced before the float64 division
    num = np.arange(m)[:, None, None] * n - np.arange(n)[None, :, None] * m            # [m, n, 1]
    ang = 2.0 * np.pi * ((k[None, None, :] * num) % (n * m)) / float(n * m)
    return (np.cos(ang) * c).sum(-1), (np.sin(ang) * c).sum(-1)


def spectral_resize_im_factors(n: int, m: int):
    """(u [m], v [n]) with Im Dx = u v^T for the full-spectrum axis, or None where Im Dx vanishes (min(n, m) odd, or
    m == n).  The one unpaired frequency -h, h = min(n, m) / 2, is real on the side whose length is 2h."""
    import numpy as np
    h2 = min(n, m)
    if h2 % 2 or n == m:
        return None
    h = h2 // 2
    if n == h2:          # exp(2 pi i h x / n) = (-1)^x
        u = -np.sin(2.0 * np.pi * ((h * np.arange(m)) % m) / m)
        v = 1.0 - 2.0 * (np.arange(n) % 2)
    else:                # exp(-2 pi i h x' / m) = (-1)^x'
        u = 1.0 - 2.0 * (np.arange(m) % 2)
        v = np.sin(2.0 * np.pi * ((h * np.arange(n)) % n) / n)
    return u, v


class ResizePlan(_TablePlan):
    """The operator matrices of dpot_spectral_resize for one size pair, built in float64, rounded to fp32, zero-padded to
    the kernel's tile multiples (include/dpot_hip.h) and kept in device memory.  `host_matrices` is the host part alone."""
    words = ("ResizePlan", "resize_plan", "matrices", "size pair", "(or the resize itself) once")

    @staticmethod
    def pads(nx: int, ny: int, mx: int, my: int):
        """(nxp, nyp, mxp, myp): contraction and y' extents in multiples of 16, output rows in multiples of 32 - the values
        dpot_spectral_resize_pad returns (checked when a plan is built)"""
        r = lambda n, q: (n + q - 1) // q * q
        return r(nx, 16), r(ny, 16), r(mx, 32), r(my, 16)

    @staticmethod
    def host_matrices(nx: int, ny: int, mx: int, my: int):
        """dict of fp32 numpy arrays: axT [nxp, mxp], ayT [nyp, myp] and, for the two-term size pairs, byT [nyp, myp],
        u [mxp], v [nxp] (else None)"""
        nxp, nyp, mxp, myp = ResizePlan.pads(nx, ny, mx, my)
        re_x, _ = spectral_resize_matrices(nx, mx, 0)
        re_y, im_y = spectral_resize_matrices(ny, my, 1)
        scale = 1.0 / (nx * ny)
        h = {"axT": padded(re_x.T, (nxp, mxp)), "ayT": padded(re_y.T * scale, (nyp, myp)), "byT": None, "u": None,
             "v": None}
        uv = spectral_resize_im_factors(nx, mx)
        if uv is not None:
            h["byT"] = padded(-im_y.T * scale, (nyp, myp))
            h["u"], h["v"] = padded(uv[0], (mxp,)), padded(uv[1], (nxp,))
        return h

    def __init__(self, nx: int, ny: int, mx: int, my: int, device):
        super().__init__((nx, ny, mx, my), device)
        self.two_terms = self.dev["byT"] is not None

    def _check(self) -> None:
        self._check_pads(_lib.load().dpot_spectral_resize_pad, (0, 0, 1, 0))

    _host = host_matrices


def resize_plan(nx: int, ny: int, mx: int, my: int, device) -> ResizePlan:
    """the cached ResizePlan of (n_x, n_y, m_x, m_y, device)"""
    return _plan(ResizePlan, (nx, ny, mx, my), device)


def spectral_resize(x: Tensor, out_size, out: Optional[Tensor] = None) -> Tensor:
    """Fourier resize of x [B, n_x, n_y, T, C] (or [B, n_x, n_y, TC]) to out_size = (m_x, m_y) or one int for both: the
    reference's resize(x, out_size, temporal=True) (utils/utilities.py:277-305), one kernel launch"""
    _req(x, "spectral_resize: x")
    if x.dim() not in (4, 5):
        raise _lib.DpotHipError(f"spectral_resize: x must be [B, X, Y, T, C] or [B, X, Y, TC], got {tuple(x.shape)}")
    mx, my = size_tuple(out_size, 2)
    B, nx, ny = x.shape[:3]
    TC = x.numel() // max(B * nx * ny, 1)
    if min(B, nx, ny, mx, my, TC) < 1 or min(nx, ny, mx, my) < 2:
        raise _lib.DpotHipError(f"spectral_resize: cannot resize {tuple(x.shape)} to {(mx, my)}: every spatial size must be "
                                ">= 2 and no dimension empty")
    out = _out_buf(out, "spectral_resize", "out", (B, mx, my) + tuple(x.shape[3:]), x.device, x=x)
    d = resize_plan(nx, ny, mx, my, x.device).dev
    check(_lib.load().dpot_spectral_resize(x.data_ptr(), out.data_ptr(), d["axT"].data_ptr(), d["ayT"].data_ptr(),
                                           _p(d["byT"]), _p(d["u"]), _p(d["v"]), B, nx, ny, mx, my, TC, _stream()),
          "spectral_resize")
    return out


# ---- three axes (csrc/resize3.hip): X and Y are full-spectrum axes ("axis 0" matrices), Z is the half-spectrum axis ("axis 1")
def spectral_resize3_terms(nx: int, ny: int, nz: int, mx: int, my: int, mz: int):
    """The float64 terms of the 3-D Fourier resize (n_x, n_y, n_z) -> (m_x, m_y, m_z): a list of (sign, Ax [m_x, n_x],
    Ay [m_y, n_y], Az [m_z, n_z]) with operator = sum sign * Ax (x) Ay (x) Az / (n_x n_y n_z).  The operator is
    Re(Dx (x) Dy (x) Dz): the products with an even number of imaginary factors, Rx Ry Rz - Rx Iy Iz - Ix Ry Iz - Ix Iy Rz,
    and a term is listed only where it survives: Ix (Iy) is u v^T of spectral_resize_im_factors or zero (min(n, m) odd, or
    n == m), Iz is general.  Neither vanishing: all four; Ix = 0: the first two; Iy = 0: the first and the third; both: one."""
    import numpy as np
    rx, _ = spectral_resize_matrices(nx, mx, 0)
    ry, _ = spectral_resize_matrices(ny, my, 0)
    rz, iz = spectral_resize_matrices(nz, mz, 1)
    fx, fy = spectral_resize_im_factors(nx, mx), spectral_resize_im_factors(ny, my)
    ix = None if fx is None else np.outer(*fx)
    iy = None if fy is None else np.outer(*fy)
    terms = [(1.0, rx, ry, rz)]
    if iy is not None:
        terms.append((-1.0, rx, iy, iz))
    if ix is not None:
        terms.append((-1.0, ix, ry, iz))
    if ix is not None and iy is not None:
        terms.append((-1.0, ix, iy, rz))
    return terms


class Resize3Plan(_TablePlan):
    """The operator matrices of dpot_spectral_resize3 for one size tuple, built in float64, rounded once to fp32, zero-padded
    to the kernels' tile multiples (include/dpot_hip.h) and kept in device memory.  `host_matrices` is the host part alone."""
    words = ("Resize3Plan", "resize3_plan", "matrices", "size tuple", "(or the resize itself) once")

    @staticmethod
    def pads(nx: int, ny: int, nz: int, mx: int, my: int, mz: int):
        """(nxp, nyp, nzp, mxp, myp, mzp): contraction extents and z' in multiples of 16, the output rows x' (axis launch) and
        y' (plane launch) in multiples of 32 - the values dpot_spectral_resize3_pad returns (checked when a plan is built)"""
        r = lambda n, q: (n + q - 1) // q * q
        return r(nx, 16), r(ny, 16), r(nz, 16), r(mx, 32), r(my, 32), r(mz, 16)

    @staticmethod
    def host_matrices(nx: int, ny: int, nz: int, mx: int, my: int, mz: int):
        """dict of fp32 numpy arrays: rxT [nxp, mxp], ryT [nyp, myp], rzT and izT [nzp, mzp] (both / (nx ny nz); izT None where
        neither X nor Y has an imaginary term), nux [mxp] = -ux and vx [nxp] (None where Im Dx = 0), uy2 [2, myp] = (+uy, -uy)
        and vy [nyp] (None where Im Dy = 0)"""
        import numpy as np
        nxp, nyp, nzp, mxp, myp, mzp = Resize3Plan.pads(nx, ny, nz, mx, my, mz)
        rx, _ = spectral_resize_matrices(nx, mx, 0)
        ry, _ = spectral_resize_matrices(ny, my, 0)
        rz, iz = spectral_resize_matrices(nz, mz, 1)
        scale = 1.0 / (nx * ny * nz)
        h = {"rxT": padded(rx.T, (nxp, mxp)), "ryT": padded(ry.T, (nyp, myp)), "rzT": padded(rz.T * scale, (nzp, mzp)),
             "izT": None, "nux": None, "vx": None, "uy2": None, "vy": None}
        fx, fy = spectral_resize_im_factors(nx, mx), spectral_resize_im_factors(ny, my)
        if fx is not None or fy is not None:
            h["izT"] = padded(iz.T * scale, (nzp, mzp))
        if fx is not None:
            h["nux"], h["vx"] = padded(-fx[0], (mxp,)), padded(fx[1], (nxp,))
        if fy is not None:
            h["uy2"], h["vy"] = padded(np.stack([fy[0], -fy[0]]), (2, myp)), padded(fy[1], (nyp,))
        return h

    def __init__(self, nx: int, ny: int, nz: int, mx: int, my: int, mz: int, device):
        super().__init__((nx, ny, nz, mx, my, mz), device)
        self.terms = 1 + (self.dev["nux"] is not None) + (self.dev["uy2"] is not None) \
            + (self.dev["nux"] is not None and self.dev["uy2"] is not None)

    def _check(self) -> None:
        self._check_pads(_lib.load().dpot_spectral_resize3_pad, (0, 0, 0, 1, 1, 0))

    _host = host_matrices


def _check_resize3_sizes(sizes):
    if min(sizes) < 2:
        raise _lib.DpotHipError(f"spectral_resize3: every spatial size must be >= 2, got {sizes[:3]} -> {sizes[3:]}")
    cap = _lib.load().dpot_spectral_resize3_max_size()
    if max(sizes) > cap:
        raise _lib.DpotHipError(f"spectral_resize3: {sizes[:3]} -> {sizes[3:]}: the size {max(sizes)} is beyond the LDS "
                                f"intermediate of a workgroup (every size <= {cap})")


def resize3_plan(nx: int, ny: int, nz: int, mx: int, my: int, mz: int, device) -> Resize3Plan:
    """the cached Resize3Plan of (n_x, n_y, n_z, m_x, m_y, m_z, device)"""
    return _plan(Resize3Plan, (nx, ny, nz, mx, my, mz), device, check=_check_resize3_sizes)


def spectral_resize3(x: Tensor, out_size, out: Optional[Tensor] = None) -> Tensor:
    """Fourier resize of x [B, n_x, n_y, n_z, T, C] (or [B, n_x, n_y, n_z, TC]) to out_size = (m_x, m_y, m_z) or one int for
    all three: the three-axis form of the reference's resize (utils/utilities.py:277-305) - rfftn over X, Y, Z, the four
    corner blocks of the full-spectrum axes X, Y and the low columns of the half-spectrum axis Z, irfftn, rescale.  Two to
    five launches around a workspace this call allocates (dpot_spectral_resize3_ws_elems)."""
    _req(x, "spectral_resize3: x")
    if x.dim() not in (5, 6):
        raise _lib.DpotHipError(f"spectral_resize3: x must be [B, X, Y, Z, T, C] or [B, X, Y, Z, TC], got {tuple(x.shape)}")
    m = size_tuple(out_size, 3, strict=True)
    if m is None:
        raise _lib.DpotHipError(f"spectral_resize3: out_size must be one int or (m_x, m_y, m_z), got {tuple(out_size)}")
    mx, my, mz = m
    B, nx, ny, nz = x.shape[:4]
    TC = x.numel() // max(B * nx * ny * nz, 1)
    if min(B, TC) < 1:
        raise _lib.DpotHipError(f"spectral_resize3: cannot resize {tuple(x.shape)}: no dimension may be empty")
    _check_resize3_sizes((nx, ny, nz, mx, my, mz))
    out = _out_buf(out, "spectral_resize3", "out", (B, mx, my, mz) + tuple(x.shape[4:]), x.device, x=x)
    lib = _lib.load()
    d = resize3_plan(nx, ny, nz, mx, my, mz, x.device).dev
    n_ws = lib.dpot_spectral_resize3_ws_elems(B, nx, ny, nz, mx, my, mz, TC)
    if n_ws <= 0:
        raise _lib.DpotHipError(f"spectral_resize3: no workspace size: {(lib.dpot_last_error() or b'?').decode()}")
    ws = torch.empty(n_ws, dtype=torch.float32, device=x.device)
    check(lib.dpot_spectral_resize3(x.data_ptr(), out.data_ptr(), ws.data_ptr(), d["rxT"].data_ptr(), d["ryT"].data_ptr(),
                                    d["rzT"].data_ptr(), _p(d["izT"]), _p(d["nux"]), _p(d["vx"]), _p(d["uy2"]), _p(d["vy"]),
                                    B, nx, ny, nz, mx, my, mz, TC, _stream()), "spectral_resize3")
    return out


# ------------------------------------------------------------------------------------------------------
# Rollout evaluation metrics: the reference's Evaluator (utils/criterion.py:189-239, compute_fourier_error :246-360) on the
# device, for 2-D rollouts [B, X, Y, T, C] (csrc/evalmetrics.hip) and 3-D ones [B, X, Y, Z, T, C] (csrc/evalmetrics3d.hip) through
# one host path.  The host tables are pure numpy: the CPU tests check them without a GPU.
# ------------------------------------------------------------------------------------------------------
EVAL_KEYS = ("nmae", "nmse", "nmxe", "nmae_t", "nmse_t", "nmxe_t", "bdmse", "fmse_low", "fmse_mid", "fmse_high")


def _eval_work_plane(lib, B, nx, ny, TC):
    """one record of 8 doubles and K shell partials per (b, plane, stripe of 16 wavenumbers i)"""
    n = B * TC * (lib.dpot_eval_metrics_pad(nx, 1) // 16)
    return n * 8, n * min(nx // 2, ny // 2)


def _eval_work_field(lib, B, nx, ny, nz, TC):
    """the library's own figures: statistics partials, shell partials and the half spectrum G between the z and the xy pass"""
    return tuple(lib.dpot_eval3_work_elems(which, B, nx, ny, nz, TC) for which in range(3))


class _EvalRank(NamedTuple):
    """What differs between planes [B, X, Y, T, C] (csrc/evalmetrics.hip) and fields [B, X, Y, Z, T, C]
    (csrc/evalmetrics3d.hip: column c of every key is the reference's Evaluator(temporal=True, griddata=True, component=c));
    everything below this record serves both and takes the rank from the number of spatial sizes."""
    noun: str            # what one (b, t, c) slice is called in messages
    axes: tuple          # table name suffix per axis (cos "c" + suffix, sin "s" + suffix): the stats entry point takes them in
                         # this order, then jlo, then the workspace
    limits: str          # the size limits of max_size(axis), as the message words them
    pad: str             # C entry points
    max_size: str
    acc_elems: str
    stats: str
    finalize: str
    work: object         # (lib, B, *sizes, TC) -> elements of statp (doubles) and of each fp32 buffer behind it


_EVAL_RANKS = {
    2: _EvalRank("plane", ("xT", "y"), "nx <= {}, ny <= {}: the LDS intermediate of a workgroup", "dpot_eval_metrics_pad",
                 "dpot_eval_metrics_max_size", "dpot_eval_metrics_acc_elems", "dpot_eval_metrics_stats",
                 "dpot_eval_metrics_finalize", _eval_work_plane),
    3: _EvalRank("field", ("xT", "y", "zT"), "nx <= {}; ny <= {}: the LDS intermediate of a workgroup; nz <= {}",
                 "dpot_eval3_pad", "dpot_eval3_max_size", "dpot_eval3_acc_elems", "dpot_eval3_stats", "dpot_eval3_finalize",
                 _eval_work_field),
}


def _eval_rank(what: str, sizes) -> _EvalRank:
    rank = _EVAL_RANKS.get(len(sizes))
    if rank is None:
        raise ValueError(f"{what}: need the 2 or 3 spatial sizes of a plane or a field, got {tuple(sizes)}")
    return rank


def eval_dft_tables(n: int):
    """float64 (cos, sin) [n // 2, n] of the forward DFT's positive half: row i, column x holds cos / sin(2 pi i x / n), so
    that sum_x e[x] exp(-2 pi 1j i x / n) = cos @ e - 1j * sin @ e.  The phase i x is reduced modulo n as an exact integer
    before the float64 division."""
    import numpy as np
    if n < 2:
        raise ValueError(f"eval_dft_tables: the size must be >= 2, got {n}")
    ang = 2.0 * np.pi * ((np.arange(n // 2)[:, None] * np.arange(n)[None, :]) % n) / float(n)
    return np.cos(ang), np.sin(ang)


def eval_shell_table(*sizes: int):
    """int32 [nx // 2, ny // 2] or [nx // 2, ny // 2, nz // 2]: the shell floor(sqrt(i^2 + j^2 (+ k^2))) of a wavenumber of the
    positive quadrant (octant), or -1 where that shell is >= K = min(n // 2 for n in sizes) and the reference drops the
    wavenumber.  Integer arithmetic: the float square root is only a first guess that two integer comparisons correct."""
    import numpy as np
    _eval_rank("eval_shell_table", sizes)
    if min(sizes) < 2:
        raise ValueError(f"eval_shell_table: sizes must be >= 2, got {' x '.join(map(str, sizes))}")
    v = sum(g.astype(np.int64) ** 2 for g in np.ogrid[tuple(slice(n // 2) for n in sizes)])
    s = np.sqrt(v.astype(np.float64)).astype(np.int64)
    s -= (s * s > v)
    s += ((s + 1) * (s + 1) <= v)
    assert ((s * s <= v) & ((s + 1) * (s + 1) > v)).all()
    return np.where(s < min(n // 2 for n in sizes), s, -1).astype(np.int32)


def eval_shell_ranges(*sizes: int):
    """int32 [nx // 2, K + 1] or [nz // 2, nx // 2, K + 1]: entry [(k,) i, s] = number of j in [0, ny // 2) whose shell in row
    (k,) i is below s.  The shell grows with j, so the members of shell s in a row are the j range [.., s] .. [.., s + 1]; what
    lies at or beyond [.., K] is dropped.  This is the form of eval_shell_table the kernels walk."""
    import numpy as np
    sh = eval_shell_table(*sizes).astype(np.int64)
    K = min(n // 2 for n in sizes)
    sh = np.where(sh < 0, K, sh)                                   # dropped: beyond every kept shell
    below = np.stack([(sh < s).sum(axis=1) for s in range(K + 1)], axis=-1)          # [i, (k,) s]
    return np.ascontiguousarray(np.moveaxis(below, 0, -2), dtype=np.int32)


def eval_acc_layout(*dims: int):
    """(offsets, total) of the accumulator of dims = (X, Y[, Z], T, C) in 8-byte words: 'count' (int64), then doubles - 'c'
    [3, C] = nmae | nmse | nmxe, 'tc' [4, T, C] = nmae_t | nmse_t | nmxe_t | boundary, 'spec' [T, C, K] - every entry a sum
    over the samples"""
    *sizes, T, C = dims
    _eval_rank("eval_acc_layout", sizes)
    off = {"count": 0, "c": 2, "tc": 2 + 3 * C, "spec": 2 + 3 * C + 4 * T * C}
    return off, off["spec"] + T * C * min(n // 2 for n in sizes)


def eval_finish(acc, samples: int, *dims: int, ilow: int = 4, ihigh: int = 12):
    """the dict of RolloutEvaluator.read() from the accumulated sums (`acc`: float64 array of eval_acc_layout's words, the
    count word ignored; `samples`: the count; dims = (X, Y[, Z], T, C), or (X, Y[, Z], T, C, ilow, ihigh) with both band
    limits behind them - 4 or 5 numbers without, 6 or 7 with, so the count tells): the means over the samples, the root of the mean
    shell sums over the product of the spatial sizes, and the three band means (an empty band is NaN, as torch.mean of an
    empty slice in the reference).  float32 arrays with the reference's shapes: nmae.. [1, C], nmae_t.. [1, T, C], fmse_*
    [T, C], bdmse [C, T] (the reference returns the boundary error - of a field: on the six faces - untransposed)."""
    import numpy as np
    import warnings
    if len(dims) in (6, 7):
        *dims, ilow, ihigh = dims
    *sizes, T, C = dims
    acc = np.asarray(acc, dtype=np.float64)
    off, total = eval_acc_layout(*dims)
    if acc.shape != (total,):
        raise ValueError(f"eval_finish: the accumulator of {'x'.join(map(str, sizes))}, T={T}, C={C} has {total} words, got "
                         f"{acc.shape}")
    n = float(samples) if samples else float("nan")
    c = acc[off["c"]:off["tc"]].reshape(3, C) / n
    tc = acc[off["tc"]:off["spec"]].reshape(4, T, C) / n
    shells = np.sqrt(acc[off["spec"]:].reshape(T, C, -1) / n) / float(np.prod(sizes, dtype=np.int64))
    out = {"nmae": c[0:1], "nmse": c[1:2], "nmxe": c[2:3], "nmae_t": tc[0:1], "nmse_t": tc[1:2], "nmxe_t": tc[2:3],
           "bdmse": tc[3].T}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)            # the mean of an empty band IS NaN
        for key, band in (("fmse_low", shells[..., :ilow]), ("fmse_mid", shells[..., ilow:ihigh]),
                          ("fmse_high", shells[..., ihigh:])):
            out[key] = band.mean(axis=-1) if band.shape[-1] else np.full((T, C), np.nan)
    out = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}
    out["samples"] = int(samples)
    return out


class EvalPlan(_TablePlan):
    """The tables of dpot_eval_metrics_stats / dpot_eval3_stats for one plane or field size, built in float64, rounded to
    fp32, zero-padded to the kernels' tile multiples and kept in device memory.  `host_tables` is the host part alone."""

    @staticmethod
    def pads(*sizes: int):
        """(nxp, nyp[, nzp], hxp, hyp[, hzp]): the contraction extents and the wavenumber extents n // 2, each rounded up to
        16 - the values the library's pad entry point returns (checked when a plan is built)"""
        r = lambda n: (n + 15) // 16 * 16
        return tuple(r(n) for n in sizes) + tuple(r(n // 2) for n in sizes)

    @staticmethod
    def host_tables(*sizes: int):
        """dict of numpy arrays: cxT, sxT fp32 [nxp, hxp], cy, sy fp32 [nyp, hyp], for a field czT, szT fp32 [nzp, hzp], and
        jlo int32 = eval_shell_ranges"""
        import numpy as np
        rank, pads, out = _eval_rank("EvalPlan", sizes), EvalPlan.pads(*sizes), {}
        for a, (axis, n) in enumerate(zip(rank.axes, sizes)):
            for name, tab in zip("cs", eval_dft_tables(n)):
                t = out[name + axis] = np.zeros((pads[a], pads[len(sizes) + a]), dtype=np.float32)
                t[:n, :n // 2] = tab.T.astype(np.float32)
        out["jlo"] = eval_shell_ranges(*sizes)
        return out

    def __init__(self, *sizes_device):
        super().__init__(sizes_device[:-1], sizes_device[-1])
        self.work = {}

    @property
    def words(self):
        return "EvalPlan", "eval_plan", "tables", f"{self.rank.noun} size", "(or one update)"

    def _check(self) -> None:
        lib, sizes = _lib.load(), self.sizes
        self.rank = _eval_rank("EvalPlan", sizes)
        limits = [getattr(lib, self.rank.max_size)(a) for a in range(len(sizes))]
        if any(n > m for n, m in zip(sizes, limits)):
            raise _lib.DpotHipError(f"eval_metrics: a {' x '.join(map(str, sizes))} {self.rank.noun} is beyond the supported "
                                    f"size ({self.rank.limits.format(*limits)})")
        self._check_pads(getattr(lib, self.rank.pad), (0,) * len(sizes) + (1,) * len(sizes), sizes * 2)

    _host = host_tables

    def workspace(self, B: int, TC: int, device):
        """the buffers of a batch size between the two launches - statp (doubles), then the fp32 ones, in the order the
        stats entry point takes them: allocated when the size is first seen (not under capture), then reused"""
        w = self.work.get((B, TC))
        if w is None:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.DpotHipError(f"EvalPlan {self.sizes}: the workspace of B={B}, T*C={TC} is allocated when that shape "
                                        "is first used - run one update before capturing")
            n = self.rank.work(_lib.load(), B, *self.sizes, TC)
            if min(n) < 1:
                raise _lib.DpotHipError(f"EvalPlan {self.sizes}: the library sizes no workspace for B={B}, T*C={TC}")
            w = self.work[(B, TC)] = tuple(torch.empty(m, dtype=torch.float32 if i else torch.float64, device=device)
                                           for i, m in enumerate(n))
        return w


def eval_plan(*sizes_device) -> EvalPlan:
    """the cached EvalPlan of (n_x, n_y[, n_z], device)"""
    return _plan(EvalPlan, sizes_device[:-1], sizes_device[-1])


def eval_acc_alloc(*dims_device) -> Tensor:
    """a zeroed accumulator of (X, Y[, Z], T, C, device) for eval_metrics_update (int64 words; word 0 the sample count, the
    rest doubles)"""
    *dims, device = dims_device
    n = eval_acc_layout(*dims)[1]
    if n != getattr(_lib.load(), _eval_rank("eval_acc_alloc", dims[:-2]).acc_elems)(*dims):
        raise _lib.DpotHipError(f"eval_acc_alloc: the library lays the accumulator of {'x'.join(map(str, dims[:-2]))}, "
                                f"T={dims[-2]}, C={dims[-1]} out differently")
    return torch.zeros(n, dtype=torch.int64, device=device)


def eval_metrics_update(pred: Tensor, target: Tensor, acc: Tensor) -> None:
    """acc += the Evaluator sums of this batch: pred, target [B, X, Y, T, C] or [B, X, Y, Z, T, C] fp32 contiguous on the
    GPU, acc from eval_acc_alloc for the same (X, Y[, Z], T, C).  Two launches (a field: three) on the current stream, no
    synchronisation; capturable once the spatial size and the batch size have been seen (their tables and workspace are
    cached)."""
    _req(pred, "eval_metrics: pred")
    _req(target, "eval_metrics: target")
    rank = _EVAL_RANKS.get(pred.dim() - 3)
    if rank is None or pred.shape != target.shape or pred.device != target.device:
        raise _lib.DpotHipError(f"eval_metrics: pred and target must be [B, X, Y, T, C] or [B, X, Y, Z, T, C] of one shape on "
                                f"one device, got {tuple(pred.shape)} on {pred.device} and {tuple(target.shape)} on "
                                f"{target.device}")
    B, *dims = pred.shape
    *sizes, T, C = dims
    if min(B, T, C) < 1 or min(sizes) < 2:
        raise _lib.DpotHipError(f"eval_metrics: cannot evaluate {tuple(pred.shape)}: every spatial size must be >= 2 and no "
                                "dimension empty")
    words = eval_acc_layout(*dims)[1]
    if (not acc.is_cuda or acc.device != pred.device or acc.dtype != torch.int64 or not acc.is_contiguous()
            or acc.numel() != words):
        raise _lib.DpotHipError(f"eval_metrics: acc must be the {words} int64 words of eval_acc_alloc"
                                f"({', '.join(map(str, dims))}) on {pred.device}")
    plan = eval_plan(*sizes, pred.device)
    work = [w.data_ptr() for w in plan.workspace(B, T * C, pred.device)]
    lib = _lib.load()
    check(getattr(lib, rank.stats)(pred.data_ptr(), target.data_ptr(), *(t.data_ptr() for t in plan.dev.values()), *work, B,
                                   *sizes, T * C, _stream()), rank.stats[5:])
    check(getattr(lib, rank.finalize)(work[0], work[1], acc.data_ptr(), B, *sizes, T, C, _stream()), rank.finalize[5:])


# ------------------------------------------------------------------------------------------------------
# Anti-aliased activation of the CDPOT model (csrc/aa_act.hip): bilinear up by 2, LeakyReLU, anti-aliased bilinear down by 2,
# optionally bilinear up to an output size, + a per-channel bias (models/filter_networks.py:481-518).  The resize matrices
# and tap tables are pure numpy: the CPU tests check them without a GPU.
# ------------------------------------------------------------------------------------------------------
def aa_resize_matrix(n: int, m: int):
    """float64 [m, n]: one axis of F.interpolate(mode='bilinear', antialias=True) from n to m samples.  Output i sits at
    c = (n/m)(i + 0.5) and weighs the inputs j in [int(c - s + 0.5), int(c + s + 0.5)), clipped to the axis, by the triangle
    max(0, 1 - |(j - c + 0.5) / s|) of half-width s = max(n/m, 1), normalised to sum 1."""
    import numpy as np
    n, m = int(n), int(m)
    if n < 1 or m < 1:
        raise ValueError(f"aa_resize_matrix: sizes must be >= 1 (got {n} -> {m})")
    scale = n / m
    support = max(scale, 1.0)
    inv = 1.0 / support
    A = np.zeros((m, n), dtype=np.float64)
    for i in range(m):
        c = scale * (i + 0.5)
        lo, hi = max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n)
        j = np.arange(lo, hi, dtype=np.float64)
        wt = np.maximum(0.0, 1.0 - np.abs((j - c + 0.5) * inv))
        A[i, lo:hi] = wt / wt.sum()
    return A


def _aa_taps(A, K: int, what: str):
    """rows of a dense matrix as K taps each: (index int32 [rows, K], weight fp32 [rows, K]); unused taps carry weight 0 and
    repeat the row's last index (always inside the axis)"""
    import numpy as np
    rows = A.shape[0]
    idx = np.zeros((rows, K), dtype=np.int32)
    wt = np.zeros((rows, K), dtype=np.float32)
    for r in range(rows):
        nz = np.nonzero(A[r])[0]
        if len(nz) > K:
            raise ValueError(f"aa tables: {what} row {r} has {len(nz)} taps, the kernels take {K}")
        idx[r, :len(nz)] = nz
        idx[r, len(nz):] = nz[-1] if len(nz) else 0
        wt[r, :len(nz)] = A[r, nz]
    return idx, wt


def _aa_csr(A):
    """rows of a dense matrix [rows, cols] in CSR form padded to 2 * cols entries: (ptr int32 [rows + 1], index int32, weight fp32)"""
    import numpy as np
    rows, cols = A.shape
    ptr = np.zeros(rows + 1, dtype=np.int32)
    idx = np.zeros(2 * cols, dtype=np.int32)
    wt = np.zeros(2 * cols, dtype=np.float32)
    k = 0
    for r in range(rows):
        nz = np.nonzero(A[r])[0]
        if k + len(nz) > 2 * cols:
            raise ValueError("aa tables: a bilinear up-sampling row has more than 2 taps")
        idx[k:k + len(nz)] = nz
        wt[k:k + len(nz)] = A[r, nz]
        k += len(nz)
        ptr[r + 1] = k
    return ptr, idx, wt


def aa_core_tables(h: int, w: int):
    """int32 words [32 (h + w)] of dpot_aa_lrelu_fwd / _bwd (include/dpot_hip.h): per axis the taps of U (n -> 2n), D (2n -> n),
    U^T and D^T, weights as fp32 bit patterns"""
    import numpy as np
    parts = []
    for n in (int(h), int(w)):
        U, D = aa_resize_matrix(n, 2 * n), aa_resize_matrix(2 * n, n)
        for A, K, what in ((U, 2, "U"), (D, 4, "D"), (U.T, 4, "U^T"), (D.T, 2, "D^T")):
            idx, wt = _aa_taps(A, K, f"{what} ({n})")
            parts += [idx.reshape(-1), wt.reshape(-1).view(np.int32)]
    return np.concatenate(parts)


def aa_up_tables(h: int, w: int, H: int, W: int):
    """int32 words of dpot_aa_up_fwd / _adj: the taps of V (rows h -> H, columns w -> W), then V^T of both in CSR form"""
    import numpy as np
    Vh, Vw = aa_resize_matrix(h, H), aa_resize_matrix(w, W)
    parts = []
    for V in (Vh, Vw):
        idx, wt = _aa_taps(V, 2, "V")
        parts += [idx.reshape(-1), wt.reshape(-1).view(np.int32)]
    for V in (Vh, Vw):
        ptr, idx, wt = _aa_csr(V.T)
        parts += [ptr, idx, wt.view(np.int32)]
    return np.concatenate(parts)


class AAPlan(_TablePlan):
    """The tap tables of the anti-aliased activation for one size tuple (h, w, H, W) - H = W = 0: no output size - built in
    float64, rounded to fp32 and kept in device memory: .tab, and .vtab of the output size (else None)"""
    words = ("AAPlan", "aa_plan", "tap tables", "size tuple", "(or the operator itself) once")

    def __init__(self, h: int, w: int, H: int, W: int, device):
        super().__init__((h, w, H, W), device)
        self.tab, self.vtab = self.dev["tab"], self.dev["vtab"]

    def _check(self) -> None:
        lib, (h, w, H, W) = _lib.load(), self.sizes
        lat, outm = lib.dpot_aa_max_size(0), lib.dpot_aa_max_size(1)
        if not (1 <= h <= lat and 1 <= w <= lat):
            raise ValueError(f"aa_lrelu: latent size {h}x{w} is not supported (1 <= h, w <= {lat})")
        if (H or W) and not (h <= H <= outm and w <= W <= outm):
            raise ValueError(f"aa_lrelu: output size {H}x{W} is not supported for a {h}x{w} field (per axis: input size <= "
                             f"output size <= {outm})")

    @staticmethod
    def _host(h: int, w: int, H: int, W: int):
        """the word tables, each held to the length the library expects"""
        lib = _lib.load()
        core, up = aa_core_tables(h, w), None
        if len(core) != lib.dpot_aa_tab_words(h, w):
            raise _lib.DpotHipError(f"AAPlan: {len(core)} table words, the library expects {lib.dpot_aa_tab_words(h, w)}")
        if H or W:
            up = aa_up_tables(h, w, H, W)
            if len(up) != lib.dpot_aa_vtab_words(h, w, H, W):
                raise _lib.DpotHipError(f"AAPlan: {len(up)} up-sampling table words, the library expects "
                                        f"{lib.dpot_aa_vtab_words(h, w, H, W)}")
        return {"tab": core, "vtab": up}


def aa_plan(h: int, w: int, H: int, W: int, device) -> AAPlan:
    """the cached AAPlan of (h, w, H, W, device); H = W = 0 without an output size"""
    return _plan(AAPlan, (h, w, H, W), device)


def _aa_out_size(out_size, h: int, w: int):
    if out_size is None:
        return 0, 0
    H, W = size_tuple(out_size, 2)
    return (0, 0) if (H, W) == (h, w) else (H, W)      # V is the identity at the input size: skipped, as the reference does


def _aa_args(x: Tensor, bias: Tensor, what: str):
    _req(x, f"{what}: x")
    _req(bias, f"{what}: bias")
    if x.dim() != 4 or bias.dim() != 1 or x.numel() == 0 or bias.numel() == 0 or x.shape[3] % bias.shape[0] or \
            bias.device != x.device:
        raise ValueError(f"{what}: x must be a non-empty [N, h, w, C] and bias [Cb] with C % Cb == 0 on one device, got "
                         f"{tuple(x.shape)} and {tuple(bias.shape)}")
    return tuple(x.shape)


def aa_lrelu(x: Tensor, bias: Tensor, out_size=None, slope: float = 0.01, out: Optional[Tensor] = None) -> Tensor:
    """y [N, H, W, C] = V D lrelu(U x U^T) D^T V^T + bias[c % Cb] of a channels-last x [N, h, w, C]: bilinear up by 2,
    LeakyReLU(slope), anti-aliased bilinear down by 2, bilinear up to out_size = (H, W) / one int (None or the input size:
    skipped), + bias [Cb] (the reference's LReLu_torch).  One launch, two with an output size (the field at the latent size
    goes through a scratch tensor; the 2h x 2w field never exists)."""
    N, h, w, C = _aa_args(x, bias, "aa_lrelu")
    H, W = _aa_out_size(out_size, h, w)
    plan = aa_plan(h, w, H, W, x.device)
    out = _out_buf(out, "aa_lrelu", "out", (N, H or h, W or w, C), x.device, x=x)
    lib = _lib.load()
    Cb = bias.shape[0]
    if plan.vtab is None:
        check(lib.dpot_aa_lrelu_fwd(x.data_ptr(), bias.data_ptr(), out.data_ptr(), plan.tab.data_ptr(), N, h, w, C, Cb,
                                    float(slope), _stream()), "aa_lrelu_fwd")
        return out
    z = _scratch(torch.empty_like(x))
    check(lib.dpot_aa_lrelu_fwd(x.data_ptr(), None, z.data_ptr(), plan.tab.data_ptr(), N, h, w, C, Cb, float(slope),
                                _stream()), "aa_lrelu_fwd")
    check(lib.dpot_aa_up_fwd(z.data_ptr(), bias.data_ptr(), out.data_ptr(), plan.vtab.data_ptr(), N, h, w, H, W, C, Cb,
                             _stream()), "aa_up_fwd")
    return out


def aa_lrelu_bwd(x: Tensor, dy: Tensor, Cb: int, slope: float = 0.01, out_dbias: Optional[Tensor] = None):
    """(dx [N, h, w, C], dbias [Cb]) of aa_lrelu for dy [N, H, W, C] (H x W the output size of the forward, or h x w): the
    up-sampled field is recomputed from x inside the kernel; the kernel's per-sample bias partials are finished by colsum"""
    _req(x, "aa_lrelu_bwd: x")
    _req(dy, "aa_lrelu_bwd: dy")
    if x.dim() != 4 or dy.dim() != 4 or x.numel() == 0 or dy.shape[0] != x.shape[0] or dy.shape[3] != x.shape[3] or \
            Cb < 1 or x.shape[3] % Cb or dy.device != x.device:
        raise ValueError(f"aa_lrelu_bwd: x [N, h, w, C] and dy [N, H, W, C] with C % Cb == 0 on one device, got "
                         f"{tuple(x.shape)}, {tuple(dy.shape)} and Cb = {Cb}")
    N, h, w, C = x.shape
    H, W = _aa_out_size((dy.shape[1], dy.shape[2]), h, w)
    plan = aa_plan(h, w, H, W, x.device)
    lib = _lib.load()
    g = dy
    if plan.vtab is not None:
        g = _scratch(torch.empty_like(x))
        check(lib.dpot_aa_up_adj(dy.data_ptr(), g.data_ptr(), plan.vtab.data_ptr(), N, h, w, H, W, C, _stream()), "aa_up_adj")
    dx = torch.empty_like(x)
    part = _scratch(torch.empty(N, C, dtype=torch.float32, device=x.device))
    check(lib.dpot_aa_lrelu_bwd(x.data_ptr(), g.data_ptr(), dx.data_ptr(), part.data_ptr(), plan.tab.data_ptr(), N, h, w, C,
                                float(slope), _stream()), "aa_lrelu_bwd")
    return dx, colsum(part, N * (C // Cb), Cb, out=out_dbias)


# ------------------------------------------------------------------------------------------------------
# The FNO baselines (csrc/fno.hip, csrc/fno3.hip; models/fno.py SpectralConv2d_fast and SpectralConv3d): truncated transforms of
# a channels-last field x [B, H, W, C] or [B, X, Y, Z, C] to / from the kept spectrum S [B, 2 m1, m2, 2, C] or
# [B, 2 m1, 2 m2, m3, 2, C] (every axis but the last keeps k < m and k >= N - m, the last k < m; re | im planes, channels
# innermost) and the per-mode channel mixing: two weights [2, Cin, Cout, m1, m2] (planar) in 2-D, four corner weights
# [Cin, Cout, m1, m2, m3, 2] (real pairs) in 3-D.  ONE host path serves both ranks: `dims` and `modes` are tuples of 2 or 3,
# and `what`, the caller's name in every message, is the library entry point without its prefix.  A 3-D transform is two launches
# around a workspace this module allocates.  The twiddle tables are pure numpy: the CPU tests check them.
# ------------------------------------------------------------------------------------------------------
_FNO_AXES = {2: "HW", 3: "XYZ"}
_FNO_WORDS = {2: ("two kept row blocks", "columns"), 3: ("kept corner blocks", "planes")}     # as each rank's messages say it


def _fno_check_modes(dims, modes, what: str) -> None:
    """the two refusals, narrower than the reference: the kept blocks of a two-sided axis must not overlap (the reference lets
    later weights silently overwrite what they share with earlier ones) and the last axis' modes must fit the half spectrum (the
    reference raises inside its slice assignment)"""
    axes, (blocks, last) = _FNO_AXES[len(dims)], _FNO_WORDS[len(dims)]
    if min(*dims, *modes) < 1:
        raise ValueError(f"{what}: field {'x'.join(map(str, dims))} and modes {tuple(modes)} must be positive")
    for k, (n, m) in enumerate(zip(dims[:-1], modes[:-1])):
        if 2 * m > n:
            raise ValueError(f"{what}: modes{k + 1} = {m} needs 2 * modes{k + 1} <= {axes[k]} = {n}: the {blocks} would "
                             "overlap")
    n, m, k = dims[-1], modes[-1], len(dims)
    if m > n // 2 + 1:
        raise ValueError(f"{what}: modes{k} = {m} exceeds the {axes[-1]} // 2 + 1 = {n // 2 + 1} {last} of the half "
                         f"spectrum of {axes[-1]} = {n}")


def _fno_limits(rank: int):
    """(largest axis, largest mode count) the kernels of a rank cover (dpot_fno_max_size / dpot_fno3_max_size)"""
    lib = _lib.load()
    max_size = lib.dpot_fno_max_size if rank == 2 else lib.dpot_fno3_max_size
    return max_size(0), max_size(1)


def _fno_supported(dims, modes) -> bool:
    n, m = _fno_limits(len(dims))
    return (min(*dims, *modes) >= 1 and all(2 * mk <= nk for nk, mk in zip(dims[:-1], modes[:-1]))
            and modes[-1] <= dims[-1] // 2 + 1 and max(dims) <= n and max(modes) <= m)


def fno_check_modes(H: int, W: int, m1: int, m2: int, what: str = "fno") -> None:
    _fno_check_modes((H, W), (m1, m2), what)


def fno3_check_modes(X: int, Y: int, Z: int, m1: int, m2: int, m3: int, what: str = "fno3") -> None:
    _fno_check_modes((X, Y, Z), (m1, m2, m3), what)


def fno_supported(H: int, W: int, m1: int, m2: int) -> bool:
    """valid modes for the field, within the sizes the kernels cover (dpot_fno_max_size)"""
    return _fno_supported((H, W), (m1, m2))


def fno3_supported(X: int, Y: int, Z: int, m1: int, m2: int, m3: int) -> bool:
    """valid modes for the field, within the sizes the kernels cover (dpot_fno3_max_size)"""
    return _fno_supported((X, Y, Z), (m1, m2, m3))


def fno_kept_rows(H: int, m1: int):
    """the wavenumbers kx of the 2 m1 kept rows, in the spectrum's row order"""
    import numpy as np
    return np.concatenate([np.arange(m1), np.arange(H - m1, H)])


def fno_twiddles(H: int, W: int, m1: int, m2: int):
    """float64 (tx [H, 2 m1, 2], ty [W, m2, 2]): cos | sin of 2 pi kx x / H over the kept rows and of 2 pi ky y / W, the
    angle reduced in integers"""
    import numpy as np
    kx = fno_kept_rows(H, m1)
    ax = 2.0 * np.pi * ((np.arange(H)[:, None] * kx[None, :]) % H) / H
    ay = 2.0 * np.pi * ((np.arange(W)[:, None] * np.arange(m2)[None, :]) % W) / W
    return np.stack([np.cos(ax), np.sin(ax)], -1), np.stack([np.cos(ay), np.sin(ay)], -1)


def fno3_twiddles(X: int, Y: int, Z: int, m1: int, m2: int, m3: int):
    """float64 (tx [X, 2 m1, 2], ty [Y, 2 m2, 2], tz [Z, m3, 2]): cos | sin of 2 pi k n / N over the kept wavenumbers, the angle
    reduced in integers.  (tx, tz) and (ty, tz) are fno_twiddles tables: the plane kernels are FNO2d's"""
    tx, tz = fno_twiddles(X, Z, m1, m3)
    ty, _ = fno_twiddles(Y, Z, m2, m3)
    return tx, ty, tz


def fno_col_weights(W: int, m2: int):
    """w(ky) of irfft2 for a spectrum that is not Hermitian: 1 at ky = 0 and, for even W, at ky = W / 2, else 2"""
    import numpy as np
    w = np.full(m2, 2.0)
    w[0] = 1.0
    if W % 2 == 0 and W // 2 < m2:
        w[W // 2] = 1.0
    return w


class FNOPlan(_TablePlan):
    """The twiddle tables of the truncated transforms for one (H, W, m1, m2, device) or (X, Y, Z, m1, m2, m3, device): .tx, .ty
    (and .tz), one per axis and all of them in .tables, built in float64, rounded to fp32 and kept in device memory.  FNO3Plan
    is the same class: the number of sizes gives the rank."""

    def __init__(self, *sizes_device):
        super().__init__(sizes_device[:-1], sizes_device[-1])
        self.tables = list(self.dev.values())
        for axis, t in self.dev.items():
            setattr(self, axis, t)

    @property
    def words(self):
        name, entry = ("FNOPlan", "fno_plan") if len(self.sizes) == 4 else ("FNO3Plan", "fno3_plan")
        return name, entry, "tables", "size tuple", "(or the operator itself) once"

    def _check(self) -> None:
        rank = len(self.sizes) // 2
        dims, modes = self.sizes[:rank], self.sizes[rank:]
        _fno_check_modes(dims, modes, self.words[0])
        if not _fno_supported(dims, modes):
            n, m = _fno_limits(rank)
            raise ValueError(f"{self.words[0]}: field {'x'.join(map(str, dims))} with modes {modes} is beyond the kernels' "
                             f"limits ({', '.join(_FNO_AXES[rank])} <= {n}, modes <= {m})")

    @staticmethod
    def _host(*sizes):
        return dict(zip(("tx", "ty", "tz"), (fno_twiddles if len(sizes) == 4 else fno3_twiddles)(*sizes)))


FNO3Plan = FNOPlan


def fno_plan(H: int, W: int, m1: int, m2: int, device) -> FNOPlan:
    """the cached FNOPlan of (H, W, m1, m2, device)"""
    return _plan(FNOPlan, (H, W, m1, m2), device)


def fno3_plan(X: int, Y: int, Z: int, m1: int, m2: int, m3: int, device) -> FNOPlan:
    """the cached FNO3Plan of (X, Y, Z, m1, m2, m3, device)"""
    return _plan(FNOPlan, (X, Y, Z, m1, m2, m3), device)


def _fno_kept(modes):
    """the kept-mode axes of a spectrum: (2 m1, m2) or (2 m1, 2 m2, m3)"""
    return tuple(2 * m for m in modes[:-1]) + (modes[-1],)


def _fno_kept_text(rank: int) -> str:
    """the same axes as the messages spell them"""
    return ", ".join([f"2 m{k + 1}" for k in range(rank - 1)] + [f"m{rank}"])


def _fno_kept_modes(S: Tensor, rank: int):
    """the modes of a spectrum [B, kept axes, 2, C]; None unless it is one of this rank"""
    if S.dim() != rank + 3 or S.shape[-2] != 2 or any(n % 2 for n in S.shape[1:rank]) or S.numel() == 0:
        return None
    return tuple(n // 2 for n in S.shape[1:rank]) + (S.shape[rank],)


def _fno_transform(what: str, head, B: int, dims, Cc: int, modes, tail, device) -> None:
    """one transform entry point: dpot_<what>(*head, [ws,] tables, B, dims, C, modes, *tail, stream).  The 3-D workspace
    [B, X, 2 m2, m3, 2, C] between the two launches is a local here: it lives until both launches have been issued and is
    dropped when the operator returns"""
    lib = _lib.load()
    plan = _plan(FNOPlan, (*dims, *modes), device)
    entry = getattr(lib, "dpot_" + what)
    tables = [t.data_ptr() for t in plan.tables]
    sizes = (B, *dims, Cc, *modes, *tail, _stream())
    if len(dims) == 2:
        check(entry(*head, *tables, *sizes), what)
    else:
        ws = _scratch(torch.empty(lib.dpot_fno3_ws_elems(B, dims[0], Cc, modes[1], modes[2]), dtype=torch.float32, device=device))
        check(entry(*head, ws.data_ptr(), *tables, *sizes), what)


def _fno_rfft(what: str, x: Tensor, modes, adjoint: bool, out: Optional[Tensor]) -> Tensor:
    rank = len(modes)
    if x.dim() != rank + 2 or x.numel() == 0:
        raise ValueError(f"{what}: the field must be a non-empty [B, {', '.join(_FNO_AXES[rank])}, C], got {tuple(x.shape)}")
    B, *dims, Cc = x.shape
    _fno_check_modes(dims, modes, what)
    _req(x, f"{what}: x")
    out = _out_buf(out, what, "out", (B,) + _fno_kept(modes) + (2, Cc), x.device, ValueError)
    _fno_transform(what, (x.data_ptr(), out.data_ptr()), B, dims, Cc, modes,
                   (1 if adjoint else 0, 1.0 / math.prod(dims) if adjoint else 1.0), x.device)
    return out


def _fno_irfft(what: str, S: Tensor, dims, add, act: int, save_pre: bool, adjoint: bool, out):
    modes = _fno_kept_modes(S, len(dims))
    if modes is None:
        raise ValueError(f"{what}: the spectrum must be a non-empty [B, {_fno_kept_text(len(dims))}, 2, C], got {tuple(S.shape)}")
    B, Cc = S.shape[0], S.shape[-1]
    _fno_check_modes(dims, modes, what)
    _req(S, f"{what}: S")
    shape = (B, *dims, Cc)
    if add is not None:
        _out_buf(add, what, "add", shape, S.device, ValueError)
    out = _out_buf(out, what, "out", shape, S.device, ValueError)
    pre = torch.empty_like(out) if save_pre else None
    _fno_transform(what, (S.data_ptr(), _p(add), out.data_ptr(), _p(pre)), B, tuple(dims), Cc, modes,
                   (0 if adjoint else 1, 1.0 if adjoint else 1.0 / math.prod(dims), int(act)), S.device)
    return out, pre


def fno_rfft2(x: Tensor, m1: int, m2: int, adjoint: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """x [B, H, W, C] -> the kept spectrum S [B, 2 m1, m2, 2, C] of the unnormalised rfft2.  adjoint=True: the adjoint of
    fno_irfft2 instead (the same sums times w(ky) / (H W)): the gradient of the spectrum from the gradient of the field"""
    return _fno_rfft("fno_rfft2", x, (m1, m2), adjoint, out)


def fno3_rfft3(x: Tensor, m1: int, m2: int, m3: int, adjoint: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """x [B, X, Y, Z, C] -> the kept spectrum S [B, 2 m1, 2 m2, m3, 2, C] of the unnormalised rfftn.  adjoint=True: the adjoint
    of fno3_irfft3 instead (the same sums times w(kz) / (X Y Z)): the gradient of the spectrum from the gradient of the field"""
    return _fno_rfft("fno3_rfft3", x, (m1, m2, m3), adjoint, out)


def fno_irfft2(S: Tensor, H: int, W: int, add: Optional[Tensor] = None, act: int = 0, save_pre: bool = False,
               adjoint: bool = False, out: Optional[Tensor] = None):
    """the kept spectrum S [B, 2 m1, m2, 2, C] -> (y, pre): y [B, H, W, C] = act(irfft2(S, s=(H, W)) + add), pre the value
    before the activation (save_pre, else None).  adjoint=True: the adjoint of fno_rfft2 instead (column weights 1, no
    1 / (H W)): the gradient of the field from the gradient of its spectrum"""
    return _fno_irfft("fno_irfft2", S, (H, W), add, act, save_pre, adjoint, out)


def fno3_irfft3(S: Tensor, X: int, Y: int, Z: int, add: Optional[Tensor] = None, act: int = 0, save_pre: bool = False,
                adjoint: bool = False, out: Optional[Tensor] = None):
    """the kept spectrum S [B, 2 m1, 2 m2, m3, 2, C] -> (y, pre): y [B, X, Y, Z, C] = act(irfftn(S, s=(X, Y, Z)) + add), pre
    the value before the activation (save_pre, else None).  adjoint=True: the adjoint of fno3_rfft3 instead (weights 1, no
    1 / (X Y Z)): the gradient of the field from the gradient of its spectrum"""
    return _fno_irfft("fno3_irfft3", S, (X, Y, Z), add, act, save_pre, adjoint, out)


def _fno_weights(ws, what: str, planar: bool):
    """(Cin, Cout, modes) of a layer's spectral weights: planar [2, Cin, Cout, m1, m2] or real-pair [Cin, Cout, m1, m2, m3, 2]"""
    w0 = ws[0]
    ok = w0.dim() == 5 and w0.shape[0] == 2 if planar else w0.dim() == 6 and w0.shape[-1] == 2
    for k, w in enumerate(ws):
        _req(w, f"{what}: weights{k + 1}")
        if not ok or w.shape != w0.shape or w.numel() == 0:
            if planar:
                raise ValueError(f"{what}: weights1 / weights2 must both be [2, Cin, Cout, m1, m2], got {tuple(ws[0].shape)} and "
                                 f"{tuple(ws[1].shape)}")
            raise ValueError(f"{what}: every weight must be the real-pair [Cin, Cout, m1, m2, m3, 2], got "
                             f"{[tuple(t.shape) for t in ws]}")
    Cin, Cout, *modes = w0.shape[1:] if planar else w0.shape[:-1]
    return Cin, Cout, tuple(modes)


def _fno_mix(what: str, X: Tensor, ws, adjoint: bool, planar: bool) -> Tensor:
    Cin, Cout, modes = _fno_weights(ws, what, planar)
    K, N = (Cout, Cin) if adjoint else (Cin, Cout)
    _req(X, f"{what}: X")
    kept = _fno_kept(modes)
    if tuple(X.shape[1:]) != kept + (2, K) or X.shape[0] < 1:
        raise ValueError(f"{what}: the spectrum must be [B, {', '.join(map(str, kept))}, 2, {K}], got {tuple(X.shape)}")
    B = X.shape[0]
    O = torch.empty((B,) + kept + (2, N), dtype=torch.float32, device=X.device)
    check(getattr(_lib.load(), "dpot_" + what)(X.data_ptr(), *(w.data_ptr() for w in ws), O.data_ptr(), B, Cin, Cout, *modes,
                                               1 if adjoint else 0, _stream()), what)
    return O


def _fno_mix_wgrad(what: str, X: Tensor, dO: Tensor, outs, accumulate: bool, planar: bool):
    rank = 2 if planar else 3
    _req(X, f"{what}: X")
    _req(dO, f"{what}: dO")
    modes = _fno_kept_modes(X, rank)
    if modes is None or dO.dim() != X.dim() or X.shape[:-1] != dO.shape[:-1] or dO.numel() == 0:
        kept = _fno_kept_text(rank)
        raise ValueError(f"{what}: X [B, {kept}, 2, Cin] and dO [B, {kept}, 2, Cout], got {tuple(X.shape)} and {tuple(dO.shape)}")
    B, Cin, Cout = X.shape[0], X.shape[-1], dO.shape[-1]
    shape = (2, Cin, Cout, *modes) if planar else (Cin, Cout, *modes, 2)
    outs = [_out_buf(o, what, "out", shape, X.device, ValueError) for o in outs]
    check(getattr(_lib.load(), "dpot_" + what)(X.data_ptr(), dO.data_ptr(), *(o.data_ptr() for o in outs), B, Cin, Cout, *modes,
                                               1 if accumulate else 0, _stream()), what)
    return tuple(outs)


def fno_mix(X: Tensor, w1: Tensor, w2: Tensor, adjoint: bool = False) -> Tensor:
    """O[b, r, ky, :, o] = sum_i X[b, r, ky, :, i] W[i, o, r mod m1, ky] (complex), W = w[0] + i w[1], weights1 on the rows
    below m1 and weights2 above, read in place.  adjoint=True: sum over o with conj(W): the data gradient"""
    return _fno_mix("fno_mix", X, (w1, w2), adjoint, planar=True)


def fno3_mix(X: Tensor, ws, adjoint: bool = False) -> Tensor:
    """O[b, r, q, kz, :, o] = sum_i X[b, r, q, kz, :, i] W[i, o, r mod m1, q mod m2, kz] (complex), W the corner weight
    1 + (r >= m1) + 2 (q >= m2) of `ws` = (weights1..weights4), read in place.  adjoint=True: sum over o with conj(W)"""
    if len(ws) != 4:
        raise ValueError(f"fno3_mix: four corner weights (weights1..weights4), got {len(ws)}")
    return _fno_mix("fno3_mix", X, tuple(ws), adjoint, planar=False)


def fno_mix_wgrad(X: Tensor, dO: Tensor, out1: Optional[Tensor] = None, out2: Optional[Tensor] = None,
                  accumulate: bool = False):
    """(dweights1, dweights2) [2, Cin, Cout, m1, m2] from the layer's input spectrum X [B, 2 m1, m2, 2, Cin] and the gradient
    dO [B, 2 m1, m2, 2, Cout] of its output spectrum, summed over b in ascending order; accumulate: added to out1 / out2"""
    if accumulate and (out1 is None or out2 is None):
        raise ValueError("fno_mix_wgrad: accumulate needs out1 and out2")
    return _fno_mix_wgrad("fno_mix_wgrad", X, dO, (out1, out2), accumulate, planar=True)


def fno3_mix_wgrad(X: Tensor, dO: Tensor, outs=None, accumulate: bool = False):
    """(dweights1..dweights4) [Cin, Cout, m1, m2, m3, 2] from the layer's input spectrum X [B, 2 m1, 2 m2, m3, 2, Cin] and the
    gradient dO [.., Cout] of its output spectrum, summed over b in ascending order; outs: four buffers to write (None entries are
    allocated); accumulate: added to them"""
    outs = list(outs) if outs is not None else [None] * 4
    if len(outs) != 4 or (accumulate and any(o is None for o in outs)):
        raise ValueError("fno3_mix_wgrad: outs holds four buffers, and accumulate needs all of them")
    return _fno_mix_wgrad("fno3_mix_wgrad", X, dO, outs, accumulate, planar=False)


def act_bwd_mul(dy: Tensor, pre: Tensor, act: int) -> Tensor:
    """dy * act'(pre), elementwise: the gradient of a pre-activation that feeds no GEMM epilogue"""
    _req(dy, "act_bwd_mul: dy")
    _req(pre, "act_bwd_mul: pre")
    if dy.shape != pre.shape or dy.numel() == 0:
        raise ValueError(f"act_bwd_mul: dy and pre must have one non-empty shape, got {tuple(dy.shape)} and {tuple(pre.shape)}")
    out = torch.empty_like(dy)
    check(_lib.load().dpot_fno_dact(dy.data_ptr(), pre.data_ptr(), out.data_ptr(), dy.numel(), int(act), _stream()), "fno_dact")
    return out


# ------------------------------------------------------------------------------------------------------
# the UNet baseline (csrc/unet.hip): 3x3 convolution, BatchNorm statistics, normalise + activation (+ 2x2 max pooling)
# ------------------------------------------------------------------------------------------------------
BN_MOMENTUM, BN_EPS = 0.1, 1e-5          # torch.nn.BatchNorm2d's defaults, which the reference leaves alone


def unet_limits() -> Tuple[int, int]:
    """(the longest row W, the most channels) the convolution kernels take"""
    lib = _lib.load()
    return lib.dpot_unet_max_size(0), lib.dpot_unet_max_size(1)


def unet_check_sizes(W: int, channels, what: str = "unet") -> None:
    """ValueError naming the size beyond what the kernels of csrc/unet.hip stage (checked before anything is launched)"""
    max_w, max_c = unet_limits()
    if W > max_w:
        raise ValueError(f"{what}: a row of {W} pixels is beyond the staged halo of the convolution kernels (W <= {max_w})")
    for c in channels:
        if c > max_c:
            raise ValueError(f"{what}: {c} channels are beyond the convolution kernels' grid (channels <= {max_c})")


def _field(t: Tensor, what: str, name: str):
    if t.dim() != 4 or t.numel() == 0:
        raise ValueError(f"{what}: {name} must be a non-empty channels-last field [B, H, W, C], got {tuple(t.shape)}")
    _req(t, f"{what}: {name}")
    return tuple(t.shape)


def _conv_weight(w: Tensor, what: str):
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.numel() == 0:
        raise ValueError(f"{what}: the weight must be the parameter [Cout, Cin, 3, 3], got {tuple(w.shape)}")
    _req(w, f"{what}: weight")
    return w.shape[0], w.shape[1]


def conv3x3_stats_elems(npix: int, Cout: int) -> int:
    return int(_lib.load().dpot_conv3x3_stats_elems(npix, Cout))


def _conv3x3(what: str, x: Tensor, w: Tensor, adjoint: bool, stats: bool, out: Optional[Tensor]):
    Cout, Cin = _conv_weight(w, what)
    B, H, W, Cx = _field(x, what, "x")
    K, N = (Cout, Cin) if adjoint else (Cin, Cout)
    if Cx != K:
        raise ValueError(f"{what}: x has {Cx} channels, the weight {tuple(w.shape)} takes {K}")
    unet_check_sizes(W, (Cin, Cout), what)
    out = _out_buf(out, what, "out", (B, H, W, N), x.device, ValueError, x)
    lib = _lib.load()
    part = None
    if stats:
        part = torch.empty(lib.dpot_conv3x3_stats_elems(B * H * W, N), dtype=torch.float32, device=x.device)
    check(lib.dpot_conv3x3(x.data_ptr(), w.data_ptr(), out.data_ptr(), _p(part), B, H, W, Cin, Cout, 1 if adjoint else 0,
                           _stream()), what)
    return out, part


def conv3x3(x: Tensor, w: Tensor, stats: bool = False, out: Optional[Tensor] = None):
    """x [B, H, W, Cin], w the parameter [Cout, Cin, 3, 3] read in place -> z [B, H, W, Cout] = Conv2d(k = 3, padding 1, no
    bias).  stats=True: (z, the per-tile count | mean | M2 partials of z that bn_stats merges) instead of z alone"""
    z, part = _conv3x3("conv3x3", x, w, False, stats, out)
    return (z, part) if stats else z


def conv3x3_bwd_data(dz: Tensor, w: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """dz [B, H, W, Cout] -> dx [B, H, W, Cin]: the same kernel with the taps mirrored and the channel roles exchanged"""
    return _conv3x3("conv3x3_bwd_data", dz, w, True, False, out)[0]


def conv3x3_wgrad(x: Tensor, dz: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """dw [Cout, Cin, 3, 3] = sum over the pixels of dz[p, co] x[p + tap, ci], in the parameter's layout; accumulate: added to
    `out` (a further step of a rollout)"""
    what = "conv3x3_wgrad"
    B, H, W, Cin = _field(x, what, "x")
    if tuple(dz.shape[:3]) != (B, H, W) or dz.dim() != 4:
        raise ValueError(f"{what}: x [B, H, W, Cin] and dz [B, H, W, Cout], got {tuple(x.shape)} and {tuple(dz.shape)}")
    Cout = _field(dz, what, "dz")[3]
    if accumulate and out is None:
        raise ValueError(f"{what}: accumulate needs out")
    unet_check_sizes(W, (Cin, Cout), what)
    out = _out_buf(out, what, "out", (Cout, Cin, 3, 3), x.device, ValueError)
    lib = _lib.load()
    ws = _scratch(torch.empty(lib.dpot_conv3x3_wgrad_ws_elems(B * H * W, Cin, Cout), dtype=torch.float32, device=x.device))
    check(lib.dpot_conv3x3_wgrad(x.data_ptr(), dz.data_ptr(), out.data_ptr(), ws.data_ptr(), B, H, W, Cin, Cout,
                                 1 if accumulate else 0, _stream()), what)
    return out


def _bn_vec(t: Tensor, C: int, what: str, name: str) -> Tensor:
    if tuple(_req(t, f"{what}: {name}").shape) != (C,):
        raise ValueError(f"{what}: {name} must be [{C}], got {tuple(t.shape)}")
    return t


def bn_stats(part: Tensor, npix: int, C: int, running_mean: Optional[Tensor] = None, running_var: Optional[Tensor] = None,
             num_batches_tracked: Optional[Tensor] = None, momentum: float = BN_MOMENTUM, eps: float = BN_EPS):
    """the partials conv3x3(stats=True) left, merged in ascending order -> (mean [C], invstd [C]) of the batch; the running
    buffers (momentum, the unbiased variance) and the int64 counter are updated in the same launch where they are given.  One
    value per channel has no variance: the ValueError of torch.nn.functional.batch_norm"""
    what = "bn_stats"
    if npix <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {[npix, C]}")
    lib = _lib.load()
    if part.numel() != lib.dpot_conv3x3_stats_elems(npix, C):
        raise ValueError(f"{what}: {part.numel()} partials do not belong to {npix} pixels of {C} channels")
    _req(part, f"{what}: partials")
    for name, t in (("running_mean", running_mean), ("running_var", running_var)):
        if t is not None:
            _bn_vec(t, C, what, name)
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1
                                            or not num_batches_tracked.is_cuda):
        raise ValueError(f"{what}: num_batches_tracked must be one int64 on the device")
    stat = torch.empty(2, C, dtype=torch.float32, device=part.device)
    check(lib.dpot_bn_finalize(part.data_ptr(), npix, C, stat[0].data_ptr(), stat[1].data_ptr(), _p(running_mean),
                               _p(running_var), _p(num_batches_tracked), float(momentum), float(eps), _stream()), what)
    return stat[0], stat[1]


def bn_act(z: Tensor, mean: Tensor, stat2: Tensor, gamma: Tensor, beta: Tensor, act: int, pool: bool = False,
           stat_is_var: bool = False, eps: float = BN_EPS, out: Optional[Tensor] = None, out_pool: Optional[Tensor] = None):
    """y = act(gamma (z - mean) invstd + beta) on z [B, H, W, C]; pool: (y, the 2x2 / stride-2 maximum of y [B, H/2, W/2, C])
    from the same launch.  stat_is_var (eval mode): stat2 is the running variance, invstd = 1 / sqrt(stat2 + eps)"""
    what = "bn_act"
    B, H, W, C = _field(z, what, "z")
    for name, t in (("mean", mean), ("stat2", stat2), ("gamma", gamma), ("beta", beta)):
        _bn_vec(t, C, what, name)
    if pool and (H % 2 or W % 2):
        raise ValueError(f"{what}: 2x2 pooling needs an even field, got {H}x{W}")
    y = _out_buf(out, what, "out", (B, H, W, C), z.device, ValueError, z)
    yp = _out_buf(out_pool, what, "out_pool", (B, H // 2, W // 2, C), z.device, ValueError, z) if pool else None
    check(_lib.load().dpot_bn_act(z.data_ptr(), mean.data_ptr(), stat2.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                  y.data_ptr(), _p(yp), B, H, W, C, int(act), 1 if stat_is_var else 0, float(eps), _stream()),
          what)
    return (y, yp) if pool else y


def bn_act_bwd(dy: Optional[Tensor], dpool: Optional[Tensor], z: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor,
               beta: Tensor, act: int, out: Optional[Tensor] = None, out_dgamma: Optional[Tensor] = None,
               out_dbeta: Optional[Tensor] = None):
    """backward of bn_act in training mode -> (dz, dgamma, dbeta).  dy: the gradient of y, dpool: of the pooled field (not
    None exactly when the forward pooled and its pooled output took a gradient; it goes to the FIRST maximum of its window, in
    (row, column) order, as torch.max_pool2d routes it); one of the two may be None.  Two launches: the per-chunk sums of
    g = (dy + routed dpool) act'(pre) and g xhat, then dz = gamma invstd (g - mean(g) - xhat mean(g xhat)) with the sums finished in
    ascending order.  xhat, pre and the maxima are recomputed from z"""
    what = "bn_act_bwd"
    B, H, W, C = _field(z, what, "z")
    if dy is None and dpool is None:
        raise ValueError(f"{what}: neither dy nor dpool")
    if dy is not None and _field(dy, what, "dy") != (B, H, W, C):
        raise ValueError(f"{what}: dy must be {(B, H, W, C)}, got {tuple(dy.shape)}")
    if dpool is not None:
        if H % 2 or W % 2 or _field(dpool, what, "dpool") != (B, H // 2, W // 2, C):
            raise ValueError(f"{what}: dpool must be the pooled field of an even {H}x{W} field, got {tuple(dpool.shape)}")
    for name, t in (("mean", mean), ("invstd", invstd), ("gamma", gamma), ("beta", beta)):
        _bn_vec(t, C, what, name)
    lib = _lib.load()
    dz = _out_buf(out, what, "out", (B, H, W, C), z.device, ValueError, z)
    dgamma = _out_buf(out_dgamma, what, "out_dgamma", (C,), z.device, ValueError)
    dbeta = _out_buf(out_dbeta, what, "out_dbeta", (C,), z.device, ValueError)
    ws = _scratch(torch.empty(lib.dpot_bn_act_bwd_ws_elems(B * H * W, C), dtype=torch.float32, device=z.device))
    head = (_p(dy), _p(dpool), z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ws.data_ptr())
    check(lib.dpot_bn_act_bwd_reduce(*head, B, H, W, C, int(act), _stream()), what + " (reduce)")
    check(lib.dpot_bn_act_bwd_apply(*head, dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), B, H, W, C, int(act), _stream()),
          what + " (apply)")
    return dz, dgamma, dbeta


def unet_upshuffle(z: Tensor, B: int, h: int, w: int, C: int, bias: Optional[Tensor] = None, inverse: bool = False) -> Tensor:
    """the shuffle of a k = s = 2 transposed convolution whose GEMM read the parameter [Cin, C, 2, 2] in place as [Cin, 4 C]:
    z [B h w, 4 C] with columns (c, i, j) -> [B, 2 h, 2 w, C] (+ bias); inverse=True: the field's gradient gathered back into
    that matrix.  (ops.pixel_shuffle takes columns (i, j, c), which would need a permuted copy of the weight.)"""
    what = "unet_upshuffle"
    _req(z, f"{what}: z")
    if z.numel() != B * h * w * 4 * C or z.numel() == 0:
        raise ValueError(f"{what}: {tuple(z.shape)} does not hold B h w 4 C = {B} {h} {w} 4 {C} values")
    if bias is not None:
        _bn_vec(bias, C, what, "bias")
    out = torch.empty((B * h * w, 4 * C) if inverse else (B, 2 * h, 2 * w, C), dtype=torch.float32, device=z.device)
    check(_lib.load().dpot_unet_upshuffle(z.data_ptr(), None if inverse else _p(bias), out.data_ptr(), B, h, w, C,
                                          1 if inverse else 0, _stream()), what)
    return out
