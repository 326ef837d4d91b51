"""Input pipeline for the DPOT step, MI355X side (reference: utils/griddataset.py:27-174 and the
DataLoader of train_temporal.py:106-109).

The reference resizes / pads / windows every sample on CPU workers (F.interpolate per sample) and ships finished
[B,res,res,T,C] batches (2.9 MB per sample at 128^2) through a DataLoader - at the GPU step's ~9 k samples/s that
pipeline is the bottleneck.  Here the CPU side only hands over the RAW trajectories ([H,W,T,C] as stored, e.g. 64x64
for ns2d_fno: 16x fewer bytes than the padded 128x128x4 batch):

    host:    raw samples -> one pinned staging buffer -> ONE async H2D copy on a copy stream
    device:  dpot_resize_pad_window (csrc/data.hip): bilinear resize to res x res, channel pad with ones, temporal
             window [t0, t0+t_in+t_ar) -> xx, yy written straight into one of two (n_buffers) batch slots
    step:    the compute stream waits on the slot's event; while it trains on slot k the copy stream fills slot k+1

HDF5 reading (h5py is not available in this image) stays with the caller: `DeviceBatcher.submit` takes numpy arrays /
CPU tensors.  Dataset mixing and index sharding are host logic (`MixedIndex`, dp.shard_indices).

Also covered (griddataset.py:159-174): test-mode windows (`train=False`: x = the first t_in frames, y = the following
t_test frames, the resolution / channel mask of `get_target_mask`), the per-dataset strided `downsample` of the resized
fields, and `idx_cls` (the dataset index of every sample, int64 [B, 1]).

The 3-D fine-tuning loop (reference: TemporalDataset3D, griddataset.py:454-564, behind the DataLoader of
finetune3d.py:113-117) is fed the same way from raw [H,W,L,T,C] trajectories: `resize_pad_window3` (csrc/data3d.hip:
trilinear resize, channel pad, window, sub-sampling in one launch), `target_mask3`, `DeviceBatcher3D`.  The two batchers
share their slot / event bookkeeping (`_SlotBatcher`); the 3-D one stages only the frames of the window.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import Sample3Desc, SampleDesc, check

Tensor = torch.Tensor


def random_window_start(T: int, t_in: int, t_ar: int, rng: np.random.Generator) -> int:
    """griddataset.py:151  start_idx = np.random.randint(max(T - (t_in + t_ar) + 1, 1))"""
    return int(rng.integers(max(T - (t_in + t_ar) + 1, 1)))


def eval_window(T: int, t_in: int, t_test: int) -> Tuple[int, int]:
    """griddataset.py:159-161 (test datasets return the whole trajectory): (t0, t_ar) = (0, number of frames of
    sample[..., t_in : t_in + t_test, :] that exist)"""
    return 0, max(0, min(t_test, T - t_in))


def target_mask(res: int, size_orig: Sequence[int], n_channels: int) -> Tensor:
    """griddataset.py:103-117: evaluation mask [res, res, 1, n_channels] - ones on the grid points that exist at the
    dataset's own resolution and on its own channels (size_orig = [H, W, T, C_pred])"""
    msk = torch.zeros(res, res, 1, n_channels)
    kx, ky = res // size_orig[0], res // size_orig[1]
    kx, ky = max(kx, 1), max(ky, 1)
    msk[::kx, ::ky, :, :size_orig[-1]] = 1
    return msk


def target_mask3(res: int, size_orig: Sequence[int], n_channels: int) -> Tensor:
    """griddataset.py:503-518: the 3-D evaluation mask [res, res, res, 1, n_channels]
    (size_orig = [H, W, L, T, C_pred]; a target coarser than the data: k == 0 -> 1)"""
    msk = torch.zeros(res, res, res, 1, n_channels)
    kx, ky, kz = (max(res // size_orig[i], 1) for i in range(3))
    msk[::kx, ::ky, ::kz, :, :size_orig[-1]] = 1
    return msk


class MixedIndex:
    """index arithmetic of MixedTemporalDataset (griddataset.py:50-56,133-141): datasets are concatenated, dataset d
    is repeated data_weights[d] times; global index -> (dataset, sample)"""

    def __init__(self, sizes: Sequence[int], weights: Optional[Sequence[int]] = None):
        self.sizes = list(sizes)
        self.weights = list(weights) if weights is not None else [1] * len(self.sizes)
        self.cumulative = np.cumsum([s * w for s, w in zip(self.sizes, self.weights)])

    def __len__(self) -> int:
        return int(self.cumulative[-1])

    def locate(self, idx: int) -> Tuple[int, int]:
        d = int(np.searchsorted(self.cumulative, idx + 1))
        local = idx if d == 0 else idx - int(self.cumulative[d - 1])
        return d, int(local // self.weights[d])


DESC_BYTES = C.sizeof(SampleDesc)          # 32
DESC_FLOATS = DESC_BYTES // 4
assert C.sizeof(Sample3Desc) == DESC_BYTES


def _check_window(i: int, shape: Sequence[int], t0: int, t_in: int, t_ar: int, n_channels: int) -> None:
    """what the kernels assume of sample i, shape = (*spatial, T, C): its channels fit and the window lies inside it"""
    T, Cc = shape[-2], shape[-1]
    if Cc > n_channels or t0 < 0 or t0 + t_in + t_ar > T:
        raise ValueError(f"sample {i}: shape {tuple(shape)}, window [{t0}, {t0 + t_in + t_ar}) - needs C <= "
                         f"{n_channels} and the window inside its {T} frames")


def _fill_table(table: np.ndarray, ptrs: Sequence[int], shapes: Sequence[Sequence[int]], starts: Sequence[int],
                t_in: int, t_ar: int, n_channels: int, desc=SampleDesc) -> None:
    """write the dpot_sample_desc (desc=Sample3Desc: dpot_sample3_desc) records into `table` (uint8 view of host memory),
    validating what the kernel assumes"""
    descs = (desc * len(ptrs)).from_buffer(table)
    for i, (ptr, shape, t0) in enumerate(zip(ptrs, shapes, starts)):
        _check_window(i, shape, t0, t_in, t_ar, n_channels)
        descs[i].data, descs[i].t0 = ptr, int(t0)
        for (name, _), n in zip(desc._fields_[1:], shape):          # H, W, (L,) T, C in the order of the sample's axes
            setattr(descs[i], name, n)


def _down_shape(res: int, downsample: Sequence[int]) -> Tuple[int, ...]:
    down = tuple(int(d) for d in downsample)
    if any(d < 1 for d in down):
        raise ValueError(f"downsample {downsample}: factors must be >= 1")
    return tuple((res + d - 1) // d for d in down)


# spatial axes -> (descriptor, entry point of libdpot_hip, the samples' layout)
_PIPELINES = {2: (SampleDesc, "dpot_resize_pad_window", "[H,W,T,C]"),
              3: (Sample3Desc, "dpot_resize_pad_window3", "[H,W,L,T,C]")}


def _resize_pad_window(nd: int, samples, starts, res, t_in, t_ar, n_channels, out_xx, out_yy, downsample):
    """resize_pad_window (nd = 2) and resize_pad_window3 (nd = 3)"""
    desc, entry, layout = _PIPELINES[nd]
    what = entry[len("dpot_"):]
    if len(downsample) != nd:
        raise ValueError(f"{what}: downsample needs {nd} factors, got {tuple(downsample)}")
    B = len(samples)
    dev = samples[0].device
    out = _down_shape(res, downsample)
    xx = out_xx if out_xx is not None else torch.empty(B, *out, t_in, n_channels, dtype=torch.float32, device=dev)
    yy = out_yy if out_yy is not None else (
        torch.empty(B, *out, t_ar, n_channels, dtype=torch.float32, device=dev) if t_ar > 0 else None)
    for name, buf, t in (("out_xx", out_xx, t_in), ("out_yy", out_yy, t_ar)):
        # the kernel writes a dense [B, *ceil(res/d), t, C] block: any other caller-supplied buffer would be garbled or
        # overrun
        if buf is not None and not (tuple(buf.shape) == (B, *out, t, n_channels) and buf.is_contiguous()
                                    and buf.dtype == torch.float32 and buf.device == dev):
            raise _lib.DpotHipError(f"{what}: {name} must be a contiguous float32 tensor of shape "
                                    f"{(B, *out, t, n_channels)} on {dev}, got {tuple(buf.shape)} {buf.dtype} "
                                    f"{buf.device}")
    for s in samples:
        if not (s.is_cuda and s.dtype == torch.float32 and s.is_contiguous() and s.dim() == nd + 2):
            raise _lib.DpotHipError(f"{what}: samples must be contiguous float32 CUDA tensors {layout}")
    host = np.zeros(B * DESC_BYTES, dtype=np.uint8)
    _fill_table(host, [s.data_ptr() for s in samples], [tuple(s.shape) for s in samples], starts, t_in, t_ar, n_channels,
                desc)
    table = torch.from_numpy(host).to(dev)
    check(getattr(_lib.load(), entry)(table.data_ptr(), B, xx.data_ptr(), yy.data_ptr() if yy is not None else None,
                                      res, t_in, t_ar, n_channels, *(int(d) for d in downsample),
                                      torch.cuda.current_stream().cuda_stream),
          what)
    return xx, yy


def resize_pad_window(samples: Sequence[Tensor], starts: Sequence[int], res: int, t_in: int, t_ar: int,
                      n_channels: int, out_xx: Optional[Tensor] = None, out_yy: Optional[Tensor] = None,
                      downsample: Tuple[int, int] = (1, 1)):
    """samples: CUDA tensors [H,W,T,C] (fp32, contiguous), one per batch entry -> (xx [B,res,res,t_in,Cmax],
    yy [B,res,res,t_ar,Cmax]) through ONE launch of csrc/data.hip.  downsample = (dh, dw): the reference's
    x[::dh, ::dw] on the resized fields (griddataset.py:170-172) - the outputs then have ceil(res/d) points per axis"""
    return _resize_pad_window(2, samples, starts, res, t_in, t_ar, n_channels, out_xx, out_yy, downsample)


def resize_pad_window3(samples: Sequence[Tensor], starts: Sequence[int], res: int, t_in: int, t_ar: int,
                       n_channels: int, out_xx: Optional[Tensor] = None, out_yy: Optional[Tensor] = None,
                       downsample: Tuple[int, int, int] = (1, 1, 1)):
    """samples: CUDA tensors [H,W,L,T,C] (fp32, contiguous), one per batch entry -> (xx [B,res,res,res,t_in,Cmax],
    yy [B,res,res,res,t_ar,Cmax]; yy is None when t_ar == 0) through ONE launch of csrc/data3d.hip: trilinear resize,
    channel pad with ones, window [t0, t0 + t_in + t_ar).  downsample = (d0, d1, d2): the reference's
    x[::d0, ::d1, ::d2] on the resized fields (griddataset.py:557-558) - ceil(res/d) points per axis"""
    return _resize_pad_window(3, samples, starts, res, t_in, t_ar, n_channels, out_xx, out_yy, downsample)


class _SlotBatcher:
    """What DeviceBatcher and DeviceBatcher3D share, i.e. everything but the layout of a sample: the pinned staging buffers
    with the descriptor table at their head, the batch slots, and the slot / event / pending bookkeeping of submit, get
    and release.  A subclass names its number of spatial axes and says which part of a raw sample is staged."""
    _nd: int

    def __init__(self, batch: int, res: int, t_in: int, t_ar: int, n_channels: int, max_raw_floats_per_sample: int,
                 device, n_buffers: int, downsample: Sequence[int]):
        nd = self._nd
        self._desc, entry, self._layout = _PIPELINES[nd]
        self._entry, self._what = entry, entry[len("dpot_"):]
        if len(downsample) != nd:
            raise ValueError(f"{type(self).__name__}: downsample needs {nd} factors, got {tuple(downsample)}")
        self.B, self.res, self.t_in, self.t_ar, self.C = batch, res, t_in, t_ar, n_channels
        self.down = tuple(int(d) for d in downsample)
        out = _down_shape(res, self.down)
        self.dev = torch.device(device)
        self.n = n_buffers
        self.head = batch * DESC_FLOATS                # the descriptor table rides at the head of the staging buffer
        cap = self.head + batch * max_raw_floats_per_sample
        self.stream = torch.cuda.Stream(device=self.dev)
        self.host = [torch.empty(cap, dtype=torch.float32).pin_memory() for _ in range(n_buffers)]
        self.raw = [torch.empty(cap, dtype=torch.float32, device=self.dev) for _ in range(n_buffers)]
        self.xx = [torch.empty(batch, *out, t_in, n_channels, device=self.dev) for _ in range(n_buffers)]
        self.yy = [torch.empty(batch, *out, t_ar, n_channels, device=self.dev) for _ in range(n_buffers)]
        # training mask (griddataset.py:157, :548: ones at the window's resolution, i.e. BEFORE the down-sampling - the
        # reference does not sub-sample msk; test-mode masks: `target_mask` / `target_mask3` per dataset)
        self.msk = torch.ones(batch, *(res,) * nd, 1, n_channels, device=self.dev)
        self.cls = [torch.zeros(batch, 1, dtype=torch.int64, device=self.dev) for _ in range(n_buffers)]
        self.cls_host = [torch.zeros(batch, 1, dtype=torch.int64).pin_memory() for _ in range(n_buffers)]
        self.ready = [torch.cuda.Event() for _ in range(n_buffers)]       # slot filled (recorded on the copy stream)
        self.consumed = [None] * n_buffers                                # slot's last reader (recorded on compute)
        self.k = 0
        self.pending: List[int] = []
        self.used = [False] * n_buffers                                   # slot has been filled at least once
        self._out = set()                                                 # slots handed out by get(), not yet released
        self._last: Optional[int] = None
        self.h2d_bytes = 0

    def _stage(self, a: np.ndarray, t0: int) -> Tuple[np.ndarray, int]:
        """(the part of raw sample `a` that goes to the device - a view, any strides -, the window start inside it)"""
        raise NotImplementedError

    def submit(self, samples: Sequence, starts: Sequence[int], dataset_ids: Optional[Sequence[int]] = None) -> None:
        """enqueue one batch: samples = numpy arrays / CPU tensors in the batcher's layout (or without the channel axis);
        returns immediately.  dataset_ids: the dataset index of every sample (griddataset.py:174 idx_cls; default zeros)"""
        assert len(samples) == self.B and len(starts) == self.B
        assert dataset_ids is None or len(dataset_ids) == self.B
        me = type(self).__name__
        slot = self.k % self.n
        # validate BEFORE anything is overwritten (a bad batch must leave the slot and the counters untouched)
        parts, offs, t0s, off = [], [], [], self.head
        for i, (s, t0) in enumerate(zip(samples, starts)):
            a = np.asarray(s, dtype=np.float32) if not torch.is_tensor(s) else s.detach().float().numpy()
            if a.ndim == self._nd + 1:
                a = a[..., None]                       # griddataset.py:145, :535 "augment channel dim"
            if a.ndim != self._nd + 2:
                raise ValueError(f"sample {i}: shape {a.shape} is not {self._layout}")
            _check_window(i, a.shape, t0, self.t_in, self.t_ar, self.C)
            part, t0 = self._stage(a, int(t0))
            if off + part.size > self.host[slot].numel():
                raise ValueError(f"{me}: raw samples exceed max_raw_floats_per_sample")
            parts.append(part)
            offs.append(off)
            t0s.append(t0)
            off += part.size
        # the slot is reused: its pinned staging buffer, raw buffer and xx / yy must be free.  The previous H2D copy +
        # transform of this slot (copy stream) and the step that read it (recorded by release()) are waited for; a slot
        # that was handed out by get() but never release()d has an unknown reader - wait for the whole device then
        if slot in self.pending or slot in self._out:
            if slot in self.pending:
                raise RuntimeError(f"{me}: all {self.n} slots hold batches that were never fetched with get()")
            torch.cuda.synchronize(self.dev)           # unreleased consumer: conservative, correct
            self._out.discard(slot)
        if self.used[slot]:
            self.ready[slot].synchronize()
        if self.consumed[slot] is not None:
            self.consumed[slot].synchronize()          # host buffer / device slot are free again (normally long since)
            self.consumed[slot] = None
        self.k += 1
        self.used[slot] = True
        host = self.host[slot]
        hnp = host.numpy()
        for p, o in zip(parts, offs):
            hnp[o:o + p.size].reshape(p.shape)[...] = p
        base = self.raw[slot].data_ptr()
        _fill_table(hnp[:self.head].view(np.uint8), [base + 4 * o for o in offs], [p.shape for p in parts], t0s, self.t_in,
                    self.t_ar, self.C, self._desc)
        self.cls_host[slot].zero_()
        if dataset_ids is not None:
            self.cls_host[slot][:, 0] = torch.as_tensor(list(dataset_ids), dtype=torch.int64)
        with torch.cuda.stream(self.stream):
            self.raw[slot][:off].copy_(host[:off], non_blocking=True)            # ONE H2D copy: table + raw samples
            self.cls[slot].copy_(self.cls_host[slot], non_blocking=True)
            check(getattr(_lib.load(), self._entry)(base, self.B, self.xx[slot].data_ptr(), self.yy[slot].data_ptr(),
                                                    self.res, self.t_in, self.t_ar, self.C, *self.down,
                                                    self.stream.cuda_stream),
                  self._what)
            self.ready[slot].record(self.stream)
        self.h2d_bytes += (off - self.head) * 4
        self.pending.append(slot)

    def get(self) -> Tuple[Tensor, Tensor, Tensor]:
        """the oldest submitted batch; the CURRENT stream waits for it (no host synchronisation).  The tensors stay
        valid until `n_buffers` further submits; call `release()` (or `release(slot)` with `last_slot`) after the step that
        reads them was enqueued - a slot that is re-used without having been released costs a device synchronise."""
        slot = self.pending.pop(0)
        torch.cuda.current_stream().wait_event(self.ready[slot])
        self._last = slot
        self._out.add(slot)
        return self.xx[slot], self.yy[slot], self.msk

    @property
    def last_cls(self) -> Optional[Tensor]:
        """idx_cls [B, 1] int64 of the batch the latest get() returned (griddataset.py:174; train_temporal.py:199)"""
        return None if self._last is None else self.cls[self._last]

    @property
    def last_slot(self) -> Optional[int]:
        """token of the batch the latest get() returned (pass it to release() when several batches are in flight)"""
        return self._last

    def release(self, slot: Optional[int] = None) -> None:
        """the step reading batch `slot` (default: the latest get()) has been enqueued on the current stream"""
        slot = self._last if slot is None else slot
        if slot is None or slot not in self._out:
            raise RuntimeError(f"{type(self).__name__}.release: no batch outstanding for this slot")
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self.consumed[slot] = ev
        self._out.discard(slot)


class DeviceBatcher(_SlotBatcher):
    """Double-buffered batch producer: raw samples [H,W,T,C] in, device-resident (xx, yy, msk) out, overlapped with the
    step."""
    _nd = 2

    def __init__(self, batch: int, res: int, t_in: int, t_ar: int, n_channels: int, max_raw_floats_per_sample: int,
                 device="cuda", n_buffers: int = 2, downsample: Tuple[int, int] = (1, 1)):
        """t_ar: frames of y per sample (training: the rollout length; test mode: t_test of the dataset, with
        starts = 0 - see `eval_window`).  downsample: one factor pair per batcher (a batch is one tensor)."""
        super().__init__(batch, res, t_in, t_ar, n_channels, max_raw_floats_per_sample, device, n_buffers, downsample)

    def _stage(self, a, t0):
        return a, t0                                   # the whole trajectory


class DeviceBatcher3D(_SlotBatcher):
    """DeviceBatcher for raw samples [H,W,L,T,C] (csrc/data3d.hip): (xx [B,r0,r1,r2,t_in,C], yy [B,r0,r1,r2,t_ar,C],
    msk = ones [B,res,res,res,1,C]).  One difference: only the FRAMES OF THE WINDOW are staged and copied - a
    [128,128,128,21,5] trajectory sends the 461 MB of its 11 frames, not 880 MB - so the device sees samples with
    T = t_in + t_ar and t0 = 0, and `max_raw_floats_per_sample` / `h2d_bytes` count the staged floats (`staged_floats`)."""
    _nd = 3

    def __init__(self, batch: int, res: int, t_in: int, t_ar: int, n_channels: int, max_raw_floats_per_sample: int,
                 device="cuda", n_buffers: int = 2, downsample: Tuple[int, int, int] = (1, 1, 1)):
        super().__init__(batch, res, t_in, t_ar, n_channels, max_raw_floats_per_sample, device, n_buffers, downsample)

    def _stage(self, a, t0):
        return a[..., t0:t0 + self.t_in + self.t_ar, :], 0


def staged_floats(shape: Sequence[int], t_in: int, t_ar: int) -> int:
    """floats DeviceBatcher3D stages for one raw sample of `shape` ([H,W,L,T,C] or [H,W,L,T]): its window's frames"""
    H, W, L = shape[:3]
    return H * W * L * (t_in + t_ar) * (shape[4] if len(shape) == 5 else 1)
