"""Guarded, poisoned allocations for the parity tests: the out-of-bounds and unwritten-output check of this suite.

A plain helper module like helpers.py (no conftest, no plugin, no product change).  dpot_amd.ops / functional / train / data
allocate every result tensor, workspace and pack through their module attribute `torch` (torch.empty, torch.empty_like,
torch.zeros, torch.zeros_like).  A test swaps that attribute for a proxy (the `guarded` fixture does it with monkeypatch);
the proxy forwards everything to the real torch except those four allocators, which hand out

    [ guard | body | guard ]      one raw byte buffer; guard = min(max(body bytes, 64 KiB), 8 MiB) rounded up to 512 bytes

with the body returned as a contiguous, 512-byte aligned tensor of the requested shape and dtype (the alignment the kernels
ask for: aligned16, ld % 4).  The upper guard starts at the first byte after the body.

  floating / complex dtypes   guards are bytes 0xFF (every fp32, bf16, fp16, fp64 lane a NaN); the body of empty / empty_like
                              is NaN as well, the body of zeros / zeros_like is zero as the product code asked
  integer / bool dtypes       body AND guards are zero (job tables, chunk tables, counters): a poison must never be a value
                              that sends a kernel out of bounds when it is read as an index or a count - the harness finds
                              faults, it does not make them.  Limit: a stray write of ZERO into an integer guard is not seen.

What it finds, together with helpers.assert_close (which rejects NaN):
  * an element of a result the kernel never wrote (it stays NaN),
  * a kernel that needs its workspace, or the padded rows of a pack, to hold zeros or finite numbers (garbage * 0 in a masked
    tail is only right while the garbage is finite: NaN * 0 = NaN reaches the result),
  * a store before or past a buffer (check() compares every guard byte with its pattern),
  * a load before or past a buffer whose value reaches a result (NaN from the guard).
What it does not find: a load past a buffer whose value is discarded; a stray access that jumps further than the guard; a
stray write into an integer guard of the value zero, or into a float guard of the byte 0xFF.

Not covered: allocations made while the stream is capturing (torch.cuda.is_current_stream_capturing(): a poison fill must
not be recorded into a graph - they pass through), CPU tensors (unless Harness(cpu=True): the self-tests), zero-element
tensors, exotic forms (out=, pin_memory, a non-contiguous memory format or a non-contiguous empty_like source: passed
through and counted in Harness.passed_through), and the five Tensor.new_empty calls of the package: four are the
zero-element placeholders of save_for_backward (functional.py, train.py: nothing to guard) and one is the embed weight
table of packs.WeightPacks, a buffer that lives as long as the model and so outlives any one test's check().

The harness keeps its raw buffers until check().  Above 8 GiB held it checks early and releases what nothing else
references: a buffer whose storage is still in use (the test or the product code holds the tensor or a view of it) stays on
record and is checked again at the end - it is for op-level and small-model tests, not for the DPOT-L sized ones.

Test-facing surface: wrap(t) (a test's own input in a guarded buffer), full_nan(shape) (an out= slot: NaN body, guards),
check(), and the fixture `guarded` (install the proxy, yield the harness, check() at teardown).
"""
import sys

import pytest
import torch as _torch

ALIGN = 512
GUARD_MIN = 64 << 10
GUARD_MAX = 8 << 20
HOLD_LIMIT = 8 << 30
PATCHED = ("dpot_amd.ops", "dpot_amd.functional", "dpot_amd.train", "dpot_amd.data")


def guard_bytes(body_bytes):
    g = min(max(body_bytes, GUARD_MIN), GUARD_MAX)
    return (g + ALIGN - 1) // ALIGN * ALIGN


def _poisoned(dtype):
    return dtype.is_floating_point or dtype.is_complex


class GuardError(AssertionError):
    pass


class _Rec:
    __slots__ = ("raw", "lo", "hi", "pat", "shape", "dtype", "who", "total")


def _in_use(raw):
    """does anything but the harness's own `raw` tensor use this storage (the body handed out, or a view of it)?  Unknown
    (no use count in this torch) counts as in use: a record is never dropped while its buffer may still be written"""
    st = raw.untyped_storage()
    count = getattr(_torch._C, "_storage_Use_Count", None)
    return True if count is None else count(st._cdata) > 2      # 2 = `raw` + the handle `st`


class Harness:
    def __init__(self, cpu=False, modules=PATCHED):
        self.cpu = cpu
        self.modules = tuple(modules)
        self.records = []
        self.held = 0
        self.n_guarded = 0
        self.passed_through = 0
        self.proxy = TorchProxy(self)

    # -- allocation ----------------------------------------------------------------------------------------
    def _who(self):
        """the innermost function of a patched module on the call stack: 'dpot_amd.ops.gemm:123'"""
        f = sys._getframe(2)
        first = None
        while f is not None:
            mod = f.f_globals.get("__name__", "")
            if mod != __name__ and first is None:
                first = f"{mod}.{f.f_code.co_name}:{f.f_lineno}"
            if mod in self.modules:
                return f"{mod}.{f.f_code.co_name}:{f.f_lineno}"
            f = f.f_back
        return first or "?"

    def eligible(self, device, n_elems):
        if n_elems == 0:
            return False
        if device.type == "cpu":
            return self.cpu
        if device.type != "cuda":
            return False
        return not _torch.cuda.is_current_stream_capturing()

    def alloc(self, shape, dtype, device, zero=False, who=None):
        """[guard | body | guard] on `device`; returns the body.  Caller has checked eligible()."""
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        nbytes = n * dtype.itemsize
        g = guard_bytes(nbytes)
        total = g + nbytes + g + ALIGN
        if self.held + total > HOLD_LIMIT and self.records:
            self.check(keep_live=True)
        poisoned = _poisoned(dtype)
        if poisoned:
            raw = _torch.full((total,), 0xFF, dtype=_torch.uint8, device=device)
        else:
            raw = _torch.zeros(total, dtype=_torch.uint8, device=device)
        off = (-raw.data_ptr()) % ALIGN + g                      # body starts 512-aligned, a whole guard above the base
        body = raw[off:off + nbytes]
        if poisoned and zero:
            body.zero_()
        body = body.view(dtype).view(shape)
        r = _Rec()
        r.raw, r.lo, r.hi = raw, (off - g, off), (off + nbytes, off + nbytes + g)
        r.pat = 0xFF if poisoned else 0
        r.shape, r.dtype, r.who, r.total = shape, dtype, who or self._who(), total
        self.records.append(r)
        self.held += total
        self.n_guarded += 1
        return body

    # -- the test-facing surface ---------------------------------------------------------------------------
    def wrap(self, t, device=None):
        """a copy of t (on `device`, default t's own) inside a guarded buffer"""
        device = _torch.device(device) if device is not None else t.device
        if device.type == "cuda" and device.index is None:
            device = _torch.device("cuda", _torch.cuda.current_device())
        t = t.detach()
        if not self.eligible(device, t.numel()):
            return t.to(device).contiguous()
        out = self.alloc(t.shape, t.dtype, device, who="guard.wrap (test input)")
        out.copy_(t)
        return out

    def full_nan(self, shape, dtype=_torch.float32, device="cuda"):
        """an out= slot: NaN body between guards (the torch.full(shape, nan) idiom, with guards)"""
        if isinstance(shape, int):
            shape = (shape,)
        device = _torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = _torch.device("cuda", _torch.cuda.current_device())
        assert _poisoned(dtype), "full_nan is for floating dtypes"
        if not self.eligible(device, 1):
            return _torch.full(tuple(shape), float("nan"), dtype=dtype, device=device)
        return self.alloc(shape, dtype, device, who="guard.full_nan (test out= slot)")

    def check(self, keep_live=False):
        """compare every guard byte with its pattern (reductions on the device, one host sync), name the offenders, release
        the harness's references - all of them, or with keep_live (the early check) only those of buffers nothing else uses"""
        recs = self.records
        self.records = [r for r in recs if _in_use(r.raw)] if keep_live else []
        self.held = sum(r.total for r in self.records)
        if not recs:
            return
        stats = []
        for r in recs:
            lo, hi = r.raw[r.lo[0]:r.lo[1]], r.raw[r.hi[0]:r.hi[1]]
            if r.pat:                                            # 0xFF everywhere <=> min == 255
                stats.append(255 - _torch.minimum(lo.amin(), hi.amin()).to(_torch.int32))
            else:                                                # 0 everywhere <=> max == 0
                stats.append(_torch.maximum(lo.amax(), hi.amax()).to(_torch.int32))
        by_dev = {}
        for i, s in enumerate(stats):
            by_dev.setdefault(s.device, []).append(i)
        bad = []
        for dev, idx in by_dev.items():
            flags = _torch.stack([stats[i] for i in idx]).cpu()  # the one host sync (per device)
            bad += [idx[j] for j in _torch.nonzero(flags).flatten().tolist()]
        if not bad:
            return
        lines = []
        for i in sorted(bad):
            r = recs[i]
            for side, (a, b) in (("below", r.lo), ("above", r.hi)):
                hit = _torch.nonzero(r.raw[a:b] != r.pat).flatten().cpu()
                if hit.numel():
                    first = int(hit[0])
                    # byte offset relative to the body: negative = before its first byte, >= 0 = past its last byte
                    rel = first - (b - a) if side == "below" else first
                    lines.append(f"{tuple(r.shape)} {str(r.dtype).replace('torch.', '')} allocated by {r.who}: "
                                 f"{hit.numel()} guard byte(s) overwritten {side} the buffer, first at byte offset {rel} "
                                 f"({'from the start of the body' if side == 'below' else 'past the end of the body'})")
        raise GuardError(f"stray writes into {len(bad)} of {len(recs)} guarded buffers:\n  " + "\n  ".join(lines))


class TorchProxy:
    """stands in for the module attribute `torch` of a product module: the four allocators are guarded, all else is torch's"""

    def __init__(self, harness):
        object.__setattr__(self, "_h", harness)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def _new(self, real, zero, size, kw):
        h = self._h
        if len(size) == 1 and isinstance(size[0], (tuple, list, _torch.Size)):
            size = tuple(size[0])
        extra = set(kw) - {"dtype", "device", "requires_grad", "memory_format", "layout", "pin_memory"}
        plain = (not extra and not kw.get("pin_memory") and kw.get("layout", _torch.strided) is _torch.strided
                 and kw.get("memory_format", _torch.contiguous_format) is _torch.contiguous_format
                 and all(isinstance(s, int) for s in size))
        if plain:
            dtype = kw.get("dtype") or _torch.get_default_dtype()
            device = _torch.device(kw["device"]) if kw.get("device") is not None else _torch.get_default_device()
            if device.type == "cuda" and device.index is None:
                device = _torch.device("cuda", _torch.cuda.current_device())
            n = 1
            for s in size:
                n *= s
            if h.eligible(device, n):
                t = h.alloc(size, dtype, device, zero=zero)
                return t.requires_grad_(True) if kw.get("requires_grad") else t
        h.passed_through += 1
        return real(*size, **kw) if size else real(size, **kw)

    def _like(self, real, zero, src, kw):
        h = self._h
        extra = set(kw) - {"dtype", "device", "requires_grad", "memory_format", "layout", "pin_memory"}
        fmt = kw.get("memory_format", _torch.preserve_format)
        plain = (not extra and not kw.get("pin_memory") and kw.get("layout", _torch.strided) is _torch.strided
                 and src.layout is _torch.strided and src.is_contiguous()
                 and fmt in (_torch.preserve_format, _torch.contiguous_format))
        if plain:
            dtype = kw.get("dtype") or src.dtype
            device = _torch.device(kw["device"]) if kw.get("device") is not None else src.device
            if device.type == "cuda" and device.index is None:
                device = _torch.device("cuda", _torch.cuda.current_device())
            if h.eligible(device, src.numel()):
                t = h.alloc(src.shape, dtype, device, zero=zero)
                return t.requires_grad_(True) if kw.get("requires_grad") else t
        h.passed_through += 1
        return real(src, **kw)

    def empty(self, *size, **kw):
        return self._new(_torch.empty, False, size, kw)

    def zeros(self, *size, **kw):
        return self._new(_torch.zeros, True, size, kw)

    def empty_like(self, src, **kw):
        return self._like(_torch.empty_like, False, src, kw)

    def zeros_like(self, src, **kw):
        return self._like(_torch.zeros_like, True, src, kw)


# ---- module-level surface: the harness the `guarded` fixture installed ------------------------------------------------
_active = None


def _need():
    assert _active is not None, "no guard harness is active: use the `guarded` fixture"
    return _active


def wrap(t, device=None):
    return _need().wrap(t, device)


def full_nan(shape, dtype=_torch.float32, device="cuda"):
    return _need().full_nan(shape, dtype, device)


def check():
    _need().check()


@pytest.fixture
def guarded(monkeypatch):
    """install the proxy in the product modules, yield the harness, check the guards at teardown"""
    global _active
    import importlib
    h = Harness()
    for name in h.modules:
        monkeypatch.setattr(importlib.import_module(name), "torch", h.proxy)
    prev, _active = _active, h
    try:
        yield h
        h.check()
    finally:
        _active = prev
        h.records, h.held = [], 0
