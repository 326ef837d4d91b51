"""shared helpers for the parity tests"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# north_star tolerance: outputs match the reference PyTorch-CPU path within rtol=1e-4 (fp32 / complex64).
# Element-wise rtol is meaningless for values that cancel to ~0, so - like torch.testing - we pair it with an
# absolute term scaled to the tensor's magnitude:  |a-b| <= RTOL*|b| + RTOL*max|b|
RTOL = 1e-4


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def _first_index(mask):
    """index tuple of the first True element of a bool tensor (row-major order)"""
    flat = int(torch.nonzero(mask.reshape(-1))[0])
    return tuple(int(i) for i in np.unravel_index(flat, tuple(mask.shape))) if mask.dim() else ()


def assert_close(a, b, what="", rtol=RTOL, atol_scale=RTOL, equal_nan=False):
    """|a-b| <= rtol*|b| + atol_scale*max|b| element-wise.  A NaN or inf in a or b fails, whatever the other side holds:
    it cannot be compared (NaN > tol is False, so the tolerance test alone would pass it).  equal_nan=True admits the
    positions where b holds the SAME non-finite value (NaN with NaN, +inf with +inf, -inf with -inf) - only for a
    comparison whose reference itself is non-finite there.  The message counts NaN and inf apart from the
    out-of-tolerance elements: an all-NaN output was never written, a few wrong numbers were computed wrongly."""
    a = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a.detach().cpu()).double()
    b = torch.as_tensor(np.asarray(b) if not torch.is_tensor(b) else b.detach().cpu()).double()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    nonfin = ~(torch.isfinite(a) & torch.isfinite(b))
    n_nan, n_inf = int(a.isnan().sum()), int(a.isinf().sum())
    if nonfin.any():
        same = (a.isnan() & b.isnan()) | (a.isinf() & b.isinf() & (a == b))
        reject = nonfin & ~same if equal_nan else nonfin
        assert not reject.any(), (
            f"{what}: non-finite values cannot be compared: got has {n_nan} NaN and {n_inf} "
            f"inf, reference has {int(b.isnan().sum())} NaN and {int(b.isinf().sum())} inf, of {a.numel()} elements; "
            f"first offender at index {_first_index(reject)} (got {a[reject][0].item()}, reference {b[reject][0].item()})")
        fin = ~nonfin                                                 # equal_nan: the rest is compared as usual
        if not fin.any():
            return 0.0
        scale = b[fin].abs().max().item()
        a, b = torch.where(fin, a, torch.zeros_like(a)), torch.where(fin, b, torch.zeros_like(b))
    else:
        scale = b.abs().max().item()
    tol = rtol * b.abs() + atol_scale * scale + 1e-30
    err = (a - b).abs()
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} elements out of tolerance ({n_nan} NaN, {n_inf} inf"
                           f"{' equal to the reference and not compared' if n_nan + n_inf else ''}); "
                           f"max|d|={err.max().item():.3e} scale={scale:.3e}; first offender at index {_first_index(bad)} "
                           f"(got {a[bad][0].item():.9g}, reference {b[bad][0].item():.9g})")
    return err.max().item() / (scale + 1e-30)


def assert_sub(t, fx, key, what="", rtol=RTOL):
    """compare a big tensor against a stored subsample + checksums"""
    stride = int(fx[key + ".stride"])
    f = t.detach().cpu().reshape(-1)
    nonfin = ~torch.isfinite(f)
    assert not nonfin.any(), (f"{what}: non-finite values cannot be compared: got has {int(f.isnan().sum())} NaN and "
                              f"{int(f.isinf().sum())} inf of {f.numel()} elements; first offender at flat index "
                              f"{_first_index(nonfin)}")
    assert_close(f[::stride], fx[key + ".sub"], what + ".sub", rtol=rtol)
    s = f.double().sum().item()
    a = f.double().abs().sum().item()
    assert abs(a - float(fx[key + ".abssum"])) <= 10 * rtol * float(fx[key + ".abssum"]), what + ".abssum"
    assert abs(s - float(fx[key + ".sum"])) <= 10 * rtol * float(fx[key + ".abssum"]), what + ".sum"


def set_tune(monkeypatch, **kv):
    """DPOT_TUNE with the given keys set (merged over whatever the process - e.g. an opt-out child - already has); only the
    PYTHON-side readers see a change made inside a running process (the C library reads DPOT_TUNE once): use it for the keys
    dpot_amd/ops.py consults per call (mixer, afno_layer, packs, fused_small, embed_implicit)"""
    import os
    cur = dict(x.split("=") for x in os.environ.get("DPOT_TUNE", "").split(",") if x)
    cur.update({k: str(v) for k, v in kv.items()})
    monkeypatch.setenv("DPOT_TUNE", ",".join(f"{k}={v}" for k, v in cur.items()))


def tune_value(key, default):
    import os
    cur = dict(x.split("=") for x in os.environ.get("DPOT_TUNE", "").split(",") if x)
    return int(cur.get(key, default))

