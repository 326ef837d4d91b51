#!/usr/bin/env python
"""Generate tests/golden/g16_evalmetrics.npz from the REFERENCE's Evaluator(temporal=True, griddata=True, component='all')
(utils/criterion.py:189-239, compute_fourier_error :246-360).  TEST INFRASTRUCTURE ONLY: the reference is imported at run
time from $DPOT_REFERENCE and nothing of it is copied.

    DPOT_REFERENCE=/path/to/DPOT python scripts/make_golden_evalmetrics.py

Per case: `<case>.shape` [B, X, Y, T, C], `<case>.batches` (how the B samples are split into update() calls; the expectation
is always the reference on ALL B samples at once), `<case>.bands` (ilow, ihigh), the inputs (`<case>.pred`, `<case>.target`
float32 for the small cases; the evaluation-sized cases store only `<case>.salt`, tests/eval_ref.hashed_pair restores them
bit for bit), and for each of the reference's ten keys its float64 result (`<case>.<key>.r64`, float64) and its own float32
result (`<case>.<key>.r32`), so that a test can print the reference's float32 error beside the kernel's.

The float64 run widens the inputs and also sets torch's default dtype to float64 around the call: compute_fourier_error
allocates its shell buffer with torch.zeros(...) in the DEFAULT dtype, so without that its "float64" spectrum would be
rounded to float32 on every accumulation.  The float32 run is the reference as a user calls it.

Small cases: even / odd / rectangular planes, T x C of 1x1, 2x2, 3x2 and 10x4, plain independent fields and
nearly-equal ones; `e16_default` has the default bands on a plane so small (K = 8 <= ihigh) that fmse_high is an empty
band: NaN, stored as NaN.  The evaluation-sized cases take target = smooth + offset + noise and pred = target + a small
perturbation, the regime in which the float32 difference of two spectra cancels."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DPOT_REFERENCE")
if not REF:
    sys.exit("set DPOT_REFERENCE to a checkout of the reference (HaoZhongkai/DPOT)")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from utils.criterion import Evaluator  # noqa: E402  (reference)
from eval_ref import KEYS, hashed_pair  # noqa: E402  (tests/)
from resize_ref import hash_field  # noqa: E402  (tests/)

OUT = os.path.join(ROOT, "tests", "golden", "g16_evalmetrics.npz")
# name: (batches, n_x, n_y, T, C, ilow, ihigh, kind)   kind: 'indep' = independent fields, 'near' = pred close to target,
#                                                            'hash' = near, inputs from the integer hash (not stored)
CASES = {
    "e16_default": ((2,), 16, 16, 2, 2, 4, 12, "indep"),
    "e16_t10c4": ((2,), 16, 16, 10, 4, 2, 5, "near"),
    "o9x11_t3c2": ((3,), 9, 11, 3, 2, 2, 3, "indep"),
    "r12x10_t1c1": ((1,), 12, 10, 1, 1, 1, 3, "near"),
    "two_batches": ((2, 3), 12, 10, 2, 2, 2, 4, "near"),
    "big64": ((2,), 64, 64, 1, 4, 4, 12, "hash"),
    "big128": ((1,), 128, 128, 2, 2, 4, 12, "hash"),
}


def main():
    gen = torch.Generator().manual_seed(1616)
    out = {"names": np.array(list(CASES))}
    for i, (name, (batches, nx, ny, T, C, ilow, ihigh, kind)) in enumerate(CASES.items()):
        shape = (sum(batches), nx, ny, T, C)
        if kind == "hash":
            p, t = (torch.from_numpy(a) for a in hashed_pair(shape, i, hash_field))
            out[f"{name}.salt"] = np.int64(i)
        else:
            if kind == "indep":
                p, t = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
            else:
                t = torch.randn(shape, generator=gen) + 0.5
                p = t + 0.05 * torch.randn(shape, generator=gen)
            out[f"{name}.pred"], out[f"{name}.target"] = p.numpy(), t.numpy()
        out[f"{name}.shape"] = np.array(shape, dtype=np.int64)
        out[f"{name}.batches"] = np.array(batches, dtype=np.int64)
        out[f"{name}.bands"] = np.array([ilow, ihigh], dtype=np.int64)
        ev = Evaluator(temporal=True, griddata=True, component="all", ilow=ilow, ihigh=ihigh)
        r32 = ev(p, t)
        torch.set_default_dtype(torch.float64)
        try:
            r64 = ev(p.double(), t.double())
        finally:
            torch.set_default_dtype(torch.float32)
        assert set(r32) == set(KEYS) == set(r64)
        for key in KEYS:
            assert r64[key].dtype == np.float64 and r32[key].dtype == np.float32 and r64[key].shape == r32[key].shape
            out[f"{name}.{key}.r64"], out[f"{name}.{key}.r32"] = r64[key], r32[key]
        K = min(nx // 2, ny // 2)
        assert np.isnan(r64["fmse_high"]).all() == (K <= ihigh), name
        assert tuple(r64["bdmse"].shape) == (C, T) and tuple(r64["fmse_low"].shape) == (T, C)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.0f} KiB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
