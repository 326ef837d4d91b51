#!/usr/bin/env python
"""Generate tests/golden/g15_resize.npz from the REFERENCE's Fourier resize (utils/utilities.py:277-305, temporal=True) and
its refill_mask rule.  TEST INFRASTRUCTURE ONLY: the reference is imported at run time from $DPOT_REFERENCE and nothing of
it is copied.

    DPOT_REFERENCE=/path/to/DPOT python scripts/make_golden_resize.py

Every case is a seeded field x [B, n_x, n_y, T, C] resized to (m_x, m_y): stored are the float32 input (`<case>.x`; the
float64 run uses the same values widened; the evaluation-sized cases take theirs from tests/resize_ref.hash_field, an
exact integer hash, and store only its salt), the reference's float64 result rounded to fp32 (`<case>.y64`) together with
the float64 result itself for the small cases (`<case>.y64d`, what the 1e-10 checks need), and the reference's own float32
result as its distance from `y64` in fp32 bit patterns (`<case>.y32ulps`, int32: small integers compress where the
floats do not; tests/resize_ref.ulps_apply restores the exact float32 values).  Small cases cover every parity combination, the identity size pair, rectangular planes and
T x C of 2 x 2 and 1 x 1; three evaluation-sized cases carry one or two planes.  Also one refill_mask case with an empty
channel (evaluate_varyingres.py:198-201, restated below in three lines because that script cannot be imported: it runs an
evaluation at import)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DPOT_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from utils.utilities import resize  # noqa: E402  (reference)
from resize_ref import hash_field, ulps_apply  # noqa: E402  (tests/)

OUT = os.path.join(ROOT, "tests", "golden", "g15_resize.npz")
# name: (B, n_x, n_y, T, C, m_x, m_y)
CASES = {
    "e16_o9": (2, 16, 16, 2, 2, 9, 9),
    "e16_e10": (2, 16, 16, 2, 2, 10, 10),
    "o9_e16": (2, 9, 9, 2, 2, 16, 16),
    "e10_e16": (2, 10, 10, 2, 2, 16, 16),
    "e10_e10": (2, 10, 10, 1, 1, 10, 10),
    "e16_e16": (1, 16, 16, 2, 2, 16, 16),
    "o9_o9": (1, 9, 9, 1, 1, 9, 9),
    "rect_up": (2, 12, 10, 2, 2, 16, 14),
    "rect_down": (2, 16, 14, 1, 1, 7, 10),
    "big128_41": (1, 128, 128, 1, 2, 41, 41),
    "big50_128": (1, 50, 50, 1, 1, 128, 128),
    "big128_122": (1, 128, 128, 1, 1, 122, 122),
}


def main():
    gen = torch.Generator().manual_seed(1515)
    out = {"names": np.array(list(CASES))}
    for i, (name, (B, nx, ny, T, C, mx, my)) in enumerate(CASES.items()):
        big = name.startswith("big")
        x = torch.from_numpy(hash_field((B, nx, ny, T, C), i)) if big else torch.randn(B, nx, ny, T, C, generator=gen)
        y64 = resize(x.double(), out_size=[mx, my], temporal=True)
        y32 = resize(x, out_size=[mx, my], temporal=True)
        assert y64.dtype == torch.float64 and y32.dtype == torch.float32 and tuple(y64.shape) == (B, mx, my, T, C)
        if big:
            out[f"{name}.x_salt"], out[f"{name}.x_shape"] = np.int64(i), np.array(x.shape, dtype=np.int64)
        else:
            out[f"{name}.x"] = x.numpy()
        out[f"{name}.out_size"] = np.array([mx, my], dtype=np.int64)
        out[f"{name}.y64"] = y64.numpy().astype(np.float32)
        if not big:
            out[f"{name}.y64d"] = y64.numpy()
        y64f, y32n = out[f"{name}.y64"], y32.contiguous().numpy()
        out[f"{name}.y32ulps"] = y32n.view(np.int32) - y64f.view(np.int32)
        assert np.array_equal(ulps_apply(y64f, out[f"{name}.y32ulps"]).view(np.int32), y32n.view(np.int32))
    # refill_mask: sample 0 has channel 1 empty, sample 1 is full
    msk = torch.ones(2, 6, 6, 1, 3)
    msk[0, :, :, :, 1] = 0.0
    res = 5
    nonzero = (msk.sum(dim=(1, 2, 3)) > 0)[:, None, None, None, :]
    filled = torch.where(nonzero, torch.ones(2, res, res, 1, 3), torch.zeros(2, res, res, 1, 3))
    out["mask.in"], out["mask.res"], out["mask.out"] = msk.numpy(), np.int64(res), filled.numpy()
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.0f} KiB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
