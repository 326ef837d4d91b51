#!/usr/bin/env python
"""Generate tests/golden/g20_evalmetrics3d.npz from the REFERENCE's Evaluator(temporal=True, griddata=True, component=c)
(utils/criterion.py:189-239, the 3-D branch of compute_fourier_error :295-340).  TEST INFRASTRUCTURE ONLY: the reference is
imported at run time from $DPOT_REFERENCE and nothing of it is copied.

    DPOT_REFERENCE=/path/to/DPOT python scripts/make_golden_evalmetrics3d.py

The reference cannot evaluate a 6-D field with component='all' (its face error views a permuted tensor, which only a
degenerate T = C = 1 field survives; asserted below, so that a later reference that can is noticed, and where 'all' does run
it must agree with the columns).  With component=c - one channel, pred[..., c] - the same code runs, and column c
of every key of the fixture is that call's result, the columns stacked into the shapes the 2-D evaluator returns: nmae..
[1, C], nmae_t.. [1, T, C], bdmse [C, T], fmse_* [T, C].

Per case: `<case>.shape` [B, X, Y, Z, T, C], `<case>.batches` (how the B samples are split into update() calls; the
expectation is always the reference on ALL B samples at once), `<case>.bands` (ilow, ihigh), the inputs (`<case>.pred`,
`<case>.target` float32 for the small cases; the 'hash' cases - the two larger ones, and the two mid-sized near-equal ones to
keep the file small - store only `<case>.salt`, tests/eval3d_ref.hashed_pair restores them bit for bit), and for each of the
ten keys the reference's float64 result (`<case>.<key>.r64`, float64) and its own float32 result (`<case>.<key>.r32`).

The float64 run widens the inputs and also sets torch's default dtype to float64 around the call, for the reason given in
scripts/make_golden_evalmetrics.py: compute_fourier_error allocates its shell buffer in the DEFAULT dtype."""
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
from eval3d_ref import KEYS, hashed_pair  # noqa: E402  (tests/)

OUT = os.path.join(ROOT, "tests", "golden", "g20_evalmetrics3d.npz")
# name: (batches, n_x, n_y, n_z, T, C, ilow, ihigh, kind)   kind: 'indep' = independent fields, 'near' = pred close to target,
#                                                                 'hash' = near, inputs from the integer hash (not stored)
CASES = {
    "o6x5x7_t3c2": ((2,), 6, 5, 7, 3, 2, 1, 2, "indep"),
    "e8_t10c4": ((1,), 8, 8, 8, 10, 4, 1, 3, "near"),
    "r10x12x9_t2c3": ((2,), 10, 12, 9, 2, 3, 1, 3, "indep"),
    "r12x10x8_t1c1": ((1,), 12, 10, 8, 1, 1, 1, 2, "near"),
    "two_batches": ((2, 3), 12, 10, 8, 2, 2, 1, 2, "near"),
    "r20x33x26_t1c2": ((1,), 20, 33, 26, 1, 2, 4, 8, "hash"),
    "e16_default": ((2,), 16, 16, 16, 2, 2, 4, 12, "hash"),
    "big32": ((2,), 32, 32, 32, 2, 2, 4, 12, "hash"),
    "big64": ((1,), 64, 64, 64, 1, 2, 4, 12, "hash"),
}


def per_component(p, t, ilow, ihigh):
    """the ten keys, column c from Evaluator(component=c)"""
    T, C = p.shape[-2], p.shape[-1]
    cols = []
    for c in range(C):
        r = Evaluator(temporal=True, griddata=True, component=c, ilow=ilow, ihigh=ihigh)(p[..., c].contiguous(), t)
        assert set(r) == set(KEYS)
        assert r["nmae"].shape == (1, 1) and r["nmae_t"].shape == (1, T, 1)
        assert r["bdmse"].shape == (T,), r["bdmse"].shape                # one component: no channel axis
        assert r["fmse_low"].shape == r["fmse_mid"].shape == r["fmse_high"].shape == (T, 1)
        cols.append(r)
    out = {k: np.concatenate([r[k] for r in cols], axis=-1) for k in KEYS if k != "bdmse"}
    out["bdmse"] = np.stack([r["bdmse"] for r in cols], axis=0)          # [C, T], channel-major like the 2-D key
    return out


def main():
    gen = torch.Generator().manual_seed(2020)
    out = {"names": np.array(list(CASES))}
    for i, (name, (batches, nx, ny, nz, T, C, ilow, ihigh, kind)) in enumerate(CASES.items()):
        shape = (sum(batches), nx, ny, nz, T, C)
        if kind == "hash":
            p, t = (torch.from_numpy(a) for a in hashed_pair(shape, i))
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
        r32 = per_component(p, t, ilow, ihigh)
        try:
            whole = Evaluator(temporal=True, griddata=True, component="all", ilow=ilow, ihigh=ihigh)(p, t)
        except RuntimeError:
            pass
        else:
            assert T * C == 1, (f"{name}: the reference now evaluates a 6-D field with component='all': compare it with the "
                                "per-component columns and revisit this fixture")
            for key in KEYS:
                assert np.allclose(whole[key].reshape(-1), r32[key].reshape(-1), rtol=1e-5, atol=0.0, equal_nan=True), key
        torch.set_default_dtype(torch.float64)
        try:
            r64 = per_component(p.double(), t.double(), ilow, ihigh)
        finally:
            torch.set_default_dtype(torch.float32)
        for key in KEYS:
            assert r64[key].dtype == np.float64 and r32[key].dtype == np.float32 and r64[key].shape == r32[key].shape
            out[f"{name}.{key}.r64"], out[f"{name}.{key}.r32"] = r64[key], r32[key]
        K = min(nx // 2, ny // 2, nz // 2)
        assert np.isnan(r64["fmse_high"]).all() == (K <= ihigh), name
        assert tuple(r64["bdmse"].shape) == (C, T) and tuple(r64["fmse_low"].shape) == (T, C)
        assert tuple(r64["nmae"].shape) == (1, C) and tuple(r64["nmae_t"].shape) == (1, T, C)
        print(f"{name}: {shape} done", flush=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.0f} KiB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
