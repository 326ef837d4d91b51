"""float64 restatement of the reference's Evaluator(temporal=True, griddata=True, component=c) on 3-D fields (utils/criterion.py:
189-239 with the 3-D branch of compute_fourier_error, :295-340), one column per channel c - the 3-D counterpart of
tests/eval_ref.py: what the GPU tests compare against where the fixture g20_evalmetrics3d has no case.

For pred, target [B, X, Y, Z, T, C] and e = pred - target, per sample b:

    nmae[c]      = sum_{x,y,z,t} |e| / sum_{x,y,z,t} |target|                 nmae_t[t, c]: the same sums over x, y, z only
    nmse[c]      = sqrt(sum e^2 / sum target^2)                               nmse_t[t, c]
    nmxe[c]      = max |e| / max |target|                                     nmxe_t[t, c]
    bd[c, t]     = sqrt((e^2 summed over the faces x = 0, X-1; y = 0, Y-1; z = 0, Z-1, each a whole face: an edge counts
                   twice, a corner three times) / (2 X Y + 2 Y Z + 2 Z X))
    S[c, s, t]   = sum over 0 <= i < X//2, 0 <= j < Y//2, 0 <= k < Z//2 with floor(sqrt(i^2 + j^2 + k^2)) = s < K of
                   |fftn(e)[i, j, k]|^2,  K = min(X//2, Y//2, Z//2)

and over the batch: the mean of each of the first seven, and F[c, s, t] = sqrt(mean_b S) / (X Y Z); the three bands are the
means of F over the shells [0, ilow), [ilow, ihigh), [ihigh, K) (an empty band: NaN).  Shapes as the 2-D evaluator returns
them: nmae.. [1, C], nmae_t.. [1, T, C], bdmse [C, T], fmse_* [T, C].

Vectorised (np.fft.fftn, np.add.at on a shell table built with math.isqrt); it shares no code with dpot_amd.ops."""
import math
import warnings

import numpy as np

KEYS = ("nmae", "nmse", "nmxe", "nmae_t", "nmse_t", "nmxe_t", "bdmse", "fmse_low", "fmse_mid", "fmse_high")
SPECTRUM_KEYS = ("fmse_low", "fmse_mid", "fmse_high")


def shell_table(nx, ny, nz):
    """int64 [nx//2, ny//2, nz//2] of floor(sqrt(i^2 + j^2 + k^2)) in exact integer arithmetic"""
    return np.array([[[math.isqrt(i * i + j * j + k * k) for k in range(nz // 2)] for j in range(ny // 2)]
                     for i in range(nx // 2)], dtype=np.int64).reshape(nx // 2, ny // 2, nz // 2)


def batch_sums(pred, target):
    """the sums over the samples every metric is made of, float64: dict with 'c' [3, C] (nmae | nmse | nmxe), 'tc' [4, T, C]
    (nmae_t | nmse_t | nmxe_t | faces), 'spec' [T, C, K] (shell sums) and 'count'.  Additive over batches."""
    p, t = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    B, nx, ny, nz, T, C = p.shape
    e = p - t
    sp, al = (1, 2, 3), (1, 2, 3, 4)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.stack([(np.abs(e).sum(al) / np.abs(t).sum(al)).sum(0),
                      np.sqrt((e ** 2).sum(al) / (t ** 2).sum(al)).sum(0),
                      (np.abs(e).max(al) / np.abs(t).max(al)).sum(0)])
        e2 = e ** 2
        bd = ((e2[:, 0] + e2[:, -1]).sum((1, 2)) + (e2[:, :, 0] + e2[:, :, -1]).sum((1, 2))
              + (e2[:, :, :, 0] + e2[:, :, :, -1]).sum((1, 2)))                             # [B, T, C]
        tc = np.stack([(np.abs(e).sum(sp) / np.abs(t).sum(sp)).sum(0),
                       np.sqrt(e2.sum(sp) / (t ** 2).sum(sp)).sum(0),
                       (np.abs(e).max(sp) / np.abs(t).max(sp)).sum(0),
                       np.sqrt(bd / (2 * nx * ny + 2 * ny * nz + 2 * nz * nx)).sum(0)])
    K = min(nx // 2, ny // 2, nz // 2)
    sh = shell_table(nx, ny, nz)
    keep = sh < K
    power = np.abs(np.fft.fftn(e, axes=(1, 2, 3))[:, :nx // 2, :ny // 2, :nz // 2]) ** 2     # [B, hx, hy, hz, T, C]
    spec = np.zeros((K, T, C))
    np.add.at(spec, sh[keep], power.sum(0)[keep])
    return {"c": c, "tc": tc, "spec": np.ascontiguousarray(spec.transpose(1, 2, 0)), "count": B}


def add_sums(a, b):
    return {k: a[k] + b[k] for k in a}


def finish(sums, nx, ny, nz, ilow=4, ihigh=12):
    """the Evaluator's dict (float64 arrays) from batch_sums"""
    n = float(sums["count"])
    c, tc = sums["c"] / n, sums["tc"] / n
    F = np.sqrt(sums["spec"] / n) / float(nx * ny * nz)            # [T, C, K]
    out = {"nmae": c[0:1], "nmse": c[1:2], "nmxe": c[2:3], "nmae_t": tc[0:1], "nmse_t": tc[1:2], "nmxe_t": tc[2:3],
           "bdmse": tc[3].T.copy()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        out["fmse_low"] = F[..., :ilow].mean(-1)
        out["fmse_mid"] = F[..., ilow:ihigh].mean(-1)
        out["fmse_high"] = F[..., ihigh:].mean(-1)
    return out


def eval_ref(pred, target, ilow=4, ihigh=12):
    """float64 dict of the ten keys for pred, target [B, X, Y, Z, T, C] (any float dtype)"""
    return finish(batch_sums(pred, target), pred.shape[1], pred.shape[2], pred.shape[3], ilow, ihigh)


def case_fields(fx, name):
    """(pred, target) float32 of a g20_evalmetrics3d case, one pair per batch of the case: stored arrays for the small cases,
    hashed_pair by salt for the two larger ones"""
    shape = tuple(int(s) for s in fx[f"{name}.shape"])
    batches = [int(b) for b in fx[f"{name}.batches"]]
    if f"{name}.pred" in fx.files:
        p, t = fx[f"{name}.pred"], fx[f"{name}.target"]
    else:
        p, t = hashed_pair(shape, int(fx[f"{name}.salt"]))
    out, b0 = [], 0
    for nb in batches:
        out.append((np.ascontiguousarray(p[b0:b0 + nb]), np.ascontiguousarray(t[b0:b0 + nb])))
        b0 += nb
    assert b0 == shape[0]
    return out


def hashed_pair(shape, salt):
    """near-equal inputs without storage (target = smooth + offset + noise, pred = target + a small perturbation - the regime
    where the float32 spectra of two nearly equal fields cancel): every operation is an exactly rounded fp32 (or exact
    integer) one, so the pair is bit-identical wherever it is formed"""
    from resize_ref import hash_field
    B, nx, ny, nz, T, C = shape
    one, two = np.float32(1.0), np.float32(2.0)
    x = (np.arange(nx, dtype=np.float32) / np.float32(nx))[None, :, None, None, None, None]
    y = (np.arange(ny, dtype=np.float32) / np.float32(ny))[None, None, :, None, None, None]
    z = (np.arange(nz, dtype=np.float32) / np.float32(nz))[None, None, None, :, None, None]
    smooth = ((np.float32(4.0) * x * (one - x)) * (one - two * y * (one - y))).astype(np.float32) * (one - z * (one - z))
    target = (hash_field(shape, 2 * salt) * np.float32(0.25) + smooth.astype(np.float32) + np.float32(0.5)).astype(np.float32)
    pred = (target + hash_field(shape, 2 * salt + 1) * np.float32(0.05)).astype(np.float32)
    return pred, target


def independent_pair(shape, salt):
    """two unrelated hashed fields (the target shifted off zero mean)"""
    from resize_ref import hash_field
    return hash_field(shape, 2 * salt), (hash_field(shape, 2 * salt + 1) + np.float32(0.25)).astype(np.float32)
