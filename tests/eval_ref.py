"""float64 restatement of the reference's Evaluator(temporal=True, griddata=True, component='all') (utils/criterion.py:
189-239 with compute_fourier_error, :246-360), the counterpart of tests/resize_ref.py: what the GPU tests compare against
where the fixture g16_evalmetrics has no case.

For pred, target [B, X, Y, T, C] and e = pred - target, per sample b:

    nmae[c]      = sum_{x,y,t} |e| / sum_{x,y,t} |target|                     nmae_t[t, c]: the same sums over x, y only
    nmse[c]      = sqrt(sum e^2 / sum target^2)                               nmse_t[t, c]
    nmxe[c]      = max |e| / max |target|                                     nmxe_t[t, c]
    bd[c, t]     = sqrt((sum_y e[0,y]^2 + e[X-1,y]^2 + sum_x e[x,0]^2 + e[x,Y-1]^2) / (2 X + 2 Y))
    S[c, s, t]   = sum over 0 <= i < X//2, 0 <= j < Y//2 with floor(sqrt(i^2 + j^2)) = s < K of |fft2(e)[i, j]|^2,  K = min(X//2, Y//2)

and over the batch: the mean of each of the first seven, and F[c, s, t] = sqrt(mean_b S) / (X Y); the three bands are the
means of F over the shells [0, ilow), [ilow, ihigh), [ihigh, K) (an empty band: NaN).  Shapes as the reference returns them:
nmae.. [1, C], nmae_t.. [1, T, C], bdmse [C, T], fmse_* [T, C].

Vectorised (np.fft.fft2, np.add.at on a shell table built with math.isqrt); it shares no code with dpot_amd.ops."""
import math
import warnings

import numpy as np

KEYS = ("nmae", "nmse", "nmxe", "nmae_t", "nmse_t", "nmxe_t", "bdmse", "fmse_low", "fmse_mid", "fmse_high")
SPECTRUM_KEYS = ("fmse_low", "fmse_mid", "fmse_high")


def shell_table(nx, ny):
    """int64 [nx//2, ny//2] of floor(sqrt(i^2 + j^2)) in exact integer arithmetic"""
    return np.array([[math.isqrt(i * i + j * j) for j in range(ny // 2)] for i in range(nx // 2)], dtype=np.int64)


def batch_sums(pred, target):
    """the sums over the samples every metric is made of, float64: dict with 'c' [3, C] (nmae | nmse | nmxe), 'tc' [4, T, C]
    (nmae_t | nmse_t | nmxe_t | boundary), 'spec' [T, C, K] (shell sums) and 'count'.  Additive over batches."""
    p, t = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    B, nx, ny, T, C = p.shape
    e = p - t
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.stack([(np.abs(e).sum((1, 2, 3)) / np.abs(t).sum((1, 2, 3))).sum(0),
                      np.sqrt((e ** 2).sum((1, 2, 3)) / (t ** 2).sum((1, 2, 3))).sum(0),
                      (np.abs(e).max((1, 2, 3)) / np.abs(t).max((1, 2, 3))).sum(0)])
        e2 = e ** 2
        bd = (e2[:, 0] + e2[:, -1]).sum(1) + (e2[:, :, 0] + e2[:, :, -1]).sum(1)           # [B, T, C]
        tc = np.stack([(np.abs(e).sum((1, 2)) / np.abs(t).sum((1, 2))).sum(0),
                       np.sqrt(e2.sum((1, 2)) / (t ** 2).sum((1, 2))).sum(0),
                       (np.abs(e).max((1, 2)) / np.abs(t).max((1, 2))).sum(0),
                       np.sqrt(bd / (2 * nx + 2 * ny)).sum(0)])
    K = min(nx // 2, ny // 2)
    sh = shell_table(nx, ny)
    keep = sh < K
    power = np.abs(np.fft.fft2(e, axes=(1, 2))[:, :nx // 2, :ny // 2]) ** 2                 # [B, hx, hy, T, C]
    spec = np.zeros((K, T, C))
    np.add.at(spec, sh[keep], power.sum(0)[keep])
    return {"c": c, "tc": tc, "spec": np.ascontiguousarray(spec.transpose(1, 2, 0)), "count": B}


def add_sums(a, b):
    return {k: a[k] + b[k] for k in a}


def finish(sums, nx, ny, ilow=4, ihigh=12):
    """the Evaluator's dict (float64 arrays) from batch_sums"""
    n = float(sums["count"])
    c, tc = sums["c"] / n, sums["tc"] / n
    F = np.sqrt(sums["spec"] / n) / float(nx * ny)                 # [T, C, K]
    out = {"nmae": c[0:1], "nmse": c[1:2], "nmxe": c[2:3], "nmae_t": tc[0:1], "nmse_t": tc[1:2], "nmxe_t": tc[2:3],
           "bdmse": tc[3].T.copy()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        out["fmse_low"] = F[..., :ilow].mean(-1)
        out["fmse_mid"] = F[..., ilow:ihigh].mean(-1)
        out["fmse_high"] = F[..., ihigh:].mean(-1)
    return out


def eval_ref(pred, target, ilow=4, ihigh=12):
    """float64 dict of the ten keys for pred, target [B, X, Y, T, C] (any float dtype)"""
    return finish(batch_sums(pred, target), pred.shape[1], pred.shape[2], ilow, ihigh)


def case_fields(fx, name):
    """(pred, target) float32 of a g16_evalmetrics case, one pair per batch of the case: stored arrays for the small cases,
    resize_ref.hash_field by salt for the evaluation-sized ones (target = smooth + offset + noise, pred = target + a small
    perturbation - the regime where the float32 spectra of two nearly equal fields cancel)"""
    from resize_ref import hash_field
    shape = tuple(int(s) for s in fx[f"{name}.shape"])
    batches = [int(b) for b in fx[f"{name}.batches"]]
    if f"{name}.pred" in fx.files:
        p, t = fx[f"{name}.pred"], fx[f"{name}.target"]
    else:
        salt = int(fx[f"{name}.salt"])
        p, t = hashed_pair(shape, salt, hash_field)
    out, b0 = [], 0
    for nb in batches:
        out.append((np.ascontiguousarray(p[b0:b0 + nb]), np.ascontiguousarray(t[b0:b0 + nb])))
        b0 += nb
    assert b0 == shape[0]
    return out


def hashed_pair(shape, salt, hash_field):
    """the evaluation-sized inputs: every operation is an exactly rounded fp32 (or exact integer) one, so the pair is
    bit-identical wherever it is formed"""
    B, nx, ny, T, C = shape
    x = (np.arange(nx, dtype=np.float32) / np.float32(nx))[None, :, None, None, None]
    y = (np.arange(ny, dtype=np.float32) / np.float32(ny))[None, None, :, None, None]
    smooth = (np.float32(4.0) * x * (np.float32(1.0) - x)) * (np.float32(1.0) - np.float32(2.0) * y * (np.float32(1.0) - y))
    target = (hash_field(shape, 2 * salt) * np.float32(0.25) + smooth.astype(np.float32) + np.float32(0.5)).astype(np.float32)
    pred = (target + hash_field(shape, 2 * salt + 1) * np.float32(0.05)).astype(np.float32)
    return pred, target
