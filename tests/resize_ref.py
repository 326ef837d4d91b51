"""float64 restatement of the Fourier resize (utils/utilities.py:277-305) from its closed form, the counterpart of
tests/lamb_ref.py: what the GPU tests compare against where the fixture g15_resize has no case.

Per plane, n_x x n_y -> m_x x m_y:

    out[x', y'] = 1 / (n_x n_y) * sum_{x, y} in[x, y] * Re( Dx[x', x] * Dy[y', y] )
    Dx[x', x] = sum_{k in Kx} exp(2 pi i k (x'/m_x - x/n_x)),   Kx = {0 .. t1-1} u {-b1 .. -1}
                t1 = min((n_x+1)//2, (m_x+1)//2),  b1 = min(n_x//2, m_x//2)
    Dy[y', y] = sum_{k = 0 .. t2-1} c_k exp(2 pi i k (y'/m_y - y/n_y)),  t2 = min(n_y//2 + 1, m_y//2 + 1)
                c_k = 1 for k = 0 and for 2k = m_y, else 2

Written as the dense complex operator and one einsum; it shares no code with dpot_amd.ops.spectral_resize_matrices."""
import numpy as np


def axis_operator(n, m, half):
    """complex128 [m, n]: Dy (half=True) or Dx (half=False)"""
    if half:
        ks = list(range(min(n // 2 + 1, m // 2 + 1)))
        cs = [1.0 if (k == 0 or 2 * k == m) else 2.0 for k in ks]
    else:
        ks = list(range(min((n + 1) // 2, (m + 1) // 2))) + list(range(-min(n // 2, m // 2), 0))
        cs = [1.0] * len(ks)
    jo = np.arange(m, dtype=np.float64)[:, None] / m
    ji = np.arange(n, dtype=np.float64)[None, :] / n
    D = np.zeros((m, n), dtype=np.complex128)
    for k, c in zip(ks, cs):
        D += c * np.exp(2j * np.pi * k * (jo - ji))
    return D


def resize_ref(x, out_size):
    """x [B, n_x, n_y, ...planes] (any float dtype) -> float64 [B, m_x, m_y, ...planes]"""
    x = np.asarray(x, dtype=np.float64)
    mx, my = (out_size, out_size) if isinstance(out_size, int) else out_size
    B, nx, ny = x.shape[:3]
    Dx, Dy = axis_operator(nx, mx, False), axis_operator(ny, my, True)
    flat = x.reshape(B, nx, ny, -1)
    out = np.einsum("ux,vy,bxyp->buvp", Dx, Dy, flat.astype(np.complex128), optimize=True).real / (nx * ny)
    return out.reshape((B, mx, my) + x.shape[3:])


def hash_field(shape, salt):
    """float32 field in [-1.5, 1.5) from an integer hash of the element index (the 64-bit finaliser of MurmurHash3, exact
    integer arithmetic, then a division by 2^32): bit-identical wherever it is evaluated, so the evaluation-sized cases of
    g15_resize need not store their inputs"""
    n = int(np.prod(shape))
    m64 = np.uint64(0xFFFFFFFFFFFFFFFF)
    h = np.arange(n, dtype=np.uint64) + np.uint64((0x9E3779B97F4A7C15 * (int(salt) + 1)) & 0xFFFFFFFFFFFFFFFF)   # wraps
    for mul in (0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53):
        h ^= h >> np.uint64(33)
        h = (h * np.uint64(mul)) & m64
    h ^= h >> np.uint64(33)
    u = (h >> np.uint64(32)).astype(np.float64) / 4294967296.0
    return ((u - 0.5) * 3.0).astype(np.float32).reshape(shape)


def ulps_apply(base, d):
    """the float32 array that lies d (int32) bit patterns away from float32 `base`: how g15_resize stores the reference's
    float32 result next to its float64 one"""
    return (np.ascontiguousarray(base, dtype=np.float32).view(np.int32) + d.astype(np.int32)).view(np.float32)


def refill_mask_ref(msk, res):
    """evaluate_varyingres.py:198-201: a channel of a sample is 1 everywhere if the mask has any non-zero in it, else 0"""
    msk = np.asarray(msk)
    rx, ry = (res, res) if isinstance(res, int) else res
    nz = (msk.sum(axis=(1, 2, 3)) > 0)[:, None, None, None, :]
    return np.where(nz, np.ones((msk.shape[0], rx, ry, 1, msk.shape[-1]), dtype=np.float32),
                    np.zeros((msk.shape[0], rx, ry, 1, msk.shape[-1]), dtype=np.float32))
