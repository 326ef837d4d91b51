"""Plain numpy restatement of the in-kernel noise generator of csrc/loss_opt.hip (philox_normal4): Philox4x32-10 (Salmon,
Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) followed by the kernel's uniform and Box-Muller
mapping.  Checked against the Random123 known-answer vectors in tests/test_cpu_streaming.py.

    counter = {index lo, index hi, offset lo, offset hi}     key = {seed lo, seed hi}

The uniforms are formed in float32 exactly as the kernel forms them (u0 = float(c0) * 2^-32 + 2^-33, u1 = float(c1) * 2^-32:
the product by a power of two is exact, so the kernel's fused multiply-add rounds once, as the float32 addition here does);
everything after the uniforms is float64, so the hardware's log2 / sin / cos approximations show up as a small difference
and an indexing mistake as an O(1) one.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key schedule (Weyl) increments
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: uint32 [..., 4], key: two 32-bit words -> uint32 [..., 4]"""
    c = np.asarray(counter, dtype=np.uint64) & MASK
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c0                       # 32 x 32 -> 64-bit products (no overflow in uint64)
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniforms(words):
    """uint32 [..., 4] -> float32 (u0, u1, u2, u3) as the kernel forms them: u0, u2 in (0, 1], u1, u3 in [0, 1]"""
    f = words.astype(np.float32)                      # round to nearest even, as v_cvt_f32_u32
    s = np.float32(2.0 ** -32)
    h = np.float32(2.0 ** -33)
    return f[..., 0] * s + h, f[..., 1] * s, f[..., 2] * s + h, f[..., 3] * s


def normal4(seed, offset, index):
    """the four standard normals of counter `index` (array of non-negative ints) -> float64 [..., 4]"""
    index = np.asarray(index, dtype=np.uint64)
    seed, offset = int(seed), int(offset)
    ctr = np.stack([index & np.uint64(MASK), index >> np.uint64(32),
                    np.full(index.shape, offset & MASK, dtype=np.uint64),
                    np.full(index.shape, (offset >> 32) & MASK, dtype=np.uint64)], axis=-1)
    u0, u1, u2, u3 = (u.astype(np.float64) for u in uniforms(philox4x32_10(ctr, (seed & MASK, (seed >> 32) & MASK))))
    r0, r1 = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    a0, a1 = 2.0 * np.pi * u1, 2.0 * np.pi * u3
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)


def field_noise(seed, offset, B, n):
    """eps [B, n] (n = S*C, a multiple of 4) the noise kernels draw for a [B, S, C] field: element i of sample b is component
    i % 4 of counter index b * (n / 4) + i // 4"""
    assert n % 4 == 0
    idx = np.arange(B * (n // 4), dtype=np.uint64)
    return normal4(seed, offset, idx).reshape(B, n)
