"""Shape tables of the streaming-kernel tests (csrc/loss_opt.hip, csrc/misc.hip).

One module, two readers: tests/test_cpu_streaming.py asserts with the library's own planners that every case still reaches
the code path it is here for (a case that silently stops reaching its path is worthless), tests/test_gpu_streaming.py and
tests/test_gpu_misc.py run the kernels on the very same tuples.

A case names the [B, S, C] field the kernel sees and the 5-D window [B,X,Y,T,C] (S = X*Y*T, C' = C) or 6-D window
[B,X,Y,Z,T,C] (S = X*Y*Z, C' = T*C; noise kernels only) that factors to it.  `off` = 1: the tensors start one float into a
larger buffer (4 bytes off a 16-byte boundary), which sends a C == 4 field down the generic path.
"""
from collections import namedtuple

# ---- relative-L2 loss: rel_l2_stats_kernel is one 1024-thread block per (sample, chunk); chunks = cdiv(S*C, 4096) <= 32 -------
RelL2 = namedtuple("RelL2", "name B S C Tt chunks shape off why")
REL_L2 = [
    RelL2("c4_pair_tail", 2, 1029, 4, 3, 2, (2, 7, 49, 3, 4), 0,
          "two chunks of 515 and 514 rows: the pair loop runs once and leaves a 3-point tail; boundaries no multiple of Tt"),
    RelL2("c4_cap32", 1, 32773, 4, 1, 32, (1, 13, 2521, 1, 4), 0, "the 32-chunk cap"),
    RelL2("c4_misaligned", 2, 1029, 4, 3, 2, (2, 7, 49, 3, 4), 1, "C == 4 through the generic path (misalignment fallback)"),
    RelL2("c3", 2, 700, 3, 2, 1, (2, 10, 35, 2, 3), 0, "generic, CP = 4 with one idle channel lane"),
    RelL2("c5", 2, 500, 5, 1, 1, (2, 20, 25, 1, 5), 0, "generic, CP = 8 with three idle channel lanes"),
    RelL2("c1", 3, 257, 1, 1, 1, (3, 257, 1, 1, 1), 0, "generic, CP = 1: 1024 row lanes, a row tail of 257"),
    RelL2("c40", 2, 210, 40, 3, 3, (2, 7, 10, 3, 40), 0, "generic, CP = 64 far from C, three chunks of 70 rows"),
    RelL2("c1024", 1, 130, 1024, 1, 32, (1, 10, 13, 1, 1024), 0,
          "TS == 1 (no reduction tree), 32 chunks of 5 rows of which the last six lie wholly past S"),
]

# ---- noise injection: chan_sumsq_part_kernel / noise_bwd_part_kernel run cdiv(S*C', 8192) <= 64 chunks ---------------------------
Noise = namedtuple("Noise", "name B S C chunks shape off why")
NOISE_FWD = [
    Noise("c4_deep_tail", 2, 2047, 4, 1, (2, 23, 89, 1, 4), 0, "the 4-deep loop (one trip) plus its tail, one chunk"),
    Noise("c4_two_chunks", 2, 2050, 4, 2, (2, 41, 10, 5, 4), 0, "two ragged chunks of 1025 points"),
    Noise("c4_misaligned", 2, 2047, 4, 1, (2, 23, 89, 1, 4), 1, "the generic sum and the scalar axpy at C == 4"),
    Noise("c3", 2, 301, 3, 1, (2, 7, 43, 1, 3), 0, "generic sum, scalar axpy (C % 4 != 0)"),
    Noise("c5", 2, 100, 5, 1, (2, 5, 5, 4, 5), 0, "generic sum, CP = 8, scalar axpy"),
    Noise("c2_odd", 3, 101, 2, 1, (3, 101, 1, 1, 2), 0, "odd S at C == 2: S*C % 4 != 0, sample bases 8 bytes off: scalar fallback"),
    Noise("c8", 2, 64, 8, 1, (2, 4, 4, 4, 2, 4), 0, "float4 eps path, channel index wraps at 8"),
    Noise("c12", 2, 30, 12, 1, (2, 2, 3, 5, 3, 4), 0, "float4 eps path, channel index wraps at 12"),
    Noise("c40", 2, 36, 40, 1, (2, 3, 3, 4, 10, 4), 0, "generic sum, CP = 64 with 24 idle lanes, TS = 4"),
    Noise("c256", 1, 33, 256, 2, (1, 3, 11, 1, 64, 4), 0, "the channel limit: CP = 256, TS == 1, two chunks of 17 and 16 rows"),
]
NOISE_BWD = [
    Noise("c3_cut_point", 2, 2732, 3, 2, (2, 4, 683, 1, 3), 0,
          "two chunks of 4100 flattened elements: the boundary falls inside grid point 1366, so sfirst matters"),
    Noise("c4_two_chunks", 2, 2050, 4, 2, (2, 41, 10, 5, 4), 0, "two chunks at C == 4"),
    Noise("c40", 2, 36, 40, 1, (2, 3, 3, 4, 10, 4), 0, "40 channel passes"),
    Noise("c256", 1, 33, 256, 2, (1, 3, 11, 1, 64, 4), 0, "the channel limit, two chunks"),
]
NOISE_BWD_ZERO = Noise("c8_zero_sample", 2, 64, 8, 1, (2, 4, 4, 4, 2, 4), 0, "one all-zero sample: the nrm > 1e-30 guard")
NOISE_RNG = [
    Noise("c4_single_tail", 2, 2047, 4, 1, (2, 23, 89, 1, 4), 0,
          "C == 4 generator loop: 4 workgroups of 512 float4, the last thread of the last one takes the two == false arm"),
    Noise("c4_three_samples", 3, 520, 4, 1, (3, 8, 13, 5, 4), 0, "three samples; the second workgroup draws one float4 per thread"),
    Noise("c3", 2, 300, 3, 1, (2, 10, 10, 3, 3), 0, "generic generator path, channel index wraps at 3"),
    Noise("c6", 2, 98, 6, 1, (2, 7, 7, 2, 2, 3), 0, "generic generator path (6-D window), channel index wraps at 6"),
]
NOISE_ALL = NOISE_FWD + NOISE_BWD + [NOISE_BWD_ZERO] + NOISE_RNG
NOISE_MAX_C = 256           # the three noise entry points refuse more channels

# ---- column sums: colsum_kernel<16 | 32 | 64> by N; stage-1 parts = min(dpot_colsum_parts(M), cdiv(1024, column blocks)) ------
ColSum = namedtuple("ColSum", "M N parts width")
COLSUM = [
    ColSum(5000, 16, 20, 16), ColSum(5000, 1, 20, 16), ColSum(3001, 17, 12, 32), ColSum(700, 32, 3, 32),
    ColSum(257, 65, 2, 64), ColSum(3, 200, 1, 64),
]
COLSUM_SCATTER = (3001, 30, 12, [(0, 8), (8, 10), (22, 8)])     # M, N, parts, (first column, length): columns 18..21 go nowhere

GROUP_ROWSUM = [(1, 3, 1, 65), (1, 2, 5, 64), (3, 6, 3, 130)]      # (B, R, T, N)
TOKEN_MEAN_T = [1, 3, 28, 29, 33, 61]                               # around the `t + 28 < T` bound of the eight-in-flight loop
TOKEN_MEAN_E = [65, 100]
TOKEN_MEAN_B = 2
SCALE_SHIFT = [(2, 1, 65), (3, 7, 100), (1, 130, 64)]               # (B, T, E)
TIMEAGG = [(1, 64), (3, 300), (4, 257)]                             # (T, E): E > 256 takes a second `j += 256` trip
TRANSPOSE = [(1, 31, 1), (2, 32, 33), (3, 65, 64)]                  # (nbatch, R, C)
PATCHIFY = [(2, 16, 24, 3, 2, 8), (1, 8, 12, 10, 7, 4)]             # (B, X, Y, T, C, P)


def field_dims(shape):
    """(B, S, C') the noise kernels see for a 5-D or 6-D window (dpot_amd.ops.noise_dims, restated for the CPU tests)"""
    B = shape[0]
    C = shape[-1] * (shape[-2] if len(shape) == 6 else 1)
    n = 1
    for d in shape:
        n *= d
    return B, n // (B * C), C
