"""Case table of the 2-D DFT kernel tests (csrc/dft_fast.h, csrc/dft.hip).

One module, two readers: tests/test_cpu_dft.py asserts with the library's own selection (dpot_dft2_kernel_kind) that every
case still reaches the kernel it is here for and that the table reaches every kernel that is compiled
(dpot_dft2_kernel_kinds); tests/test_gpu_dft.py runs the kernels on the very same tuples.

A case is (B, h, w, E, nb, mx, my, kind_fwd, kind_inv): x[B, h*w, E] in nb channel blocks, kept modes kx < mx, ky < my, and
the kind rfft2 / irfft2 must run for it: H * 1000 + CC for the register FFT of the H x H grid with CC-channel chunks, 0 for
the generic direct sums, -1 for a refusal.  The kinds written here are read off the selection rules by hand:
    16 x 16, 8 x 8   CC 64 when E % 64 == 0 and B * (E / 64) >= 512, else CC 32 when E % 32 == 0
    32 x 32 forward  CC 32 when E % 32 == 0 and B * (E / 32) >= 512; else CC 12 when E % 12 == 0, (E / nb) % 12 == 0 and
                     B * (E / 12) >= 256; else CC 32 when E % 32 == 0 and B * (E / 32) >= 128; else CC 16 when E % 16 == 0
    32 x 32 inverse  the CC 12 rule, else CC 16 when E % 16 == 0 (there is no 32-channel inverse)
    64 x 64          CC 8 when E % 8 == 0
    24 x 24          CC 32 when E % 32 == 0, else CC 8 when E % 8 == 0
    48 x 48          CC 16 when E % 16 == 0, else CC 4 when E % 4 == 0;        96 x 96: CC 4 when E % 4 == 0
    128 x 128        CC 4 when E % 4 == 0 and my <= 36, else CC 2 when E % 2 == 0
    anything else    generic, with the widest power-of-two chunk <= 64 that divides E and fits 150 KiB of LDS; none fits: -1
"""
from collections import namedtuple

Case = namedtuple("Case", "B h w E nb mx my kind_fwd kind_inv")


def case_id(c):
    return f"{c.h}x{c.w}-B{c.B}-E{c.E}-nb{c.nb}-m{c.mx}x{c.my}"


def mode_sets(h, w):
    """what every register kind is run with: all modes; the DC mode alone; an odd, asymmetric truncation; and every column
    but the Nyquist one of a three-row band"""
    return [(h, w // 2 + 1), (1, 1), (h // 2 + 1, 3), (3, w // 2)]


def _each_mode(B, n, E, nb, kf, ki):
    return [Case(B, n, n, E, nb, mx, my, kf, ki) for mx, my in mode_sets(n, n)]


CASES = []

# ---- 16 x 16 --------------------------------------------------------------------------------------------------------
CASES += _each_mode(2, 16, 32, 1, 16032, 16032)                  # one chunk, one block
CASES += [Case(2, 16, 16, 64, 4, 16, 9, 16032, 16032),           # blocks of 16 channels inside a 32-channel chunk
          Case(3, 16, 16, 256, 2, 9, 3, 16032, 16032),           # 8 chunks: the XCD remap of the chunk index
          Case(511, 16, 16, 64, 1, 16, 9, 16032, 16032),         # B * (E / 64) = 511: one short of the 64-channel kernel
          Case(512, 16, 16, 64, 1, 16, 9, 16064, 16064),         # ... = 512: DPOT-S / -M at batch 32 run this kernel
          Case(64, 16, 16, 512, 4, 16, 9, 16064, 16064)]         # 8 chunks of 64: the XCD remap, blocks of 128
CASES += [Case(512, 16, 16, 64, 4, mx, my, 16064, 16064)         # blocks of 16 channels inside the 64-channel chunk
          for mx, my in mode_sets(16, 16)[1:]]
# ---- 8 x 8 ----------------------------------------------------------------------------------------------------------
CASES += _each_mode(2, 8, 32, 1, 8032, 8032)
CASES += [Case(2, 8, 8, 64, 4, 8, 5, 8032, 8032),
          Case(511, 8, 8, 64, 1, 8, 5, 8032, 8032),
          Case(512, 8, 8, 64, 1, 8, 5, 8064, 8064),
          Case(64, 8, 8, 512, 4, 8, 5, 8064, 8064)]
CASES += [Case(512, 8, 8, 64, 4, mx, my, 8064, 8064) for mx, my in mode_sets(8, 8)[1:]]
# ---- 32 x 32 --------------------------------------------------------------------------------------------------------
CASES += _each_mode(2, 32, 16, 1, 32016, 32016)
CASES += [Case(2, 32, 32, 32, 4, 32, 17, 32016, 32016),          # blocks of 8 channels inside a 16-channel chunk
          Case(127, 32, 32, 32, 1, 32, 17, 32016, 32016),        # B * (E / 32) = 127
          Case(128, 32, 32, 32, 1, 32, 17, 32032, 32016),        # ... = 128: 32-channel chunks, forward only
          Case(128, 32, 32, 32, 4, 1, 1, 32032, 32016),          # blocks of 8 channels inside the 32-channel chunk
          Case(128, 32, 32, 32, 1, 17, 3, 32032, 32016),
          Case(128, 32, 32, 32, 1, 3, 16, 32032, 32016),
          Case(511, 32, 32, 32, 1, 32, 17, 32032, 32016),        # the >= 512 rule picks the same kernel for E = 32 ...
          Case(512, 32, 32, 32, 1, 32, 17, 32032, 32016),
          Case(170, 32, 32, 96, 2, 32, 17, 32012, 32012),        # ... so E = 96: B * 3 = 510 leaves the CC 12 rule in front
          Case(171, 32, 32, 96, 2, 32, 17, 32032, 32012),        # B * 3 = 513: the >= 512 rule goes first
          Case(42, 32, 32, 96, 3, 32, 17, 32016, 32016),         # blocks of 32 (no CC 12), B * 3 = 126
          Case(43, 32, 32, 96, 3, 32, 17, 32032, 32016),         # B * 3 = 129
          Case(63, 32, 32, 48, 1, 32, 17, 32016, 32016),         # B * (E / 12) = 252, the nearest below 256 with E % 16 == 0
          Case(64, 32, 32, 48, 1, 32, 17, 32012, 32012),         # ... = 256
          Case(64, 32, 32, 48, 3, 32, 17, 32016, 32016),         # ... = 256 with blocks of 16: (E / nb) % 12 != 0
          Case(255, 32, 32, 12, 1, 32, 17, 0, 0),                # B * (E / 12) = 255 exactly: E = 12 has no other register kernel
          Case(256, 32, 32, 12, 1, 32, 17, 32012, 32012)]
CASES += [Case(128, 32, 32, 24, 2, mx, my, 32012, 32012) for mx, my in mode_sets(32, 32)[1:]]   # two blocks of 12
# ---- 64 x 64 --------------------------------------------------------------------------------------------------------
CASES += _each_mode(2, 64, 8, 1, 64008, 64008)
CASES += [Case(2, 64, 64, 16, 4, 64, 33, 64008, 64008)]          # blocks of 4 channels inside an 8-channel chunk
# ---- 3 * 2^k grids --------------------------------------------------------------------------------------------------
CASES += _each_mode(2, 24, 32, 1, 24032, 24032)
CASES += [Case(2, 24, 24, 64, 8, 24, 13, 24032, 24032)]
CASES += _each_mode(2, 24, 8, 1, 24008, 24008)
CASES += [Case(2, 24, 24, 24, 6, 24, 13, 24008, 24008)]
CASES += _each_mode(2, 48, 16, 1, 48016, 48016)
CASES += [Case(2, 48, 48, 32, 4, 48, 25, 48016, 48016)]
CASES += _each_mode(2, 48, 4, 1, 48004, 48004)
CASES += [Case(2, 48, 48, 12, 6, 48, 25, 48004, 48004)]
CASES += _each_mode(1, 96, 4, 1, 96004, 96004)
CASES += [Case(1, 96, 96, 8, 4, 96, 49, 96004, 96004)]
# ---- 128 x 128: 4-channel chunks keep at most 36 columns, so their "all modes" is (128, 36) and their widest band (3, 36) ----
CASES += [Case(1, 128, 128, 4, 1, 128, 36, 128004, 128004),
          Case(1, 128, 128, 4, 1, 1, 1, 128004, 128004),
          Case(1, 128, 128, 4, 1, 65, 3, 128004, 128004),
          Case(1, 128, 128, 4, 1, 3, 36, 128004, 128004),
          Case(1, 128, 128, 4, 2, 21, 36, 128004, 128004),       # blocks of 2 channels inside the 4-channel chunk, odd mx
          Case(1, 128, 128, 8, 1, 97, 1, 128004, 128004),        # 64 < mx < 128, one column
          Case(1, 128, 128, 4, 1, 65, 37, 128002, 128002),       # my = 37: one column too many for 4 channels
          Case(1, 128, 128, 4, 1, 128, 65, 128002, 128002)]
CASES += _each_mode(1, 128, 6, 3, 128002, 128002)                # E % 4 != 0
CASES += [Case(1, 128, 128, 6, 1, 97, 65, 128002, 128002),
          Case(1, 128, 128, 6, 1, 21, 1, 128002, 128002),
          Case(1, 128, 128, 2, 2, 65, 36, 128002, 128002)]       # blocks of 1 channel inside the 2-channel chunk
# ---- generic direct sums: non-square, degenerate and odd grids; E = 7 / 24 / 64 make the chunk 1 / 8 / 64 channels wide ----------
GENERIC_GRIDS = [(5, 7), (7, 5), (12, 20), (20, 12), (1, 8), (8, 1), (14, 14)]
for _h, _w in GENERIC_GRIDS:
    for _E in (7, 24, 64):
        CASES += [Case(2, _h, _w, _E, 1, _h, _w // 2 + 1, 0, 0),
                  Case(3, _h, _w, _E, _E, (_h + 1) // 2, max(1, _w // 4), 0, 0)]
CASES += [Case(2, 16, 16, 24, 3, 16, 9, 0, 0),                   # register grids whose E no chunk width divides
          Case(2, 32, 32, 8, 1, 17, 3, 0, 0)]
# ---- refused: the generic slab of one channel is larger than the LDS budget --------------------------------------------
CASES += [Case(1, 200, 200, 1, 1, 200, 101, -1, -1)]

RUNNABLE = [c for c in CASES if c.kind_fwd >= 0 and c.kind_inv >= 0]
REFUSED = [c for c in CASES if c.kind_fwd < 0 or c.kind_inv < 0]

# GroupNorm on the load (dpot_rfft2_norm / dpot_irfft2_norm): (case, G) with E / G a multiple of 4 - every grid the norm forms
# admit, every chunk width of it
NORM_CASES = [(Case(2, 8, 8, 32, 1, 8, 5, 8032, 8032), 8),
              (Case(512, 8, 8, 64, 4, 5, 3, 8064, 8064), 8),
              (Case(3, 16, 16, 64, 4, 16, 9, 16032, 16032), 8),
              (Case(64, 16, 16, 512, 4, 16, 9, 16064, 16064), 8),
              (Case(2, 32, 32, 16, 1, 32, 17, 32016, 32016), 2),
              (Case(64, 32, 32, 48, 1, 17, 3, 32012, 32012), 4),
              (Case(128, 32, 32, 32, 4, 32, 17, 32032, 32016), 8),
              (Case(2, 64, 64, 8, 2, 64, 33, 64008, 64008), 2)]
# norm = 1 where no kernel applies the GroupNorm on its load: (case, G); the kinds are those of the plain call
NORM_REFUSED = [(Case(2, 24, 24, 32, 1, 24, 13, 24032, 24032), 8),
                (Case(1, 128, 128, 8, 1, 128, 36, 128004, 128004), 2),
                (Case(2, 16, 32, 32, 1, 16, 17, 0, 0), 8)]
