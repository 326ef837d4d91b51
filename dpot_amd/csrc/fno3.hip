// fno3.hip - the kernels of the 3-D FNO baseline (the reference's models/fno.py: SpectralConv3d and compl_mul3d) on channels-last
// fp32 fields x[B, X, Y, Z, C].  The layer is  y = act( irfftn( W . rfftn(x) restricted to the kept modes ) + add ):
//   kept modes      kx in [0, m1) and [X - m1, X), ky in [0, m2) and [Y - m2, Y), kz in [0, m3): four corner blocks of
//                   m1 x m2 x m3 modes.  The full X x Y x (Z/2+1) spectrum and the reference's zero-filled out_ft never exist.
//   kept spectrum   S[B][2 m1][2 m2][m3][2 = re | im][C]: kept row r is kx = r for r < m1 and kx = X - 2 m1 + r above, the same
//                   rule for q and ky; channels innermost.  The weight block of a kept mode is 1 + (r >= m1) + 2 (q >= m2).
// A (b, x) plane of 16 channels of a 64^3 field is 256 KB: the three axes cannot be contracted in one workgroup's LDS.  Each
// transform is TWO launches around a workspace ws[B][X][2 m2][m3][2][C], (2 m2 / Y)(2 m3 / Z) of the field:
//   dpot_fno3_rfft3   launch 1: every (b, x) plane is a 2-D field [Y, Z, C], and its kept 2-D spectrum [2 m2][m3][2][C] is
//                     exactly a row of ws: the FNO2d forward kernel (fno.hip, dpot_fno_rfft2 over B X "samples" with modes
//                     (m2, m3)) contracts z straight from global memory and y through LDS, with the weights w(kz), the scale
//                     and its XCD-aware workgroup ids.  launch 2 (fno3_axis_kernel) contracts x: a complex DFT of length X onto
//                     the 2 m1 kept rows, per (b, mode (q, kz), channel quad).
//   dpot_fno3_irfft3  launch 1: fno3_axis_kernel expands the kept rows to all X rows (ws), launch 2: the FNO2d inverse kernel
//                     (dpot_fno_irfft2 over the planes) contracts ky and kz, applies w(kz), the scale, + add, pre, activation.
// fno3_axis_kernel  out[b][o][g][.][c] = sum_n in[b][n][g][.][c] e^{sgn i theta(o, n)}: a thread owns (mode g, 4 channels) and
//                   FNO3_RT = 8 output rows (16 accumulators); lanes run over (g, channel quad), which is the memory order: 16
//                   bytes per lane, whole rows coalesced; the twiddles are uniform across the workgroup (scalar loads).  The
//                   workgroups of the other output rows re-read the same input block: one XCD (fno_xcd_item).
// dpot_fno3_mix     O[b, g, o] = sum_i X[b, g, i] W_blk(g)[i, o, g'] (complex) per kept mode, G = 4 m1 m2 m3 modes; lanes run
//                   over the modes and read the weights IN PLACE in the parameter's layout [Cin][Cout][m1][m2][m3][2] (the
//                   view_as_real of the reference's cfloat parameter): one coalesced float2 per lane.  adjoint = 1: the data
//                   gradient, sum over o with conj(W).  The kernel is fno_mix_kernel of fno_common.h, the one FNO2d runs;
//                   FnoWeights3 below is this rank's weight addressing (corner decode, float2).
// dpot_fno3_mix_wgrad  dW[i, o, g'] = sum_b conj(X[b, g, i]) dO[b, g, o], b ascending; written (or added) as float2 into the
//                   four parameters' own layout (fno_mix_wgrad_kernel of fno_common.h).
// Nothing outside the tensors is read: every load past an extent is predicated to 0.0f (table indices are clamped into the
// table), stores are masked.  Fixed summation order, no atomics, no allocation (the caller owns ws).
#include "common.h"
#include "fno_common.h"

namespace dpot {

constexpr int FNO3_MAX_N = 128;       // X, Y, Z: Y is bounded by the LDS intermediate of the plane kernel (Y * 512 bytes)
constexpr int FNO3_MAX_MODES = 32;    // m1, m2, m3: m3 by the LDS intermediate of the inverse plane kernel (m3 * 2 KiB)
constexpr int FNO3_RT = 8;            // axis kernel: output rows per thread

template <bool VEC>
__global__ __launch_bounds__(256) void fno3_axis_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                        const float* __restrict__ t, int B, int Nin, int Nout, int G, int C,
                                                        int ts_out, int ts_in, float sgn) {
  const int CQ = (C + 3) / 4;
  const int nib = (G * CQ + 255) / 256;
  int grp, member;                                   // the row chunks of one (b, item block) re-read its input: one XCD
  if (!fno_xcd_item(blockIdx.x, B * nib, (Nout + FNO3_RT - 1) / FNO3_RT, grp, member)) return;
  const int b = grp / nib, item = (grp % nib) * 256 + threadIdx.x;
  const int g = item / CQ, c = 4 * (item % CQ), nc = C - c;
  if (g >= G) return;
  const int o0 = member * FNO3_RT;
  const float* __restrict__ tj[FNO3_RT];             // clamped into the table; rows past Nout are never stored
#pragma unroll
  for (int j = 0; j < FNO3_RT; ++j) tj[j] = t + (size_t)(o0 + j < Nout ? o0 + j : Nout - 1) * ts_out;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 ar[FNO3_RT], ai[FNO3_RT];
#pragma unroll
  for (int j = 0; j < FNO3_RT; ++j) ar[j] = ai[j] = zero4;
  const size_t row = (size_t)G * 2 * C;
  const float* __restrict__ p = in + (size_t)b * Nin * row + (size_t)g * 2 * C + c;
#pragma unroll 2
  for (int n = 0; n < Nin; ++n) {
    const f32x4 vr = fno_ld4<VEC>(p + (size_t)n * row, nc);
    const f32x4 vi = fno_ld4<VEC>(p + (size_t)n * row + C, nc);
#pragma unroll
    for (int j = 0; j < FNO3_RT; ++j) {
      const float cs = tj[j][(size_t)n * ts_in], sn = sgn * tj[j][(size_t)n * ts_in + 1];
      ar[j] += vr * cs;
      ar[j] -= vi * sn;
      ai[j] += vr * sn;
      ai[j] += vi * cs;
    }
  }
  float* __restrict__ d = out + (size_t)b * Nout * row + (size_t)g * 2 * C + c;
#pragma unroll
  for (int j = 0; j < FNO3_RT; ++j) {
    if (o0 + j < Nout) {
      fno_st4<VEC>(d + (size_t)(o0 + j) * row, ar[j], nc);
      fno_st4<VEC>(d + (size_t)(o0 + j) * row + C, ai[j], nc);
    }
  }
}

// ---- per-mode channel mixing: the weight addressing of fno_mix_kernel / fno_mix_wgrad_kernel (fno_common.h) ---------------------
struct Fno3Modes {
  int m1, m2, m3;
};
// kept mode g of S[2 m1][2 m2][m3] -> its weight block (0..3) and its mode index inside the block's [m1][m2][m3]
__device__ __forceinline__ void fno3_mode(const Fno3Modes m, int g, int& blk, int& gm) {
  const int plane = 2 * m.m2 * m.m3;
  const int r = g / plane, rem = g - r * plane;
  const int q = rem / m.m3, kz = rem - q * m.m3;
  const int hi_r = r >= m.m1, hi_q = q >= m.m2;
  blk = hi_r + 2 * hi_q;
  gm = ((r - hi_r * m.m1) * m.m2 + (q - hi_q * m.m2)) * m.m3 + kz;
}

// G = 4 M kept modes over the four corner parameters [Cin][Cout][M][2]: one complex weight is the float2 (re, im).
// T = const float (weights) or float (their gradients)
template <class T>
struct FnoWeights3 {
  static constexpr int BLOCKS = 4;
  T *w1, *w2, *w3, *w4;
  Fno3Modes md;
  __host__ __device__ int block_modes() const { return md.m1 * md.m2 * md.m3; }
  __device__ __forceinline__ T* at(int g) const {
    int blk, gm;
    fno3_mode(md, g, blk, gm);
    return (blk == 0 ? w1 : blk == 1 ? w2 : blk == 2 ? w3 : w4) + 2 * (size_t)gm;
  }
  __device__ __forceinline__ void load(const float* p, size_t off, float& re, float& im) const {
    const float2 wv = *reinterpret_cast<const float2*>(p + 2 * off);
    re = wv.x;
    im = wv.y;
  }
  __device__ __forceinline__ void store(float* p, size_t off, float re, float im, int accumulate) const {
    float2* d = reinterpret_cast<float2*>(p + 2 * off);
    float2 v = make_float2(re, im);
    if (accumulate) {
      const float2 old = *d;
      v.x = old.x + v.x;
      v.y = old.y + v.y;
    }
    *d = v;
  }
};

static int fno3_check_sizes(const char* what, int B, int X, int Y, int Z, int C, int m1, int m2, int m3) {
  DPOT_REQUIRE(B > 0 && X > 0 && Y > 0 && Z > 0 && C > 0 && m1 > 0 && m2 > 0 && m3 > 0,
               "%s: bad sizes B=%d field %dx%dx%d C=%d modes (%d, %d, %d)", what, B, X, Y, Z, C, m1, m2, m3);
  DPOT_REQUIRE(2 * m1 <= X && 2 * m2 <= Y && m3 <= Z / 2 + 1,
               "%s: modes (%d, %d, %d) do not fit a %dx%dx%d field (2 m1 <= X, 2 m2 <= Y, m3 <= Z/2 + 1)", what, m1, m2, m3, X, Y,
               Z);
  if (X > FNO3_MAX_N || Y > FNO3_MAX_N || Z > FNO3_MAX_N || m1 > FNO3_MAX_MODES || m2 > FNO3_MAX_MODES || m3 > FNO3_MAX_MODES) {
    set_error("%s: field %dx%dx%d with modes (%d, %d, %d) is beyond the kernels' limits (X, Y, Z <= %d, modes <= %d)", what, X, Y,
              Z, m1, m2, m3, FNO3_MAX_N, FNO3_MAX_MODES);
    return DPOT_EUNSUP;
  }
  DPOT_REQUIRE((int64_t)B * X <= 65535 && cdiv(C, 16) <= 65535,
               "%s: B * X = %lld planes or C = %d channels exceed the plane kernels' grid (B * X <= 65535)", what,
               (long long)B * X, C);
  return DPOT_OK;
}

// in[B][Nin][G][2][C] -> out[B][Nout][G][2][C] along the x axis; t = tx[X][2 m1][2]
static int fno3_axis_launch(const char* what, const float* in, float* out, const float* tx, int B, int X, int R, int G, int C,
                            bool forward, dpot_stream_t stream) {
  const int Nin = forward ? X : R, Nout = forward ? R : X;
  const int ts_out = forward ? 2 : 2 * R, ts_in = forward ? 2 * R : 2;
  const int64_t nib = cdiv64((int64_t)G * cdiv(C, 4), 256);
  DPOT_REQUIRE((int64_t)B * nib <= (1 << 24), "%s: too many workgroups", what);
  const int64_t nwg = fno_xcd_grid((int)(B * nib), cdiv(Nout, FNO3_RT));
  DPOT_REQUIRE(nwg <= 0x7fffffff, "%s: too many workgroups", what);
  const bool vec = C % 4 == 0 && aligned16(in) && aligned16(out);
  const float sgn = forward ? -1.f : 1.f;
  if (vec)
    hipLaunchKernelGGL(fno3_axis_kernel<true>, dim3((unsigned)nwg), dim3(256), 0, as_stream(stream), in, out, tx, B, Nin, Nout, G,
                       C, ts_out, ts_in, sgn);
  else
    hipLaunchKernelGGL(fno3_axis_kernel<false>, dim3((unsigned)nwg), dim3(256), 0, as_stream(stream), in, out, tx, B, Nin, Nout,
                       G, C, ts_out, ts_in, sgn);
  return check_launch("fno3_axis_kernel");
}

static int fno3_mix_check(const char* what, int B, int Cin, int Cout, int m1, int m2, int m3) {
  DPOT_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && m1 > 0 && m2 > 0 && m3 > 0 && (int64_t)m1 * m2 * m3 <= (1 << 22),
               "%s: bad sizes B=%d Cin=%d Cout=%d modes (%d, %d, %d)", what, B, Cin, Cout, m1, m2, m3);
  return DPOT_OK;
}
static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace dpot

using namespace dpot;

extern "C" int dpot_fno3_max_size(int modes) { return modes ? FNO3_MAX_MODES : FNO3_MAX_N; }

extern "C" int64_t dpot_fno3_ws_elems(int B, int X, int C, int m2, int m3) {
  if (B <= 0 || X <= 0 || C <= 0 || m2 <= 0 || m3 <= 0) return 0;
  return (int64_t)B * X * 2 * m2 * m3 * 2 * C;
}

extern "C" int dpot_fno3_rfft3(const float* x, float* S, float* ws, const float* tx, const float* ty, const float* tz, int B,
                               int X, int Y, int Z, int C, int m1, int m2, int m3, int col_weights, float scale,
                               dpot_stream_t stream) {
  DPOT_REQUIRE(x && S && ws && tx && ty && tz && x != S && x != ws && S != ws, "fno3_rfft3: null or aliased pointer");
  if (int rc = fno3_check_sizes("fno3_rfft3", B, X, Y, Z, C, m1, m2, m3)) return rc;
  if (int rc = dpot_fno_rfft2(x, ws, ty, tz, B * X, Y, Z, C, m2, m3, col_weights, scale, stream)) return rc;
  return fno3_axis_launch("fno3_rfft3", ws, S, tx, B, X, 2 * m1, 2 * m2 * m3, C, true, stream);
}

extern "C" int dpot_fno3_irfft3(const float* S, const float* add, float* y, float* pre, float* ws, const float* tx,
                                const float* ty, const float* tz, int B, int X, int Y, int Z, int C, int m1, int m2, int m3,
                                int col_weights, float scale, int act, dpot_stream_t stream) {
  DPOT_REQUIRE(S && y && ws && tx && ty && tz && S != y && S != ws && y != ws && y != pre, "fno3_irfft3: null or aliased pointer");
  DPOT_REQUIRE(act >= DPOT_ACT_NONE && act <= DPOT_ACT_SILU, "fno3_irfft3: unknown activation %d", act);
  if (int rc = fno3_check_sizes("fno3_irfft3", B, X, Y, Z, C, m1, m2, m3)) return rc;
  if (int rc = fno3_axis_launch("fno3_irfft3", S, ws, tx, B, X, 2 * m1, 2 * m2 * m3, C, false, stream)) return rc;
  return dpot_fno_irfft2(ws, add, y, pre, ty, tz, B * X, Y, Z, C, m2, m3, col_weights, scale, act, stream);
}

extern "C" int dpot_fno3_mix(const float* X, const float* w1, const float* w2, const float* w3, const float* w4, float* O, int B,
                             int Cin, int Cout, int m1, int m2, int m3, int adjoint, dpot_stream_t stream) {
  DPOT_REQUIRE(X && w1 && w2 && w3 && w4 && O && X != O, "fno3_mix: null or aliased pointer");
  DPOT_REQUIRE(aligned8(w1) && aligned8(w2) && aligned8(w3) && aligned8(w4), "fno3_mix: the weights must be 8-byte aligned");
  if (int rc = fno3_mix_check("fno3_mix", B, Cin, Cout, m1, m2, m3)) return rc;
  const FnoWeights3<const float> w = {w1, w2, w3, w4, {m1, m2, m3}};
  return fno_mix_launch("fno3_mix", "fno3_mix_kernel", X, w, O, B, Cin, Cout, adjoint, stream);
}

extern "C" int dpot_fno3_mix_wgrad(const float* X, const float* dO, float* dw1, float* dw2, float* dw3, float* dw4, int B,
                                   int Cin, int Cout, int m1, int m2, int m3, int accumulate, dpot_stream_t stream) {
  DPOT_REQUIRE(X && dO && dw1 && dw2 && dw3 && dw4 && dw1 != dw2 && dw1 != dw3 && dw1 != dw4 && dw2 != dw3 && dw2 != dw4 &&
                   dw3 != dw4,
               "fno3_mix_wgrad: null or aliased pointer");
  DPOT_REQUIRE(aligned8(dw1) && aligned8(dw2) && aligned8(dw3) && aligned8(dw4),
               "fno3_mix_wgrad: the gradients must be 8-byte aligned");
  if (int rc = fno3_mix_check("fno3_mix_wgrad", B, Cin, Cout, m1, m2, m3)) return rc;
  const FnoWeights3<float> dw = {dw1, dw2, dw3, dw4, {m1, m2, m3}};
  return fno_mix_wgrad_launch("fno3_mix_wgrad", "fno3_mix_wgrad_kernel", X, dO, dw, B, Cin, Cout, accumulate, stream);
}
