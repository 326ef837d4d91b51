// fno.hip - the kernels of the FNO baseline (the reference's models/fno.py: SpectralConv2d_fast and compl_mul2d) on
// channels-last fp32 fields x[B, H, W, C].  The layer is  y = act( irfft2( W . rfft2(x) restricted to the kept modes ) + add ):
//   kept modes      rows kx in [0, m1) and [H - m1, H), columns ky in [0, m2): 2 m1 rows x m2 columns.  The full H x (W/2+1)
//                   spectrum and the reference's zero-filled out_ft never exist.
//   kept spectrum   S[B][R = 2 m1][m2][2 = re | im][C]: kept row r is kx = r for r < m1 and kx = H - 2 m1 + r above; channels
//                   innermost, so the transforms read and write 16 bytes per lane and the mixing reads a lane's channels in order.
// Twiddle tables (built in float64 on the host with the angle reduced in integers, dpot_amd/ops.py FNOPlan; plain device pointers):
//   tx[H][R][2] = cos | sin of 2 pi kx(r) x / H,       ty[W][m2][2] = cos | sin of 2 pi ky y / W.
//
// dpot_fno_rfft2   S = s w(ky) sum_{x,y} x e^{-i(..)}.  Workgroup = (b, 4 columns ky, 16 channels), 512 threads.
//                  pass 1 contracts y: a thread owns (row x, 4 channels), keeps the 4 columns x (re, im) x 4 channels in 32
//                  accumulators and reads the field once per workgroup (16 bytes per lane, 64 bytes per row and lane group); the
//                  twiddles are uniform across the workgroup (scalar loads).  The H x 4 x 2 x 16 intermediate lives in LDS.
//                  pass 2 contracts x: a thread owns (kept row r < m1 AND its partner r + m1, column, 4 channels): one pair of
//                  16-byte LDS reads feeds both rows.  The cut is along ky, the free axis of both passes: nothing is recomputed.
// dpot_fno_irfft2  y = act( Re sum_{r,ky} s w(ky) S e^{+i(..)} + add ).  Workgroup = (b, 16 rows x, 16 channels).
//                  pass 1 contracts the kept rows: U[x][ky] (complex, weight and scale applied) into LDS, a thread owns
//                  (column, 4 channels, rows xi and xi + 8) so one pair of spectrum loads feeds two rows.
//                  pass 2 contracts ky: a wave owns 4 columns y at a time (uniform: scalar twiddle loads), its lanes are the
//                  16 rows x 4 channel quads; one pair of LDS reads feeds the 4 columns.  The LDS row stride is 16 floats off a
//                  multiple of 32, which spreads the 16 lanes of a 16-byte read over all banks.  Epilogue: + add, pre, act.
// With weights off and scale 1 each transform is the exact adjoint of the other (the same tables, the conjugate sign).
// dpot_fno_mix     O[b, g, o] = sum_i X[b, g, i] W[i, o, g] (complex) per kept mode g; lanes run over the modes, so the weights
//                  - the dominant bytes, mode index innermost in the parameter - are read coalesced IN PLACE: no packed copy.
//                  A thread keeps 4 samples x 4 outputs (32 accumulators).  adjoint = 1: the data gradient, sum over o with
//                  conj(W[i, o]).  The kernel is fno_mix_kernel of fno_common.h, which FNO3d runs too; FnoWeights2 below is
//                  this rank's weight addressing.
// dpot_fno_mix_wgrad  dW[i, o, g] = sum_b conj(X[b, g, i]) dO[b, g, o], b ascending, a thread keeps a 4 x 4 (i, o) tile of one
//                  mode; written (or added) coalesced in the parameter's own layout [2][Cin][Cout][m1][m2]
//                  (fno_mix_wgrad_kernel of fno_common.h).
// dpot_fno_dact    dpre = dy act'(pre), elementwise.
// Nothing outside the tensors is read: every load past H, W, C, m2 or B is predicated to 0.0f (table indices are clamped into
// the table), stores are masked.  Fixed summation order (one fma chain per output), no atomics, no allocation.
#include "common.h"
#include "dft_common.h"
#include "fno_common.h"

namespace dpot {

constexpr int FNO_MAX_N = 256;        // H, W
constexpr int FNO_MAX_MODES = 64;     // m1, m2
constexpr int FNO_CC = 16;            // channels per workgroup of the transforms
constexpr int FNO_KYC = 4;            // rfft2: columns ky per workgroup
constexpr int FNO_XS = 16;            // irfft2: rows x per workgroup
constexpr int FNO_NT = 256;           // threads of irfft2
constexpr int FNO_NTF = 512;          // threads of rfft2: one sweep of the (row, channel quad) items of a 128-row field

struct FnoArgs {
  const float* x;      // field in (rfft2)
  float* S;            // kept spectrum (rfft2: out, irfft2: in)
  const float* tx;
  const float* ty;
  const float* add;    // irfft2, optional
  float* y;            // irfft2
  float* pre;          // irfft2, optional
  int B, H, W, C, m1, m2, colw, act;
  float scale;
};

// ---- field -> kept spectrum ----------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(FNO_NTF) void fno_rfft2_kernel(const FnoArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fno_lds[];
  const int tid = threadIdx.x;
  const int nk = (a.m2 + FNO_KYC - 1) / FNO_KYC, ncc = (a.C + FNO_CC - 1) / FNO_CC;
  int b, member;                                     // the workgroups of a sample re-read its field: one XCD
  if (!fno_xcd_item(blockIdx.x, a.B, nk * ncc, b, member)) return;
  const int ky0 = (member % nk) * FNO_KYC, c0 = (member / nk) * FNO_CC;
  const int R = 2 * a.m1;
  const float* __restrict__ xin = a.x + (size_t)b * a.H * a.W * a.C;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  int kyc[FNO_KYC];                                   // clamped into the table; columns past m2 are never stored
#pragma unroll
  for (int k = 0; k < FNO_KYC; ++k) kyc[k] = 2 * (ky0 + k < a.m2 ? ky0 + k : a.m2 - 1);

  // pass 1: T[x][k][re | im][16 channels] = sum_y x[x, y, c] e^{-2 pi i ky y / W}
  for (int it = tid; it < a.H * 4; it += FNO_NTF) {
    const int q = it & 3, x = it >> 2;
    const int c = c0 + 4 * q, nc = a.C - c;
    f32x4 are[FNO_KYC], aim[FNO_KYC];
#pragma unroll
    for (int k = 0; k < FNO_KYC; ++k) are[k] = aim[k] = zero4;
    if (nc > 0) {
      const float* __restrict__ row = xin + (size_t)x * a.W * a.C + c;
#pragma unroll 4
      for (int y = 0; y < a.W; ++y) {
        const f32x4 v = fno_ld4<VEC>(row + (size_t)y * a.C, nc);
        const float* __restrict__ t = a.ty + (size_t)y * a.m2 * 2;
#pragma unroll
        for (int k = 0; k < FNO_KYC; ++k) {
          const float cs = t[kyc[k]], sn = t[kyc[k] + 1];
          are[k] += v * cs;
          aim[k] -= v * sn;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < FNO_KYC; ++k) {
      float* d = fno_lds + ((x * FNO_KYC + k) * 2) * FNO_CC + 4 * q;
      *reinterpret_cast<f32x4*>(d) = are[k];
      *reinterpret_cast<f32x4*>(d + FNO_CC) = aim[k];
    }
  }
  __syncthreads();

  // pass 2: S[r][ky] = sum_x T[x][ky] e^{-2 pi i kx(r) x / H}, rows r and r + m1 together
  for (int it = tid; it < a.m1 * FNO_KYC * 4; it += FNO_NTF) {
    const int q = it & 3, k = (it >> 2) & (FNO_KYC - 1), r = it >> 4;
    const int ky = ky0 + k, c = c0 + 4 * q, nc = a.C - c;
    if (ky >= a.m2 || nc <= 0) continue;
    f32x4 re0 = zero4, im0 = zero4, re1 = zero4, im1 = zero4;
    const float* lds = fno_lds + (k * 2) * FNO_CC + 4 * q;
    const float* __restrict__ t0 = a.tx + (size_t)r * 2;
    const float* __restrict__ t1 = a.tx + (size_t)(r + a.m1) * 2;
#pragma unroll 8
    for (int x = 0; x < a.H; ++x) {
      const f32x4 tr = *reinterpret_cast<const f32x4*>(lds + x * (FNO_KYC * 2 * FNO_CC));
      const f32x4 ti = *reinterpret_cast<const f32x4*>(lds + x * (FNO_KYC * 2 * FNO_CC) + FNO_CC);
      const size_t o = (size_t)x * R * 2;
      const float ca = t0[o], sa = t0[o + 1], cb = t1[o], sb = t1[o + 1];
      re0 += tr * ca;
      re0 += ti * sa;
      im0 += ti * ca;
      im0 -= tr * sa;
      re1 += tr * cb;
      re1 += ti * sb;
      im1 += ti * cb;
      im1 -= tr * sb;
    }
    const float w = a.scale * hermitian_weight(a.colw, ky, a.W);
    float* d0 = a.S + ((((size_t)b * R + r) * a.m2 + ky) * 2) * a.C + c;
    float* d1 = a.S + ((((size_t)b * R + r + a.m1) * a.m2 + ky) * 2) * a.C + c;
    fno_st4<VEC>(d0, re0 * w, nc);
    fno_st4<VEC>(d0 + a.C, im0 * w, nc);
    fno_st4<VEC>(d1, re1 * w, nc);
    fno_st4<VEC>(d1 + a.C, im1 * w, nc);
  }
}

// ---- kept spectrum -> field, + add, activation --------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(FNO_NT) void fno_irfft2_kernel(const FnoArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fno_lds[];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * FNO_XS, c0 = blockIdx.y * FNO_CC, b = blockIdx.z;
  const int R = 2 * a.m1;
  const int LDX = a.m2 * 2 * FNO_CC + 16;
  const float* __restrict__ S = a.S + (size_t)b * R * a.m2 * 2 * a.C;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // pass 1: U[xi][ky][re | im][16 channels] = s w(ky) sum_r S[r][ky] e^{+2 pi i kx(r) x / H}, rows xi and xi + 8 together
  for (int it = tid; it < a.m2 * 32; it += FNO_NT) {
    const int q = it & 3, xp = (it >> 2) & 7, ky = it >> 5;
    const int c = c0 + 4 * q, nc = a.C - c;
    const int xa = x0 + xp < a.H ? x0 + xp : a.H - 1, xb = x0 + xp + 8 < a.H ? x0 + xp + 8 : a.H - 1;
    f32x4 ar = zero4, ai = zero4, br = zero4, bi = zero4;
    if (nc > 0) {
      const float* __restrict__ sp = S + ((size_t)ky * 2) * a.C + c;
      const float* __restrict__ ta = a.tx + (size_t)xa * R * 2;
      const float* __restrict__ tb = a.tx + (size_t)xb * R * 2;
#pragma unroll 2
      for (int r = 0; r < R; ++r) {
        const f32x4 sr = fno_ld4<VEC>(sp + (size_t)r * a.m2 * 2 * a.C, nc);
        const f32x4 si = fno_ld4<VEC>(sp + (size_t)r * a.m2 * 2 * a.C + a.C, nc);
        const float ca = ta[2 * r], sa = ta[2 * r + 1], cb = tb[2 * r], sb = tb[2 * r + 1];
        ar += sr * ca;
        ar -= si * sa;
        ai += sr * sa;
        ai += si * ca;
        br += sr * cb;
        br -= si * sb;
        bi += sr * sb;
        bi += si * cb;
      }
    }
    const float w = a.scale * hermitian_weight(a.colw, ky, a.W);
    float* d = fno_lds + xp * LDX + ky * 2 * FNO_CC + 4 * q;
    *reinterpret_cast<f32x4*>(d) = ar * w;
    *reinterpret_cast<f32x4*>(d + FNO_CC) = ai * w;
    *reinterpret_cast<f32x4*>(d + 8 * LDX) = br * w;
    *reinterpret_cast<f32x4*>(d + 8 * LDX + FNO_CC) = bi * w;
  }
  __syncthreads();

  // pass 2: out[x][y] = sum_ky Re U[x][ky] cos(2 pi ky y / W) - Im U[x][ky] sin(2 pi ky y / W)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int q = lane & 3, xi = lane >> 2;
  const int x = x0 + xi, c = c0 + 4 * q, nc = a.C - c;
  const float* u = fno_lds + xi * LDX + 4 * q;
  for (int yb = wave * 4; yb < a.W; yb += 4 * (FNO_NT / 64)) {
    f32x4 acc[4];
    const float* __restrict__ t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j] = zero4;
      t[j] = a.ty + (size_t)(yb + j < a.W ? yb + j : a.W - 1) * a.m2 * 2;
    }
    for (int ky = 0; ky < a.m2; ++ky) {
      const f32x4 ur = *reinterpret_cast<const f32x4*>(u + ky * 2 * FNO_CC);
      const f32x4 ui = *reinterpret_cast<const f32x4*>(u + ky * 2 * FNO_CC + FNO_CC);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[j] += ur * t[j][2 * ky];
        acc[j] -= ui * t[j][2 * ky + 1];
      }
    }
    if (x < a.H && nc > 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (yb + j < a.W) {
          const size_t off = (((size_t)b * a.H + x) * a.W + yb + j) * a.C + c;
          f32x4 v = acc[j];
          if (a.add) v += fno_ld4<VEC>(a.add + off, nc);
          if (a.pre) fno_st4<VEC>(a.pre + off, v, nc);
          if (a.act) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = act_fwd(a.act, v[e]);
          }
          fno_st4<VEC>(a.y + off, v, nc);
        }
      }
    }
  }
}

// ---- per-mode channel mixing: the weight addressing of fno_mix_kernel / fno_mix_wgrad_kernel (fno_common.h) ---------------------
// G = 2 M kept modes (mode g < M reads weights1, the others weights2); the parameter is planar [2 = re | im][Cin][Cout][M]: the
// imaginary part sits `plane` = Cin Cout M floats after the real part.  T = const float (weights) or float (their gradients)
template <class T>
struct FnoWeights2 {
  static constexpr int BLOCKS = 2;
  T *w1, *w2;
  int M;
  size_t plane;
  __host__ __device__ int block_modes() const { return M; }
  __device__ __forceinline__ T* at(int g) const { return g < M ? w1 + g : w2 + (g - M); }
  __device__ __forceinline__ void load(const float* p, size_t off, float& re, float& im) const {
    re = p[off];
    im = p[off + plane];
  }
  __device__ __forceinline__ void store(float* p, size_t off, float re, float im, int accumulate) const {
    if (accumulate) {
      p[off] += re;
      p[off + plane] += im;
    } else {
      p[off] = re;
      p[off + plane] = im;
    }
  }
};

template <bool VEC>
__global__ __launch_bounds__(256) void fno_dact_kernel(const float* __restrict__ dy, const float* __restrict__ pre,
                                                       float* __restrict__ dpre, int64_t n, int act) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  const int m = n - i < 4 ? (int)(n - i) : 4;
  f32x4 g = fno_ld4<VEC>(dy + i, m);
  const f32x4 p = fno_ld4<VEC>(pre + i, m);
#pragma unroll
  for (int e = 0; e < 4; ++e) g[e] *= act_bwd(act, p[e]);
  fno_st4<VEC>(dpre + i, g, m);
}

static int fno_check_sizes(const char* what, int B, int H, int W, int C, int m1, int m2) {
  DPOT_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && C > 0 && m1 > 0 && m2 > 0 && cdiv(C, FNO_CC) <= 65535,
               "%s: bad sizes B=%d field %dx%d C=%d modes (%d, %d)", what, B, H, W, C, m1, m2);
  DPOT_REQUIRE(2 * m1 <= H && m2 <= W / 2 + 1, "%s: modes (%d, %d) do not fit a %dx%d field (2 m1 <= H, m2 <= W/2 + 1)", what, m1,
               m2, H, W);
  if (H > FNO_MAX_N || W > FNO_MAX_N || m1 > FNO_MAX_MODES || m2 > FNO_MAX_MODES) {
    set_error("%s: field %dx%d with modes (%d, %d) is beyond the LDS intermediates of a workgroup (H, W <= %d, modes <= %d)", what,
              H, W, m1, m2, FNO_MAX_N, FNO_MAX_MODES);
    return DPOT_EUNSUP;
  }
  return DPOT_OK;
}

}  // namespace dpot

using namespace dpot;

extern "C" int dpot_fno_max_size(int modes) { return modes ? FNO_MAX_MODES : FNO_MAX_N; }

extern "C" int dpot_fno_rfft2(const float* x, float* S, const float* tx, const float* ty, int B, int H, int W, int C, int m1,
                              int m2, int col_weights, float scale, dpot_stream_t stream) {
  DPOT_REQUIRE(x && S && x != S && tx && ty, "fno_rfft2: null or aliased pointer");
  if (int rc = fno_check_sizes("fno_rfft2", B, H, W, C, m1, m2)) return rc;
  FnoArgs a = {};
  a.x = x, a.S = S, a.tx = tx, a.ty = ty;
  a.B = B, a.H = H, a.W = W, a.C = C, a.m1 = m1, a.m2 = m2, a.colw = col_weights, a.scale = scale;
  const size_t lds = sizeof(float) * (size_t)H * FNO_KYC * 2 * FNO_CC;
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(S);
  const int64_t nwg = fno_xcd_grid(B, cdiv(m2, FNO_KYC) * cdiv(C, FNO_CC));
  DPOT_REQUIRE(nwg <= 0x7fffffff, "fno_rfft2: too many workgroups");
  const dim3 grid((unsigned)nwg);
  if (vec) {
    if (int rc = raise_dynamic_lds<fno_rfft2_kernel<true>>("fno_rfft2")) return rc;
    hipLaunchKernelGGL(fno_rfft2_kernel<true>, grid, dim3(FNO_NTF), lds, as_stream(stream), a);
  } else {
    if (int rc = raise_dynamic_lds<fno_rfft2_kernel<false>>("fno_rfft2")) return rc;
    hipLaunchKernelGGL(fno_rfft2_kernel<false>, grid, dim3(FNO_NTF), lds, as_stream(stream), a);
  }
  return check_launch("fno_rfft2_kernel");
}

extern "C" int dpot_fno_irfft2(const float* S, const float* add, float* y, float* pre, const float* tx, const float* ty, int B,
                               int H, int W, int C, int m1, int m2, int col_weights, float scale, int act,
                               dpot_stream_t stream) {
  DPOT_REQUIRE(S && y && S != y && tx && ty && y != pre, "fno_irfft2: null or aliased pointer");
  DPOT_REQUIRE(act >= DPOT_ACT_NONE && act <= DPOT_ACT_SILU, "fno_irfft2: unknown activation %d", act);
  if (int rc = fno_check_sizes("fno_irfft2", B, H, W, C, m1, m2)) return rc;
  FnoArgs a = {};
  a.S = const_cast<float*>(S), a.add = add, a.y = y, a.pre = pre, a.tx = tx, a.ty = ty;
  a.B = B, a.H = H, a.W = W, a.C = C, a.m1 = m1, a.m2 = m2, a.colw = col_weights, a.scale = scale, a.act = act;
  const size_t lds = sizeof(float) * (size_t)FNO_XS * (m2 * 2 * FNO_CC + 16);
  const bool vec = C % 4 == 0 && aligned16(S) && aligned16(y) && aligned16(add) && aligned16(pre);
  const dim3 grid(cdiv(H, FNO_XS), cdiv(C, FNO_CC), B);
  if (vec) {
    if (int rc = raise_dynamic_lds<fno_irfft2_kernel<true>>("fno_irfft2")) return rc;
    hipLaunchKernelGGL(fno_irfft2_kernel<true>, grid, dim3(FNO_NT), lds, as_stream(stream), a);
  } else {
    if (int rc = raise_dynamic_lds<fno_irfft2_kernel<false>>("fno_irfft2")) return rc;
    hipLaunchKernelGGL(fno_irfft2_kernel<false>, grid, dim3(FNO_NT), lds, as_stream(stream), a);
  }
  return check_launch("fno_irfft2_kernel");
}

extern "C" int dpot_fno_mix(const float* X, const float* w1, const float* w2, float* O, int B, int Cin, int Cout, int m1, int m2,
                            int adjoint, dpot_stream_t stream) {
  DPOT_REQUIRE(X && w1 && w2 && O && X != O, "fno_mix: null or aliased pointer");
  DPOT_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && m1 > 0 && m2 > 0 && (int64_t)m1 * m2 <= (1 << 24),
               "fno_mix: bad sizes B=%d Cin=%d Cout=%d modes (%d, %d)", B, Cin, Cout, m1, m2);
  const FnoWeights2<const float> w = {w1, w2, m1 * m2, (size_t)Cin * Cout * m1 * m2};
  return fno_mix_launch("fno_mix", "fno_mix_kernel", X, w, O, B, Cin, Cout, adjoint, stream);
}

extern "C" int dpot_fno_mix_wgrad(const float* X, const float* dO, float* dw1, float* dw2, int B, int Cin, int Cout, int m1,
                                  int m2, int accumulate, dpot_stream_t stream) {
  DPOT_REQUIRE(X && dO && dw1 && dw2 && dw1 != dw2, "fno_mix_wgrad: null or aliased pointer");
  DPOT_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && m1 > 0 && m2 > 0 && (int64_t)m1 * m2 <= (1 << 24),
               "fno_mix_wgrad: bad sizes B=%d Cin=%d Cout=%d modes (%d, %d)", B, Cin, Cout, m1, m2);
  const FnoWeights2<float> dw = {dw1, dw2, m1 * m2, (size_t)Cin * Cout * m1 * m2};
  return fno_mix_wgrad_launch("fno_mix_wgrad", "fno_mix_wgrad_kernel", X, dO, dw, B, Cin, Cout, accumulate, stream);
}

extern "C" int dpot_fno_dact(const float* dy, const float* pre, float* dpre, int64_t n, int act, dpot_stream_t stream) {
  DPOT_REQUIRE(dy && pre && dpre && n > 0 && n <= ((int64_t)1 << 40), "fno_dact: null pointer or bad length");
  DPOT_REQUIRE(act >= DPOT_ACT_NONE && act <= DPOT_ACT_SILU, "fno_dact: unknown activation %d", act);
  const bool vec = n % 4 == 0 && aligned16(dy) && aligned16(pre) && aligned16(dpre);
  const int64_t blocks = cdiv64(cdiv64(n, 4), 256);
  DPOT_REQUIRE(blocks <= 0x7fffffff, "fno_dact: too long");
  if (vec)
    hipLaunchKernelGGL(fno_dact_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), dy, pre, dpre, n, act);
  else
    hipLaunchKernelGGL(fno_dact_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), dy, pre, dpre, n, act);
  return check_launch("fno_dact_kernel");
}
