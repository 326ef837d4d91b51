// fno_common.h - what the kernels of the FNO baselines share (fno.hip: FNO2d, fno3.hip: FNO3d): predicated 4-channel accesses,
// the XCD-aware workgroup ids, and the per-mode channel mixing with its weight gradient - ONE kernel pair and ONE launcher pair
// for both ranks, which differ only in how a kept mode finds its complex weight (a policy W, defined beside each entry point).
#pragma once
#include "common.h"

namespace dpot {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <bool VEC>
__device__ __forceinline__ f32x4 fno_ld4(const float* __restrict__ p, int n) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    if (n > 0) v = *reinterpret_cast<const f32x4*>(p);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) v[j] = p[j];
  }
  return v;
}

template <bool VEC>
__device__ __forceinline__ void fno_st4(float* __restrict__ p, f32x4 v, int n) {
  if (VEC) {
    if (n > 0) *reinterpret_cast<f32x4*>(p) = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) p[j] = v[j];
  }
}

// Workgroups that re-read the same bytes should share an XCD's L2 (workgroups are dealt round-robin over the 8 XCDs: ids i and
// i + 8 share one - a matter of speed only, nothing depends on it).  A one-dimensional grid of fno_xcd_grid(groups, members)
// workgroups; workgroup id -> (group g, member k) with all members of a group 8 ids apart.  false: a padding workgroup.
__device__ __forceinline__ bool fno_xcd_item(int id, int n_groups, int n_members, int& g, int& k) {
  const int j = id >> 3;
  g = (j / n_members) * 8 + (id & 7);
  k = j % n_members;
  return g < n_groups;
}
static inline int64_t fno_xcd_grid(int n_groups, int n_members) { return (int64_t)cdiv(n_groups, 8) * 8 * n_members; }

// ---- per-mode channel mixing ---------------------------------------------------------------------------------------------
// X[B][G][2][K], O[B][G][2][N] over the G kept modes of a sample, which fall into W::BLOCKS weight tensors of block_modes()
// modes each.  W is the rank's weight addressing, passed by value and resolved at compile time.  It answers four things:
//   W::BLOCKS, w.block_modes()          the kept modes: G = BLOCKS * block_modes()
//   w.at(g)                             kept mode g -> its weight tensor, advanced to g's mode index inside it
//   w.load(p, off, re, im)              the complex weight `off` mode strides from p = at(g); off = a * sa + n * sn for
//                                       (reduced index a, output index n).  The kernel multiplies im by sgn (-1: conj(W))
//   w.store(p, off, re, im, accumulate) one element of the weight gradient, written or added
template <bool VEC, class W>
__global__ __launch_bounds__(256) void fno_mix_kernel(const float* __restrict__ X, const W w, float* __restrict__ O, int B, int K,
                                                      int N, size_t sa, size_t sn, float sgn) {
  const int G = W::BLOCKS * w.block_modes();
  const int gx = (G + 63) / 64, gy = ((N + 3) / 4 + 3) / 4;
  int grp, bt;                                       // the sample tiles of a (mode block, output tile) re-read its weights: one XCD
  if (!fno_xcd_item(blockIdx.x, gx * gy, (B + 3) / 4, grp, bt)) return;
  const int g = (grp % gx) * 64 + threadIdx.x, o0 = ((grp / gx) * 4 + threadIdx.y) * 4, b0 = bt * 4;
  if (g >= G || o0 >= N) return;
  const float* __restrict__ wg = w.at(g);
  const int no = N - o0;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 accr[4], acci[4];                             // per sample, over the 4 outputs
#pragma unroll
  for (int bb = 0; bb < 4; ++bb) accr[bb] = acci[bb] = zero4;
  for (int i0 = 0; i0 < K; i0 += 4) {
    const int ni = K - i0;
    f32x4 xr[4], xi[4];
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      const float* p = X + (((size_t)(b0 + bb) * G + g) * 2) * K + i0;
      const int n = b0 + bb < B ? ni : 0;
      xr[bb] = fno_ld4<VEC>(p, n);
      xi[bb] = fno_ld4<VEC>(p + K, n);
    }
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      if (ii < ni) {
        f32x4 wr = zero4, wi = zero4;
#pragma unroll
        for (int oo = 0; oo < 4; ++oo) {
          if (oo < no) {
            float re, im;
            w.load(wg, (size_t)(i0 + ii) * sa + (size_t)(o0 + oo) * sn, re, im);
            wr[oo] = re;
            wi[oo] = sgn * im;
          }
        }
#pragma unroll
        for (int bb = 0; bb < 4; ++bb) {
          accr[bb] += wr * xr[bb][ii];
          accr[bb] -= wi * xi[bb][ii];
          acci[bb] += wi * xr[bb][ii];
          acci[bb] += wr * xi[bb][ii];
        }
      }
    }
  }
#pragma unroll
  for (int bb = 0; bb < 4; ++bb) {
    if (b0 + bb < B) {
      float* p = O + (((size_t)(b0 + bb) * G + g) * 2) * N + o0;
      fno_st4<VEC>(p, accr[bb], no);
      fno_st4<VEC>(p + N, acci[bb], no);
    }
  }
}

// dW[i, o, g] = sum_b conj(X[b, g, i]) dO[b, g, o], b ascending; a thread keeps a 4 x 4 (i, o) tile of one mode
template <bool VEC, class W>
__global__ __launch_bounds__(256) void fno_mix_wgrad_kernel(const float* __restrict__ X, const float* __restrict__ dO, const W dw,
                                                            int B, int Cin, int Cout, int accumulate) {
  const int M = dw.block_modes(), G = W::BLOCKS * M;
  const int nto = (Cout + 3) / 4, nti = (Cin + 3) / 4;
  int mb, tr;                                        // the channel tiles of a mode block re-read its rows of X and dO: one XCD
  if (!fno_xcd_item(blockIdx.x, (G + 63) / 64, (nti * nto + 3) / 4, mb, tr)) return;
  const int g = mb * 64 + threadIdx.x, t = tr * 4 + threadIdx.y;
  if (g >= G || t >= nti * nto) return;
  const int i0 = (t / nto) * 4, o0 = (t % nto) * 4;
  const int ni = Cin - i0, no = Cout - o0;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 ar[4], ai[4];                                 // per input channel, over the 4 outputs
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) ar[ii] = ai[ii] = zero4;
  for (int b = 0; b < B; ++b) {
    const float* px = X + (((size_t)b * G + g) * 2) * Cin + i0;
    const float* pd = dO + (((size_t)b * G + g) * 2) * Cout + o0;
    const f32x4 xr = fno_ld4<VEC>(px, ni), xi = fno_ld4<VEC>(px + Cin, ni);
    const f32x4 dr = fno_ld4<VEC>(pd, no), di = fno_ld4<VEC>(pd + Cout, no);
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      ar[ii] += dr * xr[ii];
      ar[ii] += di * xi[ii];
      ai[ii] += di * xr[ii];
      ai[ii] -= dr * xi[ii];
    }
  }
  float* __restrict__ out = dw.at(g);
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
#pragma unroll
    for (int oo = 0; oo < 4; ++oo) {
      if (ii < ni && oo < no) dw.store(out, ((size_t)(i0 + ii) * Cout + o0 + oo) * M, ar[ii][oo], ai[ii][oo], accumulate);
    }
  }
}

// The launches behind dpot_fno_mix / dpot_fno3_mix and their weight gradients.  `what` names the entry point in the error
// texts and `kernel` the launch in check_launch's; the entry point has checked its pointers and B, Cin, Cout, modes > 0 (its
// own message names the rank's mode tuple).

template <class W>
static int fno_mix_launch(const char* what, const char* kernel, const float* X, const W w, float* O, int B, int Cin, int Cout,
                          int adjoint, dpot_stream_t stream) {
  const int M = w.block_modes();
  // forward: reduce the layer's inputs i, produce its outputs o; adjoint: reduce o, produce i, conj(W)
  const int K = adjoint ? Cout : Cin, N = adjoint ? Cin : Cout;
  const size_t si = (size_t)Cout * M, so = (size_t)M;
  const size_t sa = adjoint ? so : si, sn = adjoint ? si : so;
  const int64_t groups = (int64_t)cdiv(W::BLOCKS * M, 64) * cdiv(cdiv(N, 4), 4);
  const int64_t nwg = groups <= (1 << 24) ? fno_xcd_grid((int)groups, cdiv(B, 4)) : -1;
  DPOT_REQUIRE(nwg > 0 && nwg <= 0x7fffffff, "%s: too many workgroups", what);
  const bool vec = K % 4 == 0 && N % 4 == 0 && aligned16(X) && aligned16(O);
  const dim3 grid((unsigned)nwg), block(64, 4);
  const float sgn = adjoint ? -1.f : 1.f;
  if (vec)
    hipLaunchKernelGGL((fno_mix_kernel<true, W>), grid, block, 0, as_stream(stream), X, w, O, B, K, N, sa, sn, sgn);
  else
    hipLaunchKernelGGL((fno_mix_kernel<false, W>), grid, block, 0, as_stream(stream), X, w, O, B, K, N, sa, sn, sgn);
  return check_launch(kernel);
}

template <class W>
static int fno_mix_wgrad_launch(const char* what, const char* kernel, const float* X, const float* dO, const W dw, int B, int Cin,
                                int Cout, int accumulate, dpot_stream_t stream) {
  const int64_t tiles = (int64_t)cdiv(Cin, 4) * cdiv(Cout, 4);
  DPOT_REQUIRE(cdiv64(tiles, 4) <= (1 << 20), "%s: too many channel pairs (%d x %d)", what, Cin, Cout);
  const int64_t nwg = fno_xcd_grid(cdiv(W::BLOCKS * dw.block_modes(), 64), (int)cdiv64(tiles, 4));
  DPOT_REQUIRE(nwg <= 0x7fffffff, "%s: too many workgroups", what);
  const bool vec = Cin % 4 == 0 && Cout % 4 == 0 && aligned16(X) && aligned16(dO);
  const dim3 grid((unsigned)nwg), block(64, 4);
  if (vec)
    hipLaunchKernelGGL((fno_mix_wgrad_kernel<true, W>), grid, block, 0, as_stream(stream), X, dO, dw, B, Cin, Cout, accumulate);
  else
    hipLaunchKernelGGL((fno_mix_wgrad_kernel<false, W>), grid, block, 0, as_stream(stream), X, dO, dw, B, Cin, Cout, accumulate);
  return check_launch(kernel);
}

}  // namespace dpot
