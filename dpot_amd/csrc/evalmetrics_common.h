// evalmetrics_common.h - what evalmetrics.hip ([B, X, Y, T, C]) and evalmetrics3d.hip ([B, X, Y, Z, T, C]) share: everything of
// the metric set that is not a transform.  The pointwise statistics of a chunk of planes and their way from the lanes to one
// partial record in HBM, the NaN-propagating maximum, the pad rule, the accumulator layout and the arithmetic that folds the
// partials of a batch into the accumulator.  A new key or a mask is written here once.
//
// The two finalize kernels stay two kernels because the ORDER in which an entry's partials are added is part of the bits: the
// 2-D kernel has few partials per entry (stripes of 16 wavenumbers) and one thread walks them in order; the 3-D kernel has
// nz/2 x stripes shell partials and row-tiles / 4 statistics partials per entry and needs a wave per entry (lane-strided,
// then a butterfly).  Each hands its order to eval_finalize_entry as a gather policy; the arithmetic per entry is one body.
#pragma once
#include "common.h"

#include <math.h>

namespace dpot {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int EVAL_PC = 4;                 // planes p = (t, c) whose statistics one workgroup counts: one 16-byte load
constexpr int EVAL_NW = 4;                 // waves of such a workgroup
constexpr int EVAL_NSTAT = 7;              // sum|e| sum|t| sum e^2 sum t^2 max|e| max|t| boundary; slot 7 of a record unused

// ---- host -------------------------------------------------------------------------------------------------------------
// the contraction extent n, or the wavenumber extent n / 2 (half), rounded up to the 16 of an MFMA tile
static inline int eval_pad(int n, int half) {
  if (n <= 0) return 0;
  const int m = half ? n / 2 : n;
  return m <= 0 ? 0 : (m + 15) / 16 * 16;
}

// 8-byte words of the accumulator: [0] = number of samples (int64 bits), [1] reserved, then doubles: nmae|nmse|nmxe [3][C],
// nmae_t|nmse_t|nmxe_t|bd [4][T][C], the shell sums [T][C][K]; every entry a sum over the samples seen
static inline int64_t eval_acc_elems(int64_t K, int T, int C) {
  const int64_t TC = (int64_t)T * C;
  return 2 + 3 * (int64_t)C + 4 * TC + TC * K;
}

// accumulator entries eval_finalize_entry serves: C channels, T C planes, T C K shells and the sample count
__host__ __device__ static inline int64_t eval_finalize_items(int64_t K, int T, int C) {
  return (int64_t)C + (int64_t)T * C * (1 + K) + 1;
}

// ---- the NaN-propagating maximum -----------------------------------------------------------------------------------------
__device__ __forceinline__ float eval_max_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ double eval_max_nan(double a, double b) { return (b > a || b != b) ? b : a; }

// ---- pointwise statistics of EVAL_PC planes, per lane -------------------------------------------------------------------------
struct EvalStats {
  float ae[EVAL_PC], at[EVAL_PC], se[EVAL_PC], st[EVAL_PC], me[EVAL_PC], mt[EVAL_PC], bd[EVAL_PC];
};

__device__ __forceinline__ void eval_stats_zero(EvalStats& st) {
#pragma unroll
  for (int pc = 0; pc < EVAL_PC; ++pc) st.ae[pc] = st.at[pc] = st.se[pc] = st.st[pc] = st.me[pc] = st.mt[pc] = st.bd[pc] = 0.f;
}

// one point of every plane: e = pred - target, t = target, w = number of edges (faces) of the domain the point lies on.  An
// out-of-range point holds e = t = 0 and adds nothing.
__device__ __forceinline__ void eval_stats_point(EvalStats& st, const f32x4& e, const f32x4& t, float w) {
#pragma unroll
  for (int pc = 0; pc < EVAL_PC; ++pc) {
    const float ev = e[pc], tv = t[pc];
    const float e2 = ev * ev;
    st.ae[pc] += __builtin_fabsf(ev);
    st.at[pc] += __builtin_fabsf(tv);
    st.se[pc] += e2;
    st.st[pc] = fmaf(tv, tv, st.st[pc]);
    // the builtin that the float eval_max_nan wraps, itself: through the wrapper eval_stats_kernel of evalmetrics.hip is
    // scheduled differently (3134 instead of 3206 instructions) and [32, 128, 128, 10, 4] measured 0.5 % slower
    st.me[pc] = __builtin_elementwise_maximum(st.me[pc], __builtin_fabsf(ev));
    st.mt[pc] = __builtin_elementwise_maximum(st.mt[pc], __builtin_fabsf(tv));
    st.bd[pc] = fmaf(w, e2, st.bd[pc]);
  }
}

// the lanes of a wave into wstat [wave][pc][8] (LDS, doubles); __syncthreads() before eval_stats_store
__device__ __forceinline__ void eval_stats_wave_reduce(const EvalStats& st, double* __restrict__ wstat, int wave, int lane) {
#pragma unroll
  for (int pc = 0; pc < EVAL_PC; ++pc) {
    const double v0 = wave_sum_d((double)st.ae[pc]), v1 = wave_sum_d((double)st.at[pc]);
    const double v2 = wave_sum_d((double)st.se[pc]), v3 = wave_sum_d((double)st.st[pc]);
    const double v6 = wave_sum_d((double)st.bd[pc]);
    float me = st.me[pc], mt = st.mt[pc];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      me = eval_max_nan(me, __shfl_xor(me, off, 64));
      mt = eval_max_nan(mt, __shfl_xor(mt, off, 64));
    }
    if (lane == 0) {
      double* w = wstat + (wave * EVAL_PC + pc) * 8;
      w[0] = v0, w[1] = v1, w[2] = v2, w[3] = v3, w[4] = (double)me, w[5] = (double)mt, w[6] = v6;
    }
  }
}

// the waves of a workgroup, in order, into partial record `part` of `parts` of the planes plane0 .. plane0 + npc - 1 (plane =
// b TC + p): statp [B][TC][parts][8]
__device__ __forceinline__ void eval_stats_store(const double* __restrict__ wstat, double* __restrict__ statp, size_t plane0,
                                                 int npc, int parts, int part) {
  if ((int)threadIdx.x < EVAL_PC * EVAL_NSTAT) {
    const int pc = threadIdx.x / EVAL_NSTAT, k = threadIdx.x % EVAL_NSTAT;
    if (pc < npc) {
      double v = wstat[pc * 8 + k];
      for (int w = 1; w < EVAL_NW; ++w) {                          // the waves in order
        const double o = wstat[(w * EVAL_PC + pc) * 8 + k];
        if (k == 4 || k == 5)
          v = eval_max_nan(v, o);
        else
          v += o;
      }
      statp[((plane0 + pc) * parts + part) * 8 + k] = v;
    }
  }
}

// v (op)= one partial record r: what every gather does with the records it walks
__device__ __forceinline__ void eval_stats_fold(double* v, const double* __restrict__ r) {
  v[0] += r[0], v[1] += r[1], v[2] += r[2], v[3] += r[3], v[6] += r[6];
  v[4] = eval_max_nan(v[4], r[4]);
  v[5] = eval_max_nan(v[5], r[5]);
}

// ---- finalize: one accumulator entry ------------------------------------------------------------------------------------
// `idx` of eval_finalize_items: what acc gains from the B samples of this batch.  The gather policy G supplies the partials in
// its own fixed order:
//   void   plane_stats(int b, int p, double v[EVAL_NSTAT])   the statistics of plane p of sample b
//   double shell_sum(double sum, int b, int p, int s)         sum + the partials of shell s of that plane (the 2-D gather
//                                                             adds them to the running sum one by one, the 3-D one adds their
//                                                             wave-wide total: both orders are kept as they were)
//   bool   writes()                                            whether this lane owns the entry
template <class G>
__device__ __forceinline__ void eval_finalize_entry(const G& g, long long idx, double* __restrict__ acc, int B, double faces,
                                                    int T, int C, int K) {
  const int TC = T * C;
  const long long n_items = eval_finalize_items(K, T, C);
  if (idx >= n_items) return;
  double* out = acc + 2;
  if (idx == n_items - 1) {                                        // the sample count
    long long* cnt = reinterpret_cast<long long*>(acc);
    if (g.writes()) cnt[0] += B;
    return;
  }
  if (idx < C) {                                                   // whole-rollout ratios of channel c
    const int c = (int)idx;
    double mae = 0.0, mse = 0.0, mxe = 0.0;
    for (int b = 0; b < B; ++b) {
      double tot[EVAL_NSTAT] = {0, 0, 0, 0, 0, 0, 0};
      for (int t = 0; t < T; ++t) {
        double v[EVAL_NSTAT];
        g.plane_stats(b, t * C + c, v);
        tot[0] += v[0], tot[1] += v[1], tot[2] += v[2], tot[3] += v[3];
        tot[4] = eval_max_nan(tot[4], v[4]);
        tot[5] = eval_max_nan(tot[5], v[5]);
      }
      mae += tot[0] / tot[1];
      mse += sqrt(tot[2] / tot[3]);
      mxe += tot[4] / tot[5];
    }
    if (g.writes()) {
      out[c] += mae;
      out[C + c] += mse;
      out[2 * C + c] += mxe;
    }
    return;
  }
  if (idx < C + TC) {                                              // per-step ratios and the boundary (face) error of plane p
    const int p = (int)(idx - C);
    double mae = 0.0, mse = 0.0, mxe = 0.0, bd = 0.0;
    for (int b = 0; b < B; ++b) {
      double v[EVAL_NSTAT];
      g.plane_stats(b, p, v);
      mae += v[0] / v[1];
      mse += sqrt(v[2] / v[3]);
      mxe += v[4] / v[5];
      bd += sqrt(v[6] / faces);
    }
    if (g.writes()) {
      double* o = out + 3 * C;
      o[p] += mae;
      o[TC + p] += mse;
      o[2 * TC + p] += mxe;
      o[3 * TC + p] += bd;
    }
    return;
  }
  {                                                                // shell s of plane p
    const long long e = idx - C - TC;
    const int p = (int)(e / K), s = (int)(e % K);
    double sum = 0.0;
    for (int b = 0; b < B; ++b) sum = g.shell_sum(sum, b, p, s);
    if (g.writes()) out[3 * C + 4 * TC + e] += sum;
  }
}

}  // namespace dpot
