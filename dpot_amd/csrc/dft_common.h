// dft_common.h - what every spectral kernel family shares: the twiddle table builder, the Hermitian weight of a half spectrum
// and the channel-slab width of the generic transforms (dft.hip, dft3.hip, dft_fast.h and through it gn_dft.hip /
// afno_fused.hip, fno.hip).
#pragma once
#include "common.h"

namespace dpot {

// c[t] = cos(2 pi t / n), s[t] = sin(2 pi t / n), t < n, by the whole workgroup (the caller's barrier publishes them)
__device__ __forceinline__ void make_twiddles(float* c, float* s, int n) {
  for (int t = threadIdx.x; t < n; t += blockDim.x) {
    const double a = (double)(2 * t) / (double)n;  // angle / pi
    c[t] = (float)cospi(a);
    s[t] = (float)sinpi(a);
  }
}

// weight of bin k of the half spectrum of an n-point real axis in the inverse transform's sum (and in its adjoint): 1 at k = 0
// and (n even) at k = n / 2, the bins that are their own mirror image, else 2; on = 0: 1 everywhere
__device__ __forceinline__ float hermitian_weight(int on, int k, int n) {
  if (!on || k == 0 || ((n & 1) == 0 && k == (n >> 1))) return 1.f;
  return 2.f;
}

// the largest power-of-two channel slab (<= 64) dividing E whose floats_per_channel * cc + tw_floats floats meet
// LDS_GENERIC_BUDGET; 0: not even one channel fits
static inline int lds_slab_cc(int E, long long floats_per_channel, int tw_floats) {
  for (int cc = 64; cc >= 1; cc >>= 1) {
    if (E % cc) continue;
    if (floats_per_channel * cc + tw_floats <= LDS_GENERIC_BUDGET / 4) return cc;
  }
  return 0;
}

}  // namespace dpot
