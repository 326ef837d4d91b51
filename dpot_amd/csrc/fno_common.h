// fno_common.h - what the kernels of the FNO baselines share (fno.hip: FNO2d, fno3.hip: FNO3d): predicated 4-channel accesses and
// the XCD-aware workgroup ids.
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

}  // namespace dpot
