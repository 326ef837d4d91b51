// metrics.hip - what a training loop logs, computed without leaving the stream: the dataset-classification cross-entropy
// (train_temporal.py:209-213), the full-rollout relative L2 from the per-step statistics dpot_rel_l2_fwd already leaves
// (utils/criterion.py:38-59 on the concatenated rollout) and the running metrics of train_temporal.py:221-223, 232-233.
// All four kernels are LATENCY-sized (a few KB of traffic): one launch each, one workgroup where a reduction is involved,
// fixed reduction order, no atomics - a result never depends on the launch.  No host synchronisation: legal under capture.
#include "common.h"

#include <math.h>

namespace dpot {

// ---- cross-entropy (sum over rows) + argmax accuracy --------------------------------------------------------------
// One 1024-thread workgroup.  A row is handled by a group of G lanes (G = pow2 >= n_cls, at most one wave): the lanes stride
// over the classes, the group reduces {max, first index of the max} and then sum exp(x - max) with xor butterflies that stay
// inside the group.  Lane 0 of every group adds its rows' losses in row order (double); the block sum is a fixed tree.
constexpr int CE_NONE = 0x7fffffff;                    // "this lane has seen no class yet"

__global__ __launch_bounds__(1024) void cls_ce_fwd_kernel(const float* __restrict__ logits,
                                                          const long long* __restrict__ labels,
                                                          float* __restrict__ row_stats, dpot_cls_ce_out* __restrict__ out,
                                                          int B, int n_cls, int G) {
  __shared__ double shd[16];
  const int lane = threadIdx.x & 63;
  const int sub = lane & (G - 1);                      // lane inside its row group
  const int groups = 1024 / G;                         // rows in flight per trip of the block
  const int grp = threadIdx.x / G;
  double loss = 0.0;
  long long correct = 0, valid = 0, invalid = 0;
  for (int row = grp; row < B; row += groups) {
    const float* x = logits + (long long)row * n_cls;
    float mx = -INFINITY;
    int am = CE_NONE;
    for (int c = sub; c < n_cls; c += G) {
      const float v = x[c];
      if (v > mx || am == CE_NONE) {                   // strict: the first maximal index among this lane's classes
        mx = v;
        am = c;
      }
    }
    for (int o = G >> 1; o >= 1; o >>= 1) {
      const float om = __shfl_xor(mx, o, 64);
      const int oa = __shfl_xor(am, o, 64);
      if (oa != CE_NONE && (am == CE_NONE || om > mx || (om == mx && oa < am))) {
        mx = om;
        am = oa;
      }
    }
    float se = 0.f;
    for (int c = sub; c < n_cls; c += G) se += expf(x[c] - mx);
    for (int o = G >> 1; o >= 1; o >>= 1) se += __shfl_xor(se, o, 64);
    if (sub == 0) {
      const float lse = mx + logf(se);
      row_stats[2 * row] = mx;
      row_stats[2 * row + 1] = lse;
      const long long lab = labels[row];
      if (lab >= 0 && lab < n_cls) {                   // a label outside [0, n_cls) indexes nothing
        loss += (double)lse - (double)x[lab];
        correct += (am == (int)lab) ? 1 : 0;
        ++valid;
      } else {
        ++invalid;
      }
    }
  }
  // counts: exact in double (<= 2^31 rows), so the four block sums share one reduction shape
  const double l = block_sum_d(loss, shd);
  const double c = block_sum_d((double)correct, shd);
  const double v = block_sum_d((double)valid, shd);
  const double iv = block_sum_d((double)invalid, shd);
  if (threadIdx.x == 0) {
    out->loss = (float)l;
    out->reserved = 0;
    out->correct = (long long)c;
    out->valid = (long long)v;
    out->invalid = (long long)iv;
  }
}

// dlogits = gloss[0] * (softmax - onehot); rows with a label outside [0, n_cls): zeros
__global__ __launch_bounds__(256) void cls_ce_bwd_kernel(const float* __restrict__ logits,
                                                         const long long* __restrict__ labels,
                                                         const float* __restrict__ row_stats,
                                                         const float* __restrict__ gloss, float* __restrict__ dlogits,
                                                         long long total, int n_cls) {
  const float g = gloss[0];
  for (long long idx = blockIdx.x * 256ll + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long row = idx / n_cls;
    const int c = (int)(idx - row * n_cls);
    const long long lab = labels[row];
    float v = 0.f;
    if (lab >= 0 && lab < n_cls) {
      const float p = expf(logits[idx] - row_stats[2 * row + 1]);
      v = g * (p - (c == (int)lab ? 1.f : 0.f));
    }
    dlogits[idx] = v;
  }
}

// ---- full-rollout relative L2 from the per-step statistics --------------------------------------------------------
// One 1024-thread workgroup walks the batch in tiles of SPT = 1024 / C whole samples: thread (b, c) adds the n_steps
// {sum d^2, sum y^2} of its channel in step order (double) and leaves the channel's term in LDS, then one thread per
// sample adds its channels in order and divides by the number of channels whose mask sum is not zero.
__device__ __forceinline__ const float* step_stats(const float* const* __restrict__ ptrs, const float* __restrict__ base,
                                                   long long stride, int t) {
  return ptrs ? ptrs[t] : base + t * stride;
}
__global__ __launch_bounds__(1024) void rel_l2_combine_kernel(const float* const* __restrict__ ptrs,
                                                              const float* __restrict__ base, long long stride,
                                                              int n_steps, int B, int C, float* __restrict__ out) {
  __shared__ double term[1024];
  __shared__ int live[1024];
  __shared__ double shd[16];
  const int spt = 1024 / C;                            // C <= 1024: at least one whole sample per tile
  double acc = 0.0;
  for (int b0 = 0; b0 < B; b0 += spt) {
    const int nb = min(spt, B - b0);
    if ((int)threadIdx.x < nb * C) {
      const long long e = ((long long)b0 * C + threadIdx.x) * 4;
      double d2 = 0.0, y2 = 0.0;
      float msum = 0.f;
#pragma unroll 4
      for (int t = 0; t < n_steps; ++t) {
        const float4 v = *reinterpret_cast<const float4*>(step_stats(ptrs, base, stride, t) + e);
        d2 += (double)v.x;
        y2 += (double)v.y;
        if (t == 0) msum = v.z;                        // the mask is the same at every step: the first one decides
      }
      live[threadIdx.x] = msum != 0.f;
      term[threadIdx.x] = sqrt(d2) / (sqrt(y2) + 1e-8);
    }
    __syncthreads();
    if ((int)threadIdx.x < nb) {
      double s = 0.0;
      int nch = 0;
      for (int c = 0; c < C; ++c) {
        s += term[threadIdx.x * C + c];
        nch += live[threadIdx.x * C + c];
      }
      acc += s / (double)nch;
    }
    __syncthreads();
  }
  acc = block_sum_d(acc, shd);
  if (threadIdx.x == 0) out[0] = (float)acc;
}

// ---- running metrics ----------------------------------------------------------------------------------------------
// acc[0] += this step, acc[1] = this step.  One wave; lane 0 forms the values and stores them with plain vector stores.
__global__ __launch_bounds__(64) void metrics_accum_kernel(dpot_metrics* __restrict__ acc, const float* __restrict__ l2_step,
                                                           const float* __restrict__ l2_full,
                                                           const dpot_cls_ce_out* __restrict__ cls, int n_cls_out,
                                                           const float* __restrict__ sumsq, float grad_scale,
                                                           long long samples, long long ar_steps, long long opt_steps) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  dpot_metrics m;
  m.l2_step = l2_step ? (double)l2_step[0] : 0.0;
  m.l2_full = l2_full ? (double)l2_full[0] : 0.0;
  m.cls_loss = 0.0;
  m.cls_correct = m.cls_total = m.cls_invalid = 0;
  for (int k = 0; k < n_cls_out; ++k) {                // the AR steps of the rollout, in order
    m.cls_loss += (double)cls[k].loss;
    m.cls_correct += cls[k].correct;
    m.cls_total += cls[k].valid;
    m.cls_invalid += cls[k].invalid;
  }
  m.grad_norm = sumsq ? sqrt((double)sumsq[0]) * (double)grad_scale : 0.0;
  m.samples = samples;
  m.ar_steps = ar_steps;
  m.opt_steps = opt_steps;
  const double watched = m.l2_step + m.l2_full + m.cls_loss;       // NaN or inf in any of the step's losses
  m.nonfinite_steps = isfinite(watched) ? 0 : 1;
  m.reserved = 0;
  dpot_metrics a = acc[0];
  a.l2_step += m.l2_step;
  a.l2_full += m.l2_full;
  a.cls_loss += m.cls_loss;
  a.grad_norm += m.grad_norm;
  a.cls_correct += m.cls_correct;
  a.cls_total += m.cls_total;
  a.cls_invalid += m.cls_invalid;
  a.samples += m.samples;
  a.ar_steps += m.ar_steps;
  a.opt_steps += m.opt_steps;
  a.nonfinite_steps += m.nonfinite_steps;
  a.reserved = 0;
  acc[0] = a;
  acc[1] = m;
}

}  // namespace dpot

using namespace dpot;

extern "C" int dpot_cls_ce_fwd(const float* logits, const int64_t* labels, float* row_stats, dpot_cls_ce_out* out, int B,
                               int n_cls, dpot_stream_t stream) {
  DPOT_REQUIRE(logits && labels && row_stats && out, "cls_ce_fwd: null pointer");
  DPOT_REQUIRE(B > 0 && n_cls >= 1 && n_cls <= 1024, "cls_ce_fwd: need B > 0 and 1 <= n_cls <= 1024");
  DPOT_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7u) == 0, "cls_ce_fwd: out must be 8-byte aligned");
  int G = 1;
  while (G < n_cls && G < 64) G <<= 1;
  hipLaunchKernelGGL(cls_ce_fwd_kernel, dim3(1), dim3(1024), 0, as_stream(stream), logits,
                     reinterpret_cast<const long long*>(labels), row_stats, out, B, n_cls, G);
  return check_launch("cls_ce_fwd_kernel");
}

extern "C" int dpot_cls_ce_bwd(const float* logits, const int64_t* labels, const float* row_stats, const float* gloss,
                               float* dlogits, int B, int n_cls, dpot_stream_t stream) {
  DPOT_REQUIRE(logits && labels && row_stats && gloss && dlogits, "cls_ce_bwd: null pointer");
  DPOT_REQUIRE(B > 0 && n_cls >= 1 && n_cls <= 1024, "cls_ce_bwd: need B > 0 and 1 <= n_cls <= 1024");
  const long long total = (long long)B * n_cls;
  long long g = (total + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(cls_ce_bwd_kernel, dim3((unsigned)g), dim3(256), 0, as_stream(stream), logits,
                     reinterpret_cast<const long long*>(labels), row_stats, gloss, dlogits, total, n_cls);
  return check_launch("cls_ce_bwd_kernel");
}

extern "C" int dpot_rel_l2_combine(const float* const* stats_ptrs, const float* stats_base, int64_t step_stride,
                                   int n_steps, int B, int C, float* out, dpot_stream_t stream) {
  DPOT_REQUIRE((stats_ptrs != nullptr) != (stats_base != nullptr), "rel_l2_combine: exactly one of stats_ptrs / stats_base");
  DPOT_REQUIRE(out && n_steps > 0 && B > 0 && C > 0 && C <= 1024, "rel_l2_combine: bad argument");
  DPOT_REQUIRE(stats_ptrs || (aligned16(stats_base) && step_stride % 4 == 0 && step_stride >= (int64_t)B * C * 4),
               "rel_l2_combine: stats_base must be 16-byte aligned, step_stride a multiple of 4 and >= B*C*4 floats");
  hipLaunchKernelGGL(rel_l2_combine_kernel, dim3(1), dim3(1024), 0, as_stream(stream), stats_ptrs, stats_base,
                     (long long)step_stride, n_steps, B, C, out);
  return check_launch("rel_l2_combine_kernel");
}

extern "C" int dpot_metrics_accum(dpot_metrics* acc, const float* l2_step, const float* l2_full, const dpot_cls_ce_out* cls,
                                  int n_cls_out, const float* sumsq, float grad_scale, int64_t samples, int64_t ar_steps,
                                  int64_t opt_steps, dpot_stream_t stream) {
  DPOT_REQUIRE(acc && (reinterpret_cast<uintptr_t>(acc) & 7u) == 0, "metrics_accum: acc must be an 8-byte aligned pointer");
  DPOT_REQUIRE(n_cls_out >= 0 && (n_cls_out == 0 || cls), "metrics_accum: n_cls_out entries need a cls pointer");
  DPOT_REQUIRE(samples >= 0 && ar_steps >= 0 && opt_steps >= 0, "metrics_accum: negative count");
  hipLaunchKernelGGL(metrics_accum_kernel, dim3(1), dim3(64), 0, as_stream(stream), acc, l2_step, l2_full, cls, n_cls_out,
                     sumsq, grad_scale, (long long)samples, (long long)ar_steps, (long long)opt_steps);
  return check_launch("metrics_accum_kernel");
}
