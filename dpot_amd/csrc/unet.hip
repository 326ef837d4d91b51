// unet.hip - the UNet baseline (models/unet.py:372-564): 3x3 convolution as an implicit GEMM on the fp32 matrix cores (forward and,
// with taps mirrored and the channel roles exchanged, the data gradient), its weight gradient split over the pixels, BatchNorm in
// training mode (Welford/Chan partials from the convolution's epilogue, merged in ascending order), the fused
// normalise + activation (+ 2x2 max pooling) and its two-launch backward, and the k = s = 2 shuffle of the transposed convolution.
//
// All fields are channels-last [B, H, W, C] fp32 and addressed as FLAT pixels p = (b H + h) W + w: a tile is a run of consecutive
// flat pixels, so it spans rows and samples alike.  A tap (dy, dx) of pixel p lives at flat pixel p + dy W + dx whenever
// 0 <= h + dy < H and 0 <= w + dx < W - the same sample then, by construction - and is zero otherwise: a 9-bit mask per pixel
// decides, the staged halo is never trusted for it.  No atomics anywhere; every sum has one fixed order.
#include "common.h"

namespace dpot {

typedef float un_f4 __attribute__((ext_vector_type(4)));

constexpr int UN_NT = 256;          // threads of every kernel here (4 waves)
constexpr int UN_MAX_W = 512;       // row length the staged halo (2 W + 2 pixels beside the tile) is sized for
constexpr int UN_MAX_C = 1 << 20;   // channels (grid.y / grid.z of the convolution kernels)

// ---- convolution -------------------------------------------------------------------------------------------------------
constexpr int CV_M = 128;   // output pixels of a workgroup: 8 MFMA row tiles, two per wave
constexpr int CV_N = 32;    // output channels of a workgroup: 2 MFMA column tiles
constexpr int CV_K = 16;    // input channels staged at a time (a K chunk): 4 MFMA k-steps per tap
constexpr int CV_KP = 20;   // LDS row stride of the staged pixels: 20 m + k hits 64 different banks for m < 16, k < 4
constexpr int CV_NP = 48;   // LDS row stride of the staged weights: 48 k + n likewise
constexpr int CV_OP = 36;   // LDS row stride of the output tile (16-byte rows)

struct ConvArgs {
  const float* x;   // [npix, Ck]
  const float* w;   // the parameter [Cout, Cin, 3, 3], read in place
  float* out;       // [npix, Cn]
  float* stats;     // [tiles, 3, Cn] count, mean, M2 of this workgroup's values per channel, or NULL
  long long npix;
  int H, W, Ck, Cn, adjoint;
};

static size_t conv_xs_floats(int W) {
  const size_t stage = (size_t)(CV_M + 2 * W + 2) * CV_KP, tile = (size_t)CV_M * CV_OP;
  return stage > tile ? stage : tile;
}

// the 9 tap bits of flat pixel p (bit 3 (dy + 1) + dx + 1), 0 beyond the field
__device__ __forceinline__ unsigned tap_mask(long long p, long long npix, int H, int W) {
  if (p >= npix) return 0u;
  const long long row = p / W;
  const int w = (int)(p - row * W), h = (int)(row % H);
  unsigned rows = 2u | (h > 0 ? 1u : 0u) | (h < H - 1 ? 4u : 0u);
  unsigned cols = 2u | (w > 0 ? 1u : 0u) | (w < W - 1 ? 4u : 0u);
  unsigned m = 0u;
#pragma unroll
  for (int r = 0; r < 3; ++r)
    if (rows >> r & 1u) m |= cols << (3 * r);
  return m;
}

template <bool VEC>
__global__ __launch_bounds__(UN_NT) void conv3x3_kernel(ConvArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, kq = lane >> 4;
  const int W = a.W, Ck = a.Ck, Cn = a.Cn;
  const long long p0 = (long long)blockIdx.x * CV_M, s0 = p0 - W - 1;
  const int n0 = blockIdx.y * CV_N;
  const int rows = CV_M + 2 * W + 2;
  float* xs = lds;
  float* wl = lds + ((size_t)rows * CV_KP > (size_t)CV_M * CV_OP ? (size_t)rows * CV_KP : (size_t)CV_M * CV_OP);

  unsigned mask[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) mask[t] = tap_mask(p0 + (wave * 2 + t) * 16 + m, a.npix, a.H, W);

  un_f4 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) acc[t][nt] = un_f4{0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < Ck; c0 += CV_K) {
    __syncthreads();   // the previous chunk has been read
    if (VEC) {
      for (int i = tid; i < rows * 4; i += UN_NT) {
        const int r = i >> 2, q = i & 3, c = c0 + q * 4;
        const long long p = s0 + r;
        un_f4 v = {0.f, 0.f, 0.f, 0.f};
        if (p >= 0 && p < a.npix && c < Ck) v = *reinterpret_cast<const un_f4*>(a.x + p * Ck + c);
        *reinterpret_cast<un_f4*>(xs + r * CV_KP + q * 4) = v;
      }
    } else {
      for (int i = tid; i < rows * CV_K; i += UN_NT) {
        const int r = i >> 4, k = i & 15, c = c0 + k;
        const long long p = s0 + r;
        xs[r * CV_KP + k] = (p >= 0 && p < a.npix && c < Ck) ? a.x[p * Ck + c] : 0.f;
      }
    }
    // weights of the chunk as wl[tap][k][n]; the parameter is [Cout, Cin, 9]: forward n = co, k = ci; the data gradient n = ci,
    // k = co with the taps mirrored.  The loop order follows the parameter's memory order in either role
    if (!a.adjoint) {
      for (int i = tid; i < CV_N * CV_K * 9; i += UN_NT) {
        const int tap = i % 9, k = (i / 9) % CV_K, n = i / (9 * CV_K);
        float v = 0.f;
        if (n0 + n < Cn && c0 + k < Ck) v = a.w[((long long)(n0 + n) * Ck + c0 + k) * 9 + tap];
        wl[(tap * CV_K + k) * CV_NP + n] = v;
      }
    } else {
      for (int i = tid; i < CV_N * CV_K * 9; i += UN_NT) {
        const int tap = i % 9, n = (i / 9) % CV_N, k = i / (9 * CV_N);
        float v = 0.f;
        if (n0 + n < Cn && c0 + k < Ck) v = a.w[((long long)(c0 + k) * Cn + n0 + n) * 9 + tap];
        wl[((8 - tap) * CV_K + k) * CV_NP + n] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int toff = (tap / 3 - 1) * W + (tap % 3 - 1) + W + 1;
#pragma unroll
      for (int kk = 0; kk < CV_K / 4; ++kk) {
        const float* wr = wl + (tap * CV_K + kk * 4 + kq) * CV_NP + m;
        const float b0 = wr[0], b1 = wr[16];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const float xv = xs[((wave * 2 + t) * 16 + m + toff) * CV_KP + kk * 4 + kq];
          const float av = (mask[t] >> tap & 1u) ? xv : 0.f;
          acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc[t][0], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc[t][1], 0, 0, 0);
        }
      }
    }
  }
  // the tile through LDS: rows go out whole (16 bytes a lane where the field allows), and the statistics read columns
  __syncthreads();
  float* ot = xs;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) ot[((wave * 2 + t) * 16 + 4 * kq + e) * CV_OP + nt * 16 + m] = acc[t][nt][e];
  __syncthreads();
  const long long left = a.npix - p0;
  const int cnt = left < CV_M ? (int)left : CV_M;
  if (VEC) {
    for (int i = tid; i < CV_M * (CV_N / 4); i += UN_NT) {
      const int q = i >> 3, c = (i & 7) * 4;
      if (q < cnt && n0 + c < Cn)
        *reinterpret_cast<un_f4*>(a.out + (p0 + q) * Cn + n0 + c) = *reinterpret_cast<const un_f4*>(ot + q * CV_OP + c);
    }
  } else {
    for (int i = tid; i < CV_M * CV_N; i += UN_NT) {
      const int q = i >> 5, c = i & 31;
      if (q < cnt && n0 + c < Cn) a.out[(p0 + q) * Cn + n0 + c] = ot[q * CV_OP + c];
    }
  }
  if (a.stats) {
    // per channel: 8 neighbouring lanes take 16 pixels each; the mean about the tile's first value, then M2 about the mean
    const int n = tid >> 3, sub = tid & 7;
    const float ref = ot[n];
    float s = 0.f;
    for (int j = 0; j < 16; ++j) {
      const int q = sub * 16 + j;
      if (q < cnt) s += ot[q * CV_OP + n] - ref;
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    const float mean = ref + s / (float)cnt;
    float m2 = 0.f;
    for (int j = 0; j < 16; ++j) {
      const int q = sub * 16 + j;
      if (q < cnt) {
        const float d = ot[q * CV_OP + n] - mean;
        m2 = fmaf(d, d, m2);
      }
    }
    m2 += __shfl_xor(m2, 1, 64);
    m2 += __shfl_xor(m2, 2, 64);
    m2 += __shfl_xor(m2, 4, 64);
    if (sub == 0 && n0 + n < Cn) {
      float* st = a.stats + (long long)blockIdx.x * 3 * Cn + n0 + n;
      st[0] = (float)cnt;
      st[Cn] = mean;
      st[2 * Cn] = m2;
    }
  }
}

// ---- BatchNorm statistics ------------------------------------------------------------------------------------------------
// Chan's merge of (n, mean, M2) with a second partial
__device__ __forceinline__ void chan_merge(float& n, float& mu, float& m2, float nb, float mb, float m2b) {
  if (nb == 0.f) return;
  const float nn = n + nb, d = mb - mu, f = nb / nn;
  mu = fmaf(d, f, mu);
  m2 = m2 + m2b + d * d * n * f;
  n = nn;
}

constexpr int BF_C = 32, BF_S = 8;   // channels and tile slices of a finalize workgroup

__global__ __launch_bounds__(UN_NT) void bn_finalize_kernel(const float* __restrict__ part, int tiles, int C,
                                                            float* __restrict__ mean, float* __restrict__ invstd,
                                                            float* __restrict__ rmean, float* __restrict__ rvar,
                                                            long long* __restrict__ nbt, float momentum, float eps) {
  __shared__ float sh[BF_S][3][BF_C];
  const int cx = threadIdx.x % BF_C, sy = threadIdx.x / BF_C, c = blockIdx.x * BF_C + cx;
  const int per = (tiles + BF_S - 1) / BF_S;
  float n = 0.f, mu = 0.f, m2 = 0.f;
  if (c < C) {
    const int t1 = (sy + 1) * per < tiles ? (sy + 1) * per : tiles;
    for (int t = sy * per; t < t1; ++t) {
      const float* st = part + (long long)t * 3 * C + c;
      chan_merge(n, mu, m2, st[0], st[C], st[2 * C]);
    }
  }
  sh[sy][0][cx] = n, sh[sy][1][cx] = mu, sh[sy][2][cx] = m2;
  __syncthreads();
  if (sy == 0 && c < C) {
    for (int s = 1; s < BF_S; ++s) chan_merge(n, mu, m2, sh[s][0][cx], sh[s][1][cx], sh[s][2][cx]);
    const float var = m2 / n;
    mean[c] = mu;
    invstd[c] = 1.0f / sqrtf(var + eps);
    if (rmean) rmean[c] = fmaf(momentum, mu - rmean[c], rmean[c]);
    if (rvar) {
      const float unbiased = m2 / (n - 1.0f);
      rvar[c] = fmaf(momentum, unbiased - rvar[c], rvar[c]);
    }
  }
  if (nbt && blockIdx.x == 0 && threadIdx.x == 0) nbt[0] += 1;
}

// ---- normalise + activation (+ pooling), forward and backward ----------------------------------------------------------------
struct BnArgs {
  const float* z;      // [npix, C] the convolution's output
  const float* mean;   // [C]
  const float* stat2;  // [C] invstd, or the variance (is_var: eval mode, the running buffers)
  const float* gamma;
  const float* beta;
  float* y;            // [npix, C]
  float* pool;         // [npix / 4, C] or NULL
  const float* dy;     // backward: gradient of y, or NULL
  const float* dpool;  // backward: gradient of the pooled field, or NULL
  float* dz;
  float* part;         // [chunks, 2, C] sum g, sum g xhat
  float* dgamma;
  float* dbeta;
  long long npix, items;   // items: windows when pooling, else pixels
  int H, W, C, act, is_var, chunks, cl;
  float eps;
};

constexpr int BN_CHUNK = 2048;   // pixels of a backward workgroup

template <int V>
struct Vec {
  float v[V];
};
template <int V>
__device__ __forceinline__ Vec<V> ldv(const float* __restrict__ p) {
  Vec<V> r;
  if constexpr (V == 4) {
    const un_f4 t = *reinterpret_cast<const un_f4*>(p);
    r.v[0] = t[0], r.v[1] = t[1], r.v[2] = t[2], r.v[3] = t[3];
  } else {
    r.v[0] = p[0];
  }
  return r;
}
template <int V>
__device__ __forceinline__ void stv(float* __restrict__ p, const Vec<V>& r) {
  if constexpr (V == 4) *reinterpret_cast<un_f4*>(p) = un_f4{r.v[0], r.v[1], r.v[2], r.v[3]};
  else p[0] = r.v[0];
}

// the per-channel constants of a lane
template <int V>
struct BnCoef {
  Vec<V> mean, invstd, gamma, beta;
};
template <int V>
__device__ __forceinline__ BnCoef<V> bn_coef(const BnArgs& a, int c) {
  BnCoef<V> k;
  k.mean = ldv<V>(a.mean + c);
  k.invstd = ldv<V>(a.stat2 + c);
  if (a.is_var)
#pragma unroll
    for (int j = 0; j < V; ++j) k.invstd.v[j] = 1.0f / sqrtf(k.invstd.v[j] + a.eps);
  k.gamma = ldv<V>(a.gamma + c);
  k.beta = ldv<V>(a.beta + c);
  return k;
}
// xhat and the pre-activation: ONE spelling, so that the backward recomputes the forward's bits
__device__ __forceinline__ float bn_xhat(float z, float mean, float invstd) { return (z - mean) * invstd; }
__device__ __forceinline__ float bn_pre(float xhat, float gamma, float beta) { return fmaf(xhat, gamma, beta); }

// flat pixel of corner (0, 0) of pooling window `wi` (windows in [b, H/2, W/2] order)
__device__ __forceinline__ long long window_pixel(long long wi, int H, int W) {
  const int Wo = W >> 1;
  const long long ro = wi / Wo;   // b * (H/2) + ho
  const int wo = (int)(wi - ro * Wo);
  return (2 * ro) * W + 2 * wo;   // (b H + 2 ho) W + 2 wo, as H is even
}
// torch's max_pool2d: the first maximum in (row, column) order, a NaN wins
__device__ __forceinline__ bool pool_takes(float v, float best) { return v > best || v != v; }

template <int V, bool POOL>
__global__ __launch_bounds__(UN_NT) void bn_act_kernel(BnArgs a) {
  const int CG = a.C / V;
  const long long idx = (long long)blockIdx.x * UN_NT + threadIdx.x;
  if (idx >= a.items * CG) return;
  const int c = (int)(idx % CG) * V;
  const long long it = idx / CG;
  const BnCoef<V> k = bn_coef<V>(a, c);
  if (!POOL) {
    const Vec<V> z = ldv<V>(a.z + it * a.C + c);
    Vec<V> y;
#pragma unroll
    for (int j = 0; j < V; ++j)
      y.v[j] = act_fwd(a.act, bn_pre(bn_xhat(z.v[j], k.mean.v[j], k.invstd.v[j]), k.gamma.v[j], k.beta.v[j]));
    stv<V>(a.y + it * a.C + c, y);
  } else {
    const long long p00 = window_pixel(it, a.H, a.W);
    Vec<V> best;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long p = p00 + (q >> 1) * a.W + (q & 1);
      const Vec<V> z = ldv<V>(a.z + p * a.C + c);
      Vec<V> y;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        y.v[j] = act_fwd(a.act, bn_pre(bn_xhat(z.v[j], k.mean.v[j], k.invstd.v[j]), k.gamma.v[j], k.beta.v[j]));
        if (q == 0 || pool_takes(y.v[j], best.v[j])) best.v[j] = y.v[j];
      }
      stv<V>(a.y + p * a.C + c, y);
    }
    stv<V>(a.pool + it * a.C + c, best);
  }
}

// g = (dy + the pooled gradient at the window's first maximum) act'(pre) and xhat of the 1 (pixel) or 4 (window) positions of an
// item, recomputed from z: what the reduce and the apply kernel share
template <int V, bool POOL>
struct BnItem {
  static constexpr int Q = POOL ? 4 : 1;
  long long p[Q];
  Vec<V> g[Q], xh[Q];
};
template <int V, bool POOL>
__device__ __forceinline__ void bn_item(const BnArgs& a, const BnCoef<V>& k, long long it, int c, BnItem<V, POOL>& o) {
  constexpr int Q = BnItem<V, POOL>::Q;
  const long long p00 = POOL ? window_pixel(it, a.H, a.W) : it;
  Vec<V> pre[Q], best;
  int arg[V];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    o.p[q] = p00 + (q >> 1) * a.W + (q & 1);
    const Vec<V> z = ldv<V>(a.z + o.p[q] * a.C + c);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      o.xh[q].v[j] = bn_xhat(z.v[j], k.mean.v[j], k.invstd.v[j]);
      pre[q].v[j] = bn_pre(o.xh[q].v[j], k.gamma.v[j], k.beta.v[j]);
      if (POOL && a.dpool) {
        const float y = act_fwd(a.act, pre[q].v[j]);
        if (q == 0 || pool_takes(y, best.v[j])) best.v[j] = y, arg[j] = q;
      }
    }
  }
  Vec<V> dp;
  if (POOL && a.dpool) dp = ldv<V>(a.dpool + it * a.C + c);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    Vec<V> d;
    if (a.dy) d = ldv<V>(a.dy + o.p[q] * a.C + c);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float up = a.dy ? d.v[j] : 0.f;
      if (POOL && a.dpool && arg[j] == q) up += dp.v[j];
      o.g[q].v[j] = up * act_bwd(a.act, pre[q].v[j]);
    }
  }
}

// threads of a backward workgroup: cl channel lanes (V channels each) times UN_NT / cl item lanes; a workgroup owns the items
// [chunk * per, (chunk + 1) * per) and the channel lanes [blockIdx.y * cl, ...)
template <int V, bool POOL>
__global__ __launch_bounds__(UN_NT) void bn_bwd_reduce_kernel(BnArgs a) {
  __shared__ float sh[UN_NT * 2 * V];
  const int cl = a.cl, pl = UN_NT / cl, lc = threadIdx.x % cl, lp = threadIdx.x / cl;
  const int c = (blockIdx.y * cl + lc) * V;
  const int per = POOL ? BN_CHUNK / 4 : BN_CHUNK;
  const long long i0 = (long long)blockIdx.x * per;
  const long long i1 = i0 + per < a.items ? i0 + per : a.items;
  float sg[V], sx[V];
#pragma unroll
  for (int j = 0; j < V; ++j) sg[j] = sx[j] = 0.f;
  if (c < a.C) {
    const BnCoef<V> k = bn_coef<V>(a, c);
    for (long long it = i0 + lp; it < i1; it += pl) {
      BnItem<V, POOL> o;
      bn_item<V, POOL>(a, k, it, c, o);
#pragma unroll
      for (int q = 0; q < BnItem<V, POOL>::Q; ++q)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          sg[j] += o.g[q].v[j];
          sx[j] = fmaf(o.g[q].v[j], o.xh[q].v[j], sx[j]);
        }
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    sh[(threadIdx.x * 2 + 0) * V + j] = sg[j];
    sh[(threadIdx.x * 2 + 1) * V + j] = sx[j];
  }
  __syncthreads();
  if (lp == 0 && c < a.C) {
    for (int s = 1; s < pl; ++s)
#pragma unroll
      for (int j = 0; j < V; ++j) {
        sg[j] += sh[((s * cl + lc) * 2 + 0) * V + j];
        sx[j] += sh[((s * cl + lc) * 2 + 1) * V + j];
      }
    float* out = a.part + (long long)blockIdx.x * 2 * a.C + c;
#pragma unroll
    for (int j = 0; j < V; ++j) out[j] = sg[j], out[a.C + j] = sx[j];
  }
}

template <int V, bool POOL>
__global__ __launch_bounds__(UN_NT) void bn_bwd_apply_kernel(BnArgs a) {
  __shared__ float sh[UN_NT * 2 * V];
  const int cl = a.cl, pl = UN_NT / cl, lc = threadIdx.x % cl, lp = threadIdx.x / cl;
  const int c = (blockIdx.y * cl + lc) * V;
  const bool live = c < a.C;
  // the partials of all chunks: item lane lp sums its slice in ascending order, then every lane adds the slices in ascending order
  float sg[V], sx[V];
#pragma unroll
  for (int j = 0; j < V; ++j) sg[j] = sx[j] = 0.f;
  const int slice = (a.chunks + pl - 1) / pl;
  if (live) {
    const int k1 = (lp + 1) * slice < a.chunks ? (lp + 1) * slice : a.chunks;
    for (int kk = lp * slice; kk < k1; ++kk) {
      const float* in = a.part + (long long)kk * 2 * a.C + c;
#pragma unroll
      for (int j = 0; j < V; ++j) sg[j] += in[j], sx[j] += in[a.C + j];
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    sh[(threadIdx.x * 2 + 0) * V + j] = sg[j];
    sh[(threadIdx.x * 2 + 1) * V + j] = sx[j];
  }
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int j = 0; j < V; ++j) sg[j] = sx[j] = 0.f;
  for (int s = 0; s < pl; ++s)
#pragma unroll
    for (int j = 0; j < V; ++j) {
      sg[j] += sh[((s * cl + lc) * 2 + 0) * V + j];
      sx[j] += sh[((s * cl + lc) * 2 + 1) * V + j];
    }
  if (blockIdx.x == 0 && lp == 0) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (a.dbeta) a.dbeta[c + j] = sg[j];
      if (a.dgamma) a.dgamma[c + j] = sx[j];
    }
  }
  const BnCoef<V> k = bn_coef<V>(a, c);
  const float inv_n = 1.0f / (float)a.npix;
  float mg[V], mx[V], sc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) mg[j] = sg[j] * inv_n, mx[j] = sx[j] * inv_n, sc[j] = k.gamma.v[j] * k.invstd.v[j];
  const int per = POOL ? BN_CHUNK / 4 : BN_CHUNK;
  const long long i0 = (long long)blockIdx.x * per;
  const long long i1 = i0 + per < a.items ? i0 + per : a.items;
  for (long long it = i0 + lp; it < i1; it += pl) {
    BnItem<V, POOL> o;
    bn_item<V, POOL>(a, k, it, c, o);
#pragma unroll
    for (int q = 0; q < BnItem<V, POOL>::Q; ++q) {
      Vec<V> d;
#pragma unroll
      for (int j = 0; j < V; ++j) d.v[j] = sc[j] * (o.g[q].v[j] - mg[j] - o.xh[q].v[j] * mx[j]);
      stv<V>(a.dz + o.p[q] * a.C + c, d);
    }
  }
}

// ---- weight gradient -----------------------------------------------------------------------------------------------------
constexpr int WG_P = 128;    // pixels of a sub-tile: 32 per wave, 8 MFMA k-steps
constexpr int WG_CO = 32;    // output channels of a workgroup (2 MFMA row tiles)
constexpr int WG_CI = 16;    // input channels of a workgroup (1 MFMA column tile)
constexpr int WG_XP = 16;    // LDS row stride of the staged x: 16 k + n hits 64 banks
constexpr int WG_DP = 48;    // LDS row stride of the staged dy: 48 k + m likewise

struct WgradArgs {
  const float* x;    // [npix, Cin]
  const float* dy;   // [npix, Cout]
  float* ws;         // [chunks, Cout, Cin, 9]
  long long npix;
  int H, W, Cin, Cout, nsub, subtiles;
};

static void wgrad_plan(long long npix, int Cin, int Cout, int* nsub, int* chunks) {
  const long long total = cdiv64(npix, WG_P);
  const long long blocks = (long long)cdiv(Cout, WG_CO) * cdiv(Cin, WG_CI);
  const long long target = blocks >= 1024 ? 1 : 1024 / blocks;
  const long long ns = cdiv64(total, target);
  *nsub = (int)ns;
  *chunks = (int)cdiv64(total, ns);
}

template <bool VEC>
__global__ __launch_bounds__(UN_NT) void conv3x3_wgrad_kernel(WgradArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, kq = lane >> 4;
  const int W = a.W, Cin = a.Cin, Cout = a.Cout;
  const int co0 = blockIdx.y * WG_CO, ci0 = blockIdx.z * WG_CI;
  const int rows = WG_P + 2 * W + 2;
  float* xs = lds;                                  // [rows][WG_XP]
  float* ds = xs + (size_t)rows * WG_XP;            // [WG_P][WG_DP]; afterwards the cross-wave sum [18][64][4]
  unsigned* vm = reinterpret_cast<unsigned*>(ds + WG_P * WG_DP);   // [WG_P] tap masks

  un_f4 acc[2][9];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc[ct][tap] = un_f4{0.f, 0.f, 0.f, 0.f};

  const int t0 = blockIdx.x * a.nsub;
  const int t1 = t0 + a.nsub < a.subtiles ? t0 + a.nsub : a.subtiles;
  for (int st = t0; st < t1; ++st) {
    const long long p0 = (long long)st * WG_P, s0 = p0 - W - 1;
    __syncthreads();
    if (VEC) {
      for (int i = tid; i < rows * 4; i += UN_NT) {
        const int r = i >> 2, c = ci0 + (i & 3) * 4;
        const long long p = s0 + r;
        un_f4 v = {0.f, 0.f, 0.f, 0.f};
        if (p >= 0 && p < a.npix && c < Cin) v = *reinterpret_cast<const un_f4*>(a.x + p * Cin + c);
        *reinterpret_cast<un_f4*>(xs + r * WG_XP + (i & 3) * 4) = v;
      }
      for (int i = tid; i < WG_P * 8; i += UN_NT) {
        const int q = i >> 3, c = co0 + (i & 7) * 4;
        const long long p = p0 + q;
        un_f4 v = {0.f, 0.f, 0.f, 0.f};
        if (p < a.npix && c < Cout) v = *reinterpret_cast<const un_f4*>(a.dy + p * Cout + c);
        *reinterpret_cast<un_f4*>(ds + q * WG_DP + (i & 7) * 4) = v;
      }
    } else {
      for (int i = tid; i < rows * WG_CI; i += UN_NT) {
        const int r = i >> 4, c = ci0 + (i & 15);
        const long long p = s0 + r;
        xs[r * WG_XP + (i & 15)] = (p >= 0 && p < a.npix && c < Cin) ? a.x[p * Cin + c] : 0.f;
      }
      for (int i = tid; i < WG_P * WG_CO; i += UN_NT) {
        const int q = i >> 5, c = co0 + (i & 31);
        const long long p = p0 + q;
        ds[q * WG_DP + (i & 31)] = (p < a.npix && c < Cout) ? a.dy[p * Cout + c] : 0.f;
      }
    }
    if (tid < WG_P) vm[tid] = tap_mask(p0 + tid, a.npix, a.H, W);
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < WG_P / 16; ++j) {
      const int q = wave * (WG_P / 4) + j * 4 + kq;
      const unsigned mk = vm[q];
      const float a0 = ds[q * WG_DP + m], a1 = ds[q * WG_DP + 16 + m];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int toff = (tap / 3 - 1) * W + (tap % 3 - 1) + W + 1;
        const float xv = xs[(q + toff) * WG_XP + m];
        const float bv = (mk >> tap & 1u) ? xv : 0.f;
        acc[0][tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, acc[0][tap], 0, 0, 0);
        acc[1][tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, acc[1][tap], 0, 0, 0);
      }
    }
  }
  // the four waves' sums, wave 0 first
  un_f4* red = reinterpret_cast<un_f4*>(ds);
  for (int wv = 0; wv < 4; ++wv) {
    __syncthreads();
    if (wave == wv) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          un_f4* r = red + (ct * 9 + tap) * 64 + lane;
          *r = wv == 0 ? acc[ct][tap] : *r + acc[ct][tap];
        }
    }
  }
  __syncthreads();
  const float* rf = reinterpret_cast<const float*>(red);
  float* out = a.ws + (long long)blockIdx.x * Cout * Cin * 9;
  for (int i = tid; i < WG_CO * WG_CI * 9; i += UN_NT) {
    const int tap = i % 9, ci = (i / 9) % WG_CI, co = i / (9 * WG_CI);
    if (co0 + co < Cout && ci0 + ci < Cin) {
      const int ct = co >> 4, kq2 = (co & 15) >> 2, e = co & 3;
      out[((long long)(co0 + co) * Cin + ci0 + ci) * 9 + tap] = rf[(((ct * 9 + tap) * 64) + kq2 * 16 + ci) * 4 + e];
    }
  }
}

__global__ __launch_bounds__(UN_NT) void conv3x3_wgrad_finish_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                                     long long n, int chunks, int accumulate) {
  const long long i = (long long)blockIdx.x * UN_NT + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int k = 0; k < chunks; ++k) s += ws[(long long)k * n + i];
  dw[i] = accumulate ? dw[i] + s : s;   // the same sum as a plain write, then one add
}

// ---- the k = s = 2 transposed convolution's shuffle ------------------------------------------------------------------------
// z [B h w, C 4] with columns (c, i, j), the order of the parameter [Cin, C, 2, 2] read as a [Cin, 4 C] matrix
//   forward: out[b, 2 hy + i, 2 wx + j, c] = z[(b, hy, wx), 4 c + 2 i + j] + bias[c];   inverse: the gather back, no bias
__global__ __launch_bounds__(UN_NT) void upshuffle_kernel(const float* __restrict__ src, const float* __restrict__ bias,
                                                          float* __restrict__ dst, int h, int w, int C, int inverse,
                                                          long long total) {
  const long long idx = (long long)blockIdx.x * UN_NT + threadIdx.x;   // enumerates the image [b, 2h, 2w, C]
  if (idx >= total) return;
  const int c = (int)(idx % C);
  long long r = idx / C;
  const int X = (int)(r % (2 * w));
  r /= 2 * w;
  const int Y = (int)(r % (2 * h));
  const long long b = r / (2 * h);
  const long long zi = (((b * h + (Y >> 1)) * w + (X >> 1)) * C + c) * 4 + (Y & 1) * 2 + (X & 1);
  if (inverse) dst[zi] = src[idx];
  else dst[idx] = src[zi] + (bias ? bias[c] : 0.f);
}

static int unet_check_field(const char* what, int B, int H, int W, long long* npix) {
  DPOT_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad sizes B=%d field %dx%d", what, B, H, W);
  *npix = (long long)B * H * W;
  DPOT_REQUIRE(*npix <= ((long long)1 << 36), "%s: B H W = %lld pixels is beyond 2^36", what, *npix);
  return DPOT_OK;
}

static int unet_check_conv(const char* what, int B, int H, int W, int Cin, int Cout, long long* npix) {
  if (int rc = unet_check_field(what, B, H, W, npix)) return rc;
  DPOT_REQUIRE(Cin > 0 && Cout > 0, "%s: bad channels Cin=%d Cout=%d", what, Cin, Cout);
  if (W > UN_MAX_W || Cin > UN_MAX_C || Cout > UN_MAX_C) {
    set_error("%s: field %dx%d with %d -> %d channels is beyond the staged halo of a workgroup (W <= %d) or the grid (channels <= %d)",
              what, H, W, Cin, Cout, UN_MAX_W, UN_MAX_C);
    return DPOT_EUNSUP;
  }
  DPOT_REQUIRE(cdiv64(*npix, CV_M) <= 0x7fffffff, "%s: too many pixel tiles", what);
  return DPOT_OK;
}

static int bn_fill(const char* what, BnArgs& a, int B, int H, int W, int C, int act, bool pool) {
  if (int rc = unet_check_field(what, B, H, W, &a.npix)) return rc;
  DPOT_REQUIRE(C > 0, "%s: bad channel count %d", what, C);
  DPOT_REQUIRE(act >= DPOT_ACT_NONE && act <= DPOT_ACT_SILU, "%s: unknown activation %d", what, act);
  DPOT_REQUIRE(!pool || (H % 2 == 0 && W % 2 == 0), "%s: 2x2 pooling needs an even field, got %dx%d", what, H, W);
  a.H = H, a.W = W, a.C = C, a.act = act;
  a.items = pool ? a.npix / 4 : a.npix;
  return DPOT_OK;
}

// channel lanes of a backward workgroup: the power of two >= the channel groups, at most 64
static int bn_lanes(int groups) {
  int cl = 1;
  while (cl < groups && cl < 64) cl *= 2;
  return cl;
}

template <int V, bool POOL>
static int bn_bwd_launch(bool apply, BnArgs& a, hipStream_t s) {
  const int groups = a.C / V;
  a.cl = bn_lanes(groups);
  const dim3 grid((unsigned)a.chunks, (unsigned)cdiv(groups, a.cl));
  if (apply) hipLaunchKernelGGL((bn_bwd_apply_kernel<V, POOL>), grid, dim3(UN_NT), 0, s, a);
  else hipLaunchKernelGGL((bn_bwd_reduce_kernel<V, POOL>), grid, dim3(UN_NT), 0, s, a);
  return check_launch(apply ? "bn_bwd_apply_kernel" : "bn_bwd_reduce_kernel");
}

static int bn_bwd(const char* what, bool apply, const float* dy, const float* dpool, const float* z, const float* mean,
                  const float* invstd, const float* gamma, const float* beta, float* part, float* dz, float* dgamma,
                  float* dbeta, int B, int H, int W, int C, int act, dpot_stream_t stream) {
  DPOT_REQUIRE((dy || dpool) && z && mean && invstd && gamma && beta && part, "%s: null pointer", what);
  DPOT_REQUIRE(!apply || (dz && dz != z && dz != dy), "%s: null or aliased dz", what);
  BnArgs a = {};
  const bool pool = dpool != nullptr;
  if (int rc = bn_fill(what, a, B, H, W, C, act, pool)) return rc;
  a.dy = dy, a.dpool = dpool, a.z = z, a.mean = mean, a.stat2 = invstd, a.gamma = gamma, a.beta = beta;
  a.part = part, a.dz = dz, a.dgamma = dgamma, a.dbeta = dbeta;
  const long long chunks = cdiv64(a.npix, BN_CHUNK);
  DPOT_REQUIRE(chunks <= 0x7fffffff, "%s: too many chunks", what);
  a.chunks = (int)chunks;
  const bool vec = C % 4 == 0 && aligned16(dy) && aligned16(dpool) && aligned16(z) && aligned16(dz) && aligned16(mean) &&
                   aligned16(invstd) && aligned16(gamma) && aligned16(beta);
  const hipStream_t s = as_stream(stream);
  if (vec) return pool ? bn_bwd_launch<4, true>(apply, a, s) : bn_bwd_launch<4, false>(apply, a, s);
  return pool ? bn_bwd_launch<1, true>(apply, a, s) : bn_bwd_launch<1, false>(apply, a, s);
}

}  // namespace dpot

using namespace dpot;

extern "C" int dpot_unet_max_size(int channels) { return channels ? UN_MAX_C : UN_MAX_W; }

extern "C" int64_t dpot_conv3x3_stats_elems(int64_t npix, int Cout) {
  if (npix <= 0 || Cout <= 0) return 0;
  return cdiv64(npix, CV_M) * 3 * Cout;
}

extern "C" int dpot_conv3x3(const float* x, const float* w, float* out, float* stats, int B, int H, int W, int Cin, int Cout,
                            int adjoint, dpot_stream_t stream) {
  DPOT_REQUIRE(x && w && out && x != out, "conv3x3: null or aliased pointer");
  DPOT_REQUIRE(!(adjoint && stats), "conv3x3: the data gradient takes no statistics");
  ConvArgs a = {};
  if (int rc = unet_check_conv("conv3x3", B, H, W, Cin, Cout, &a.npix)) return rc;
  a.x = x, a.w = w, a.out = out, a.stats = stats, a.H = H, a.W = W, a.adjoint = adjoint ? 1 : 0;
  a.Ck = adjoint ? Cout : Cin, a.Cn = adjoint ? Cin : Cout;
  const size_t lds = sizeof(float) * (conv_xs_floats(W) + (size_t)9 * CV_K * CV_NP);
  const dim3 grid((unsigned)cdiv64(a.npix, CV_M), (unsigned)cdiv(a.Cn, CV_N));
  const bool vec = a.Ck % 4 == 0 && a.Cn % 4 == 0 && aligned16(x) && aligned16(out);
  if (vec) {
    if (int rc = raise_dynamic_lds<conv3x3_kernel<true>>("conv3x3")) return rc;
    hipLaunchKernelGGL(conv3x3_kernel<true>, grid, dim3(UN_NT), lds, as_stream(stream), a);
  } else {
    if (int rc = raise_dynamic_lds<conv3x3_kernel<false>>("conv3x3")) return rc;
    hipLaunchKernelGGL(conv3x3_kernel<false>, grid, dim3(UN_NT), lds, as_stream(stream), a);
  }
  return check_launch("conv3x3_kernel");
}

extern "C" int dpot_bn_finalize(const float* stats, int64_t npix, int C, float* mean, float* invstd, float* running_mean,
                                float* running_var, void* num_batches_tracked, float momentum, float eps,
                                dpot_stream_t stream) {
  DPOT_REQUIRE(stats && mean && invstd && npix > 0 && C > 0, "bn_finalize: null pointer or bad sizes");
  const long long tiles = cdiv64(npix, CV_M);
  DPOT_REQUIRE(tiles <= 0x7fffffff, "bn_finalize: too many tiles");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, BF_C)), dim3(UN_NT), 0, as_stream(stream), stats, (int)tiles, C, mean,
                     invstd, running_mean, running_var, static_cast<long long*>(num_batches_tracked), momentum, eps);
  return check_launch("bn_finalize_kernel");
}

extern "C" int dpot_bn_act(const float* z, const float* mean, const float* stat2, const float* gamma, const float* beta,
                           float* y, float* pool, int B, int H, int W, int C, int act, int stat_is_var, float eps,
                           dpot_stream_t stream) {
  DPOT_REQUIRE(z && mean && stat2 && gamma && beta && y && y != z && pool != y, "bn_act: null or aliased pointer");
  BnArgs a = {};
  if (int rc = bn_fill("bn_act", a, B, H, W, C, act, pool != nullptr)) return rc;
  a.z = z, a.mean = mean, a.stat2 = stat2, a.gamma = gamma, a.beta = beta, a.y = y, a.pool = pool;
  a.is_var = stat_is_var ? 1 : 0, a.eps = eps;
  const bool vec = C % 4 == 0 && aligned16(z) && aligned16(y) && aligned16(pool) && aligned16(mean) && aligned16(stat2) &&
                   aligned16(gamma) && aligned16(beta);
  const long long blocks = cdiv64(a.items * (vec ? C / 4 : C), UN_NT);
  DPOT_REQUIRE(blocks <= 0x7fffffff, "bn_act: too many workgroups");
  const dim3 grid((unsigned)blocks);
  const hipStream_t s = as_stream(stream);
  if (pool) {
    if (vec) hipLaunchKernelGGL((bn_act_kernel<4, true>), grid, dim3(UN_NT), 0, s, a);
    else hipLaunchKernelGGL((bn_act_kernel<1, true>), grid, dim3(UN_NT), 0, s, a);
  } else {
    if (vec) hipLaunchKernelGGL((bn_act_kernel<4, false>), grid, dim3(UN_NT), 0, s, a);
    else hipLaunchKernelGGL((bn_act_kernel<1, false>), grid, dim3(UN_NT), 0, s, a);
  }
  return check_launch("bn_act_kernel");
}

extern "C" int64_t dpot_bn_act_bwd_ws_elems(int64_t npix, int C) {
  if (npix <= 0 || C <= 0) return 0;
  return cdiv64(npix, BN_CHUNK) * 2 * C;
}

extern "C" int dpot_bn_act_bwd_reduce(const float* dy, const float* dpool, const float* z, const float* mean,
                                      const float* invstd, const float* gamma, const float* beta, float* part, int B, int H,
                                      int W, int C, int act, dpot_stream_t stream) {
  return bn_bwd("bn_act_bwd_reduce", false, dy, dpool, z, mean, invstd, gamma, beta, part, nullptr, nullptr, nullptr, B, H, W,
                C, act, stream);
}

extern "C" int dpot_bn_act_bwd_apply(const float* dy, const float* dpool, const float* z, const float* mean,
                                     const float* invstd, const float* gamma, const float* beta, const float* part, float* dz,
                                     float* dgamma, float* dbeta, int B, int H, int W, int C, int act, dpot_stream_t stream) {
  return bn_bwd("bn_act_bwd_apply", true, dy, dpool, z, mean, invstd, gamma, beta, const_cast<float*>(part), dz, dgamma, dbeta,
                B, H, W, C, act, stream);
}

extern "C" int64_t dpot_conv3x3_wgrad_ws_elems(int64_t npix, int Cin, int Cout) {
  if (npix <= 0 || Cin <= 0 || Cout <= 0) return 0;
  int nsub, chunks;
  wgrad_plan(npix, Cin, Cout, &nsub, &chunks);
  return (int64_t)chunks * Cout * Cin * 9;
}

extern "C" int dpot_conv3x3_wgrad(const float* x, const float* dy, float* dw, float* ws, int B, int H, int W, int Cin,
                                  int Cout, int accumulate, dpot_stream_t stream) {
  DPOT_REQUIRE(x && dy && dw && ws && ws != dw, "conv3x3_wgrad: null or aliased pointer");
  WgradArgs a = {};
  if (int rc = unet_check_conv("conv3x3_wgrad", B, H, W, Cin, Cout, &a.npix)) return rc;
  int chunks;
  wgrad_plan(a.npix, Cin, Cout, &a.nsub, &chunks);
  a.x = x, a.dy = dy, a.ws = ws, a.H = H, a.W = W, a.Cin = Cin, a.Cout = Cout;
  a.subtiles = (int)cdiv64(a.npix, WG_P);
  const size_t lds = sizeof(float) * ((size_t)(WG_P + 2 * W + 2) * WG_XP + (size_t)WG_P * WG_DP + WG_P);
  const dim3 grid((unsigned)chunks, (unsigned)cdiv(Cout, WG_CO), (unsigned)cdiv(Cin, WG_CI));
  DPOT_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "conv3x3_wgrad: too many channel blocks");
  const bool vec = Cin % 4 == 0 && Cout % 4 == 0 && aligned16(x) && aligned16(dy);
  if (vec) {
    if (int rc = raise_dynamic_lds<conv3x3_wgrad_kernel<true>>("conv3x3_wgrad")) return rc;
    hipLaunchKernelGGL(conv3x3_wgrad_kernel<true>, grid, dim3(UN_NT), lds, as_stream(stream), a);
  } else {
    if (int rc = raise_dynamic_lds<conv3x3_wgrad_kernel<false>>("conv3x3_wgrad")) return rc;
    hipLaunchKernelGGL(conv3x3_wgrad_kernel<false>, grid, dim3(UN_NT), lds, as_stream(stream), a);
  }
  if (int rc = check_launch("conv3x3_wgrad_kernel")) return rc;
  const long long n = (long long)Cout * Cin * 9;
  hipLaunchKernelGGL(conv3x3_wgrad_finish_kernel, dim3((unsigned)cdiv64(n, UN_NT)), dim3(UN_NT), 0, as_stream(stream), ws, dw, n,
                     chunks, accumulate ? 1 : 0);
  return check_launch("conv3x3_wgrad_finish_kernel");
}

extern "C" int dpot_unet_upshuffle(const float* src, const float* bias, float* dst, int B, int h, int w, int C, int inverse,
                                   dpot_stream_t stream) {
  DPOT_REQUIRE(src && dst && src != dst && B > 0 && h > 0 && w > 0 && C > 0, "unet_upshuffle: bad argument");
  const long long total = (long long)B * h * w * 4 * C;
  const long long blocks = cdiv64(total, UN_NT);
  DPOT_REQUIRE(blocks <= 0x7fffffff, "unet_upshuffle: too many workgroups");
  hipLaunchKernelGGL(upshuffle_kernel, dim3((unsigned)blocks), dim3(UN_NT), 0, as_stream(stream), src, bias, dst, h, w, C,
                     inverse ? 1 : 0, total);
  return check_launch("upshuffle_kernel");
}
