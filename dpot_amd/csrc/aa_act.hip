// aa_act.hip - the anti-aliased activation of the reference's CDPOT model (models/filter_networks.py:481-518, LReLu_torch):
// an activation applied above the sampling rate.  For a channels-last field x[N, h, w, C]
//
//   y[n, :, :, c] = V_h D_h lrelu( U_h x[n, :, :, c] U_w^T ) D_w^T V_w^T + bias[c % Cb]
//
// U: bilinear n -> 2n (2 taps per axis), D: anti-aliased bilinear 2n -> n (at most 4 taps), V: bilinear n -> H (2 taps; only with
// an output size).  torch applies the three resizes separably, so the dense form is exact.  The tap tables - index and weight per
// output coordinate, and their transposes for the gather-form adjoints - are built on the host in float64, rounded to fp32 and
// uploaded once per size tuple (dpot_amd/ops.py AAPlan); the kernels copy them to LDS.
//
// Four kernels, every one free of atomics, with a fixed summation order, reading nothing outside the tensors:
//   aa_core_fwd   z = D lrelu(U x U^T) D^T (+ bias when there is no V).  One workgroup per (n, chunk of CHW channels) holds the
//                 h x w plane of its channels in LDS; an item is (pixel, 4 channels), channels fastest, so a lane group reads
//                 and writes CHW contiguous floats of a pixel.  The 2h x 2w up-sampled values live in registers only: each z
//                 element evaluates its 4 x 4 of them from the 2 x 2 x-taps of each.
//   aa_core_bwd   dx = U^T [ lrelu'(U x U^T) . (D^T g D) ] U from the planes of x and g in LDS, the up-sampled field recomputed
//                 per element as in the forward (lrelu' = 1 where it is > 0, the slope elsewhere, also at exactly 0), and the
//                 bias partials part[n, c] = sum over pixels of g (rows of V sum to 1, so sum g = sum dy; ops.colsum finishes).
//   aa_up_fwd     y = V z V^T + bias: an item per (output pixel, 4 channels), written once with 16-byte stores.
//   aa_up_adj     g = V^T dy V: one workgroup per (n, latent row, channel chunk) sums its <= 2 H/h + 1 weighted dy rows into an
//                 LDS row [W][CHW] (coalesced reads, each dy element is read by two latent rows), then contracts the columns.
// 16-byte loads and stores when C % 4 == 0 and the pointers are 16-byte aligned, scalar ones otherwise (C = 35 in DPOT-Tiny).
#include "common.h"

namespace dpot {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int AA_MAX = 64;                // latent size per axis
constexpr int AA_OUT_MAX = 1024;          // output size per axis
constexpr int AA_THREADS = 256;
constexpr int AA_LDS_BUDGET = 64 * 1024;  // planes of a workgroup, where a narrower channel chunk can meet it

// word offsets of one axis' tables inside the core table block (32 n words per axis; axis h first, then axis w)
struct AaAxis {
  const int* ui;     // [2n][2]  U taps: input index
  const float* uw;   // [2n][2]
  const int* di;     // [n][4]   D taps: index into the 2n up-sampled values
  const float* dw;   // [n][4]
  const int* uti;    // [n][4]   U^T: the up-sampled values an input feeds
  const float* utw;  // [n][4]
  const int* dti;    // [2n][2]  D^T: the outputs an up-sampled value feeds
  const float* dtw;  // [2n][2]
};
__device__ __forceinline__ AaAxis aa_axis(const int* base, int n) {
  AaAxis t;
  t.ui = base, t.uw = reinterpret_cast<const float*>(base + 4 * n);
  t.di = base + 8 * n, t.dw = reinterpret_cast<const float*>(base + 12 * n);
  t.uti = base + 16 * n, t.utw = reinterpret_cast<const float*>(base + 20 * n);
  t.dti = base + 24 * n, t.dtw = reinterpret_cast<const float*>(base + 28 * n);
  return t;
}

struct AaCoreArgs {
  const float* x;
  const float* g;      // backward: the gradient at the latent size
  const float* bias;   // forward: may be NULL
  float* out;          // forward: z / y; backward: dx
  float* part;         // backward: [N][C] bias partials
  const int* tab;
  int N, h, w, C, Cb, lg_chw, nchunk;
  float slope;
};

template <bool VEC>
__device__ __forceinline__ f32x4 aa_ld4(const float* __restrict__ p, int nv) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    v = *reinterpret_cast<const f32x4*>(p);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nv) v[k] = p[k];
  }
  return v;
}
template <bool VEC>
__device__ __forceinline__ void aa_st4(float* __restrict__ p, f32x4 v, int nv) {
  if (VEC) {
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nv) p[k] = v[k];
  }
}
__device__ __forceinline__ f32x4 aa_bias4(const float* __restrict__ bias, int c, int C, int Cb) {
  f32x4 b = {0.f, 0.f, 0.f, 0.f};
  if (bias) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c + k < C) b[k] = bias[(c + k) % Cb];
  }
  return b;
}

// the tables, then one plane [h*w][CHW] of the workgroup's channels (zero beyond C)
template <bool VEC>
__device__ __forceinline__ void aa_load_plane(f32x4* __restrict__ P, const float* __restrict__ src, int npix, int C, int c0,
                                              int lg_nc4) {
  const int nc4 = 1 << lg_nc4;
  for (int idx = threadIdx.x; idx < npix * nc4; idx += AA_THREADS) {
    const int c = c0 + 4 * (idx & (nc4 - 1));
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (c < C) v = aa_ld4<VEC>(src + (size_t)(idx >> lg_nc4) * C + c, C - c);
    P[idx] = v;
  }
}

// u(a, b) = sum of the 2 x 2 x-taps of one up-sampled value, for the 4 channels of an item
__device__ __forceinline__ f32x4 aa_up_value(const f32x4* __restrict__ X, const AaAxis& th, const AaAxis& tw, int a, int b, int w,
                                             int lg_nc4, int c4) {
  f32x4 u = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kp = 0; kp < 2; ++kp) {
    const int p = th.ui[2 * a + kp];
    const float wp = th.uw[2 * a + kp];
#pragma unroll
    for (int kq = 0; kq < 2; ++kq) {
      const int q = tw.ui[2 * b + kq];
      const float wq = wp * tw.uw[2 * b + kq];
      const f32x4 xv = X[((p * w + q) << lg_nc4) + c4];
      u += wq * xv;
    }
  }
  return u;
}

template <bool VEC>
__global__ __launch_bounds__(AA_THREADS) void aa_core_fwd_kernel(const AaCoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) int aa_lds[];
  const int h = a.h, w = a.w, C = a.C, ntab = 32 * (h + w), npix = h * w;
  const int lg_nc4 = a.lg_chw - 2, nc4 = 1 << lg_nc4;
  const int n = blockIdx.x / a.nchunk, c0 = (blockIdx.x % a.nchunk) << a.lg_chw;
  for (int i = threadIdx.x; i < ntab; i += AA_THREADS) aa_lds[i] = a.tab[i];
  f32x4* X = reinterpret_cast<f32x4*>(aa_lds + ntab);
  aa_load_plane<VEC>(X, a.x + (size_t)n * npix * C, npix, C, c0, lg_nc4);
  __syncthreads();
  const AaAxis th = aa_axis(aa_lds, h), tw = aa_axis(aa_lds + 32 * h, w);
  float* __restrict__ out = a.out + (size_t)n * npix * C;
  for (int idx = threadIdx.x; idx < npix * nc4; idx += AA_THREADS) {
    const int c4 = idx & (nc4 - 1), pix = idx >> lg_nc4, c = c0 + 4 * c4;
    if (c >= C) continue;
    const int i = pix / w, j = pix - i * w;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // the outer tap loop stays rolled: unrolled, all 64 LDS reads are in flight at once (256 VGPR, one wave per SIMD) and the
    // launch is 1.6x slower at [32, 16, 16, 350]; rolled: 96 VGPR, five waves per SIMD, the same order of additions
#pragma unroll 1
    for (int ka = 0; ka < 4; ++ka) {
      const int ua = th.di[4 * i + ka];
      const float wa = th.dw[4 * i + ka];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const int ub = tw.di[4 * j + kb];
        const float wab = wa * tw.dw[4 * j + kb];
        const f32x4 u = aa_up_value(X, th, tw, ua, ub, w, lg_nc4, c4);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(wab, u[k] > 0.f ? u[k] : a.slope * u[k], acc[k]);
      }
    }
    acc += aa_bias4(a.bias, c, C, a.Cb);
    aa_st4<VEC>(out + (size_t)pix * C + c, acc, C - c);
  }
}

template <bool VEC>
__global__ __launch_bounds__(AA_THREADS) void aa_core_bwd_kernel(const AaCoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) int aa_lds[];
  const int h = a.h, w = a.w, C = a.C, ntab = 32 * (h + w), npix = h * w;
  const int lg_nc4 = a.lg_chw - 2, nc4 = 1 << lg_nc4, chw = 1 << a.lg_chw;
  const int n = blockIdx.x / a.nchunk, c0 = (blockIdx.x % a.nchunk) << a.lg_chw;
  for (int i = threadIdx.x; i < ntab; i += AA_THREADS) aa_lds[i] = a.tab[i];
  f32x4* X = reinterpret_cast<f32x4*>(aa_lds + ntab);
  f32x4* G = X + (size_t)npix * nc4;
  float* red = reinterpret_cast<float*>(G + (size_t)npix * nc4);      // [AA_THREADS]
  aa_load_plane<VEC>(X, a.x + (size_t)n * npix * C, npix, C, c0, lg_nc4);
  aa_load_plane<VEC>(G, a.g + (size_t)n * npix * C, npix, C, c0, lg_nc4);
  __syncthreads();
  const AaAxis th = aa_axis(aa_lds, h), tw = aa_axis(aa_lds + 32 * h, w);
  float* __restrict__ dx = a.out + (size_t)n * npix * C;
  for (int idx = threadIdx.x; idx < npix * nc4; idx += AA_THREADS) {
    const int c4 = idx & (nc4 - 1), pix = idx >> lg_nc4, c = c0 + 4 * c4;
    if (c >= C) continue;
    const int p = pix / w, q = pix - p * w;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int ka = 0; ka < 4; ++ka) {
      const int ua = th.uti[4 * p + ka];
      const float wa = th.utw[4 * p + ka];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const int ub = tw.uti[4 * q + kb];
        const float wab = wa * tw.utw[4 * q + kb];
        const f32x4 u = aa_up_value(X, th, tw, ua, ub, w, lg_nc4, c4);
        f32x4 gg = {0.f, 0.f, 0.f, 0.f};                               // (D^T g D)(ua, ub)
#pragma unroll
        for (int ki = 0; ki < 2; ++ki) {
          const int i = th.dti[2 * ua + ki];
          const float wi = th.dtw[2 * ua + ki];
#pragma unroll
          for (int kj = 0; kj < 2; ++kj) {
            const int j = tw.dti[2 * ub + kj];
            gg += (wi * tw.dtw[2 * ub + kj]) * G[((i * w + j) << lg_nc4) + c4];
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(wab * (u[k] > 0.f ? 1.0f : a.slope), gg[k], acc[k]);
      }
    }
    aa_st4<VEC>(dx + (size_t)pix * C + c, acc, C - c);
  }
  // bias partials: thread t sums channel t % CHW over the pixels t / CHW, t / CHW + 256 / CHW, ...; then CHW threads add the
  // 256 / CHW sub-sums in order
  const float* Gs = reinterpret_cast<const float*>(G);
  const int ch = threadIdx.x & (chw - 1), sub = threadIdx.x >> a.lg_chw, nsub = AA_THREADS >> a.lg_chw;
  float s = 0.f;
  for (int pix = sub; pix < npix; pix += nsub) s += Gs[(pix << a.lg_chw) + ch];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < chw && c0 + threadIdx.x < C) {
    float t = 0.f;
    for (int k = 0; k < nsub; ++k) t += red[(k << a.lg_chw) + threadIdx.x];
    a.part[(size_t)n * C + c0 + threadIdx.x] = t;
  }
}

// ---- V: bilinear h x w -> H x W and its adjoint ---------------------------------------------------------------------------
// table block: vh_i [2H] vh_w [2H] vw_i [2W] vw_w [2W] | th_ptr [h+1] th_i [2H] th_w [2H] | tw_ptr [w+1] tw_i [2W] tw_w [2W]
struct AaUpArgs {
  const float* in;     // forward: z [N,h,w,C]; adjoint: dy [N,H,W,C]
  const float* bias;
  float* out;
  const int* vtab;
  int N, h, w, H, W, C, Cb, lg_chw, nchunk;
};

template <bool VEC>
__global__ __launch_bounds__(AA_THREADS) void aa_up_fwd_kernel(const AaUpArgs a) {
  const int C4 = (a.C + 3) >> 2;
  const int64_t total = (int64_t)a.N * a.H * a.W * C4;
  const int64_t idx = (int64_t)blockIdx.x * AA_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int c = 4 * (int)(idx % C4);
  const int64_t pix = idx / C4;
  const int J = (int)(pix % a.W), I = (int)((pix / a.W) % a.H), n = (int)(pix / ((int64_t)a.W * a.H));
  const int* vhi = a.vtab;
  const float* vhw = reinterpret_cast<const float*>(a.vtab + 2 * a.H);
  const int* vwi = a.vtab + 4 * a.H;
  const float* vww = reinterpret_cast<const float*>(a.vtab + 4 * a.H + 2 * a.W);
  const float* __restrict__ z = a.in + (size_t)n * a.h * a.w * a.C;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ki = 0; ki < 2; ++ki) {
    const int i = vhi[2 * I + ki];
    const float wi = vhw[2 * I + ki];
#pragma unroll
    for (int kj = 0; kj < 2; ++kj) {
      const int j = vwi[2 * J + kj];
      acc += (wi * vww[2 * J + kj]) * aa_ld4<VEC>(z + ((size_t)i * a.w + j) * a.C + c, a.C - c);
    }
  }
  acc += aa_bias4(a.bias, c, a.C, a.Cb);
  aa_st4<VEC>(a.out + (size_t)pix * a.C + c, acc, a.C - c);
}

template <bool VEC>
__global__ __launch_bounds__(AA_THREADS) void aa_up_adj_kernel(const AaUpArgs a) {
  extern __shared__ __attribute__((aligned(16))) int aa_lds[];
  f32x4* R = reinterpret_cast<f32x4*>(aa_lds);                        // [W][CHW]
  const int H = a.H, W = a.W, C = a.C;
  const int lg_nc4 = a.lg_chw - 2, nc4 = 1 << lg_nc4;
  const int row = blockIdx.x / a.nchunk, c0 = (blockIdx.x % a.nchunk) << a.lg_chw;
  const int n = row / a.h, i = row - n * a.h;
  const int* thp = a.vtab + 4 * H + 4 * W;
  const int* thi = thp + a.h + 1;
  const float* thw = reinterpret_cast<const float*>(thi + 2 * H);
  const int* twp = thi + 4 * H;
  const int* twi = twp + a.w + 1;
  const float* tww = reinterpret_cast<const float*>(twi + 2 * W);
  const float* __restrict__ dy = a.in + (size_t)n * H * W * C;
  const int r0 = thp[i], r1 = thp[i + 1];
  for (int idx = threadIdx.x; idx < W * nc4; idx += AA_THREADS) {
    const int c = c0 + 4 * (idx & (nc4 - 1)), J = idx >> lg_nc4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (c < C)
      for (int r = r0; r < r1; ++r) acc += thw[r] * aa_ld4<VEC>(dy + ((size_t)thi[r] * W + J) * C + c, C - c);
    R[idx] = acc;
  }
  __syncthreads();
  float* __restrict__ g = a.out + (size_t)row * a.w * C;
  for (int idx = threadIdx.x; idx < a.w * nc4; idx += AA_THREADS) {
    const int c4 = idx & (nc4 - 1), j = idx >> lg_nc4, c = c0 + 4 * c4;
    if (c >= C) continue;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int r = twp[j]; r < twp[j + 1]; ++r) acc += tww[r] * R[(twi[r] << lg_nc4) + c4];
    aa_st4<VEC>(g + (size_t)j * C + c, acc, C - c);
  }
}

// the widest channel chunk (a power of two, 4 .. 32) whose `planes` LDS planes of `npix` pixels meet the budget, narrowed while
// the launch has fewer than 1024 workgroups or the chunk is wider than the channels need
static int aa_lg_chunk(int planes, int npix, int C, int64_t rows) {
  int lg = 5;
  while (lg > 2 && (int64_t)planes * npix * (4 << lg) > AA_LDS_BUDGET) --lg;
  while (lg > 2 && (1 << (lg - 1)) >= C) --lg;
  while (lg > 2 && rows * cdiv(C, 1 << lg) < 1024) --lg;
  return lg;
}

static int aa_check_core(const char* what, int N, int h, int w, int C) {
  DPOT_REQUIRE(N > 0 && C > 0 && h > 0 && w > 0, "%s: bad sizes N=%d field=%dx%d C=%d", what, N, h, w, C);
  if (h > AA_MAX || w > AA_MAX) {
    set_error("%s: latent size %dx%d is beyond the supported size (1 <= h, w <= %d: the plane of a workgroup lives in LDS)", what,
              h, w, AA_MAX);
    return DPOT_EUNSUP;
  }
  return DPOT_OK;
}

}  // namespace dpot

using namespace dpot;

extern "C" int dpot_aa_max_size(int output) { return output ? AA_OUT_MAX : AA_MAX; }
extern "C" int64_t dpot_aa_tab_words(int h, int w) { return 32 * ((int64_t)h + w); }
extern "C" int64_t dpot_aa_vtab_words(int h, int w, int H, int W) { return 8 * ((int64_t)H + W) + h + w + 2; }

extern "C" int dpot_aa_lrelu_fwd(const float* x, const float* bias, float* out, const int32_t* tab, int N, int h, int w, int C, int Cb,
                                 float slope, dpot_stream_t stream) {
  DPOT_REQUIRE(x && out && tab && x != out, "aa_lrelu_fwd: null or aliased pointer");
  if (int rc = aa_check_core("aa_lrelu_fwd", N, h, w, C)) return rc;
  DPOT_REQUIRE(!bias || (Cb > 0 && C % Cb == 0), "aa_lrelu_fwd: the bias length %d does not divide C = %d", Cb, C);
  AaCoreArgs a{};
  a.x = x, a.bias = bias, a.out = out, a.tab = tab;
  a.N = N, a.h = h, a.w = w, a.C = C, a.Cb = Cb > 0 ? Cb : 1, a.slope = slope;
  a.lg_chw = aa_lg_chunk(1, h * w, C, N);
  a.nchunk = cdiv(C, 1 << a.lg_chw);
  DPOT_REQUIRE((int64_t)N * a.nchunk < (1ll << 31), "aa_lrelu_fwd: too many workgroups (N=%d C=%d)", N, C);
  const size_t lds = sizeof(float) * ((size_t)32 * (h + w) + ((size_t)h * w << a.lg_chw));
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(out);
  const dim3 grid((unsigned)(N * a.nchunk)), block(AA_THREADS);
  if (vec) {
    if (int rc = raise_dynamic_lds<aa_core_fwd_kernel<true>>("aa_lrelu_fwd")) return rc;
    hipLaunchKernelGGL(aa_core_fwd_kernel<true>, grid, block, lds, as_stream(stream), a);
  } else {
    if (int rc = raise_dynamic_lds<aa_core_fwd_kernel<false>>("aa_lrelu_fwd")) return rc;
    hipLaunchKernelGGL(aa_core_fwd_kernel<false>, grid, block, lds, as_stream(stream), a);
  }
  return check_launch("aa_core_fwd_kernel");
}

extern "C" int dpot_aa_lrelu_bwd(const float* x, const float* g, float* dx, float* part, const int* tab, int N, int h, int w,
                                 int C, float slope, dpot_stream_t stream) {
  DPOT_REQUIRE(x && g && dx && part && tab && dx != x && dx != g, "aa_lrelu_bwd: null or aliased pointer");
  if (int rc = aa_check_core("aa_lrelu_bwd", N, h, w, C)) return rc;
  AaCoreArgs a{};
  a.x = x, a.g = g, a.out = dx, a.part = part, a.tab = tab;
  a.N = N, a.h = h, a.w = w, a.C = C, a.Cb = 1, a.slope = slope;
  a.lg_chw = aa_lg_chunk(2, h * w, C, N);
  a.nchunk = cdiv(C, 1 << a.lg_chw);
  DPOT_REQUIRE((int64_t)N * a.nchunk < (1ll << 31), "aa_lrelu_bwd: too many workgroups (N=%d C=%d)", N, C);
  const size_t lds = sizeof(float) * ((size_t)32 * (h + w) + 2 * ((size_t)h * w << a.lg_chw) + AA_THREADS);
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(g) && aligned16(dx);
  const dim3 grid((unsigned)(N * a.nchunk)), block(AA_THREADS);
  if (vec) {
    if (int rc = raise_dynamic_lds<aa_core_bwd_kernel<true>>("aa_lrelu_bwd")) return rc;
    hipLaunchKernelGGL(aa_core_bwd_kernel<true>, grid, block, lds, as_stream(stream), a);
  } else {
    if (int rc = raise_dynamic_lds<aa_core_bwd_kernel<false>>("aa_lrelu_bwd")) return rc;
    hipLaunchKernelGGL(aa_core_bwd_kernel<false>, grid, block, lds, as_stream(stream), a);
  }
  return check_launch("aa_core_bwd_kernel");
}

static int aa_check_up(const char* what, int N, int h, int w, int H, int W, int C) {
  int rc = aa_check_core(what, N, h, w, C);
  if (rc) return rc;
  if (H < h || W < w || H > AA_OUT_MAX || W > AA_OUT_MAX) {
    set_error("%s: output size %dx%d is not supported for a %dx%d field (per axis: input size <= output size <= %d)", what, H, W,
              h, w, AA_OUT_MAX);
    return DPOT_EUNSUP;
  }
  return DPOT_OK;
}

extern "C" int dpot_aa_up_fwd(const float* z, const float* bias, float* y, const int* vtab, int N, int h, int w, int H, int W,
                              int C, int Cb, dpot_stream_t stream) {
  DPOT_REQUIRE(z && y && vtab && z != y, "aa_up_fwd: null or aliased pointer");
  const int rc = aa_check_up("aa_up_fwd", N, h, w, H, W, C);
  if (rc) return rc;
  DPOT_REQUIRE(!bias || (Cb > 0 && C % Cb == 0), "aa_up_fwd: the bias length %d does not divide C = %d", Cb, C);
  AaUpArgs a{};
  a.in = z, a.bias = bias, a.out = y, a.vtab = vtab;
  a.N = N, a.h = h, a.w = w, a.H = H, a.W = W, a.C = C, a.Cb = Cb > 0 ? Cb : 1;
  const int64_t blocks = cdiv64((int64_t)N * H * W * cdiv(C, 4), AA_THREADS);
  DPOT_REQUIRE(blocks < (1ll << 31), "aa_up_fwd: too many workgroups (N=%d out=%dx%d C=%d)", N, H, W, C);
  const bool vec = C % 4 == 0 && aligned16(z) && aligned16(y);
  if (vec)
    hipLaunchKernelGGL(aa_up_fwd_kernel<true>, dim3((unsigned)blocks), dim3(AA_THREADS), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(aa_up_fwd_kernel<false>, dim3((unsigned)blocks), dim3(AA_THREADS), 0, as_stream(stream), a);
  return check_launch("aa_up_fwd_kernel");
}

extern "C" int dpot_aa_up_adj(const float* dy, float* g, const int* vtab, int N, int h, int w, int H, int W, int C,
                              dpot_stream_t stream) {
  DPOT_REQUIRE(dy && g && vtab && dy != g, "aa_up_adj: null or aliased pointer");
  const int rc = aa_check_up("aa_up_adj", N, h, w, H, W, C);
  if (rc) return rc;
  AaUpArgs a{};
  a.in = dy, a.out = g, a.vtab = vtab;
  a.N = N, a.h = h, a.w = w, a.H = H, a.W = W, a.C = C, a.Cb = 1;
  a.lg_chw = aa_lg_chunk(2, W, C, (int64_t)N * h);       // 2: half the budget, so several workgroups share a CU
  a.nchunk = cdiv(C, 1 << a.lg_chw);
  DPOT_REQUIRE((int64_t)N * h * a.nchunk < (1ll << 31), "aa_up_adj: too many workgroups (N=%d h=%d C=%d)", N, h, C);
  const size_t lds = sizeof(float) * ((size_t)W << a.lg_chw);
  const bool vec = C % 4 == 0 && aligned16(dy) && aligned16(g);
  const dim3 grid((unsigned)(N * h * a.nchunk)), block(AA_THREADS);
  if (vec)
    hipLaunchKernelGGL(aa_up_adj_kernel<true>, grid, block, lds, as_stream(stream), a);
  else
    hipLaunchKernelGGL(aa_up_adj_kernel<false>, grid, block, lds, as_stream(stream), a);
  return check_launch("aa_up_adj_kernel");
}
