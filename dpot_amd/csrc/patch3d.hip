// patch3d.hip - the index rearrangements at the two ends of DPOTNet3D (all fp32, pure data movement, HBM-bound):
//   dpot_patchify3    x[B,S,S,S,T,C] -> patch matrix A[(b,t,hx,hy,hz), (c,i,j,k)] with the four coordinate channels
//   dpot_unpatchify3  its adjoint for the data channels
//   dpot_fold3        [B*h^3, old*P^3] (columns (o,i,j,k)) <-> [B*(hP)^3, old] (rows (b,x,y,z)): the scatter of a k = s = P
//                     transposed convolution and its inverse
// All three are ONE map between a channels-last FIELD f[b, x, y, z, (t, c)] and a matrix of patch ROWS
// m[(b, t, hx, hy, hz), (c, i, j, k)], x = hx P + i, y = hy P + j, z = hz P + k (fold3: T = 1, c = o, no coordinate columns).
#include "common.h"

namespace dpot {

// One workgroup moves one (patch, i)-slab: the P field runs j = 0..P-1 at x = hx P + i, each P*T*C contiguous floats (the z
// extent of the patch with its channels-last tail).  On the rows side the same slab is T * channels runs of P^2 contiguous
// floats (columns (j, k) of one (c, i)).  The slab is staged through LDS (P * (P T C + 1) floats: 10 KB at P = 8, T C = 40),
// so both global sides are coalesced and every element is read once and written once.  Field side: one wave per run;
// rows side: consecutive lanes on consecutive columns.  LDS row stride P T C + 1: the rows-side accesses (stride T C over k,
// + 1 over j) fall on 64 distinct banks at P = 8, T C = 40.
// GATHER: field -> rows (patchify3, fold3 inverse), else rows -> field.  ncoord = 4: the rows carry the coordinate channels
// C..C+3 = gs[x], gs[y], gs[z], gt[t] - written from the tables by GATHER, skipped by the scatter.
// VEC: 16-byte global accesses; the host proves P % 4 == 0 (so every run starts on a 4-float boundary) and 16-byte bases.
template <bool GATHER, bool VEC>
__global__ __launch_bounds__(256) void patch3_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                     const float* __restrict__ gs, const float* __restrict__ gt, int h,
                                                     int P, int T, int C, int ncoord) {
  extern __shared__ float sm[];
  const int S = h * P, TC = T * C, run = P * TC, rp = run + 1, PP = P * P;
  const long long K = (long long)(C + ncoord) * PP * P, tok = (long long)h * h * h;
  unsigned site = blockIdx.x;
  const int i = site % P;
  site /= P;
  const int hz = site % h;
  site /= h;
  const int hy = site % h;
  site /= h;
  const int hx = site % h, b = site / h;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* fsrc = src;
  float* fdst = dst;
  const long long f0 = ((((long long)b * S + hx * P + i) * S + hy * P) * S + hz * P) * TC;   // run j starts at f0 + j S TC
  const long long m0 = ((long long)b * T * tok + ((long long)hx * h + hy) * h + hz) * K + (long long)i * PP;  // t = 0, c = 0

  auto field_side = [&]() {
    for (int j = wave; j < P; j += 4) {
      const long long f = f0 + (long long)j * S * TC;
      float* s = sm + j * rp;
      if (VEC) {
        for (int r = lane; r < run / 4; r += 64) {
          if (GATHER) {
            const float4 v = reinterpret_cast<const float4*>(fsrc + f)[r];
            s[4 * r] = v.x, s[4 * r + 1] = v.y, s[4 * r + 2] = v.z, s[4 * r + 3] = v.w;
          } else {
            reinterpret_cast<float4*>(fdst + f)[r] = make_float4(s[4 * r], s[4 * r + 1], s[4 * r + 2], s[4 * r + 3]);
          }
        }
      } else {
        for (int r = lane; r < run; r += 64) {
          if (GATHER) s[r] = fsrc[f + r];
          else fdst[f + r] = s[r];
        }
      }
    }
  };

  if (GATHER) {
    field_side();
    __syncthreads();
  }
  // rows side: element (t, c, j, k) of the slab is m[m0 + t tok K + c P^3 + j P + k] and sm[j rp + k TC + t C + c]
  const int nch = GATHER ? C + ncoord : C, W = VEC ? 4 : 1, per = PP / W, n = T * nch * per;
  for (int o = threadIdx.x; o < n; o += 256) {
    const int rc = o / per, e = (o - rc * per) * W;
    const int t = rc / nch, c = rc - t * nch;
    const int j = e / P, k = e - j * P;
    const long long m = m0 + (long long)t * tok * K + (long long)c * PP * P + e;
    float* s = sm + j * rp + k * TC + t * C + c;
    float v[4];
    if (GATHER) {
      if (c < C) {
#pragma unroll
        for (int q = 0; q < W; ++q) v[q] = s[q * TC];
      } else {
        const int cc = c - C;
#pragma unroll
        for (int q = 0; q < W; ++q)
          v[q] = cc == 0 ? gs[hx * P + i] : cc == 1 ? gs[hy * P + j] : cc == 2 ? gs[hz * P + k + q] : gt[t];
      }
      if (VEC) *reinterpret_cast<float4*>(dst + m) = make_float4(v[0], v[1], v[2], v[3]);
      else dst[m] = v[0];
    } else {
      if (VEC) {
        const float4 u = *reinterpret_cast<const float4*>(src + m);
        v[0] = u.x, v[1] = u.y, v[2] = u.z, v[3] = u.w;
      } else {
        v[0] = src[m];
      }
#pragma unroll
      for (int q = 0; q < W; ++q) s[q * TC] = v[q];
    }
  }
  if (!GATHER) {
    __syncthreads();
    field_side();
  }
}

static int launch_patch3(const char* what, bool gather, const float* src, float* dst, const float* gs, const float* gt,
                         int B, int h, int P, int T, int C, int ncoord, dpot_stream_t stream) {
  const size_t lds = sizeof(float) * (size_t)P * ((size_t)P * T * C + 1);
  DPOT_REQUIRE(lds <= 64 * 1024, "%s: a slab of P * (P*T*C + 1) floats = %zu bytes exceeds 64 KiB of LDS", what, lds);
  const long long blocks = (long long)B * h * h * h * P;
  DPOT_REQUIRE(blocks < (1ll << 31) && (long long)(C + ncoord) * P * P * P < (1ll << 31), "%s: too many slabs / columns", what);
  const bool vec = P % 4 == 0 && aligned16(src) && aligned16(dst);
  const dim3 grid((unsigned)blocks), block(256);
#define DPOT_PATCH3(G, V) \
  hipLaunchKernelGGL((patch3_kernel<G, V>), grid, block, lds, as_stream(stream), src, dst, gs, gt, h, P, T, C, ncoord)
  if (gather) {
    if (vec) DPOT_PATCH3(true, true);
    else DPOT_PATCH3(true, false);
  } else {
    if (vec) DPOT_PATCH3(false, true);
    else DPOT_PATCH3(false, false);
  }
#undef DPOT_PATCH3
  return check_launch(what);
}

}  // namespace dpot

using namespace dpot;

extern "C" int dpot_patchify3(const float* x, const float* gs, const float* gt, float* A, int B, int S, int T, int C, int P,
                              dpot_stream_t stream) {
  DPOT_REQUIRE(x && gs && gt && A, "patchify3: null pointer");
  DPOT_REQUIRE(B > 0 && P > 0 && S > 0 && S % P == 0 && T > 0 && C > 0, "patchify3: bad shape B=%d S=%d P=%d T=%d C=%d", B, S,
               P, T, C);
  return launch_patch3("patchify3", true, x, A, gs, gt, B, S / P, P, T, C, 4, stream);
}

extern "C" int dpot_unpatchify3(const float* dA, float* dx, int B, int S, int T, int C, int P, dpot_stream_t stream) {
  DPOT_REQUIRE(dA && dx, "unpatchify3: null pointer");
  DPOT_REQUIRE(B > 0 && P > 0 && S > 0 && S % P == 0 && T > 0 && C > 0, "unpatchify3: bad shape B=%d S=%d P=%d T=%d C=%d", B,
               S, P, T, C);
  return launch_patch3("unpatchify3", false, dA, dx, nullptr, nullptr, B, S / P, P, T, C, 4, stream);
}

extern "C" int dpot_fold3(const float* src, float* dst, int B, int h, int P, int old, int inverse, dpot_stream_t stream) {
  DPOT_REQUIRE(src && dst, "fold3: null pointer");
  DPOT_REQUIRE(B > 0 && h > 0 && P > 0 && old > 0, "fold3: bad shape B=%d h=%d P=%d old=%d", B, h, P, old);
  return launch_patch3("fold3", inverse != 0, src, dst, nullptr, nullptr, B, h, P, 1, old, 0, stream);
}
