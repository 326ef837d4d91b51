// resize3.hip - Fourier ("spectral") resize of channels-last 3-D fields [B, X, Y, Z, TC]: the three-axis form of the
// reference's utils/utilities.py:277-305 (rfftn over X, Y, Z -> the four low-frequency corner blocks of the two full-spectrum
// axes and the low half-spectrum columns of Z into a spectrum of the new size -> irfftn -> rescale), as dense products on the
// fp32 matrix cores.
//
// The operator is Re(Dx (x) Dy (x) Dz) / (nx ny nz) on a real field: the products with an even number of imaginary factors,
//   Rx Ry Rz - Rx Iy Iz - Ix Ry Iz - Ix Iy Rz                                       (R = Re D, I = Im D)
//   = Rx (x) P - Ix (x) Q,     P = Ry (x) Rz - Iy (x) Iz = Re(Dy (x) Dz),   Q = Ry (x) Iz + Iy (x) Rz = Im(Dy (x) Dz).
// Ix = ux vx^T and Iy = uy vy^T are rank one, or zero when min(n, m) is odd or n == m (ops.spectral_resize_im_factors); Iz is
// a general matrix.  So with ex = (Ix != 0), ey = (Iy != 0):
//   ex ey   surviving terms
//   0  0    Rx Ry Rz
//   0  1    Rx Ry Rz - Rx Iy Iz
//   1  0    Rx Ry Rz - Ix Ry Iz
//   1  1    all four
// P and Q both have the shape of the 2-D operator of resize_core.h - a product of two matrices plus, when ey, a rank-one factor
// times a second matrix product - so ONE kernel (spectral_resize_kernel, the plane launch) applies either to every plane:
//   P:  AxT = RyT, AyT = RzT s, ByT = IzT s, u = -uy, v = vy          s = 1 / (nx ny nz), folded into the Z matrices
//   Q:  AxT = RyT, AyT = IzT s, ByT = RzT s, u = +uy, v = vy
// and because Ix is rank one, Q is needed of ONE plane per sample only: Ix (x) Q in = ux (x) Q(sum_x vx[x] in[b, x]).
//
// Launches (ex adds the three marked *):
//   * reduce   s[b] = sum_x vx[x] in[b, x]                    VALU, one pass over the input, x-ordered fma chain
//   * plane Q  q[b] = Q s[b]                                  B planes
//     plane P  every (b, x) plane: contracts Y, then Z (intermediate in LDS, resize_core.h)
//     axis     contracts X: a dense product [mx x nx] x [nx x (rest)] over HBM, the field as the B operand straight from global
//              memory (16 bytes per lane = 4 column tiles, as pass 1 of the plane kernel), 32 output rows per workgroup
//   out = Rx (x) P in - ux (x) q: the launch that runs LAST adds (-ux[x']) q[b] in its epilogue.
// Pass order: the workspace between the plane and the axis launch is [B, nx, my, mz, TC] when the planes run first and
// [B, mx, ny, nz, TC] when the axis runs first; the smaller one is taken, so shrinking axes are contracted first and growing
// ones last.  Workspace = that field, then (ex) s [B, ny, nz, TC] and q [B, my, mz, TC]: dpot_spectral_resize3_ws_elems.
// Nothing outside the tensors and the workspace is touched: loads past an extent are predicated to 0.0f, stores are masked.
// Fixed reduction order (k-ordered chains), no atomics, no allocation, capture-legal.
#include <algorithm>

#include "resize_core.h"

namespace dpot {

// s[b, r] = sum_x v[x] in[b, x, r]; r < R (R4 = R / 4 vectors when VEC)
template <bool VEC>
__global__ __launch_bounds__(256) void resize3_reduce_kernel(const float* __restrict__ in, float* __restrict__ s,
                                                             const float* __restrict__ v, int nx, int64_t R) {
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  in += (size_t)b * nx * R;
  s += (size_t)b * R;
  if (VEC) {
    if (i >= R / 4) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int x = 0; x < nx; ++x) {
      const f32x4 f = *reinterpret_cast<const f32x4*>(in + (size_t)x * R + 4 * i);
      const float vx = v[x];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(vx, f[j], acc[j]);
    }
    *reinterpret_cast<f32x4*>(s + 4 * i) = acc;
  } else {
    if (i >= R) return;
    float acc = 0.f;
    for (int x = 0; x < nx; ++x) acc = fmaf(v[x], in[(size_t)x * R + i], acc);
    s[i] = acc;
  }
}

// out[b, x', r] = sum_x axT[x][x'] in[b, x, r]  (+ coef[x'] add[b, r]);  r < R.  Of ResizeArgs: in, out, axT, nx, mx, nxp, mxp,
// add, coef.  Workgroup = (stripe of RS_XS rows x', 64 RS_NW columns r), wave w the columns 64 w ..: lane (lr, lg) loads the 4
// floats r0 = 4 (16 (RS_NW blockIdx.y + w) + lr) .. of row x = k0 + 4 s + lg, each float its own 16-column MFMA tile.
template <bool VEC, bool ADD>
__global__ __launch_bounds__(64 * RS_NW) void resize3_axis_kernel(const ResizeArgs a, const int64_t R) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int x0 = blockIdx.x * RS_XS, b = blockIdx.z;
  const int64_t r0 = 4 * (((int64_t)blockIdx.y * RS_NW + wave) * 16 + lr);
  const bool ok = r0 < R;
  const int npc = !ok ? 0 : (R - r0 < RS_PC ? (int)(R - r0) : RS_PC);
  const float* __restrict__ col = a.in + (size_t)b * a.nx * R + r0;
  float* __restrict__ out = a.out + (size_t)b * a.mx * R + r0;
  const bool two = x0 + 16 < a.mx;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[2][RS_PC];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int pc = 0; pc < RS_PC; ++pc) acc[i][pc] = zero4;
  ResizeChunk cur, nxt;
  resize_load_chunk<false, VEC>(cur, a, col, (size_t)R, 0, ok, x0, npc, lr, lg, two);
  for (int k0 = 0; k0 < a.nxp; k0 += 16) {
    if (k0 + 16 < a.nxp) resize_load_chunk<false, VEC>(nxt, a, col, (size_t)R, k0 + 16, ok, x0, npc, lr, lg, two);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int pc = 0; pc < RS_PC; ++pc)
        acc[0][pc] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.am[0][s], cur.f[s][pc], acc[0][pc], 0, 0, 0);
      if (two) {
#pragma unroll
        for (int pc = 0; pc < RS_PC; ++pc)
          acc[1][pc] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.am[1][s], cur.f[s][pc], acc[1][pc], 0, 0, 0);
      }
    }
    cur = nxt;
  }
  if (!ok) return;
  // accumulator: column = lr (the lane's own 4 floats, one per pc), row = 4 lg + reg (x' inside the tile)
  f32x4 q = zero4;
  if (ADD) {
    const float* __restrict__ addp = a.add + (size_t)b * R + r0;
    if (VEC) {
      q = *reinterpret_cast<const f32x4*>(addp);
    } else {
#pragma unroll
      for (int pc = 0; pc < RS_PC; ++pc)
        if (pc < npc) q[pc] = addp[pc];
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int xo = x0 + 16 * i + 4 * lg + reg;
      if (xo < a.mx) {
        f32x4 r = {acc[i][0][reg], acc[i][1][reg], acc[i][2][reg], acc[i][3][reg]};
        if (ADD) {
          const float cf = a.coef[xo];
#pragma unroll
          for (int pc = 0; pc < RS_PC; ++pc) r[pc] = fmaf(cf, q[pc], r[pc]);
        }
        float* dst = out + (size_t)xo * R;
        if (VEC) {
          *reinterpret_cast<f32x4*>(dst) = r;
        } else {
#pragma unroll
          for (int pc = 0; pc < RS_PC; ++pc)
            if (pc < npc) dst[pc] = r[pc];
        }
      }
    }
}

static inline bool resize3_two_terms(int n, int m) { return n != m && (n < m ? n : m) % 2 == 0; }

struct Resize3Sizes {
  int B, nx, ny, nz, mx, my, mz, TC;
  bool ex, ey, plane_first;
  int64_t w_elems, s_elems, q_elems;   // the workspace's three parts (s, q: 0 without ex)
};

static int resize3_sizes(Resize3Sizes& z, int B, int nx, int ny, int nz, int mx, int my, int mz, int TC) {
  DPOT_REQUIRE(B > 0 && nx > 1 && ny > 1 && nz > 1 && mx > 1 && my > 1 && mz > 1 && TC > 0,
               "spectral_resize3: bad sizes B=%d in=%dx%dx%d out=%dx%dx%d TC=%d (every spatial size must be >= 2)", B, nx, ny, nz,
               mx, my, mz, TC);
  const int big = std::max(std::max(std::max(nx, ny), nz), std::max(std::max(mx, my), mz));
  if (big > RS_NY_MAX) {
    set_error("spectral_resize3: %dx%dx%d -> %dx%dx%d: the size %d is beyond the LDS intermediate of a workgroup (every size <= %d)",
              nx, ny, nz, mx, my, mz, big, RS_NY_MAX);
    return DPOT_EUNSUP;
  }
  z.B = B, z.nx = nx, z.ny = ny, z.nz = nz, z.mx = mx, z.my = my, z.mz = mz, z.TC = TC;
  z.ex = resize3_two_terms(nx, mx), z.ey = resize3_two_terms(ny, my);
  const int64_t pf = (int64_t)nx * my * mz, af = (int64_t)mx * ny * nz;
  z.plane_first = pf <= af;
  z.w_elems = (int64_t)B * (z.plane_first ? pf : af) * TC;
  z.s_elems = z.ex ? (int64_t)B * ny * nz * TC : 0;
  z.q_elems = z.ex ? (int64_t)B * my * mz * TC : 0;
  const int64_t R = (int64_t)(z.plane_first ? my * mz : ny * nz) * TC;      // the axis launch's columns
  DPOT_REQUIRE((int64_t)B * std::max(nx, mx) <= 65535 && cdiv(TC, RS_PC) <= 65535 && cdiv64(R, 64 * RS_NW) <= 65535,
               "spectral_resize3: B * X = %lld planes, TC = %d or %lld columns of the X pass exceed the launch grid (65535 planes, "
               "4 * 65535 planes of (t, c), 256 * 65535 columns)", (long long)B * std::max(nx, mx), TC, (long long)R);
  return DPOT_OK;
}

static int resize3_plane(const Resize3Sizes& z, const float* in, float* out, int planes, const float* ryT, const float* azT,
                         const float* bzT, const float* u, const float* vy, const float* add, const float* coef, int xper,
                         hipStream_t s) {
  ResizeArgs a;
  a.in = in, a.out = out, a.axT = ryT, a.ayT = azT, a.byT = bzT, a.u = u, a.v = vy;
  a.nx = z.ny, a.ny = z.nz, a.mx = z.my, a.my = z.mz, a.TC = z.TC;
  a.add = add, a.coef = coef, a.xper = xper;
  const bool vec = z.TC % 4 == 0 && aligned16(in) && aligned16(out) && (!add || aligned16(add));
  const char* what = "spectral_resize3 (plane launch)";
  if (add) {
    if (z.ey)
      return vec ? launch_spectral_resize<true, true, true>(what, a, planes, s)
                 : launch_spectral_resize<true, false, true>(what, a, planes, s);
    return vec ? launch_spectral_resize<false, true, true>(what, a, planes, s)
               : launch_spectral_resize<false, false, true>(what, a, planes, s);
  }
  // the 3-D instantiations without ADD are the 2-D launcher's own: one more copy of them here would only be a second symbol
  return dpot_spectral_resize(in, out, ryT, azT, z.ey ? bzT : nullptr, u, vy, planes, z.ny, z.nz, z.my, z.mz, z.TC,
                              reinterpret_cast<dpot_stream_t>(s));
}

static int resize3_axis(const Resize3Sizes& z, const float* in, float* out, const float* rxT, int64_t R, const float* add,
                        const float* coef, hipStream_t s) {
  ResizeArgs a = {};
  a.in = in, a.out = out, a.axT = rxT, a.nx = z.nx, a.mx = z.mx;
  a.nxp = resize_pad(z.nx, 0), a.mxp = resize_pad(z.mx, 1);
  a.add = add, a.coef = coef, a.xper = 1;
  const bool vec = R % 4 == 0 && aligned16(in) && aligned16(out) && (!add || aligned16(add));
  const dim3 grid(a.mxp / RS_XS, (unsigned)cdiv64(R, 64 * RS_NW), z.B), block(64 * RS_NW);
  if (add) {
    if (vec) hipLaunchKernelGGL((resize3_axis_kernel<true, true>), grid, block, 0, s, a, R);
    else hipLaunchKernelGGL((resize3_axis_kernel<false, true>), grid, block, 0, s, a, R);
  } else {
    if (vec) hipLaunchKernelGGL((resize3_axis_kernel<true, false>), grid, block, 0, s, a, R);
    else hipLaunchKernelGGL((resize3_axis_kernel<false, false>), grid, block, 0, s, a, R);
  }
  return check_launch("resize3_axis_kernel");
}

}  // namespace dpot

using namespace dpot;

extern "C" int dpot_spectral_resize3_pad(int n, int output_rows) { return resize_pad(n, output_rows); }

extern "C" int dpot_spectral_resize3_max_size(void) { return RS_NY_MAX; }

extern "C" int64_t dpot_spectral_resize3_ws_elems(int B, int nx, int ny, int nz, int mx, int my, int mz, int TC) {
  Resize3Sizes z;
  if (resize3_sizes(z, B, nx, ny, nz, mx, my, mz, TC) != DPOT_OK) return 0;
  return z.w_elems + z.s_elems + z.q_elems;
}

extern "C" int dpot_spectral_resize3(const float* in, float* out, float* ws, const float* rxT, const float* ryT, const float* rzT,
                                     const float* izT, const float* nux, const float* vx, const float* uy2, const float* vy,
                                     int B, int nx, int ny, int nz, int mx, int my, int mz, int TC, dpot_stream_t stream) {
  DPOT_REQUIRE(in && out && ws && in != out && rxT && ryT && rzT, "spectral_resize3: null or aliased field / matrix pointer");
  Resize3Sizes z;
  if (int rc = resize3_sizes(z, B, nx, ny, nz, mx, my, mz, TC)) return rc;
  DPOT_REQUIRE(!z.ex || (izT && nux && vx), "spectral_resize3: %d -> %d along X has an imaginary term: izT, nux and vx are needed",
               nx, mx);
  DPOT_REQUIRE(!z.ey || (izT && uy2 && vy), "spectral_resize3: %d -> %d along Y has an imaginary term: izT, uy2 and vy are needed",
               ny, my);
  hipStream_t s = as_stream(stream);
  float* W = ws;
  float* S = ws + z.w_elems;
  float* Q = S + z.s_elems;
  const float* uy = uy2;                                          // +uy: the Q operator
  const float* nuy = uy2 ? uy2 + resize_pad(my, 1) : nullptr;     // -uy: the P operator
  const int64_t Rin = (int64_t)ny * nz * TC, Rout = (int64_t)my * mz * TC;
  if (z.ex) {
    const bool vec = TC % 4 == 0 && aligned16(in) && aligned16(S);
    const int64_t n = vec ? Rin / 4 : Rin;
    const dim3 grid((unsigned)cdiv64(n, 256), B);
    if (vec) hipLaunchKernelGGL((resize3_reduce_kernel<true>), grid, dim3(256), 0, s, in, S, vx, nx, Rin);
    else hipLaunchKernelGGL((resize3_reduce_kernel<false>), grid, dim3(256), 0, s, in, S, vx, nx, Rin);
    if (int rc = check_launch("resize3_reduce_kernel")) return rc;
    if (int rc = resize3_plane(z, S, Q, B, ryT, izT, rzT, uy, vy, nullptr, nullptr, 1, s)) return rc;
  }
  const float* q = z.ex ? Q : nullptr;
  if (z.plane_first) {
    if (int rc = resize3_plane(z, in, W, B * nx, ryT, rzT, izT, nuy, vy, nullptr, nullptr, 1, s)) return rc;
    return resize3_axis(z, W, out, rxT, Rout, q, nux, s);
  }
  if (int rc = resize3_axis(z, in, W, rxT, Rin, nullptr, nullptr, s)) return rc;
  return resize3_plane(z, W, out, B * mx, ryT, rzT, izT, nuy, vy, q, nux, mx, s);
}
