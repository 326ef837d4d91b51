// resize_core.h - the one copy of the two-pass Fourier-resize kernel: csrc/resize.hip launches it on the planes of a 2-D field,
// csrc/resize3.hip on the (b, x) planes of a 3-D one (its Y / Z contractions) and borrows the operand loader for its X pass.
//
//   out[b, x', y', p] = sum_y AyT[y, y'] * ( sum_x AxT[x, x'] * in[b, x, y, p] )                      p = (t, c) plane
//                     + u[x'] * sum_y ByT[y, y'] * ( sum_x v[x] * in[b, x, y, p] )                    EVEN only
//                     + coef[b % xper] * add[b / xper, x', y', p]                                     ADD only (resize3.hip)
//
// One launch, one workgroup per (b, stripe of RS_XS output rows x', chunk of RS_PC planes), RS_NW waves:
//   pass 1 (X)  Tmp[(x', pc), y] = sum_x Ax[x', x] in[x, y, pc]     A = AxT fragments (global, L1/L2 resident),
//               B = the field straight from global memory (one 16-byte load per lane = the 4 planes of one (x, y), each plane
//               its own column tile), wave w owns the y tiles w, w + RS_NW, ...; result to LDS, row (x', pc), y contiguous.
//               Even pairs: w[pc, y] = sum_x v[x] in[x, y, pc] rides on the VALU beside the MFMAs (one fma per loaded value,
//               the 4 k-groups summed in a fixed shuffle order) and becomes 4 more LDS rows.
//   pass 2 (Y)  out[(x', pc), y'] = sum_y Tmp[(x', pc), y] AyT[y, y']   A = Tmp from LDS (ds_read_b128 along y), B = AyT
//               fragments, wave w owns the y' tiles w, w + RS_NW, ... with all 8 row tiles in accumulators.  The accumulator
//               layout puts the 4 planes of one (x', y') into the 4 registers of a lane: one 16-byte store per lane, 16 lanes
//               cover 16 consecutive y'.  Even pairs: one more row tile z = w ByT, then out += u[x'] z (an fma per element).
// The X pass runs first and the workgroup is cut over x' because the second pass contracts the axis the first leaves free:
// only a cut along the FINAL pass's free axis keeps both passes free of recomputation.  The field is re-read once per stripe
// (mx / 32 times) - neighbouring blockIdx.x, so from L2 - and every output element is written once.
// Nothing outside the tensors is read: field loads past nx, ny or TC are predicated to 0.0f (never garbage x 0), stores are
// masked.  Fixed reduction order (k-ordered fma chains of v_mfma_f32_16x16x4_f32), no atomics, no allocation.
#pragma once
#include "common.h"

namespace dpot {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RS_XS = 32;                 // output rows x' per workgroup (two 16-row MFMA tiles)
constexpr int RS_PC = 4;                  // planes per workgroup
constexpr int RS_ROWS = RS_XS * RS_PC;    // rows (x', pc) of the LDS intermediate
constexpr int RS_NW = 4;                  // waves
// one limit for both forms (the two-term form's 16 extra rows decide it): a size pair's parity must not change what fits
constexpr int RS_LD_MAX = LDS_BYTES / 4 / (RS_ROWS + 16);
constexpr int RS_NY_MAX = (RS_LD_MAX - 4) / 16 * 16;   // the largest second-axis input size (272)

static inline int resize_pad(int n, int output_rows) {
  const int q = output_rows ? RS_XS : 16;
  return n <= 0 ? 0 : (n + q - 1) / q * q;
}

struct ResizeArgs {
  const float* in;
  float* out;
  const float* axT;   // [nxp][mxp]
  const float* ayT;   // [nyp][myp]
  const float* byT;   // [nyp][myp]   even pairs
  const float* u;     // [mxp]        even pairs
  const float* v;     // [nxp]        even pairs
  int nx, ny, mx, my, TC, nxp, nyp, mxp, myp;
  const float* add;   // [planes / xper][mx][my][TC]   ADD only
  const float* coef;  // [xper]                        ADD only
  int xper;
};

struct ResizeChunk {   // the operands of 16 k (= x) values of pass 1, per lane
  f32x4 f[4];
  float am[2][4];
  float vv[4];
};

// `col` points at the lane's 4 values of row x = 0 (valid when ok), rows are `xstride` floats apart
template <bool EVEN, bool VEC>
__device__ __forceinline__ void resize_load_chunk(ResizeChunk& c, const ResizeArgs& a, const float* __restrict__ col,
                                                  size_t xstride, int k0, bool ok, int x0, int npc, int lr, int lg, bool two) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int x = k0 + 4 * s + lg;
    f32x4 f = {0.f, 0.f, 0.f, 0.f};
    if (ok && x < a.nx) {
      const float* src = col + (size_t)x * xstride;
      if (VEC) {
        f = *reinterpret_cast<const f32x4*>(src);
      } else {
#pragma unroll
        for (int pc = 0; pc < RS_PC; ++pc)
          if (pc < npc) f[pc] = src[pc];
      }
    }
    c.f[s] = f;
    const float* arow = a.axT + (size_t)x * a.mxp + x0 + lr;     // x < nxp: inside the padded matrix
    c.am[0][s] = arow[0];
    c.am[1][s] = two ? arow[16] : 0.f;
    if (EVEN) c.vv[s] = a.v[x];
  }
}

template <bool EVEN, bool VEC, bool ADD>
__global__ __launch_bounds__(64 * RS_NW) void spectral_resize_kernel(const ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int x0 = blockIdx.x * RS_XS, p0 = blockIdx.y * RS_PC, b = blockIdx.z;
  const int LD = a.nyp + 4;                                        // + 4: rows 16 bytes apart from a bank-aligned stride
  const float* __restrict__ in = a.in + (size_t)b * a.nx * a.ny * a.TC;
  float* __restrict__ out = a.out + (size_t)b * a.mx * a.my * a.TC;
  const int npc = a.TC - p0 < RS_PC ? a.TC - p0 : RS_PC;
  const bool two = x0 + 16 < a.mx;                                 // does the second 16-row tile hold any real x'?
  const size_t xstride = (size_t)a.ny * a.TC;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // ---- pass 1: contract x --------------------------------------------------------------------------------------------
  for (int yt = wave; yt < a.nyp / 16; yt += RS_NW) {
    const int y = yt * 16 + lr;
    const bool yok = y < a.ny;
    const float* __restrict__ col = in + (size_t)y * a.TC + p0;
    f32x4 acc[2][RS_PC];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int pc = 0; pc < RS_PC; ++pc) acc[i][pc] = zero4;
    float w[RS_PC] = {0.f, 0.f, 0.f, 0.f};
    ResizeChunk cur, nxt;
    resize_load_chunk<EVEN, VEC>(cur, a, col, xstride, 0, yok, x0, npc, lr, lg, two);
    for (int k0 = 0; k0 < a.nxp; k0 += 16) {
      if (k0 + 16 < a.nxp) resize_load_chunk<EVEN, VEC>(nxt, a, col, xstride, k0 + 16, yok, x0, npc, lr, lg, two);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int pc = 0; pc < RS_PC; ++pc) {
          acc[0][pc] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.am[0][s], cur.f[s][pc], acc[0][pc], 0, 0, 0);
          if (EVEN) w[pc] = fmaf(cur.vv[s], cur.f[s][pc], w[pc]);
        }
        if (two) {
#pragma unroll
          for (int pc = 0; pc < RS_PC; ++pc)
            acc[1][pc] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.am[1][s], cur.f[s][pc], acc[1][pc], 0, 0, 0);
        }
      }
      cur = nxt;
    }
    // accumulator: column = lr (y), row = 4 lg + reg (x' inside the tile)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int pc = 0; pc < RS_PC; ++pc)
#pragma unroll
        for (int r = 0; r < 4; ++r) rs_lds[((16 * i + 4 * lg + r) * RS_PC + pc) * LD + y] = acc[i][pc][r];
    if (EVEN) {
#pragma unroll
      for (int pc = 0; pc < RS_PC; ++pc) {
        float t = w[pc];
        t += __shfl_xor(t, 16, 64);
        t += __shfl_xor(t, 32, 64);
        rs_lds[(RS_ROWS + 4 * lg + pc) * LD + y] = lg == 0 ? t : 0.f;   // rows 4 .. 15 of the extra tile are zero
      }
    }
  }
  __syncthreads();

  // ---- pass 2: contract y --------------------------------------------------------------------------------------------
  for (int ct = wave; ct < a.myp / 16; ct += RS_NW) {
    const int yo = ct * 16 + lr;
    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = zero4;
    f32x4 accz = zero4;
    for (int k0 = 0; k0 < a.nyp; k0 += 16) {
      float bm[4], bz[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const size_t o = (size_t)(k0 + 4 * lg + s) * a.myp + yo;
        bm[s] = a.ayT[o];
        if (EVEN) bz[s] = a.byT[o];
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        if (t < 4 || two) {
          const f32x4 av = *reinterpret_cast<const f32x4*>(&rs_lds[(16 * t + lr) * LD + k0 + 4 * lg]);
#pragma unroll
          for (int s = 0; s < 4; ++s) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bm[s], acc[t], 0, 0, 0);
        }
      }
      if (EVEN) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(&rs_lds[(RS_ROWS + lr) * LD + k0 + 4 * lg]);
#pragma unroll
        for (int s = 0; s < 4; ++s) accz = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bz[s], accz, 0, 0, 0);
      }
    }
    // accumulator: column = lr (y'), row = 4 lg + reg = (x' = 4 t + lg, pc = reg); z sits in the lanes with lg == 0
    f32x4 z = zero4;
    if (EVEN) {
#pragma unroll
      for (int pc = 0; pc < RS_PC; ++pc) z[pc] = __shfl(accz[pc], lr, 64);
    }
    const float cf = ADD ? a.coef[b % a.xper] : 0.f;
    const float* __restrict__ addp = ADD ? a.add + (size_t)(b / a.xper) * a.mx * a.my * a.TC : nullptr;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int xo = x0 + 4 * t + lg;
      if (xo < a.mx && yo < a.my) {
        f32x4 r = acc[t];
        if (EVEN) {
          const float uu = a.u[xo];
#pragma unroll
          for (int pc = 0; pc < RS_PC; ++pc) r[pc] = fmaf(uu, z[pc], r[pc]);
        }
        const size_t o = ((size_t)xo * a.my + yo) * a.TC + p0;
        float* dst = out + o;
        if (VEC) {
          if (ADD) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(addp + o);
#pragma unroll
            for (int pc = 0; pc < RS_PC; ++pc) r[pc] = fmaf(cf, q[pc], r[pc]);
          }
          *reinterpret_cast<f32x4*>(dst) = r;
        } else {
#pragma unroll
          for (int pc = 0; pc < RS_PC; ++pc)
            if (pc < npc) dst[pc] = ADD ? fmaf(cf, addp[o + pc], r[pc]) : r[pc];
        }
      }
    }
  }
}

// a.nxp .. a.myp are filled here; `planes` is the grid's z extent (the caller checks it against 65535)
template <bool EVEN, bool VEC, bool ADD>
static int launch_spectral_resize(const char* what, ResizeArgs a, int planes, hipStream_t s) {
  a.nxp = resize_pad(a.nx, 0), a.nyp = resize_pad(a.ny, 0), a.mxp = resize_pad(a.mx, 1), a.myp = resize_pad(a.my, 0);
  const size_t lds = sizeof(float) * (size_t)(RS_ROWS + (EVEN ? 16 : 0)) * (a.nyp + 4);
  DPOT_REQUIRE(a.nyp + 4 <= RS_LD_MAX, "%s: ny = %d is beyond the LDS intermediate of a workgroup (ny <= %d)", what, a.ny,
               RS_NY_MAX);
  if (int rc = raise_dynamic_lds<spectral_resize_kernel<EVEN, VEC, ADD>>(what)) return rc;
  hipLaunchKernelGGL((spectral_resize_kernel<EVEN, VEC, ADD>), dim3(a.mxp / RS_XS, cdiv(a.TC, RS_PC), planes), dim3(64 * RS_NW),
                     lds, s, a);
  return check_launch("spectral_resize_kernel");
}

}  // namespace dpot
