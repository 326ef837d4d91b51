// evalmetrics3d.hip - the PDEBench metric set of the reference's Evaluator(temporal=True, griddata=True, component=c), one
// column per channel c (utils/criterion.py:189-239 with the 3-D branch of compute_fourier_error, :295-340), for channels-last
// 3-D rollouts [B, X, Y, Z, T, C], kept on the device: normalised mean-absolute / root-mean-square / maximum error, the error on
// the six faces and the error spectrum summed over radial wavenumber shells of the positive octant.  Three launches per
// update, no host synchronisation, no atomics.  The transform is separable and only the low half of every axis is wanted:
//
// eval3_z_kernel: e = pred - target is formed in fp32 when a value is loaded (the DFT is linear: the difference is transformed,
//   never the two fields).  The field is a matrix [R = X Y rows r = (x, y)][Z][TC]; a wave owns tiles of 16 rows and contracts z:
//     Gc[k, r] = sum_z cos(2 pi k z / nz) e[r, z],  Gs = the same with sin,  0 <= k < nz/2
//   as fp32 MFMA products, A = the table fragments (global, cache resident), B = e straight from the two loads of one (r, z)
//   (16 bytes each = the 4 planes p = (t, c) of a chunk).  A workgroup holds up to E3_NKT = 4 tiles of 16 wavenumbers k in
//   registers (nz <= 128: every k, so pred and target are read once); beyond that the k stripes are further workgroups that
//   re-read the rows (neighbours in the grid: L2 / MALL).  The pointwise statistics ride on the VALU beside the MFMAs; a row
//   tile is counted by ONE k stripe (tile modulo stripes): per lane sum|e|, sum|t|, sum e^2, sum t^2, max|e|, max|t| and the
//   face sum (weight = number of the six faces the point lies on: edges twice, corners three times, as the reference adds whole
//   faces), per plane.  Written: the half spectrum G [B][TC][nz/2][Gc|Gs][R] (fp32, as many values as e has for even nz) and
//   [B][TC][parts][8] statistics partials, one per workgroup.
// eval3_xy_kernel: one workgroup per (b, plane), stripe of E3_IS = 16 wavenumbers i and pair of wavenumbers k.  For each k the
//   complex plane g[x, y] = Gc - 1j Gs takes the 2-D positive-quadrant transform with both passes through LDS, as
//   evalmetrics.hip treats a real plane:
//   pass 1 (X)  the four real planes (Gc, Gs of two k) against the cos / sin tables of x (MFMA), combined in registers to
//               U = sum_x g exp(-2 pi 1j i x / nx):  Re U = C Gc - S Gs,  Im U = -(C Gs + S Gc); rows (Re|Im, i, k), y contiguous.
//   pass 2 (Y)  Re E = Re U Cy^T + Im U Sy^T,  Im E = Im U Cy^T - Re U Sy^T for 0 <= j < ny/2; |E|^2 stays in registers.
//   shell sum   |E|^2 of the stripe goes to LDS (over U, which is dead); thread (k, s) adds, for i ascending, the j range of
//               shell s in row (k, i) (host table jlo[k][i][s] .. jlo[k][i][s+1], integer arithmetic) in ascending j: a fixed
//               order.  The full spectrum never reaches HBM; what does is [B][TC][nz/2][stripes][K] shell partials.
// eval3_finalize_kernel: one wave per accumulator entry adds the partials (lane-strided, then a butterfly: a fixed order) and
//   the samples in order (double) and folds the per-sample ratios into the accumulator (the arithmetic of an entry:
//   evalmetrics_common.h, shared with evalmetrics.hip, as are the pointwise statistics and their reduction).
// Bytes per update: pred and target are read once from HBM (stripes beyond nz = 128 re-read through L2), G is written once and
// read once per i stripe (nx / 32 of them, neighbours in the grid); everything else is tables and partials.
// Nothing outside the tensors is read: loads past a row, past nz or past TC are predicated to 0.0f, which adds nothing to
// any statistic, and G is read only where eval3_z_kernel wrote it.
#include "evalmetrics_common.h"

namespace dpot {

constexpr int E3_PC = EVAL_PC;             // planes (t, c) per workgroup of the z pass
constexpr int E3_NW = EVAL_NW;             // waves
constexpr int E3_NKT = 4;                  // 16-wavenumber k tiles a wave of the z pass can hold
constexpr int E3_TPW = 1;                  // row tiles per wave of the z pass (4: 64 workgroups at [1, 128^3, 1, 4] - measured slower)
constexpr int E3_TPG = E3_NW * E3_TPW;     // row tiles per workgroup
constexpr int E3_IS = 16;                  // wavenumbers i per workgroup of the xy pass
constexpr int E3_KC = 2;                   // wavenumbers k per workgroup of the xy pass
constexpr int E3_ROWS = 2 * E3_IS * E3_KC; // rows (Re|Im, i, k) of the LDS intermediate
constexpr int E3_CT = 4;                   // j tiles a wave can hold in registers: ny/2 <= 16 * E3_NW * E3_CT
constexpr int E3_NY_MAX = 512;             // (E3_NY_MAX + 4) * E3_ROWS floats = 129 KiB of LDS
constexpr int E3_NX_MAX = 512;
constexpr int E3_NZ_MAX = 512;

struct Eval3ZArgs {
  const float* pred;
  const float* target;
  const float* czT;     // [nzp][hzp]  cos(2 pi k z / nz), row z
  const float* szT;     // [nzp][hzp]  sin
  float* G;             // [B][TC][hz][2][R]
  double* statp;        // [B][TC][parts][8]
  int nx, ny, nz, TC, hz, nzp, hzp, R, ntiles, nstripes, nchunks;
  int tpw;              // row tiles per wave = E3_TPW, as a run-time value: see eval3_z_kernel
};

// one tile of 16 rows r: its NKT k tiles of Gc and Gs into G; STATS: this tile's points are counted here
template <bool VEC, int NKT, bool STATS>
__device__ __forceinline__ void eval3_z_tile(const Eval3ZArgs& a, const float* __restrict__ pr, const float* __restrict__ tg,
                                             float* __restrict__ Gb, int rt, int kt0, int p0, int npc, int lr, int lg,
                                             EvalStats& st) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int r = rt * 16 + lr;
  const bool rok = r < a.R;
  const int x = r / a.ny, y = r - x * a.ny;
  const float wxy = (x == 0 ? 1.f : 0.f) + (x == a.nx - 1 ? 1.f : 0.f) + (y == 0 ? 1.f : 0.f) + (y == a.ny - 1 ? 1.f : 0.f);
  const int nkt = a.hzp / 16 - kt0 < NKT ? a.hzp / 16 - kt0 : NKT;    // real k tiles of this stripe (>= 1)
  f32x4 acc[NKT][2][E3_PC];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int pc = 0; pc < E3_PC; ++pc) acc[kt][q][pc] = zero4;
#pragma unroll 1
  for (int z0 = 0; z0 < a.nzp; z0 += 16) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int z = z0 + 4 * s + lg;
      f32x4 p = zero4, t = zero4;
      if (rok && z < a.nz) {
        const size_t o = ((size_t)r * a.nz + z) * a.TC + p0;
        if (VEC) {
          p = *reinterpret_cast<const f32x4*>(pr + o);
          t = *reinterpret_cast<const f32x4*>(tg + o);
        } else {
#pragma unroll
          for (int pc = 0; pc < E3_PC; ++pc)
            if (pc < npc) {
              p[pc] = pr[o + pc];
              t[pc] = tg[o + pc];
            }
        }
      }
      const f32x4 e = p - t;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
        if (kt < nkt) {
          const size_t ao = (size_t)z * a.hzp + (kt0 + kt) * 16 + lr;   // z < nzp, k < hzp: inside the padded tables
          const float ac = a.czT[ao], as = a.szT[ao];
#pragma unroll
          for (int pc = 0; pc < E3_PC; ++pc) {
            acc[kt][0][pc] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac, e[pc], acc[kt][0][pc], 0, 0, 0);
            acc[kt][1][pc] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, e[pc], acc[kt][1][pc], 0, 0, 0);
          }
        }
      if (STATS) {
        const float w = wxy + (z == 0 ? 1.f : 0.f) + (z == a.nz - 1 ? 1.f : 0.f);   // out-of-range points hold e = 0
        eval_stats_point(st, e, t, w);
      }
    }
  }
  // accumulator: column = lr (row r of the field), row = 4 lg + reg (k inside the tile).  One running pointer, and a
  // scheduling barrier per group of stores: left alone the compiler forms all 32 NKT addresses first and spills
  if (rok) {
    const size_t R2 = 2 * (size_t)a.R;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int pc = 0; pc < E3_PC; ++pc) {
        const int k0 = (kt0 + kt) * 16 + 4 * lg;
        if (kt < nkt && pc < npc) {
          float* __restrict__ g = Gb + ((size_t)(p0 + pc) * a.hz + k0) * R2 + r;
#pragma unroll
          for (int rg = 0; rg < 4; ++rg)
            if (k0 + rg < a.hz) {
              g[rg * R2] = acc[kt][0][pc][rg];
              g[rg * R2 + a.R] = acc[kt][1][pc][rg];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
  }
}

template <bool VEC, int NKT>
__global__ __launch_bounds__(64 * E3_NW) void eval3_z_kernel(const Eval3ZArgs a) {
  __shared__ double wstat[E3_NW * E3_PC * 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int chunk = blockIdx.x, stripe = blockIdx.y % a.nstripes, p0 = (blockIdx.y / a.nstripes) * E3_PC, b = blockIdx.z;
  const size_t boff = (size_t)b * a.R * a.nz * a.TC;
  const float* __restrict__ pr = a.pred + boff;
  const float* __restrict__ tg = a.target + boff;
  float* __restrict__ Gb = a.G + (size_t)b * a.TC * a.hz * 2 * a.R;
  const int npc = a.TC - p0 < E3_PC ? a.TC - p0 : E3_PC;

  // zeroed here and not by eval_stats_zero: through the helper (or `= {}`) the one-tile kernels are allocated 128 / 135 VGPRs
  // instead of 142 / 146 and change occupancy; every other shared helper leaves this kernel's registers as they were
  EvalStats st;
#pragma unroll
  for (int pc = 0; pc < E3_PC; ++pc) st.ae[pc] = st.at[pc] = st.se[pc] = st.st[pc] = st.me[pc] = st.mt[pc] = st.bd[pc] = 0.f;
  // a.tpw is a run-time value so that this stays a loop around ONE copy of each tile body: with the constant 1 the compiler
  // merges the two bodies' schedules and the 4-tile kernel spills 132 bytes per lane to scratch
#pragma unroll 1
  for (int q = 0; q < a.tpw; ++q) {
    const int rt = (chunk * a.tpw + q) * E3_NW + wave;
    if (rt >= a.ntiles) break;
    if (rt % a.nstripes == stripe)                                 // one owner per tile
      eval3_z_tile<VEC, NKT, true>(a, pr, tg, Gb, rt, stripe * NKT, p0, npc, lr, lg, st);
    else
      eval3_z_tile<VEC, NKT, false>(a, pr, tg, Gb, rt, stripe * NKT, p0, npc, lr, lg, st);
  }
  eval_stats_wave_reduce(st, wstat, wave, lane);
  __syncthreads();
  eval_stats_store(wstat, a.statp, (size_t)b * a.TC + p0, npc, a.nchunks * a.nstripes, chunk * a.nstripes + stripe);
}

// ---- the two remaining axes and the shell sums ---------------------------------------------------------------------------
struct Eval3XYArgs {
  const float* G;       // [B * TC][hz][2][nx * ny]
  const float* cxT;     // [nxp][hxp]  cos(2 pi i x / nx), row x
  const float* sxT;     // [nxp][hxp]  sin
  const float* cy;      // [nyp][hyp]  cos(2 pi j y / ny), row y
  const float* sy;      // [nyp][hyp]  sin
  const int* jlo;       // [hz][hx][K + 1] first j of shell s in row (k, i)
  float* specp;         // [B * TC][hz][ns][K]
  int nx, ny, hx, hy, hz, K, nxp, nyp, hxp, hyp;
};

__global__ __launch_bounds__(64 * E3_NW) void eval3_xy_kernel(const Eval3XYArgs a) {
  extern __shared__ __attribute__((aligned(16))) float e3_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int stripe = blockIdx.x, ns = gridDim.x;
  const int i0 = stripe * E3_IS, k0z = blockIdx.y * E3_KC, bp = blockIdx.z;
  const int LD = a.nyp + 4;                                        // + 4: rows 16 bytes apart from a bank-aligned stride
  const size_t R = (size_t)a.nx * a.ny;
  const float* __restrict__ Gp = a.G + (size_t)bp * a.hz * 2 * R;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // ---- pass 1: contract x ------------------------------------------------------------------------------------------------
  for (int yt = wave; yt < a.nyp / 16; yt += E3_NW) {
    const int y = yt * 16 + lr;
    const bool yok = y < a.ny;
    f32x4 acc[2][2 * E3_KC];                                       // [cos|sin table][plane = 2 kk + (Gc|Gs)]
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int pl = 0; pl < 2 * E3_KC; ++pl) acc[q][pl] = zero4;
    for (int x0 = 0; x0 < a.nxp; x0 += 16) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int x = x0 + 4 * s + lg;
        float g[2 * E3_KC];
#pragma unroll
        for (int pl = 0; pl < 2 * E3_KC; ++pl) {
          const int k = k0z + (pl >> 1);
          g[pl] = (yok && x < a.nx && k < a.hz) ? Gp[((size_t)k * 2 + (pl & 1)) * R + (size_t)x * a.ny + y] : 0.f;
        }
        const size_t ao = (size_t)x * a.hxp + i0 + lr;             // x < nxp: inside the padded tables
        const float ac = a.cxT[ao], as = a.sxT[ao];
#pragma unroll
        for (int pl = 0; pl < 2 * E3_KC; ++pl) {
          acc[0][pl] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac, g[pl], acc[0][pl], 0, 0, 0);
          acc[1][pl] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, g[pl], acc[1][pl], 0, 0, 0);
        }
      }
    }
    // accumulator: column = lr (y), row = 4 lg + reg (i inside the stripe)
#pragma unroll
    for (int kk = 0; kk < E3_KC; ++kk) {
      const f32x4 ur = acc[0][2 * kk] - acc[1][2 * kk + 1];        // C Gc - S Gs
      const f32x4 ui = -(acc[0][2 * kk + 1] + acc[1][2 * kk]);     // -(C Gs + S Gc)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e3_lds[((4 * lg + r) * E3_KC + kk) * LD + y] = ur[r];
        e3_lds[((E3_IS + 4 * lg + r) * E3_KC + kk) * LD + y] = ui[r];
      }
    }
  }
  __syncthreads();

  // ---- pass 2: contract y, |E|^2 in registers ----------------------------------------------------------------------------
  constexpr int NT = E3_IS * E3_KC / 16;                           // 16-row tiles of one of Re U, Im U
  f32x4 spec[E3_CT][NT];
#pragma unroll
  for (int c = 0; c < E3_CT; ++c) {
    const int ct = wave + c * E3_NW;
#pragma unroll
    for (int t = 0; t < NT; ++t) spec[c][t] = zero4;
    if (ct < a.hyp / 16) {
      const int jo = ct * 16 + lr;
      f32x4 re[NT], im[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) re[t] = im[t] = zero4;
      for (int y0 = 0; y0 < a.nyp; y0 += 16) {
        float bc[4], bs[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const size_t o = (size_t)(y0 + 4 * lg + s) * a.hyp + jo;
          bc[s] = a.cy[o];
          bs[s] = a.sy[o];
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f32x4 ar = *reinterpret_cast<const f32x4*>(&e3_lds[(16 * t + lr) * LD + y0 + 4 * lg]);
          const f32x4 ai = *reinterpret_cast<const f32x4*>(&e3_lds[(E3_IS * E3_KC + 16 * t + lr) * LD + y0 + 4 * lg]);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            re[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[s], bc[s], re[t], 0, 0, 0);
            re[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai[s], bs[s], re[t], 0, 0, 0);
            im[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai[s], bc[s], im[t], 0, 0, 0);
            im[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[s], -bs[s], im[t], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) spec[c][t] = re[t] * re[t] + im[t] * im[t];
    }
  }
  __syncthreads();                                                 // every wave is done with U

  // ---- shell sum -----------------------------------------------------------------------------------------------------
  // accumulator: column = lr (j), row 16 t + 4 lg + reg of the rows (i, kk): i = (16 t + 4 lg + reg) / E3_KC, kk = the rest
  const int SLD = a.hyp + 1;
#pragma unroll
  for (int c = 0; c < E3_CT; ++c) {
    const int ct = wave + c * E3_NW;
    if (ct < a.hyp / 16) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * t + 4 * lg + r;
          e3_lds[((row % E3_KC) * E3_IS + row / E3_KC) * SLD + ct * 16 + lr] = spec[c][t][r];
        }
    }
  }
  __syncthreads();
  const int kk = threadIdx.x % E3_KC, k = k0z + kk;
  const int ni = a.hx - i0 < E3_IS ? a.hx - i0 : E3_IS;            // real rows of this stripe (>= 1)
  if (k < a.hz) {
    for (int s = threadIdx.x / E3_KC; s < a.K; s += 64 * E3_NW / E3_KC) {
      float sum = 0.f;
      for (int il = 0; il < ni; ++il) {
        const int* jl = a.jlo + ((size_t)k * a.hx + i0 + il) * (a.K + 1) + s;
        const int j1 = jl[1];
        for (int j = jl[0]; j < j1; ++j) sum += e3_lds[(kk * E3_IS + il) * SLD + j];
      }
      a.specp[(((size_t)bp * a.hz + k) * ns + stripe) * a.K + s] = sum;
    }
  }
}

// ---- finalize ------------------------------------------------------------------------------------------------------
// One WAVE per accumulator entry (eval_finalize_entry): lane l takes the partials l, l + 64, ... in order and a butterfly
// combines the lanes - a fixed order for a shape, and a + b = b + a keeps the lanes identical.  (One thread per entry, as
// evalmetrics.hip has it, walks nz/2 x stripes shell partials and row-tiles / 4 statistics partials one after the other:
// measured 84 - 183 us.)
struct Eval3Gather {
  const double* __restrict__ statp;      // [B][TC][parts][8]
  const float* __restrict__ specp;       // [B][TC][nq = (k, i stripe)][K]
  int TC, parts, nq, K, lane;
  __device__ __forceinline__ bool writes() const { return lane == 0; }
  __device__ __forceinline__ void plane_stats(int b, int p, double* v) const {
    const double* r = statp + ((size_t)b * TC + p) * parts * 8;
#pragma unroll
    for (int k = 0; k < EVAL_NSTAT; ++k) v[k] = 0.0;               // sums of magnitudes and maxima of magnitudes: 0 is neutral
    for (int s = lane; s < parts; s += 64) eval_stats_fold(v, r + (size_t)s * 8);
    v[0] = wave_sum_d(v[0]), v[1] = wave_sum_d(v[1]), v[2] = wave_sum_d(v[2]), v[3] = wave_sum_d(v[3]), v[6] = wave_sum_d(v[6]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      v[4] = eval_max_nan(v[4], __shfl_xor(v[4], off, 64));
      v[5] = eval_max_nan(v[5], __shfl_xor(v[5], off, 64));
    }
  }
  __device__ __forceinline__ double shell_sum(double sum, int b, int p, int s) const {
    const float* r = specp + ((size_t)b * TC + p) * nq * K + s;
    double part = 0.0;
    for (int q = lane; q < nq; q += 64) part += (double)r[(size_t)q * K];
    return sum + wave_sum_d(part);
  }
};

__global__ __launch_bounds__(256) void eval3_finalize_kernel(const double* __restrict__ statp, const float* __restrict__ specp,
                                                             double* __restrict__ acc, int B, double faces, int T, int C,
                                                             int parts, int nq, int K) {
  const Eval3Gather g = {statp, specp, T * C, parts, nq, K, (int)(threadIdx.x & 63)};
  eval_finalize_entry(g, blockIdx.x * 4ll + (threadIdx.x >> 6), acc, B, faces, T, C, K);   // the entry is wave-uniform
}

struct Eval3Geom {
  int hx, hy, hz, K, nxp, nyp, nzp, hxp, hyp, hzp, ns, nkt, nstripes, ntiles, nchunks, parts;
};

static Eval3Geom eval3_geom(int nx, int ny, int nz) {
  Eval3Geom g;
  g.hx = nx / 2, g.hy = ny / 2, g.hz = nz / 2;
  g.K = g.hx < g.hy ? (g.hx < g.hz ? g.hx : g.hz) : (g.hy < g.hz ? g.hy : g.hz);
  g.nxp = eval_pad(nx, 0), g.nyp = eval_pad(ny, 0), g.nzp = eval_pad(nz, 0);
  g.hxp = eval_pad(nx, 1), g.hyp = eval_pad(ny, 1), g.hzp = eval_pad(nz, 1);
  g.ns = g.hxp / E3_IS;
  const int ktiles = g.hzp / 16;
  g.nkt = ktiles >= 3 ? E3_NKT : ktiles;                           // 1, 2 or 4 k tiles per workgroup of the z pass
  g.nstripes = cdiv(ktiles, g.nkt);
  g.ntiles = cdiv(nx * ny, 16);
  g.nchunks = cdiv(g.ntiles, E3_TPG);
  g.parts = g.nchunks * g.nstripes;
  return g;
}

static bool eval3_size_ok(const char* what, int nx, int ny, int nz) {
  if (nx > E3_NX_MAX || ny > E3_NY_MAX || nz > E3_NZ_MAX) {
    set_error("%s: field %dx%dx%d is beyond the supported size (nx <= %d; ny <= %d, the LDS intermediate of a workgroup; "
              "nz <= %d)", what, nx, ny, nz, E3_NX_MAX, E3_NY_MAX, E3_NZ_MAX);
    return false;
  }
  return true;
}

template <bool VEC>
static void eval3_launch_z(const Eval3ZArgs& a, int nkt, dim3 grid, hipStream_t stream) {
  if (nkt == 1)
    hipLaunchKernelGGL((eval3_z_kernel<VEC, 1>), grid, dim3(64 * E3_NW), 0, stream, a);
  else if (nkt == 2)
    hipLaunchKernelGGL((eval3_z_kernel<VEC, 2>), grid, dim3(64 * E3_NW), 0, stream, a);
  else
    hipLaunchKernelGGL((eval3_z_kernel<VEC, E3_NKT>), grid, dim3(64 * E3_NW), 0, stream, a);
}

}  // namespace dpot

using namespace dpot;

extern "C" int dpot_eval3_pad(int n, int half) { return eval_pad(n, half); }

extern "C" int dpot_eval3_max_size(int axis) { return axis == 0 ? E3_NX_MAX : axis == 1 ? E3_NY_MAX : E3_NZ_MAX; }

extern "C" int64_t dpot_eval3_acc_elems(int nx, int ny, int nz, int T, int C) {
  if (nx < 2 || ny < 2 || nz < 2 || T < 1 || C < 1) return 0;
  return eval_acc_elems(eval3_geom(nx, ny, nz).K, T, C);
}

extern "C" int64_t dpot_eval3_work_elems(int which, int B, int nx, int ny, int nz, int TC) {
  if (B < 1 || nx < 2 || ny < 2 || nz < 2 || TC < 1 || nx > E3_NX_MAX || ny > E3_NY_MAX || nz > E3_NZ_MAX) return 0;
  const Eval3Geom g = eval3_geom(nx, ny, nz);
  const int64_t bp = (int64_t)B * TC;
  if (which == 0) return bp * g.parts * 8;                         // statp, doubles
  if (which == 1) return bp * g.hz * g.ns * g.K;                   // specp, floats
  if (which == 2) return bp * g.hz * 2 * nx * ny;                  // G, floats
  return 0;
}

extern "C" int dpot_eval3_stats(const float* pred, const float* target, const float* cxT, const float* sxT, const float* cy,
                                const float* sy, const float* czT, const float* szT, const int32_t* jlo, double* statp,
                                float* specp, float* G, int B, int nx, int ny, int nz, int TC, dpot_stream_t stream) {
  DPOT_REQUIRE(pred && target && cxT && sxT && cy && sy && czT && szT && jlo && statp && specp && G, "eval3_stats: null pointer");
  DPOT_REQUIRE(B > 0 && B <= 65535 && nx > 1 && ny > 1 && nz > 1 && TC > 0,
               "eval3_stats: bad sizes B=%d field=%dx%dx%d TC=%d (every spatial size must be >= 2)", B, nx, ny, nz, TC);
  DPOT_REQUIRE((reinterpret_cast<uintptr_t>(statp) & 7u) == 0, "eval3_stats: statp must be 8-byte aligned");
  if (!eval3_size_ok("eval3_stats", nx, ny, nz)) return DPOT_EUNSUP;
  const Eval3Geom g = eval3_geom(nx, ny, nz);
  DPOT_REQUIRE((int64_t)cdiv(TC, E3_PC) * g.nstripes <= 65535 && (int64_t)B * TC <= 65535 && cdiv(g.hz, E3_KC) <= 65535,
               "eval3_stats: B=%d with T*C=%d planes is beyond the launch grid (B * T*C <= 65535)", B, TC);
  static_assert(E3_NY_MAX / 2 <= 16 * E3_NW * E3_CT, "a wave cannot hold its j tiles");
  static_assert(E3_KC * E3_IS * (E3_NY_MAX / 2 + 16 + 1) <= E3_ROWS * (E3_NY_MAX + 4), "|E|^2 must fit over U");
  static_assert(sizeof(float) * E3_ROWS * (E3_NY_MAX + 4) <= LDS_BYTES, "the LDS intermediate of the largest ny");
  const size_t lds = sizeof(float) * (size_t)E3_ROWS * (g.nyp + 4);
  DPOT_REQUIRE(lds <= (size_t)LDS_BYTES, "eval3_stats: ny=%d needs %zu bytes of LDS, a workgroup has %d", ny, lds, LDS_BYTES);
  if (int rc = raise_dynamic_lds<eval3_xy_kernel>("eval3_stats")) return rc;

  Eval3ZArgs z;
  z.pred = pred, z.target = target, z.czT = czT, z.szT = szT, z.G = G, z.statp = statp;
  z.nx = nx, z.ny = ny, z.nz = nz, z.TC = TC, z.hz = g.hz, z.nzp = g.nzp, z.hzp = g.hzp, z.R = nx * ny;
  z.ntiles = g.ntiles, z.nstripes = g.nstripes, z.nchunks = g.nchunks, z.tpw = E3_TPW;
  const dim3 zgrid(g.nchunks, cdiv(TC, E3_PC) * g.nstripes, B);
  if (TC % 4 == 0 && aligned16(pred) && aligned16(target))
    eval3_launch_z<true>(z, g.nkt, zgrid, as_stream(stream));
  else
    eval3_launch_z<false>(z, g.nkt, zgrid, as_stream(stream));
  const int rc = check_launch("eval3_z_kernel");
  if (rc != DPOT_OK) return rc;

  Eval3XYArgs a;
  a.G = G, a.cxT = cxT, a.sxT = sxT, a.cy = cy, a.sy = sy, a.jlo = jlo, a.specp = specp;
  a.nx = nx, a.ny = ny, a.hx = g.hx, a.hy = g.hy, a.hz = g.hz, a.K = g.K;
  a.nxp = g.nxp, a.nyp = g.nyp, a.hxp = g.hxp, a.hyp = g.hyp;
  hipLaunchKernelGGL(eval3_xy_kernel, dim3(g.ns, cdiv(g.hz, E3_KC), B * TC), dim3(64 * E3_NW), lds, as_stream(stream), a);
  return check_launch("eval3_xy_kernel");
}

extern "C" int dpot_eval3_finalize(const double* statp, const float* specp, double* acc, int B, int nx, int ny, int nz, int T,
                                   int C, dpot_stream_t stream) {
  DPOT_REQUIRE(statp && specp && acc, "eval3_finalize: null pointer");
  DPOT_REQUIRE(B > 0 && nx > 1 && ny > 1 && nz > 1 && T > 0 && C > 0, "eval3_finalize: bad sizes B=%d field=%dx%dx%d T=%d C=%d",
               B, nx, ny, nz, T, C);
  DPOT_REQUIRE(((reinterpret_cast<uintptr_t>(statp) | reinterpret_cast<uintptr_t>(acc)) & 7u) == 0,
               "eval3_finalize: statp and acc must be 8-byte aligned");
  if (!eval3_size_ok("eval3_finalize", nx, ny, nz)) return DPOT_EUNSUP;
  const Eval3Geom g = eval3_geom(nx, ny, nz);
  const double faces = 2.0 * nx * ny + 2.0 * ny * nz + 2.0 * nz * nx;
  hipLaunchKernelGGL(eval3_finalize_kernel, dim3((unsigned)cdiv64(eval_finalize_items(g.K, T, C), 4)), dim3(256), 0,
                     as_stream(stream), statp, specp, acc, B, faces, T, C, g.parts, g.hz * g.ns, g.K);
  return check_launch("eval3_finalize_kernel");
}
