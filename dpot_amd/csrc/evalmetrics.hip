// evalmetrics.hip - the PDEBench metric set of the reference's Evaluator(temporal=True, griddata=True, component='all')
// (utils/criterion.py:189-239 with compute_fourier_error, :246-360) for channels-last rollouts [B, X, Y, T, C], kept on the
// device: normalised mean-absolute / root-mean-square / maximum error, the boundary error and the error spectrum summed over
// radial wavenumber shells of the positive quadrant.  Two launches per update, no host synchronisation, no atomics.
//
// eval_stats_kernel: one workgroup per (b, stripe of EV_IS = 16 wavenumbers i, chunk of EV_PC = 4 planes p = (t, c)), EV_NW waves.
//   e = pred - target is formed in fp32 when a value is loaded (the DFT is linear: the difference is transformed, not the two
//   fields - no cancellation of two large spectra).
//   pass 1 (X)  P[(i, pc), y] = sum_x cos(2 pi i x / nx) e[x, y, pc],  Q = the same with sin.  A = the table fragments (global,
//               cache resident), B = e straight from the two loads of one (x, y) (16 bytes each = the 4 planes), wave w owns
//               the y tiles w, w + EV_NW, ...; P and Q go to LDS, row (P|Q, i, pc), y contiguous - the layout of resize.hip.
//               The pointwise statistics ride on the VALU beside the MFMAs: every (x, y) of the chunk passes through exactly
//               one lane of every stripe's workgroup, so a y tile is counted by ONE stripe (round + wave modulo n_stripes): per lane
//               sum|e|, sum|t|, sum e^2, sum t^2, max|e|, max|t| and the boundary sum (weight = number of the four edges the
//               point lies on: corners twice, as the reference adds rows and columns), per plane.  pred and target therefore
//               leave HBM once per update (the other stripes' re-reads are neighbouring workgroups: L2 / MALL).
//   pass 2 (Y)  Re E = P Cy^T - Q Sy^T, Im E = -(Q Cy^T + P Sy^T) for 0 <= j < ny/2: A = P, Q from LDS, B = the y tables; a wave
//               owns the j tiles w, w + EV_NW, ... (at most EV_CT of them) and keeps |E|^2 = Re^2 + Im^2 in registers.
//   shell sum   |E|^2 of the stripe goes to LDS (over P / Q, which are dead), then thread (pc, s) adds, for i ascending, the
//               j range of shell s in row i (host table jlo[i][s] .. jlo[i][s+1], integer arithmetic) in ascending j: a fixed
//               order.  The spectrum never reaches HBM; what does is [b][plane][stripe][K] shell partials and
//               [b][plane][stripe][8] statistics partials.
// eval_finalize_kernel: one thread per accumulator entry adds the stripes and the samples in order (double) and folds the
//   per-sample ratios into the accumulator (the arithmetic of an entry: evalmetrics_common.h, shared with evalmetrics3d.hip,
//   as are the pointwise statistics and their reduction).
// Nothing outside the tensors is read: loads past nx, ny or TC are predicated to 0.0f, which adds nothing to any statistic.
#include "evalmetrics_common.h"

namespace dpot {

constexpr int EV_IS = 16;                  // wavenumbers i per workgroup (one 16-row MFMA tile each for cos and sin)
constexpr int EV_PC = EVAL_PC;             // planes per workgroup
constexpr int EV_ROWS = 2 * EV_IS * EV_PC; // rows (P|Q, i, pc) of the LDS intermediate
constexpr int EV_NW = EVAL_NW;             // waves
constexpr int EV_CT = 3;                   // j tiles a wave can hold in registers: ny/2 <= 16 * EV_NW * EV_CT
constexpr int EV_TAIL = EV_NW * EV_PC * 8 * 8;                     // bytes behind the intermediate: the waves' statistics
constexpr int EV_LD_MAX = (LDS_BYTES - EV_TAIL) / 4 / EV_ROWS;    // LDS row length nyp + 4 a workgroup can hold
constexpr int EV_NY_MAX = (EV_LD_MAX - 4) / 16 * 16;               // 304
constexpr int EV_NX_MAX = 1024;

struct EvalArgs {
  const float* pred;
  const float* target;
  const float* cxT;     // [nxp][hxp]  cos(2 pi i x / nx), row x
  const float* sxT;     // [nxp][hxp]  sin
  const float* cy;      // [nyp][hyp]  cos(2 pi j y / ny), row y
  const float* sy;      // [nyp][hyp]  sin
  const int* jlo;       // [hx][K + 1] first j of shell s in row i
  double* statp;        // [B][TC][ns][8]
  float* specp;         // [B][TC][ns][K]
  int nx, ny, TC, hx, hy, K, nxp, nyp, hxp, hyp;
};

struct EvalChunk {      // the operands of 16 k (= x) values of pass 1, per lane
  f32x4 p[4], t[4];
  float ac[4], as[4];
};

template <bool VEC>
__device__ __forceinline__ void eval_load_chunk(EvalChunk& c, const EvalArgs& a, const float* __restrict__ pr,
                                                const float* __restrict__ tg, int k0, int y, bool yok, int i0, int p0, int npc,
                                                int lr, int lg) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int x = k0 + 4 * s + lg;
    f32x4 p = {0.f, 0.f, 0.f, 0.f}, t = {0.f, 0.f, 0.f, 0.f};
    if (yok && x < a.nx) {
      const size_t o = ((size_t)x * a.ny + y) * a.TC + p0;
      if (VEC) {
        p = *reinterpret_cast<const f32x4*>(pr + o);
        t = *reinterpret_cast<const f32x4*>(tg + o);
      } else {
#pragma unroll
        for (int pc = 0; pc < EV_PC; ++pc)
          if (pc < npc) {
            p[pc] = pr[o + pc];
            t[pc] = tg[o + pc];
          }
      }
    }
    c.p[s] = p;
    c.t[s] = t;
    const size_t ao = (size_t)x * a.hxp + i0 + lr;                 // x < nxp: inside the padded tables
    c.ac[s] = a.cxT[ao];
    c.as[s] = a.sxT[ao];
  }
}

// one y tile of pass 1: P and Q of the stripe into LDS; STATS: this tile's points are counted here
template <bool VEC, bool STATS>
__device__ __forceinline__ void eval_pass1_tile(const EvalArgs& a, const float* __restrict__ pr, const float* __restrict__ tg,
                                                float* __restrict__ lds, int LD, int yt, int i0, int p0, int npc, int lr, int lg,
                                                EvalStats& st) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int y = yt * 16 + lr;
  const bool yok = y < a.ny;
  const float wy = (y == 0 ? 1.f : 0.f) + (y == a.ny - 1 ? 1.f : 0.f);
  f32x4 acc[2][EV_PC];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int pc = 0; pc < EV_PC; ++pc) acc[q][pc] = zero4;
  EvalChunk cur, nxt;
  eval_load_chunk<VEC>(cur, a, pr, tg, 0, y, yok, i0, p0, npc, lr, lg);
  for (int k0 = 0; k0 < a.nxp; k0 += 16) {
    if (k0 + 16 < a.nxp) eval_load_chunk<VEC>(nxt, a, pr, tg, k0 + 16, y, yok, i0, p0, npc, lr, lg);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const f32x4 e = cur.p[s] - cur.t[s];
#pragma unroll
      for (int pc = 0; pc < EV_PC; ++pc) {
        acc[0][pc] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.ac[s], e[pc], acc[0][pc], 0, 0, 0);
        acc[1][pc] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.as[s], e[pc], acc[1][pc], 0, 0, 0);
      }
      if (STATS) {
        const int x = k0 + 4 * s + lg;
        const float w = wy + (x == 0 ? 1.f : 0.f) + (x == a.nx - 1 ? 1.f : 0.f);   // out-of-range points hold e = 0
        eval_stats_point(st, e, cur.t[s], w);
      }
    }
    cur = nxt;
  }
  // accumulator: column = lr (y), row = 4 lg + reg (i inside the stripe)
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int pc = 0; pc < EV_PC; ++pc)
#pragma unroll
      for (int r = 0; r < 4; ++r) lds[((q * EV_IS + 4 * lg + r) * EV_PC + pc) * LD + y] = acc[q][pc][r];
}

template <bool VEC>
__global__ __launch_bounds__(64 * EV_NW, VEC ? 2 : 1) void eval_stats_kernel(const EvalArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ev_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int stripe = blockIdx.x, ns = gridDim.x;
  const int i0 = stripe * EV_IS, p0 = blockIdx.y * EV_PC, b = blockIdx.z;
  const int LD = a.nyp + 4;                                        // + 4: rows 16 bytes apart from a bank-aligned stride
  double* __restrict__ wstat = reinterpret_cast<double*>(ev_lds + (size_t)EV_ROWS * LD);   // [wave][pc][8]
  const size_t boff = (size_t)b * a.nx * a.ny * a.TC;
  const float* __restrict__ pr = a.pred + boff;
  const float* __restrict__ tg = a.target + boff;
  const int npc = a.TC - p0 < EV_PC ? a.TC - p0 : EV_PC;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // ---- pass 1: contract x, count the points --------------------------------------------------------------------------
  EvalStats st;
  eval_stats_zero(st);
  for (int yt = wave; yt < a.nyp / 16; yt += EV_NW) {
    if ((yt / EV_NW + yt % EV_NW) % ns == stripe)                  // one owner per tile, spread over the waves
      eval_pass1_tile<VEC, true>(a, pr, tg, ev_lds, LD, yt, i0, p0, npc, lr, lg, st);
    else
      eval_pass1_tile<VEC, false>(a, pr, tg, ev_lds, LD, yt, i0, p0, npc, lr, lg, st);
  }
  eval_stats_wave_reduce(st, wstat, wave, lane);
  __syncthreads();
  eval_stats_store(wstat, a.statp, (size_t)b * a.TC + p0, npc, ns, stripe);

  // ---- pass 2: contract y, |E|^2 in registers --------------------------------------------------------------------------
  f32x4 spec[EV_CT][4];
#pragma unroll
  for (int c = 0; c < EV_CT; ++c) {
    const int ct = wave + c * EV_NW;
#pragma unroll
    for (int t = 0; t < 4; ++t) spec[c][t] = zero4;
    if (ct < a.hyp / 16) {
      const int jo = ct * 16 + lr;
      f32x4 re[4], im[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) re[t] = im[t] = zero4;
      for (int k0 = 0; k0 < a.nyp; k0 += 16) {
        float bc[4], bs[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const size_t o = (size_t)(k0 + 4 * lg + s) * a.hyp + jo;
          bc[s] = a.cy[o];
          bs[s] = a.sy[o];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const f32x4 ap = *reinterpret_cast<const f32x4*>(&ev_lds[(16 * t + lr) * LD + k0 + 4 * lg]);
          const f32x4 aq = *reinterpret_cast<const f32x4*>(&ev_lds[(EV_IS * EV_PC + 16 * t + lr) * LD + k0 + 4 * lg]);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            re[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[s], bc[s], re[t], 0, 0, 0);
            re[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[s], -bs[s], re[t], 0, 0, 0);
            im[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[s], bc[s], im[t], 0, 0, 0);
            im[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[s], bs[s], im[t], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) spec[c][t] = re[t] * re[t] + im[t] * im[t];
    }
  }
  __syncthreads();                                                 // every wave is done with P and Q

  // ---- shell sum ---------------------------------------------------------------------------------------------------
  // accumulator: column = lr (j), row = 4 lg + reg = (i = 4 t + lg inside the stripe, pc = reg)
  const int SLD = a.hyp + 1;
#pragma unroll
  for (int c = 0; c < EV_CT; ++c) {
    const int ct = wave + c * EV_NW;
    if (ct < a.hyp / 16) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) ev_lds[(r * EV_IS + 4 * t + lg) * SLD + ct * 16 + lr] = spec[c][t][r];
    }
  }
  __syncthreads();
  const int pc = threadIdx.x & 3;
  const int ni = a.hx - i0 < EV_IS ? a.hx - i0 : EV_IS;            // real rows of this stripe (<= 0: none)
  for (int s = threadIdx.x >> 2; s < a.K; s += 16 * EV_NW) {
    float sum = 0.f;
    for (int il = 0; il < ni; ++il) {
      const int* jl = a.jlo + (size_t)(i0 + il) * (a.K + 1) + s;
      const int j1 = jl[1];
      for (int j = jl[0]; j < j1; ++j) sum += ev_lds[(pc * EV_IS + il) * SLD + j];
    }
    if (pc < npc) a.specp[(((size_t)b * a.TC + p0 + pc) * ns + stripe) * a.K + s] = sum;
  }
}

// ---- finalize ------------------------------------------------------------------------------------------------------
// one THREAD per accumulator entry (eval_finalize_entry) walks the stripes in order
struct EvalGather {
  const double* __restrict__ statp;      // [B][TC][ns][8]
  const float* __restrict__ specp;       // [B][TC][ns][K]
  int TC, ns, K;
  __device__ __forceinline__ bool writes() const { return true; }
  __device__ __forceinline__ void plane_stats(int b, int p, double* v) const {
    const double* r = statp + ((size_t)b * TC + p) * ns * 8;
#pragma unroll
    for (int k = 0; k < EVAL_NSTAT; ++k) v[k] = r[k];
    for (int s = 1; s < ns; ++s) eval_stats_fold(v, r += 8);
  }
  __device__ __forceinline__ double shell_sum(double sum, int b, int p, int s) const {
    const float* r = specp + ((size_t)b * TC + p) * ns * K + s;
    for (int q = 0; q < ns; ++q) sum += (double)r[(size_t)q * K];
    return sum;
  }
};

__global__ __launch_bounds__(256) void eval_finalize_kernel(const double* __restrict__ statp, const float* __restrict__ specp,
                                                            double* __restrict__ acc, int B, double faces, int T, int C, int ns,
                                                            int K) {
  const EvalGather g = {statp, specp, T * C, ns, K};
  eval_finalize_entry(g, blockIdx.x * 256ll + threadIdx.x, acc, B, faces, T, C, K);
}

}  // namespace dpot

using namespace dpot;

extern "C" int dpot_eval_metrics_pad(int n, int half) { return eval_pad(n, half); }

extern "C" int dpot_eval_metrics_max_size(int axis) { return axis == 0 ? EV_NX_MAX : EV_NY_MAX; }

extern "C" int64_t dpot_eval_metrics_acc_elems(int nx, int ny, int T, int C) {
  if (nx < 2 || ny < 2 || T < 1 || C < 1) return 0;
  return eval_acc_elems(nx / 2 < ny / 2 ? nx / 2 : ny / 2, T, C);
}

extern "C" int dpot_eval_metrics_stats(const float* pred, const float* target, const float* cxT, const float* sxT,
                                       const float* cy, const float* sy, const int32_t* jlo, double* statp, float* specp, int B,
                                       int nx, int ny, int TC, dpot_stream_t stream) {
  DPOT_REQUIRE(pred && target && cxT && sxT && cy && sy && jlo && statp && specp, "eval_metrics_stats: null pointer");
  DPOT_REQUIRE(B > 0 && B <= 65535 && nx > 1 && ny > 1 && TC > 0 && cdiv(TC, EV_PC) <= 65535,
               "eval_metrics_stats: bad sizes B=%d plane=%dx%d TC=%d (every spatial size must be >= 2)", B, nx, ny, TC);
  DPOT_REQUIRE((reinterpret_cast<uintptr_t>(statp) & 7u) == 0, "eval_metrics_stats: statp must be 8-byte aligned");
  if (nx > EV_NX_MAX || ny > EV_NY_MAX) {
    set_error("eval_metrics_stats: plane %dx%d is beyond the supported size (nx <= %d; ny <= %d, the LDS intermediate of a "
              "workgroup)", nx, ny, EV_NX_MAX, EV_NY_MAX);
    return DPOT_EUNSUP;
  }
  EvalArgs a;
  a.pred = pred, a.target = target, a.cxT = cxT, a.sxT = sxT, a.cy = cy, a.sy = sy, a.jlo = jlo;
  a.statp = statp, a.specp = specp;
  a.nx = nx, a.ny = ny, a.TC = TC, a.hx = nx / 2, a.hy = ny / 2, a.K = a.hx < a.hy ? a.hx : a.hy;
  a.nxp = eval_pad(nx, 0), a.nyp = eval_pad(ny, 0);
  a.hxp = eval_pad(nx, 1), a.hyp = eval_pad(ny, 1);
  static_assert(EV_NY_MAX / 2 <= 16 * EV_NW * EV_CT, "a wave cannot hold its j tiles");
  static_assert(EV_PC * EV_IS * (EV_NY_MAX / 2 + 16 + 1) <= EV_ROWS * (EV_NY_MAX + 4), "|E|^2 must fit over P and Q");
  const size_t lds = sizeof(float) * (size_t)EV_ROWS * (a.nyp + 4) + EV_TAIL;
  const bool vec = TC % 4 == 0 && aligned16(pred) && aligned16(target);
  const dim3 grid(a.hxp / EV_IS, cdiv(TC, EV_PC), B);
  if (vec) {
    if (int rc = raise_dynamic_lds<eval_stats_kernel<true>>("eval_metrics_stats")) return rc;
    hipLaunchKernelGGL(eval_stats_kernel<true>, grid, dim3(64 * EV_NW), lds, as_stream(stream), a);
  } else {
    if (int rc = raise_dynamic_lds<eval_stats_kernel<false>>("eval_metrics_stats")) return rc;
    hipLaunchKernelGGL(eval_stats_kernel<false>, grid, dim3(64 * EV_NW), lds, as_stream(stream), a);
  }
  return check_launch("eval_stats_kernel");
}

extern "C" int dpot_eval_metrics_finalize(const double* statp, const float* specp, double* acc, int B, int nx, int ny, int T,
                                          int C, dpot_stream_t stream) {
  DPOT_REQUIRE(statp && specp && acc, "eval_metrics_finalize: null pointer");
  DPOT_REQUIRE(B > 0 && nx > 1 && ny > 1 && T > 0 && C > 0, "eval_metrics_finalize: bad sizes B=%d plane=%dx%d T=%d C=%d", B,
               nx, ny, T, C);
  DPOT_REQUIRE(((reinterpret_cast<uintptr_t>(statp) | reinterpret_cast<uintptr_t>(acc)) & 7u) == 0,
               "eval_metrics_finalize: statp and acc must be 8-byte aligned");
  if (nx > EV_NX_MAX || ny > EV_NY_MAX) {
    set_error("eval_metrics_finalize: plane %dx%d is beyond the supported size (nx <= %d, ny <= %d)", nx, ny, EV_NX_MAX,
              EV_NY_MAX);
    return DPOT_EUNSUP;
  }
  const int ns = eval_pad(nx, 1) / EV_IS, K = nx / 2 < ny / 2 ? nx / 2 : ny / 2;
  const double edges = 2.0 * nx + 2.0 * ny;                        // corners twice, as the reference adds rows and columns
  hipLaunchKernelGGL(eval_finalize_kernel, dim3((unsigned)cdiv64(eval_finalize_items(K, T, C), 256)), dim3(256), 0,
                     as_stream(stream), statp, specp, acc, B, edges, T, C, ns, K);
  return check_launch("eval_finalize_kernel");
}
