// gemm_tn.hip - fp32 weight-gradient GEMM  C[N1, N2] = sum_t A[t, n1] * B[t, n2]   (A = dY, B = X: both stored
// token-major, the contraction runs over the ROWS of both operands; dpot_gemm_f32 with transA = 1, transB = 0).
//
// Small outputs (512 x 512 at DPOT-Tiny), 8192-long contractions, 256 CUs: the work has to be split along the
// tokens, and the kernel must make the most of each pass over its token range.  Structure:
//   * workgroup = one 128 x 128 output tile x one token range (split-K, partial sums to the workspace; the existing
//     fixed-order reduce kernels of gemm.hip finish: bias-gradient column sums, AFNO un-packing, accumulate ...);
//   * 4 compute waves in a 2 x 2 grid, each 64 x 64 = 4 x 4 accumulators of v_mfma_f32_16x16x4_f32, + 2 loader waves
//     that only issue LDS-DMA: a token row of a tile is 512 contiguous bytes, two rows per wave-instruction, the slab of
//     32 tokens lands in LDS exactly as it lies in memory ([tok][128] for each operand);
//   * ROW-INTERLEAVED fragments: the MFMA A operand wants, per lane, one element (row n, token k).  A ds_read_b128 at
//     [tok = 4q + (lane >> 4)][4 * (lane & 15) .. +3] hands every lane FOUR of them - for the four 16-row tiles made of
//     the rows n = 4 i + e (e = 0..3).  Which 16 rows form a tile is a free choice, so 64 rows of an operand cost one
//     LDS instruction per 4-token step: 2 ds_read_b128 per 16 MFMAs.  The interleave also makes the accumulator layout
//     store-friendly: a lane holds 4 consecutive columns of one output row -> 16-byte global stores, no LDS staging;
//   * ring of 4 slabs of 32 tokens (128 KiB), loaders 3 slabs ahead with counted vmcnt, ONE barrier per slab (8
//     MFMA k-steps = 128 MFMAs per wave between barriers), the first fragments of slab t+1 fetched before the barrier
//     (the loaders guarantee slab t+1 at barrier t).  Variants measured at 512 x 512 x 8192 (split 16, incl. the reduce
//     launch; generic kernel of gemm.hip: 57.4 us): 16-token slabs 54.1 us; 8 compute waves (two token groups added
//     through LDS at the end) 55.8; 8-slab ring / 6 ahead 57.2 - neither wave-level parallelism nor DMA depth is the
//     limiter, the per-slab barrier + first-fragment latency is;
//   * bias gradients (column sums of one operand over the tokens) come from the fragments the waves read anyway.
#include "common.h"
#include "gemm_epi.h"
#include <string.h>

namespace dpot {

typedef float tn_f32x4 __attribute__((ext_vector_type(4)));

// one operand set of a launch: `nper` problems that differ by the batch strides (sA, sB) only
struct TnSet {
  const float* A;        // [T, lda]  (columns = output rows n1)
  const float* B;        // [T, ldb]  (columns = output columns n2)
  int cs_of;             // 0: no column sums, 1: of A (length N1), 2: of B (length N2)
  int pad_;
};
// problem table of a launch.  A GROUP is what one reduction finishes (a DPOT block's channel MLP: two sets of one problem;
// its AFNO layer pair: two sets of nb strided problems) - `batch` problems with a workspace of their own, ws_group floats
// apart.  The per-block entry points launch one group; dpot_mlp_wgrad_batch / dpot_afno_wgrad_batch up to TN_MAXSETS / 2.
// 32 sets (DPOT-M: 12 blocks = 24 sets) keep the kernel arguments at 0.9 KB
constexpr int TN_MAXSETS = 32;
struct TnArgs {
  int lda, ldb;
  long long sA, sB;      // batch strides inside a set (elements)
  int nper;              // problems per set
  int csL;               // length of a column-sum partial slot (0: N1 or N2 by cs_of)
  int N1, N2, T, batch;  // batch: problems per group
  int tiles1, tiles2, splits, slabs_per_split;
  float* ws;             // per group [split][batch][N1][N2] (+ [split][batch][L] column-sum partials behind)
  long long ws_group;    // floats between the workspaces of consecutive groups
  // the AFNO weight gradient dW = S^H dO as THREE real 128 x 128 products instead of the four blocks of the
  // 256 x 256 real product (bs == 128): with A = [Ar | Ai], B = [Br | Bi] (columns)
  //   P1 = Ar^T Br, P2 = Ai^T Bi, P3 = (Ar + Ai)^T (Bi - Br);   dWr = P1 + P2,  dWi = Ar^T Bi - Ai^T Br = P3 + P1 - P2
  // (the reduce does the recombination).  Tile 0 / 1 are the ordinary tiles (0,0) / (1,1), tile 2 streams all
  // 256 columns of both operands in 16-token slabs (the same 32 KiB per slab) and forms the two sums on the fragments;
  // partials [split][batch][3][128][128]
  int gauss;
  // three-product form on gemm_tn_kernel (128 channels per block): the sum-product tile is the slowest of the three (four fragment
  // reads and the VALU sums per step, twice the barriers), so it gets SHORTER token ranges: it is cut into `splits` ranges, the
  // tiles P1 / P2 into splits12 <= splits (the partial slots zs >= splits12 of those tiles are neither written nor read).
  // splits12 = splits elsewhere
  int splits12, slabs_per_split12;
  // batched launches: a ONE-dimensional grid of nwg workgroups.  The hardware deals consecutive workgroup ids to the 8 XCDs in
  // turn; id -> work item is the inverse of that deal, so an XCD owns a CONTIGUOUS range of work items, ordered (problem,
  // token range, tile): one operand set per XCD at DPOT-Tiny (its operands cross into that L2 once), workgroups that share a
  // token range next to each other
  int raster, nwg;
  // chained launches (gemm_tn_chain_kernel): a workgroup owns a NODE of tn_sum_nodes' tree - 1, 2 or 4 consecutive token ranges
  // (tn_chain_node) - and stores ONE partial for it; nodes / nodes12 = tn_chain_count(splits / splits12, chain) replace splits /
  // splits12 in the grid and in the workspace layout, the ranges themselves stay those of slabs_per_split / slabs_per_split12
  int nodes, nodes12;
  TnSet sets[TN_MAXSETS];
};

// The nodes of a chain c in {1, 2, 4} over `splits` token ranges: complete subtrees of the tree tn_sum_nodes evaluates - per
// full group of eight ranges 8 / c nodes of c ranges, the ranges behind the last full group in pairs, a last odd one alone
__host__ __device__ inline int tn_chain_count(int splits, int chain) {
  if (chain <= 1) return splits;
  return (splits >> 3) * (8 / chain) + ((splits & 7) + 1) / 2;
}
// workspace slots of a three-product launch: its tiles P1 / P2 have tn_chain_count(splits12) nodes, the sum product
// tn_chain_count(splits).  At chain 4 the count is NOT monotone in the ranges (quads exist only inside full groups of eight:
// 6 ranges are three pairs, 8 ranges two quads), so splits12 <= splits does not make the first the smaller: the layout -
// slot stride, the column sums behind the last slot - goes by the larger of the two
__host__ __device__ inline int tn_chain_slots(int splits12, int splits, int chain) {
  const int a = tn_chain_count(splits12, chain), b = tn_chain_count(splits, chain);
  return a > b ? a : b;
}
__host__ __device__ inline void tn_chain_node(int splits, int chain, int i, int* first, int* n) {
  if (chain <= 1) { *first = i; *n = 1; return; }
  const int full = (splits >> 3) * (8 / chain);        // nodes inside the full groups of eight
  if (i < full) { *first = i * chain; *n = chain; return; }
  const int f = 8 * (splits >> 3) + 2 * (i - full);
  *first = f;
  *n = splits - f < 2 ? splits - f : 2;
}

constexpr int TN_TOK = 32;                 // tokens per slab
constexpr int TN_W = 128;                  // tile width (both operands)
constexpr int TN_SLABF = 2 * TN_TOK * TN_W;  // floats per slab: A [16][128] | B [16][128]
constexpr int TN_RING = 4;
constexpr int TN_AHEAD = 3;                // slabs the loaders run ahead
constexpr int TN_NI = 16;                  // DMA instructions per slab and loader wave (1 KiB each)

template <int N>
__device__ __forceinline__ void tn_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void tn_glds16(const float* g, float* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// CHAIN = 1: a workgroup owns one token range.  CHAIN = 2 / 4 (the batched launches): it owns a node of up to CHAIN consecutive
// ranges (tn_chain_node).  The loader waves stream the node's slabs as one run; the compute waves accumulate every range from
// 0.0f exactly as its own workgroup would, and at a range boundary fold `acc` into a hold tile in the association of
// tn_sum_nodes' tree: (r0 + r1) for a pair, (r0 + r1) + (r2 + r3) for a quad - plain fp32 adds, the roundings the finalising
// launch performs on the partials of CHAIN = 1.  A quad would need three live tiles (acc, r2, r0 + r1: 146 + 128 VGPRs, over
// the 256 two waves on a SIMD can have): its first pair sum is parked in the node's own workspace slot - each lane reads back
// what it stored itself - and added when r2 + r3 is complete.  zs is the node index then, the workspace is [node][batch]...
template <int CHAIN>
__device__ __forceinline__ void tn_body(const TnArgs& p) {
  __shared__ __attribute__((aligned(16))) float lds[TN_RING * TN_SLABF];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int ntiles = p.tiles1 * p.tiles2;
  const int ns = CHAIN == 1 ? p.splits : p.nodes, ns12 = CHAIN == 1 ? p.splits12 : p.nodes12;   // slots per tile
  int tile, zbg, zs;                                    // zbg: problem index over the whole launch
  if (p.raster) {
    const int bid = blockIdx.x, xcd = bid & 7, slot = bid >> 3;
    const int q = p.nwg >> 3, r = p.nwg & 7;
    const int w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    if (p.gauss) {
      const int W = 2 * ns12 + ns;
      zbg = w / W;
      const int rr = w - zbg * W;
      tile = rr < ns12 ? 0 : rr < 2 * ns12 ? 1 : 2;
      zs = rr - (tile == 2 ? 2 * ns12 : tile * ns12);
    } else {
      const int per = ntiles * ns;
      zbg = w / per;
      const int rr = w - zbg * per;
      zs = rr / ntiles;
      tile = rr - zs * ntiles;
    }
  } else if (p.gauss) {
    // three-product form: a ONE-dimensional grid of exactly the workgroups that have work - per problem splits12 token ranges of
    // P1, splits12 of P2, `splits` of the sum-product tile (the hardware deals consecutive workgroups to the 8 XCDs in turn: a grid
    // with idle members leaves some XCD with more than its 32 workgroups and the launch with a second round)
    const int W = 2 * ns12 + ns;
    const int lin = blockIdx.x;
    zbg = lin / W;
    const int r = lin - zbg * W;
    tile = r < ns12 ? 0 : r < 2 * ns12 ? 1 : 2;
    zs = r - (tile == 2 ? 2 * ns12 : tile * ns12);
  } else {
    const int bid = blockIdx.x, xcd = bid & 7, slot = bid >> 3;
    const int q = ntiles >> 3, r = ntiles & 7;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    zbg = blockIdx.z / ns;
    zs = blockIdx.z - zbg * ns;
  }
  const int set = zbg / p.nper, zq = zbg - set * p.nper;
  const int grp = zbg / p.batch, zb = zbg - grp * p.batch;
  float* const wsg = p.ws + grp * p.ws_group;
  int t1 = tile / p.tiles2, t2 = tile - t1 * p.tiles2;
  const bool g3 = p.gauss && tile == 2;                 // the sum-product tile of the three-product form
  if (p.gauss) t1 = t2 = (tile == 1 ? 1 : 0);
  const int nslab_all = p.T / TN_TOK;
  const int sps = p.gauss && !g3 ? p.slabs_per_split12 : p.slabs_per_split;
  int r0 = zs, nr = 1;                                  // the node's first range and its ranges
  if constexpr (CHAIN > 1) tn_chain_node(p.gauss && !g3 ? p.splits12 : p.splits, CHAIN, zs, &r0, &nr);
  int slab0 = r0 * sps;
  int nslab = nslab_all - slab0;
  nslab = nslab < nr * sps ? nslab : nr * sps;
  if (nslab < 0) nslab = 0;
  if (g3) {                                             // 16-token slabs: twice as many over the same token range
    slab0 *= 2;
    nslab *= 2;
  }
  const int rslab = g3 ? 2 * sps : sps;                 // slabs of this workgroup per ORIGINAL token range

  auto bar = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  if (wave >= 4) {
    // ---------------------------------- loader waves ----------------------------------
    // wave L issues the tokens 16L .. 16L+15 of both operands (instruction j = tokens 16L + 2j, + 2j + 1 of one operand);
    // lane -> (token parity lane >> 5, 16 B piece lane & 31)
    const int L = wave - 4;
    const float* const A = p.sets[set].A;
    const float* const B = p.sets[set].B;
    // ordinary tile: an instruction moves two token rows of 128 columns; sum-product tile: ONE token row of all 256 columns
    // (wave L: tokens 8L .. 8L+7 of a 16-token slab) - 8 + 8 instructions per slab and wave either way
    const float* a0 = g3 ? A + zq * p.sA + (long long)(slab0 * 16 + 8 * L) * p.lda + lane * 4
                         : A + zq * p.sA + (long long)(slab0 * TN_TOK + 16 * L + (lane >> 5)) * p.lda +
                               t1 * TN_W + (lane & 31) * 4;
    const float* b0 = g3 ? B + zq * p.sB + (long long)(slab0 * 16 + 8 * L) * p.ldb + lane * 4
                         : B + zq * p.sB + (long long)(slab0 * TN_TOK + 16 * L + (lane >> 5)) * p.ldb +
                               t2 * TN_W + (lane & 31) * 4;
    const long long sa2 = (g3 ? 1ll : 2ll) * p.lda, sb2 = (g3 ? 1ll : 2ll) * p.ldb;
    const long long saS = (long long)(g3 ? 16 : TN_TOK) * p.lda, sbS = (long long)(g3 ? 16 : TN_TOK) * p.ldb;
    auto issue = [&](int t, int ring) __attribute__((always_inline)) {
      float* dst = lds + ring * TN_SLABF + L * 8 * 256;
      const float* a = a0 + t * saS;
      const float* b = b0 + t * sbS;
#pragma unroll
      for (int j = 0; j < 8; ++j) tn_glds16(a + j * sa2, dst + j * 256);
#pragma unroll
      for (int j = 0; j < 8; ++j) tn_glds16(b + j * sb2, dst + TN_TOK * TN_W + j * 256);
    };
    if (nslab > 0) issue(0, 0);
    if (nslab > 1) issue(1, 1);
    if (nslab > 2) issue(2, 2);
    if (nslab > 2) tn_wait_vm<2 * TN_NI>(); else if (nslab > 1) tn_wait_vm<TN_NI>(); else tn_wait_vm<0>();
    bar();                                              // P: slab 0 landed
    int ring = TN_AHEAD;                                // slot of slab g + 3
#pragma unroll 1
    for (int g = 0; g < nslab; ++g) {
      // slab g + 1 must have landed before B_g (the compute waves prefetch its first fragments before B_(g+1))
      if (g + 2 < nslab) tn_wait_vm<TN_NI>(); else tn_wait_vm<0>();
      bar();                                            // B_g: everyone is done with slab g - 1 -> its slot is free
      if (g + TN_AHEAD < nslab) issue(g + TN_AHEAD, ring);
      ring = ring == TN_RING - 1 ? 0 : ring + 1;
    }
    return;
  }

  // ---------------------------------- compute waves ----------------------------------
  const int wm = wave >> 1, wn = wave & 1;
  const int i16 = lane & 15, kq = lane >> 4;
  tn_f32x4 acc[4][4];
#pragma unroll
  for (int ea = 0; ea < 4; ++ea)
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) acc[ea][eb] = tn_f32x4{0.f, 0.f, 0.f, 0.f};
  tn_f32x4 cs = {0.f, 0.f, 0.f, 0.f};
  const int cs_sel = p.sets[set].cs_of;
  const bool cs_a = cs_sel == 1 && (p.gauss ? !g3 : t2 == 0) && wn == 0;
  const bool cs_b = cs_sel == 2 && (p.gauss ? !g3 : t1 == 0) && wm == 0;

  // this lane's fragment addresses inside a slab: A [tok = 4q + kq][wm*64 + 4*i16], B likewise with wn
  const int offA = kq * TN_W + wm * 64 + 4 * i16;
  const int offB = TN_TOK * TN_W + kq * TN_W + wn * 64 + 4 * i16;
  constexpr int NQ = TN_TOK / 4;                        // 4-token MFMA steps per slab

  // where this lane's part of the partial tile goes: element (n1 = 4*(4*kq + r) + ea, n2 = 4*i16 + eb) of the wave's 64 x 64
  // block (three-product form: [split][batch][3 tiles][128][128])
  float* const ws = p.gauss ? wsg + (((long long)zs * p.batch + zb) * 3 + tile) * (TN_W * TN_W)
                            : wsg + ((long long)zs * p.batch + zb) * p.N1 * p.N2;
  const int ldw = p.gauss ? TN_W : p.N2;
  const int n1b = (p.gauss ? 0 : t1 * TN_W) + wm * 64, n2b = (p.gauss ? 0 : t2 * TN_W) + wn * 64 + 4 * i16;
  // lanes with equal i16 hold the column sums over the tokens = kq (mod 4): fixed-order butterfly over kq
  auto cs_butterfly = [&]() __attribute__((always_inline)) {
    auto over_kq = [](float v) __attribute__((always_inline)) {
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      return v;
    };
    cs = tn_f32x4{over_kq(cs.x), over_kq(cs.y), over_kq(cs.z), over_kq(cs.w)};
  };
  // chained ranges: `fold` ends the original range k < 3 of the node when more slabs follow.  k = 0, 2: the range opens a pair,
  // its tile moves to `hold`; k = 1: the pair (r0 + r1) of a quad is complete and is parked in the node's slot
  tn_f32x4 hold[4][4];
#pragma unroll
  for (int ea = 0; ea < 4; ++ea)
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) hold[ea][eb] = tn_f32x4{0.f, 0.f, 0.f, 0.f};
  tn_f32x4 csh = {0.f, 0.f, 0.f, 0.f}, csp = csh;
  int k = 0, left = rslab;
  auto fold = [&]() __attribute__((always_inline)) {
    if (cs_a || cs_b) cs_butterfly();
    const bool quad_pair = CHAIN > 2 && k == 1;
    csp = quad_pair ? csh + cs : csp;                   // (selects, not conditional stores)
    csh = quad_pair ? csh : cs;
    if (quad_pair) {
#pragma unroll
      for (int ea = 0; ea < 4; ++ea)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n1 = n1b + 4 * (4 * kq + r) + ea;
          *reinterpret_cast<float4*>(ws + (long long)n1 * ldw + n2b) =
              make_float4(hold[ea][0][r] + acc[ea][0][r], hold[ea][1][r] + acc[ea][1][r], hold[ea][2][r] + acc[ea][2][r],
                          hold[ea][3][r] + acc[ea][3][r]);
        }
    } else {
#pragma unroll
      for (int ea = 0; ea < 4; ++ea)
#pragma unroll
        for (int eb = 0; eb < 4; ++eb) hold[ea][eb] = acc[ea][eb];
    }
#pragma unroll
    for (int ea = 0; ea < 4; ++ea)
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) acc[ea][eb] = tn_f32x4{0.f, 0.f, 0.f, 0.f};
    cs = tn_f32x4{0.f, 0.f, 0.f, 0.f};
    ++k;
    left = rslab;
  };

  bar();                                                // P
  if (g3) {
    // sum-product tile: slab image A [16 tok][256] | B [16 tok][256]; per 4-token step four fragment reads (Ar, Ai, Br, Bi),
    // a = Ar + Ai, b = Bi - Br on the VALU, 16 MFMAs
    const int oA = kq * 256 + wm * 64 + 4 * i16, oB = TN_TOK * TN_W + kq * 256 + wn * 64 + 4 * i16;
    tn_f32x4 far = {0.f, 0.f, 0.f, 0.f}, fai = far, fbr = far, fbi = far;
    if (nslab > 0) {
      far = *reinterpret_cast<const tn_f32x4*>(lds + oA);
      fai = *reinterpret_cast<const tn_f32x4*>(lds + oA + 128);
      fbr = *reinterpret_cast<const tn_f32x4*>(lds + oB);
      fbi = *reinterpret_cast<const tn_f32x4*>(lds + oB + 128);
    }
    int ring = 0;
#pragma unroll 1
    for (int g = 0; g < nslab; ++g) {
      bar();                                            // B_g
      const float* cur = lds + ring * TN_SLABF;
      const int rn = ring == TN_RING - 1 ? 0 : ring + 1;
      const float* nxt = g + 1 < nslab ? lds + rn * TN_SLABF : cur;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const tn_f32x4 a = far + fai, b = fbi - fbr;
        const float* src = q + 1 < 4 ? cur + (q + 1) * 4 * 256 : nxt;
        far = *reinterpret_cast<const tn_f32x4*>(src + oA);
        fai = *reinterpret_cast<const tn_f32x4*>(src + oA + 128);
        fbr = *reinterpret_cast<const tn_f32x4*>(src + oB);
        fbi = *reinterpret_cast<const tn_f32x4*>(src + oB + 128);
#pragma unroll
        for (int ea = 0; ea < 4; ++ea)
#pragma unroll
          for (int eb = 0; eb < 4; ++eb)
            acc[ea][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ea], b[eb], acc[ea][eb], 0, 0, 0);
      }
      ring = rn;
      if constexpr (CHAIN > 1) {
        if (--left == 0 && g + 1 < nslab) fold();
      }
    }
  } else {
  tn_f32x4 fa = {0.f, 0.f, 0.f, 0.f}, fb = fa;
  if (nslab > 0) {
    fa = *reinterpret_cast<const tn_f32x4*>(lds + offA);
    fb = *reinterpret_cast<const tn_f32x4*>(lds + offB);
  }
  int ring = 0;
#pragma unroll 1
  for (int g = 0; g < nslab; ++g) {
    bar();                                              // B_g
    const float* cur = lds + ring * TN_SLABF;
    const int rn = ring == TN_RING - 1 ? 0 : ring + 1;
    // the step after the last one of this slab is the first one of the next slab (landed before B_g); on the very last
    // slab the address is clamped to this slab (the value is never used)
    const float* nxt = g + 1 < nslab ? lds + rn * TN_SLABF : cur;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const tn_f32x4 a = fa, b = fb;
      const float* src = q + 1 < NQ ? cur + (q + 1) * 4 * TN_W : nxt;
      fa = *reinterpret_cast<const tn_f32x4*>(src + offA);
      fb = *reinterpret_cast<const tn_f32x4*>(src + offB);
      if (cs_a) cs += a;
      if (cs_b) cs += b;
#pragma unroll
      for (int ea = 0; ea < 4; ++ea)
#pragma unroll
        for (int eb = 0; eb < 4; ++eb)
          acc[ea][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ea], b[eb], acc[ea][eb], 0, 0, 0);
    }
    ring = rn;
    if constexpr (CHAIN > 1) {
      if (--left == 0 && g + 1 < nslab) fold();
    }
  }
  }

  // the node's last range is in acc, k ranges were folded before it: k odd - it closes a pair with `hold`; k >= 2 - the parked
  // first pair of the quad comes back, (r0 + r1) + (r2 + r3)
  if constexpr (CHAIN > 1) {
    if (k & 1) {
#pragma unroll
      for (int ea = 0; ea < 4; ++ea)
#pragma unroll
        for (int eb = 0; eb < 4; ++eb) acc[ea][eb] = hold[ea][eb] + acc[ea][eb];
    }
  }
#pragma unroll
  for (int ea = 0; ea < 4; ++ea)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n1 = n1b + 4 * (4 * kq + r) + ea;
      float4* const dst = reinterpret_cast<float4*>(ws + (long long)n1 * ldw + n2b);
      float4 o = make_float4(acc[ea][0][r], acc[ea][1][r], acc[ea][2][r], acc[ea][3][r]);
      if constexpr (CHAIN > 2) {
        if (k >= 2) {
          const float4 pk = *dst;
          o = make_float4(pk.x + o.x, pk.y + o.y, pk.z + o.z, pk.w + o.w);
        }
      }
      *dst = o;
    }
  if (cs_a || cs_b) {
    cs_butterfly();
    if constexpr (CHAIN > 1) {
      if (k & 1) cs = csh + cs;
      if (k >= 2) cs = csp + cs;
    }
    if (kq == 0) {
      const int L = p.csL ? p.csL : (cs_a ? p.N1 : p.N2);
      const int g0 = cs_a ? t1 * TN_W + wm * 64 : t2 * TN_W + wn * 64;
      const long long prod = p.gauss ? 3ll * TN_W * TN_W : (long long)p.N1 * p.N2;
      const int nslot = ns12 > ns ? ns12 : ns;          // = splits unchained (splits12 <= splits); tn_chain_slots chained
      float* wc = wsg + (long long)nslot * p.batch * prod + ((long long)zs * p.batch + zb) * L + g0 + 4 * i16;
      *reinterpret_cast<float4*>(wc) = make_float4(cs[0], cs[1], cs[2], cs[3]);
    }
  }
}

__global__ __launch_bounds__(384) void gemm_tn_kernel(const TnArgs p) { tn_body<1>(p); }
// the chained forms (dpot_mlp_wgrad_batch / dpot_afno_wgrad_batch at a chain of 2 or 4)
template <int CHAIN>
__global__ __launch_bounds__(384) void gemm_tn_chain_kernel(const TnArgs p) { tn_body<CHAIN>(p); }


// ---------------------------------------------------------------------------------------------------------------------
// 192 x 192 variant (round 3): the AFNO weight gradients of DPOT-Large (bs = 96 -> N = 2*bs = 192, not a multiple of the
// 128-wide tile above; they ran on the generic kernel of gemm.hip at 68 TFLOP/s, 5 % of the DPOT-L step).  One workgroup
// owns the WHOLE 192 x 192 output of a (channel block, layer) problem x a token range: 3 x 3 compute waves of 64 x 64
// (same row-interleaved fragments, same 16-byte stores) + 2 loader waves; slabs of 32 tokens = [32][192] per operand
// (48 KiB), ring of three; a DMA piece is 1 KiB of the slab's linear image - 192 floats per token is a multiple of the
// 16-byte lane chunk, so a piece never splits a chunk across rows.  Nine waves on four SIMDs leave one SIMD with three:
// the matrix pipes can reach 75 % at best - against 43 % on the generic kernel.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int TW = 192;                      // tile width (both operands)
constexpr int TW_SLABF = 2 * TN_TOK * TW;    // floats per slab: A [32][192] | B [32][192]
constexpr int TW_RING = 3;
constexpr int TW_NI = 24;                    // DMA instructions per slab and loader wave (12 of A + 12 of B)

__global__ __launch_bounds__(704) void gemm_tn192_kernel(const TnArgs p) {
  __shared__ __attribute__((aligned(16))) float lds[TW_RING * TW_SLABF];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int zb = blockIdx.z / p.splits, zs = blockIdx.z - zb * p.splits;
  const int nslab_all = p.T / TN_TOK;
  const int slab0 = zs * p.slabs_per_split;
  int nslab = nslab_all - slab0;
  nslab = nslab < p.slabs_per_split ? nslab : p.slabs_per_split;
  if (nslab < 0) nslab = 0;

  auto bar = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  if (wave >= 9) {
    // ---------------------------------- loader waves ----------------------------------
    const int L = wave - 9;
    const int set = zb / p.nper, zq = zb - set * p.nper;
    const float* abase = p.sets[set].A + zq * p.sA + (long long)slab0 * TN_TOK * p.lda;
    const float* bbase = p.sets[set].B + zq * p.sB + (long long)slab0 * TN_TOK * p.ldb;
    auto issue = [&](int t, int ring) __attribute__((always_inline)) {
      float* dst = lds + ring * TW_SLABF;
      const float* a = abase + (long long)t * TN_TOK * p.lda;
      const float* b = bbase + (long long)t * TN_TOK * p.ldb;
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        const int f = 256 * (L + 2 * j) + 4 * lane;     // float index inside the operand's [32][192] image
        const int tok = f / TW, col = f - tok * TW;
        tn_glds16(a + (long long)tok * p.lda + col, dst + 256 * (L + 2 * j));
      }
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        const int f = 256 * (L + 2 * j) + 4 * lane;
        const int tok = f / TW, col = f - tok * TW;
        tn_glds16(b + (long long)tok * p.ldb + col, dst + TN_TOK * TW + 256 * (L + 2 * j));
      }
    };
    if (nslab > 0) issue(0, 0);
    if (nslab > 1) issue(1, 1);
    if (nslab > 1) tn_wait_vm<TW_NI>(); else tn_wait_vm<0>();
    bar();                                              // P: slab 0 landed
    int ring = 2;                                       // slot of slab g + 2
#pragma unroll 1
    for (int g = 0; g < nslab; ++g) {
      tn_wait_vm<0>();                                  // slab g + 1 landed (the compute waves prefetch its first fragments)
      bar();                                            // B_g: everyone is done with slab g - 1 -> its slot is free
      if (g + 2 < nslab) issue(g + 2, ring);
      ring = ring == TW_RING - 1 ? 0 : ring + 1;
    }
    return;
  }

  // ---------------------------------- compute waves ----------------------------------
  const int wm = wave / 3, wn = wave - 3 * wm;
  const int i16 = lane & 15, kq = lane >> 4;
  tn_f32x4 acc[4][4];
#pragma unroll
  for (int ea = 0; ea < 4; ++ea)
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) acc[ea][eb] = tn_f32x4{0.f, 0.f, 0.f, 0.f};
  tn_f32x4 cs = {0.f, 0.f, 0.f, 0.f};
  const int cs_sel = p.sets[zb / p.nper].cs_of;
  const bool cs_a = cs_sel == 1 && wn == 0;
  const bool cs_b = cs_sel == 2 && wm == 0;
  const int offA = kq * TW + wm * 64 + 4 * i16;
  const int offB = TN_TOK * TW + kq * TW + wn * 64 + 4 * i16;
  constexpr int NQ = TN_TOK / 4;

  bar();                                                // P
  tn_f32x4 fa = {0.f, 0.f, 0.f, 0.f}, fb = fa;
  if (nslab > 0) {
    fa = *reinterpret_cast<const tn_f32x4*>(lds + offA);
    fb = *reinterpret_cast<const tn_f32x4*>(lds + offB);
  }
  int ring = 0;
#pragma unroll 1
  for (int g = 0; g < nslab; ++g) {
    bar();                                              // B_g
    const float* cur = lds + ring * TW_SLABF;
    const int rn = ring == TW_RING - 1 ? 0 : ring + 1;
    const float* nxt = g + 1 < nslab ? lds + rn * TW_SLABF : cur;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const tn_f32x4 a = fa, b = fb;
      const float* src = q + 1 < NQ ? cur + (q + 1) * 4 * TW : nxt;
      fa = *reinterpret_cast<const tn_f32x4*>(src + offA);
      fb = *reinterpret_cast<const tn_f32x4*>(src + offB);
      if (cs_a) cs += a;
      if (cs_b) cs += b;
#pragma unroll
      for (int ea = 0; ea < 4; ++ea)
#pragma unroll
        for (int eb = 0; eb < 4; ++eb)
          acc[ea][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ea], b[eb], acc[ea][eb], 0, 0, 0);
    }
    ring = rn;
  }

  float* ws = p.ws + ((long long)zs * p.batch + zb) * p.N1 * p.N2;
  const int n1b = wm * 64, n2b = wn * 64 + 4 * i16;
#pragma unroll
  for (int ea = 0; ea < 4; ++ea)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n1 = n1b + 4 * (4 * kq + r) + ea;
      *reinterpret_cast<float4*>(ws + (long long)n1 * p.N2 + n2b) =
          make_float4(acc[ea][0][r], acc[ea][1][r], acc[ea][2][r], acc[ea][3][r]);
    }
  if (cs_a || cs_b) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = cs[e];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      cs[e] = v;
    }
    if (kq == 0) {
      const int Lc = p.csL ? p.csL : (cs_a ? p.N1 : p.N2);
      const int g0 = cs_a ? wm * 64 : wn * 64;
      float* wc = p.ws + (long long)p.splits * p.batch * p.N1 * p.N2 + ((long long)zs * p.batch + zb) * Lc + g0 + 4 * i16;
      *reinterpret_cast<float4*>(wc) = make_float4(cs[0], cs[1], cs[2], cs[3]);
    }
  }
}


// ---------------------------------------------------------------------------------------------------------------------
// 96-channel three-product variant (round 5): the AFNO weight gradients of DPOT-Large in the Gauss form of TnArgs::gauss
//     P1 = Ar^T Br,  P2 = Ai^T Bi,  P3 = (Ar + Ai)^T (Bi - Br)          (three 96 x 96 products instead of 192 x 192)
// on TWELVE compute waves - product p on waves 4p .. 4p+3 in a 2 x 2 grid of 48 x 48 (3 x 3 accumulators) - + 2 loader
// waves: 14 waves put 3 compute waves on every SIMD (the 192 x 192 kernel above has 3 / 2 / 2 / 2: its matrix pipes can
// reach 75 % at best), and the launch executes 3/4 of the FLOPs.  Same slabs ([32 tok][192] per operand, ring of three),
// same loaders, same split-K.  Fragments: tile e of a wave = 16 consecutive channels, one ds_read_b32 per tile and 4-token
// step (consecutive lanes, consecutive floats); the P3 waves read both halves of both operands and form the sums on the
// VALU.  Partials [split][problem][3][96][96] (+ column sums of dO from the P1 / P2 waves) - afno_wgrad2_reduce_body's
// three-product branch recombines.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int TG_BS = 96;
constexpr int TGS = 208;                     // LDS row stride (floats): 192 + 16 - the four token groups of a ds_read_b32 (rows
                                             // kq, kq+1, ..) start 16 banks apart; with 192 (= 0 mod 64 banks) they collide 4-way
constexpr int TG_SLABF = 2 * TN_TOK * TGS;   // floats per slab: A [32][208] | B [32][208]  (3 slabs = 156 KiB)
constexpr int TG_NI = 32;                    // DMA instructions per slab and loader wave: one token row each (48 lanes x 16 B)

__global__ __launch_bounds__(896) void gemm_tn96g_kernel(const TnArgs p) {
  __shared__ __attribute__((aligned(16))) float lds[TW_RING * TG_SLABF];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int zb = blockIdx.z / p.splits, zs = blockIdx.z - zb * p.splits;
  const int nslab_all = p.T / TN_TOK;
  const int slab0 = zs * p.slabs_per_split;
  int nslab = nslab_all - slab0;
  nslab = nslab < p.slabs_per_split ? nslab : p.slabs_per_split;
  if (nslab < 0) nslab = 0;

  auto bar = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  if (wave >= 12) {
    // ---------------------------------- loader waves (as in gemm_tn192_kernel) ----------------------------------
    const int L = wave - 12;
    const int set = zb / p.nper, zq = zb - set * p.nper;
    const float* abase = p.sets[set].A + zq * p.sA + (long long)slab0 * TN_TOK * p.lda;
    const float* bbase = p.sets[set].B + zq * p.sB + (long long)slab0 * TN_TOK * p.ldb;
    auto issue = [&](int t, int ring) __attribute__((always_inline)) {
      float* dst = lds + ring * TG_SLABF;
      const float* a = abase + (long long)t * TN_TOK * p.lda + 4 * lane;
      const float* b = bbase + (long long)t * TN_TOK * p.ldb + 4 * lane;
      if (lane < 48) {                                  // a token row = 192 floats = 48 lanes x 16 B, padded to TGS in LDS
#pragma unroll
        for (int j = 0; j < 16; ++j) tn_glds16(a + (long long)(L + 2 * j) * p.lda, dst + (L + 2 * j) * TGS);
#pragma unroll
        for (int j = 0; j < 16; ++j) tn_glds16(b + (long long)(L + 2 * j) * p.ldb, dst + (TN_TOK + L + 2 * j) * TGS);
      }
    };
    if (nslab > 0) issue(0, 0);
    if (nslab > 1) issue(1, 1);
    if (nslab > 1) tn_wait_vm<TG_NI>(); else tn_wait_vm<0>();
    bar();                                              // P
    int ring = 2;
#pragma unroll 1
    for (int g = 0; g < nslab; ++g) {
      tn_wait_vm<0>();
      bar();                                            // B_g
      if (g + 2 < nslab) issue(g + 2, ring);
      ring = ring == TW_RING - 1 ? 0 : ring + 1;
    }
    return;
  }

  // ---------------------------------- compute waves ----------------------------------
  const int prod = wave >> 2;                           // 0: Ar^T Br, 1: Ai^T Bi, 2: (Ar + Ai)^T (Bi - Br)
  const int wm = (wave >> 1) & 1, wn = wave & 1;
  const int i16 = lane & 15, kq = lane >> 4;
  tn_f32x4 acc[3][3];
#pragma unroll
  for (int ea = 0; ea < 3; ++ea)
#pragma unroll
    for (int eb = 0; eb < 3; ++eb) acc[ea][eb] = tn_f32x4{0.f, 0.f, 0.f, 0.f};
  float cs[3] = {0.f, 0.f, 0.f};
  const int cs_sel = p.sets[zb / p.nper].cs_of;
  const bool cs_a = cs_sel == 1 && prod < 2 && wn == 0;
  const bool cs_b = cs_sel == 2 && prod < 2 && wm == 0;
  const int half = prod == 1 ? TG_BS : 0;               // P2 reads the imaginary halves; P3 reads both (half = 0, + TG_BS)
  const int offA = kq * TGS + half + wm * 48 + i16;
  const int offB = TN_TOK * TGS + kq * TGS + half + wn * 48 + i16;
  constexpr int NQ = TN_TOK / 4;

  bar();                                                // P
  if (prod < 2) {
    float fa[3] = {0.f, 0.f, 0.f}, fb[3] = {0.f, 0.f, 0.f};
    if (nslab > 0) {
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        fa[e] = lds[offA + 16 * e];
        fb[e] = lds[offB + 16 * e];
      }
    }
    int ring = 0;
#pragma unroll 1
    for (int g = 0; g < nslab; ++g) {
      bar();                                            // B_g
      const float* cur = lds + ring * TG_SLABF;
      const int rn = ring == TW_RING - 1 ? 0 : ring + 1;
      const float* nxt = g + 1 < nslab ? lds + rn * TG_SLABF : cur;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        float a[3], b[3];
        const float* src = q + 1 < NQ ? cur + (q + 1) * 4 * TGS : nxt;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          a[e] = fa[e];
          b[e] = fb[e];
          fa[e] = src[offA + 16 * e];
          fb[e] = src[offB + 16 * e];
        }
        if (cs_a) { cs[0] += a[0]; cs[1] += a[1]; cs[2] += a[2]; }
        if (cs_b) { cs[0] += b[0]; cs[1] += b[1]; cs[2] += b[2]; }
#pragma unroll
        for (int ea = 0; ea < 3; ++ea)
#pragma unroll
          for (int eb = 0; eb < 3; ++eb)
            acc[ea][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ea], b[eb], acc[ea][eb], 0, 0, 0);
      }
      ring = rn;
    }
  } else {
    float far[3] = {0.f, 0.f, 0.f}, fai[3] = {0.f, 0.f, 0.f}, fbr[3] = {0.f, 0.f, 0.f}, fbi[3] = {0.f, 0.f, 0.f};
    if (nslab > 0) {
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        far[e] = lds[offA + 16 * e];
        fai[e] = lds[offA + TG_BS + 16 * e];
        fbr[e] = lds[offB + 16 * e];
        fbi[e] = lds[offB + TG_BS + 16 * e];
      }
    }
    int ring = 0;
#pragma unroll 1
    for (int g = 0; g < nslab; ++g) {
      bar();                                            // B_g
      const float* cur = lds + ring * TG_SLABF;
      const int rn = ring == TW_RING - 1 ? 0 : ring + 1;
      const float* nxt = g + 1 < nslab ? lds + rn * TG_SLABF : cur;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        float a[3], b[3];
        const float* src = q + 1 < NQ ? cur + (q + 1) * 4 * TGS : nxt;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          a[e] = far[e] + fai[e];
          b[e] = fbi[e] - fbr[e];
          far[e] = src[offA + 16 * e];
          fai[e] = src[offA + TG_BS + 16 * e];
          fbr[e] = src[offB + 16 * e];
          fbi[e] = src[offB + TG_BS + 16 * e];
        }
#pragma unroll
        for (int ea = 0; ea < 3; ++ea)
#pragma unroll
          for (int eb = 0; eb < 3; ++eb)
            acc[ea][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ea], b[eb], acc[ea][eb], 0, 0, 0);
      }
      ring = rn;
    }
  }

  // partial tile: element (row = wm*48 + 16*ea + 4*kq + r, col = wn*48 + 16*eb + i16) of product `prod`
  float* ws = p.ws + (((long long)zs * p.batch + zb) * 3 + prod) * (TG_BS * TG_BS);
#pragma unroll
  for (int ea = 0; ea < 3; ++ea)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* row = ws + (long long)(wm * 48 + 16 * ea + 4 * kq + r) * TG_BS + wn * 48 + i16;
#pragma unroll
      for (int eb = 0; eb < 3; ++eb) row[16 * eb] = acc[ea][eb][r];
    }
  if (cs_a || cs_b) {
    // lanes with equal i16 hold the sums over the tokens = kq (mod 4): fixed-order butterfly over kq
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      float v = cs[e];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      cs[e] = v;
    }
    if (kq == 0) {
      const int Lc = p.csL ? p.csL : (cs_a ? p.N1 : p.N2);
      const int g0 = half + (cs_a ? wm : wn) * 48 + i16;
      float* wc = p.ws + (long long)p.splits * p.batch * (3ll * TG_BS * TG_BS) + ((long long)zs * p.batch + zb) * Lc + g0;
#pragma unroll
      for (int e = 0; e < 3; ++e) wc[16 * e] = cs[e];
    }
  }
}

}  // namespace dpot

using namespace dpot;

// split count the TN kernel wants for a shape (0: the shape is not eligible)
extern "C" int dpot_gemm_tn_splitk(int M, int N, int K, int batch) {
  static const int enabled = tune("panel", 1);
  // batched descriptors (the AFNO weight gradients: 4 x [256 x 256], 4608 tokens) stay on the generic kernel: measured
  // 37.4 us here against 36.2 us there
  if (!enabled || M <= 0 || N <= 0 || K <= 0 || batch != 1 || M % TN_W || N % TN_W || K % TN_TOK) return 0;
  const long long tiles = (long long)(M / TN_W) * (N / TN_W) * batch;
  const int nslab = K / TN_TOK;
  long long s = (256 + tiles / 2) / tiles;            // one workgroup per CU
  const long long smax = nslab / 4;                   // >= 4 slabs (128 tokens) per split
  if (s > smax) s = smax;
  if (s < 2) s = 2;                                   // the kernel always goes through the workspace + reduce
  if (s > nslab) return 0;
  const long long sps = (nslab + s - 1) / s;          // slabs per split; drop the splits that would come out empty
  s = (nslab + sps - 1) / sps;                        // (e.g. 256 slabs / 21 splits -> 13 per split -> 20 splits)
  if (s < 2) return 0;
  return (int)s;
}

// called by dpot_gemm_f32 (gemm.hip) for transA && !transB, native fp32, split-K descriptors; returns -1 when the
// descriptor is not eligible (the generic kernel runs instead), else the launch status.  The partial sums land in
// d->workspace in the layout the generic kernel uses, so the caller's reduce launch is unchanged.
int dpot_gemm_tn_try(const dpot_gemm_desc* d, hipStream_t s) {
  static const int enabled = tune("panel", 1);
  if (!enabled || !d->transA || d->transB || d->splitk <= 1 || !d->workspace || d->batch != 1) return -1;
  if (d->M % TN_W || d->N % TN_W || d->K % TN_TOK || d->lda % 4 || d->ldb % 4 || d->strideA % 4 || d->strideB % 4 ||
      !aligned16(d->A) || !aligned16(d->B) || !aligned16(d->workspace) || d->N % 4)
    return -1;
  const int nslab = d->K / TN_TOK;
  if (d->splitk > nslab || (long long)d->batch * d->splitk > 65535) return -1;
  TnArgs p{};
  p.sets[0] = TnSet{d->A, d->B, d->colsum_of, 0};
  p.nper = d->batch; p.lda = d->lda; p.ldb = d->ldb; p.sA = d->strideA; p.sB = d->strideB; p.csL = 0;
  p.N1 = d->M; p.N2 = d->N; p.T = d->K; p.batch = d->batch;
  p.tiles1 = d->M / TN_W; p.tiles2 = d->N / TN_W;
  p.splits = d->splitk;
  p.slabs_per_split = (nslab + d->splitk - 1) / d->splitk;
  if ((long long)p.slabs_per_split * (d->splitk - 1) >= nslab) return -1;      // an empty split would leave its partial unwritten
  p.ws = d->workspace;
  p.gauss = 0; p.splits12 = p.splits; p.slabs_per_split12 = p.slabs_per_split;
  hipLaunchKernelGGL(gemm_tn_kernel, dim3((unsigned)(p.tiles1 * p.tiles2), 1, (unsigned)(d->batch * d->splitk)), dim3(384),
                     0, s, p);
  return check_launch("gemm_tn_kernel");
}


// ---------------------------------------------------------------------------------------------------------------------
// Both weight gradients of an AFNO block's complex MLP in ONE launch: per channel block k
//     dWbig1[k] = S[:, k]^T dO1pre[:, k],    dWbig2[k] = O1[:, k]^T dO2[:, k]        (N x N, N = 2*bs, K = Mm tokens)
// = 2*nb independent problems of the kernel above.  One launch halves the split factor each problem needs to fill the
// chip (18 instead of 9 slabs per workgroup, half the partial-sum traffic) against two launches of the generic kernel:
// 2 x 36.5 us -> one launch + one reduce.  The reduce un-packs  dWr = D[0:bs,0:bs] + D[bs:,bs:],
// dWi = D[0:bs,bs:] - D[bs:,0:bs]  and the bias gradients (column sums of dO) for both layers, fixed order.
// ---------------------------------------------------------------------------------------------------------------------
namespace dpot {
// sum_s w[s * stride], s < splits: always the same association ((0+1)+(2+3))+((4+5)+(6+7)) per group of eight, groups in
// order - deterministic - with eight independent loads in flight (a dependent chain of `splits` L2 round trips made the
// reduce kernels latency bound: 16 MB in 12 us)
//
// chain = 2 / 4: the workspace holds one partial per NODE (tn_chain_node: the kernel has already formed the pairs / quads of
// this very tree, with the same fp32 adds), slot j = node j; what is left of the tree is evaluated here - every rounding is the
// one chain = 1 performs
__device__ __forceinline__ float tn_sum_nodes(const float* __restrict__ w, long long stride, int splits, int chain) {
  float v = 0.f;
  int s = 0;
  if (chain > 1) {
    int j = 0;
    if (chain == 2) {
      for (; s + 8 <= splits; s += 8, j += 4) {
        const float a0 = w[(long long)(j + 0) * stride], a1 = w[(long long)(j + 1) * stride];
        const float a2 = w[(long long)(j + 2) * stride], a3 = w[(long long)(j + 3) * stride];
        v += (a0 + a1) + (a2 + a3);
      }
    } else {
      for (; s + 8 <= splits; s += 8, j += 2) {
        const float a0 = w[(long long)(j + 0) * stride], a1 = w[(long long)(j + 1) * stride];
        v += a0 + a1;
      }
    }
    // the tail's pairs and a last odd range: at most four slots, loaded before the first add (independent loads in flight)
    const int nt = (splits - s + 1) >> 1;
    const float t0 = nt > 0 ? w[(long long)(j + 0) * stride] : 0.f, t1 = nt > 1 ? w[(long long)(j + 1) * stride] : 0.f;
    const float t2 = nt > 2 ? w[(long long)(j + 2) * stride] : 0.f, t3 = nt > 3 ? w[(long long)(j + 3) * stride] : 0.f;
    if (nt > 0) v += t0;
    if (nt > 1) v += t1;
    if (nt > 2) v += t2;
    if (nt > 3) v += t3;
    return v;
  }
  for (; s + 8 <= splits; s += 8) {
    const float a0 = w[(long long)(s + 0) * stride], a1 = w[(long long)(s + 1) * stride];
    const float a2 = w[(long long)(s + 2) * stride], a3 = w[(long long)(s + 3) * stride];
    const float a4 = w[(long long)(s + 4) * stride], a5 = w[(long long)(s + 5) * stride];
    const float a6 = w[(long long)(s + 6) * stride], a7 = w[(long long)(s + 7) * stride];
    v += ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
  }
  for (; s + 2 <= splits; s += 2) {
    const float a0 = w[(long long)s * stride], a1 = w[(long long)(s + 1) * stride];
    v += a0 + a1;
  }
  if (s < splits) v += w[(long long)s * stride];
  return v;
}

// (bid, nblk: this workgroup's index / the number of workgroups working on the reduction - the stand-alone kernel passes
// blockIdx.x / gridDim.x, block_finalize_kernel a slice of its grid)
__device__ __forceinline__ void afno_wgrad2_reduce_body(int bid, int nblk, const float* __restrict__ ws, int splits, int nb,
                                                        int bs, float* __restrict__ dw1, float* __restrict__ db1,
                                                        float* __restrict__ dw2, float* __restrict__ db2, int gauss,
                                                        int chain) {
  const int n2 = 2 * bs;
  const long long MN = gauss ? 3ll * bs * bs : (long long)n2 * n2, total = MN * 2 * nb;
  const long long nw = (long long)nb * bs * bs;
  for (long long idx = bid * 256ll + threadIdx.x; idx < 2 * nw; idx += (long long)nblk * 256) {
    const int layer = idx >= nw;
    const long long q = idx - layer * nw;
    const int o = (int)(q % bs), i = (int)((q / bs) % bs), k = (int)(q / ((long long)bs * bs));
    const float* base = ws + (long long)(layer * nb + k) * MN;
    float* dw = layer ? dw2 : dw1;
    if (gauss) {     // P1 = Ar^T Br, P2 = Ai^T Bi, P3 = (Ar + Ai)^T (Bi - Br): dWr = P1 + P2, dWi = P3 + P1 - P2
      // (gauss = the number of token ranges of P1 / P2 and of the column sums, TnArgs::splits12 - <= splits)
      const long long e = (long long)i * bs + o, t = (long long)bs * bs;
      const float p1 = tn_sum_nodes(base + e, total, gauss, chain);
      const float p2 = tn_sum_nodes(base + t + e, total, gauss, chain);
      const float p3 = tn_sum_nodes(base + 2 * t + e, total, splits, chain);
      dw[q] = p1 + p2;
      dw[nw + q] = p3 + p1 - p2;
      continue;
    }
    const float rr = tn_sum_nodes(base + (long long)i * n2 + o, total, splits, chain);
    const float ii = tn_sum_nodes(base + (long long)(bs + i) * n2 + bs + o, total, splits, chain);
    const float ri = tn_sum_nodes(base + (long long)i * n2 + bs + o, total, splits, chain);
    const float ir = tn_sum_nodes(base + (long long)(bs + i) * n2 + o, total, splits, chain);
    dw[q] = rr + ii;
    dw[nw + q] = ri - ir;
  }
  const float* wc = ws + (long long)tn_chain_slots(gauss ? gauss : splits, splits, chain) * total;
  const long long nc = (long long)2 * nb * n2;
  for (long long idx = bid * 256ll + threadIdx.x; idx < nc; idx += (long long)nblk * 256) {
    const float v = tn_sum_nodes(wc + idx, nc, gauss ? gauss : splits, chain);
    const int layer = idx >= (long long)nb * n2;
    const long long q = idx - (long long)layer * nb * n2;
    const int c = (int)(q % bs), part = (int)((q / bs) & 1), k = (int)(q / n2);
    (layer ? db2 : db1)[((long long)part * nb + k) * bs + c] = v;
  }
}
__global__ __launch_bounds__(256) void afno_wgrad2_reduce_kernel(const float* __restrict__ ws, int splits, int nb, int bs,
                                                                 float* __restrict__ dw1, float* __restrict__ db1,
                                                                 float* __restrict__ dw2, float* __restrict__ db2, int gauss) {
  afno_wgrad2_reduce_body(blockIdx.x, gridDim.x, ws, splits, nb, bs, dw1, db1, dw2, db2, gauss, 1);
}

// three-product form of the AFNO weight gradient (TnArgs::gauss): 128 channels per block, and 96 (DPOT-Large): gemm_tn96g_kernel;
// DPOT_TUNE wgrad_gauss=0: four products (128: four tiles of gemm_tn_kernel; 96: the 192 x 192 kernel)
static int tn_gauss(int bs) {
  static const int enabled = tune("wgrad_gauss", 1);
  return enabled && (bs == TN_W || bs == TG_BS) ? 1 : 0;
}
// token ranges of the tiles P1 / P2 when the sum-product tile is cut into `splitk` (TnArgs::splits12): 5/6 of them at 128 channels
// per block (profiles/r05_tn_skew.txt); the 96-channel kernel computes the three products in one workgroup
static int tn_gauss_s12(int bs, int splitk) {
  constexpr int num = 5, den = 6;
  if (bs != TN_W) return splitk;
  const int s = splitk * num / den;
  return s < 1 ? 1 : s;
}
}  // namespace dpot

extern "C" int dpot_afno_wgrad2_splitk(int Mm, int nb, int bs) {
  static const int enabled = tune("panel", 1);
  const int N = 2 * bs;
  if (!enabled || nb <= 0 || bs <= 0 || (N % TN_W && N != TW) || Mm <= 0 || Mm % TN_TOK) return 0;
  const long long tiles = N == TW ? (long long)2 * nb : tn_gauss(bs) ? 6ll * nb : (long long)2 * nb * (N / TN_W) * (N / TN_W);
  const int nslab = Mm / TN_TOK;
  // three-product form: 3 tiles per problem do not divide 256 - round DOWN (one round of workgroups: 24 tiles x 10 splits = 240
  // at DPOT-Tiny; rounded to 11 the launch needs a second round: 75 against 59 us, profiles/r05_tn_bench_gauss.txt)
  long long s = tn_gauss(bs) && N != TW ? 256 / tiles : (256 + tiles / 2) / tiles;
  const long long smax = nslab / 4;
  if (tn_gauss(bs) && N != TW) {
    // skewed ranges: the largest split count whose 2 * s12 + s workgroups per problem still fit one round of 256
    // (DPOT-Tiny: 8 problems x (10 + 10 + 12), DPOT-S / -M: 16 x (5 + 5 + 6))
    long long best = 1;
    for (long long c = 1; c <= smax && c <= 64; ++c)
      if (2ll * nb * (2 * tn_gauss_s12(bs, (int)c) + c) <= 256) best = c;
    s = best;
  }
  if (s > smax) s = smax;
  if (s < 1) s = 1;
  // no empty split
  while (s > 1 && ((nslab + s - 1) / s) * (s - 1) >= nslab) --s;
  return (int)s;
}

// token ranges of the products P1 / P2 of the three-product form when the sum product is cut into `splitk` (= splitk for the
// other forms): what dpot_afno_wgrad2 launches and dpot_block_finalize reduces
extern "C" int dpot_afno_wgrad2_splits12(int bs, int splitk) {
  return tn_gauss(bs) ? tn_gauss_s12(bs, splitk) : splitk;
}

extern "C" int64_t dpot_afno_wgrad2_ws_elems(int nb, int bs, int splitk) {
  const int64_t N = 2 * bs;
  return (int64_t)splitk * 2 * nb * ((tn_gauss(bs) ? 3 * (int64_t)bs * bs : N * N) + N);
}

extern "C" int dpot_afno_wgrad2(const float* S, const float* dO1pre, const float* O1, const float* dO2, int ld, int Mm,
                                int nb, int bs, float* dw1, float* db1, float* dw2, float* db2, float* workspace,
                                int splitk, dpot_stream_t stream) {
  DPOT_REQUIRE(S && dO1pre && O1 && dO2 && workspace, "afno_wgrad2: null pointer");
  DPOT_REQUIRE((dw1 && db1 && dw2 && db2) || (!dw1 && !db1 && !dw2 && !db2), "afno_wgrad2: outputs must be all given or all NULL");
  const int N = 2 * bs;
  DPOT_REQUIRE(nb > 0 && bs > 0 && (N % TN_W == 0 || N == TW) && Mm > 0 && Mm % TN_TOK == 0 && ld >= nb * N && ld % 4 == 0,
               "afno_wgrad2: needs 2*bs %% 128 == 0 or 2*bs == 192, Mm %% 32 == 0");
  DPOT_REQUIRE(aligned16(S) && aligned16(dO1pre) && aligned16(O1) && aligned16(dO2) && aligned16(workspace),
               "afno_wgrad2: operands must be 16-byte aligned");
  const int nslab = Mm / TN_TOK;
  DPOT_REQUIRE(splitk >= 1 && splitk <= nslab && (long long)2 * nb * splitk <= 65535, "afno_wgrad2: bad split factor");
  TnArgs p{};
  p.sets[0] = TnSet{S, dO1pre, 2, 0};
  p.sets[1] = TnSet{O1, dO2, 2, 0};
  p.nper = nb; p.csL = 0;
  p.lda = ld; p.ldb = ld; p.sA = N; p.sB = N;
  p.N1 = N; p.N2 = N; p.T = Mm; p.batch = 2 * nb;
  p.tiles1 = N / TN_W; p.tiles2 = N / TN_W;
  p.splits = splitk;
  p.slabs_per_split = (nslab + splitk - 1) / splitk;
  DPOT_REQUIRE((long long)p.slabs_per_split * (splitk - 1) < nslab, "afno_wgrad2: split factor leaves an empty split");
  p.ws = workspace;
  p.gauss = tn_gauss(bs);
  p.splits12 = p.gauss ? tn_gauss_s12(bs, splitk) : splitk;
  p.slabs_per_split12 = (nslab + p.splits12 - 1) / p.splits12;
  hipStream_t s = as_stream(stream);
  if (N == TW) {
    p.tiles1 = p.tiles2 = 1;
    if (p.gauss)
      hipLaunchKernelGGL(gemm_tn96g_kernel, dim3(1, 1, (unsigned)(2 * nb * splitk)), dim3(896), 0, s, p);
    else
      hipLaunchKernelGGL(gemm_tn192_kernel, dim3(1, 1, (unsigned)(2 * nb * splitk)), dim3(704), 0, s, p);
  } else {
    if (p.gauss)
      hipLaunchKernelGGL(gemm_tn_kernel, dim3((unsigned)(2 * nb * (2 * p.splits12 + splitk))), dim3(384), 0, s, p);
    else
      hipLaunchKernelGGL(gemm_tn_kernel, dim3((unsigned)(p.tiles1 * p.tiles2), 1, (unsigned)(2 * nb * splitk)), dim3(384), 0, s, p);
  }
  int rc = check_launch("gemm_tn_kernel");
  if (rc || !dw1) return rc;            // dw1 == NULL: partials only, dpot_block_finalize reduces them
  long long blocks = (2ll * nb * bs * bs + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(afno_wgrad2_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)workspace, splitk, nb,
                     bs, dw1, db1, dw2, db2, p.gauss ? p.splits12 : 0);
  return check_launch("afno_wgrad2_reduce_kernel");
}


// ---------------------------------------------------------------------------------------------------------------------
// Both weight gradients of a channel MLP (y = fc2(act(fc1(x)))) in one launch:
//     dW2 [E, mh]   = do2^T Hh        + db2 = colsum(do2)      (problem 0: column sums of the A operand)
//     dW1^T [E, mh] = xn2^T dHpre     + db1 = colsum(dHpre)    (problem 1: of the B operand; stored transposed -> dW1 [mh, E])
// Two same-shaped problems -> half the split factor of two separate launches (less partial traffic, longer token ranges).
// ---------------------------------------------------------------------------------------------------------------------
namespace dpot {
__device__ __forceinline__ void mlp_wgrad2_reduce_body(int bid, int nblk, const float* __restrict__ ws, int splits, int E,
                                                       int mh, float* __restrict__ dW2, float* __restrict__ dW1,
                                                       float* __restrict__ db2, float* __restrict__ db1, int chain) {
  __shared__ float tile[32][33];
  const long long MN = (long long)E * mh, total = 2 * MN;
  const int L = E > mh ? E : mh;
  // 32 x 32 tiles of the [E, mh] outputs: problem 0 is copied, problem 1 goes out transposed (coalesced both ways)
  const int tn = mh / 32, tcount = (E / 32) * tn;
  for (int tix = bid; tix < 2 * tcount; tix += nblk) {
    const int prob = tix >= tcount, tt = tix - prob * tcount;
    const int r0 = (tt / tn) * 32, c0 = (tt % tn) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = r0 + ty + 8 * q;
      const float v = tn_sum_nodes(ws + (long long)prob * MN + (long long)r * mh + c0 + tx, total, splits, chain);
      if (prob == 0) dW2[(long long)r * mh + c0 + tx] = v;
      else tile[ty + 8 * q][tx] = v;
    }
    if (prob) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + ty + 8 * q;                                   // row of dW1 [mh, E]
        dW1[(long long)c * E + r0 + tx] = tile[tx][ty + 8 * q];
      }
      __syncthreads();
    }
  }
  const float* wc = ws + (long long)tn_chain_count(splits, chain) * total;
  for (int idx = bid * 256 + threadIdx.x; idx < E + mh; idx += nblk * 256) {
    const int prob = idx >= E, g = idx - prob * E;
    (prob ? db1 : db2)[g] = tn_sum_nodes(wc + (long long)prob * L + g, 2ll * L, splits, chain);
  }
}
__global__ __launch_bounds__(256) void mlp_wgrad2_reduce_kernel(const float* __restrict__ ws, int splits, int E, int mh,
                                                                float* __restrict__ dW2, float* __restrict__ dW1,
                                                                float* __restrict__ db2, float* __restrict__ db1) {
  mlp_wgrad2_reduce_body(blockIdx.x, gridDim.x, ws, splits, E, mh, dW2, dW1, db2, db1, 1);
}

// ---------------------------------------------------------------------------------------------------------------------
// ONE finalising launch per DPOT block (round 4): the fixed-order reductions that end a block's backward - the split-K
// partials of the two AFNO weight gradients (+ un-packing to the parameters' layout, bias gradients), those of the two
// channel-MLP weight gradients (+ bias gradients), and the per-sample partials of both GroupNorms' parameter gradients -
// were three launches of a few microseconds each (DPOT-Tiny: 8.1 + 6.5 + 5.3 us per block as eager kernel time, ~4 us each
// inside the replayed graph).  The grid is cut into three slices; each slice runs the body of the stand-alone kernel
// unchanged, so every sum keeps its order (bit-identical results).  A slice of zero workgroups is skipped.
// ---------------------------------------------------------------------------------------------------------------------
struct FinalizeArgs {
  // slice A: AFNO weight gradients (dpot_afno_wgrad2's reduction)
  const float* a_ws; int a_splits, a_nb, a_bs, a_gauss; float *a_dw1, *a_db1, *a_dw2, *a_db2; int nA;
  // slice M: channel-MLP weight gradients (dpot_mlp_wgrad2's reduction)
  const float* m_ws; int m_splits, m_E, m_mh; float *m_dW2, *m_dW1, *m_db2, *m_db1; int nM;
  // slice G: GroupNorm parameter gradients (dpot_groupnorm_param_grads): g_jobs jobs x ceil(E / 64) workgroups
  const float* g_part[2]; float* g_dgamma[2]; float* g_dbeta[2]; int g_jobs, g_B, g_E, nG;
  // slice C: column sums of up to two partial matrices [rows, N] (the bias gradients of the bf16 channel MLP, whose
  // producers - the pack pass and the GEMM epilogue - leave per-row-tile partial sums): out[n] = sum_r part[r, n]
  const float* c_part[2]; float* c_out[2]; int c_rows[2], c_N[2], c_blocks[2];
};
// a workgroup = 32 columns x 8 row lanes (128-byte row segments); a lane strides the rows by 8 with four accumulators
// (four loads in flight), the eight lanes of a column are combined through LDS in a fixed order.  (One thread per column
// over all rows - 16 workgroups of 256 dependent loads at DPOT-M - made the whole finalising launch slower than the
// launches it replaced: DPOT-M 13.23 -> 13.38 ms, profiles/r04_block_finalize_colsum.txt.)
constexpr int CS_COLS = 32, CS_LANES = 8;
__device__ __forceinline__ void colsum_rows_body(int bx, const float* __restrict__ part, float* __restrict__ out, int rows,
                                                 int N) {
  __shared__ float red[CS_LANES][CS_COLS];
  const int tc = threadIdx.x % CS_COLS, tr = threadIdx.x / CS_COLS;
  const int n = bx * CS_COLS + tc;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (n < N) {
    int r = tr;
    for (; r + 3 * CS_LANES < rows; r += 4 * CS_LANES) {
      s0 += part[(long long)r * N + n];
      s1 += part[(long long)(r + CS_LANES) * N + n];
      s2 += part[(long long)(r + 2 * CS_LANES) * N + n];
      s3 += part[(long long)(r + 3 * CS_LANES) * N + n];
    }
    for (; r < rows; r += CS_LANES) s0 += part[(long long)r * N + n];
  }
  red[tr][tc] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (tr == 0 && n < N) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < CS_LANES; ++k) v += red[k][tc];
    out[n] = v;
  }
}
// = norm.hip groupnorm_param_grad_kernel: block = 64 channels x 4 sample lanes, fixed order
__device__ __forceinline__ void gn_param_grad_body(int bx, const float* __restrict__ part, float* __restrict__ dgamma,
                                                   float* __restrict__ dbeta, int B, int E) {
  __shared__ float red[2][4][64];
  const int tc = threadIdx.x & 63, tr = threadIdx.x >> 6;
  const int c = bx * 64 + tc;
  float sg0 = 0.f, sg1 = 0.f, sb0 = 0.f, sb1 = 0.f;
  if (c < E) {
    int b = tr;
    for (; b + 4 < B; b += 8) {
      sg0 += part[((long long)0 * B + b) * E + c];
      sg1 += part[((long long)0 * B + b + 4) * E + c];
      sb0 += part[((long long)1 * B + b) * E + c];
      sb1 += part[((long long)1 * B + b + 4) * E + c];
    }
    for (; b < B; b += 4) {
      sg0 += part[((long long)0 * B + b) * E + c];
      sb0 += part[((long long)1 * B + b) * E + c];
    }
  }
  red[0][tr][tc] = sg0 + sg1;
  red[1][tr][tc] = sb0 + sb1;
  __syncthreads();
  if (tr == 0 && c < E) {
    dgamma[c] = (red[0][0][tc] + red[0][1][tc]) + (red[0][2][tc] + red[0][3][tc]);
    dbeta[c] = (red[1][0][tc] + red[1][1][tc]) + (red[1][2][tc] + red[1][3][tc]);
  }
}
__global__ __launch_bounds__(256) void block_finalize_kernel(const FinalizeArgs a) {
  const int b = blockIdx.x;
  if (b < a.nA) {
    afno_wgrad2_reduce_body(b, a.nA, a.a_ws, a.a_splits, a.a_nb, a.a_bs, a.a_dw1, a.a_db1, a.a_dw2, a.a_db2, a.a_gauss, 1);
  } else if (b < a.nA + a.nM) {
    mlp_wgrad2_reduce_body(b - a.nA, a.nM, a.m_ws, a.m_splits, a.m_E, a.m_mh, a.m_dW2, a.m_dW1, a.m_db2, a.m_db1, 1);
  } else if (b < a.nA + a.nM + a.nG) {
    const int g = b - a.nA - a.nM, per = (a.g_E + 63) / 64;
    const int job = g / per;
    gn_param_grad_body(g - job * per, a.g_part[job], a.g_dgamma[job], a.g_dbeta[job], a.g_B, a.g_E);
  } else {
    int c = b - a.nA - a.nM - a.nG;
    const int job = c >= a.c_blocks[0] ? 1 : 0;
    c -= job * a.c_blocks[0];
    colsum_rows_body(c, a.c_part[job], a.c_out[job], a.c_rows[job], a.c_N[job]);
  }
}
}  // namespace dpot

extern "C" int dpot_mlp_wgrad2_splitk(int T, int E, int mh) {
  static const int enabled = tune("panel", 1);
  if (!enabled || T <= 0 || E <= 0 || mh <= 0 || E % TN_W || mh % TN_W || T % TN_TOK) return 0;
  const long long tiles = 2ll * (E / TN_W) * (mh / TN_W);
  if (tiles > 256) return 0;                           // big layers fill the chip per launch: nothing to merge for
  const int nslab = T / TN_TOK;
  long long s = (256 + tiles / 2) / tiles;
  const long long smax = nslab / 4;
  if (s > smax) s = smax;
  if (s < 1) s = 1;
  while (s > 1 && ((nslab + s - 1) / s) * (s - 1) >= nslab) --s;
  return (int)s;
}

extern "C" int64_t dpot_mlp_wgrad2_ws_elems(int E, int mh, int splitk) {
  const int64_t L = E > mh ? E : mh;
  return (int64_t)splitk * 2 * ((int64_t)E * mh + L);
}

extern "C" int dpot_mlp_wgrad2(const float* do2, const float* Hh, const float* xn2, const float* dHpre, int T, int E,
                               int mh, float* dW2, float* db2, float* dW1, float* db1, float* workspace, int splitk,
                               dpot_stream_t stream) {
  DPOT_REQUIRE(do2 && Hh && xn2 && dHpre && workspace, "mlp_wgrad2: null pointer");
  DPOT_REQUIRE((dW2 && db2 && dW1 && db1) || (!dW2 && !db2 && !dW1 && !db1), "mlp_wgrad2: outputs must be all given or all NULL");
  DPOT_REQUIRE(T > 0 && E % TN_W == 0 && mh % TN_W == 0 && T % TN_TOK == 0, "mlp_wgrad2: needs E, mh %% 128 == 0, T %% 32 == 0");
  DPOT_REQUIRE(aligned16(do2) && aligned16(Hh) && aligned16(xn2) && aligned16(dHpre) && aligned16(workspace),
               "mlp_wgrad2: operands must be 16-byte aligned");
  const int nslab = T / TN_TOK;
  DPOT_REQUIRE(splitk >= 1 && splitk <= nslab && 2ll * splitk <= 65535, "mlp_wgrad2: bad split factor");
  TnArgs p{};
  p.sets[0] = TnSet{do2, Hh, 1, 0};
  p.sets[1] = TnSet{xn2, dHpre, 2, 0};
  p.nper = 1;
  p.lda = E; p.ldb = mh; p.sA = 0; p.sB = 0;
  p.N1 = E; p.N2 = mh; p.T = T; p.batch = 2;
  p.tiles1 = E / TN_W; p.tiles2 = mh / TN_W;
  p.splits = splitk;
  p.slabs_per_split = (nslab + splitk - 1) / splitk;
  DPOT_REQUIRE((long long)p.slabs_per_split * (splitk - 1) < nslab, "mlp_wgrad2: split factor leaves an empty split");
  p.ws = workspace;
  p.csL = E > mh ? E : mh;
  p.gauss = 0; p.splits12 = p.splits; p.slabs_per_split12 = p.slabs_per_split;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(gemm_tn_kernel, dim3((unsigned)(p.tiles1 * p.tiles2), 1, (unsigned)(2 * splitk)), dim3(384), 0, s, p);
  int rc = check_launch("gemm_tn_kernel");
  if (rc || !dW2) return rc;            // dW2 == NULL: partials only, dpot_block_finalize reduces them
  int blocks = 2 * (E / 32) * (mh / 32);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(mlp_wgrad2_reduce_kernel, dim3(blocks), dim3(256), 0, s, (const float*)workspace, splitk, E, mh, dW2,
                     dW1, db2, db1);
  return check_launch("mlp_wgrad2_reduce_kernel");
}

extern "C" int dpot_block_finalize(const float* afno_ws, int afno_splitk, int nb, int bs, float* dw1, float* db1, float* dw2,
                                   float* db2, const float* mlp_ws, int mlp_splitk, int E, int mh, float* dW2, float* dfb2,
                                   float* dW1, float* dfb1, const float* const* gn_parts, float* const* gn_dgammas,
                                   float* const* gn_dbetas, int gn_jobs, int B, int Egn, const float* const* cs_parts,
                                   float* const* cs_outs, const int* cs_rows, const int* cs_cols, int cs_jobs,
                                   dpot_stream_t stream) {
  FinalizeArgs a{};
  if (cs_jobs > 0) {
    DPOT_REQUIRE(cs_jobs <= 2 && cs_parts && cs_outs && cs_rows && cs_cols, "block_finalize: bad column-sum slice");
    for (int i = 0; i < cs_jobs; ++i) {
      DPOT_REQUIRE(cs_parts[i] && cs_outs[i] && cs_rows[i] > 0 && cs_cols[i] > 0, "block_finalize: bad column-sum job %d", i);
      a.c_part[i] = cs_parts[i]; a.c_out[i] = cs_outs[i]; a.c_rows[i] = cs_rows[i]; a.c_N[i] = cs_cols[i];
      a.c_blocks[i] = (cs_cols[i] + CS_COLS - 1) / CS_COLS;
    }
  }
  if (afno_ws) {
    DPOT_REQUIRE(afno_splitk >= 1 && nb > 0 && bs > 0 && dw1 && db1 && dw2 && db2, "block_finalize: bad AFNO slice");
    a.a_ws = afno_ws; a.a_splits = afno_splitk; a.a_nb = nb; a.a_bs = bs; a.a_gauss = tn_gauss(bs) ? tn_gauss_s12(bs, afno_splitk) : 0; a.a_dw1 = dw1; a.a_db1 = db1; a.a_dw2 = dw2; a.a_db2 = db2;
    long long blocks = (2ll * nb * bs * bs + 255) / 256;            // as dpot_afno_wgrad2
    a.nA = (int)(blocks > 4096 ? 4096 : blocks);
  }
  if (mlp_ws) {
    DPOT_REQUIRE(mlp_splitk >= 1 && E > 0 && mh > 0 && E % 32 == 0 && mh % 32 == 0 && dW2 && dfb2 && dW1 && dfb1,
                 "block_finalize: bad channel-MLP slice");
    a.m_ws = mlp_ws; a.m_splits = mlp_splitk; a.m_E = E; a.m_mh = mh; a.m_dW2 = dW2; a.m_dW1 = dW1; a.m_db2 = dfb2; a.m_db1 = dfb1;
    int blocks = 2 * (E / 32) * (mh / 32);                          // as dpot_mlp_wgrad2
    a.nM = blocks > 2048 ? 2048 : blocks;
  }
  if (gn_jobs > 0) {
    DPOT_REQUIRE(gn_jobs <= 2 && gn_parts && gn_dgammas && gn_dbetas && B > 0 && Egn > 0, "block_finalize: bad GroupNorm slice");
    for (int i = 0; i < gn_jobs; ++i) {
      DPOT_REQUIRE(gn_parts[i] && gn_dgammas[i] && gn_dbetas[i], "block_finalize: null pointer in GroupNorm job %d", i);
      a.g_part[i] = gn_parts[i]; a.g_dgamma[i] = gn_dgammas[i]; a.g_dbeta[i] = gn_dbetas[i];
    }
    a.g_jobs = gn_jobs; a.g_B = B; a.g_E = Egn; a.nG = gn_jobs * ((Egn + 63) / 64);
  }
  const int total = a.nA + a.nM + a.nG + a.c_blocks[0] + a.c_blocks[1];
  DPOT_REQUIRE(total > 0, "block_finalize: nothing to do");
  hipLaunchKernelGGL(block_finalize_kernel, dim3((unsigned)total), dim3(256), 0, as_stream(stream), a);
  return check_launch("block_finalize_kernel");
}


// ---------------------------------------------------------------------------------------------------------------------
// Weight gradients of SEVERAL DPOT blocks in one launch.  Nothing on the backward's data path reads a weight gradient - only
// the optimiser does, after the last block - so the blocks' small problems need not run (and fill 256 CUs by deep token
// splits) one block at a time: the operands of n blocks go into the problem table of ONE gemm_tn_kernel launch, and ONE
// finalising launch reduces every block's partials, bias column sums and GroupNorm parameter-gradient partials.  Every block
// keeps a workspace in the layout of its per-block launch, so the reduce bodies above run unchanged; every sum has a fixed
// order.  The caller chooses the split factors: those of the per-block entries (several rounds of workgroups in one launch; the
// same partials and sums - bit-identical results, the model's default) or the one-round rules below, which need 1/n of the
// split factor (longer token ranges per workgroup, 1/n of the partial-sum traffic; another summation order).
// ---------------------------------------------------------------------------------------------------------------------
namespace dpot {
constexpr int WB_MAXBLK = TN_MAXSETS / 2;             // blocks per launch (two sets each)

// the largest split count <= s that leaves no token range empty (ranges of ceil(nslab / s) slabs)
static int tn_no_empty(int nslab, long long s) {
  if (s > nslab) s = nslab;
  if (s < 1) s = 1;
  while (s > 1 && ((nslab + s - 1) / s) * (s - 1) >= nslab) --s;
  return (int)s;
}
// n blocks that do not fit one problem table are cut into equal launches
static int wb_per_launch(int n) {
  const int launches = (n + WB_MAXBLK - 1) / WB_MAXBLK;
  return (n + launches - 1) / launches;
}
static bool mlp_batch_shape_ok(int T, int E, int mh) {
  return T > 0 && E > 0 && mh > 0 && E % TN_W == 0 && mh % TN_W == 0 && T % TN_TOK == 0;
}
// (splits12, splits) of a three-product launch of `per` blocks: the largest split count whose workgroups fit one round of 256
// with at least four slabs per range; 0: not even one range per tile fits
static int afno_batch_splits(int nslab, int nb, int bs, int per, int* s12_out) {
  const long long P = 2ll * per * nb;
  const int smax = nslab / 4 > 1 ? nslab / 4 : 1;
  int best = 0, best12 = 0;
  for (int c = 1; c <= smax && c <= 64; ++c) {
    if (tn_no_empty(nslab, c) != c) continue;
    const int s12 = tn_no_empty(nslab, tn_gauss_s12(bs, c));
    if (P * (2 * s12 + c) <= 256) { best = c; best12 = s12; }
  }
  *s12_out = best12;
  return best;
}

struct WgradFinalizeArgs {
  dpot_wgrad_block blk[WB_MAXBLK];                    // 128 bytes each
  int a_splits, a_nb, a_bs, a_gauss, a_chain, nA;             // slice A of every block: afno_wgrad2_reduce_body
  int m_splits, m_E, m_mh, m_chain, nM;                       // slice M: mlp_wgrad2_reduce_body
  int g_jobs, g_B, g_E, nG;                           // slice G: gn_param_grad_body
};
// grid = blocks x (nA + nM + nG) workgroups, block-major: the slices of block_finalize_kernel, once per DPOT block
__global__ __launch_bounds__(256) void wgrad_batch_finalize_kernel(const WgradFinalizeArgs a) {
  const int per = a.nA + a.nM + a.nG;
  const int k = blockIdx.x / per, b = blockIdx.x - k * per;
  const dpot_wgrad_block& w = a.blk[k];
  if (b < a.nA) {
    afno_wgrad2_reduce_body(b, a.nA, w.afno_ws, a.a_splits, a.a_nb, a.a_bs, w.dw1, w.db1, w.dw2, w.db2, a.a_gauss, a.a_chain);
  } else if (b < a.nA + a.nM) {
    mlp_wgrad2_reduce_body(b - a.nA, a.nM, w.mlp_ws, a.m_splits, a.m_E, a.m_mh, w.dW2, w.dW1, w.dfb2, w.dfb1, a.m_chain);
  } else {
    const int g = b - a.nA - a.nM, pj = (a.g_E + 63) / 64;
    const int job = g / pj;
    gn_param_grad_body(g - job * pj, w.gn_part[job], w.gn_dgamma[job], w.gn_dbeta[job], a.g_B, a.g_E);
  }
}
}  // namespace dpot

extern "C" int dpot_wgrad_batch_max_blocks(void) { return WB_MAXBLK; }

extern "C" int dpot_tn_split_range(int T, int splits, int i, int* first_tok, int* ntok) {
  DPOT_REQUIRE(T > 0 && T % TN_TOK == 0 && splits >= 1 && i >= 0 && i < splits && first_tok && ntok, "tn_split_range: bad arguments");
  // as gemm_tn_kernel cuts the slabs: ranges of ceil(nslab / splits) slabs, the last one shorter
  const int nslab = T / TN_TOK, sps = (nslab + splits - 1) / splits;
  int n = nslab - i * sps;
  n = n < sps ? n : sps;
  if (n < 0) n = 0;
  *first_tok = i * sps * TN_TOK;
  *ntok = n * TN_TOK;
  return DPOT_OK;
}

// split factor of a batched channel-MLP launch over n blocks (0: shape not covered): max(1, 256 / tiles) token ranges of at
// least four slabs - DPOT-Tiny, 4 blocks: 128 tiles x 2
extern "C" int dpot_mlp_wgrad_batch_splitk(int T, int E, int mh, int n) {
  static const int enabled = tune("panel", 1);
  if (!enabled || n < 1 || !mlp_batch_shape_ok(T, E, mh)) return 0;
  const long long tiles = 2ll * wb_per_launch(n) * (E / TN_W) * (mh / TN_W);
  const int nslab = T / TN_TOK;
  long long s = 256 / tiles;
  const long long smax = nslab / 4;
  if (s > smax) s = smax;
  return tn_no_empty(nslab, s);
}

extern "C" int64_t dpot_mlp_wgrad_batch_ws_elems(int E, int mh, int splitk, int n) {
  return (int64_t)n * dpot_mlp_wgrad2_ws_elems(E, mh, splitk);
}

// ---- chained token ranges ----------------------------------------------------------------------------------------------------
// At the per-block split factors the batched launches run several rounds of short workgroups and move ~130 MB of partials per
// DPOT-Tiny step through HBM, only for the finalising launch to add them again in tn_sum_nodes' tree.  A chain c in {2, 4} lets
// ONE workgroup walk the ranges of a node of that tree and add them in registers in the tree's association: the same bits, 1/c
// of the partials and workgroups.  Node j of a tile takes slot j of the workspace (tn_chain_count slots instead of `splits`).
static bool tn_chain_ok(int chain) { return chain == 1 || chain == 2 || chain == 4; }

extern "C" int dpot_tn_chain_count(int splits, int chain) {
  if (splits < 1 || !tn_chain_ok(chain)) return 0;
  return tn_chain_count(splits, chain);
}

extern "C" int dpot_tn_chain_nodes(int splits, int chain, int i, int* first_range, int* nranges) {
  DPOT_REQUIRE(splits >= 1 && tn_chain_ok(chain) && first_range && nranges && i >= 0 && i < tn_chain_count(splits, chain),
               "tn_chain_nodes: bad arguments");
  tn_chain_node(splits, chain, i, first_range, nranges);
  return DPOT_OK;
}

// the largest chain that still leaves one full round of 256 workgroups: the fastest for the launch ALONE.  The model does not
// chain by default - beside the embed backward every chain setting costs the step 20 - 40 us (profiles/wgrad_chain_ab.txt)
extern "C" int dpot_mlp_wgrad_batch_chain(int E, int mh, int splitk, int n) {
  if (n < 1 || splitk < 1 || E <= 0 || mh <= 0 || E % TN_W || mh % TN_W) return 1;
  const long long tiles = 2ll * wb_per_launch(n) * (E / TN_W) * (mh / TN_W);
  for (int c = 4; c > 1; c >>= 1)
    if (tiles * tn_chain_count(splitk, c) >= 256) return c;
  return 1;
}
// (three-product form; `per_launch` blocks per launch.)  Capped at TN_AFNO_CHAIN_MAX: measured at DPOT-Tiny, 2 - 512 equal
// workgroups - 158 us, as unchained; 4 - 320 workgroups of 4, 4, 2 (, 2) ranges - 201 us (profiles/wgrad_chain_ab.txt)
constexpr int TN_AFNO_CHAIN_MAX = 2;
extern "C" int dpot_afno_wgrad_batch_chain(int nb, int per_launch, int splits12, int splitk) {
  if (nb < 1 || per_launch < 1 || splits12 < 1 || splitk < splits12) return 1;
  const long long P = 2ll * per_launch * nb;
  for (int c = TN_AFNO_CHAIN_MAX; c > 1; c >>= 1)
    if (P * (2 * tn_chain_count(splits12, c) + tn_chain_count(splitk, c)) >= 256) return c;
  return 1;
}

extern "C" int64_t dpot_mlp_wgrad_chain_ws_elems(int E, int mh, int splitk, int mlp_chain) {
  return dpot_mlp_wgrad2_ws_elems(E, mh, tn_chain_ok(mlp_chain) ? tn_chain_count(splitk, mlp_chain) : splitk);
}
// (splits12 <= 0: splitk.)  Slots by tn_chain_slots: the larger node count of the P1 / P2 tiles and the sum-product tile
extern "C" int64_t dpot_afno_wgrad_chain_ws_elems(int nb, int bs, int splits12, int splitk, int afno_chain) {
  if (splits12 <= 0 || splits12 > splitk) splits12 = splitk;
  return dpot_afno_wgrad2_ws_elems(nb, bs, tn_chain_ok(afno_chain) ? tn_chain_slots(splits12, splitk, afno_chain) : splitk);
}

namespace dpot {
static void tn_launch_chain(int chain, unsigned nwg, hipStream_t s, const TnArgs& p) {
  if (chain == 4) hipLaunchKernelGGL(gemm_tn_chain_kernel<4>, dim3(nwg), dim3(384), 0, s, p);
  else if (chain == 2) hipLaunchKernelGGL(gemm_tn_chain_kernel<2>, dim3(nwg), dim3(384), 0, s, p);
  else hipLaunchKernelGGL(gemm_tn_kernel, dim3(nwg), dim3(384), 0, s, p);
}
}  // namespace dpot

extern "C" int dpot_mlp_wgrad_batch(const float* const* do2, const float* const* Hh, const float* const* xn2,
                                    const float* const* dHpre, int n, int T, int E, int mh, float* workspace, int splitk,
                                    int mlp_chain, dpot_stream_t stream) {
  DPOT_REQUIRE(tn_chain_ok(mlp_chain), "mlp_wgrad_batch: chain %d (1, 2 or 4)", mlp_chain);
  DPOT_REQUIRE(do2 && Hh && xn2 && dHpre && workspace && n >= 1, "mlp_wgrad_batch: null pointer");
  DPOT_REQUIRE(mlp_batch_shape_ok(T, E, mh), "mlp_wgrad_batch: needs E, mh %% 128 == 0, T %% 32 == 0");
  const int nslab = T / TN_TOK;
  DPOT_REQUIRE(splitk >= 1 && splitk <= nslab && tn_no_empty(nslab, splitk) == splitk,
               "mlp_wgrad_batch: split factor %d leaves an empty token range (%d slabs)", splitk, nslab);
  DPOT_REQUIRE(aligned16(workspace), "mlp_wgrad_batch: workspace must be 16-byte aligned");
  const int per = wb_per_launch(n);
  const long long wsb = dpot_mlp_wgrad_chain_ws_elems(E, mh, splitk, mlp_chain);
  hipStream_t s = as_stream(stream);
  for (int b0 = 0; b0 < n; b0 += per) {
    const int nb_l = n - b0 < per ? n - b0 : per;
    TnArgs p{};
    for (int i = 0; i < nb_l; ++i) {
      const int k = b0 + i;
      DPOT_REQUIRE(do2[k] && Hh[k] && xn2[k] && dHpre[k] && aligned16(do2[k]) && aligned16(Hh[k]) && aligned16(xn2[k]) &&
                       aligned16(dHpre[k]), "mlp_wgrad_batch: operands of block %d must be non-null and 16-byte aligned", k);
      p.sets[2 * i] = TnSet{do2[k], Hh[k], 1, 0};
      p.sets[2 * i + 1] = TnSet{xn2[k], dHpre[k], 2, 0};
    }
    p.nper = 1;
    p.lda = E; p.ldb = mh; p.sA = 0; p.sB = 0;
    p.N1 = E; p.N2 = mh; p.T = T; p.batch = 2;
    p.tiles1 = E / TN_W; p.tiles2 = mh / TN_W;
    p.splits = splitk;
    p.slabs_per_split = (nslab + splitk - 1) / splitk;
    p.ws = workspace + (long long)b0 * wsb;
    p.ws_group = wsb;
    p.csL = E > mh ? E : mh;
    p.gauss = 0; p.splits12 = p.splits; p.slabs_per_split12 = p.slabs_per_split;
    p.nodes = p.nodes12 = tn_chain_count(splitk, mlp_chain);
    const long long nwg = 2ll * nb_l * p.tiles1 * p.tiles2 * p.nodes;
    DPOT_REQUIRE(nwg <= 0x7fffffff, "mlp_wgrad_batch: grid too large");
    p.raster = 1; p.nwg = (int)nwg;
    tn_launch_chain(mlp_chain, (unsigned)nwg, s, p);
    int rc = check_launch("gemm_tn_kernel");
    if (rc) return rc;
  }
  return DPOT_OK;
}

// blocks per launch of the batched three-product AFNO weight gradient (0: shape not covered - per-block launches) and its
// split factors.  The workgroups sets * nb * (2 * splits12 + splits) must fit one round of 256, and the P1 / P2 ranges must
// keep the 5 / 6 proportion to the sum-product ranges (profiles/r05_tn_skew.txt) unless the tokens, not the chip, limit the
// split: DPOT-Tiny (nb = 4) two blocks per launch at (5, 6) - three or four blocks leave (3, 4) / (2, 3); nb = 8: one block
extern "C" int dpot_afno_wgrad_batch_plan(int Mm, int nb, int bs, int n, int* splits12, int* splits) {
  static const int enabled = tune("panel", 1);
  if (!enabled || !splits12 || !splits || n < 1 || nb <= 0 || bs != TN_W || !tn_gauss(bs) || Mm <= 0 || Mm % TN_TOK) return 0;
  const int nslab = Mm / TN_TOK;
  const int smax = tn_no_empty(nslab, nslab / 4);
  for (int per = n < WB_MAXBLK ? n : WB_MAXBLK; per >= 1; --per) {
    int s12 = 0;
    const int c = afno_batch_splits(nslab, nb, bs, per, &s12);
    if (!c) continue;
    const bool balanced = 6 * s12 == 5 * c, token_limited = c == smax;
    if (balanced || token_limited || per == 1) {
      *splits12 = s12; *splits = c;
      return per;
    }
  }
  return 0;
}

extern "C" int64_t dpot_afno_wgrad_batch_ws_elems(int nb, int bs, int splitk, int n) {
  return (int64_t)n * dpot_afno_wgrad2_ws_elems(nb, bs, splitk);
}

extern "C" int dpot_afno_wgrad_batch(const float* const* S, const float* const* dO1pre, const float* const* O1,
                                     const float* const* dO2, int n, int ld, int Mm, int nb, int bs, float* workspace,
                                     int per_launch, int splits12, int splitk, int afno_chain, dpot_stream_t stream) {
  DPOT_REQUIRE(S && dO1pre && O1 && dO2 && workspace && n >= 1, "afno_wgrad_batch: null pointer");
  DPOT_REQUIRE(tn_chain_ok(afno_chain), "afno_wgrad_batch: chain %d (1, 2 or 4)", afno_chain);
  const int N = 2 * bs;
  DPOT_REQUIRE(nb > 0 && bs == TN_W && tn_gauss(bs) && Mm > 0 && Mm % TN_TOK == 0 && ld >= nb * N && ld % 4 == 0,
               "afno_wgrad_batch: needs the three-product form (bs == 128, DPOT_TUNE wgrad_gauss != 0), Mm %% 32 == 0");
  const int nslab = Mm / TN_TOK;
  DPOT_REQUIRE(per_launch >= 1 && per_launch <= WB_MAXBLK, "afno_wgrad_batch: 1 .. %d blocks per launch", WB_MAXBLK);
  DPOT_REQUIRE(splitk >= 1 && splits12 >= 1 && splits12 <= splitk && tn_no_empty(nslab, splitk) == splitk &&
                   tn_no_empty(nslab, splits12) == splits12,
               "afno_wgrad_batch: split factors (%d, %d) leave an empty token range (%d slabs)", splits12, splitk, nslab);
  DPOT_REQUIRE(aligned16(workspace), "afno_wgrad_batch: workspace must be 16-byte aligned");
  const long long wsb = dpot_afno_wgrad_chain_ws_elems(nb, bs, splits12, splitk, afno_chain);
  hipStream_t s = as_stream(stream);
  for (int b0 = 0; b0 < n; b0 += per_launch) {
    const int nb_l = n - b0 < per_launch ? n - b0 : per_launch;
    TnArgs p{};
    for (int i = 0; i < nb_l; ++i) {
      const int k = b0 + i;
      DPOT_REQUIRE(S[k] && dO1pre[k] && O1[k] && dO2[k] && aligned16(S[k]) && aligned16(dO1pre[k]) && aligned16(O1[k]) &&
                       aligned16(dO2[k]), "afno_wgrad_batch: operands of block %d must be non-null and 16-byte aligned", k);
      p.sets[2 * i] = TnSet{S[k], dO1pre[k], 2, 0};
      p.sets[2 * i + 1] = TnSet{O1[k], dO2[k], 2, 0};
    }
    p.nper = nb; p.csL = 0;
    p.lda = ld; p.ldb = ld; p.sA = N; p.sB = N;
    p.N1 = N; p.N2 = N; p.T = Mm; p.batch = 2 * nb;
    p.tiles1 = N / TN_W; p.tiles2 = N / TN_W;
    p.splits = splitk;
    p.slabs_per_split = (nslab + splitk - 1) / splitk;
    p.gauss = 1;
    p.splits12 = splits12;
    p.slabs_per_split12 = (nslab + splits12 - 1) / splits12;
    p.ws = workspace + (long long)b0 * wsb;
    p.ws_group = wsb;
    p.nodes = tn_chain_count(splitk, afno_chain);
    p.nodes12 = tn_chain_count(splits12, afno_chain);
    const long long nwg = 2ll * nb_l * nb * (2 * p.nodes12 + p.nodes);
    DPOT_REQUIRE(nwg <= 0x7fffffff, "afno_wgrad_batch: grid too large");
    p.raster = 1; p.nwg = (int)nwg;
    tn_launch_chain(afno_chain, (unsigned)nwg, s, p);
    int rc = check_launch("gemm_tn_kernel");
    if (rc) return rc;
  }
  return DPOT_OK;
}

extern "C" int dpot_wgrad_batch_finalize(const dpot_wgrad_block* blocks, int n, int afno_splits12, int afno_splitk, int nb,
                                         int bs, int mlp_splitk, int E, int mh, int gn_jobs, int B, int Egn, int mlp_chain,
                                         int afno_chain, dpot_stream_t stream) {
  DPOT_REQUIRE(blocks && n >= 1, "wgrad_batch_finalize: no blocks");
  DPOT_REQUIRE(tn_chain_ok(mlp_chain) && tn_chain_ok(afno_chain), "wgrad_batch_finalize: chains (%d, %d) must be 1, 2 or 4",
               mlp_chain, afno_chain);
  DPOT_REQUIRE(gn_jobs >= 0 && gn_jobs <= 2, "wgrad_batch_finalize: at most two GroupNorm jobs per block");
  WgradFinalizeArgs a{};
  if (afno_splitk > 0) {
    DPOT_REQUIRE(nb > 0 && bs == TN_W && afno_splits12 >= 1 && afno_splits12 <= afno_splitk, "wgrad_batch_finalize: bad AFNO slice");
    a.a_splits = afno_splitk; a.a_nb = nb; a.a_bs = bs; a.a_gauss = afno_splits12; a.a_chain = afno_chain;
    long long blocksA = (2ll * nb * bs * bs + 255) / 256;
    a.nA = (int)(blocksA > 4096 ? 4096 : blocksA);
  }
  if (mlp_splitk > 0) {
    DPOT_REQUIRE(E > 0 && mh > 0 && E % 32 == 0 && mh % 32 == 0, "wgrad_batch_finalize: bad channel-MLP slice");
    a.m_splits = mlp_splitk; a.m_E = E; a.m_mh = mh; a.m_chain = mlp_chain;
    const long long blocksM = 2ll * (E / 32) * (mh / 32);
    a.nM = (int)(blocksM > 2048 ? 2048 : blocksM);
  }
  if (gn_jobs > 0) {
    DPOT_REQUIRE(B > 0 && Egn > 0, "wgrad_batch_finalize: bad GroupNorm slice");
    a.g_jobs = gn_jobs; a.g_B = B; a.g_E = Egn; a.nG = gn_jobs * ((Egn + 63) / 64);
  }
  const int per = a.nA + a.nM + a.nG;
  DPOT_REQUIRE(per > 0, "wgrad_batch_finalize: nothing to do");
  hipStream_t s = as_stream(stream);
  for (int b0 = 0; b0 < n; b0 += WB_MAXBLK) {
    const int nl = n - b0 < WB_MAXBLK ? n - b0 : WB_MAXBLK;
    for (int i = 0; i < nl; ++i) {
      const dpot_wgrad_block& w = blocks[b0 + i];
      DPOT_REQUIRE(!a.nA || (w.afno_ws && w.dw1 && w.db1 && w.dw2 && w.db2), "wgrad_batch_finalize: null AFNO pointer, block %d", b0 + i);
      DPOT_REQUIRE(!a.nM || (w.mlp_ws && w.dW2 && w.dfb2 && w.dW1 && w.dfb1), "wgrad_batch_finalize: null channel-MLP pointer, block %d", b0 + i);
      for (int j = 0; j < gn_jobs; ++j)
        DPOT_REQUIRE(w.gn_part[j] && w.gn_dgamma[j] && w.gn_dbeta[j], "wgrad_batch_finalize: null GroupNorm pointer, block %d", b0 + i);
      a.blk[i] = w;
    }
    hipLaunchKernelGGL(wgrad_batch_finalize_kernel, dim3((unsigned)(nl * per)), dim3(256), 0, s, a);
    int rc = check_launch("wgrad_batch_finalize_kernel");
    if (rc) return rc;
  }
  return DPOT_OK;
}
