// data3d.hip - device side of the 3-D input pipeline (reference: utils/griddataset.py:488-501 pad_data and :521-561
// __getitem__ of TemporalDataset3D): for every sample of a batch, in ONE launch,
//     raw [H, W, L, T, C]  --trilinear resize to res^3 (F.interpolate(mode='trilinear'), align_corners=False)-->
//     --channel pad with ones up to n_channels--> --temporal window [t0, t0 + t_in + t_ar)-->
//     --strided sub-sampling [::d0, ::d1, ::d2]-->   xx [r0,r1,r2,t_in,Cmax],  yy [r0,r1,r2,t_ar,Cmax],  r = ceil(res / d)
// Only the frames of the window are resized (the reference resizes the whole trajectory and slices it afterwards).
// Samples of one batch may differ in H, W, L, T and C: the per-sample geometry is a table in DEVICE memory that the caller
// uploads with the raw samples.  Reads the window of the raw sample (corners shared by neighbouring voxels come from the
// caches), writes xx / yy once: 0.78 of the copy rate from 128^3 sources, 0.37 from 64^3 ones, where the instructions per
// element and not the memory set the time (profiles/data3d.txt).
//
// Mapping.  In the source the window of one voxel is ONE contiguous run of (t_in + t_ar) * C floats; in xx (and in yy)
// consecutive voxels are dense, t_in * Cmax (t_ar * Cmax) floats each.  So the lanes run along the flattened (t, c) run of
// a voxel and go on into the next voxel: lane i of a tile handles element i of [voxel][t][c].  Every store instruction
// then writes consecutive floats of xx (a piece of yy where a voxel's run crosses from x to y frames), and each of the
// eight corner loads reads consecutive floats of a source run, for any C and Cmax - no channel count is special.  What
// depends on the voxel alone (three source indices, eight corner offsets, three weights) is computed once per voxel by
// one lane and handed to the others through LDS, where all lanes of a voxel read the same address (a broadcast).
#include "common.h"

namespace dpot {

namespace {

constexpr int kTileVox = 64;            // voxels per tile: 64 * 55 elements = 14 per thread at t_in + t_ar = 11, Cmax = 5
constexpr int kMaxRun = 16384;          // (t_in + t_ar) * Cmax: the bound under which run_frame() is exact
constexpr int kUnroll = 4;              // elements per thread whose loads are in flight together
constexpr int kMaxBlocks = 2048;        // 8 resident workgroups of 256 on each of the 256 CUs

// ATen's area_pixel_compute_source_index + guard_index_and_lambda (align_corners = false, not cubic) in float: the rule of
// data.hip's src_index, here handing back the two indices and the upper weight
__device__ __forceinline__ void src_index3(int dst, float scale, int in_size, int& i0, int& i1, float& l1) {
  float s = scale * (dst + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = s - (float)i0;
}

// e / Cmax for 0 <= e < kMaxRun without an integer division: (e + 0.5) / Cmax is at least 0.5 / Cmax away from an integer,
// the float product is off by less than kMaxRun / Cmax * 2^-22 = 0.004 / Cmax
__device__ __forceinline__ int run_frame(int e, float inv_c) { return (int)(((float)e + 0.5f) * inv_c); }

}  // namespace

// grid (tiles of kTileVox output voxels, grid-strided; sample)
__global__ __launch_bounds__(256) void resize_pad_window3_kernel(const dpot_sample3_desc* __restrict__ jobs,
                                                                 float* __restrict__ xx, float* __restrict__ yy, int res,
                                                                 int t_in, int t_ar, int Cmax, int d0, int d1, int d2) {
  __shared__ long long s_off[kTileVox][8];      // element offset of the voxel's eight corners (frame 0, channel 0)
  __shared__ float s_lam[kTileVox][4];          // upper weight along H, W, L
  const int j = blockIdx.y;
  const dpot_sample3_desc job = jobs[j];
  const int H = job.H, W = job.W, L = job.L, T = job.T, C = job.C, t0 = job.t0;
  // the pointer comes out of a table, so the compiler takes it for a generic one (flat loads): say that it is global
  typedef const float __attribute__((address_space(1))) * global_floats;
  const global_floats src = (global_floats)job.data;
  // malformed entry: the whole workgroup skips it (before any barrier)
  if (!src || H <= 0 || W <= 0 || L <= 0 || C <= 0 || C > Cmax || t0 < 0 || (long long)t0 + t_in + t_ar > T ||
      (long long)T * C > 0x7fffffffll)
    return;
  // d0, d1, d2: the strided sub-sampling x[::d0, ::d1, ::d2] the reference applies AFTER the resize
  // (griddataset.py:557-558): output voxel (o0, o1, o2) is voxel (o0 * d0, o1 * d1, o2 * d2) of the res^3 field
  const int r1 = (res + d1 - 1) / d1, r2 = (res + d2 - 1) / d2;
  const long long nvox = (long long)((res + d0 - 1) / d0) * r1 * r2;
  const long long ntiles = (nvox + kTileVox - 1) / kTileVox;
  const float sh = (float)H / (float)res, sw = (float)W / (float)res, sl = (float)L / (float)res;
  const long long TC = (long long)T * C;
  const int nxe = t_in * Cmax, nye = t_ar * Cmax, run = nxe + nye;
  const float inv_c = 1.f / (float)Cmax;
  const int tid = threadIdx.x;
  // thread tid handles elements tid, tid + 256, ... of the tile's [voxel][run]: (v, e) advance by (dv, de) with a carry
  const int v_first = tid / run, e_first = tid - v_first * run;
  const int dv = 256 / run, de = 256 - dv * run;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long vox0 = tile * kTileVox;
    const int nv = (int)((nvox - vox0 < kTileVox) ? (nvox - vox0) : kTileVox);
    __syncthreads();                                       // the previous tile's records have been read
    if (tid < nv) {
      const long long vox = vox0 + tid;
      const int o0 = (int)(vox / ((long long)r1 * r2));
      const int rem = (int)(vox - (long long)o0 * r1 * r2);
      const int o1 = rem / r2, o2 = rem - o1 * r2;
      int h0, h1, w0, w1, l0, l1;
      float lh, lw, ll;
      src_index3(o0 * d0, sh, H, h0, h1, lh);
      src_index3(o1 * d1, sw, W, w0, w1, lw);
      src_index3(o2 * d2, sl, L, l0, l1, ll);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const long long h = (k & 4) ? h1 : h0, w = (k & 2) ? w1 : w0, l = (k & 1) ? l1 : l0;
        s_off[tid][k] = ((h * W + w) * L + l) * TC;
      }
      s_lam[tid][0] = lh;
      s_lam[tid][1] = lw;
      s_lam[tid][2] = ll;
    }
    __syncthreads();
    const int nitems = nv * run;
    float* const tile_x = xx + ((long long)j * nvox + vox0) * nxe;
    float* const tile_y = yy + ((long long)j * nvox + vox0) * nye;
    int v = v_first, e = e_first;
    // kUnroll elements per thread and trip: all their corner loads are issued before the first is used.  Branch-free, so
    // that they can be: a padded channel loads the sample's last channel and drops it, an element past the tile's end
    // loads what element 0 of the tile loads and stores nothing
    for (int item = tid; item < nitems; item += 256 * kUnroll) {
      float q[kUnroll][8], lam[kUnroll][3];
      float* dst[kUnroll];
      bool pad[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const bool live = item + 256 * u < nitems;
        const int vu = live ? v : 0, eu = live ? e : 0;
        const int t = run_frame(eu, inv_c), c = eu - t * Cmax;
        pad[u] = c >= C;                                   // channels the dataset does not have are ones (griddataset.py:498)
        const global_floats p = src + ((t0 + t) * C + (pad[u] ? C - 1 : c));          // T * C fits an int
#pragma unroll
        for (int k = 0; k < 8; ++k) q[u][k] = p[s_off[vu][k]];
#pragma unroll
        for (int k = 0; k < 3; ++k) lam[u][k] = s_lam[vu][k];
        dst[u] = !live ? nullptr : (eu < nxe ? tile_x + (vu * nxe + eu) : tile_y + (vu * nye + (eu - nxe)));
        v += dv;
        e += de;
        if (e >= run) {
          e -= run;
          ++v;
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const float a1 = lam[u][0], b1 = lam[u][1], c1 = lam[u][2];
        const float a0 = 1.f - a1, b0 = 1.f - b1, c0 = 1.f - c1;
        // ATen's nesting: the first axis outermost, the last axis innermost
        const float val = a0 * (b0 * (c0 * q[u][0] + c1 * q[u][1]) + b1 * (c0 * q[u][2] + c1 * q[u][3])) +
                          a1 * (b0 * (c0 * q[u][4] + c1 * q[u][5]) + b1 * (c0 * q[u][6] + c1 * q[u][7]));
        if (dst[u]) *dst[u] = pad[u] ? 1.f : val;
      }
    }
  }
}

}  // namespace dpot

using namespace dpot;

extern "C" int dpot_resize_pad_window3(const dpot_sample3_desc* samples_dev, int nsamples, float* xx, float* yy, int res,
                                       int t_in, int t_ar, int n_channels, int down0, int down1, int down2,
                                       dpot_stream_t stream) {
  DPOT_REQUIRE(samples_dev && nsamples > 0 && nsamples <= 65535 && xx && res > 0 && t_in > 0 && t_ar >= 0 &&
                   n_channels > 0,
               "resize_pad_window3: bad argument");
  DPOT_REQUIRE(down0 >= 1 && down1 >= 1 && down2 >= 1 && down0 <= res && down1 <= res && down2 <= res,
               "resize_pad_window3: bad down-sampling factors");
  DPOT_REQUIRE(t_ar == 0 || yy != nullptr, "resize_pad_window3: t_ar > 0 needs yy");
  DPOT_REQUIRE((long long)(t_in + (long long)t_ar) * n_channels <= kMaxRun,
               "resize_pad_window3: (t_in + t_ar) * n_channels must not exceed 16384");
  const long long nvox = (long long)((res + down0 - 1) / down0) * ((res + down1 - 1) / down1) * ((res + down2 - 1) / down2);
  long long blocks = (nvox + kTileVox - 1) / kTileVox;
  const long long cap = kMaxBlocks / nsamples > 0 ? kMaxBlocks / nsamples : 1;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(resize_pad_window3_kernel, dim3((unsigned)blocks, nsamples), dim3(256), 0, as_stream(stream),
                     samples_dev, xx, yy, res, t_in, t_ar, n_channels, down0, down1, down2);
  return check_launch("resize_pad_window3_kernel");
}
