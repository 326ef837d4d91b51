// dft3.hip - rfftn / irfftn (norm="ortho") over the three spatial axes of a channels-last latent cube, with the box
// truncation of the reference's AFNO3D (models/dpot3d.py:46-97), as three in-LDS direct DFT passes.
//
// The 3-D form of dft.hip's generic kernels.  One workgroup stages a [X*Y*Z, CC] channel slab of one sample in LDS,
// transforms one axis per pass out of LDS and writes once: one read of the field and one write of the kept box (or the
// reverse).  The latent cubes are small (8^3 for 64^3 data at patch 8, 16^3 at most), so dense DFTs cost X + Y + Z MACs
// per point per pass - nothing next to the memory traffic - and any size works: non-cubic, odd, not a power of two.
//
//   forward : z (real -> half complex, only kz < mz: the slab nearly halves) -> y (ky < my) -> x (kx < mx)
//   inverse : x -> y -> z (weights, real part)
//
// The spectrum the mixer MLP leaves is NOT Hermitian on the kz = 0 and Nyquist planes.  torch.fft.irfftn (complex inverse
// over x and y, real inverse over z last) equals
//     Re sum_{kx,ky,kz} w(kz) S e^{+2 pi i (kx x / X + ky y / Y + kz z / Z)} / sqrt(XYZ),
// w = 1 at kz = 0 and (Z even) kz = Z/2, w = 2 otherwise - that sum is what irfft3 evaluates (col_weights = 1).  Its
// adjoint is w(kz) rfftn(g) (rfft3 with col_weights = 1); the adjoint of rfftn is the same sum with w = 1.
//
// LDS layout: channel innermost ([point][re|im][CC]); a wave's lanes are CC channels x 64/CC neighbouring items, the items
// ordered kz (z) fastest, so the complex passes read consecutive words and the real pass a broadcast.
#include "common.h"
#include "dft_common.h"

namespace dpot {

struct Dft3Tw {
  float *cx, *sx, *cy, *sy, *cz, *sz;
};
__device__ __forceinline__ int tw_floats3(int X, int Y, int Z) { return (2 * (X + Y + Z) + 3) & ~3; }
__device__ __forceinline__ Dft3Tw twiddles3(float* sm, int X, int Y, int Z) {
  Dft3Tw t;
  t.cx = sm;
  t.sx = t.cx + X;
  t.cy = t.sx + X;
  t.sy = t.cy + Y;
  t.cz = t.sy + Y;
  t.sz = t.cz + Z;
  make_twiddles(t.cx, t.sx, X);
  make_twiddles(t.cy, t.sy, Y);
  make_twiddles(t.cz, t.sz, Z);
  return t;
}

// x[B,X,Y,Z,E] -> spec[B,mx,my,mz,nb,2,bs]
// LDS: twiddles | R0 = max(X*Y*Z, X*my*mz*2) * CC (the field, later the y-pass output) | R1 = X*Y*mz*2 * CC
__global__ __launch_bounds__(256) void rfft3_kernel(const float* __restrict__ x, float* __restrict__ spec, int X, int Y,
                                                    int Z, int E, int nb, int mx, int my, int mz, int CC, int r0, int colw,
                                                    float scale) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const Dft3Tw tw = twiddles3(sm, X, Y, Z);
  float* in = sm + tw_floats3(X, Y, Z);
  float* A = in + r0 * CC;   // [X*Y, mz, 2, CC]
  float* Bf = in;            // [X, my, mz, 2, CC] (the field is dead after the z pass)

  const int b = blockIdx.y, c0 = blockIdx.x * CC;
  const int tid = threadIdx.x;
  const int c = tid % CC, g = tid / CC, G = 256 / CC;
  const int bs = E / nb;

  const int npts = X * Y * Z;
  const float* xb = x + (long long)b * npts * E + c0;
  for (int idx = tid; idx < npts * CC; idx += 256) in[idx] = xb[(long long)(idx / CC) * E + c];
  __syncthreads();

  // pass 1: along z (real -> half complex, only kz < mz)
  for (int item = g; item < X * Y * mz; item += G) {
    const int xy = item / mz, kz = item % mz;
    const float* row = in + xy * Z * CC + c;
    float re = 0.f, im = 0.f;
    int ti = 0;
    for (int z = 0; z < Z; ++z) {
      const float v = row[z * CC];
      re = fmaf(v, tw.cz[ti], re);
      im = fmaf(-v, tw.sz[ti], im);
      ti += kz;
      if (ti >= Z) ti -= Z;
    }
    A[(item * 2 + 0) * CC + c] = re;
    A[(item * 2 + 1) * CC + c] = im;
  }
  __syncthreads();

  // pass 2: along y (complex -> complex, only ky < my)
  for (int item = g; item < X * my * mz; item += G) {
    const int kz = item % mz, ky = (item / mz) % my, xr = item / (mz * my);
    float re = 0.f, im = 0.f;
    int ti = 0;
    for (int y = 0; y < Y; ++y) {
      const int a = (((xr * Y + y) * mz + kz) * 2) * CC + c;
      const float zr = A[a], zi = A[a + CC];
      const float cc_ = tw.cy[ti], ss_ = tw.sy[ti];
      re = fmaf(zr, cc_, fmaf(zi, ss_, re));
      im = fmaf(zi, cc_, fmaf(-zr, ss_, im));
      ti += ky;
      if (ti >= Y) ti -= Y;
    }
    Bf[(item * 2 + 0) * CC + c] = re;
    Bf[(item * 2 + 1) * CC + c] = im;
  }
  __syncthreads();

  // pass 3: along x (only kx < mx), scale and weight, store planar per channel block
  const int chn = c0 + c;
  const int blk = chn / bs, ci = chn % bs;
  const int plane = my * mz;
  for (int item = g; item < mx * plane; item += G) {
    const int kx = item / plane, rest = item % plane, kz = rest % mz;
    float re = 0.f, im = 0.f;
    int ti = 0;
    for (int xr = 0; xr < X; ++xr) {
      const int a = ((xr * plane + rest) * 2) * CC + c;
      const float zr = Bf[a], zi = Bf[a + CC];
      const float cc_ = tw.cx[ti], ss_ = tw.sx[ti];
      re = fmaf(zr, cc_, fmaf(zi, ss_, re));
      im = fmaf(zi, cc_, fmaf(-zr, ss_, im));
      ti += kx;
      if (ti >= X) ti -= X;
    }
    const float wgt = scale * hermitian_weight(colw, kz, Z);
    const long long o = (((long long)b * mx * plane + item) * nb + blk) * 2 * bs + ci;
    spec[o] = re * wgt;
    spec[o + bs] = im * wgt;
  }
}

// spec[B,mx,my,mz,nb,2,bs] (+ res[B,X,Y,Z,E]) -> y[B,X,Y,Z,E]
// LDS: twiddles | R0 = X*Y*mz*2 * CC (the spectrum [mx*my*mz*2], later the y-pass output) | R1 = X*my*mz*2 * CC
__global__ __launch_bounds__(256) void irfft3_kernel(const float* __restrict__ spec, const float* __restrict__ res,
                                                     float* __restrict__ y, int X, int Y, int Z, int E, int nb, int mx,
                                                     int my, int mz, int CC, int colw, float scale) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const Dft3Tw tw = twiddles3(sm, X, Y, Z);
  float* S = sm + tw_floats3(X, Y, Z);    // [mx, my, mz, 2, CC]
  float* V = S;                           // [X, Y, mz, 2, CC] (the spectrum is dead after the x pass)
  float* U = S + X * Y * mz * 2 * CC;     // [X, my, mz, 2, CC]

  const int b = blockIdx.y, c0 = blockIdx.x * CC;
  const int tid = threadIdx.x;
  const int c = tid % CC, g = tid / CC, G = 256 / CC;
  const int bs = E / nb;
  const int chn = c0 + c;
  const int blk = chn / bs, ci = chn % bs;
  const int plane = my * mz;

  {
    const int total = mx * plane * 2 * CC;
    for (int idx = tid; idx < total; idx += 256) {
      const int part = (idx / CC) & 1, mode = idx / (2 * CC);
      S[idx] = spec[((((long long)b * mx * plane + mode) * nb + blk) * 2 + part) * bs + ci];
    }
  }
  __syncthreads();

  // pass A: along x, U[x,ky,kz] = sum_kx S[kx,ky,kz] e^{+2 pi i kx x / X}
  for (int item = g; item < X * plane; item += G) {
    const int xr = item / plane, rest = item % plane;
    float ur = 0.f, ui = 0.f;
    int ti = 0;
    for (int kx = 0; kx < mx; ++kx) {
      const int a = ((kx * plane + rest) * 2) * CC + c;
      const float sr = S[a], si = S[a + CC];
      const float cc_ = tw.cx[ti], ss_ = tw.sx[ti];
      ur = fmaf(sr, cc_, fmaf(-si, ss_, ur));
      ui = fmaf(sr, ss_, fmaf(si, cc_, ui));
      ti += xr;
      if (ti >= X) ti -= X;
    }
    U[(item * 2 + 0) * CC + c] = ur;
    U[(item * 2 + 1) * CC + c] = ui;
  }
  __syncthreads();

  // pass B: along y, V[x,y,kz] = w(kz) sum_ky U[x,ky,kz] e^{+2 pi i ky y / Y}
  for (int item = g; item < X * Y * mz; item += G) {
    const int kz = item % mz, yy = (item / mz) % Y, xr = item / (mz * Y);
    float vr = 0.f, vi = 0.f;
    int ti = 0;
    for (int ky = 0; ky < my; ++ky) {
      const int a = (((xr * my + ky) * mz + kz) * 2) * CC + c;
      const float ur = U[a], ui = U[a + CC];
      const float cc_ = tw.cy[ti], ss_ = tw.sy[ti];
      vr = fmaf(ur, cc_, fmaf(-ui, ss_, vr));
      vi = fmaf(ur, ss_, fmaf(ui, cc_, vi));
      ti += yy;
      if (ti >= Y) ti -= Y;
    }
    const float wgt = hermitian_weight(colw, kz, Z);
    V[(item * 2 + 0) * CC + c] = vr * wgt;
    V[(item * 2 + 1) * CC + c] = vi * wgt;
  }
  __syncthreads();

  // pass C: along z, y[x,y,z] = scale * sum_kz Re(V[x,y,kz] e^{+2 pi i kz z / Z}) (+ res)
  const int npts = X * Y * Z;
  const long long base = (long long)b * npts * E + c0 + c;
  for (int item = g; item < npts; item += G) {
    const int xy = item / Z, zz = item % Z;
    const float* row = V + xy * mz * 2 * CC + c;
    float acc = 0.f;
    int ti = 0;
    for (int kz = 0; kz < mz; ++kz) {
      const float vr = row[(kz * 2) * CC], vi = row[(kz * 2 + 1) * CC];
      acc = fmaf(vr, tw.cz[ti], fmaf(-vi, tw.sz[ti], acc));
      ti += zz;
      if (ti >= Z) ti -= Z;
    }
    const long long o = base + (long long)item * E;
    float v = acc * scale;
    if (res) v += res[o];
    y[o] = v;
  }
}

}  // namespace dpot

using namespace dpot;

namespace {

long long imax(long long a, long long b) { return a > b ? a : b; }
int host_tw_floats(int X, int Y, int Z) { return (2 * (X + Y + Z) + 3) & ~3; }
// floats per channel of the two slab regions: forward {R0, R1}, inverse {R0, R1}
long long fwd_r0(int X, int Y, int Z, int my, int mz) { return imax((long long)X * Y * Z, (long long)X * my * mz * 2); }
long long fwd_r1(int X, int Y, int mz) { return (long long)X * Y * mz * 2; }
long long inv_r0(int X, int Y, int mz) { return (long long)X * Y * mz * 2; }   // >= mx*my*mz*2: mx <= X, my <= Y
long long inv_r1(int X, int my, int mz) { return (long long)X * my * mz * 2; }

// the widest slab that fits (lds_slab_cc), then narrower ones, down to 16 channels (64-byte runs of the global accesses),
// while the launch would not fill the chip
int pick_cc(int E, int B, long long floats_per_channel, int tw) {
  int cc = lds_slab_cc(E, floats_per_channel, tw);
  while (cc > 16 && (long long)(E / cc) * B < 256) cc >>= 1;
  return cc;
}

bool shape_ok(int X, int Y, int Z, int E, int mx, int my, int mz) {
  return X > 0 && Y > 0 && Z > 0 && E > 0 && mx >= 1 && mx <= X && my >= 1 && my <= Y && mz >= 1 && mz <= Z / 2 + 1 &&
         (long long)X * Y * Z <= (1 << 24);
}

int check_dft3_args(const char* who, int B, int X, int Y, int Z, int E, int nb, int mx, int my, int mz) {
  DPOT_REQUIRE(B > 0 && X > 0 && Y > 0 && Z > 0 && E > 0 && nb > 0, "%s: bad shape", who);
  DPOT_REQUIRE(E % nb == 0, "%s: E=%d not divisible by nb=%d", who, E, nb);
  DPOT_REQUIRE(mx >= 1 && mx <= X && my >= 1 && my <= Y && mz >= 1 && mz <= Z / 2 + 1,
               "%s: kept modes (%d,%d,%d) outside (%d,%d,%d)", who, mx, my, mz, X, Y, Z / 2 + 1);
  DPOT_REQUIRE(B <= 65535, "%s: batch too large for grid.y", who);
  return DPOT_OK;
}

}  // namespace

extern "C" int dpot_dft3_supported(int X, int Y, int Z, int E, int mx, int my, int mz) {
  if (!shape_ok(X, Y, Z, E, mx, my, mz)) return 0;
  const int tw = host_tw_floats(X, Y, Z);
  return lds_slab_cc(E, fwd_r0(X, Y, Z, my, mz) + fwd_r1(X, Y, mz), tw) > 0 &&
         lds_slab_cc(E, inv_r0(X, Y, mz) + inv_r1(X, my, mz), tw) > 0;
}

extern "C" int dpot_rfft3(const float* x, float* spec, int B, int X, int Y, int Z, int E, int nb, int mx, int my, int mz,
                          int col_weights, dpot_stream_t stream) {
  if (int rc = check_dft3_args("rfft3", B, X, Y, Z, E, nb, mx, my, mz)) return rc;
  if (!dpot_dft3_supported(X, Y, Z, E, mx, my, mz)) {
    set_error("rfft3: latent grid %dx%dx%d (kept %dx%dx%d) does not fit LDS", X, Y, Z, mx, my, mz);
    return DPOT_EUNSUP;
  }
  DPOT_REQUIRE(x && spec, "rfft3: null pointer");
  const int tw = host_tw_floats(X, Y, Z);
  const long long r0 = fwd_r0(X, Y, Z, my, mz), r1 = fwd_r1(X, Y, mz);
  const int CC = pick_cc(E, B, r0 + r1, tw);
  const size_t lds = sizeof(float) * ((size_t)tw + (size_t)CC * (size_t)(r0 + r1));
  if (int rc = raise_dynamic_lds<rfft3_kernel>("rfft3")) return rc;
  const float scale = (float)(1.0 / sqrt((double)X * (double)Y * (double)Z));
  hipLaunchKernelGGL(rfft3_kernel, dim3(E / CC, B), dim3(256), lds, as_stream(stream), x, spec, X, Y, Z, E, nb, mx, my,
                     mz, CC, (int)r0, col_weights, scale);
  return check_launch("rfft3_kernel");
}

extern "C" int dpot_irfft3(const float* spec, const float* res, float* y, int B, int X, int Y, int Z, int E, int nb,
                           int mx, int my, int mz, int col_weights, dpot_stream_t stream) {
  if (int rc = check_dft3_args("irfft3", B, X, Y, Z, E, nb, mx, my, mz)) return rc;
  if (!dpot_dft3_supported(X, Y, Z, E, mx, my, mz)) {
    set_error("irfft3: latent grid %dx%dx%d (kept %dx%dx%d) does not fit LDS", X, Y, Z, mx, my, mz);
    return DPOT_EUNSUP;
  }
  DPOT_REQUIRE(spec && y, "irfft3: null pointer");
  const int tw = host_tw_floats(X, Y, Z);
  const long long r0 = inv_r0(X, Y, mz), r1 = inv_r1(X, my, mz);
  const int CC = pick_cc(E, B, r0 + r1, tw);
  const size_t lds = sizeof(float) * ((size_t)tw + (size_t)CC * (size_t)(r0 + r1));
  if (int rc = raise_dynamic_lds<irfft3_kernel>("irfft3")) return rc;
  const float scale = (float)(1.0 / sqrt((double)X * (double)Y * (double)Z));
  hipLaunchKernelGGL(irfft3_kernel, dim3(E / CC, B), dim3(256), lds, as_stream(stream), spec, res, y, X, Y, Z, E, nb, mx,
                     my, mz, CC, col_weights, scale);
  return check_launch("irfft3_kernel");
}
