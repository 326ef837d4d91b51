// resize.hip - Fourier ("spectral") resize of channels-last fields, the operator of the reference's utils/utilities.py:277-305
// (rfft2 -> copy the low frequencies into a spectrum of the new size -> irfft2 -> rescale), as dense products on the fp32
// matrix cores.  evaluate_varyingres.py:225-244 applies it twice per auto-regressive step.
//
//   out[b, x', y', p] = sum_y AyT[y, y'] * ( sum_x AxT[x, x'] * in[b, x, y, p] )                      p = (t, c) plane
//                     + u[x'] * sum_y ByT[y, y'] * ( sum_x v[x] * in[b, x, y, p] )                    even size pairs only
//
// AxT = (Re Dx)^T, AyT = (Re Dy)^T / (nx ny), ByT = -(Im Dy)^T / (nx ny), Im Dx = u v^T (rank one; it vanishes when
// min(nx, mx) is odd or nx == mx).  The matrices are built on the host in float64 (dpot_amd/ops.py ResizePlan), rounded to
// fp32, ZERO-padded to the tile multiples of resize_core.h and passed as plain device pointers, K-major so that a lane group of 16
// reads 16 consecutive floats of a fragment.
//
// The kernel (its scheme, tiling and safety rules) lives in resize_core.h, shared with the 3-D resize (csrc/resize3.hip).
#include "resize_core.h"

using namespace dpot;

extern "C" int dpot_spectral_resize_pad(int n, int output_rows) {
  return resize_pad(n, output_rows);
}

extern "C" int dpot_spectral_resize(const float* in, float* out, const float* axT, const float* ayT, const float* byT,
                                    const float* u, const float* v, int B, int nx, int ny, int mx, int my, int TC,
                                    dpot_stream_t stream) {
  DPOT_REQUIRE(in && out && in != out && axT && ayT, "spectral_resize: null or aliased field / matrix pointer");
  DPOT_REQUIRE(B > 0 && B <= 65535 && nx > 1 && ny > 1 && mx > 1 && my > 1 && TC > 0 && cdiv(TC, RS_PC) <= 65535,
               "spectral_resize: bad sizes B=%d in=%dx%d out=%dx%d TC=%d (every spatial size must be >= 2)", B, nx, ny, mx, my,
               TC);
  const bool even = byT != nullptr;
  DPOT_REQUIRE(!even || (u && v), "spectral_resize: the second term needs byT, u and v together");
  ResizeArgs a;
  a.in = in, a.out = out, a.axT = axT, a.ayT = ayT, a.byT = byT, a.u = u, a.v = v;
  a.nx = nx, a.ny = ny, a.mx = mx, a.my = my, a.TC = TC;
  a.add = nullptr, a.coef = nullptr, a.xper = 1;
  const bool vec = TC % 4 == 0 && aligned16(in) && aligned16(out);
  hipStream_t s = as_stream(stream);
  const char* what = "spectral_resize";
  if (even)
    return vec ? launch_spectral_resize<true, true, false>(what, a, B, s) : launch_spectral_resize<true, false, false>(what, a, B, s);
  return vec ? launch_spectral_resize<false, true, false>(what, a, B, s) : launch_spectral_resize<false, false, false>(what, a, B, s);
}
