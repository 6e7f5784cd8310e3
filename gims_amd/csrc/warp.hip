// Image warps of the reference's data path: cv2.warpPerspective (INTER_LINEAR, BORDER_CONSTANT 0) and cv2.resize
// (INTER_LINEAR, INTER_AREA) for uint8 [n][h][w][c] images, c = 1 or 3, batched over images (blockIdx.z), one launch per call.
// OpenCV 4.x's scalar arithmetic is restated operation by operation; no multiply-add is contracted anywhere (every kernel turns
// contraction off), float64 where OpenCV computes in double.  tests/warp_ref.py is the NumPy restatement the device is pinned to.
#include "common.h"

#include <float.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#include <vector>

namespace gims {

// saturate_cast<int>(double) / saturate_cast<short>(float): cvRound, i.e. round half to even
__device__ __forceinline__ int round_i(double v) { return __double2int_rn(v); }
__device__ __forceinline__ int round_f(float v) { return __float2int_rn(v); }
__device__ __forceinline__ int sat_short(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
__device__ __forceinline__ uint8_t sat_u8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// ---------------------------------------------------------------------------------------------- warpPerspective
// WarpPerspectiveInvoker (imgwarp.cpp) + remapBilinear<FixedPtCast<int, uchar, 15>, RemapVec_8u, short>.  minv: the inverse map
// (cv::invert of M, DECOMP_LU 3x3 fast path, done on the host) [n][9] float64.  One thread per destination pixel, all channels.
__global__ __launch_bounds__(256) void warp_perspective_kernel(const uint8_t* __restrict__ src, int sh, int sw, int c,
                                                               const double* __restrict__ minv, uint8_t* __restrict__ dst, int dh, int dw,
                                                               int bw0) {
#pragma clang fp contract(off)
  const int b = blockIdx.z;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  const double* M = minv + 9 * b;
  // the x origin of the 32x32-class block enters the rounding: X0 per block row, then (X0 + M0 * x1) * W
  const int xb = (x / bw0) * bw0, x1 = x - xb;
  const double X0 = M[0] * xb + M[1] * y + M[2];
  const double Y0 = M[3] * xb + M[4] * y + M[5];
  const double W0 = M[6] * xb + M[7] * y + M[8];
  double W = W0 + M[6] * x1;
  W = W != 0.0 ? 32.0 / W : 0.0;
  double fX = (X0 + M[0] * x1) * W, fY = (Y0 + M[3] * x1) * W;
  // std::max((double)INT_MIN, std::min((double)INT_MAX, v)), NaN included
  fX = ((double)INT_MAX < fX) ? (double)INT_MAX : ((fX < (double)INT_MAX) ? fX : (double)INT_MAX);
  fX = ((double)INT_MIN < fX) ? fX : (double)INT_MIN;
  fY = ((double)INT_MAX < fY) ? (double)INT_MAX : ((fY < (double)INT_MAX) ? fY : (double)INT_MAX);
  fY = ((double)INT_MIN < fY) ? fY : (double)INT_MIN;
  const int X = round_i(fX), Y = round_i(fY);
  const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5);
  const int ax = X & 31, ay = Y & 31;
  // initInterTab2D(INTER_LINEAR, fixpt): products of (1 - t, t) at t = k / 32, scaled to 2^15 and saturated to short; the (0, 0)
  // entry saturates to 32767 and OpenCV's sum fix-up puts the missing unit on its last tap: {32767, 0, 0, 1}
  int w00 = (32 - ay) * (32 - ax) * 32, w01 = (32 - ay) * ax * 32, w10 = ay * (32 - ax) * 32, w11 = ay * ax * 32;
  if (ax == 0 && ay == 0) { w00 = 32767; w11 = 1; }
  uint8_t* out = dst + (((int64_t)b * dh + y) * dw + x) * c;
  const uint8_t* S = src + (int64_t)b * sh * sw * c;
  const bool x0in = sx >= 0 && sx < sw, x1in = sx + 1 >= 0 && sx + 1 < sw;
  const bool y0in = sy >= 0 && sy < sh, y1in = sy + 1 >= 0 && sy + 1 < sh;
  for (int k = 0; k < c; ++k) {
    // taps outside the image read the border value 0 (a neighbourhood wholly outside gives 0 either way)
    const int v00 = (y0in && x0in) ? S[((int64_t)sy * sw + sx) * c + k] : 0;
    const int v01 = (y0in && x1in) ? S[((int64_t)sy * sw + sx + 1) * c + k] : 0;
    const int v10 = (y1in && x0in) ? S[((int64_t)(sy + 1) * sw + sx) * c + k] : 0;
    const int v11 = (y1in && x1in) ? S[((int64_t)(sy + 1) * sw + sx + 1) * c + k] : 0;
    out[k] = sat_u8((v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + (1 << 14)) >> 15);
  }
}

// ---------------------------------------------------------------------------------------------- resize
struct ResizeParams {
  double scale_x, scale_y, inv_scale_x, inv_scale_y;
  int iscale_x, iscale_y, area_mode;
};

// one axis of the linear path's coefficients (the xofs / ialpha and yofs / ibeta loops of cv::resize, fixpt = true)
__device__ __forceinline__ void linear_coef(int d, double scale, double inv_scale, bool area_mode, int n, bool clamp_hi, int& s, int& a0, int& a1) {
#pragma clang fp contract(off)
  float f;
  if (!area_mode) {
    f = (float)((d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
  } else {
    s = (int)floor(d * scale);
    f = (float)((double)(d + 1) - (double)(s + 1) * inv_scale);
    f = f <= 0.f ? 0.f : f - (float)(int)floorf(f);
  }
  if (clamp_hi) {                       // x only: the y rows are clipped in the invoker instead
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n - 1) { f = 0.f; s = n - 1; }
  }
  a0 = sat_short(round_f((1.f - f) * 2048.f));
  a1 = sat_short(round_f(f * 2048.f));
}

// resizeGeneric_<HResizeLinear<uchar, int, short, 2048>, VResizeLinear<uchar, int, short, FixedPtCast<int, uchar, 22>>>: the horizontal
// pass into int rows, then the uchar specialisation of the vertical pass (identical to its SIMD form VResizeLinearVec_32s8u):
// ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
__global__ __launch_bounds__(256) void resize_linear_kernel(const uint8_t* __restrict__ src, int sh, int sw, int c, uint8_t* __restrict__ dst,
                                                            int dh, int dw, ResizeParams p) {
  const int b = blockIdx.z;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  int sx, a0, a1, sy, b0, b1;
  linear_coef(x, p.scale_x, p.inv_scale_x, p.area_mode, sw, true, sx, a0, a1);
  linear_coef(y, p.scale_y, p.inv_scale_y, p.area_mode, sh, false, sy, b0, b1);
  auto clip = [](int v, int n) { return v >= 0 ? (v < n ? v : n - 1) : 0; };
  const int r0 = clip(sy, sh), r1 = clip(sy + 1, sh);
  const uint8_t* S = src + (int64_t)b * sh * sw * c;
  const uint8_t* R0 = S + (int64_t)r0 * sw * c;
  const uint8_t* R1 = S + (int64_t)r1 * sw * c;
  const bool x1in = sx + 1 < sw;        // a1 == 0 whenever the right tap would leave the row
  uint8_t* out = dst + (((int64_t)b * dh + y) * dw + x) * c;
  for (int k = 0; k < c; ++k) {
    const int h0 = R0[sx * c + k] * a0 + (x1in ? R0[(sx + 1) * c + k] * a1 : 0);
    const int h1 = R1[sx * c + k] * a0 + (x1in ? R1[(sx + 1) * c + k] * a1 : 0);
    out[k] = (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
  }
}

// resizeAreaFast_ (integer scales >= 1): block sums; 2x2 with c in {1, 3} goes through ResizeAreaFastVec_SIMD_8u, (sum + 2) >> 2;
// other integer scales: saturate_cast<uchar>(sum * (1.f / area)); blocks cut by the right / bottom edge: (float)sum / count
__global__ __launch_bounds__(256) void resize_area_fast_kernel(const uint8_t* __restrict__ src, int sh, int sw, int c, uint8_t* __restrict__ dst,
                                                               int dh, int dw, ResizeParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.z;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  const int isx = p.iscale_x, isy = p.iscale_y;
  const uint8_t* S = src + (int64_t)b * sh * sw * c;
  uint8_t* out = dst + (((int64_t)b * dh + y) * dw + x) * c;
  const int sy0 = y * isy, sx0 = x * isx;
  if (sy0 >= sh || sx0 >= sw) {
    for (int k = 0; k < c; ++k) out[k] = 0;
    return;
  }
  const bool full = sy0 + isy <= sh && x < sw / isx;
  const bool vec2 = isx == 2 && isy == 2;
  const float scale = 1.f / (float)(isx * isy);
  for (int k = 0; k < c; ++k) {
    int sum = 0, count = 0;
    for (int yy = 0; yy < isy && sy0 + yy < sh; ++yy)
      for (int xx = 0; xx < isx && sx0 + xx < sw; ++xx) {
        sum += S[((int64_t)(sy0 + yy) * sw + sx0 + xx) * c + k];
        ++count;
      }
    int v;
    if (full) v = vec2 ? (sum + 2) >> 2 : round_f((float)sum * scale);
    else v = round_f((float)sum / (float)count);
    out[k] = sat_u8(v);
  }
}

// computeResizeAreaTab, one destination index: the taps in the order OpenCV lists them -- a partial first cell (s1 - 1), the whole
// cells s1 .. s2 - 1, a partial last cell (s2)
struct AreaAxis {
  int s1, s2, first, last;
  float a_first, a_mid, a_last;
  __device__ __forceinline__ int count() const { return first + (s2 - s1) + last; }
  __device__ __forceinline__ void tap(int k, int& s, float& a) const {
    if (first && k == 0) { s = s1 - 1; a = a_first; return; }
    k -= first;
    if (k < s2 - s1) { s = s1 + k; a = a_mid; return; }
    s = s2; a = a_last;
  }
};

__device__ __forceinline__ AreaAxis area_axis(int d, int n, double scale) {
#pragma clang fp contract(off)
  AreaAxis t;
  const double fs1 = d * scale, fs2 = fs1 + scale;
  const double cell = scale < (double)n - fs1 ? scale : (double)n - fs1;
  int s1 = (int)ceil(fs1), s2 = (int)floor(fs2);
  s2 = s2 < n - 1 ? s2 : n - 1;
  s1 = s1 < s2 ? s1 : s2;
  t.s1 = s1; t.s2 = s2;
  t.first = (double)s1 - fs1 > 1e-3;
  t.a_first = (float)(((double)s1 - fs1) / cell);
  t.a_mid = (float)(1.0 / cell);
  t.last = fs2 - (double)s2 > 1e-3;
  const double r = fs2 - (double)s2 < 1.0 ? fs2 - (double)s2 : 1.0;
  t.a_last = (float)((r < cell ? r : cell) / cell);
  return t;
}

// resizeArea_<uchar, float> (non-integer scales >= 1): per source row buf += S * alpha over the x taps, sum += beta * buf over the y
// taps, every product and sum rounded to float; saturate_cast<uchar>(sum)
__global__ __launch_bounds__(256) void resize_area_kernel(const uint8_t* __restrict__ src, int sh, int sw, int c, uint8_t* __restrict__ dst,
                                                          int dh, int dw, ResizeParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.z;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  const AreaAxis ax = area_axis(x, sw, p.scale_x), ay = area_axis(y, sh, p.scale_y);
  const int nx = ax.count(), ny = ay.count();
  const uint8_t* S = src + (int64_t)b * sh * sw * c;
  uint8_t* out = dst + (((int64_t)b * dh + y) * dw + x) * c;
  for (int k = 0; k < c; ++k) {
    float sum = 0.f;
    for (int j = 0; j < ny; ++j) {
      int sy;
      float beta;
      ay.tap(j, sy, beta);
      const uint8_t* row = S + (int64_t)sy * sw * c;
      float buf = 0.f;
      for (int i = 0; i < nx; ++i) {
        int sx;
        float alpha;
        ax.tap(i, sx, alpha);
        buf = buf + (float)row[sx * c + k] * alpha;
      }
      sum = sum + beta * buf;
    }
    out[k] = sat_u8(round_f(sum));
  }
}

// cv::invert(M, DECOMP_LU) for a 3x3 double matrix: the determinant / cofactor fast path; a singular M gives zeros
static void invert3(const double* S, double* D) {
#pragma STDC FP_CONTRACT OFF
  auto s = [&](int r, int c) { return S[3 * r + c]; };
  double d = s(0, 0) * (s(1, 1) * s(2, 2) - s(1, 2) * s(2, 1)) - s(0, 1) * (s(1, 0) * s(2, 2) - s(1, 2) * s(2, 0)) +
             s(0, 2) * (s(1, 0) * s(2, 1) - s(1, 1) * s(2, 0));
  if (d == 0.0) {
    for (int i = 0; i < 9; ++i) D[i] = 0.0;
    return;
  }
  d = 1. / d;
  double t[9];
  t[0] = (s(1, 1) * s(2, 2) - s(1, 2) * s(2, 1)) * d;
  t[1] = (s(0, 2) * s(2, 1) - s(0, 1) * s(2, 2)) * d;
  t[2] = (s(0, 1) * s(1, 2) - s(0, 2) * s(1, 1)) * d;
  t[3] = (s(1, 2) * s(2, 0) - s(1, 0) * s(2, 2)) * d;
  t[4] = (s(0, 0) * s(2, 2) - s(0, 2) * s(2, 0)) * d;
  t[5] = (s(0, 2) * s(1, 0) - s(0, 0) * s(1, 2)) * d;
  t[6] = (s(1, 0) * s(2, 1) - s(1, 1) * s(2, 0)) * d;
  t[7] = (s(0, 1) * s(2, 0) - s(0, 0) * s(2, 1)) * d;
  t[8] = (s(0, 0) * s(1, 1) - s(0, 1) * s(1, 0)) * d;
  memcpy(D, t, sizeof(t));
}

}  // namespace gims

extern "C" int gims_warp_perspective(const uint8_t* src, int32_t n, int32_t sh, int32_t sw, int32_t c, const double* m, uint8_t* dst, int32_t dh,
                                     int32_t dw, double* work, void* stream) {
  using namespace gims;
  GIMS_CHECK_ARG(src && dst && m && work && n > 0 && n <= 4096, "gims_warp_perspective: null / empty arguments");
  GIMS_CHECK_ARG(sh > 0 && sw > 0 && dh > 0 && dw > 0 && (c == 1 || c == 3) && dh <= 65535 * 4, "gims_warp_perspective: bad shape");
  GIMS_CHECK_ARG(((uintptr_t)work & 15) == 0, "gims_warp_perspective: workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  std::vector<double> inv((size_t)9 * n);
  for (int i = 0; i < n; ++i) invert3(m + 9 * i, inv.data() + 9 * i);
  const int rc = upload_table(inv.data(), sizeof(double) * inv.size(), work, s);
  if (rc != GIMS_OK) return rc;
  // WarpPerspectiveInvoker's block shape: only its width matters (the x origin enters the rounding; rows are absolute)
  int bh0 = dh < 16 ? dh : 16;
  const int bw0 = 1024 / bh0 < dw ? 1024 / bh0 : dw;
  hipLaunchKernelGGL(warp_perspective_kernel, dim3(cdiv(dw, 64), cdiv(dh, 4), n), dim3(256), 0, s, src, sh, sw, c, (const double*)work, dst, dh,
                     dw, bw0);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

extern "C" int gims_resize(const uint8_t* src, int32_t n, int32_t sh, int32_t sw, int32_t c, uint8_t* dst, int32_t dh, int32_t dw,
                           int32_t interpolation, void* stream) {
  using namespace gims;
  GIMS_CHECK_ARG(src && dst && n > 0 && n <= 65535, "gims_resize: null / empty arguments");
  GIMS_CHECK_ARG(sh > 0 && sw > 0 && dh > 0 && dw > 0 && (c == 1 || c == 3) && dh <= 65535 * 4, "gims_resize: bad shape");
  GIMS_CHECK_ARG(interpolation == GIMS_INTER_LINEAR || interpolation == GIMS_INTER_AREA, "gims_resize: interpolation must be LINEAR or AREA");
  hipStream_t s = (hipStream_t)stream;
  if (sh == dh && sw == dw) {                                         // cv::resize: equal sizes copy
    GIMS_HIP(hipMemcpyAsync(dst, src, (size_t)n * sh * sw * c, hipMemcpyDeviceToDevice, s));
    return GIMS_OK;
  }
  ResizeParams p;
  p.inv_scale_x = (double)dw / sw;
  p.inv_scale_y = (double)dh / sh;
  p.scale_x = 1. / p.inv_scale_x;
  p.scale_y = 1. / p.inv_scale_y;
  p.iscale_x = (int)nearbyint(p.scale_x);                               // saturate_cast<int>: round half to even
  p.iscale_y = (int)nearbyint(p.scale_y);
  const bool is_area_fast = fabs(p.scale_x - p.iscale_x) < DBL_EPSILON && fabs(p.scale_y - p.iscale_y) < DBL_EPSILON;
  int interp = interpolation;
  if (interp == GIMS_INTER_LINEAR && is_area_fast && p.iscale_x == 2 && p.iscale_y == 2) interp = GIMS_INTER_AREA;
  p.area_mode = interp == GIMS_INTER_AREA;
  const dim3 grid(cdiv(dw, 64), cdiv(dh, 4), n);
  if (interp == GIMS_INTER_AREA && p.scale_x >= 1 && p.scale_y >= 1) {
    if (is_area_fast) {
      hipLaunchKernelGGL(resize_area_fast_kernel, grid, dim3(256), 0, s, src, sh, sw, c, dst, dh, dw, p);
    } else {
      hipLaunchKernelGGL(resize_area_kernel, grid, dim3(256), 0, s, src, sh, sw, c, dst, dh, dw, p);
    }
  } else {
    hipLaunchKernelGGL(resize_linear_kernel, grid, dim3(256), 0, s, src, sh, sw, c, dst, dh, dw, p);
  }
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}
