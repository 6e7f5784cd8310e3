// SIFT keypoint detection on the device: OpenCV 4.x SIFT_create(nfeatures=0, nOctaveLayers=3, contrastThreshold=0.001,
// edgeThreshold=80, sigma=1.6).detect(img) (the reference's utils/common.py:838-857), restated.  DESIGN.md 4.8 lists every
// constant; tests/sift_ref.py is the float32 NumPy restatement this file matches operation for operation (no fused
// multiply-add anywhere: every kernel turns contraction off).
//
// Stages, each one launch for every image of the batch (blockIdx.z / blockIdx.y = image):
//   sift_upscale_kernel   BGR2GRAY (fixed point) + 2x INTER_LINEAR resize to float      -> scratch
//   sift_blur_kernel      separable GaussianBlur through LDS (BORDER_REFLECT_101); for layer 1 of octave o > 0 it reads
//                         octave o-1 layer 3 decimated by 2 (INTER_NEAREST) and also stores that as layer 0; the DoG
//                         (this layer minus the previous one) is its epilogue
//   sift_extrema_kernel   3x3x3 extrema of DoG layers 1..3 of every octave, appended through a wave-aggregated counter
//   sift_orient_kernel    one wave per candidate: adjustLocalExtrema + calcOrientationHist + the peak loop; up to 18
//                         keypoints land in fixed slots [candidate * 18 + rank], with the sort keys of removeDuplicatedSorted
//   sift_keep_kernel      after the host's stable key sorts: the first of every run of equal (image, x, y, size, angle)
//   sift_scatter_kernel   compaction + the firstOctave = -1 rescale, per-image counts
// and, over the Gaussian levels the detection leaves behind, the descriptor stage (GIMS_AUX_SIFT_DESCRIBE of gims_run_ops):
//   sift_describe_kernel  one wave per keypoint: calcSIFTDescriptor, 128 values
#include "common.h"

#include <math.h>

namespace gims {

constexpr int SIFT_LAYERS = 3;                 // nOctaveLayers
constexpr int SIFT_G = SIFT_LAYERS + 3;        // Gaussian levels per octave
constexpr int SIFT_D = SIFT_LAYERS + 2;        // DoG levels per octave
constexpr int SIFT_BORDER = 5;                 // SIFT_IMG_BORDER
constexpr int SIFT_STEPS = 5;                  // SIFT_MAX_INTERP_STEPS
constexpr int SIFT_BINS = 36;                  // SIFT_ORI_HIST_BINS
constexpr int SIFT_MAX_R = 16;                 // cvRound(4.5 * scl_octv) with scl_octv < 1.6 * 2^(3.5/3)
constexpr int SIFT_MAX_SAMPLES = (2 * SIFT_MAX_R + 1) * (2 * SIFT_MAX_R + 1);
constexpr float SIFT_SIGMA = 1.6f, SIFT_CONTRAST = 0.001f, SIFT_EDGE = 80.f;
constexpr int BLUR_TW = 64, BLUR_TH = 16, BLUR_R = GIMS_SIFT_MAX_RADIUS;

static double round_half_even(double x) { return nearbyint(x); }

int sift_layout(int h, int w, gims_sift_info* info) {
  if (h < 1 || w < 1 || h > 16384 || w > 16384) return GIMS_EINVAL;
  gims_sift_info L = {};
  L.h = h; L.w = w;
  L.n_octaves = (int)round_half_even(log((double)std::min(2 * w, 2 * h)) / log(2.) - 2) + 1;
  if (L.n_octaves < 1 || L.n_octaves > GIMS_SIFT_MAX_OCTAVES) return GIMS_EINVAL;
  // blur sigmas (createInitialImage takes sigma as float, buildGaussianPyramid as double): level 0 is the initial blur of the upscaled image, levels 1..5 the incremental blurs
  double sig[SIFT_G];
  sig[0] = sqrtf(std::max(SIFT_SIGMA * SIFT_SIGMA - 0.5f * 0.5f * 4, 0.01f));
  const double k = pow(2., 1. / SIFT_LAYERS);
  for (int i = 1; i < SIFT_G; ++i) {
    const double prev = pow(k, (double)(i - 1)) * 1.6, tot = prev * k;
    sig[i] = sqrt(tot * tot - prev * prev);
  }
  for (int i = 0; i < SIFT_G; ++i) {
    const int n = (int)round_half_even(sig[i] * 8 + 1) | 1;     // float images: 4 sigma each side
    if (n / 2 > GIMS_SIFT_MAX_RADIUS) return GIMS_EINVAL;
    L.sigma[i] = sig[i];
    L.ksize[i] = n;
    // getGaussianKernelBitExact in double, symmetric, then float; kernel[i][j] = k[n/2 + j]
    const double scale2x = -0.5 * 0.25 / (sig[i] * sig[i]);
    const int n2 = (n - 1) / 2;
    double vals[GIMS_SIFT_MAX_RADIUS + 1], sum = 0;
    for (int t = 0, x = 1 - n; t < n2; ++t, x += 2) { vals[t] = exp((double)(x * x) * scale2x); sum += vals[t]; }
    sum = sum * 2 + 1.0;
    const double mul = 1.0 / sum;
    L.kernel[i][0] = (float)mul;
    for (int t = 0; t < n2; ++t) L.kernel[i][n2 - t] = (float)(vals[t] * mul);
  }
  int64_t off = 0;
  int hh = 2 * h, ww = 2 * w;
  for (int o = 0; o < L.n_octaves; ++o) {
    L.oct_h[o] = hh; L.oct_w[o] = ww;
    L.gauss_offset[o] = off; off += (int64_t)SIFT_G * hh * ww;
    L.dog_offset[o] = off; off += (int64_t)SIFT_D * hh * ww;
    hh /= 2; ww /= 2;
  }
  L.image_floats = off;
  L.scratch_floats = (int64_t)4 * h * w;
  *info = L;
  return GIMS_OK;
}

__device__ __forceinline__ int refl101(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i >= n ? p - i : i;
}

// gray (uint8, OpenCV's BGR2GRAY fixed point) + resize(2x, INTER_LINEAR) on float
__global__ void sift_upscale_kernel(const uint8_t* __restrict__ img, int h, int w, int c, float* __restrict__ out, int64_t out_stride) {
#pragma clang fp contract(off)
  const int W2 = 2 * w, H2 = 2 * h;
  const int b = blockIdx.z;
  const uint8_t* src = img + (int64_t)b * h * w * c;
  float* dst = out + (int64_t)b * out_stride;
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= W2 || y >= H2) return;
  auto tap = [](int d, int n, int& s0, int& s1, float& a0, float& a1) {
    int s = (d & 1) ? (d >> 1) : (d >> 1) - 1;
    float fr = (d & 1) ? 0.25f : 0.75f;
    if (s < 0) { s = 0; fr = 0.f; }
    if (s >= n - 1) { s = n - 1; fr = 0.f; }
    s0 = s; s1 = s + 1 < n ? s + 1 : n - 1;
    a0 = 1.f - fr; a1 = fr;
  };
  auto g = [&](int yy, int xx) -> float {
    const uint8_t* p = src + ((int64_t)yy * w + xx) * c;
    if (c == 1) return (float)p[0];
    return (float)((p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + (1 << 13)) >> 14);
  };
  int x0, x1, y0, y1;
  float a0, a1, b0, b1;
  tap(x, w, x0, x1, a0, a1);
  tap(y, h, y0, y1, b0, b1);
  const float t0 = g(y0, x0) * a0 + g(y0, x1) * a1;
  const float t1 = g(y1, x0) * a0 + g(y1, x1) * a1;
  dst[(int64_t)y * W2 + x] = t0 * b0 + t1 * b1;
}

struct BlurTaps { float k[GIMS_SIFT_MAX_RADIUS + 1]; int r; };

// dst = GaussianBlur(src); src is the previous level (decimate = 0) or octave o-1 layer 3 read at (2y, 2x) (decimate = 1,
// src_h / src_w its size); then dog = dst - src and, when decimating, layer0 = the decimated source.  Row pass then column
// pass, each acc = k0 * s0, acc += k_j * (s_-j + s_+j).
__global__ __launch_bounds__(256) void sift_blur_kernel(const float* __restrict__ src, int src_w, int decimate, float* __restrict__ dst,
                                                        float* __restrict__ dog, float* __restrict__ layer0, int h, int w, int64_t stride,
                                                        BlurTaps taps) {
#pragma clang fp contract(off)
  constexpr int IH = BLUR_TH + 2 * BLUR_R, IW = BLUR_TW + 2 * BLUR_R;
  __shared__ float tin[IH * IW];
  __shared__ float trow[IH * BLUR_TW];
  const int64_t img = (int64_t)blockIdx.z * stride;
  const float* s = src + img;
  const int r = taps.r;
  const int x0 = blockIdx.x * BLUR_TW, y0 = blockIdx.y * BLUR_TH;
  const int ih = BLUR_TH + 2 * r, iw = BLUR_TW + 2 * r;
  for (int i = threadIdx.x; i < ih * iw; i += 256) {
    const int ly = i / iw, lx = i % iw;
    const int gy = refl101(y0 - r + ly, h), gx = refl101(x0 - r + lx, w);
    tin[ly * IW + lx] = decimate ? s[(int64_t)(2 * gy) * src_w + 2 * gx] : s[(int64_t)gy * src_w + gx];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ih * BLUR_TW; i += 256) {
    const int ly = i / BLUR_TW, lx = i % BLUR_TW;
    const float* p = tin + ly * IW + lx + r;
    float acc = taps.k[0] * p[0];
    for (int j = 1; j <= r; ++j) acc = acc + taps.k[j] * (p[-j] + p[j]);
    trow[ly * BLUR_TW + lx] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < BLUR_TH * BLUR_TW; i += 256) {
    const int ly = i / BLUR_TW, lx = i % BLUR_TW;
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy >= h || gx >= w) continue;
    const float* p = trow + (ly + r) * BLUR_TW + lx;
    float acc = taps.k[0] * p[0];
    for (int j = 1; j <= r; ++j) acc = acc + taps.k[j] * (p[-j * BLUR_TW] + p[j * BLUR_TW]);
    const int64_t o = img + (int64_t)gy * w + gx;
    dst[o] = acc;
    if (dog) {
      const float c = tin[(ly + r) * IW + lx + r];
      dog[o] = acc - c;
      if (layer0) layer0[o] = c;
    }
  }
}

struct OctTable {
  int n;                       // octaves with an interior
  int h[GIMS_SIFT_MAX_OCTAVES], w[GIMS_SIFT_MAX_OCTAVES];
  int64_t dog[GIMS_SIFT_MAX_OCTAVES], gauss[GIMS_SIFT_MAX_OCTAVES];
  int64_t start[GIMS_SIFT_MAX_OCTAVES + 1];   // flattened (layer, r, c) work of the interior, per octave
};

__global__ __launch_bounds__(256) void sift_extrema_kernel(const float* __restrict__ pyr, int64_t stride, OctTable T, int4* __restrict__ cand,
                                                           int cap, int32_t* __restrict__ counter) {
  const int b = blockIdx.y;
  const float* P = pyr + (int64_t)b * stride;
  const int64_t total = T.start[T.n];
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = base + threadIdx.x;
    bool hit = false;
    int o = 0, layer = 0, r = 0, c = 0;
    if (i < total) {
      while (i >= T.start[o + 1]) ++o;
      const int h = T.h[o], w = T.w[o];
      const int iw = w - 2 * SIFT_BORDER, ih = h - 2 * SIFT_BORDER;
      int64_t q = i - T.start[o];
      c = (int)(q % iw) + SIFT_BORDER; q /= iw;
      r = (int)(q % ih) + SIFT_BORDER;
      layer = (int)(q / ih) + 1;
      const int64_t plane = (int64_t)h * w;
      const float* cur = P + T.dog[o] + layer * plane + (int64_t)r * w + c;
      const float v = cur[0];
      if (v != 0.f) {
        bool mx = v > 0, mn = v < 0;
#pragma unroll
        for (int d = -1; d <= 1; ++d)
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
              if (d == 0 && dy == 0 && dx == 0) continue;
              const float n = cur[d * plane + dy * w + dx];
              mx = mx && v >= n;
              mn = mn && v <= n;
            }
        hit = mx || mn;
      }
    }
    const uint64_t m = __ballot(hit);
    if (m) {
      int first = 0;
      if (lane == __ffsll((unsigned long long)m) - 1) first = atomicAdd(counter, __popcll(m));
      first = __shfl(first, __ffsll((unsigned long long)m) - 1);
      if (hit) {
        const int slot = first + __popcll(m & ((1ull << lane) - 1));
        if (slot < cap) cand[slot] = make_int4(b, (o << 8) | layer, r, c);
      }
    }
  }
}

// Matx33f::solve(DECOMP_LU) for one right-hand side: Cramer's rule in float, zeros when the determinant is 0
__device__ __forceinline__ void solve3(float dxx, float dyy, float dss, float dxy, float dxs, float dys, float b0, float b1, float b2, float* x) {
#pragma clang fp contract(off)
  const float a00 = dxx, a01 = dxy, a02 = dxs, a10 = dxy, a11 = dyy, a12 = dys, a20 = dxs, a21 = dys, a22 = dss;
  const float det = a00 * (a11 * a22 - a21 * a12) - a01 * (a10 * a22 - a20 * a12) + a02 * (a10 * a21 - a20 * a11);
  if (det == 0.f) { x[0] = x[1] = x[2] = 0.f; return; }
  const float d = 1.f / det;
  x[0] = d * (b0 * (a11 * a22 - a12 * a21) - a01 * (b1 * a22 - a12 * b2) + a02 * (b1 * a21 - a11 * b2));
  x[1] = d * (a00 * (b1 * a22 - a12 * b2) - b0 * (a10 * a22 - a12 * a20) + a02 * (a10 * b2 - b1 * a20));
  x[2] = d * (a00 * (a11 * b2 - b1 * a21) - a01 * (a10 * b2 - b1 * a20) + b0 * (a10 * a21 - a11 * a20));
}

// cv::hal::fastAtan2 (degrees), the scalar polynomial
__device__ __forceinline__ float fast_atan2(float y, float x) {
#pragma clang fp contract(off)
  const float deg = (float)(180.0 / 3.14159265358979323846);
  const float p1 = 0.9997878412794807f * deg, p3 = -0.3258083974640975f * deg, p5 = 0.1555786518463281f * deg, p7 = -0.04432655554792128f * deg;
  const float eps = (float)2.220446049250313e-16;
  const float ax = fabsf(x), ay = fabsf(y);
  float a;
  if (ax >= ay) {
    const float c = ay / (ax + eps), c2 = c * c;
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  } else {
    const float c = ax / (ay + eps), c2 = c * c;
    a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  }
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

struct SiftSlots {             // SoA, cap * GIMS_SIFT_SLOTS entries
  float *x, *y, *size, *angle, *resp;
  int32_t *octave, *image;      // image = n_images marks an empty slot
  int64_t *k0, *k1, *k2;        // sort keys: (octave desc, response desc), (size desc, angle asc), (x asc, y asc)
};

__device__ __forceinline__ uint32_t fbits(float v) { return __float_as_uint(v); }

constexpr int ORIENT_WAVES = 4;

__global__ __launch_bounds__(64 * ORIENT_WAVES) void sift_orient_kernel(const float* __restrict__ pyr, int64_t stride, OctTable T,
                                                                         const int4* __restrict__ cand, int cap, const int32_t* __restrict__ counter,
                                                                         int n_images, SiftSlots S) {
#pragma clang fp contract(off)
  __shared__ float s_wm[ORIENT_WAVES][SIFT_MAX_SAMPLES];
  __shared__ int8_t s_bin[ORIENT_WAVES][SIFT_MAX_SAMPLES];
  __shared__ float s_hist[ORIENT_WAVES][SIFT_BINS];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_cand = min(*counter, cap);
  for (int ci = blockIdx.x * ORIENT_WAVES + wv; ci < n_cand; ci += gridDim.x * ORIENT_WAVES) {
    const int4 cd = cand[ci];
    const int b = cd.x, o = cd.y >> 8;
    int layer = cd.y & 255, r = cd.z, c = cd.w;
    const int h = T.h[o], w = T.w[o];
    const int64_t plane = (int64_t)h * w;
    const float* D = pyr + (int64_t)b * stride + T.dog[o];
    const float img_scale = 1.f / 255.f, ds = img_scale * 0.5f, s2 = img_scale, cs = img_scale * 0.25f;
    float xi = 0, xr = 0, xc = 0;
    bool ok = true;
    int step = 0;
    float dD0 = 0, dD1 = 0, dD2 = 0, dxx = 0, dyy = 0, dxy = 0;
    auto derivs = [&](float& v, float& dss, float& dxs, float& dys) {
      const float* cur = D + layer * plane + (int64_t)r * w + c;
      const float* nx = cur + plane;
      const float* pv = cur - plane;
      v = cur[0];
      dD0 = (cur[1] - cur[-1]) * ds;
      dD1 = (cur[w] - cur[-w]) * ds;
      dD2 = (nx[0] - pv[0]) * ds;
      const float v2 = v * 2.f;
      dxx = (cur[1] + cur[-1] - v2) * s2;
      dyy = (cur[w] + cur[-w] - v2) * s2;
      dss = (nx[0] + pv[0] - v2) * s2;
      dxy = (cur[w + 1] - cur[w - 1] - cur[-w + 1] + cur[-w - 1]) * cs;
      dxs = (nx[1] - nx[-1] - pv[1] + pv[-1]) * cs;
      dys = (nx[w] - nx[-w] - pv[w] + pv[-w]) * cs;
    };
    for (; step < SIFT_STEPS; ++step) {
      float v, dss, dxs, dys, X[3];
      derivs(v, dss, dxs, dys);
      solve3(dxx, dyy, dss, dxy, dxs, dys, dD0, dD1, dD2, X);
      xi = -X[2]; xr = -X[1]; xc = -X[0];
      if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) break;
      const float big = (float)(2147483647 / 3);
      if (!(fabsf(xi) <= big && fabsf(xr) <= big && fabsf(xc) <= big)) { ok = false; break; }
      c += (int)rintf(xc); r += (int)rintf(xr); layer += (int)rintf(xi);
      if (layer < 1 || layer > SIFT_LAYERS || c < SIFT_BORDER || c >= w - SIFT_BORDER || r < SIFT_BORDER || r >= h - SIFT_BORDER) { ok = false; break; }
    }
    if (step >= SIFT_STEPS) ok = false;
    float contr = 0.f;
    if (ok) {
      float v, dss, dxs, dys;
      derivs(v, dss, dxs, dys);
      const float t = dD0 * xc + dD1 * xr + dD2 * xi;
      contr = v * img_scale + t * 0.5f;
      if (fabsf(contr) * (float)SIFT_LAYERS < SIFT_CONTRAST) ok = false;
      const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
      if (det <= 0 || tr * tr * SIFT_EDGE >= (SIFT_EDGE + 1) * (SIFT_EDGE + 1) * det) ok = false;
    }
    const int64_t slot0 = (int64_t)ci * GIMS_SIFT_SLOTS;
    int npk = 0;
    if (ok) {
      const float scale = (float)(1 << o);
      const float kx = ((float)c + xc) * scale, ky = ((float)r + xr) * scale;
      const float e = ((float)layer + xi) / (float)SIFT_LAYERS;
      const float size = SIFT_SIGMA * (float)exp2((double)e) * scale * 2.f;
      const int octave = o + (layer << 8) + ((int)rint(((double)xi + 0.5) * 255) << 16);
      const float resp = fabsf(contr);
      // calcOrientationHist on Gaussian level (o, layer) around (c, r)
      const float scl = size * 0.5f / scale;
      const int rad = min((int)rintf(4.5f * scl), SIFT_MAX_R);     // the bound holds by construction; the min guards the LDS
      const float sig = 1.5f * scl;
      const float expf_scale = -1.f / (2.f * sig * sig);
      const float* G = pyr + (int64_t)b * stride + T.gauss[o] + layer * plane;
      const int side = 2 * rad + 1, len = side * side;
      for (int q = lane; q < len; q += 64) {
        const int i = q / side - rad, j = q % side - rad;
        const int yy = r + i, xx = c + j;
        int8_t bin = -1;
        float wm = 0.f;
        if (yy > 0 && yy < h - 1 && xx > 0 && xx < w - 1) {
          const float* p = G + (int64_t)yy * w + xx;
          const float dx = p[1] - p[-1], dy = p[-w] - p[w];
          const float wt = (float)exp((double)((float)(i * i + j * j) * expf_scale));
          const float ori = fast_atan2(dy, dx);
          const float mag = sqrtf(dx * dx + dy * dy);
          int bb = (int)rintf((SIFT_BINS / 360.f) * ori);
          if (bb >= SIFT_BINS) bb -= SIFT_BINS;
          if (bb < 0) bb += SIFT_BINS;
          bin = (int8_t)bb;
          wm = wt * mag;
        }
        s_bin[wv][q] = bin;
        s_wm[wv][q] = wm;
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      float acc = 0.f;                                  // temphist[lane], summed in sample order
      if (lane < SIFT_BINS)
        for (int q = 0; q < len; ++q)
          if (s_bin[wv][q] == lane) acc += s_wm[wv][q];
      if (lane < SIFT_BINS) s_hist[wv][lane] = acc;
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      float hs = 0.f;
      if (lane < SIFT_BINS) {
        const float* t = s_hist[wv];
        const int m2 = (lane + SIFT_BINS - 2) % SIFT_BINS, m1 = (lane + SIFT_BINS - 1) % SIFT_BINS;
        const int p1 = (lane + 1) % SIFT_BINS, p2 = (lane + 2) % SIFT_BINS;
        hs = (t[m2] + t[p2]) * (1.f / 16.f) + (t[m1] + t[p1]) * (4.f / 16.f) + t[lane] * (6.f / 16.f);
      }
      __builtin_amdgcn_wave_barrier();
      if (lane < SIFT_BINS) s_hist[wv][lane] = hs;
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      float mx = lane < SIFT_BINS ? hs : -1.f;
      for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
      const float thr = mx * 0.8f;
      bool pk = false;
      float angle = 0.f;
      if (lane < SIFT_BINS) {
        const float l = s_hist[wv][(lane + SIFT_BINS - 1) % SIFT_BINS], rr = s_hist[wv][(lane + 1) % SIFT_BINS];
        pk = hs > l && hs > rr && hs >= thr;
        if (pk) {
          float bin = (float)lane + 0.5f * (l - rr) / (l - 2 * hs + rr);
          bin = bin < 0 ? SIFT_BINS + bin : bin >= SIFT_BINS ? bin - SIFT_BINS : bin;
          angle = 360.f - (360.f / SIFT_BINS) * bin;
          if (fabsf(angle - 360.f) < 1.1920929e-07f) angle = 0.f;
        }
      }
      const uint64_t m = __ballot(pk);
      npk = __popcll(m);
      if (pk) {
        const int64_t s = slot0 + __popcll(m & ((1ull << lane) - 1));
        S.x[s] = kx; S.y[s] = ky; S.size[s] = size; S.angle[s] = angle; S.resp[s] = resp;
        S.octave[s] = octave; S.image[s] = b;
        S.k0[s] = ((int64_t)(0xFFFFFF - octave) << 31) | (int64_t)(0x7FFFFFFFu - fbits(resp));
        S.k1[s] = ((int64_t)(0x7FFFFFFFu - fbits(size)) << 31) | (int64_t)fbits(angle);
        S.k2[s] = ((int64_t)fbits(kx) << 31) | (int64_t)fbits(ky);
      }
      __builtin_amdgcn_wave_barrier();
    }
    if (lane >= npk && lane < GIMS_SIFT_SLOTS) {
      const int64_t s = slot0 + lane;
      S.image[s] = n_images;
      S.k0[s] = S.k1[s] = S.k2[s] = 0;
    }
  }
}

// the slots of candidates past the count (or past the capacity) are empty; the orientation kernel fills the rest
__global__ void sift_empty_kernel(const int32_t* __restrict__ counter, int cap, int n_images, SiftSlots S) {
  const int64_t n = (int64_t)cap * GIMS_SIFT_SLOTS;
  for (int64_t s = (int64_t)min(*counter, cap) * GIMS_SIFT_SLOTS + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    S.image[s] = n_images;
    S.k0[s] = S.k1[s] = S.k2[s] = 0;
  }
}

// perm: slot indices in (image, x, y, size desc, angle, response desc, octave desc) order; keep[p] = 1 for the first of every
// run of equal (image, x, y, size, angle) among filled slots
__global__ void sift_keep_kernel(const int64_t* __restrict__ perm, int64_t n, SiftSlots S, int n_images, int32_t* __restrict__ keep) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int64_t s = perm[p];
  int k = S.image[s] < n_images;
  if (k && p > 0) {
    const int64_t t = perm[p - 1];
    k = S.image[t] != S.image[s] || S.x[t] != S.x[s] || S.y[t] != S.y[s] || S.size[t] != S.size[s] || S.angle[t] != S.angle[s];
  }
  keep[p] = k;
}

// pos = inclusive prefix sum of keep; writes kept keypoints with firstOctave = -1 applied, counts[image] += 1
__global__ void sift_scatter_kernel(const int64_t* __restrict__ perm, const int32_t* __restrict__ keep, const int64_t* __restrict__ pos, int64_t n,
                                    SiftSlots S, float* __restrict__ pt, float* __restrict__ size, float* __restrict__ angle, float* __restrict__ resp,
                                    int32_t* __restrict__ octave, int32_t* __restrict__ counts) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || !keep[p]) return;
  const int64_t s = perm[p], d = pos[p] - 1;
  pt[2 * d] = S.x[s] * 0.5f;
  pt[2 * d + 1] = S.y[s] * 0.5f;
  size[d] = S.size[s] * 0.5f;
  angle[d] = S.angle[s];
  resp[d] = S.resp[s];
  const int oc = S.octave[s];
  octave[d] = (oc & ~255) | ((oc - 1) & 255);
  atomicAdd(counts + S.image[s], 1);
}

// ---- descriptors: OpenCV 4.x calcSIFTDescriptor (d = 4, n = 8) over the detector's pyramid, restated (DESIGN.md 4.14;
// include/gims_hip.h GIMS_AUX_SIFT_DESCRIBE has the arithmetic line by line, tests/sift_desc_ref.py is the NumPy restatement).
constexpr int DESC_WAVES = 4;                  // keypoints per workgroup, one wave each
constexpr int DESC_CHUNK = 256;                // candidate samples staged per pass: 9 KiB of LDS per wave
constexpr int DESC_CELLS = 36, DESC_LEN = 128;

struct DescTable {                             // Gaussian levels by pyramid octave
  int n;
  int h[GIMS_SIFT_MAX_OCTAVES], w[GIMS_SIFT_MAX_OCTAVES], diag[GIMS_SIFT_MAX_OCTAVES];   // diag = (int)sqrt(w^2 + h^2), double
  int64_t gauss[GIMS_SIFT_MAX_OCTAVES];
};

// cvRound for values that may be anything: NaN and what does not fit an int go to +-1e9 (exact in float) first
__device__ __forceinline__ int cv_round(float v) { return (int)rintf(fminf(fmaxf(v, -1e9f), 1e9f)); }

// One wave per keypoint.  The (2 radius + 1)^2 samples are visited in OpenCV's order (i outer, j inner), DESC_CHUNK candidates at a
// time: the lanes compute 64 candidates at once and append the kept ones -- their eight trilinear shares and their histogram corner --
// to the wave's LDS slab in candidate order (ballot prefix).  Then lane c < 36 owns spatial cell c of hist[6][6][10] with its ten
// orientation entries in registers (entry 8 is fed by o0 = 7, entry 9 only by o0 = -1, which an angle of -1 produces) and walks the
// slab front to back: every histogram entry is the sum of its shares in ascending sample order from 0, whatever the chunking (a sample that misses the lane's cell adds +0.f, which changes no bit of a sum that is never -0).
// Rows and columns that fall outside 0 < r < rows - 1, 0 < c < cols - 1 are cut from the loop bounds, not tested per sample: the kept
// samples and their order are the same, and a keypoint of any size costs at most the pixels of its level.
__global__ __launch_bounds__(64 * DESC_WAVES) void sift_describe_kernel(const float* __restrict__ pyr, int64_t stride, DescTable T,
                                                                        const float* __restrict__ kp4, const int32_t* __restrict__ octave,
                                                                        const int32_t* __restrict__ image, int n, int n_images,
                                                                        float* __restrict__ out, int64_t ld, int32_t* __restrict__ bad) {
#pragma clang fp contract(off)
  __shared__ float4 s_val[DESC_WAVES][DESC_CHUNK * 2];     // [sample][8]: v000 v001 v010 v011 | v100 v101 v110 v111 (row, column, orientation)
  __shared__ int s_key[DESC_WAVES][DESC_CHUNK];            // (r0 + 1) * 6 + (c0 + 1) in bits 4.., o0 in bits 0..3
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* const vals = (float*)s_val[wv];
  int* const keys = s_key[wv];
  for (int ki = blockIdx.x * DESC_WAVES + wv; ki < n; ki += gridDim.x * DESC_WAVES) {
    float* dst_row = out + (int64_t)ki * ld;
    const float4 kp = make_float4(kp4[4 * (int64_t)ki], kp4[4 * (int64_t)ki + 1], kp4[4 * (int64_t)ki + 2], kp4[4 * (int64_t)ki + 3]);
    const int oc = octave[ki];
    const int b = image ? image[ki] : 0;
    int o = oc & 255;
    o = o < 128 ? o : (-128 | o);
    const int layer = (oc >> 8) & 255;
    const int po = o + 1;                                    // firstOctave = -1
    if (po < 0 || po >= T.n || layer >= SIFT_G || b < 0 || b >= n_images) {
      dst_row[lane] = 0.f;
      dst_row[lane + 64] = 0.f;
      if (lane == 0) atomicAdd(bad, 1);
      continue;
    }
    const float scale = o >= 0 ? 1.f / (float)(1 << o) : (float)(1 << -o);
    const int rows = T.h[po], cols = T.w[po];
    const float* img = pyr + (int64_t)b * stride + T.gauss[po] + (int64_t)layer * rows * cols;
    const float ptx = kp.x * scale, pty = kp.y * scale, scl = kp.z * scale * 0.5f;
    float ori = 360.f - kp.w;
    if (fabsf(ori - 360.f) < 1.1920929e-07f) ori = 0.f;
    const int px = cv_round(ptx), py = cv_round(pty);
    const float arg = ori * (float)(3.14159265358979323846 / 180);
    float cos_t = (float)cos((double)arg), sin_t = (float)sin((double)arg);
    const float bins_per_rad = 8 / 360.f, exp_scale = -1.f / (4 * 4 * 0.5f), hist_width = 3.f * scl;
    const int radius = min(cv_round(hist_width * 1.4142135623730951f * 5 * 0.5f), T.diag[po]);
    cos_t /= hist_width;
    sin_t /= hist_width;
    // i in [i_lo, i_hi], j in [j_lo, j_hi]: the part of -radius .. radius with 0 < py + i < rows - 1, 0 < px + j < cols - 1
    const int i_lo = (int)max((int64_t)-radius, (int64_t)1 - py), i_hi = (int)min((int64_t)radius, (int64_t)rows - 2 - py);
    const int j_lo = (int)max((int64_t)-radius, (int64_t)1 - px), j_hi = (int)min((int64_t)radius, (int64_t)cols - 2 - px);
    const int nj = j_hi - j_lo + 1;
    const int total = (i_hi >= i_lo && nj > 0) ? (i_hi - i_lo + 1) * nj : 0;          // <= (rows - 2) * (cols - 2) < 2^30
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f, a8 = 0.f, a9 = 0.f;   // hist[cell][0 .. 9]
    const int cell = lane < DESC_CELLS ? lane : -64;
    for (int q0 = 0; q0 < total; q0 += DESC_CHUNK) {
      int cnt = 0;
      for (int s = 0; s < DESC_CHUNK && q0 + s < total; s += 64) {
        const int q = q0 + s + lane;
        bool keep = false;
        float v[8];
        int key = 0;
        if (q < total) {
          const int i = i_lo + q / nj, j = j_lo + q % nj;
          const float c_rot = (float)j * cos_t - (float)i * sin_t, r_rot = (float)j * sin_t + (float)i * cos_t;
          float rbin = r_rot + 2 - 0.5f, cbin = c_rot + 2 - 0.5f;
          if (rbin > -1 && rbin < 4 && cbin > -1 && cbin < 4) {
            keep = true;
            const float* p = img + (int64_t)(py + i) * cols + (px + j);
            const float dx = p[1] - p[-1], dy = p[-cols] - p[cols];
            const float mag = sqrtf(dx * dx + dy * dy) * (float)exp((double)((c_rot * c_rot + r_rot * r_rot) * exp_scale));
            float obin = (fast_atan2(dy, dx) - ori) * bins_per_rad;
            const float rf = floorf(rbin), cf = floorf(cbin), of = floorf(obin);
            rbin -= rf; cbin -= cf; obin -= of;
            int o0 = (int)of;
            if (o0 < 0) o0 += 8;
            if (o0 >= 8) o0 -= 8;
            const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
            const float v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11, v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
            v[1] = v_rc00 * obin; v[0] = v_rc00 - v[1];
            v[3] = v_rc01 * obin; v[2] = v_rc01 - v[3];
            v[5] = v_rc10 * obin; v[4] = v_rc10 - v[5];
            v[7] = v_rc11 * obin; v[6] = v_rc11 - v[7];
            // an angle in -1 .. 360 (cv::KeyPoint's range; -1 gives ori = 361) leaves o0 in -1 .. 7; a sample of any other angle whose
            // o0 falls outside that is dropped (code 14), where OpenCV would write outside its histogram
            key = ((((int)rf + 1) * 6 + (int)cf + 1) << 4) | (o0 >= -1 && o0 <= 7 ? o0 & 15 : 14);
          }
        }
        const uint64_t m = __ballot(keep);
        if (keep) {
          const int pos = cnt + __popcll(m & ((1ull << lane) - 1));
          s_val[wv][2 * pos] = make_float4(v[0], v[1], v[2], v[3]);
          s_val[wv][2 * pos + 1] = make_float4(v[4], v[5], v[6], v[7]);
          keys[pos] = key;
        }
        cnt += __popcll(m);
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int p0 = 0; p0 < cnt; p0 += 64) {
        const int mine = p0 + lane < cnt ? keys[p0 + lane] : 0;
        const int m = min(64, cnt - p0);
        for (int t = 0; t < m; ++t) {
          const int key = __builtin_amdgcn_readlane(mine, t);              // wave-uniform
          const int dc = cell - (key >> 4);                                // 0, 1, 6, 7: this lane's cell is (r0 + dr, c0 + dc)
          const bool hit = (dc & ~7) == 0 && ((0xC3 >> (dc & 7)) & 1);
          const int pair = hit ? (dc & 1) | ((dc >> 1) & 2) : 0;
          const float2 sh = *(const float2*)(vals + (p0 + t) * 8 + pair * 2);
          const float v0 = hit ? sh.x : 0.f, v1 = hit ? sh.y : 0.f;
          switch (key & 15) {                                              // o0: entries o0 and o0 + 1 of the cell
            case 0: a0 += v0; a1 += v1; break;
            case 1: a1 += v0; a2 += v1; break;
            case 2: a2 += v0; a3 += v1; break;
            case 3: a3 += v0; a4 += v1; break;
            case 4: a4 += v0; a5 += v1; break;
            case 5: a5 += v0; a6 += v1; break;
            case 6: a6 += v0; a7 += v1; break;
            case 7: a7 += v0; a8 += v1; break;
            case 15: {
              // o0 = -1 (ori above 360: angle -1).  idx - 1 is entry 9 of the cell BEFORE in the flat hist[360], idx entry 0 of this one:
              // this lane's entry 0 takes its own second share, its entry 9 the first share of the pair that lands in the cell after it
              a0 += v1;
              const int dn = dc + 1;
              const bool hn = (dn & ~7) == 0 && ((0xC3 >> (dn & 7)) & 1);
              const float vn = vals[(p0 + t) * 8 + (hn ? (dn & 1) | ((dn >> 1) & 2) : 0) * 2];
              a9 += hn ? vn : 0.f;
              break;
            }
            default: break;                                                // code 14: an o0 outside -1 .. 7, dropped
          }
        }
      }
      __builtin_amdgcn_wave_barrier();                                     // the slab is refilled by the next chunk
    }
    // finalise: fold the circular orientation entries, the interior 4 x 4 cells are the 128 values
    __builtin_amdgcn_wave_barrier();
    if (lane < DESC_CELLS) {
      const int ci = lane / 6 - 1, cj = lane % 6 - 1;
      if (ci >= 0 && ci < 4 && cj >= 0 && cj < 4) {
        float* d = vals + (ci * 4 + cj) * 8;
        d[0] = a0 + a8; d[1] = a1 + a9; d[2] = a2; d[3] = a3; d[4] = a4; d[5] = a5; d[6] = a6; d[7] = a7;
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float nrm2 = 0.f;
    for (int k = 0; k < DESC_LEN; ++k) nrm2 += vals[k] * vals[k];           // every lane the same sum, k ascending
    const float thr = sqrtf(nrm2) * 0.2f;
    const float d0 = fminf(vals[lane], thr), d1 = fminf(vals[lane + 64], thr);
    __builtin_amdgcn_wave_barrier();
    vals[lane] = d0;
    vals[lane + 64] = d1;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    nrm2 = 0.f;
    for (int k = 0; k < DESC_LEN; ++k) nrm2 += vals[k] * vals[k];
    const float f = 512.f / fmaxf(sqrtf(nrm2), 1.1920929e-07f);
    dst_row[lane] = fminf(fmaxf(rintf(d0 * f), 0.f), 255.f);               // saturate_cast<uchar>: round half to even, clamp
    dst_row[lane + 64] = fminf(fmaxf(rintf(d1 * f), 0.f), 255.f);
    __builtin_amdgcn_wave_barrier();                                       // the slab is refilled by the next keypoint
  }
}

static BlurTaps taps_of(const gims_sift_info& L, int i) {
  BlurTaps t = {};
  t.r = L.ksize[i] / 2;
  for (int j = 0; j <= t.r; ++j) t.k[j] = L.kernel[i][j];
  return t;
}

static OctTable oct_table(const gims_sift_info& L) {
  OctTable T = {};
  T.start[0] = 0;
  for (int o = 0; o < L.n_octaves; ++o) {
    T.h[o] = L.oct_h[o]; T.w[o] = L.oct_w[o];
    T.dog[o] = L.dog_offset[o]; T.gauss[o] = L.gauss_offset[o];
  }
  int n = 0;
  for (int o = 0; o < L.n_octaves; ++o) {
    if (L.oct_h[o] <= 2 * SIFT_BORDER || L.oct_w[o] <= 2 * SIFT_BORDER) break;    // later octaves are smaller still
    T.start[o + 1] = T.start[o] + (int64_t)SIFT_LAYERS * (L.oct_h[o] - 2 * SIFT_BORDER) * (L.oct_w[o] - 2 * SIFT_BORDER);
    n = o + 1;
  }
  T.n = n;
  return T;
}

static int slots_of(float* f, int64_t cap, int64_t* k, int32_t* i32, SiftSlots* S) {
  const int64_t n = cap * GIMS_SIFT_SLOTS;
  S->x = f; S->y = f + n; S->size = f + 2 * n; S->angle = f + 3 * n; S->resp = f + 4 * n;
  S->octave = i32; S->image = i32 + n;
  S->k0 = k; S->k1 = k + n; S->k2 = k + 2 * n;
  return GIMS_OK;
}

// GIMS_AUX_SIFT_DESCRIBE of gims_run_ops (include/gims_hip.h): every argument check precedes the first HIP call
int sift_describe_aux(const gims_aux_args& x, hipStream_t st) {
  const int64_t n = x.i[0], n_images = x.i[1], h = x.i[2], w = x.i[3], ld = x.i[4];
  GIMS_CHECK_ARG(n >= 0 && n <= INT32_MAX, "sift_describe: n = %lld is out of range", (long long)n);
  GIMS_CHECK_ARG(n_images >= 1 && n_images <= INT32_MAX, "sift_describe: n_images = %lld (at least 1)", (long long)n_images);
  GIMS_CHECK_ARG(x.p[3] || n_images == 1, "sift_describe: the image index may be NULL only when n_images == 1");
  GIMS_CHECK_ARG(ld >= DESC_LEN, "sift_describe: ld = %lld is below the 128 values of a descriptor", (long long)ld);
  GIMS_CHECK_ARG(x.i[5] == 0, "sift_describe: i[5] is reserved and must be 0");
  gims_sift_info L;
  if (h < 1 || w < 1 || h > INT32_MAX || w > INT32_MAX || sift_layout((int)h, (int)w, &L) != GIMS_OK) {
    set_error("sift_describe: unsupported image size %lld x %lld", (long long)h, (long long)w);
    return GIMS_EINVAL;
  }
  if (n == 0) return GIMS_OK;
  GIMS_CHECK_ARG(x.p[0] && x.p[1] && x.p[2] && x.p[4] && x.p[5], "sift_describe: pyr, kp4, octave, out and bad must not be NULL");
  DescTable T = {};
  T.n = L.n_octaves;
  for (int o = 0; o < L.n_octaves; ++o) {
    T.h[o] = L.oct_h[o]; T.w[o] = L.oct_w[o]; T.gauss[o] = L.gauss_offset[o];
    T.diag[o] = (int)sqrt((double)L.oct_w[o] * L.oct_w[o] + (double)L.oct_h[o] * L.oct_h[o]);
  }
  int32_t* bad = (int32_t*)const_cast<void*>(x.p[5]);
  GIMS_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
  const int blocks = (int)std::min<int64_t>((n + DESC_WAVES - 1) / DESC_WAVES, 1 << 16);
  sift_describe_kernel<<<blocks, 64 * DESC_WAVES, 0, st>>>((const float*)x.p[0], L.image_floats, T, (const float*)x.p[1], (const int32_t*)x.p[2],
                                                           (const int32_t*)x.p[3], (int)n, (int)n_images, (float*)const_cast<void*>(x.p[4]), ld, bad);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

}  // namespace gims

using namespace gims;

extern "C" int gims_sift_layout(int32_t h, int32_t w, gims_sift_info* info) {
  GIMS_CHECK_ARG(info, "gims_sift_layout: info is NULL");
  const int rc = sift_layout(h, w, info);
  if (rc != GIMS_OK) set_error("gims_sift_layout: unsupported image size %d x %d", (int)h, (int)w);
  return rc;
}

extern "C" int gims_sift_pyramid(const uint8_t* img, int32_t n_images, int32_t h, int32_t w, int32_t c, float* pyr, float* scratch, void* stream) {
  GIMS_CHECK_ARG(img && pyr && scratch && n_images >= 1 && (c == 1 || c == 3), "gims_sift_pyramid: bad arguments");
  gims_sift_info L;
  if (sift_layout(h, w, &L) != GIMS_OK) { set_error("gims_sift_pyramid: unsupported image size %d x %d", (int)h, (int)w); return GIMS_EINVAL; }
  hipStream_t st = (hipStream_t)stream;
  const int64_t stride = L.image_floats;
  {
    dim3 blk(64, 4), grd((2 * w + 63) / 64, (2 * h + 3) / 4, n_images);
    sift_upscale_kernel<<<grd, blk, 0, st>>>(img, h, w, c, scratch, L.scratch_floats);
    GIMS_LAUNCH_CHECK();
  }
  for (int o = 0; o < L.n_octaves; ++o) {
    const int hh = L.oct_h[o], ww = L.oct_w[o];
    const int64_t plane = (int64_t)hh * ww;
    float* G = pyr + L.gauss_offset[o];
    float* D = pyr + L.dog_offset[o];
    dim3 grd((ww + BLUR_TW - 1) / BLUR_TW, (hh + BLUR_TH - 1) / BLUR_TH, n_images);
    if (o == 0) {
      // the upscaled image lives in scratch with its own per-image stride: blur one image at a time
      for (int b = 0; b < n_images; ++b) {
        sift_blur_kernel<<<dim3(grd.x, grd.y, 1), 256, 0, st>>>(scratch + (int64_t)b * L.scratch_floats, ww, 0, G + b * stride, nullptr, nullptr,
                                                                hh, ww, 0, taps_of(L, 0));
        GIMS_LAUNCH_CHECK();
      }
    }
    for (int i = 1; i < SIFT_G; ++i) {
      const bool dec = o > 0 && i == 1;
      const float* src = dec ? pyr + L.gauss_offset[o - 1] + (int64_t)SIFT_LAYERS * L.oct_h[o - 1] * L.oct_w[o - 1] : G + (i - 1) * plane;
      sift_blur_kernel<<<grd, 256, 0, st>>>(src, dec ? L.oct_w[o - 1] : ww, dec ? 1 : 0, G + i * plane, D + (i - 1) * plane, dec ? G : nullptr,
                                            hh, ww, stride, taps_of(L, i));
      GIMS_LAUNCH_CHECK();
    }
  }
  return GIMS_OK;
}

extern "C" int gims_sift_detect(const uint8_t* img, int32_t n_images, int32_t h, int32_t w, int32_t c, float* pyr, float* scratch,
                                int32_t* cand, int32_t cand_cap, int32_t* counter, float* slot_f32, int64_t* slot_keys, int32_t* slot_i32,
                                void* stream) {
  GIMS_CHECK_ARG(cand && counter && slot_f32 && slot_keys && slot_i32 && cand_cap >= 1, "gims_sift_detect: bad arguments");
  int rc = gims_sift_pyramid(img, n_images, h, w, c, pyr, scratch, stream);
  if (rc != GIMS_OK) return rc;
  gims_sift_info L;
  sift_layout(h, w, &L);
  hipStream_t st = (hipStream_t)stream;
  const OctTable T = oct_table(L);
  GIMS_HIP(hipMemsetAsync(counter, 0, sizeof(int32_t), st));
  if (T.n > 0) {
    const int64_t total = T.start[T.n];
    const int blocks = (int)std::min<int64_t>((total + 255) / 256, 2048);
    sift_extrema_kernel<<<dim3(blocks, n_images), 256, 0, st>>>(pyr, L.image_floats, T, (int4*)cand, cand_cap, counter);
    GIMS_LAUNCH_CHECK();
  }
  SiftSlots S;
  slots_of(slot_f32, cand_cap, slot_keys, slot_i32, &S);
  {
    const int64_t n = (int64_t)cand_cap * GIMS_SIFT_SLOTS;
    sift_empty_kernel<<<(int)std::min<int64_t>((n + 255) / 256, 4096), 256, 0, st>>>(counter, cand_cap, n_images, S);
    GIMS_LAUNCH_CHECK();
  }
  const int blocks = std::max(1, std::min(cand_cap / ORIENT_WAVES + 1, 4096));
  sift_orient_kernel<<<blocks, 64 * ORIENT_WAVES, 0, st>>>(pyr, L.image_floats, T, (const int4*)cand, cand_cap, counter, n_images, S);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

extern "C" int gims_sift_compact(const int64_t* perm, int64_t n, int32_t n_images, int32_t cand_cap, float* slot_f32, int64_t* slot_keys,
                                 int32_t* slot_i32, int32_t* keep, const int64_t* pos, float* pt, float* size, float* angle, float* response,
                                 int32_t* octave, int32_t* counts, void* stream) {
  GIMS_CHECK_ARG(n >= 0 && n <= (int64_t)cand_cap * GIMS_SIFT_SLOTS, "gims_sift_compact: n out of range");
  if (n == 0) return GIMS_OK;
  hipStream_t st = (hipStream_t)stream;
  SiftSlots S;
  slots_of(slot_f32, cand_cap, slot_keys, slot_i32, &S);
  const int blocks = (int)((n + 255) / 256);
  if (pos == nullptr) {
    sift_keep_kernel<<<blocks, 256, 0, st>>>(perm, n, S, n_images, keep);
  } else {
    sift_scatter_kernel<<<blocks, 256, 0, st>>>(perm, keep, pos, n, S, pt, size, angle, response, octave, counts);
  }
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}
