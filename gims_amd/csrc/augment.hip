// Colour augmentation of the training images: the albumentations stage of the reference's COCO_loader (utils/dataset.py:23-29)
// -- brightness / contrast as a 256-entry LUT, motion blur (cv2.filter2D restated, BORDER_REFLECT_101) and Gaussian noise from a
// counter-based integer generator -- for uint8 [n][h][w][c] images, c = 1 or 3, every image under its own plan, ONE launch for the batch
// (blockIdx.y = image).  include/gims_hip.h carries the specification; tests/aug_ref.py is the NumPy restatement the device equals bit
// for bit.  Every multiply-add is an explicit fmaf; contraction is off.
//
// An image without blur is byte traffic: one thread per 16 bytes, moved as one aligned 16-byte load and store where source and
// destination are misaligned alike (the bytes before the first aligned address and after the last go one by one).  A blurred image goes
// tile by tile: 64 x 16 output pixels per workgroup, the source (LUT applied) staged once in LDS with a 3-pixel halo -- tiles whose halo
// lies inside the image by aligned dwords, rows keeping their misalignment as a per-row shift; tiles at the border byte by byte through
// the reflection.
#include "common.h"

#include <math.h>
#include <stddef.h>
#include <string.h>

namespace gims {
namespace {

constexpr int AUG_TW = 64, AUG_TH = 16, AUG_HALO = 3;
constexpr int AUG_ROWS = AUG_TH + 2 * AUG_HALO;                                 // 22 tile rows
constexpr int AUG_PITCH = ((AUG_TW + 2 * AUG_HALO) * 3 + 3 + 3) / 4 * 4;        // 70 pixels x 3 channels + a shift of <= 3, in whole dwords: 216
constexpr int AUG_CHUNK = 16;                                                   // bytes per thread of an image without blur
static_assert(sizeof(gims_aug_plan) == 472 && offsetof(gims_aug_plan, key) == 464, "gims_aug_plan layout");

__device__ __forceinline__ uint64_t aug_splitmix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// z of element e under `key`: twelve 16-bit lanes of three chained splitmix64 values, centred and scaled (exact in float32)
__device__ __forceinline__ float aug_noise_z(uint64_t key, uint32_t e) {
  uint64_t s = key ^ ((uint64_t)e * 0x9E3779B97F4A7C15ull);
  uint32_t sum = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    s = aug_splitmix(s);
    sum += (uint32_t)(s & 0xffffu) + (uint32_t)((s >> 16) & 0xffffu) + (uint32_t)((s >> 32) & 0xffffu) + (uint32_t)(s >> 48);
  }
  return (float)((int)sum - 393210) / 65536.f;
}

__device__ __forceinline__ uint32_t aug_noise_px(float sigma, uint64_t key, uint32_t e, uint32_t p) {
#pragma clang fp contract(off)
  float v = fmaf(sigma, aug_noise_z(key, e), (float)p);
  v = fminf(fmaxf(v, 0.f), 255.f);
  return (uint32_t)(int)v;                                                      // truncation
}

// cv::borderInterpolate(p, len, BORDER_REFLECT_101)
__device__ __forceinline__ int aug_reflect101(int p, int len) {
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
  return p;
}

__device__ __forceinline__ uint32_t aug_sat_u8(float acc) {                     // saturate_cast<uchar>(float): cvRound, then clamp
  const int v = __float2int_rn(acc);
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__global__ __launch_bounds__(256) void color_aug_kernel(const uint8_t* __restrict__ src, int h, int w, int c, const gims_aug_plan* __restrict__ plans,
                                                        uint8_t* __restrict__ dst) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) uint8_t tile_s[AUG_ROWS * AUG_PITCH];
  __shared__ uint8_t lut_s[256];
  __shared__ float coef_s[49];
  __shared__ int off_s[49];
  __shared__ int ntaps_s;
  const int b = blockIdx.y, tid = threadIdx.x;
  const gims_aug_plan& P = plans[b];
  const int ksize = P.ksize;
  const int hwc = h * w * c;
  const uint8_t* S = src + (int64_t)b * hwc;
  uint8_t* D = dst + (int64_t)b * hwc;
  lut_s[tid] = P.use_lut ? P.lut[tid] : (uint8_t)tid;

  if (ksize == 0) {                                                             // LUT and / or noise, or a copy
    __syncthreads();
    const float sigma = P.sigma;
    const uint64_t key = P.key;
    const bool noise = sigma > 0.f;
    const int sa = (int)((uintptr_t)S & 15), da = (int)((uintptr_t)D & 15);
    const bool vec = sa == da;
    const int64_t lo = ((int64_t)blockIdx.x * 256 + tid) * AUG_CHUNK - (vec ? sa : 0);      // this thread's bytes: [lo, lo + 16) of the image
    if (lo >= hwc) return;
    if (vec && lo >= 0 && lo + AUG_CHUNK <= hwc) {
      const uint4 v = *(const uint4*)(S + lo);
      const uint32_t in[4] = {v.x, v.y, v.z, v.w};
      uint32_t out[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t o = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t p = lut_s[(in[q] >> (8 * j)) & 255u];
          if (noise) p = aug_noise_px(sigma, key, (uint32_t)(lo + 4 * q + j), p);
          o |= p << (8 * j);
        }
        out[q] = o;
      }
      *(uint4*)(D + lo) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
      for (int j = 0; j < AUG_CHUNK; ++j) {
        const int64_t i = lo + j;
        if (i < 0 || i >= hwc) continue;
        uint32_t p = lut_s[S[i]];
        if (noise) p = aug_noise_px(sigma, key, (uint32_t)i, p);
        D[i] = (uint8_t)p;
      }
    }
    return;
  }

  // ---- motion blur
  const int tiles_x = (w + AUG_TW - 1) / AUG_TW, tiles = tiles_x * ((h + AUG_TH - 1) / AUG_TH);
  if ((int)blockIdx.x >= tiles) return;                                         // the grid is sized for the image of the batch that needs most
  const int r = ksize >> 1;
  const int x0 = ((int)blockIdx.x % tiles_x) * AUG_TW, y0 = ((int)blockIdx.x / tiles_x) * AUG_TH;
  const int rowb = (AUG_TW + 2 * AUG_HALO) * c;                                 // bytes of one tile row: 210 or 70
  if (tid < 64) {                                                               // the non-zero taps, in row-major order
    const float kf = tid < ksize * ksize ? P.kernel[tid] : 0.f;
    const unsigned long long m = __ballot(kf != 0.f);
    if (kf != 0.f) {
      const int rank = __popcll(m & ((1ull << tid) - 1ull));
      coef_s[rank] = kf;
      off_s[rank] = ((tid / ksize - r + AUG_HALO) << 8) | ((tid % ksize - r + AUG_HALO) * c);       // (tile row offset, tile byte offset)
    }
    if (tid == 0) ntaps_s = __popcll(m);
  }
  __syncthreads();
  // a tile whose halo (and the <= 3 bytes an aligned dword reaches beyond it) lies inside the image: x0 >= 64 leaves 61 pixels before the
  // halo, y0 + 19 < h leaves a whole row after the last tile row
  const bool interior = x0 >= AUG_TW && x0 + AUG_TW + AUG_HALO <= w && y0 >= AUG_TH && y0 + AUG_TH + AUG_HALO < h;
  int a0 = 0, wcm = 0;                                                          // row `row` of the tile sits (a0 + row * wcm) & 3 bytes into its LDS row
  if (interior) {
    const uint8_t* R0 = S + ((int64_t)(y0 - AUG_HALO) * w + (x0 - AUG_HALO)) * c;
    a0 = (int)((uintptr_t)R0 & 3);
    wcm = (w * c) & 3;
    constexpr int NDW = AUG_PITCH / 4;
    for (int idx = tid; idx < AUG_ROWS * NDW; idx += 256) {
      const int row = idx / NDW, k = idx - row * NDW;
      const int sh = (a0 + row * wcm) & 3;
      if (4 * k >= sh + rowb) continue;
      const uint32_t v = *(const uint32_t*)(R0 + (int64_t)row * w * c - sh + 4 * k);
      const uint32_t o = (uint32_t)lut_s[v & 255u] | ((uint32_t)lut_s[(v >> 8) & 255u] << 8) | ((uint32_t)lut_s[(v >> 16) & 255u] << 16) |
                         ((uint32_t)lut_s[v >> 24] << 24);
      *(uint32_t*)(tile_s + row * AUG_PITCH + 4 * k) = o;
    }
  } else {
    for (int idx = tid; idx < AUG_ROWS * rowb; idx += 256) {
      const int row = idx / rowb, j = idx - row * rowb;
      const int px = j / c, ch = j - px * c;
      const int y = aug_reflect101(y0 - AUG_HALO + row, h), x = aug_reflect101(x0 - AUG_HALO + px, w);
      tile_s[row * AUG_PITCH + j] = lut_s[S[((int64_t)y * w + x) * c + ch]];
    }
  }
  __syncthreads();
  const int ob = AUG_TW * c, groups = ob / 4;                                   // output bytes of a tile row, in groups of 4
  const int nt = ntaps_s;
  const int row_valid = (w - x0 < AUG_TW ? w - x0 : AUG_TW) * c;                // bytes of a tile row that lie inside the image
  for (int g = tid; g < AUG_TH * groups; g += 256) {
    const int row = g / groups, j0 = (g - row * groups) * 4;
    const int y = y0 + row, valid = row_valid - j0;
    if (y >= h || valid <= 0) continue;
    uint32_t o = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float acc = 0.f;
      for (int t = 0; t < nt; ++t) {
        const int off = off_s[t], rr = row + (off >> 8);
        const uint8_t p = tile_s[rr * AUG_PITCH + ((a0 + rr * wcm) & 3) + j0 + q + (off & 255)];
        acc = fmaf(coef_s[t], (float)p, acc);
      }
      o |= aug_sat_u8(acc) << (8 * q);
    }
    uint8_t* out = D + ((int64_t)y * w + x0) * c + j0;
    if (valid >= 4 && ((uintptr_t)out & 3) == 0) {
      *(uint32_t*)out = o;
    } else {
      for (int q = 0; q < 4 && q < valid; ++q) out[q] = (uint8_t)(o >> (8 * q));
    }
  }
}

}  // namespace
}  // namespace gims

extern "C" size_t gims_color_aug_workspace_bytes(int32_t n) { return n > 0 ? ((size_t)n * sizeof(gims_aug_plan) + 15) / 16 * 16 : 0; }

extern "C" int gims_color_aug(const uint8_t* src, int32_t n, int32_t h, int32_t w, int32_t c, const gims_aug_plan* plans, uint8_t* dst, void* work,
                              size_t work_bytes, void* stream) {
  using namespace gims;
  if (n == 0) return GIMS_OK;
  GIMS_CHECK_ARG(src && dst && plans && n > 0 && n <= 65535, "gims_color_aug: null arguments or a batch of more than 65535 images");
  GIMS_CHECK_ARG(c == 1 || c == 3, "gims_color_aug: images have 1 or 3 channels, not %d", c);
  GIMS_CHECK_ARG(h > 0 && w > 0 && (int64_t)h * w * c < ((int64_t)1 << 31), "gims_color_aug: bad shape %d x %d x %d", h, w, c);
  const size_t bytes = (size_t)n * h * w * c;
  GIMS_CHECK_ARG((uintptr_t)src + bytes <= (uintptr_t)dst || (uintptr_t)dst + bytes <= (uintptr_t)src,
                 "gims_color_aug: dst overlaps src (the blur reads neighbouring pixels)");
  bool any = false;
  int64_t blocks = 1;
  const int64_t chunks = ((int64_t)h * w * c + 2 * AUG_CHUNK - 2) / AUG_CHUNK;          // the first chunk may start up to 15 bytes before the image
  for (int i = 0; i < n; ++i) {
    const gims_aug_plan& p = plans[i];
    GIMS_CHECK_ARG(p.ksize == 0 || p.ksize == 3 || p.ksize == 5 || p.ksize == 7, "gims_color_aug: plan %d has ksize %d (0, 3, 5 or 7)", i, p.ksize);
    const bool noise = p.sigma > 0.f;
    GIMS_CHECK_ARG(!(noise && p.ksize), "gims_color_aug: plan %d has both blur and noise", i);
    GIMS_CHECK_ARG(!noise || isfinite(p.sigma), "gims_color_aug: plan %d has a sigma that is not finite", i);
    any = any || p.use_lut || p.ksize || noise;
    const int64_t need = p.ksize ? (int64_t)cdiv(w, AUG_TW) * cdiv(h, AUG_TH) : (int64_t)cdiv(chunks, 256);
    blocks = need > blocks ? need : blocks;
  }
  hipStream_t s = (hipStream_t)stream;
  if (!any) {                                                                           // nothing to apply: a copy
    GIMS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
    return GIMS_OK;
  }
  GIMS_CHECK_ARG(work && ((uintptr_t)work & 15) == 0 && work_bytes >= gims_color_aug_workspace_bytes(n),
                 "gims_color_aug: the workspace is missing, misaligned or smaller than gims_color_aug_workspace_bytes");
  GIMS_CHECK_ARG(blocks <= 0x7fffffff, "gims_color_aug: image too large");
  const int rc = upload_table(plans, sizeof(gims_aug_plan) * (size_t)n, work, s);
  if (rc != GIMS_OK) return rc;
  hipLaunchKernelGGL(color_aug_kernel, dim3((unsigned)blocks, n), dim3(256), 0, s, src, h, w, c, (const gims_aug_plan*)work, dst);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}
