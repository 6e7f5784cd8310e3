// Per-pair evaluation that follows the matcher in the reference's eval loop:
//   GT matching  -- torch_find_matches (utils/preprocess_utils.py:98-132): iterated mutual nearest neighbours between the
//                   warped keypoints of image 0 and the keypoints of image 1, accepted below dist_thresh;
//   precision / recall (eval_homography.py:207-209, 222-226);
//   homography through the four most confident matches (eval_homography.py:216-217, cv2.getPerspectiveTransform);
//   RANSAC homography over all matches (eval_homography.py:193, 218, cv2.findHomography) -- this build's own, fully
//   specified RANSAC (specification in include/gims_hip.h), OpenCV's is not reproducible from outside;
//   corner error against the ground-truth homography (eval_homography.py:210, 219-223; common.py:477-481).
// Everything is batched over pairs (blockIdx.y) and stays on the device: the records feed the statistics all-gather.
//
// Arithmetic that decides index sets follows the reference's float32 operation order exactly: the warp is the fma chain
// torch's CPU matmul produces (fma(h2, 1, fma(h1, y, h0 * x)), verified bit-exact against the reference's output), the
// distance is sqrt(dx*dx + dy*dy) with every operation rounded separately (no contraction), argmin keeps the first minimum.
// The homography estimation runs in float64.
#include "common.h"
#include "eval_geom.h"

#include <string.h>

#include <vector>

namespace gims {

struct EvalDev {
  const float* kp0; const float* kp1; const int64_t* matches0; const float* mscores0;
  int n0, n1, height, width;
  float hgt[9];
  int32_t* gt0; uint8_t* inlier; float* record; float* hom;
  // workspace
  float* proj; int32_t* alive0; int32_t* alive1; int32_t* min1; int32_t* min2; int32_t* gt1; int32_t* midx; int32_t* hypcount;
  int32_t* nvalid;     // [1] number of valid matches (set by the counts kernel)
};

__device__ __forceinline__ float ref_dist(float ax, float ay, float bx, float by) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by);
  return __fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
}

// ---------------------------------------------------------------------------------------------- GT matching
__global__ __launch_bounds__(256) void eval_warp_kernel(const EvalDev* __restrict__ ev) {
  const EvalDev& e = ev[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < e.n0) {
    const float x = e.kp0[2 * i], y = e.kp0[2 * i + 1];
    const float X = fmaf(e.hgt[2], 1.f, fmaf(e.hgt[1], y, __fmul_rn(e.hgt[0], x)));
    const float Y = fmaf(e.hgt[5], 1.f, fmaf(e.hgt[4], y, __fmul_rn(e.hgt[3], x)));
    const float W = fmaf(e.hgt[8], 1.f, fmaf(e.hgt[7], y, __fmul_rn(e.hgt[6], x)));
    e.proj[2 * i] = __fdiv_rn(X, W);
    e.proj[2 * i + 1] = __fdiv_rn(Y, W);
    e.alive0[i] = 1;
    e.gt0[i] = -1;
    e.inlier[i] = 0;
  }
  if (i < e.n1) { e.alive1[i] = 1; e.gt1[i] = -1; }
}

// one wave per alive point of A: nearest alive point of B (first minimum).  ROWS: A = proj0, B = kp1 (min1); else A = kp1, B = proj0
template <bool ROWS>
__global__ __launch_bounds__(256) void eval_argmin_kernel(const EvalDev* __restrict__ ev) {
  const EvalDev& e = ev[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int a = blockIdx.x * 4 + wave;
  const int na = ROWS ? e.n0 : e.n1, nb = ROWS ? e.n1 : e.n0;
  if (a >= na) return;
  const int32_t* alive_a = ROWS ? e.alive0 : e.alive1;
  const int32_t* alive_b = ROWS ? e.alive1 : e.alive0;
  int32_t* out = ROWS ? e.min1 : e.min2;
  if (!alive_a[a]) { if (lane == 0) out[a] = -1; return; }
  const float* pa = ROWS ? e.proj : e.kp1;
  const float* pb = ROWS ? e.kp1 : e.proj;
  const float ax = pa[2 * a], ay = pa[2 * a + 1];
  float bd = INFINITY;
  int bj = 0x7fffffff;
  for (int j = lane; j < nb; j += 64) {
    if (!alive_b[j]) continue;
    // the reference always forms (projected keypoint of image 0) - (keypoint of image 1)
    const float d = ROWS ? ref_dist(ax, ay, pb[2 * j], pb[2 * j + 1]) : ref_dist(pb[2 * j], pb[2 * j + 1], ax, ay);
    if (d < bd) { bd = d; bj = j; }                      // ascending j: the first minimum stays
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float od = __shfl_xor(bd, o, 64);
    const int oj = __shfl_xor(bj, o, 64);
    if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
  }
  if (lane == 0) out[a] = bj == 0x7fffffff ? -1 : bj;
}

__global__ __launch_bounds__(256) void eval_mutual_kernel(const EvalDev* __restrict__ ev, float dist_thresh) {
  const EvalDev& e = ev[blockIdx.y];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= e.n1 || !e.alive1[j]) return;
  const int i = e.min2[j];
  if (i < 0 || e.min1[i] != j) return;
  if (ref_dist(e.proj[2 * i], e.proj[2 * i + 1], e.kp1[2 * j], e.kp1[2 * j + 1]) < dist_thresh) {
    e.gt0[i] = j;
    e.gt1[j] = i;
    e.alive0[i] = 0;      // i is paired with exactly one j (mutual), so no two threads write the same slot
    e.alive1[j] = 0;
  }
}

// record layout (float[16])
enum { EV_NVALID = 0, EV_NGT = 1, EV_NCORRECT = 2, EV_NFN = 3, EV_PRECISION = 4, EV_RECALL = 5, EV_NINLIERS = 6, EV_ERR_DLT = 7,
       EV_ERR_RANSAC = 8, EV_DLT_OK = 9, EV_RANSAC_OK = 10 };

// ---------------------------------------------------------------------------------------------- counts, compaction, DLT
// one workgroup per pair: precision / recall counters, ascending list of valid matches, four most confident, H_dlt
__global__ __launch_bounds__(1024) void eval_counts_kernel(const EvalDev* __restrict__ ev) {
  __shared__ int s_cnt[3];
  __shared__ int s_scan[1024];
  __shared__ float s_bv[16][4];
  __shared__ int s_bi[16][4];
  const EvalDev& e = ev[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t < 3) s_cnt[t] = 0;
  __syncthreads();
  int n_gt = 0, n_corr = 0, n_fn = 0;
  for (int i = t; i < e.n0; i += 1024) {
    const int64_t m = e.matches0[i];
    const int g = e.gt0[i];
    n_gt += g >= 0;
    n_corr += g >= 0 && m == (int64_t)g;
    n_fn += m == -1 && g != -1;
  }
  atomicAdd(&s_cnt[0], n_gt);
  atomicAdd(&s_cnt[1], n_corr);
  atomicAdd(&s_cnt[2], n_fn);
  // ordered compaction of the valid matches (chunks of 1024 keypoints, inclusive scan in LDS)
  int base = 0;
  for (int c0 = 0; c0 < e.n0; c0 += 1024) {
    const int i = c0 + t;
    const int v = i < e.n0 && e.matches0[i] > -1 ? 1 : 0;
    s_scan[t] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const int add = t >= o ? s_scan[t - o] : 0;
      __syncthreads();
      s_scan[t] += add;
      __syncthreads();
    }
    if (v) e.midx[base + s_scan[t] - 1] = i;
    base += s_scan[1023];
    __syncthreads();
  }
  const int K = base;
  // four most confident valid matches; ties -> the earlier match
  float bv[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int bi[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
  auto push = [&](float v, int p) {
    if (p == 0x7fffffff) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (v > bv[q] || (v == bv[q] && p < bi[q])) {
        const float tv = bv[q]; const int tp = bi[q];
        bv[q] = v; bi[q] = p; v = tv; p = tp;
      }
    }
  };
  __syncthreads();                                     // midx complete
  for (int p = t; p < K; p += 1024) push(e.mscores0[e.midx[p]], p);
  for (int o = 32; o > 0; o >>= 1) {                   // merge the top-4 lists across the wave
    float ov[4]; int oi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { ov[q] = __shfl_xor(bv[q], o, 64); oi[q] = __shfl_xor(bi[q], o, 64); }
#pragma unroll
    for (int q = 0; q < 4; ++q) push(ov[q], oi[q]);
  }
  if (lane == 0)
    for (int q = 0; q < 4; ++q) { s_bv[wave][q] = bv[q]; s_bi[wave][q] = bi[q]; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 16; ++w)
      for (int q = 0; q < 4; ++q) push(s_bv[w][q], s_bi[w][q]);
    const float nv = (float)K, ncorr = (float)s_cnt[1], nfn = (float)s_cnt[2];
    e.nvalid[0] = K;
    e.record[EV_NVALID] = nv;
    e.record[EV_NGT] = (float)s_cnt[0];
    e.record[EV_NCORRECT] = ncorr;
    e.record[EV_NFN] = nfn;
    e.record[EV_PRECISION] = (float)((double)s_cnt[1] / (double)K);                       // 0/0 -> NaN, like NumPy
    e.record[EV_RECALL] = (float)((double)s_cnt[1] / ((double)s_cnt[1] + (double)s_cnt[2]));
    double H[9];
    bool ok = K >= 4;
    if (ok) {
      const int idx[4] = {bi[0], bi[1], bi[2], bi[3]};
      ok = homography4(e.kp0, e.kp1, idx, e.midx, e.matches0, H);
    }
    e.record[EV_DLT_OK] = ok ? 1.f : 0.f;
    e.record[EV_ERR_DLT] = ok ? corner_error(H, e.hgt, e.height, e.width) : -1.f;
    for (int c = 0; c < 9; ++c) e.hom[c] = ok ? (float)H[c] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------- RANSAC
// one wave per hypothesis: 4-point model (all lanes solve it redundantly: no divergence), inliers counted across the lanes
__global__ __launch_bounds__(256) void eval_ransac_kernel(const EvalDev* __restrict__ ev, uint64_t seed, int iters, double t2) {
  const EvalDev& e = ev[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int hyp = blockIdx.x * 4 + wave;
  const int K = e.nvalid[0];
  if (hyp >= iters) return;
  int cnt = -1;
  if (K >= 4) {
    int idx[4];
    ransac_sample(seed, hyp, K, idx);
    double H[9];
    if (homography4(e.kp0, e.kp1, idx, e.midx, e.matches0, H)) {
      cnt = 0;
      for (int p = lane; p < K; p += 64) {
        const int i = e.midx[p];
        const int j = (int)e.matches0[i];
        cnt += reproj2(H, e.kp0[2 * i], e.kp0[2 * i + 1], e.kp1[2 * j], e.kp1[2 * j + 1]) <= t2;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    }
  }
  if (lane == 0) e.hypcount[hyp] = cnt;
}

// one workgroup per pair: best hypothesis (most inliers, first such), least-squares refit on its inliers, final mask
__global__ __launch_bounds__(1024) void eval_ransac_finish_kernel(const EvalDev* __restrict__ ev, uint64_t seed, int iters, double t2) {
  __shared__ int s_best[16][2];
  __shared__ double s_H[9];
  __shared__ double s_acc[16][44];
  __shared__ int s_ok, s_cnt;
  const EvalDev& e = ev[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int K = e.nvalid[0];
  int bc = -1, bh = 0x7fffffff;
  for (int h = t; h < iters; h += 1024) {
    const int c = e.hypcount[h];
    if (c > bc) { bc = c; bh = h; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int oc = __shfl_xor(bc, o, 64), oh = __shfl_xor(bh, o, 64);
    if (oc > bc || (oc == bc && oh < bh)) { bc = oc; bh = oh; }
  }
  if (lane == 0) { s_best[wave][0] = bc; s_best[wave][1] = bh; }
  if (t == 0) { s_ok = 0; s_cnt = 0; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 16; ++w)
      if (s_best[w][0] > bc || (s_best[w][0] == bc && s_best[w][1] < bh)) { bc = s_best[w][0]; bh = s_best[w][1]; }
    if (bc >= 0 && K >= 4) {
      int idx[4];
      ransac_sample(seed, bh, K, idx);
      double H[9];
      if (homography4(e.kp0, e.kp1, idx, e.midx, e.matches0, H)) {
        for (int c = 0; c < 9; ++c) s_H[c] = H[c];
        s_ok = 1;
      }
    }
  }
  __syncthreads();
  if (!s_ok) {
    if (t == 0) {
      e.record[EV_RANSAC_OK] = 0.f; e.record[EV_NINLIERS] = 0.f; e.record[EV_ERR_RANSAC] = -1.f;
      for (int c = 0; c < 9; ++c) e.hom[9 + c] = 0.f;
    }
    return;
  }
  double H[9];
  for (int c = 0; c < 9; ++c) H[c] = s_H[c];
  // normal equations of the 2K x 8 system over the inliers of the best hypothesis: 36 entries of A^T A (upper) + 8 of A^T b
  double acc[44];
  for (int c = 0; c < 44; ++c) acc[c] = 0.0;
  int nin = 0;
  for (int p = t; p < K; p += 1024) {
    const int i = e.midx[p];
    const int j = (int)e.matches0[i];
    const double x = e.kp0[2 * i], y = e.kp0[2 * i + 1], u = e.kp1[2 * j], v = e.kp1[2 * j + 1];
    if (reproj2(H, x, y, u, v) <= t2) {
      ++nin;
      const double r0[8] = {x, y, 1, 0, 0, 0, -u * x, -u * y}, r1[8] = {0, 0, 0, x, y, 1, -v * x, -v * y};
      int q = 0;
      for (int a = 0; a < 8; ++a)
        for (int b = a; b < 8; ++b) acc[q++] += r0[a] * r0[b] + r1[a] * r1[b];
      for (int a = 0; a < 8; ++a) acc[36 + a] += r0[a] * u + r1[a] * v;
    }
  }
  for (int c = 0; c < 44; ++c) {
    double s = acc[c];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) s_acc[wave][c] = s;
  }
  atomicAdd(&s_cnt, nin);
  __syncthreads();
  if (t == 0) {
    if (s_cnt >= 4) {
      double A[8][9];
      int q = 0;
      for (int a = 0; a < 8; ++a)
        for (int b = a; b < 8; ++b) {
          double s = 0.0;
          for (int w = 0; w < 16; ++w) s += s_acc[w][q];
          A[a][b] = s; A[b][a] = s;
          ++q;
        }
      for (int a = 0; a < 8; ++a) {
        double s = 0.0;
        for (int w = 0; w < 16; ++w) s += s_acc[w][36 + a];
        A[a][8] = s;
      }
      if (solve8(A)) {
        bool fin = true;
        for (int c = 0; c < 8; ++c) fin = fin && isfinite(A[c][8]);
        if (fin) {
          for (int c = 0; c < 8; ++c) s_H[c] = A[c][8];
          s_H[8] = 1.0;
        }
      }
    }
    s_cnt = 0;
  }
  __syncthreads();
  for (int c = 0; c < 9; ++c) H[c] = s_H[c];
  nin = 0;
  for (int p = t; p < K; p += 1024) {
    const int i = e.midx[p];
    const int j = (int)e.matches0[i];
    const bool in = reproj2(H, e.kp0[2 * i], e.kp0[2 * i + 1], e.kp1[2 * j], e.kp1[2 * j + 1]) <= t2;
    e.inlier[i] = in ? 1 : 0;
    nin += in;
  }
  atomicAdd(&s_cnt, nin);
  __syncthreads();
  if (t == 0) {
    e.record[EV_RANSAC_OK] = 1.f;
    e.record[EV_NINLIERS] = (float)s_cnt;
    e.record[EV_ERR_RANSAC] = corner_error(H, e.hgt, e.height, e.width);
    for (int c = 0; c < 9; ++c) e.hom[9 + c] = (float)H[c];
  }
}

// The workspace of gims_eval_pairs: the EvalDev table, then per pair the GT-matching arrays and the RANSAC counters.  recs == nullptr: sizing only.
static void eval_layout(const gims_eval_pair* pairs, int n_pairs, int ransac_iters, WsLayout& L, EvalDev* recs) {
  L.take<EvalDev>(n_pairs);
  for (int i = 0; i < n_pairs; ++i) {
    const gims_eval_pair& p = pairs[i];
    EvalDev d;
    memset(&d, 0, sizeof(d));
    d.proj = L.take<float>((size_t)p.n0 * 2);
    d.alive0 = L.take<int32_t>(p.n0);
    d.min1 = L.take<int32_t>(p.n0);
    d.midx = L.take<int32_t>(p.n0);
    L.take<int32_t>(p.n0); L.take<int32_t>(p.n0);      // reserved: two n0 arrays no kernel uses (kept so that the size query is unchanged)
    d.alive1 = L.take<int32_t>(p.n1);
    d.min2 = L.take<int32_t>(p.n1);
    d.gt1 = L.take<int32_t>(p.n1);
    d.hypcount = L.take<int32_t>(ransac_iters);
    d.nvalid = L.take<int32_t>(64);
    if (!recs) continue;
    d.kp0 = p.kpts0; d.kp1 = p.kpts1; d.matches0 = p.matches0; d.mscores0 = p.mscores0;
    d.n0 = p.n0; d.n1 = p.n1; d.height = p.height; d.width = p.width;
    memcpy(d.hgt, p.h_gt, sizeof(d.hgt));
    d.gt0 = p.gt0; d.inlier = p.inlier; d.record = p.record; d.hom = p.homographies;
    recs[i] = d;
  }
}

// The GT-matching launches shared with gims_train_labels (defined below, behind the label kernels)
static void eval_gt_matching(const EvalDev* dev, int n_pairs, int maxn0, int maxn1, float dist_thresh, int n_iters, int32_t* const* itr, hipStream_t s);

}  // namespace gims

extern "C" size_t gims_eval_workspace_bytes(const gims_eval_pair* pairs, int32_t n_pairs, int32_t ransac_iters) {
  using namespace gims;
  if (!pairs || n_pairs <= 0 || ransac_iters < 0) return 0;
  WsLayout L(nullptr);
  eval_layout(pairs, n_pairs, ransac_iters, L, nullptr);
  return L.bytes();
}

extern "C" int gims_eval_pairs(const gims_eval_pair* pairs, int32_t n_pairs, float dist_thresh, int32_t n_iters, float ransac_thresh,
                               int32_t ransac_iters, uint64_t seed, void* work, size_t work_bytes, void* stream) {
  using namespace gims;
  GIMS_CHECK_ARG(pairs && n_pairs > 0 && work, "gims_eval_pairs: null / empty arguments");
  GIMS_CHECK_ARG(n_iters >= 0 && ransac_iters >= 0 && ransac_iters <= (1 << 20), "gims_eval_pairs: bad iteration counts");
  int maxn0 = 0, maxn1 = 0;
  for (int i = 0; i < n_pairs; ++i) {
    const gims_eval_pair& p = pairs[i];
    GIMS_CHECK_ARG(p.n0 > 0 && p.n1 > 0 && p.kpts0 && p.kpts1 && p.matches0 && p.mscores0 && p.gt0 && p.inlier && p.record && p.homographies,
                   "gims_eval_pairs: pair %d has an empty shape or a null pointer", i);
    maxn0 = p.n0 > maxn0 ? p.n0 : maxn0;
    maxn1 = p.n1 > maxn1 ? p.n1 : maxn1;
  }
  std::vector<EvalDev> h(n_pairs);
  WsLayout L(work);
  eval_layout(pairs, n_pairs, ransac_iters, L, h.data());
  GIMS_CHECK_ARG(work_bytes >= L.bytes(), "gims_eval_pairs: workspace too small (%zu < %zu)", work_bytes, L.bytes());
  hipStream_t s = (hipStream_t)stream;
  int rc = upload_table(h.data(), sizeof(EvalDev) * (size_t)n_pairs, work, s);
  if (rc != GIMS_OK) return rc;
  const EvalDev* dev = (const EvalDev*)work;
  eval_gt_matching(dev, n_pairs, maxn0, maxn1, dist_thresh, n_iters, nullptr, s);
  hipLaunchKernelGGL(eval_counts_kernel, dim3(n_pairs), dim3(1024), 0, s, dev);
  const double t2 = (double)ransac_thresh * (double)ransac_thresh;
  if (ransac_iters > 0) hipLaunchKernelGGL(eval_ransac_kernel, dim3(cdiv(ransac_iters, 4), n_pairs), dim3(256), 0, s, dev, seed, ransac_iters, t2);
  hipLaunchKernelGGL(eval_ransac_finish_kernel, dim3(n_pairs), dim3(1024), 0, s, dev, seed, ransac_iters, t2);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

// ---------------------------------------------------------------------------------------------- training labels
// torch_find_matches (utils/preprocess_utils.py:98-132) through the GT-matching kernels above, then the match_indexes rows of
// train.py:118-125: [k, i0, i1] for the matches (i1 ascending, iteration after iteration), [k, miss0, -1], [k, -1, miss1], pair
// after pair.  The homographies are read on the device; the row count is the caller's one host read.
namespace gims {

// the ground-truth homography of each pair from device memory into the descriptor table
__global__ __launch_bounds__(64) void lab_setup_kernel(EvalDev* __restrict__ ev, const float* __restrict__ hs, int32_t* __restrict__ itr_all,
                                                       int64_t n1_total) {
  const int p = blockIdx.x, t = threadIdx.x;
  if (t < 9) ev[p].hgt[t] = hs[9 * p + t];
  for (int64_t j = (int64_t)p * 64 + t; j < n1_total; j += (int64_t)gridDim.x * 64) itr_all[j] = -1;
}

// the iteration in which keypoint j of image 1 found its partner
__global__ __launch_bounds__(256) void lab_iter_kernel(const EvalDev* __restrict__ ev, int32_t* const* __restrict__ itr, int it) {
  const EvalDev& e = ev[blockIdx.y];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < e.n1 && e.gt1[j] >= 0 && itr[blockIdx.y][j] < 0) itr[blockIdx.y][j] = it;
}

// exclusive prefix of a 0/1 flag over the 1024 threads of the block; *total receives the block's count
__device__ __forceinline__ int block_prefix(bool flag, int* s_wave, int& total) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned long long bal = __ballot(flag);
  const int below = __popcll(bal & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) s_wave[wave] = __popcll(bal);
  __syncthreads();
  int before = 0;
  total = 0;
  for (int w = 0; w < 16; ++w) {
    before += w < wave ? s_wave[w] : 0;
    total += s_wave[w];
  }
  return before + below;
}

// pass 0: rows per pair = n0 + n1 - matches (one workgroup per pair); pass 1: ordered compaction into rows at the pair's offset
template <int PASS>
__global__ __launch_bounds__(1024) void lab_rows_kernel(const EvalDev* __restrict__ ev, int32_t* const* __restrict__ itr, int n_iters,
                                                        int32_t* __restrict__ counts, int64_t* __restrict__ rows, int64_t* __restrict__ total) {
  __shared__ int s_wave[16];
  __shared__ int s_red;
  const int p = blockIdx.x, t = threadIdx.x;
  const EvalDev& e = ev[p];
  if (PASS == 0) {
    if (t == 0) s_red = 0;
    __syncthreads();
    int m = 0;
    for (int j = t; j < e.n1; j += 1024) m += e.gt1[j] >= 0;
    atomicAdd(&s_red, m);
    __syncthreads();
    if (t == 0) counts[p] = e.n0 + e.n1 - s_red;
    return;
  }
  int64_t off = 0;
  for (int q = 0; q < p; ++q) off += counts[q];
  if (p == (int)gridDim.x - 1 && t == 0) total[0] = off + counts[p];
  const int32_t* it_of = itr[p];
  int cnt;
  for (int it = 0; it < n_iters; ++it)
    for (int j0 = 0; j0 < e.n1; j0 += 1024) {
      const int j = j0 + t;
      const bool f = j < e.n1 && it_of[j] == it;
      const int pos = block_prefix(f, s_wave, cnt);
      if (f) { int64_t* r = rows + 3 * (off + pos); r[0] = p; r[1] = e.gt1[j]; r[2] = j; }
      off += cnt;
    }
  for (int i0 = 0; i0 < e.n0; i0 += 1024) {
    const int i = i0 + t;
    const bool f = i < e.n0 && e.alive0[i];
    const int pos = block_prefix(f, s_wave, cnt);
    if (f) { int64_t* r = rows + 3 * (off + pos); r[0] = p; r[1] = i; r[2] = -1; }
    off += cnt;
  }
  for (int j0 = 0; j0 < e.n1; j0 += 1024) {
    const int j = j0 + t;
    const bool f = j < e.n1 && e.alive1[j];
    const int pos = block_prefix(f, s_wave, cnt);
    if (f) { int64_t* r = rows + 3 * (off + pos); r[0] = p; r[1] = -1; r[2] = j; }
    off += cnt;
  }
}

// The GT-matching launches shared by gims_eval_pairs and gims_train_labels: the warp, then n_iters rounds of the two arg-min sweeps and the
// mutual test; the labels path passes the table of its per-pair iteration arrays (itr) and gets lab_iter_kernel after every round.
static void eval_gt_matching(const EvalDev* dev, int n_pairs, int maxn0, int maxn1, float dist_thresh, int n_iters, int32_t* const* itr, hipStream_t s) {
  const int mx = maxn0 > maxn1 ? maxn0 : maxn1;
  hipLaunchKernelGGL(eval_warp_kernel, dim3(cdiv(mx, 256), n_pairs), dim3(256), 0, s, dev);
  for (int it = 0; it < n_iters; ++it) {
    hipLaunchKernelGGL(eval_argmin_kernel<true>, dim3(cdiv(maxn0, 4), n_pairs), dim3(256), 0, s, dev);
    hipLaunchKernelGGL(eval_argmin_kernel<false>, dim3(cdiv(maxn1, 4), n_pairs), dim3(256), 0, s, dev);
    hipLaunchKernelGGL(eval_mutual_kernel, dim3(cdiv(maxn1, 256), n_pairs), dim3(256), 0, s, dev, dist_thresh);
    if (itr) hipLaunchKernelGGL(lab_iter_kernel, dim3(cdiv(maxn1, 256), n_pairs), dim3(256), 0, s, dev, itr, it);
  }
}

// The workspace of gims_train_labels: the EvalDev table, the table of iteration-array pointers, the row counts, the per-pair iteration
// arrays back to back (one block: the setup kernel initialises them in one sweep), then per pair the GT-matching arrays.  recs == nullptr: sizing only.
struct LabWs { int32_t* const* ditr; int32_t* counts; int32_t* itr_all; int64_t n1_total; };
static LabWs label_layout(const gims_label_pair* pairs, int n_pairs, WsLayout& L, EvalDev* recs, int32_t** itr) {
  LabWs w{};
  L.take<EvalDev>(n_pairs);
  w.ditr = L.take<int32_t*>(n_pairs);
  w.counts = L.take<int32_t>(n_pairs);
  for (int i = 0; i < n_pairs; ++i) w.n1_total += (int64_t)(al256((size_t)pairs[i].n1 * 4) / 4);
  w.itr_all = L.take<int32_t>((size_t)w.n1_total);
  int64_t itr_off = 0;
  for (int i = 0; i < n_pairs; ++i) {
    const gims_label_pair& p = pairs[i];
    EvalDev d;
    memset(&d, 0, sizeof(d));
    d.proj = L.take<float>((size_t)p.n0 * 2);
    d.alive0 = L.take<int32_t>(p.n0);
    d.min1 = L.take<int32_t>(p.n0);
    d.gt0 = L.take<int32_t>(p.n0);
    d.inlier = L.take<uint8_t>(p.n0);
    d.alive1 = L.take<int32_t>(p.n1);
    d.min2 = L.take<int32_t>(p.n1);
    d.gt1 = L.take<int32_t>(p.n1);
    d.kp0 = p.kpts0; d.kp1 = p.kpts1; d.n0 = p.n0; d.n1 = p.n1;
    if (recs) { recs[i] = d; itr[i] = w.itr_all + itr_off; }
    itr_off += (int64_t)(al256((size_t)p.n1 * 4) / 4);
  }
  return w;
}

}  // namespace gims

extern "C" size_t gims_train_labels_workspace_bytes(const gims_label_pair* pairs, int32_t n_pairs) {
  using namespace gims;
  if (!pairs || n_pairs <= 0) return 0;
  WsLayout L(nullptr);
  label_layout(pairs, n_pairs, L, nullptr, nullptr);
  return L.bytes();
}

extern "C" int gims_train_labels(const gims_label_pair* pairs, int32_t n_pairs, const float* homographies, float dist_thresh, int32_t n_iters,
                                 int64_t* rows, int64_t* total, void* work, size_t work_bytes, void* stream) {
  using namespace gims;
  GIMS_CHECK_ARG(pairs && n_pairs > 0 && n_pairs <= 65535 && homographies && rows && total && work, "gims_train_labels: null / empty arguments");
  GIMS_CHECK_ARG(n_iters >= 0 && n_iters <= 64, "gims_train_labels: bad iteration count");
  int maxn0 = 0, maxn1 = 0;
  for (int i = 0; i < n_pairs; ++i) {
    const gims_label_pair& p = pairs[i];
    GIMS_CHECK_ARG(p.n0 > 0 && p.n1 > 0 && p.kpts0 && p.kpts1, "gims_train_labels: pair %d has an empty shape or a null pointer", i);
    maxn0 = p.n0 > maxn0 ? p.n0 : maxn0;
    maxn1 = p.n1 > maxn1 ? p.n1 : maxn1;
  }
  std::vector<EvalDev> h(n_pairs);
  std::vector<int32_t*> hitr(n_pairs);
  WsLayout L(work);
  const LabWs w = label_layout(pairs, n_pairs, L, h.data(), hitr.data());
  GIMS_CHECK_ARG(work_bytes >= L.bytes(), "gims_train_labels: workspace too small (%zu < %zu)", work_bytes, L.bytes());
  hipStream_t s = (hipStream_t)stream;
  int rc = upload_table(h.data(), sizeof(EvalDev) * (size_t)n_pairs, work, s);
  if (rc != GIMS_OK) return rc;
  rc = upload_table(hitr.data(), sizeof(int32_t*) * (size_t)n_pairs, (void*)w.ditr, s);
  if (rc != GIMS_OK) return rc;
  EvalDev* dev = (EvalDev*)work;
  hipLaunchKernelGGL(lab_setup_kernel, dim3(n_pairs), dim3(64), 0, s, dev, homographies, w.itr_all, w.n1_total);
  eval_gt_matching(dev, n_pairs, maxn0, maxn1, dist_thresh, n_iters, w.ditr, s);
  hipLaunchKernelGGL(lab_rows_kernel<0>, dim3(n_pairs), dim3(1024), 0, s, (const EvalDev*)dev, w.ditr, n_iters, w.counts, rows, total);
  hipLaunchKernelGGL(lab_rows_kernel<1>, dim3(n_pairs), dim3(1024), 0, s, (const EvalDev*)dev, w.ditr, n_iters, w.counts, rows, total);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}
