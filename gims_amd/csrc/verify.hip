// Ground-truth-free geometric verification: the RANSAC homography over a set of correspondences and its inlier mask -- what
// the reference's drivers get from cv2.findHomography(points0, points1, RANSAC | USAC_DEFAULT) (eval_homography.py:191, eval_matches.py:71,164,
// tools/parameter_search.py:161) -- as an entry point of its own, with a guarded, normalised local optimisation of the best hypothesis.
// The estimator is this build's own and fully specified in include/gims_hip.h; stage 1 and the lo_iters == 0 refit are those of
// gims_eval_pairs (csrc/eval.hip) through the helpers of eval_geom.h.  Three kernels, batched over sets, one launch each:
//   gather      one workgroup per set: ordered compaction of the correspondences into a dense float4 {x, y, u, v} array;
//   hypotheses  one workgroup per VF_HB hypotheses: VF_HB lanes solve a model each into LDS, then every thread scores one correspondence per
//               tile (one coalesced 16-byte load) against all VF_HB models (LDS broadcast reads), counters in registers;
//   finish      one workgroup per set: best hypothesis, stage 2, mask, record, corner error.
#include "common.h"
#include "eval_geom.h"

#include <math.h>
#include <string.h>

#include <vector>

namespace gims {

struct VerifyDev {
  const float* kp0; const float* kp1; const int64_t* matches0;
  int n0, n1, height, width, has_ref;
  float href[9];
  uint8_t* inlier; float* record; float* hom;
  // workspace
  float4* corr;        // [n0] dense correspondences {x, y, u, v}, ascending row
  int32_t* rows;       // [n0] the row of keypoints0 each correspondence came from
  int32_t* hypcount;   // [iters]
  int32_t* nvalid;     // [1] K (set by the gather kernel)
};

// record layout (float[8]): GIMS_VERIFY_* of include/gims_hip.h
enum { VF_NVALID = 0, VF_OK = 1, VF_NINLIERS = 2, VF_BEST_HYP = 3, VF_BEST_HYP_INLIERS = 4, VF_LO_ROUNDS = 5, VF_ERR_CORNER = 6, VF_RESERVED = 7 };

constexpr int VF_HB = 16;          // hypotheses per workgroup of the scoring kernel

// ---------------------------------------------------------------------------------------------- gather
// one workgroup per set: ascending list of the correspondences (chunks of 1024 rows, inclusive scan in LDS, as eval_counts_kernel does it);
// the mask is cleared here, so unmatched rows and sets without a model read 0
__global__ __launch_bounds__(1024) void verify_gather_kernel(const VerifyDev* __restrict__ vs) {
  __shared__ int s_scan[1024];
  const VerifyDev& e = vs[blockIdx.x];
  const int t = threadIdx.x;
  int base = 0;
  for (int c0 = 0; c0 < e.n0; c0 += 1024) {
    const int i = c0 + t;
    int64_t j = -1;
    if (i < e.n0) {
      j = e.matches0 ? e.matches0[i] : (int64_t)i;
      e.inlier[i] = 0;
    }
    const int v = j > -1 && j < (int64_t)e.n1 ? 1 : 0;       // a partner beyond keypoints1 is no correspondence (and is never read)
    s_scan[t] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const int add = t >= o ? s_scan[t - o] : 0;
      __syncthreads();
      s_scan[t] += add;
      __syncthreads();
    }
    if (v) {
      const int p = base + s_scan[t] - 1;                     // p <= i < n0
      e.corr[p] = make_float4(e.kp0[2 * i], e.kp0[2 * i + 1], e.kp1[2 * j], e.kp1[2 * j + 1]);
      e.rows[p] = i;
    }
    base += s_scan[1023];
    __syncthreads();
  }
  if (t == 0) e.nvalid[0] = base;
}

// homography4 of eval_geom.h on the dense array: the same rows, the same elimination
__device__ bool homography4_dense(const float4* __restrict__ corr, const int (&idx)[4], double (&H)[9]) {
  double A[8][9];
  for (int k = 0; k < 4; ++k) {
    const float4 c = corr[idx[k]];
    const double x = c.x, y = c.y, u = c.z, v = c.w;
    const double r0[9] = {x, y, 1, 0, 0, 0, -u * x, -u * y, u};
    const double r1[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, v};
    for (int q = 0; q < 9; ++q) { A[2 * k][q] = r0[q]; A[2 * k + 1][q] = r1[q]; }
  }
  if (!solve8(A)) return false;
  bool fin = true;
  for (int q = 0; q < 8; ++q) { H[q] = A[q][8]; fin = fin && isfinite(H[q]); }
  H[8] = 1.0;
  return fin;
}

// ---------------------------------------------------------------------------------------------- hypotheses
// one workgroup per VF_HB hypotheses of one set.  The first VF_HB lanes solve one model each (their elimination array is indexed by the
// pivot search and lives in scratch); the scoring loop keeps VF_HB counters in registers and reads the models at wave-uniform LDS addresses.
__global__ __launch_bounds__(256) void verify_hyp_kernel(const VerifyDev* __restrict__ vs, uint64_t seed, int iters, double t2) {
  __shared__ double s_H[VF_HB][10];
  __shared__ int s_ok[VF_HB];
  __shared__ int s_cnt[4][VF_HB];
  const VerifyDev& e = vs[blockIdx.y];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int K = e.nvalid[0];
  const int h0 = blockIdx.x * VF_HB;
  if (K < 4) {                                             // the same for every thread of the workgroup
    if (t < VF_HB && h0 + t < iters) e.hypcount[h0 + t] = -1;
    return;
  }
  if (t < VF_HB) {
    double H[9];
    bool ok = false;
    if (h0 + t < iters) {
      int idx[4];
      ransac_sample(seed, h0 + t, K, idx);
      ok = homography4_dense(e.corr, idx, H);
    }
    for (int c = 0; c < 9; ++c) s_H[t][c] = ok ? H[c] : 0.0;
    s_ok[t] = ok ? 1 : 0;
  }
  __syncthreads();
  int cnt[VF_HB];
#pragma unroll
  for (int b = 0; b < VF_HB; ++b) cnt[b] = 0;
  for (int p0 = 0; p0 < K; p0 += 256) {                  // K is the same for the whole workgroup
    const int p = p0 + t;
    const bool have = p < K;
    const float4 c = e.corr[have ? p : 0];
    const double x = c.x, y = c.y, u = c.z, v = c.w;
#pragma unroll
    for (int b = 0; b < VF_HB; ++b) {
      double H[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) H[q] = s_H[b][q];
      cnt[b] += have && reproj2(H, x, y, u, v) <= t2 ? 1 : 0;
    }
    // the models are read from LDS again for every tile (wave-uniform addresses: broadcasts).  Without this barrier the compiler hoists
    // all VF_HB models out of the loop, 288 registers, and the kernel runs at one wave per SIMD or spills
    __syncthreads();
  }
#pragma unroll
  for (int b = 0; b < VF_HB; ++b) {
    int s = cnt[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) s_cnt[wave][b] = s;
  }
  __syncthreads();
  if (t < VF_HB && h0 + t < iters)
    e.hypcount[h0 + t] = s_ok[t] ? s_cnt[0][t] + s_cnt[1][t] + s_cnt[2][t] + s_cnt[3][t] : -1;
}

// ---------------------------------------------------------------------------------------------- finish
// the per-thread sums of a sweep over the correspondences, reduced across each wave into one LDS row per wave; after the caller's barrier
// thread 0 adds the 16 rows in wave order (vf_total)
template <int N>
__device__ __forceinline__ void vf_partials(const double (&acc)[N], double (*s_acc)[44]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = 0; c < N; ++c) {
    double s = acc[c];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) s_acc[wave][c] = s;
  }
}
__device__ __forceinline__ double vf_total(const double (*s_acc)[44], int c) {
  double s = 0.0;
  for (int w = 0; w < 16; ++w) s += s_acc[w][c];
  return s;
}
// the 36 + 8 entries of the normal equations of the 2K x 8 system that one correspondence adds (as eval_ransac_finish_kernel forms them)
__device__ __forceinline__ void vf_normal_add(double (&acc)[44], double x, double y, double u, double v) {
  const double r0[8] = {x, y, 1, 0, 0, 0, -u * x, -u * y}, r1[8] = {0, 0, 0, x, y, 1, -v * x, -v * y};
  int q = 0;
  for (int a = 0; a < 8; ++a)
    for (int b = a; b < 8; ++b) acc[q++] += r0[a] * r0[b] + r1[a] * r1[b];
  for (int a = 0; a < 8; ++a) acc[36 + a] += r0[a] * u + r1[a] * v;
}
// thread 0: the reduced normal equations -> solve8; true and h[0..7] when the solve succeeds with finite entries
__device__ bool vf_normal_solve(const double (*s_acc)[44], double (&h)[8]) {
  double A[8][9];
  int q = 0;
  for (int a = 0; a < 8; ++a)
    for (int b = a; b < 8; ++b) {
      const double s = vf_total(s_acc, q);
      A[a][b] = s; A[b][a] = s;
      ++q;
    }
  for (int a = 0; a < 8; ++a) A[a][8] = vf_total(s_acc, 36 + a);
  if (!solve8(A)) return false;
  bool fin = true;
  for (int c = 0; c < 8; ++c) { h[c] = A[c][8]; fin = fin && isfinite(h[c]); }
  return fin;
}

// one workgroup per set: best hypothesis (most inliers, first such), stage 2, final mask, record.  Every decision of stage 2 is taken by
// thread 0, stored in LDS and read by all threads after the barrier that follows; the next store to the same word comes after a later
// barrier.  No barrier sits under a condition that is not one of those words, a kernel argument or a per-set constant.
__global__ __launch_bounds__(1024) void verify_finish_kernel(const VerifyDev* __restrict__ vs, uint64_t seed, int iters, int lo_iters, double t2) {
  __shared__ int s_best[16][2];
  __shared__ double s_H[9];          // the accepted model
  __shared__ double s_Hn[9];         // the candidate of the current round
  __shared__ double s_norm[6];       // cx, cy, cu, cv, scale0, scale1
  __shared__ double s_acc[16][44];
  __shared__ double s_nprev;         // |I_{l-1}|
  __shared__ int s_ok, s_stop, s_rounds, s_bc, s_bh, s_cnt;
  const VerifyDev& e = vs[blockIdx.x];
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
  if (t == 0) { s_ok = 0; s_stop = 0; s_rounds = 0; s_cnt = 0; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 16; ++w)
      if (s_best[w][0] > bc || (s_best[w][0] == bc && s_best[w][1] < bh)) { bc = s_best[w][0]; bh = s_best[w][1]; }
    if (bc >= 0 && K >= 4) {
      int idx[4];
      ransac_sample(seed, bh, K, idx);
      double H[9];
      if (homography4_dense(e.corr, idx, H)) {
        for (int c = 0; c < 9; ++c) s_H[c] = H[c];
        s_ok = 1; s_bc = bc; s_bh = bh;
      }
    }
  }
  __syncthreads();
  if (!s_ok) {
    if (t == 0) {
      for (int c = 0; c < 8; ++c) e.record[c] = 0.f;
      e.record[VF_NVALID] = (float)K;
      e.record[VF_ERR_CORNER] = -1.f;
      for (int c = 0; c < 9; ++c) e.hom[c] = 0.f;
    }
    return;
  }
  double H[9];
  for (int c = 0; c < 9; ++c) H[c] = s_H[c];
  if (lo_iters == 0) {
    // the single unguarded refit of gims_eval_pairs: normal equations over the inliers of the best hypothesis, raw coordinates
    double acc[44];
    for (int c = 0; c < 44; ++c) acc[c] = 0.0;
    int nin = 0;
    for (int p = t; p < K; p += 1024) {
      const float4 c4 = e.corr[p];
      const double x = c4.x, y = c4.y, u = c4.z, v = c4.w;
      if (reproj2(H, x, y, u, v) <= t2) {
        ++nin;
        vf_normal_add(acc, x, y, u, v);
      }
    }
    vf_partials(acc, s_acc);
    atomicAdd(&s_cnt, nin);
    __syncthreads();
    if (t == 0) {
      double h[8];
      if (s_cnt >= 4 && vf_normal_solve(s_acc, h)) {
        for (int c = 0; c < 8; ++c) s_H[c] = h[c];
        s_H[8] = 1.0;
      }
    }
    __syncthreads();
  } else {
    {  // |I_0|
      double a[1] = {0.0};
      for (int p = t; p < K; p += 1024) {
        const float4 c4 = e.corr[p];
        a[0] += reproj2(H, c4.x, c4.y, c4.z, c4.w) <= t2 ? 1.0 : 0.0;
      }
      vf_partials(a, s_acc);
      __syncthreads();
      if (t == 0) s_nprev = vf_total(s_acc, 0);
      __syncthreads();
    }
    for (int l = 1; l <= lo_iters; ++l) {
      // (a) centroids of the inliers of the accepted model
      {
        double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int p = t; p < K; p += 1024) {
          const float4 c4 = e.corr[p];
          const double x = c4.x, y = c4.y, u = c4.z, v = c4.w;
          if (reproj2(H, x, y, u, v) <= t2) { a[0] += 1.0; a[1] += x; a[2] += y; a[3] += u; a[4] += v; }
        }
        vf_partials(a, s_acc);
      }
      __syncthreads();
      if (t == 0) {
        const double n = vf_total(s_acc, 0);
        s_stop = n < 4.0 ? 1 : 0;
        if (n >= 4.0)
          for (int c = 0; c < 4; ++c) s_norm[c] = vf_total(s_acc, 1 + c) / n;
      }
      __syncthreads();
      if (s_stop) break;
      const double cx = s_norm[0], cy = s_norm[1], cu = s_norm[2], cv = s_norm[3];
      // (b) mean distances to the centroids
      {
        double a[3] = {0.0, 0.0, 0.0};
        for (int p = t; p < K; p += 1024) {
          const float4 c4 = e.corr[p];
          const double x = c4.x, y = c4.y, u = c4.z, v = c4.w;
          if (reproj2(H, x, y, u, v) <= t2) {
            a[0] += 1.0;
            a[1] += sqrt((x - cx) * (x - cx) + (y - cy) * (y - cy));
            a[2] += sqrt((u - cu) * (u - cu) + (v - cv) * (v - cv));
          }
        }
        vf_partials(a, s_acc);
      }
      __syncthreads();
      if (t == 0) {
        const double n = vf_total(s_acc, 0), m0 = vf_total(s_acc, 1) / n, m1 = vf_total(s_acc, 2) / n;
        s_norm[4] = m0 == 0.0 ? 1.0 : sqrt(2.0) / m0;
        s_norm[5] = m1 == 0.0 ? 1.0 : sqrt(2.0) / m1;
      }
      __syncthreads();
      const double sc0 = s_norm[4], sc1 = s_norm[5];
      // (c) normal equations over the normalised inliers, solve, back to pixel coordinates
      {
        double acc[44];
        for (int c = 0; c < 44; ++c) acc[c] = 0.0;
        for (int p = t; p < K; p += 1024) {
          const float4 c4 = e.corr[p];
          const double x = c4.x, y = c4.y, u = c4.z, v = c4.w;
          if (reproj2(H, x, y, u, v) <= t2) vf_normal_add(acc, (x - cx) * sc0, (y - cy) * sc0, (u - cu) * sc1, (v - cv) * sc1);
        }
        vf_partials(acc, s_acc);
      }
      __syncthreads();
      if (t == 0) {
        double h[8];
        bool ok = vf_normal_solve(s_acc, h);
        if (ok) {
          const double Hn[9] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], 1.0};
          double M[9], Hd[9];
          for (int r = 0; r < 3; ++r) {                   // M = Hn T0
            M[3 * r] = Hn[3 * r] * sc0;
            M[3 * r + 1] = Hn[3 * r + 1] * sc0;
            M[3 * r + 2] = Hn[3 * r + 2] - sc0 * (Hn[3 * r] * cx + Hn[3 * r + 1] * cy);
          }
          for (int c = 0; c < 3; ++c) {                   // H' = T1^-1 M
            Hd[c] = M[c] / sc1 + cu * M[6 + c];
            Hd[3 + c] = M[3 + c] / sc1 + cv * M[6 + c];
            Hd[6 + c] = M[6 + c];
          }
          const double w = Hd[8];
          ok = w != 0.0 && isfinite(w);
          if (ok) {
            for (int c = 0; c < 9; ++c) { Hd[c] = Hd[c] / w; ok = ok && isfinite(Hd[c]); }
            for (int c = 0; c < 9; ++c) s_Hn[c] = Hd[c];
          }
        }
        s_stop = ok ? 0 : 1;
      }
      __syncthreads();
      if (s_stop) break;
      double Hc[9];
      for (int c = 0; c < 9; ++c) Hc[c] = s_Hn[c];
      // (d) the candidate's inliers against the accepted model's
      {
        double a[2] = {0.0, 0.0};
        for (int p = t; p < K; p += 1024) {
          const float4 c4 = e.corr[p];
          const double x = c4.x, y = c4.y, u = c4.z, v = c4.w;
          const bool was = reproj2(H, x, y, u, v) <= t2, is = reproj2(Hc, x, y, u, v) <= t2;
          a[0] += is ? 1.0 : 0.0;
          a[1] += is != was ? 1.0 : 0.0;
        }
        vf_partials(a, s_acc);
      }
      __syncthreads();
      if (t == 0) {
        const double n = vf_total(s_acc, 0), changed = vf_total(s_acc, 1);
        if (n < s_nprev) {
          s_stop = 1;                                     // fewer inliers: keep H_{l-1}
        } else {
          for (int c = 0; c < 9; ++c) s_H[c] = s_Hn[c];
          s_nprev = n;
          s_rounds = s_rounds + 1;
          s_stop = changed == 0.0 ? 2 : 0;                // accepted; the same set again: converged
        }
      }
      __syncthreads();
      const int stop = s_stop;
      if (stop != 1)
        for (int c = 0; c < 9; ++c) H[c] = Hc[c];
      if (stop) break;
    }
  }
  // every path above ends behind a barrier that follows thread 0's last store to s_H
  for (int c = 0; c < 9; ++c) H[c] = s_H[c];
  {
    double a[1] = {0.0};
    for (int p = t; p < K; p += 1024) {
      const float4 c4 = e.corr[p];
      const bool in = reproj2(H, c4.x, c4.y, c4.z, c4.w) <= t2;
      e.inlier[e.rows[p]] = in ? 1 : 0;
      a[0] += in ? 1.0 : 0.0;
    }
    vf_partials(a, s_acc);
  }
  __syncthreads();
  if (t == 0) {
    e.record[VF_NVALID] = (float)K;
    e.record[VF_OK] = 1.f;
    e.record[VF_NINLIERS] = (float)vf_total(s_acc, 0);
    e.record[VF_BEST_HYP] = (float)s_bh;
    e.record[VF_BEST_HYP_INLIERS] = (float)s_bc;
    e.record[VF_LO_ROUNDS] = (float)s_rounds;
    e.record[VF_ERR_CORNER] = e.has_ref ? corner_error(H, e.href, e.height, e.width) : -1.f;
    e.record[VF_RESERVED] = 0.f;
    for (int c = 0; c < 9; ++c) e.hom[c] = (float)H[c];
  }
}

// The workspace of gims_verify_pairs: the VerifyDev table, then per set the dense correspondences, their rows, the hypothesis counters and K.
// recs == nullptr: sizing only.
static void verify_layout(const gims_verify_set* sets, int n_sets, int iters, WsLayout& L, VerifyDev* recs) {
  L.take<VerifyDev>(n_sets);
  for (int i = 0; i < n_sets; ++i) {
    const gims_verify_set& p = sets[i];
    VerifyDev d;
    memset(&d, 0, sizeof(d));
    d.corr = L.take<float4>(p.n0);
    d.rows = L.take<int32_t>(p.n0);
    d.hypcount = L.take<int32_t>(iters);
    d.nvalid = L.take<int32_t>(64);
    if (!recs) continue;
    d.kp0 = p.kpts0; d.kp1 = p.kpts1; d.matches0 = p.matches0;
    d.n0 = p.n0; d.n1 = p.n1; d.height = p.height; d.width = p.width; d.has_ref = p.has_ref ? 1 : 0;
    memcpy(d.href, p.h_ref, sizeof(d.href));
    d.inlier = p.inlier; d.record = p.record; d.hom = p.homography;
    recs[i] = d;
  }
}

static bool verify_shapes_ok(const gims_verify_set* sets, int n_sets) {
  for (int i = 0; i < n_sets; ++i)
    if (sets[i].n0 < 0 || sets[i].n1 < 0) return false;
  return true;
}

}  // namespace gims

extern "C" size_t gims_verify_workspace_bytes(const gims_verify_set* sets, int32_t n_sets, int32_t iters) {
  using namespace gims;
  if (!sets || n_sets <= 0 || iters < 0 || !verify_shapes_ok(sets, n_sets)) return 0;
  WsLayout L(nullptr);
  verify_layout(sets, n_sets, iters, L, nullptr);
  return L.bytes();
}

extern "C" int gims_verify_pairs(const gims_verify_set* sets, int32_t n_sets, float thresh, int32_t iters, int32_t lo_iters, uint64_t seed,
                                 void* work, size_t work_bytes, void* stream) {
  using namespace gims;
  GIMS_CHECK_ARG(sets && n_sets > 0 && work, "gims_verify_pairs: null / empty arguments");
  GIMS_CHECK_ARG(n_sets <= 65535, "gims_verify_pairs: %d sets in one call (at most 65535)", n_sets);
  GIMS_CHECK_ARG(iters >= 0 && iters <= (1 << 20) && lo_iters >= 0 && lo_iters <= 1024, "gims_verify_pairs: bad iteration counts");
  GIMS_CHECK_ARG(thresh >= 0.f && isfinite(thresh), "gims_verify_pairs: the threshold must be finite and not negative");
  for (int i = 0; i < n_sets; ++i) {
    const gims_verify_set& p = sets[i];
    GIMS_CHECK_ARG(p.n0 >= 0 && p.n1 >= 0 && (p.n0 == 0 || (p.kpts0 && p.inlier)) && (p.n1 == 0 || p.kpts1) && p.record && p.homography,
                   "gims_verify_pairs: set %d has a negative shape or a null pointer", i);
    GIMS_CHECK_ARG(p.matches0 || p.n0 == p.n1, "gims_verify_pairs: set %d has no matches0 (identity pairing) but n0 = %d != n1 = %d", i, p.n0, p.n1);
  }
  std::vector<VerifyDev> h(n_sets);
  WsLayout L(work);
  verify_layout(sets, n_sets, iters, L, h.data());
  GIMS_CHECK_ARG(work_bytes >= L.bytes(), "gims_verify_pairs: workspace too small (%zu < %zu)", work_bytes, L.bytes());
  hipStream_t s = (hipStream_t)stream;
  int rc = upload_table(h.data(), sizeof(VerifyDev) * (size_t)n_sets, work, s);
  if (rc != GIMS_OK) return rc;
  const VerifyDev* dev = (const VerifyDev*)work;
  const double t2 = (double)thresh * (double)thresh;
  hipLaunchKernelGGL(verify_gather_kernel, dim3(n_sets), dim3(1024), 0, s, dev);
  if (iters > 0) hipLaunchKernelGGL(verify_hyp_kernel, dim3(cdiv(iters, VF_HB), n_sets), dim3(256), 0, s, dev, seed, iters, t2);
  hipLaunchKernelGGL(verify_finish_kernel, dim3(n_sets), dim3(1024), 0, s, dev, seed, iters, lo_iters, t2);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}
