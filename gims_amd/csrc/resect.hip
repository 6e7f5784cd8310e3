// Absolute camera poses from 2-D to 3-D matches (resection): GIMS_AUX_RESECT_IMAGES of gims_run_ops gives every listed image
// its pose from the keypoints whose tracks already have a 3-D point, robustly: P3P hypotheses scored by reprojection inliers, a guarded
// Gauss-Newton local optimisation of the best one, one final classification of every correspondence.  include/gims_hip.h has the contract;
// tests/resect_ref.py is the NumPy restatement.  All geometry is float64 on the vector ALU.
//
// Launches, the same whatever the data: memset nodes (counters, kp_error = -1, kp_inlier = 0) -> the entry records (upload_table: kernel
// arguments, so a captured graph holds them) -> gather (a workgroup per entry: the ordered compaction of its correspondences) -> hyp (a
// workgroup per GIMS_RESECT_HB hypotheses of an entry: that many lanes solve one P3P sample each into LDS, then all 256 threads score one
// correspondence per tile against the models) -> finish (a workgroup per entry: best model, local optimisation, final sweep, record).
// Every floating-point sum over correspondences is a thread's own sum in ascending order, a butterfly over the wave, then the waves in
// order (rs_block_sum); an entry has a workgroup of its own, so its outputs do not depend on the batch, its place there, or the run.
#include "common.h"
#include "eval_geom.h"

#include <cfloat>
#include <vector>

namespace gims {

constexpr int RS_HB = GIMS_RESECT_HB;
constexpr int RS_MODELS = 4 * RS_HB;                         // a sample has up to four models
constexpr int RS_GROUP = 16;                                 // models scored per pass over the correspondences: their counters live in registers
constexpr int RS_THREADS = 256;
constexpr int RS_FT = 512;                                   // threads of the finish kernel
constexpr int RS_FW = RS_FT / 64;
constexpr int RS_REC = 6;                                    // a dense correspondence: X, u, v, keypoint index
constexpr int RS_BISECT = 80;
enum { RS_N_OK = 0, RS_N_FAILED, RS_N_CORR, RS_N_INLIER, RS_COUNTERS = 8 };

struct RsEntry {                                             // one entry as the kernels read it (56 bytes; built on the host from cams)
  double fx, fy, cx, cy, first;
  int32_t n_k, good;
  int64_t slot;                                              // the entry's place in kp_inlier / kp_error and in the dense array
};

struct RsOut {
  double* pose;
  int32_t *n_corr, *ok, *n_inliers, *best_hyp, *best_hyp_inliers, *lo_rounds, *counters, *hypscore;
  float *rms, *kp_error;
  uint8_t* kp_inlier;
  RsEntry* ent;
  double* corr;
};
static size_t rs_layout(void* base, int64_t m, int64_t S, int64_t iters, RsOut& w, WsRecord* rec = nullptr) {
  WsLayout L(base, rec);
  w.pose = L.take<double>((size_t)m * 12);
  w.n_corr = L.take<int32_t>((size_t)m);
  w.ok = L.take<int32_t>((size_t)m);
  w.n_inliers = L.take<int32_t>((size_t)m);
  w.best_hyp = L.take<int32_t>((size_t)m);
  w.best_hyp_inliers = L.take<int32_t>((size_t)m);
  w.lo_rounds = L.take<int32_t>((size_t)m);
  w.rms = L.take<float>((size_t)m);
  w.kp_inlier = L.take<uint8_t>((size_t)S);
  w.kp_error = L.take<float>((size_t)S);
  w.counters = L.take<int32_t>(RS_COUNTERS);
  L.scratch_from_here();
  w.ent = L.take<RsEntry>((size_t)m);
  w.corr = L.take<double>((size_t)S * RS_REC);
  w.hypscore = L.take<int32_t>((size_t)m * (size_t)iters);
  return L.bytes();
}

struct RsArgs {
  const int32_t* track_of;
  const double* xyz;
  const uint8_t* use;
  const float* kpts;
  RsOut out;
  int m, iters, lo_iters, min_inliers;
  int64_t N, T;
  uint64_t seed;
  double thresh2;
};

__device__ __forceinline__ bool rs_finite(double x) { return fabs(x) <= DBL_MAX; }       // (false for a NaN)

// ---------------------------------------------------------------------------------------------- gather
__global__ __launch_bounds__(RS_THREADS) void resect_gather_kernel(RsArgs a) {
  __shared__ int s_w[RS_THREADS / 64];
  const RsEntry en = a.out.ent[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double* dense = a.out.corr + en.slot * RS_REC;
  int K = 0;
  for (int i0 = 0; i0 < en.n_k; i0 += RS_THREADS) {           // the same trip count for every thread
    const int i = i0 + t;
    bool ok = false;
    double X[3] = {0.0, 0.0, 0.0};
    float u = 0.f, v = 0.f;
    const double node = en.first + (double)i;
    if (i < en.n_k && en.good && node >= 0.0 && node < (double)a.N) {
      const int64_t g = (int64_t)node;                       // 0 .. N - 1
      const int tr = a.track_of[g];
      if (tr >= 0 && (int64_t)tr < a.T && a.use[tr] != 0) {
        u = a.kpts[2 * g], v = a.kpts[2 * g + 1];
        X[0] = a.xyz[(int64_t)3 * tr], X[1] = a.xyz[(int64_t)3 * tr + 1], X[2] = a.xyz[(int64_t)3 * tr + 2];
        ok = rs_finite(X[0]) && rs_finite(X[1]) && rs_finite(X[2]) && rs_finite((double)u) && rs_finite((double)v);
      }
    }
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) s_w[wave] = __popcll(bal);
    __syncthreads();
    int before = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < RS_THREADS / 64; ++w) {
      before += w < wave ? s_w[w] : 0;
      total += s_w[w];
    }
    if (ok) {
      double* r = dense + (int64_t)(K + before) * RS_REC;    // K + before <= i < n_k: inside the entry's slots
      r[0] = X[0], r[1] = X[1], r[2] = X[2], r[3] = (double)u, r[4] = (double)v, r[5] = (double)i;
    }
    K += total;
    __syncthreads();
  }
  if (t == 0) a.out.n_corr[blockIdx.x] = K;
}

// ---------------------------------------------------------------------------------------------- P3P
// the real roots of the quartic c (ascending coefficients), ascending, by bisection between the roots of successive derivatives inside
// the bound 1 + max |c_i / c_4| (the method of vp_real_roots in verify.hip, at degree 4); -1 when c_4 is 0 or anything is not finite
__device__ int rs_real_roots(const double (&c)[5], double (&roots)[4]) {
  bool fin = c[4] != 0.0;
  double bound = 0.0;
  for (int i = 0; i < 5; ++i) fin = fin && rs_finite(c[i]);
  if (!fin) return -1;
  for (int i = 0; i < 4; ++i) bound = fmax(bound, fabs(c[i] / c[4]));
  bound = 1.0 + bound;
  if (!rs_finite(bound)) return -1;
  double prev[4], q[5];
  int nprev = 0;
#pragma unroll 1
  for (int d = 1; d <= 4; ++d) {
    const int k = 4 - d;
    for (int i = 0; i <= d; ++i) {
      double f = 1.0;
      for (int m = i + 1; m <= i + k; ++m) f *= (double)m;
      q[i] = c[i + k] * f;
    }
    int ncur = 0;
    double lo = -bound, flo = vp_horner(q, d, lo);
#pragma unroll 1
    for (int s = 0; s <= nprev; ++s) {
      const double hi = s < nprev ? prev[s] : bound, fhi = vp_horner(q, d, hi);
      if ((flo > 0.0) != (fhi > 0.0)) {
        const bool sa = flo > 0.0;
        double x = lo, y = hi;
#pragma unroll 1
        for (int it = 0; it < RS_BISECT; ++it) {
          const double mid = 0.5 * (x + y);
          const bool same = (vp_horner(q, d, mid) > 0.0) == sa;
          x = same ? mid : x;
          y = same ? y : mid;
        }
        roots[ncur++] = 0.5 * (x + y);                       // at most one root per interval: ncur <= d
      }
      lo = hi;
      flo = fhi;
    }
    nprev = ncur;
    for (int s = 0; s < ncur; ++s) prev[s] = roots[s];
  }
  return nprev;
}

// the orthonormal frame of a triangle: e1 = (P2 - P1)^, e3 = (e1 x (P3 - P1))^, e2 = e3 x e1, as the ROWS of E; returns |e1 x (P3 - P1)|^2
__device__ __forceinline__ double rs_frame(const double* P1, const double* P2, const double* P3, double (&E)[3][3]) {
  const double d0 = P2[0] - P1[0], d1 = P2[1] - P1[1], d2 = P2[2] - P1[2], dl = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  E[0][0] = d0 / dl, E[0][1] = d1 / dl, E[0][2] = d2 / dl;
  const double g0 = P3[0] - P1[0], g1 = P3[1] - P1[1], g2 = P3[2] - P1[2];
  const double n0 = E[0][1] * g2 - E[0][2] * g1, n1 = E[0][2] * g0 - E[0][0] * g2, n2 = E[0][0] * g1 - E[0][1] * g0;
  const double nn = n0 * n0 + n1 * n1 + n2 * n2, nl = sqrt(nn);
  E[2][0] = n0 / nl, E[2][1] = n1 / nl, E[2][2] = n2 / nl;
  E[1][0] = E[2][1] * E[0][2] - E[2][2] * E[0][1];
  E[1][1] = E[2][2] * E[0][0] - E[2][0] * E[0][2];
  E[1][2] = E[2][0] * E[0][1] - E[2][1] * E[0][0];
  return nn;
}

// The models of the sample (r0, r1, r2: dense records) in the camera of en: M[j] = {R row-major, t} for the real root j of the quartic
// (ascending); bit j of the result says that root j gives a model.  Nothing is written for the other roots.
__device__ __noinline__ int rs_p3p(const double* r0, const double* r1, const double* r2, const RsEntry& en, double (*M)[12]) {
  const double* rec[3] = {r0, r1, r2};
  double f[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double x = (rec[i][3] - en.cx) / en.fx, y = (rec[i][4] - en.cy) / en.fy, n = sqrt(x * x + y * y + 1.0);
    f[i][0] = x / n, f[i][1] = y / n, f[i][2] = 1.0 / n;
  }
  auto dot = [](const double* p, const double* q) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]; };
  auto dist2 = [](const double* p, const double* q) {
    const double d0 = p[0] - q[0], d1 = p[1] - q[1], d2 = p[2] - q[2];
    return d0 * d0 + d1 * d1 + d2 * d2;
  };
  const double c12 = dot(f[0], f[1]), c13 = dot(f[0], f[2]), c23 = dot(f[1], f[2]);
  const double a = dist2(r0, r1), b = dist2(r0, r2), c = dist2(r1, r2);
  double EX[3][3];
  const double nnX = rs_frame(r0, r1, r2, EX);
  if (!(a > 0.0) || !(nnX > 1e-18 * b)) return 0;            // two points coincide, or the three lie on a line
  const double q[3] = {1.0, -2.0 * c12, 1.0}, N[3] = {(b - c) - a, -2.0 * c12 * (b - c), (b - c) + a}, D[2] = {-2.0 * a * c13, 2.0 * a * c23};
  double D2[3], qD2[5], N2[5], ND[4], P[5];
  vp_pmul(D, 2, D, 2, D2);
  vp_pmul(q, 3, D2, 3, qD2);
  vp_pmul(N, 3, N, 3, N2);
  vp_pmul(N, 3, D, 2, ND);
  for (int i = 0; i < 5; ++i) P[i] = b * qD2[i] - a * ((i < 3 ? D2[i] : 0.0) + N2[i] - 2.0 * c13 * (i < 4 ? ND[i] : 0.0));
  double roots[4];
  const int nr = rs_real_roots(P, roots);
  int mask = 0;
#pragma unroll 1
  for (int j = 0; j < nr; ++j) {
    const double u = roots[j];
    const double Du = vp_horner(D, 1, u), Nu = vp_horner(N, 2, u), qu = vp_horner(q, 2, u);
    if (!(u > 0.0) || !(fabs(Du) > 1e-12 * a) || !(qu > 0.0)) continue;
    const double v = Nu / Du;
    if (!(v > 0.0)) continue;
    const double s1 = sqrt(a / qu), s2 = u * s1, s3 = v * s1;
    double Y[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) Y[0][k] = s1 * f[0][k], Y[1][k] = s2 * f[1][k], Y[2][k] = s3 * f[2][k];
    double EY[3][3];
    rs_frame(Y[0], Y[1], Y[2], EY);
    double* Mj = M[j];
    bool fin = true;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const double v_rs = EY[0][r] * EX[0][s] + EY[1][r] * EX[1][s] + EY[2][r] * EX[2][s];       // R = E_Y E_X^T, the frames as columns
        Mj[3 * r + s] = v_rs;
        fin = fin && rs_finite(v_rs);
      }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double tr = Y[0][r] - (Mj[3 * r] * r0[0] + Mj[3 * r + 1] * r0[1] + Mj[3 * r + 2] * r0[2]);
      Mj[9 + r] = tr;
      fin = fin && rs_finite(tr);
    }
    if (fin) mask |= 1 << j;
  }
  return mask;
}

// depth and squared reprojection error of X under the model M = {R, t}
__device__ __forceinline__ void rs_reproject(const double* M, const RsEntry& en, const double* r, double& z, double& e2) {
  const double x = M[0] * r[0] + M[1] * r[1] + M[2] * r[2] + M[9];
  const double y = M[3] * r[0] + M[4] * r[1] + M[5] * r[2] + M[10];
  z = M[6] * r[0] + M[7] * r[1] + M[8] * r[2] + M[11];
  const double ru = en.fx * x / z + en.cx - r[3], rv = en.fy * y / z + en.cy - r[4];
  e2 = ru * ru + rv * rv;
}

// ---------------------------------------------------------------------------------------------- hypotheses
// One workgroup per RS_HB hypotheses of one entry (the grid walks the work items by its stride).  hypscore[h] = the best inlier count of
// the sample's models << 2 | (3 - the root index of the first model that has it), -1 without a model.
// The register budget is stated: three waves per SIMD, 168 VGPRs.  The scoring loop needs RS_GROUP counters, one model (24 registers) and
// one correspondence (10); it is the P3P solver of the first RS_HB lanes -- the bearings, the two frames and the polynomials alive at
// once in float64 -- that sets the kernel's count: asked for four waves (128 registers) the compiler reports that it cannot meet them
// and takes 150; within this budget it takes all 168, spills no VGPR, and keeps 240 bytes of scratch for the root finder's indexed arrays.
__global__ __launch_bounds__(RS_THREADS, 3) void resect_hyp_kernel(RsArgs a, int blocks_per_entry) {
  __shared__ double s_M[RS_MODELS][12];
  __shared__ int s_mask[RS_HB], s_tag[RS_MODELS], s_n;
  __shared__ int s_cnt[RS_THREADS / 64][RS_MODELS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t items = (int64_t)a.m * blocks_per_entry;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
    const int e = (int)(w / blocks_per_entry), h0 = (int)(w % blocks_per_entry) * RS_HB;
    const RsEntry en = a.out.ent[e];
    const int K = a.out.n_corr[e];
    int32_t* hypscore = a.out.hypscore + (size_t)e * (size_t)a.iters;
    const double* dense = a.out.corr + en.slot * RS_REC;
    if (K < 3) {                                             // the same for every thread of the workgroup
      if (t < RS_HB && h0 + t < a.iters) hypscore[h0 + t] = -1;
      continue;
    }
    if (t < RS_HB) {
      int mask = 0;
      if (h0 + t < a.iters) {
        int idx[3];
        ransac_sample(a.seed, h0 + t, K, idx);
        mask = rs_p3p(dense + (int64_t)idx[0] * RS_REC, dense + (int64_t)idx[1] * RS_REC, dense + (int64_t)idx[2] * RS_REC, en, &s_M[4 * t]);
      }
      s_mask[t] = mask;
    }
    __syncthreads();
    if (t == 0) {                                            // the models that exist, in the order (lane, root)
      int n = 0;
      for (int j = 0; j < RS_MODELS; ++j)
        if ((s_mask[j >> 2] >> (j & 3)) & 1) s_tag[n++] = j;
      s_n = n;
    }
    __syncthreads();
    const int n_models = s_n;
    for (int g0 = 0; g0 < n_models; g0 += RS_GROUP) {
      int cnt[RS_GROUP];
#pragma unroll
      for (int b = 0; b < RS_GROUP; ++b) cnt[b] = 0;
      for (int p0 = 0; p0 < K; p0 += RS_THREADS) {
        const int p = p0 + t;
        const bool have = p < K;
        double r[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) r[j] = dense[(int64_t)(have ? p : 0) * RS_REC + j];
#pragma unroll
        for (int b = 0; b < RS_GROUP; ++b) {
          if (g0 + b < n_models) {
            double Mb[12];
            const double* src = s_M[s_tag[g0 + b]];
#pragma unroll
            for (int j = 0; j < 12; ++j) Mb[j] = src[j];
            double z, e2;
            rs_reproject(Mb, en, r, z, e2);
            cnt[b] += have && z > 0.0 && e2 <= a.thresh2 ? 1 : 0;
          }
        }
        // the models are read from LDS again for every tile (wave-uniform addresses: broadcasts); the barrier keeps the compiler from
        // hoisting RS_GROUP models, 384 registers, out of the loop (see vf_score in verify.hip)
        __syncthreads();
      }
#pragma unroll
      for (int b = 0; b < RS_GROUP; ++b) {
        int s = cnt[b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0 && g0 + b < n_models) s_cnt[wave][g0 + b] = s;
      }
    }
    __syncthreads();
    if (t < RS_HB && h0 + t < a.iters) {
      int best = -1;
      for (int j = 0; j < n_models; ++j) {
        const int tag = s_tag[j];
        if ((tag >> 2) != t) continue;
        int c = 0;
        for (int wv = 0; wv < RS_THREADS / 64; ++wv) c += s_cnt[wv][j];
        const int v = (c << 2) | (3 - (tag & 3));
        if ((v >> 2) > (best >> 2)) best = v;                // the roots come in ascending order: the first of equal count stays
      }
      hypscore[h0 + t] = best;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------- finish
// The sums acc[0 .. N - 1] of the workgroup in a fixed order: the butterfly of a wave, then the waves in order.  Ends behind a barrier with
// the totals in s_tot; s_part is [RS_FW][N].
template <int N>
__device__ __forceinline__ void rs_block_sum(double (&acc)[N], double* s_part, double* s_tot) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double v = acc[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) s_part[wave * N + j] = v;
  }
  __syncthreads();
  if (t < N) {
    double v = s_part[t];
    for (int w = 1; w < RS_FW; ++w) v += s_part[w * N + t];
    s_tot[t] = v;
  }
  __syncthreads();
}

// the inlier count and the inlier cost of the model M over the K correspondences: s_tot[0] = the cost, s_tot[1] = the count
__device__ __forceinline__ void rs_evaluate(const double* M, const RsEntry& en, const double* dense, int K, double t2, double* s_part, double* s_tot) {
  double Mr[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) Mr[j] = M[j];
  double acc[2] = {0.0, 0.0};
  for (int p = threadIdx.x; p < K; p += RS_FT) {
    double z, e2;
    rs_reproject(Mr, en, dense + (int64_t)p * RS_REC, z, e2);
    if (z > 0.0 && e2 <= t2) acc[0] += e2, acc[1] += 1.0;
  }
  rs_block_sum<2>(acc, s_part, s_tot);
}

// (sum J^T J) d = -(sum J^T r) from the 27 sums (the upper triangle by rows, then the right-hand side): Gaussian elimination with partial
// pivoting (the first row of the largest magnitude) on the 6 x 7 array, then back substitution.  false when a pivot is not above 1e-12
// times the largest diagonal entry of the matrix
__device__ bool rs_solve6(const double* sums, double (&d)[6]) {
  double A[6][7];
  int k = 0;
  double diag = 0.0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = sums[k++];
  for (int i = 0; i < 6; ++i) {
    A[i][6] = sums[21 + i];
    diag = fmax(diag, fabs(A[i][i]));
  }
  if (!rs_finite(diag)) return false;
  for (int c = 0; c < 6; ++c) {
    int piv = c;
    double best = fabs(A[c][c]);
    for (int r = c + 1; r < 6; ++r)
      if (fabs(A[r][c]) > best) best = fabs(A[r][c]), piv = r;
    if (!(best > 1e-12 * diag)) return false;
    if (piv != c)
      for (int j = 0; j < 7; ++j) {
        const double x = A[c][j];
        A[c][j] = A[piv][j];
        A[piv][j] = x;
      }
    for (int r = c + 1; r < 6; ++r) {
      const double f = A[r][c] / A[c][c];
      for (int j = c; j < 7; ++j) A[r][j] -= f * A[c][j];
    }
  }
  for (int c = 5; c >= 0; --c) {
    double s = A[c][6];
    for (int j = c + 1; j < 6; ++j) s -= A[c][j] * d[j];
    d[c] = s / A[c][c];
  }
  return true;
}

__global__ __launch_bounds__(RS_FT) void resect_finish_kernel(RsArgs a) {
  __shared__ double s_part[RS_FW * 27], s_tot[27], s_cur[12], s_cand[12];
  __shared__ int s_best[RS_FW][2], s_flag;
  const int e = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const RsEntry en = a.out.ent[e];
  const int K = a.out.n_corr[e];
  const double* dense = a.out.corr + en.slot * RS_REC;
  const int32_t* hypscore = a.out.hypscore + (size_t)e * (size_t)a.iters;

  // ---- the best hypothesis: the largest count, then the smallest h (its root is in the low bits)
  int bv = -1, bh = 0x7fffffff;
  if (K >= 3)
    for (int h = t; h < a.iters; h += RS_FT) {
      const int v = hypscore[h];
      if ((v >> 2) > (bv >> 2)) bv = v, bh = h;
    }
  for (int o = 32; o > 0; o >>= 1) {
    const int ov = __shfl_xor(bv, o, 64), oh = __shfl_xor(bh, o, 64);
    if ((ov >> 2) > (bv >> 2) || ((ov >> 2) == (bv >> 2) && oh < bh)) bv = ov, bh = oh;
  }
  if (lane == 0) s_best[wave][0] = bv, s_best[wave][1] = bh;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < RS_FW; ++w)
      if ((s_best[w][0] >> 2) > (bv >> 2) || ((s_best[w][0] >> 2) == (bv >> 2) && s_best[w][1] < bh)) bv = s_best[w][0], bh = s_best[w][1];
    int have = 0;
    if (bv >= 0) {                                           // the model again, by the arithmetic that scored it
      double M[4][12];
      int idx[3];
      ransac_sample(a.seed, bh, K, idx);
      const int mask = rs_p3p(dense + (int64_t)idx[0] * RS_REC, dense + (int64_t)idx[1] * RS_REC, dense + (int64_t)idx[2] * RS_REC, en, M);
      const int root = 3 - (bv & 3);
      if ((mask >> root) & 1) {
        have = 1;
        for (int j = 0; j < 12; ++j) s_cur[j] = M[root][j];
      }
    }
    s_flag = have;
    s_best[0][0] = bv, s_best[0][1] = bh;
  }
  __syncthreads();
  const bool model = s_flag != 0;
  bv = s_best[0][0], bh = s_best[0][1];
  __syncthreads();

  int rounds = 0, n_in = 0;
  double sum = 0.0;
  if (model) {
    // ---- stage 2: guarded Gauss-Newton over the current inlier set
    rs_evaluate(s_cur, en, dense, K, a.thresh2, s_part, s_tot);
    double cost = s_tot[0], count = s_tot[1];
    for (int it = 0; it < a.lo_iters && count >= 4.0; ++it) {        // (three correspondences fit their model: nothing to optimise)
      double acc[27], Mr[12];
#pragma unroll
      for (int j = 0; j < 27; ++j) acc[j] = 0.0;
#pragma unroll
      for (int j = 0; j < 12; ++j) Mr[j] = s_cur[j];
      for (int p = t; p < K; p += RS_FT) {
        const double* r = dense + (int64_t)p * RS_REC;
        const double y0 = Mr[0] * r[0] + Mr[1] * r[1] + Mr[2] * r[2], y1 = Mr[3] * r[0] + Mr[4] * r[1] + Mr[5] * r[2];
        const double y2 = Mr[6] * r[0] + Mr[7] * r[1] + Mr[8] * r[2];
        const double x = y0 + Mr[9], y = y1 + Mr[10], z = y2 + Mr[11];
        const double ru = en.fx * x / z + en.cx - r[3], rv = en.fy * y / z + en.cy - r[4];
        if (!(z > 0.0 && ru * ru + rv * rv <= a.thresh2)) continue;
        const double au = en.fx / z, bu = -en.fx * x / (z * z), av = en.fy / z, bw = -en.fy * y / (z * z);
        const double ju[6] = {bu * y1, au * y2 - bu * y0, -au * y1, au, 0.0, bu};
        const double jv[6] = {bw * y1 - av * y2, -bw * y0, av * y0, 0.0, av, bw};
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = i; j < 6; ++j) acc[k++] += ju[i] * ju[j] + jv[i] * jv[j];
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[21 + i] += -(ju[i] * ru + jv[i] * rv);
      }
      rs_block_sum<27>(acc, s_part, s_tot);
      if (t == 0) {
        double d[6];
        bool ok = rs_solve6(s_tot, d);
        if (ok) {
          const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], th = sqrt(th2);
          const double ca = th > 1e-8 ? sin(th) / th : 1.0, cb = th > 1e-8 ? (1.0 - cos(th)) / th2 : 0.5;
          const double W[3][3] = {{0.0, -d[2], d[1]}, {d[2], 0.0, -d[0]}, {-d[1], d[0], 0.0}};
          double Ex[3][3];
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
              Ex[i][j] = (i == j ? 1.0 : 0.0) + ca * W[i][j] + cb * (W[i][0] * W[0][j] + W[i][1] * W[1][j] + W[i][2] * W[2][j]);
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
              const double v = Ex[i][0] * s_cur[j] + Ex[i][1] * s_cur[3 + j] + Ex[i][2] * s_cur[6 + j];
              s_cand[3 * i + j] = v;
              ok = ok && rs_finite(v);
            }
          for (int i = 0; i < 3; ++i) {
            s_cand[9 + i] = s_cur[9 + i] + d[3 + i];
            ok = ok && rs_finite(s_cand[9 + i]);
          }
        }
        s_flag = ok ? 1 : 0;
      }
      __syncthreads();
      if (!s_flag) break;                                    // (the same for every thread)
      rs_evaluate(s_cand, en, dense, K, a.thresh2, s_part, s_tot);
      const double cost_c = s_tot[0], count_c = s_tot[1];
      // equal counts: the costs are compared as floats, so that the decision does not hang on the last bits of two float64 sums
      if (!(count_c > count || (count_c == count && (float)cost_c < (float)cost))) break;
      __syncthreads();                                       // every thread has read s_tot and s_flag
      if (t < 12) s_cur[t] = s_cand[t];
      cost = cost_c, count = count_c;
      ++rounds;
      __syncthreads();
    }
    __syncthreads();
    n_in = (int)count, sum = cost;                           // the final sweep's count and sum: the current model was scored by the same arithmetic
  }
  const int need = a.min_inliers > 4 ? a.min_inliers : 4;
  const bool ok = model && n_in >= need;
  if (ok) {
    // ---- the final sweep: every correspondence once at the final model
    double Mr[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) Mr[j] = s_cur[j];
    for (int p = t; p < K; p += RS_FT) {
      const double* r = dense + (int64_t)p * RS_REC;
      double z, e2;
      rs_reproject(Mr, en, r, z, e2);
      const double err = sqrt(e2);
      const int64_t at = en.slot + (int64_t)r[5];
      a.out.kp_inlier[at] = z > 0.0 && e2 <= a.thresh2 ? 1 : 0;
      a.out.kp_error[at] = z > 0.0 && err == err ? (err < (double)FLT_MAX ? (float)err : FLT_MAX) : -1.f;
    }
  }
  if (t < 12) a.out.pose[(int64_t)12 * e + t] = ok ? s_cur[t] : 0.0;
  if (t == 0) {
    a.out.ok[e] = ok ? 1 : 0;
    a.out.n_inliers[e] = ok ? n_in : 0;
    a.out.rms[e] = ok ? (float)sqrt(sum / (double)n_in) : 0.f;
    a.out.best_hyp[e] = model ? bh : -1;
    a.out.best_hyp_inliers[e] = model ? bv >> 2 : 0;
    a.out.lo_rounds[e] = rounds;
    atomicAdd(a.out.counters + (ok ? RS_N_OK : RS_N_FAILED), 1);
    if (K) atomicAdd(a.out.counters + RS_N_CORR, K);
    if (ok) atomicAdd(a.out.counters + RS_N_INLIER, n_in);
  }
}

// gims_aux_layout for GIMS_AUX_RESECT_IMAGES: sizes = {m, S, iters}, S the sum of the entries' n_k; the bounds are the op's below
int resect_images_aux_layout(const int64_t* sizes, int n, WsRecord& rec) {
  GIMS_CHECK_ARG(n == 3, "resect_images: the layout takes 3 sizes {m, S, iters}, not %d", n);
  const int64_t m = sizes[0], S = sizes[1], iters = sizes[2];
  GIMS_CHECK_ARG(m >= 0 && m <= (1 << 24), "resect_images: m = %lld is out of range (0 .. 2^24)", (long long)m);
  GIMS_CHECK_ARG(S >= 0 && S <= (1 << 30), "resect_images: the entries have S = %lld keypoints in all (out of range: 0 .. 2^30)", (long long)S);
  GIMS_CHECK_ARG(iters >= 0 && iters <= 65535, "resect_images: iters = %lld is out of range (0 .. 65535)", (long long)iters);
  RsOut w;
  rec.bytes = rs_layout(nullptr, m, S, iters, w, &rec);
  return GIMS_OK;
}

// GIMS_AUX_RESECT_IMAGES of gims_run_ops (include/gims_hip.h): every argument check precedes the first HIP call
int resect_images_aux(const gims_aux_args& x, hipStream_t st) {
  const int64_t m = x.i[0], N = x.i[1], T = x.i[2], mode = x.i[3];
  const float thresh = x.f[0];
  // i[5] is where a later form of this function would be selected: it is read FIRST (see assemble_rows_aux)
  GIMS_CHECK_ARG(x.i[5] == 0, "gims_run_ops: unknown auxiliary function form: resect_images with i[5] = %lld (i[5] is reserved and must be 0)",
                 (long long)x.i[5]);
  GIMS_CHECK_ARG(m >= 0 && m <= (1 << 24), "resect_images: m = %lld is out of range (0 .. 2^24)", (long long)m);
  GIMS_CHECK_ARG(N >= 0 && N <= (1 << 30), "resect_images: N = %lld is out of range (0 .. 2^30)", (long long)N);
  GIMS_CHECK_ARG(T >= 0 && T <= (1 << 30), "resect_images: T = %lld is out of range (0 .. 2^30)", (long long)T);
  const int64_t iters = mode & 0xffff, lo_iters = (mode >> 16) & 0xff, min_inliers = mode >> 24;
  GIMS_CHECK_ARG(mode >= 0 && min_inliers <= (1 << 30),
                 "resect_images: i[3] = %lld: iters | lo_iters << 16 | min_inliers << 24 with iters in 0 .. 65535, lo_iters in 0 .. 255 and "
                 "min_inliers in 0 .. 2^30", (long long)mode);
  GIMS_CHECK_ARG(thresh - thresh == 0.f && thresh > 0.f, "resect_images: thresh = %g must be finite and > 0", (double)thresh);
  GIMS_CHECK_ARG(x.f[1] == 0.f, "resect_images: f[1] = %g is reserved and must be 0", (double)x.f[1]);
  GIMS_CHECK_ARG(x.p[5], "resect_images: the output buffer is NULL");
  GIMS_CHECK_ARG(m == 0 || (x.p[0] && x.p[1] && x.p[2] && x.p[3] && x.p[4]),
                 "resect_images: track_of, xyz, use, kpts or cams is NULL while m = %lld", (long long)m);
  GIMS_CHECK_ARG(((uintptr_t)x.p[5] & 15) == 0, "resect_images: the output buffer must be 16-byte aligned");
  GIMS_CHECK_ARG((((uintptr_t)x.p[1] | (uintptr_t)x.p[4]) & 7) == 0, "resect_images: xyz and cams must be 8-byte aligned");
  GIMS_CHECK_ARG((((uintptr_t)x.p[0] | (uintptr_t)x.p[3]) & 3) == 0, "resect_images: track_of and kpts must be 4-byte aligned");
  // cams is a HOST array, like the op table itself: the slots of kp_inlier / kp_error follow from its n_k
  const double* cams = (const double*)x.p[4];
  std::vector<RsEntry> ent((size_t)m);
  int64_t S = 0;
  for (int64_t e = 0; e < m; ++e) {
    const double* r = cams + GIMS_RESECT_CAMERA_WORDS * e;
    const double n_k = r[5];
    GIMS_CHECK_ARG(n_k >= 0.0 && n_k <= (double)(1 << 30) && n_k == (double)(int64_t)n_k,
                   "resect_images: entry %lld: n_k = %g is out of range (an integer in 0 .. 2^30)", (long long)e, n_k);
    bool good = r[0] > 0.0 && r[1] > 0.0;
    for (int j = 0; j < 5; ++j) good = good && fabs(r[j]) <= DBL_MAX;
    RsEntry& d = ent[(size_t)e];
    d.fx = r[0], d.fy = r[1], d.cx = r[2], d.cy = r[3], d.first = good ? r[4] : 0.0;
    d.n_k = (int32_t)n_k, d.good = good ? 1 : 0, d.slot = S;
    S += (int64_t)n_k;
    GIMS_CHECK_ARG(S <= (1 << 30), "resect_images: the entries have more than 2^30 keypoints in all (out of range)");
  }

  RsArgs a;
  rs_layout((void*)x.p[5], m, S, iters, a.out);
  GIMS_HIP(hipMemsetAsync(a.out.counters, 0, sizeof(int32_t) * RS_COUNTERS, st));
  if (m == 0) return GIMS_OK;
  a.track_of = (const int32_t*)x.p[0], a.xyz = (const double*)x.p[1], a.use = (const uint8_t*)x.p[2], a.kpts = (const float*)x.p[3];
  a.m = (int)m, a.N = N, a.T = T, a.iters = (int)iters, a.lo_iters = (int)lo_iters, a.min_inliers = (int)min_inliers;
  a.seed = (uint64_t)x.i[4], a.thresh2 = (double)thresh * (double)thresh;
  if (S > 0) {
    GIMS_HIP(hipMemsetD32Async((hipDeviceptr_t)a.out.kp_error, (int)0xBF800000u, (size_t)S, st));          // -1.f
    GIMS_HIP(hipMemsetAsync(a.out.kp_inlier, 0, (size_t)S, st));
  }
  const int rc = upload_table(ent.data(), sizeof(RsEntry) * (size_t)m, a.out.ent, st);
  if (rc != GIMS_OK) return rc;
  resect_gather_kernel<<<(unsigned)m, RS_THREADS, 0, st>>>(a);
  GIMS_LAUNCH_CHECK();
  if (iters > 0) {
    const int bpe = cdiv(iters, RS_HB);
    const int64_t items = m * bpe, cap = (int64_t)device_cus() * 64;
    resect_hyp_kernel<<<(unsigned)(items < cap ? items : cap), RS_THREADS, 0, st>>>(a, bpe);
    GIMS_LAUNCH_CHECK();
  }
  resect_finish_kernel<<<(unsigned)m, RS_FT, 0, st>>>(a);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

}  // namespace gims
