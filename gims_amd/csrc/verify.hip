// Ground-truth-free geometric verification: a RANSAC model over a set of correspondences and its inlier mask -- what
// the reference's drivers get from cv2.findHomography(points0, points1, RANSAC | USAC_DEFAULT) (eval_homography.py:191, eval_matches.py:71,164,
// tools/parameter_search.py:161) -- as an entry point of its own, with a guarded, normalised local optimisation of the best hypothesis.
// The estimator is this build's own and fully specified in include/gims_hip.h; the homography's stage 1 and its lo_iters == 0 refit are
// those of gims_eval_pairs (csrc/eval.hip) through the helpers of eval_geom.h.
//
// Three models, chosen per set (gims_verify_set.model): homography, fundamental matrix, calibrated relative pose.  What they share is
// written once and templated on a model policy (HomographyModel, FundamentalModel, PoseModel below: minimum count, coordinates, inlier
// predicate, the sums of a refit and its solve):
//   vf_score        up to VF_HB models in LDS against all correspondences, counters in registers;
//   vf_local_opt    the guarded local optimisation, its LDS state in one struct (VfLo), the rule on barriers stated above it;
//   vf_best, vf_no_model, vf_final_sweep, vf_sign   the prologue and epilogue of a finish kernel.
// Five kernels, batched over sets:
//   gather                one workgroup per set: ordered compaction of the correspondences into a dense float4 {x, y, u, v} array;
//   hyp / pose_hyp        one workgroup per VF_HB hypotheses: VF_HB lanes solve a sample each into LDS, then every thread scores one
//                         correspondence per tile (one coalesced 16-byte load) against the models (LDS broadcast reads);
//   finish / pose_finish  one workgroup per set: best hypothesis, stage 2, mask, record (and corner error, or the pose).
// Homography and fundamental sets share the second and third kernel, the model a per-set branch that is uniform over the workgroup; pose
// sets run in the last two, launched over their own part of the set table (a sample of theirs has up to ten models).
#include "common.h"
#include "eval_geom.h"

#include <math.h>
#include <string.h>

#include <vector>

namespace gims {

struct VerifyDev {
  const float* kp0; const float* kp1; const int64_t* matches0;
  int n0, n1, height, width, has_ref, model;
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

constexpr int VF_HB = 16;          // hypotheses per workgroup of the scoring kernels
constexpr int VF_ACC = 45;         // widest row of per-wave partial sums: the 45 sums of the epipolar refit (the homography's uses 44)
constexpr int VF_JACOBI_SWEEPS = 12;

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

// ---------------------------------------------------------------------------------------------- minimal models on the dense array
// homography4 of eval_geom.h on the dense array: other loads, the same system
__device__ bool homography4_dense(const float4* __restrict__ corr, const int (&idx)[4], double (&H)[9]) {
  return homography4_solve([&](int k, double& x, double& y, double& u, double& v) {
    const float4 c = corr[idx[k]];
    x = c.x; y = c.y; u = c.z; v = c.w;
  }, H);
}

// inlier(F, x, y, u, v) of the specification: squared Sampson distance <= thresh^2, without the division
__device__ __forceinline__ bool sampson_in(const double (&F)[9], double x, double y, double u, double v, double t2) {
  const double a0 = F[0] * x + F[1] * y + F[2], a1 = F[3] * x + F[4] * y + F[5], a2 = F[6] * x + F[7] * y + F[8];
  const double g0 = F[0] * u + F[3] * v + F[6], g1 = F[1] * u + F[4] * v + F[7];
  const double e = u * a0 + v * a1 + a2, den = a0 * a0 + a1 * a1 + g0 * g0 + g1 * g1;
  return den > 0.0 && e * e <= t2 * den;
}

// unit(F): false when the norm is 0 or anything is not finite
__device__ bool vf_unit(double (&F)[9]) {
  double n2 = 0.0;
  for (int c = 0; c < 9; ++c) n2 += F[c] * F[c];
  const double n = sqrt(n2);
  if (!(n > 0.0) || !isfinite(n)) return false;
  bool fin = true;
  for (int c = 0; c < 9; ++c) { F[c] = F[c] / n; fin = fin && isfinite(F[c]); }
  return fin;
}

// denormalise: F = T1^T Fn T0 for the similarities (centroid, scale) of the two images
__device__ void vf_denormalise(const double (&Fn)[9], double cx, double cy, double s0, double cu, double cv, double s1, double (&F)[9]) {
  double M[9];
  for (int r = 0; r < 3; ++r) {
    M[3 * r] = Fn[3 * r] * s0;
    M[3 * r + 1] = Fn[3 * r + 1] * s0;
    M[3 * r + 2] = Fn[3 * r + 2] - s0 * (Fn[3 * r] * cx + Fn[3 * r + 1] * cy);
  }
  for (int c = 0; c < 3; ++c) {
    F[c] = s1 * M[c];
    F[3 + c] = s1 * M[3 + c];
    F[6 + c] = M[6 + c] - s1 * (cu * M[c] + cv * M[3 + c]);
  }
}

// Gauss-Jordan elimination with complete pivoting of an R x 9 system (R = 8: the fundamental model, R = 5: the five-point solver); the
// 9 - R columns left without a pivot (the clear bits of cused) are the free variables of its null space.  prow, pcol: four bits per
// elimination step.  The array is indexed by the pivot search, so it lives in LDS: entry (r, c) at A[(9 r + c) ld].  The variable of
// step s for the free column fc is -A(prow_s, fc) / A(prow_s, pcol_s); false when a pivot is 0 or not finite
template <int R>
__device__ __forceinline__ bool vf_eliminate(double* A, int ld, unsigned& cused, unsigned& prow, unsigned& pcol) {
  unsigned rused = 0u;
  cused = 0u; prow = 0u; pcol = 0u;
#pragma unroll 1
  for (int s = 0; s < R; ++s) {
    int pr = -1, pc = -1;
    double best = 0.0;
#pragma unroll 1
    for (int r = 0; r < R; ++r) {
      if ((rused >> r) & 1u) continue;
      for (int c = 0; c < 9; ++c) {
        if ((cused >> c) & 1u) continue;
        const double a = fabs(A[(9 * r + c) * ld]);
        if (a > best) { best = a; pr = r; pc = c; }
      }
    }
    if (pr < 0 || !isfinite(best)) return false;
    rused |= 1u << pr;
    cused |= 1u << pc;
    prow |= (unsigned)pr << (4 * s);
    pcol |= (unsigned)pc << (4 * s);
    const double piv = A[(9 * pr + pc) * ld];
#pragma unroll 1
    for (int r = 0; r < R; ++r) {
      if (r == pr) continue;
      const double m = A[(9 * r + pc) * ld] / piv;
      for (int c = 0; c < 9; ++c) A[(9 * r + c) * ld] -= m * A[(9 * pr + c) * ld];
    }
  }
  return true;
}

// F_h of the specification through eight correspondences of the dense array; A: 72 doubles of LDS at stride ld (vf_eliminate)
__device__ bool fundamental8_dense(const float4* __restrict__ corr, const int (&idx)[8], double* A, int ld, double (&F)[9]) {
  double cx = 0.0, cy = 0.0, cu = 0.0, cv = 0.0;
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    const float4 c = corr[idx[k]];
    cx += (double)c.x; cy += (double)c.y; cu += (double)c.z; cv += (double)c.w;
  }
  cx = cx / 8.0; cy = cy / 8.0; cu = cu / 8.0; cv = cv / 8.0;
  double m0 = 0.0, m1 = 0.0;
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    const float4 c = corr[idx[k]];
    const double px = c.x, py = c.y, pu = c.z, pv = c.w;
    m0 += sqrt((px - cx) * (px - cx) + (py - cy) * (py - cy));
    m1 += sqrt((pu - cu) * (pu - cu) + (pv - cv) * (pv - cv));
  }
  m0 = m0 / 8.0; m1 = m1 / 8.0;
  const double s0 = m0 == 0.0 ? 1.0 : sqrt(2.0) / m0, s1 = m1 == 0.0 ? 1.0 : sqrt(2.0) / m1;
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    const float4 c = corr[idx[k]];
    const double x = ((double)c.x - cx) * s0, y = ((double)c.y - cy) * s0, u = ((double)c.z - cu) * s1, v = ((double)c.w - cv) * s1;
    const double row[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
#pragma unroll
    for (int q = 0; q < 9; ++q) A[(9 * k + q) * ld] = row[q];
  }
  // the null vector: the column without a pivot is the free variable and keeps the value 1
  unsigned cused, prow, pcol;
  if (!vf_eliminate<8>(A, ld, cused, prow, pcol)) return false;
  const int fc = __ffs((int)(~cused & 0x1ffu)) - 1;          // eight of nine bits are set: 0 <= fc <= 8
  double fn[9];
  bool fin = true;
#pragma unroll
  for (int c = 0; c < 9; ++c) fn[c] = 1.0;
  for (int s = 0; s < 8; ++s) {
    const int pr = (prow >> (4 * s)) & 15, pc = (pcol >> (4 * s)) & 15;
    const double val = -A[(9 * pr + fc) * ld] / A[(9 * pr + pc) * ld];
    fin = fin && isfinite(val);
#pragma unroll
    for (int c = 0; c < 9; ++c) fn[c] = c == pc ? val : fn[c];
  }
  if (!fin) return false;
  vf_denormalise(fn, cx, cy, s0, cu, cv, s1, F);
  return vf_unit(F);
}

// ---------------------------------------------------------------------------------------------- sums over the correspondences, refits
// the per-thread sums of a sweep over the correspondences, reduced across each wave into one LDS row per wave; after the caller's barrier
// thread 0 adds the 16 rows in wave order (vf_total)
template <int N>
__device__ __forceinline__ void vf_partials(const double (&acc)[N], double (*s_acc)[VF_ACC]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = 0; c < N; ++c) {
    double s = acc[c];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) s_acc[wave][c] = s;
  }
}
__device__ __forceinline__ double vf_total(const double (*s_acc)[VF_ACC], int c) {
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
// thread 0: the reduced normal equations -> solve8; true and h[0..7] when the solve succeeds with finite entries.  Out of line: its two
// callers in verify_finish_kernel (the lo_iters == 0 refit and HomographyModel::refit) then share one 8 x 9 array of scratch
__device__ __noinline__ bool vf_normal_solve(const double (*s_acc)[VF_ACC], double (&h)[8]) {
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
// the 45 sums a_i a_j (i <= j) that one normalised correspondence adds
__device__ __forceinline__ void vf_epipolar_add(double (&acc)[45], double x, double y, double u, double v) {
  const double a[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
  int q = 0;
  for (int i = 0; i < 9; ++i)
    for (int j = i; j < 9; ++j) acc[q++] += a[i] * a[j];
}

// jacobi(S) of the specification on an n x n symmetric matrix held in LDS (leading dimension 9): the eigenvector of the smallest
// eigenvalue.  One thread; S is destroyed, V receives all eigenvectors.
__device__ void vf_jacobi(double (*S)[9], double (*V)[9], int n, double* vec) {
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < VF_JACOBI_SWEEPS; ++sweep)
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = S[p][q];
        if (apq == 0.0) continue;
        const double d = S[q][q] - S[p][p], b = 2.0 * apq;
        const double tn = (d >= 0.0 ? b : -b) / (fabs(d) + hypot(d, b));
        const double cs = 1.0 / sqrt(tn * tn + 1.0), sn = tn * cs;
        for (int k = 0; k < n; ++k) {
          const double akp = S[k][p], akq = S[k][q];
          S[k][p] = cs * akp - sn * akq;
          S[k][q] = sn * akp + cs * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = S[p][k], aqk = S[q][k];
          S[p][k] = cs * apk - sn * aqk;
          S[q][k] = sn * apk + cs * aqk;
        }
        S[p][q] = 0.0;
        S[q][p] = 0.0;
        for (int k = 0; k < n; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = cs * vkp - sn * vkq;
          V[k][q] = sn * vkp + cs * vkq;
        }
      }
  int m = 0;
  for (int k = 1; k < n; ++k)
    if (S[k][k] < S[m][m]) m = k;
  for (int k = 0; k < n; ++k) vec[k] = V[k][m];
}

// rank2(F) of the specification (one thread; S, V: the LDS of vf_jacobi)
__device__ void vf_rank2(double (&F)[9], double (*S)[9], double (*V)[9]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) S[i][j] = F[i] * F[j] + F[3 + i] * F[3 + j] + F[6 + i] * F[6 + j];
  double v[3];
  vf_jacobi(S, V, 3, v);
  double G[9];
  for (int r = 0; r < 3; ++r) {
    const double fv = F[3 * r] * v[0] + F[3 * r + 1] * v[1] + F[3 * r + 2] * v[2];
    for (int c = 0; c < 3; ++c) G[3 * r + c] = F[3 * r + c] - fv * v[c];
  }
  if (vf_unit(G))
    for (int c = 0; c < 9; ++c) F[c] = G[c];
}

// v1, v2, v3 of the specification's svd(E) (v3 at the smallest eigenvalue of E^T E), w1 = E v1, w2 = E v2 and their lengths (one thread;
// S, V: the LDS of vf_jacobi)
__device__ void vp_svd(const double (&E)[9], double (*S)[9], double (*V)[9], double (&v)[3][3], double (&w)[2][3], double (&s)[2]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) S[i][j] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];
  double unused[3];
  vf_jacobi(S, V, 3, unused);
  int m = 0;
  for (int k = 1; k < 3; ++k)
    if (S[k][k] < S[m][m]) m = k;
  const int a = m == 0 ? 1 : 0, b = m == 2 ? 1 : 2;
  for (int k = 0; k < 3; ++k) { v[0][k] = V[k][a]; v[1][k] = V[k][b]; v[2][k] = V[k][m]; }
  for (int q = 0; q < 2; ++q) {
    for (int r = 0; r < 3; ++r) w[q][r] = E[3 * r] * v[q][0] + E[3 * r + 1] * v[q][1] + E[3 * r + 2] * v[q][2];
    s[q] = sqrt(w[q][0] * w[q][0] + w[q][1] * w[q][1] + w[q][2] * w[q][2]);
  }
}

// ess(E) of the specification: singular values (1, 1, 0), unit norm; E itself when that fails
__device__ void vp_ess(double (&E)[9], double (*S)[9], double (*V)[9]) {
  double v[3][3], w[2][3], s[2];
  vp_svd(E, S, V, v, w, s);
  if (!(s[0] > 0.0 && s[1] > 0.0)) return;
  double G[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) G[3 * r + c] = w[0][r] * v[0][c] / s[0] + w[1][r] * v[1][c] / s[1];
  if (vf_unit(G))
    for (int c = 0; c < 9; ++c) E[c] = G[c];
}

// camera coordinates of a correspondence: (x - cx) / fx, (y - cy) / fy for cam = fx0, fy0, cx0, cy0, fx1, fy1, cx1, cy1
__device__ __forceinline__ void vp_norm(const float4 c, const double (&cam)[8], double& x, double& y, double& u, double& v) {
  x = ((double)c.x - cam[2]) / cam[0];
  y = ((double)c.y - cam[3]) / cam[1];
  u = ((double)c.z - cam[6]) / cam[4];
  v = ((double)c.w - cam[7]) / cam[5];
}

// ---------------------------------------------------------------------------------------------- the models
// What the shared code below is templated on.  MIN: the least number of inliers a refit takes (and of correspondences a hypothesis of
// the homography and the fundamental model takes; a pose set needs five, which its kernels check); NACC: the sums of a refit;
// coords: the coordinates a correspondence is judged in (cam is read by the pose model only); inlier; add: what one normalised inlier
// adds to the NACC sums; refit: thread 0's solve of the reduced sums (S, V: the LDS of vf_jacobi) and the way back through the
// similarities (cx, cy, sc0), (cu, cv, sc1) into out, false when there is no finite candidate; minimal: the model of hypothesis hyp.
struct HomographyModel {
  static constexpr int MIN = 4, NACC = 44;
  static __device__ __forceinline__ void coords(const float4 c, const double (&)[8], double& x, double& y, double& u, double& v) {
    x = c.x; y = c.y; u = c.z; v = c.w;
  }
  static __device__ __forceinline__ bool inlier(const double (&H)[9], double x, double y, double u, double v, double t2) {
    return reproj2(H, x, y, u, v) <= t2;
  }
  static __device__ __forceinline__ void add(double (&acc)[44], double x, double y, double u, double v) { vf_normal_add(acc, x, y, u, v); }
  static __device__ __forceinline__ bool minimal(const float4* __restrict__ corr, uint64_t seed, int hyp, int K, double*, int, double (&H)[9]) {
    int idx[4];
    ransac_sample(seed, hyp, K, idx);
    return homography4_dense(corr, idx, H);
  }
  static __device__ __forceinline__ bool refit(const double (*s_acc)[VF_ACC], double (*)[9], double (*)[9], double cx, double cy, double sc0,
                                               double cu, double cv, double sc1, double* out) {
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
        for (int c = 0; c < 9; ++c) out[c] = Hd[c];
      }
    }
    return ok;
  }
};

// x1^T M x0 = 0 with the Sampson distance: the fundamental matrix on pixel coordinates, made rank 2, and (CALIBRATED) the essential
// matrix on camera coordinates, projected onto the essential manifold
template <bool CALIBRATED>
struct EpipolarModel {
  static constexpr int MIN = 8, NACC = 45;
  static __device__ __forceinline__ void coords(const float4 c, const double (&cam)[8], double& x, double& y, double& u, double& v) {
    if constexpr (CALIBRATED) {
      vp_norm(c, cam, x, y, u, v);
    } else {
      x = c.x; y = c.y; u = c.z; v = c.w;
    }
  }
  static __device__ __forceinline__ bool inlier(const double (&F)[9], double x, double y, double u, double v, double t2) {
    return sampson_in(F, x, y, u, v, t2);
  }
  static __device__ __forceinline__ void add(double (&acc)[45], double x, double y, double u, double v) { vf_epipolar_add(acc, x, y, u, v); }
  // rank2(F) or ess(E) of the specification (one thread)
  static __device__ __forceinline__ void project(double (&F)[9], double (*S)[9], double (*V)[9]) {
    if constexpr (CALIBRATED) vp_ess(F, S, V);
    else vf_rank2(F, S, V);
  }
  // the 9 x 9 matrix of sums, its smallest eigenvector, back through the similarities, unit norm, the projection
  static __device__ __forceinline__ bool refit(const double (*s_acc)[VF_ACC], double (*S)[9], double (*V)[9], double cx, double cy, double sc0,
                                               double cu, double cv, double sc1, double* out) {
    int q = 0;
    for (int i = 0; i < 9; ++i)
      for (int j = i; j < 9; ++j) {
        const double s = vf_total(s_acc, q);
        S[i][j] = s; S[j][i] = s;
        ++q;
      }
    double fn[9], Fd[9];
    vf_jacobi(S, V, 9, fn);
    vf_denormalise(fn, cx, cy, sc0, cu, cv, sc1, Fd);
    const bool ok = vf_unit(Fd);
    if (ok) {
      project(Fd, S, V);
      for (int c = 0; c < 9; ++c) out[c] = Fd[c];
    }
    return ok;
  }
};
struct FundamentalModel : EpipolarModel<false> {
  // eight indices: the four of the homography's sample, then four more.  A: 72 doubles of LDS at stride ld
  static __device__ __forceinline__ bool minimal(const float4* __restrict__ corr, uint64_t seed, int hyp, int K, double* A, int ld, double (&F)[9]) {
    int idx[8];
    ransac_sample(seed, hyp, K, idx);
    return fundamental8_dense(corr, idx, A, ld, F);
  }
};
using PoseModel = EpipolarModel<true>;           // its hypotheses are the five-point solver's: up to ten models per sample, no `minimal`

// ---------------------------------------------------------------------------------------------- scoring
// Scores the models in the rows g0 .. min(g0 + VF_HB, M) - 1 of s_M (LDS) against the K correspondences of the set, by the whole
// workgroup of 256: every thread takes one correspondence per tile and keeps VF_HB counters in registers; the models are read at
// wave-uniform LDS addresses.  Leaves the sums of wave w in s_cnt[w][0 .. VF_HB - 1]; the caller's barrier publishes them.
template <class Model>
__device__ __forceinline__ void vf_score(const VerifyDev& e, int K, const double (&cam)[8], double t2, const double (*s_M)[10], int g0, int M,
                                         int (*s_cnt)[VF_HB]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int cnt[VF_HB];
#pragma unroll
  for (int b = 0; b < VF_HB; ++b) cnt[b] = 0;
  for (int p0 = 0; p0 < K; p0 += 256) {                  // K is the same for the whole workgroup
    const int p = p0 + t;
    const bool have = p < K;
    double x, y, u, v;
    Model::coords(e.corr[have ? p : 0], cam, x, y, u, v);
#pragma unroll
    for (int b = 0; b < VF_HB; ++b) {
      if (g0 + b < M) {
        double Mb[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) Mb[q] = s_M[g0 + b][q];
        cnt[b] += have && Model::inlier(Mb, x, y, u, v, t2) ? 1 : 0;
      }
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
}

// ---------------------------------------------------------------------------------------------- hypotheses (homography, fundamental)
// The first VF_HB lanes solve one model each (the homography's elimination array is indexed by the pivot search and lives in scratch,
// the fundamental model's in s_A, lane-minor); then vf_score.  hypcount[h] = the score, -1 without a model.
template <class Model>
__device__ __forceinline__ void vf_hypotheses(const VerifyDev& e, int K, int h0, uint64_t seed, int iters, double t2, double (*s_A)[VF_HB],
                                              double (*s_H)[10], int* s_ok, int (*s_cnt)[VF_HB]) {
  const int t = threadIdx.x;
  if (K < Model::MIN) {                                    // the same for every thread of the workgroup
    if (t < VF_HB && h0 + t < iters) e.hypcount[h0 + t] = -1;
    return;
  }
  if (t < VF_HB) {
    double H[9];
    bool ok = false;
    if (h0 + t < iters) ok = Model::minimal(e.corr, seed, h0 + t, K, &s_A[0][t], VF_HB, H);
    for (int c = 0; c < 9; ++c) s_H[t][c] = ok ? H[c] : 0.0;
    s_ok[t] = ok ? 1 : 0;
  }
  __syncthreads();
  const double cam[8] = {};                                // no camera in these models
  vf_score<Model>(e, K, cam, t2, s_H, 0, VF_HB, s_cnt);
  __syncthreads();
  if (t < VF_HB && h0 + t < iters)
    e.hypcount[h0 + t] = s_ok[t] ? s_cnt[0][t] + s_cnt[1][t] + s_cnt[2][t] + s_cnt[3][t] : -1;
}

// one workgroup per VF_HB hypotheses of one set.  The register budget is stated (8 waves per SIMD: 64 VGPRs, which the kernel meets
// without a spill): left to itself the scheduler spreads the constant rows of the four-point system over 62 to 84 registers, depending
// on code that has nothing to do with them
__global__ __launch_bounds__(256, 8) void verify_hyp_kernel(const VerifyDev* __restrict__ vs, uint64_t seed, int iters, double t2) {
  __shared__ double s_A[72][VF_HB];                       // the elimination arrays of the VF_HB lanes that solve a fundamental matrix
  __shared__ double s_H[VF_HB][10];
  __shared__ int s_ok[VF_HB];
  __shared__ int s_cnt[4][VF_HB];
  const VerifyDev& e = vs[blockIdx.y];
  const int K = e.nvalid[0];
  const int h0 = blockIdx.x * VF_HB;
  if (e.model == GIMS_VERIFY_MODEL_FUNDAMENTAL)             // per set: the same for every thread of the workgroup
    vf_hypotheses<FundamentalModel>(e, K, h0, seed, iters, t2, s_A, s_H, s_ok, s_cnt);
  else
    vf_hypotheses<HomographyModel>(e, K, h0, seed, iters, t2, s_A, s_H, s_ok, s_cnt);
}

// ---------------------------------------------------------------------------------------------- the pieces of a finish kernel
// The best hypothesis of a set -- highest hypcount >> SHIFT, lowest index among equals -- by a workgroup of 1024.  Ends behind a barrier;
// only thread 0 returns the result in (bc, bh): bc the counter itself (-1 when no hypothesis has a model, or iters == 0).
template <int SHIFT>
__device__ __forceinline__ void vf_best(const VerifyDev& e, int iters, int (*s_best)[2], int& bc, int& bh) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  bc = -1; bh = 0x7fffffff;
  for (int h = t; h < iters; h += 1024) {
    const int c = e.hypcount[h];
    if ((c >> SHIFT) > (bc >> SHIFT)) { bc = c; bh = h; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int oc = __shfl_xor(bc, o, 64), oh = __shfl_xor(bh, o, 64);
    if ((oc >> SHIFT) > (bc >> SHIFT) || ((oc >> SHIFT) == (bc >> SHIFT) && oh < bh)) { bc = oc; bh = oh; }
  }
  if (lane == 0) { s_best[wave][0] = bc; s_best[wave][1] = bh; }
  __syncthreads();
  if (t == 0)
    for (int w = 1; w < 16; ++w)
      if ((s_best[w][0] >> SHIFT) > (bc >> SHIFT) || ((s_best[w][0] >> SHIFT) == (bc >> SHIFT) && s_best[w][1] < bh)) {
        bc = s_best[w][0]; bh = s_best[w][1];
      }
}

// the outputs of a set without a model (the mask was cleared by the gather kernel); width: the floats of its model output
__device__ __forceinline__ void vf_no_model(const VerifyDev& e, int K, int width) {
  if (threadIdx.x == 0) {
    for (int c = 0; c < 8; ++c) e.record[c] = 0.f;
    e.record[VF_NVALID] = (float)K;
    e.record[VF_ERR_CORNER] = -1.f;
    for (int c = 0; c < width; ++c) e.hom[c] = 0.f;
  }
}

// the sign rule of the specification: the factor that makes the entry of largest magnitude (the first such) positive
__device__ __forceinline__ double vf_sign(const double (&F)[9]) {
  int m = 0;
  for (int c = 1; c < 9; ++c)
    if (fabs(F[c]) > fabs(F[m])) m = c;
  return F[m] < 0.0 ? -1.0 : 1.0;
}

// the LDS state of stage 2, one per finish kernel.  Thread 0 stores M (the model of the best hypothesis), stop = 0 and rounds = 0 before
// the barrier in front of vf_local_opt
struct VfLo {
  double M[9];             // the accepted model
  double Mn[9];            // the candidate of the current round
  double norm[6];          // cx, cy, cu, cv, scale0, scale1
  double S[9][9], V[9][9]; // thread 0's eigen-solves (and, before stage 2, the elimination array of its minimal solve)
  double nprev;            // |I_{l-1}|
  int stop, rounds;
};

// The guarded local optimisation of the specification, by a workgroup of 1024: |I_0|, then per round (a) the centroids of the inliers of
// the accepted model, (b) their mean distances to them, (c) the model's sums over the normalised inliers and thread 0's refit, (d) the
// candidate's inliers against the accepted model's; the candidate is accepted unless it has fewer.  Stops after lo_iters rounds, when
// fewer than Model::MIN inliers are left, when a refit fails, when a candidate is refused, or (accepted) when the inlier set repeats.
//
// THE RULE ON BARRIERS, which holds in this function and in the kernels that call it: every decision is taken by thread 0, stored in LDS
// and read by all threads after the barrier that follows; the next store to the same word comes after a later barrier.  No barrier sits
// under a condition that is not one of those words, a kernel argument or a per-set constant.
//
// Returns behind a barrier that follows thread 0's last stores to lo.M and lo.rounds (lo_iters <= 0: nothing is done).
template <class Model>
__device__ __forceinline__ void vf_local_opt(const VerifyDev& e, int K, const double (&cam)[8], double t2, int lo_iters, VfLo& lo,
                                             double (*s_acc)[VF_ACC]) {
  if (lo_iters <= 0) return;
  const int t = threadIdx.x;
  constexpr double least = Model::MIN;
  double F[9];
  for (int c = 0; c < 9; ++c) F[c] = lo.M[c];
  {  // |I_0|
    double a[1] = {0.0};
    for (int p = t; p < K; p += 1024) {
      double x, y, u, v;
      Model::coords(e.corr[p], cam, x, y, u, v);
      a[0] += Model::inlier(F, x, y, u, v, t2) ? 1.0 : 0.0;
    }
    vf_partials(a, s_acc);
    __syncthreads();
    if (t == 0) lo.nprev = vf_total(s_acc, 0);
    __syncthreads();
  }
  for (int l = 1; l <= lo_iters; ++l) {
    // (a) centroids of the inliers of the accepted model
    {
      double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      for (int p = t; p < K; p += 1024) {
        double x, y, u, v;
        Model::coords(e.corr[p], cam, x, y, u, v);
        if (Model::inlier(F, x, y, u, v, t2)) { a[0] += 1.0; a[1] += x; a[2] += y; a[3] += u; a[4] += v; }
      }
      vf_partials(a, s_acc);
    }
    __syncthreads();
    if (t == 0) {
      const double n = vf_total(s_acc, 0);
      lo.stop = n < least ? 1 : 0;
      if (n >= least)
        for (int c = 0; c < 4; ++c) lo.norm[c] = vf_total(s_acc, 1 + c) / n;
    }
    __syncthreads();
    if (lo.stop) break;
    const double cx = lo.norm[0], cy = lo.norm[1], cu = lo.norm[2], cv = lo.norm[3];
    // (b) mean distances to the centroids
    {
      double a[3] = {0.0, 0.0, 0.0};
      for (int p = t; p < K; p += 1024) {
        double x, y, u, v;
        Model::coords(e.corr[p], cam, x, y, u, v);
        if (Model::inlier(F, x, y, u, v, t2)) {
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
      lo.norm[4] = m0 == 0.0 ? 1.0 : sqrt(2.0) / m0;
      lo.norm[5] = m1 == 0.0 ? 1.0 : sqrt(2.0) / m1;
    }
    __syncthreads();
    const double sc0 = lo.norm[4], sc1 = lo.norm[5];
    // (c) the model's sums over the normalised inliers, thread 0's refit and the way back to the coordinates of the inlier test
    {
      double acc[Model::NACC];
      for (int c = 0; c < Model::NACC; ++c) acc[c] = 0.0;
      for (int p = t; p < K; p += 1024) {
        double x, y, u, v;
        Model::coords(e.corr[p], cam, x, y, u, v);
        if (Model::inlier(F, x, y, u, v, t2)) Model::add(acc, (x - cx) * sc0, (y - cy) * sc0, (u - cu) * sc1, (v - cv) * sc1);
      }
      vf_partials(acc, s_acc);
    }
    __syncthreads();
    if (t == 0) lo.stop = Model::refit(s_acc, lo.S, lo.V, cx, cy, sc0, cu, cv, sc1, lo.Mn) ? 0 : 1;
    __syncthreads();
    if (lo.stop) break;
    double Fc[9];
    for (int c = 0; c < 9; ++c) Fc[c] = lo.Mn[c];
    // (d) the candidate's inliers against the accepted model's
    {
      double a[2] = {0.0, 0.0};
      for (int p = t; p < K; p += 1024) {
        double x, y, u, v;
        Model::coords(e.corr[p], cam, x, y, u, v);
        const bool was = Model::inlier(F, x, y, u, v, t2), is = Model::inlier(Fc, x, y, u, v, t2);
        a[0] += is ? 1.0 : 0.0;
        a[1] += is != was ? 1.0 : 0.0;
      }
      vf_partials(a, s_acc);
    }
    __syncthreads();
    if (t == 0) {
      const double n = vf_total(s_acc, 0), changed = vf_total(s_acc, 1);
      if (n < lo.nprev) {
        lo.stop = 1;                                    // fewer inliers: keep the model of round l - 1
      } else {
        for (int c = 0; c < 9; ++c) lo.M[c] = lo.Mn[c];
        lo.nprev = n;
        lo.rounds = lo.rounds + 1;
        lo.stop = changed == 0.0 ? 2 : 0;               // accepted; the same set again: converged
      }
    }
    __syncthreads();
    const int stop = lo.stop;
    if (stop != 1)
      for (int c = 0; c < 9; ++c) F[c] = Fc[c];
    if (stop) break;
  }
}

// The final sweep: the mask under the model F, the inlier count in column 0 of the NSUM sums -- an inlier may add to the others through
// extra(a, x, y, u, v) --, a barrier, and thread 0 writes the record (err_corner = -1).  score: the inliers of the best hypothesis bh
struct VfNoExtra {
  __device__ __forceinline__ void operator()(double (&)[1], double, double, double, double) const {}
};
template <class Model, int NSUM, class Extra>
__device__ __forceinline__ void vf_final_sweep(const VerifyDev& e, int K, const double (&cam)[8], double t2, const double (&F)[9], int bh, int score,
                                               const VfLo& lo, double (*s_acc)[VF_ACC], Extra extra) {
  const int t = threadIdx.x;
  {
    double a[NSUM];
    for (int c = 0; c < NSUM; ++c) a[c] = 0.0;
    for (int p = t; p < K; p += 1024) {
      double x, y, u, v;
      Model::coords(e.corr[p], cam, x, y, u, v);
      const bool in = Model::inlier(F, x, y, u, v, t2);
      e.inlier[e.rows[p]] = in ? 1 : 0;
      if (in) {
        a[0] += 1.0;
        extra(a, x, y, u, v);
      }
    }
    vf_partials(a, s_acc);
  }
  __syncthreads();
  if (t == 0) {
    e.record[VF_NVALID] = (float)K;
    e.record[VF_OK] = 1.f;
    e.record[VF_NINLIERS] = (float)vf_total(s_acc, 0);
    e.record[VF_BEST_HYP] = (float)bh;
    e.record[VF_BEST_HYP_INLIERS] = (float)score;
    e.record[VF_LO_ROUNDS] = (float)lo.rounds;
    e.record[VF_ERR_CORNER] = -1.f;
    e.record[VF_RESERVED] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------- finish (homography, fundamental)
// thread 0 solves the best hypothesis (bc, bh) again into lo.M; true, for every thread and behind a barrier, when the set has a model
template <class Model>
__device__ __forceinline__ bool vf_best_model(const VerifyDev& e, int K, int bc, int bh, uint64_t seed, VfLo& lo, int* s_flag) {
  if (threadIdx.x == 0) {
    s_flag[0] = 0; s_flag[1] = 0;
    lo.stop = 0; lo.rounds = 0;
    if (bc >= 0 && K >= Model::MIN) {
      double M[9];
      if (Model::minimal(e.corr, seed, bh, K, &lo.S[0][0], 1, M)) {
        for (int c = 0; c < 9; ++c) lo.M[c] = M[c];
        s_flag[0] = 1;
      }
    }
  }
  __syncthreads();
  return s_flag[0] != 0;
}

// one workgroup per set: best hypothesis (most inliers, first such), stage 2, final mask, record
__global__ __launch_bounds__(1024) void verify_finish_kernel(const VerifyDev* __restrict__ vs, uint64_t seed, int iters, int lo_iters, double t2) {
  __shared__ int s_best[16][2];
  __shared__ double s_acc[16][VF_ACC];
  __shared__ VfLo s_lo;
  __shared__ int s_flag[2];          // 0: the set has a model; 1: the inlier count of the lo_iters == 0 refit
  const VerifyDev& e = vs[blockIdx.x];
  const int t = threadIdx.x;
  const int K = e.nvalid[0];
  const double cam[8] = {};          // no camera in these models
  int bc, bh;
  vf_best<0>(e, iters, s_best, bc, bh);
  double F[9];
  if (e.model == GIMS_VERIFY_MODEL_FUNDAMENTAL) {           // per set: the same for every thread of the workgroup
    if (!vf_best_model<FundamentalModel>(e, K, bc, bh, seed, s_lo, s_flag)) {
      vf_no_model(e, K, 9);
      return;
    }
    vf_local_opt<FundamentalModel>(e, K, cam, t2, lo_iters, s_lo, s_acc);
    // no accepted round (lo_iters == 0 has none): the model is the best hypothesis made rank 2
    if (s_lo.rounds == 0) {
      if (t == 0) {
        double G[9];
        for (int c = 0; c < 9; ++c) G[c] = s_lo.M[c];
        FundamentalModel::project(G, s_lo.S, s_lo.V);
        for (int c = 0; c < 9; ++c) s_lo.M[c] = G[c];
      }
      __syncthreads();
    }
    for (int c = 0; c < 9; ++c) F[c] = s_lo.M[c];
    vf_final_sweep<FundamentalModel, 1>(e, K, cam, t2, F, bh, bc, s_lo, s_acc, VfNoExtra());
    if (t == 0) {
      const double sg = vf_sign(F);
      for (int c = 0; c < 9; ++c) e.hom[c] = (float)(sg * F[c]);
    }
    return;
  }
  if (!vf_best_model<HomographyModel>(e, K, bc, bh, seed, s_lo, s_flag)) {
    vf_no_model(e, K, 9);
    return;
  }
  if (lo_iters == 0) {
    // the single unguarded refit of gims_eval_pairs: normal equations over the inliers of the best hypothesis, raw coordinates
    for (int c = 0; c < 9; ++c) F[c] = s_lo.M[c];
    double acc[44];
    for (int c = 0; c < 44; ++c) acc[c] = 0.0;
    int nin = 0;
    for (int p = t; p < K; p += 1024) {
      const float4 c4 = e.corr[p];
      const double x = c4.x, y = c4.y, u = c4.z, v = c4.w;
      if (reproj2(F, x, y, u, v) <= t2) {
        ++nin;
        vf_normal_add(acc, x, y, u, v);
      }
    }
    vf_partials(acc, s_acc);
    atomicAdd(&s_flag[1], nin);
    __syncthreads();
    if (t == 0) {
      double h[8];
      if (s_flag[1] >= 4 && vf_normal_solve(s_acc, h)) {
        for (int c = 0; c < 8; ++c) s_lo.M[c] = h[c];
        s_lo.M[8] = 1.0;
      }
    }
    __syncthreads();
  } else {
    vf_local_opt<HomographyModel>(e, K, cam, t2, lo_iters, s_lo, s_acc);
  }
  for (int c = 0; c < 9; ++c) F[c] = s_lo.M[c];
  vf_final_sweep<HomographyModel, 1>(e, K, cam, t2, F, bh, bc, s_lo, s_acc, VfNoExtra());
  if (t == 0) {
    if (e.has_ref) e.record[VF_ERR_CORNER] = corner_error(F, e.href, e.height, e.width);
    for (int c = 0; c < 9; ++c) e.hom[c] = (float)F[c];
  }
}

// ---------------------------------------------------------------------------------------------- calibrated relative pose (model 3)
// The five-point model and the pose of the result (specification: include/gims_hip.h).  Pose sets run in two kernels of
// their own, built from the pieces above; the gather kernel is shared.
constexpr int VP_MAXM = 10;        // models of one sample: the real roots of a degree-10 polynomial
constexpr int VP_BISECT = 80;      // halvings per isolated root
constexpr int VP_A = 200;          // the 10 x 20 elimination array (the 5 x 9 one before it lives in the same words)

// the best model of workgroup b of the hypotheses kernel: 9 doubles behind the `iters` counters of a pose set (verify_layout)
__device__ __forceinline__ double* vp_block_model(const VerifyDev& e, int iters, int b) {
  return (double*)(e.hypcount + ((iters + 1) & ~1)) + 9 * b;
}

// variables 0: x, 1: y, 2: z, 3: the constant 1.  A quadratic form has ten coefficients (i <= j), a cubic one twenty; the column of
// x^a y^b z^c among the twenty is base[a][b] + (3 - a - b - c):
//   x^3 y^3 x^2y xy^2 | x^2z x^2 | y^2z y^2 | xyz xy | xz^2 xz x | yz^2 yz y | z^3 z^2 z 1
__device__ __forceinline__ constexpr int vp_qi(int i, int j) { return i <= j ? 4 * i - i * (i - 1) / 2 + (j - i) : 4 * j - j * (j - 1) / 2 + (i - j); }
__device__ __forceinline__ constexpr int vp_col(int i, int j, int k) {
  const int a = (i == 0) + (j == 0) + (k == 0), b = (i == 1) + (j == 1) + (k == 1), c = (i == 2) + (j == 2) + (k == 2);
  const int base = a == 0 ? (b == 0 ? 16 : b == 1 ? 13 : b == 2 ? 6 : 1) : a == 1 ? (b == 0 ? 10 : b == 1 ? 8 : 3) : a == 2 ? (b == 0 ? 4 : 2) : 0;
  return base + (3 - a - b - c);
}
// q += s * (a * b) for two linear forms
__device__ __forceinline__ void vp_ll(const double* a, const double* b, double s, double (&q)[10]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) q[vp_qi(i, j)] += s * (a[i] * b[j]);
}
// row += s * (q * l) for a quadratic and a linear form
__device__ __forceinline__ void vp_ql(const double (&q)[10], const double* l, double s, double (&row)[20]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) row[vp_col(i, j, k)] += s * (q[vp_qi(i, j)] * l[k]);
}
// (vp_pmul and vp_horner, the polynomial product and evaluation, live in eval_geom.h: csrc/resect.hip uses them too)

// the real roots of the degree-10 polynomial c (ascending coefficients), ascending, by bisection between the roots of successive
// derivatives inside the bound 1 + max |c_i / c_10|; -1 when c_10 is 0 or anything is not finite
__device__ int vp_real_roots(const double (&c)[11], double (&roots)[VP_MAXM]) {
  bool fin = c[10] != 0.0;
  double bound = 0.0;
  for (int i = 0; i < 11; ++i) fin = fin && isfinite(c[i]);
  if (!fin) return -1;
  for (int i = 0; i < 10; ++i) bound = fmax(bound, fabs(c[i] / c[10]));
  bound = 1.0 + bound;
  if (!isfinite(bound)) return -1;
  double prev[VP_MAXM], q[11];
  int nprev = 0;
#pragma unroll 1
  for (int d = 1; d <= 10; ++d) {
    const int k = 10 - d;
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
        double a = lo, b = hi;
#pragma unroll 1
        for (int it = 0; it < VP_BISECT; ++it) {
          const double m = 0.5 * (a + b);
          const bool same = (vp_horner(q, d, m) > 0.0) == sa;
          a = same ? m : a;
          b = same ? b : m;
        }
        roots[ncur++] = 0.5 * (a + b);                     // at most one root per interval: ncur <= d
      }
      lo = hi;
      flo = fhi;
    }
    nprev = ncur;
    for (int s = 0; s < ncur; ++s) prev[s] = roots[s];
  }
  return nprev;
}

// the ten cubic constraints of E = x X + y Y + z Z + W as 10 x 20 coefficients in A and their Gauss-Jordan elimination over the columns
// 0 .. 9; prow10: four bits per column, the row of its pivot.  Returns the smallest pivot magnitude, -1 when the elimination fails
__device__ double vp_constraints_eliminate(const double (&L)[9][4], double* A, int ld, uint64_t& prow10) {
  // the ten cubic constraints: det E, then the entries of 2 E E^T E - tr(E E^T) E by rows, as 10 x 20 coefficients in A
  {
    double q[10], row[20];
    for (int c = 0; c < 20; ++c) row[c] = 0.0;
    for (int c = 0; c < 10; ++c) q[c] = 0.0;
    vp_ll(L[4], L[8], 1.0, q); vp_ll(L[5], L[7], -1.0, q); vp_ql(q, L[0], 1.0, row);
    for (int c = 0; c < 10; ++c) q[c] = 0.0;
    vp_ll(L[3], L[8], 1.0, q); vp_ll(L[5], L[6], -1.0, q); vp_ql(q, L[1], -1.0, row);
    for (int c = 0; c < 10; ++c) q[c] = 0.0;
    vp_ll(L[3], L[7], 1.0, q); vp_ll(L[4], L[6], -1.0, q); vp_ql(q, L[2], 1.0, row);
    for (int c = 0; c < 20; ++c) A[c * ld] = row[c];
  }
  {
    double G[3][3][10], T[10];
#pragma unroll 1
    for (int i = 0; i < 3; ++i)
#pragma unroll 1
      for (int j = 0; j < 3; ++j) {
        double q[10];
        for (int c = 0; c < 10; ++c) q[c] = 0.0;
        for (int k = 0; k < 3; ++k) vp_ll(L[3 * i + k], L[3 * j + k], 1.0, q);
        for (int c = 0; c < 10; ++c) G[i][j][c] = q[c];
      }
    for (int c = 0; c < 10; ++c) T[c] = G[0][0][c] + G[1][1][c] + G[2][2][c];
#pragma unroll 1
    for (int i = 0; i < 3; ++i)
#pragma unroll 1
      for (int j = 0; j < 3; ++j) {
        double row[20], q[10];
        for (int c = 0; c < 20; ++c) row[c] = 0.0;
        for (int k = 0; k < 3; ++k) {
          for (int c = 0; c < 10; ++c) q[c] = G[i][k][c];
          vp_ql(q, L[3 * k + j], 2.0, row);
        }
        for (int c = 0; c < 10; ++c) q[c] = T[c];
        vp_ql(q, L[3 * i + j], -1.0, row);
        for (int c = 0; c < 20; ++c) A[(20 * (1 + 3 * i + j) + c) * ld] = row[c];
      }
  }
  // Gauss-Jordan over the columns 0 .. 9, the pivot of column c the largest entry among the rows without one
  prow10 = 0ull;
  double quality = INFINITY;
  {
    unsigned used = 0u;
#pragma unroll 1
    for (int c = 0; c < 10; ++c) {
      int pr = -1;
      double best = 0.0;
      for (int r = 0; r < 10; ++r) {
        if ((used >> r) & 1u) continue;
        const double a = fabs(A[(20 * r + c) * ld]);
        if (a > best) { best = a; pr = r; }
      }
      if (pr < 0 || !isfinite(best)) return -1.0;
      quality = fmin(quality, best);
      used |= 1u << pr;
      prow10 |= (uint64_t)pr << (4 * c);
      const double piv = A[(20 * pr + c) * ld];
#pragma unroll 1
      for (int r = 0; r < 10; ++r) {
        if (r == pr) continue;
        const double m = A[(20 * r + c) * ld] / piv;
        for (int k = 0; k < 20; ++k) A[(20 * r + k) * ld] -= m * A[(20 * pr + k) * ld];
      }
    }
  }
  return quality;
}

// the models of the specification through five correspondences of the dense array, in ascending root order; returns their number.
// A: VP_A doubles of LDS at stride ld (indexed by the pivot searches)
__device__ int vp_five_point(const float4* __restrict__ corr, const int (&idx)[5], const double (&cam)[8], double* A, int ld, double (&E)[VP_MAXM][9]) {
#pragma unroll 1
  for (int k = 0; k < 5; ++k) {
    double x, y, u, v;
    vp_norm(corr[idx[k]], cam, x, y, u, v);
    const double row[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
#pragma unroll
    for (int q = 0; q < 9; ++q) A[(9 * k + q) * ld] = row[q];
  }
  // the null space: five pivots, four free columns
  unsigned cused, prow, pcol;
  if (!vf_eliminate<5>(A, ld, cused, prow, pcol)) return 0;
  // L[e][j]: the coefficient of basis vector j (X, Y, Z, W) in entry e of E -- the linear form E_e in (x, y, z, 1)
  double L[9][4];
  bool fin = true;
  {
    unsigned freec = ~cused & 0x1ffu;
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      const int fc = __ffs((int)freec) - 1;                 // four of nine bits are clear in cused: 0 <= fc <= 8
      freec &= freec - 1u;
      for (int c = 0; c < 9; ++c) L[c][j] = c == fc ? 1.0 : 0.0;
      for (int s = 0; s < 5; ++s) {
        const int pr = (prow >> (4 * s)) & 15, pc = (pcol >> (4 * s)) & 15;
        const double val = -A[(9 * pr + fc) * ld] / A[(9 * pr + pc) * ld];
        fin = fin && isfinite(val);
        L[pc][j] = val;
      }
    }
  }
  if (!fin) return 0;
  // the hidden variable is pivoted: of the three orders of the basis (X, Y, Z) = (b0, b1, b2), (b0, b2, b1), (b2, b1, b0) the one whose
  // elimination has the largest smallest pivot (the first such) is used; W = b3 always
  uint64_t prow10 = 0ull;
  {
    int order = -1;
    double bq = -1.0;
#pragma unroll 1
    for (int o = 0; o < 3; ++o) {
      double Lp[9][4];
      for (int e = 0; e < 9; ++e) {
        Lp[e][0] = o == 2 ? L[e][2] : L[e][0];
        Lp[e][1] = o == 1 ? L[e][2] : L[e][1];
        Lp[e][2] = o == 1 ? L[e][1] : o == 2 ? L[e][0] : L[e][2];
        Lp[e][3] = L[e][3];
      }
      const double q = vp_constraints_eliminate(Lp, A, ld, prow10);
      if (q > bq) { bq = q; order = o; }
    }
    if (order < 0) return 0;
    for (int e = 0; e < 9; ++e) {
      const double l0 = L[e][0], l1 = L[e][1], l2 = L[e][2];
      L[e][0] = order == 2 ? l2 : l0;
      L[e][1] = order == 1 ? l2 : l1;
      L[e][2] = order == 1 ? l1 : order == 2 ? l0 : l2;
    }
    if (order != 2) vp_constraints_eliminate(L, A, ld, prow10);
  }
  // the rows <x^2 z> - z <x^2>, <y^2 z> - z <y^2>, <xyz> - z <xy>: polynomials in z (ascending) that multiply x, y and 1
  double Bz[3][3][5];
  fin = true;
#pragma unroll 1
  for (int r = 0; r < 3; ++r) {
    const int ra = (int)((prow10 >> (4 * (4 + 2 * r))) & 15ull), rb = (int)((prow10 >> (4 * (5 + 2 * r))) & 15ull);
    const double pa = A[(20 * ra + 4 + 2 * r) * ld], pb = A[(20 * rb + 5 + 2 * r) * ld];
    double a[10], b[10];
    for (int k = 0; k < 10; ++k) {
      a[k] = A[(20 * ra + 10 + k) * ld] / pa;
      b[k] = A[(20 * rb + 10 + k) * ld] / pb;
      fin = fin && isfinite(a[k]) && isfinite(b[k]);
    }
    for (int v = 0; v < 2; ++v) {
      const int o = 3 * v;
      Bz[r][v][0] = a[o + 2];
      Bz[r][v][1] = a[o + 1] - b[o + 2];
      Bz[r][v][2] = a[o] - b[o + 1];
      Bz[r][v][3] = -b[o];
      Bz[r][v][4] = 0.0;
    }
    Bz[r][2][0] = a[9];
    Bz[r][2][1] = a[8] - b[9];
    Bz[r][2][2] = a[7] - b[8];
    Bz[r][2][3] = a[6] - b[7];
    Bz[r][2][4] = -b[6];
  }
  if (!fin) return 0;
  // its determinant, expanded along the first row: degree 10
  double c11[11];
  {
    double m1[8], m2[8], t11[11];
    vp_pmul(Bz[1][1], 4, Bz[2][2], 5, m1); vp_pmul(Bz[1][2], 5, Bz[2][1], 4, m2);
    for (int i = 0; i < 8; ++i) m1[i] -= m2[i];
    vp_pmul(Bz[0][0], 4, m1, 8, c11);
    vp_pmul(Bz[1][0], 4, Bz[2][2], 5, m1); vp_pmul(Bz[1][2], 5, Bz[2][0], 4, m2);
    for (int i = 0; i < 8; ++i) m1[i] -= m2[i];
    vp_pmul(Bz[0][1], 4, m1, 8, t11);
    for (int i = 0; i < 11; ++i) c11[i] -= t11[i];
    vp_pmul(Bz[1][0], 4, Bz[2][1], 4, m1); vp_pmul(Bz[1][1], 4, Bz[2][0], 4, m2);
    for (int i = 0; i < 7; ++i) m1[i] -= m2[i];
    vp_pmul(Bz[0][2], 5, m1, 7, t11);
    for (int i = 0; i < 11; ++i) c11[i] += t11[i];
  }
  double roots[VP_MAXM];
  const int nr = vp_real_roots(c11, roots);
  int nm = 0;
#pragma unroll 1
  for (int r = 0; r < nr; ++r) {
    const double z = roots[r];
    double M[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) M[i][j] = vp_horner(Bz[i][j], 4, z);
    double n[3] = {0.0, 0.0, 0.0}, best = -1.0;
    for (int p = 0; p < 3; ++p) {                           // the row pairs (0, 1), (0, 2), (1, 2)
      const int i = p == 2 ? 1 : 0, j = p == 0 ? 1 : 2;
      const double c0 = M[i][1] * M[j][2] - M[i][2] * M[j][1], c1 = M[i][2] * M[j][0] - M[i][0] * M[j][2], c2 = M[i][0] * M[j][1] - M[i][1] * M[j][0];
      if (fabs(c2) > best) { best = fabs(c2); n[0] = c0; n[1] = c1; n[2] = c2; }
    }
    if (n[2] == 0.0) continue;
    const double x = n[0] / n[2], y = n[1] / n[2];
    double e[9];
    for (int q = 0; q < 9; ++q) e[q] = x * L[q][0] + y * L[q][1] + z * L[q][2] + L[q][3];
    if (!vf_unit(e)) continue;
    for (int q = 0; q < 9; ++q) E[nm][q] = e[q];
    ++nm;
  }
  return nm;
}

// one workgroup per VF_HB hypotheses of one pose set: VF_HB lanes solve a sample each (elimination arrays in LDS, lane-minor), the
// models of all samples are packed into LDS and scored VF_HB at a time by vf_score.
// hypcount[h] = 16 score + 15 - (index of the best model): the finish kernel compares the scores and finds the model in the low bits
__global__ __launch_bounds__(256) void verify_pose_hyp_kernel(const VerifyDev* __restrict__ vs, uint64_t seed, int iters, double thresh) {
  __shared__ double s_A[VP_A][VF_HB];
  __shared__ double s_E[VF_HB * VP_MAXM][10];
  __shared__ int s_nm[VF_HB], s_off[VF_HB + 1], s_cnt[4][VF_HB], s_score[VF_HB * VP_MAXM];
  const VerifyDev& e = vs[blockIdx.y];
  const int t = threadIdx.x;
  const int K = e.nvalid[0];
  const int h0 = blockIdx.x * VF_HB;
  if (K < 5) {                                             // the same for every thread of the workgroup
    if (t < VF_HB && h0 + t < iters) e.hypcount[h0 + t] = -1;
    return;
  }
  double cam[8];
  for (int c = 0; c < 8; ++c) cam[c] = (double)e.href[c];
  const double tn = thresh / ((cam[0] + cam[5]) / 2.0), t2 = tn * tn;
  double E[VP_MAXM][9];
  int nm = 0;
  if (t < VF_HB) {
    if (h0 + t < iters) {
      int idx[5];
      ransac_sample(seed, h0 + t, K, idx);
      nm = vp_five_point(e.corr, idx, cam, &s_A[0][t], VF_HB, E);
    }
    s_nm[t] = nm;
  }
  __syncthreads();
  int off = 0;
  if (t < VF_HB) {
    for (int b = 0; b < t; ++b) off += s_nm[b];
    for (int r = 0; r < nm; ++r)
      for (int c = 0; c < 9; ++c) s_E[off + r][c] = E[r][c];
    s_off[t] = off;
    if (t == VF_HB - 1) s_off[VF_HB] = off + nm;
  }
  __syncthreads();
  const int M = s_off[VF_HB];                              // the same for every thread of the workgroup, at most VF_HB * VP_MAXM
  for (int g0 = 0; g0 < M; g0 += VF_HB) {
    vf_score<PoseModel>(e, K, cam, t2, s_E, g0, M, s_cnt);
    __syncthreads();
    if (t < VF_HB && g0 + t < M) s_score[g0 + t] = s_cnt[0][t] + s_cnt[1][t] + s_cnt[2][t] + s_cnt[3][t];
    __syncthreads();
  }
  int enc = -1, br = 0;
  if (t < VF_HB && h0 + t < iters) {
    int best = -1;
    for (int r = 0; r < nm; ++r) {
      const int sc = s_score[off + r];
      if (sc > best) { best = sc; br = r; }
    }
    enc = nm > 0 ? best * 16 + 15 - br : -1;
    e.hypcount[h0 + t] = enc;
  }
  if (t < VF_HB) s_nm[t] = enc;                             // (the model counts were last read before the scoring loop's barriers)
  __syncthreads();
  // the best hypothesis of the workgroup -- highest score, lowest h -- leaves its best model for the finish kernel: the best
  // hypothesis of the set is the best one of its workgroup, so the model that was scored is the model that is refined
  if (t < VF_HB && enc >= 0) {
    bool win = true;
    for (int b = 0; b < VF_HB; ++b) win = win && !((s_nm[b] >> 4) > (enc >> 4) || ((s_nm[b] >> 4) == (enc >> 4) && b < t));
    if (win) {
      double* dst = vp_block_model(e, iters, blockIdx.x);
      for (int c = 0; c < 9; ++c) dst[c] = E[br][c];
    }
  }
}

// the depth numerators of l1 x1 = l0 R x0 + t by least squares: in front of both cameras iff D > 0, n0 > 0 and n1 > 0
__device__ __forceinline__ void vp_depths(const double* R, const double* tv, double x, double y, double u, double v, double& n0, double& n1, double& D) {
  const double a0 = R[0] * x + R[1] * y + R[2], a1 = R[3] * x + R[4] * y + R[5], a2 = R[6] * x + R[7] * y + R[8];
  const double aa = a0 * a0 + a1 * a1 + a2 * a2, bb = u * u + v * v + 1.0, ab = u * a0 + v * a1 + a2;
  const double at = a0 * tv[0] + a1 * tv[1] + a2 * tv[2], bt = u * tv[0] + v * tv[1] + tv[2];
  n0 = ab * bt - bb * at;
  n1 = bt * aa - ab * at;
  D = bb * aa - ab * ab;
}

// one workgroup per pose set: best hypothesis and model, stage 2 on camera coordinates, the mask, the four decompositions and the vote
// of the inliers
__global__ __launch_bounds__(1024) void verify_pose_finish_kernel(const VerifyDev* __restrict__ vs, uint64_t seed, int iters, int lo_iters, double thresh) {
  __shared__ int s_best[16][2];
  __shared__ double s_acc[16][VF_ACC];
  __shared__ VfLo s_lo;
  __shared__ double p_R[2][9], p_t[3];
  __shared__ int s_ok, p_dec;
  const VerifyDev& e = vs[blockIdx.x];
  const int t = threadIdx.x;
  const int K = e.nvalid[0];
  double cam[8];
  for (int c = 0; c < 8; ++c) cam[c] = (double)e.href[c];
  const double tn = thresh / ((cam[0] + cam[5]) / 2.0), t2 = tn * tn;
  // hypcount = 16 score + 15 - model (or -1): the hypotheses compare by score alone (>> 4 keeps -1), the lowest h among equals
  int bc, bh;
  vf_best<4>(e, iters, s_best, bc, bh);
  if (t == 0) {
    s_ok = 0; s_lo.stop = 0; s_lo.rounds = 0; p_dec = 0;
    if (bc >= 0 && K >= 5) {                                 // the model its workgroup of the hypotheses kernel left: nothing is solved again
      const double* src = vp_block_model(e, iters, bh / VF_HB);
      for (int c = 0; c < 9; ++c) s_lo.M[c] = src[c];
      s_ok = 1;
    }
  }
  __syncthreads();
  if (!s_ok) {
    vf_no_model(e, K, 24);
    return;
  }
  vf_local_opt<PoseModel>(e, K, cam, t2, lo_iters, s_lo, s_acc);
  // thread 0: no accepted round -> ess() of the best model; the sign rule; the decompositions
  if (t == 0) {
    double G[9];
    for (int c = 0; c < 9; ++c) G[c] = s_lo.M[c];
    if (s_lo.rounds == 0) PoseModel::project(G, s_lo.S, s_lo.V);
    const double sg = vf_sign(G);
    for (int c = 0; c < 9; ++c) { G[c] = sg * G[c]; s_lo.M[c] = G[c]; }
    double v[3][3], w[2][3], s[2];
    vp_svd(G, s_lo.S, s_lo.V, v, w, s);
    if (s[0] > 0.0 && s[1] > 0.0) {
      double u1[3], u2[3], u3[3];
      for (int k = 0; k < 3; ++k) { u1[k] = w[0][k] / s[0]; u2[k] = w[1][k] / s[1]; }
      u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
      const double n3 = sqrt(u3[0] * u3[0] + u3[1] * u3[1] + u3[2] * u3[2]);
      if (n3 > 0.0) {
        for (int k = 0; k < 3; ++k) u3[k] = u3[k] / n3;
        const double c0 = v[0][1] * v[1][2] - v[0][2] * v[1][1], c1 = v[0][2] * v[1][0] - v[0][0] * v[1][2], c2 = v[0][0] * v[1][1] - v[0][1] * v[1][0];
        const double sv = c0 * v[2][0] + c1 * v[2][1] + c2 * v[2][2] < 0.0 ? -1.0 : 1.0;
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) {
            const double uv = u3[r] * (sv * v[2][c]);
            p_R[0][3 * r + c] = u2[r] * v[0][c] - u1[r] * v[1][c] + uv;
            p_R[1][3 * r + c] = u1[r] * v[1][c] - u2[r] * v[0][c] + uv;
          }
        for (int k = 0; k < 3; ++k) p_t[k] = u3[k];
        p_dec = 1;
      }
    }
  }
  __syncthreads();
  double F[9];
  for (int c = 0; c < 9; ++c) F[c] = s_lo.M[c];
  const int dec = p_dec;
  double Ra[9], Rb[9], tv[3];
  for (int c = 0; c < 9; ++c) { Ra[c] = dec ? p_R[0][c] : 0.0; Rb[c] = dec ? p_R[1][c] : 0.0; }
  for (int c = 0; c < 3; ++c) tv[c] = dec ? p_t[c] : 0.0;
  // the votes of an inlier: in front of both cameras under (Ra, t), (Ra, -t), (Rb, t), (Rb, -t)
  vf_final_sweep<PoseModel, 5>(e, K, cam, t2, F, bh, bc >> 4, s_lo, s_acc, [&](double (&a)[5], double x, double y, double u, double v) {
    double n0, n1, D;
    vp_depths(Ra, tv, x, y, u, v, n0, n1, D);
    a[1] += D > 0.0 && n0 > 0.0 && n1 > 0.0 ? 1.0 : 0.0;
    a[2] += D > 0.0 && n0 < 0.0 && n1 < 0.0 ? 1.0 : 0.0;
    vp_depths(Rb, tv, x, y, u, v, n0, n1, D);
    a[3] += D > 0.0 && n0 > 0.0 && n1 > 0.0 ? 1.0 : 0.0;
    a[4] += D > 0.0 && n0 < 0.0 && n1 < 0.0 ? 1.0 : 0.0;
  });
  if (t == 0) {
    for (int c = 0; c < 9; ++c) e.hom[c] = (float)F[c];
    int w = 0;
    double votes = vf_total(s_acc, 1);
    for (int q = 1; q < 4; ++q) {
      const double vq = vf_total(s_acc, 1 + q);
      if (vq > votes) { votes = vq; w = q; }
    }
    const double st = (w & 1) ? -1.0 : 1.0;
    for (int c = 0; c < 9; ++c) e.hom[9 + c] = dec ? (float)p_R[w >> 1][c] : 0.f;
    for (int c = 0; c < 3; ++c) e.hom[18 + c] = dec ? (float)(st * p_t[c]) : 0.f;
    e.hom[21] = dec ? (float)votes : 0.f;
    e.hom[22] = (float)(15 - (bc & 15));                    // the index of the best model among those of its sample
    e.hom[23] = 0.f;
  }
}

// The workspace of gims_verify_pairs: the VerifyDev table, then per set the dense correspondences, their rows, the hypothesis counters and K.
// recs == nullptr: sizing only.
// The table holds the sets without the pose model first (recs[0 .. n_other - 1], in their order) and the pose sets after them, so that
// each pair of kernels runs over its own contiguous part; every set finds its outputs through its pointers.
static void verify_layout(const gims_verify_set* sets, int n_sets, int iters, WsLayout& L, VerifyDev* recs) {
  L.take<VerifyDev>(n_sets);
  int n_other = 0;
  for (int i = 0; i < n_sets; ++i) n_other += sets[i].model == GIMS_VERIFY_MODEL_POSE ? 0 : 1;
  int at_other = 0, at_pose = n_other;
  for (int i = 0; i < n_sets; ++i) {
    const gims_verify_set& p = sets[i];
    VerifyDev d;
    memset(&d, 0, sizeof(d));
    d.corr = L.take<float4>(p.n0);
    d.rows = L.take<int32_t>(p.n0);
    // a pose set keeps, behind its counters, the best model (9 doubles) of every workgroup of the hypotheses kernel
    d.hypcount = L.take<int32_t>(p.model == GIMS_VERIFY_MODEL_POSE ? (size_t)iters + 2 + 18 * (size_t)cdiv(iters, VF_HB) : (size_t)iters);
    d.nvalid = L.take<int32_t>(64);
    if (!recs) continue;
    d.kp0 = p.kpts0; d.kp1 = p.kpts1; d.matches0 = p.matches0;
    d.n0 = p.n0; d.n1 = p.n1; d.height = p.height; d.width = p.width; d.has_ref = p.has_ref ? 1 : 0; d.model = p.model;
    memcpy(d.href, p.h_ref, sizeof(d.href));
    d.inlier = p.inlier; d.record = p.record; d.hom = p.homography;
    recs[p.model == GIMS_VERIFY_MODEL_POSE ? at_pose++ : at_other++] = d;
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
  int n_pose = 0;
  for (int i = 0; i < n_sets; ++i) {
    const gims_verify_set& p = sets[i];
    GIMS_CHECK_ARG(p.n0 >= 0 && p.n1 >= 0 && (p.n0 == 0 || (p.kpts0 && p.inlier)) && (p.n1 == 0 || p.kpts1) && p.record && p.homography,
                   "gims_verify_pairs: set %d has a negative shape or a null pointer", i);
    GIMS_CHECK_ARG(p.matches0 || p.n0 == p.n1, "gims_verify_pairs: set %d has no matches0 (identity pairing) but n0 = %d != n1 = %d", i, p.n0, p.n1);
    GIMS_CHECK_ARG(p.model == GIMS_VERIFY_MODEL_HOMOGRAPHY || p.model == GIMS_VERIFY_MODEL_FUNDAMENTAL || p.model == GIMS_VERIFY_MODEL_POSE,
                   "gims_verify_pairs: set %d has model = %d (GIMS_VERIFY_MODEL_HOMOGRAPHY, GIMS_VERIFY_MODEL_FUNDAMENTAL or GIMS_VERIFY_MODEL_POSE)", i,
                   p.model);
    if (p.model == GIMS_VERIFY_MODEL_POSE) {
      GIMS_CHECK_ARG(!p.has_ref && p.h_ref[8] == 0.f,
                     "gims_verify_pairs: set %d has model = pose: h_ref carries the intrinsics, so has_ref and h_ref[8] must be 0", i);
      bool cam_ok = true;
      for (int c = 0; c < 8; ++c) cam_ok = cam_ok && isfinite(p.h_ref[c]);
      cam_ok = cam_ok && p.h_ref[0] > 0.f && p.h_ref[1] > 0.f && p.h_ref[4] > 0.f && p.h_ref[5] > 0.f;
      GIMS_CHECK_ARG(cam_ok, "gims_verify_pairs: set %d has model = pose and intrinsics that are not finite, or a focal length that is not positive", i);
      GIMS_CHECK_ARG(p.n0 < (1 << 27), "gims_verify_pairs: set %d has model = pose and n0 = %d (at most 2^27 - 1)", i, p.n0);
      ++n_pose;
    }
    GIMS_CHECK_ARG(p.model != GIMS_VERIFY_MODEL_FUNDAMENTAL || !p.has_ref,
                   "gims_verify_pairs: set %d has model = fundamental and a reference homography (has_ref): there is no error column for F", i);
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
  const int n_other = n_sets - n_pose;
  if (n_other > 0) {
    if (iters > 0) hipLaunchKernelGGL(verify_hyp_kernel, dim3(cdiv(iters, VF_HB), n_other), dim3(256), 0, s, dev, seed, iters, t2);
    hipLaunchKernelGGL(verify_finish_kernel, dim3(n_other), dim3(1024), 0, s, dev, seed, iters, lo_iters, t2);
  }
  if (n_pose > 0) {
    if (iters > 0)
      hipLaunchKernelGGL(verify_pose_hyp_kernel, dim3(cdiv(iters, VF_HB), n_pose), dim3(256), 0, s, dev + n_other, seed, iters, (double)thresh);
    hipLaunchKernelGGL(verify_pose_finish_kernel, dim3(n_pose), dim3(1024), 0, s, dev + n_other, seed, iters, lo_iters, (double)thresh);
  }
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}
