// Device helpers of the homography estimation shared by csrc/eval.hip (evaluation against a ground truth) and csrc/verify.hip
// (ground-truth-free verification): the float64 elimination, the 4-point model, the reprojection error, the sampler of the
// specification in include/gims_hip.h and the corner error.  Both files score and refit with these very functions, so that the same
// inputs give the same model in either entry point.  Also here: the polynomial product and evaluation that the five-point solver of
// verify.hip and the P3P solver of csrc/resect.hip share (resect.hip takes the sampler from here as well).
#pragma once
#include "common.h"

namespace gims {

// ---------------------------------------------------------------------------------------------- small dense algebra
// H (h[8] = 1) through 4 point pairs: Gaussian elimination with partial pivoting on the 8x8 system, float64.
__device__ bool solve8(double (&A)[8][9]) {
  for (int c = 0; c < 8; ++c) {
    int piv = c;
    double best = fabs(A[c][c]);
    for (int r = c + 1; r < 8; ++r)
      if (fabs(A[r][c]) > best) { best = fabs(A[r][c]); piv = r; }
    if (!(best > 1e-300)) return false;
    if (piv != c)
      for (int k = c; k < 9; ++k) { const double t = A[c][k]; A[c][k] = A[piv][k]; A[piv][k] = t; }
    const double inv = 1.0 / A[c][c];
    for (int r = c + 1; r < 8; ++r) {
      const double f = A[r][c] * inv;
      if (f != 0.0)
        for (int k = c; k < 9; ++k) A[r][k] -= f * A[c][k];
    }
  }
  for (int c = 7; c >= 0; --c) {
    double s = A[c][8];
    for (int k = c + 1; k < 8; ++k) s -= A[c][k] * A[k][8];
    A[c][8] = s / A[c][c];
  }
  return true;
}

// the 8 x 9 system of four point pairs and its solution; false without a finite model.  load(k, x, y, u, v) fetches pair k: the rows of
// a pair are formed right behind its loads, whoever loads them (homography4 below, homography4_dense of verify.hip)
template <class Load>
__device__ __forceinline__ bool homography4_solve(Load load, double (&H)[9]) {
  double A[8][9];
  for (int k = 0; k < 4; ++k) {
    double x, y, u, v;
    load(k, x, y, u, v);
    const double r0[9] = {x, y, 1, 0, 0, 0, -u * x, -u * y, u};
    const double r1[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, v};
    for (int c = 0; c < 9; ++c) { A[2 * k][c] = r0[c]; A[2 * k + 1][c] = r1[c]; }
  }
  if (!solve8(A)) return false;
  bool fin = true;
  for (int c = 0; c < 8; ++c) { H[c] = A[c][8]; fin = fin && isfinite(H[c]); }
  H[8] = 1.0;
  return fin;
}

__device__ bool homography4(const float* p0, const float* p1, const int (&idx)[4], const int32_t* midx, const int64_t* matches0,
                            double (&H)[9]) {
  return homography4_solve([&](int k, double& x, double& y, double& u, double& v) {
    const int i = midx[idx[k]];
    const int j = (int)matches0[i];
    x = p0[2 * i]; y = p0[2 * i + 1]; u = p1[2 * j]; v = p1[2 * j + 1];
  }, H);
}

__device__ __forceinline__ double reproj2(const double (&H)[9], double x, double y, double u, double v) {
  const double w = H[6] * x + H[7] * y + H[8];
  const double qx = (H[0] * x + H[1] * y + H[2]) / w, qy = (H[3] * x + H[4] * y + H[5]) / w;
  return (qx - u) * (qx - u) + (qy - v) * (qy - v);
}

// mean corner distance between two homographies (eval_homography.py:210, 219-223): corners transformed in float64,
// rounded to float32 like cv2.perspectiveTransform's output, error in float32 like compute_pixel_error
__device__ float corner_error(const double (&He)[9], const float* hgt, int height, int width) {
  const float cx[4] = {0.f, 0.f, (float)width, (float)width}, cy[4] = {0.f, (float)height, (float)height, 0.f};
  double Hg[9];
  for (int c = 0; c < 9; ++c) Hg[c] = hgt[c];
  float acc = 0.f;
  for (int k = 0; k < 4; ++k) {
    const double x = cx[k], y = cy[k];
    const double we = He[6] * x + He[7] * y + He[8], wg = Hg[6] * x + Hg[7] * y + Hg[8];
    const float ex = (float)((He[0] * x + He[1] * y + He[2]) / we), ey = (float)((He[3] * x + He[4] * y + He[5]) / we);
    const float gx = (float)((Hg[0] * x + Hg[1] * y + Hg[2]) / wg), gy = (float)((Hg[3] * x + Hg[4] * y + Hg[5]) / wg);
    const float dx = gx - ex, dy = gy - ey;
    acc += sqrtf(dx * dx + dy * dy);
  }
  return acc / 4.f;
}

__device__ __forceinline__ uint64_t splitmix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// sampler of the specification in include/gims_hip.h: N distinct indices below k.  A larger N continues the stream of a smaller one,
// so the first four of an eight-point sample are the four-point sample of the same hypothesis
template <int N>
__device__ void ransac_sample(uint64_t seed, int hyp, int k, int (&idx)[N]) {
  uint64_t state = seed ^ ((uint64_t)hyp * 0xD1342543DE82EF95ull);
  int n = 0;
  while (n < N) {
    state = splitmix(state);
    const int c = (int)(state % (uint64_t)k);
    bool dup = false;
    for (int q = 0; q < n; ++q) dup = dup || idx[q] == c;
    if (!dup) idx[n++] = c;
  }
}

// ---------------------------------------------------------------------------------------------- polynomials (ascending coefficients)
// shared by the five-point solver of verify.hip and the P3P solver of resect.hip
// out (na + nb - 1 coefficients, ascending) = a * b
__device__ void vp_pmul(const double* a, int na, const double* b, int nb, double* out) {
  for (int i = 0; i < na + nb - 1; ++i) out[i] = 0.0;
  for (int i = 0; i < na; ++i)
    for (int j = 0; j < nb; ++j) out[i + j] += a[i] * b[j];
}
__device__ __forceinline__ double vp_horner(const double* c, int deg, double z) {
  double v = c[deg];
  for (int i = deg - 1; i >= 0; --i) v = v * z + c[i];
  return v;
}

}  // namespace gims
