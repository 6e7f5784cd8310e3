// Exact geometric predicates of the Delaunay graph build (delaunay.hip), for float32 input coordinates.  Compiles for the host
// (any C++ compiler; the tests compare it against exact rational arithmetic) and for the device.
//
//   orient(a, b, c)      > 0  iff  a, b, c turn counter-clockwise (c lies left of a -> b)
//   incircle(a, b, c, d) > 0  iff  d lies strictly inside the circle through a, b, c, when a, b, c turn counter-clockwise
//                              (= the 4x4 determinant with rows [x, y, x^2 + y^2, 1] of a, b, c, d)
//
// Every predicate comes in two tiers.
//   *_filter: float64 evaluation with Shewchuk's static error bound (orient2dfast / incirclefast and their "A" bounds, which cover the
//     rounding of the coordinate differences too).  It returns the sign when the bound proves it, and also when every coordinate is an
//     integer and every difference is at most 4096 in magnitude (then the float64 evaluation has no rounding at all: |incircle terms|
//     <= 3 * 2^50); otherwise DP_UNDECIDED.  No arrays: it costs registers only.
//   *_exact: the sign of the exact value.  The determinants are expanded in the raw coordinates (no differences), so every term is a
//     product of float32 values, exact in float64, or such a product times x^2 or y^2, split exactly by a two-product (FMA); the terms
//     are summed into a non-overlapping expansion (Shewchuk's Grow-Expansion with zero elimination), whose largest component carries
//     the sign.  Exact for every finite float32 input (no product under- or overflows).  Up to 97 doubles of state: meant for the
//     fallback kernel only.
//
// TIE RULE (incircle == 0, four or more cocircular points): Simulation of Simplicity on the lifted coordinate.  The lift of the point
// with id i becomes x^2 + y^2 + eps^(2^i) for an infinitesimal eps > 0: a LOWER id gets a LARGER perturbation.  Perturbing the lift of
// row k of the determinant adds eps_k times its cofactor, so the sign of the perturbed determinant is the sign of the first non-zero
// cofactor, the points taken in ascending id:
//     a: +orient(b, c, d)    b: -orient(a, c, d)    c: +orient(a, b, d)    d: -orient(a, b, c)
// Geometrically: of a cocircular set, a point is "inside" the circle through three others iff the first non-zero cofactor says so;
// in particular, when d has the lowest id of the four and a, b, c turn counter-clockwise, d counts as OUTSIDE (-orient(a, b, c) < 0).
// The perturbed determinant is still an alternating function of its four arguments, so the rule is consistent under every permutation,
// and it is non-zero unless all four points are collinear.  The triangulation it selects is the unique regular triangulation of the
// perturbed lifted points: one Delaunay triangulation of the input, the same whichever point's star is computed.
#pragma once

#include <math.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define DP_FN __host__ __device__ inline
#else
#define DP_FN static inline
#endif

// the error bounds assume every product and sum is rounded on its own: no contraction into FMAs
#if defined(__clang__)
#define DP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DP_NO_CONTRACT
#endif

namespace dpred {

constexpr int DP_UNDECIDED = 2;
constexpr double DP_EPS = 1.1102230246251565e-16;                        // 2^-53
constexpr double DP_CCW_BOUND = (3.0 + 16.0 * DP_EPS) * DP_EPS;
constexpr double DP_ICC_BOUND = (10.0 + 96.0 * DP_EPS) * DP_EPS;
constexpr int DP_EXACT_TERMS = 97;                                      // capacity of the incircle expansion (96 terms + 1)

DP_FN int dp_sign(double v) { return (v > 0.0) - (v < 0.0); }
DP_FN bool dp_int(double v) { return v == rint(v); }
DP_FN bool dp_small(double v) { return fabs(v) <= 4096.0; }

// ---------------------------------------------------------------- filters
DP_FN int orient_filter(double ax, double ay, double bx, double by, double cx, double cy) {
  DP_NO_CONTRACT
  const double acx = ax - cx, bcx = bx - cx, acy = ay - cy, bcy = by - cy;
  const double l = acx * bcy, r = acy * bcx, det = l - r;
  const double bound = DP_CCW_BOUND * (fabs(l) + fabs(r));
  if (det > bound) return 1;
  if (-det > bound) return -1;
  if (bound == 0.0) return 0;                 // both products are exact zeros (a difference of float32 values rounds to 0 only when it is 0)
  if (dp_int(ax) && dp_int(ay) && dp_int(bx) && dp_int(by) && dp_int(cx) && dp_int(cy) && dp_small(acx) && dp_small(bcx) &&
      dp_small(acy) && dp_small(bcy))
    return dp_sign(det);
  return DP_UNDECIDED;
}

DP_FN int incircle_filter(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy) {
  DP_NO_CONTRACT
  const double adx = ax - dx, bdx = bx - dx, cdx = cx - dx, ady = ay - dy, bdy = by - dy, cdy = cy - dy;
  const double bdxcdy = bdx * cdy, cdxbdy = cdx * bdy, alift = adx * adx + ady * ady;
  const double cdxady = cdx * ady, adxcdy = adx * cdy, blift = bdx * bdx + bdy * bdy;
  const double adxbdy = adx * bdy, bdxady = bdx * ady, clift = cdx * cdx + cdy * cdy;
  const double det = alift * (bdxcdy - cdxbdy) + blift * (cdxady - adxcdy) + clift * (adxbdy - bdxady);
  const double perm = (fabs(bdxcdy) + fabs(cdxbdy)) * alift + (fabs(cdxady) + fabs(adxcdy)) * blift + (fabs(adxbdy) + fabs(bdxady)) * clift;
  const double bound = DP_ICC_BOUND * perm;
  if (det > bound) return 1;
  if (-det > bound) return -1;
  if (perm == 0.0) return 0;
  if (dp_int(ax) && dp_int(ay) && dp_int(bx) && dp_int(by) && dp_int(cx) && dp_int(cy) && dp_int(dx) && dp_int(dy) && dp_small(adx) &&
      dp_small(bdx) && dp_small(cdx) && dp_small(ady) && dp_small(bdy) && dp_small(cdy))
    return dp_sign(det);
  return DP_UNDECIDED;
}

// sign of |p - a|^2 - |p - b|^2 (which of a, b is nearer to p)
DP_FN int dist_cmp_filter(double px, double py, double ax, double ay, double bx, double by) {
  DP_NO_CONTRACT
  const double dax = ax - px, day = ay - py, dbx = bx - px, dby = by - py;
  const double da = dax * dax + day * day, db = dbx * dbx + dby * dby;
  const double bound = 8.0 * DP_EPS * (da + db);             // each of da, db carries a relative error below 4.0001 eps
  if (da - db > bound) return 1;
  if (db - da > bound) return -1;
  if (dp_int(px) && dp_int(py) && dp_int(ax) && dp_int(ay) && dp_int(bx) && dp_int(by) && dp_small(dax) && dp_small(day) &&
      dp_small(dbx) && dp_small(dby))
    return dp_sign(da - db);
  return DP_UNDECIDED;
}

// ---------------------------------------------------------------- exact expansion arithmetic
DP_FN void two_sum(double a, double b, double& x, double& y) {
  DP_NO_CONTRACT
  x = a + b;
  const double bv = x - a, av = x - bv;
  y = (a - av) + (b - bv);
}

// e (n components, non-overlapping, increasing magnitude) += b, zero components eliminated
DP_FN void grow(double* e, int& n, double b) {
  DP_NO_CONTRACT
  double q = b;
  int k = 0;
  for (int i = 0; i < n; ++i) {
    double x, y;
    two_sum(q, e[i], x, y);
    if (y != 0.0) e[k++] = y;
    q = x;
  }
  if (q != 0.0 || k == 0) e[k++] = q;
  n = k;
}

DP_FN void grow_product(double* e, int& n, double a, double b) {
  DP_NO_CONTRACT
  const double x = a * b, y = fma(a, b, -x);
  grow(e, n, y);
  grow(e, n, x);
}

DP_FN int expansion_sign(const double* e, int n) { return n > 0 ? dp_sign(e[n - 1]) : 0; }

// the six products of orient(a, b, c) = ax (by - cy) + bx (cy - ay) + cx (ay - by), each exact in float64 for float32 inputs
DP_FN void orient_terms(double ax, double ay, double bx, double by, double cx, double cy, double* t) {
  DP_NO_CONTRACT
  t[0] = ax * by; t[1] = -(ax * cy); t[2] = bx * cy; t[3] = -(bx * ay); t[4] = cx * ay; t[5] = -(cx * by);
}

DP_FN int orient_exact(double ax, double ay, double bx, double by, double cx, double cy) {
  double t[6], e[8];
  int n = 0;
  orient_terms(ax, ay, bx, by, cx, cy, t);
  for (int i = 0; i < 6; ++i) grow(e, n, t[i]);
  return expansion_sign(e, n);
}

// sum over rows k of sign_k (x_k^2 + y_k^2) orient(other three rows): the cofactor expansion along the lift column
DP_FN int incircle_exact(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy) {
  DP_NO_CONTRACT
  const double X[4] = {ax, bx, cx, dx}, Y[4] = {ay, by, cy, dy};
  double e[DP_EXACT_TERMS];
  int n = 0;
  for (int k = 0; k < 4; ++k) {
    int o[3], m = 0;
    for (int j = 0; j < 4; ++j)
      if (j != k) o[m++] = j;
    double t[6];
    orient_terms(X[o[0]], Y[o[0]], X[o[1]], Y[o[1]], X[o[2]], Y[o[2]], t);
    const double s = (k & 1) ? -1.0 : 1.0;
    const double xx = X[k] * X[k], yy = Y[k] * Y[k];                 // exact
    for (int i = 0; i < 6; ++i) {
      grow_product(e, n, s * xx, t[i]);
      grow_product(e, n, s * yy, t[i]);
    }
  }
  return expansion_sign(e, n);
}

DP_FN int dist_cmp_exact(double px, double py, double ax, double ay, double bx, double by) {
  DP_NO_CONTRACT
  // |p-a|^2 - |p-b|^2 = ax^2 + ay^2 - bx^2 - by^2 - 2 (px ax + py ay - px bx - py by)
  const double t[8] = {ax * ax, ay * ay, -(bx * bx), -(by * by), -2.0 * (px * ax), -2.0 * (py * ay), 2.0 * (px * bx), 2.0 * (py * by)};
  double e[9];
  int n = 0;
  for (int i = 0; i < 8; ++i) grow(e, n, t[i]);
  return expansion_sign(e, n);
}

// ---------------------------------------------------------------- two-tier wrappers; EXACT = false never leaves the filters
template <bool EXACT>
DP_FN int orient(double ax, double ay, double bx, double by, double cx, double cy) {
  const int s = orient_filter(ax, ay, bx, by, cx, cy);
  if (EXACT && s == DP_UNDECIDED) return orient_exact(ax, ay, bx, by, cx, cy);
  return s;
}

template <bool EXACT>
DP_FN int dist_cmp(double px, double py, double ax, double ay, double bx, double by) {
  const int s = dist_cmp_filter(px, py, ax, ay, bx, by);
  if (EXACT && s == DP_UNDECIDED) return dist_cmp_exact(px, py, ax, ay, bx, by);
  return s;
}

// incircle with the tie rule above: never 0 unless the four points are collinear; DP_UNDECIDED only when EXACT = false
template <bool EXACT>
DP_FN int incircle_sos(double ax, double ay, int ia, double bx, double by, int ib, double cx, double cy, int ic, double dx, double dy, int id) {
  int s = incircle_filter(ax, ay, bx, by, cx, cy, dx, dy);
  if (s == DP_UNDECIDED) {
    if (!EXACT) return DP_UNDECIDED;
    s = incircle_exact(ax, ay, bx, by, cx, cy, dx, dy);
  }
  if (s != 0) return s;
  // cofactors in ascending id (ranks by comparison: no runtime-indexed array, so the filter-only path stays in registers)
  const int ra = (ib < ia) + (ic < ia) + (id < ia), rb = (ia < ib) + (ic < ib) + (id < ib), rc = (ia < ic) + (ib < ic) + (id < ic);
  for (int rank = 0; rank < 4; ++rank) {
    int c;
    if (ra == rank) c = orient<EXACT>(bx, by, cx, cy, dx, dy);
    else if (rb == rank) c = orient<EXACT>(ax, ay, cx, cy, dx, dy), c = c == DP_UNDECIDED ? c : -c;
    else if (rc == rank) c = orient<EXACT>(ax, ay, bx, by, dx, dy);
    else c = orient<EXACT>(ax, ay, bx, by, cx, cy), c = c == DP_UNDECIDED ? c : -c;
    if (c == DP_UNDECIDED) return DP_UNDECIDED;
    if (c != 0) return c;
  }
  return 0;
}

}  // namespace dpred
