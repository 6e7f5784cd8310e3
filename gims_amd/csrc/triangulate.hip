// Multi-view triangulation of tracks from known cameras: GIMS_AUX_TRIANGULATE_TRACKS of gims_run_ops turns every track of a
// Tracks (GIMS_AUX_BUILD_TRACKS) into a 3-D point, robustly: two-view hypotheses scored by reprojection, a midpoint over the best inlier set,
// guarded Gauss-Newton rounds, one final classification of every observation.  include/gims_hip.h has the contract; tests/triangulate_ref.py
// is the NumPy restatement.  All geometry is float64 on the vector ALU.
//
// Launches, the same whatever the data: memset nodes (counters, list counters, obs_error = -1, obs_inlier = 0) -> classify (a thread per
// track: the range check of indptr, the tracks that are not processed, the lists of the mid and the long tracks) -> short (a group of
// GIMS_TRI_SHORT_TRACK lanes per track of up to that many observations, sixteen tracks a wave) -> mid (a wave per track of up to 64) -> long
// (a wave per track of up to GIMS_TRI_MAX_OBS, observations in slots of 64).  The three are one body, tri_track: lane j of a group of G
// lanes owns observations j, j + G, ... of the track's usable ones.  Every sum over observations is the lane's own sum in ascending slot
// order followed by a butterfly over the group's lanes (__shfl_xor: both partners add the same two numbers, so all lanes hold the same bits);
// G depends on the track's length alone, so a track's outputs do not depend on the batch it is in, its place there, or the run.
#include "common.h"

#include <cfloat>

namespace gims {

constexpr int TRI_MAX_OBS = GIMS_TRI_MAX_OBS;
constexpr int TRI_CAM = GIMS_TRI_CAMERA_WORDS;
constexpr int TRI_SHORT = GIMS_TRI_SHORT_TRACK;                // a track of up to this many observations is served by that many lanes
constexpr int TRI_MID = 64;                                    // ... of up to this many by a wave with one observation per lane
constexpr int TRI_THREADS = 256;
enum { TRI_N_OK = 0, TRI_N_LOW_ANGLE, TRI_N_NO_MODEL, TRI_N_TOO_SHORT, TRI_N_TOO_LONG, TRI_N_BAD_OBS, TRI_N_INLIER_OBS, TRI_COUNTERS = 8 };
enum { TRI_TOO_SHORT = 1, TRI_NO_MODEL = 2, TRI_LOW_ANGLE = 4, TRI_TOO_LONG = 8 };
enum { TRI_CLS_SHORT = 1, TRI_CLS_MID = 2, TRI_CLS_LONG = 3 };

// The output buffer and, behind it, the scratch (the formula of include/gims_hip.h; gims_aux_layout reports this routine's offsets)
struct TriOut {
  double* xyz;
  float *max_angle, *rms, *obs_error;
  int32_t *n_inliers, *counters, *list_mid, *list_long, *n_list;
  uint8_t *status, *obs_inlier;
};
static size_t tri_layout(void* base, int64_t T, int64_t n_obs, TriOut& w, WsRecord* rec = nullptr) {
  WsLayout L(base, rec);
  w.xyz = L.take<double>((size_t)T * 3);
  w.max_angle = L.take<float>((size_t)T);
  w.rms = L.take<float>((size_t)T);
  w.n_inliers = L.take<int32_t>((size_t)T);
  w.obs_error = L.take<float>((size_t)n_obs);
  w.status = L.take<uint8_t>((size_t)T);
  w.obs_inlier = L.take<uint8_t>((size_t)n_obs);
  w.counters = L.take<int32_t>(TRI_COUNTERS);
  L.scratch_from_here();
  w.list_mid = L.take<int32_t>((size_t)T);
  w.list_long = L.take<int32_t>((size_t)T);
  w.n_list = L.take<int32_t>(2);
  return L.bytes();
}

struct TriArgs {
  const int32_t *indptr, *obs_image, *obs_keypoint;
  const float* kpts;
  const double* cams;
  TriOut out;
  int T, n_obs, n_images, max_hyp, refine_iters;
  int64_t N;
  double thresh2, min_angle;
};

__device__ __forceinline__ bool tri_range(const TriArgs& a, int t, int& beg, int& len) {
  const int b = a.indptr[t], e = a.indptr[t + 1];
  beg = b;
  len = e - b;
  return b >= 0 && e >= b && e <= a.n_obs;
}

// the outputs of a track without a model: zeros (its observations keep the -1 / 0 of the memset nodes)
__device__ __forceinline__ void tri_write_track(const TriOut& o, int t, int status, const double X[3], float angle, float rms, int n_in) {
  const bool model = (status & ~TRI_LOW_ANGLE) == 0;
  for (int j = 0; j < 3; ++j) o.xyz[(int64_t)3 * t + j] = model ? X[j] : 0.0;
  o.max_angle[t] = model ? angle : 0.f;
  o.rms[t] = model ? rms : 0.f;
  o.n_inliers[t] = model ? n_in : 0;
  o.status[t] = (uint8_t)status;
}

// ---------------------------------------------------------------------------------------------- classify
__global__ __launch_bounds__(TRI_THREADS) void tri_classify_kernel(TriArgs a) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * TRI_THREADS + threadIdx.x;
  int cls = 0, too_short = 0, too_long = 0;
  if (t < a.T) {
    int beg, len;
    const double zero[3] = {0.0, 0.0, 0.0};
    if (!tri_range(a, t, beg, len)) {
      too_short = 1;
      tri_write_track(a.out, t, TRI_TOO_SHORT, zero, 0.f, 0.f, 0);
    } else if (len > TRI_MAX_OBS) {
      too_long = 1;
      tri_write_track(a.out, t, TRI_TOO_LONG, zero, 0.f, 0.f, 0);
    } else {
      cls = len <= TRI_SHORT ? TRI_CLS_SHORT : len <= TRI_MID ? TRI_CLS_MID : TRI_CLS_LONG;
    }
  }
  // one atomic per wave and list; the order of a list is the order of the race, and no output depends on it
  for (int c = TRI_CLS_MID; c <= TRI_CLS_LONG; ++c) {
    const unsigned long long m = __ballot(cls == c);
    if (m == 0ull) continue;
    const int leader = __builtin_ctzll(m);
    int base = 0;
    if (lane == leader) base = atomicAdd(a.out.n_list + (c - TRI_CLS_MID), __popcll(m));
    base = __shfl(base, leader, 64);
    const int at = base + __popcll(m & ((1ull << lane) - 1ull));
    if (cls == c && at >= 0 && at < a.T) (c == TRI_CLS_MID ? a.out.list_mid : a.out.list_long)[at] = t;
  }
  const int n_short = __popcll(__ballot(too_short)), n_long = __popcll(__ballot(too_long));
  if (lane == 0) {
    if (n_short) atomicAdd(a.out.counters + TRI_N_TOO_SHORT, n_short);
    if (n_long) atomicAdd(a.out.counters + TRI_N_TOO_LONG, n_long);
  }
}

// ---------------------------------------------------------------------------------------------- one track on a group of G lanes
template <int G>
__device__ __forceinline__ double tri_gsum(double v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;
}
template <int G>
__device__ __forceinline__ int tri_gsum(int v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;
}
template <int G>
__device__ __forceinline__ int tri_gmin(int v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    const int x = __shfl_xor(v, o, G);
    v = x < v ? x : v;
  }
  return v;
}

// X = adj(A) b / det A for the symmetric A = {a00, a01, a02, a11, a12, a22}; returns det (X is only meaningful when the caller accepts it)
__device__ __forceinline__ double tri_solve(const double A[6], const double b[3], double X[3]) {
  const double c00 = A[3] * A[5] - A[4] * A[4], c01 = A[2] * A[4] - A[1] * A[5], c02 = A[1] * A[4] - A[2] * A[3];
  const double c11 = A[0] * A[5] - A[2] * A[2], c12 = A[1] * A[2] - A[0] * A[4], c22 = A[0] * A[3] - A[1] * A[1];
  const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
  X[0] = (c00 * b[0] + c01 * b[1] + c02 * b[2]) / det;
  X[1] = (c01 * b[0] + c11 * b[1] + c12 * b[2]) / det;
  X[2] = (c02 * b[0] + c12 * b[1] + c22 * b[2]) / det;
  return det;
}

// the angle at X between the centres Cp and Cq, degrees
__device__ __forceinline__ double tri_angle(const double X[3], const double* Cp, const double* Cq) {
  const double a0 = X[0] - Cp[0], a1 = X[1] - Cp[1], a2 = X[2] - Cp[2], b0 = X[0] - Cq[0], b1 = X[1] - Cq[1], b2 = X[2] - Cq[2];
  const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
  return atan2(sqrt(c0 * c0 + c1 * c1 + c2 * c2), a0 * b0 + a1 * b1 + a2 * b2) * 57.295779513082320876798154814105;
}

struct TriCam {                                                // one observation as the reprojection needs it
  double fx, fy, cx, cy, R[9], t[3], u, v;
};
__device__ __forceinline__ bool tri_finite(double x) { return fabs(x) <= DBL_MAX; }      // (false for a NaN)

__device__ __forceinline__ void tri_load_cam(const TriArgs& a, int k, float u, float v, TriCam& c) {
  const double* r = a.cams + (int64_t)TRI_CAM * k;
  c.fx = r[0], c.fy = r[1], c.cx = r[2], c.cy = r[3];
#pragma unroll
  for (int j = 0; j < 9; ++j) c.R[j] = r[4 + j];
#pragma unroll
  for (int j = 0; j < 3; ++j) c.t[j] = r[13 + j];
  c.u = (double)u, c.v = (double)v;
}

// depth and squared reprojection error of X in one observation
__device__ __forceinline__ void tri_reproject(const TriCam& c, const double X[3], double& z, double& e2) {
  const double x = c.R[0] * X[0] + c.R[1] * X[1] + c.R[2] * X[2] + c.t[0];
  const double y = c.R[3] * X[0] + c.R[4] * X[1] + c.R[5] * X[2] + c.t[1];
  z = c.R[6] * X[0] + c.R[7] * X[1] + c.R[8] * X[2] + c.t[2];
  const double ru = c.fx * x / z + c.cx - c.u, rv = c.fy * y / z + c.cy - c.v;
  e2 = ru * ru + rv * rv;
}

// The staging area of one group: rays, centres, pixels, image and place in the track of the USABLE observations, in track order
struct TriLds {
  double *d, *c;               // [CAP][3] each; d holds the unit vectors centre -> X once the point is final
  float* uv;                   // [CAP][2]; uv[2 i] holds the observation's error once it is classified
  int* k;                      // [CAP]
  uint16_t* oi;                // [CAP]: the place in the track, and in bit 15 the flag: member of the set S, then final inlier
  __device__ __forceinline__ bool in(int i) const { return (oi[i] >> 15) != 0; }
  __device__ __forceinline__ void set_in(int i, bool f) const { oi[i] = (uint16_t)((oi[i] & 0x7fff) | (f ? 0x8000 : 0)); }
  __device__ __forceinline__ int o(int i) const { return oi[i] & 0x7fff; }
};

template <int G, int CAP>
__device__ void tri_track(const TriArgs& a, int t, int lane, int wave_lane, const TriLds& s, int* cnt) {
  constexpr bool ONE = CAP == G;                               // one observation per lane: it stays in registers
  const double zero[3] = {0.0, 0.0, 0.0};
  int beg, L;
  if (!tri_range(a, t, beg, L) || L > CAP) return;             // (the lists hold no such track: classify read the same indptr)

  // ---- stage the usable observations, compacted in track order
  int Lu = 0;
  for (int s0 = 0; s0 < L; s0 += G) {
    const int o = s0 + lane;
    bool ok = false;
    double d[3], c[3];
    float u = 0.f, v = 0.f;
    int k = -1;
    if (o < L) {
      k = a.obs_image[beg + o];
      const int i = a.obs_keypoint[beg + o];
      if (k >= 0 && k < a.n_images) {
        const double* r = a.cams + (int64_t)TRI_CAM * k;
        double w[TRI_CAM];
        bool fin = true;
#pragma unroll
        for (int j = 0; j < TRI_CAM; ++j) {
          w[j] = r[j];
          fin = fin && tri_finite(w[j]);
        }
        const double node = w[16] + (double)i;
        if (fin && w[0] > 0.0 && w[1] > 0.0 && i >= 0 && (double)i < w[17] && node >= 0.0 && node < (double)a.N) {
          const int64_t g = (int64_t)node;                     // 0 .. N - 1
          u = a.kpts[2 * g], v = a.kpts[2 * g + 1];
          if (tri_finite((double)u) && tri_finite((double)v)) {
            ok = true;
            const double x0 = ((double)u - w[2]) / w[0], x1 = ((double)v - w[3]) / w[1];
            const double nrm = sqrt(x0 * x0 + x1 * x1 + 1.0);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              d[j] = (w[4 + j] * x0 + w[7 + j] * x1 + w[10 + j]) / nrm;                     // R^T x / |x|
              c[j] = -(w[4 + j] * w[13] + w[7 + j] * w[14] + w[10 + j] * w[15]);            // -R^T t
            }
          }
        }
      }
    }
    const unsigned long long all = __ballot(ok);
    const unsigned bits = G == 64 ? 0u : (unsigned)((all >> (wave_lane & ~(G - 1))) & ((1ull << (G & 63)) - 1ull));
    const int before = G == 64 ? __popcll(all & ((1ull << lane) - 1ull)) : __popc(bits & ((1u << lane) - 1u));
    const int here = G == 64 ? __popcll(all) : __popc(bits);
    if (ok) {
      const int at = Lu + before;                              // < CAP: at most L <= CAP observations in all
      for (int j = 0; j < 3; ++j) s.d[3 * at + j] = d[j], s.c[3 * at + j] = c[j];
      s.uv[2 * at] = u, s.uv[2 * at + 1] = v;
      s.k[at] = k, s.oi[at] = (uint16_t)o;
    }
    Lu += here;
  }
  __builtin_amdgcn_wave_barrier();
  if (lane == 0 && L > Lu) atomicAdd(cnt + TRI_N_BAD_OBS, L - Lu);
  if (Lu < 2) {
    if (lane == 0) {
      tri_write_track(a.out, t, TRI_TOO_SHORT, zero, 0.f, 0.f, 0);
      atomicAdd(cnt + TRI_N_TOO_SHORT, 1);
    }
    return;
  }
  TriCam mine;
  if (ONE && lane < Lu) tri_load_cam(a, s.k[lane], s.uv[2 * lane], s.uv[2 * lane + 1], mine);
  auto cam_of = [&](int idx, TriCam& c) {
    if (ONE) c = mine; else tri_load_cam(a, s.k[idx], s.uv[2 * idx], s.uv[2 * idx + 1], c);
  };
  auto no_model = [&]() {
    if (lane == 0) {
      tri_write_track(a.out, t, TRI_NO_MODEL, zero, 0.f, 0.f, 0);
      atomicAdd(cnt + TRI_N_NO_MODEL, 1);
    }
  };

  // ---- hypotheses: H pairs spread evenly over the E pairs of usable observations, each scored over all of them
  if (a.max_hyp >= 1) {
    const int64_t E = (int64_t)Lu * (Lu - 1) / 2, H = E < a.max_hyp ? E : a.max_hyp;
    int bn = 0, p = 0;
    double bc = 0.0, bX[3] = {0.0, 0.0, 0.0};
    for (int64_t h = 0; h < H; ++h) {
      const int64_t e = h * E / H;                             // ascending in h, so p only moves forward: Lu steps over the whole loop
      while ((int64_t)(p + 1) * (2 * Lu - p - 2) / 2 <= e) ++p;
      const int q = p + 1 + (int)(e - (int64_t)p * (2 * Lu - p - 1) / 2);
      const double *dp = s.d + 3 * p, *dq = s.d + 3 * q, *cp = s.c + 3 * p, *cq = s.c + 3 * q;
      const double sp = dp[0] * cp[0] + dp[1] * cp[1] + dp[2] * cp[2], sq = dq[0] * cq[0] + dq[1] * cq[1] + dq[2] * cq[2];
      const double A[6] = {2.0 - dp[0] * dp[0] - dq[0] * dq[0], -dp[0] * dp[1] - dq[0] * dq[1], -dp[0] * dp[2] - dq[0] * dq[2],
                           2.0 - dp[1] * dp[1] - dq[1] * dq[1], -dp[1] * dp[2] - dq[1] * dq[2], 2.0 - dp[2] * dp[2] - dq[2] * dq[2]};
      const double b[3] = {cp[0] - dp[0] * sp + cq[0] - dq[0] * sq, cp[1] - dp[1] * sp + cq[1] - dq[1] * sq, cp[2] - dp[2] * sp + cq[2] - dq[2] * sq};
      double X[3];
      const double det = tri_solve(A, b, X);
      if (!(det > 8e-12)) continue;                            // 1e-12 |S|^3, |S| = 2
      if (!(tri_angle(X, cp, cq) >= a.min_angle)) continue;
      int n = 0;
      double c = 0.0;
      for (int idx = lane; idx < Lu; idx += G) {
        TriCam cam;
        cam_of(idx, cam);
        double z, e2;
        tri_reproject(cam, X, z, e2);
        if (z > 0.0 && e2 <= a.thresh2) ++n, c += e2;
      }
      n = tri_gsum<G>(n);
      c = tri_gsum<G>(c);
      if (n >= 2 && (n > bn || (n == bn && c < bc))) bn = n, bc = c, bX[0] = X[0], bX[1] = X[1], bX[2] = X[2];
    }
    if (bn < 2) return no_model();
    for (int idx = lane; idx < Lu; idx += G) {                 // the set S: the inliers of the best hypothesis (the same arithmetic as its score)
      TriCam cam;
      cam_of(idx, cam);
      double z, e2;
      tri_reproject(cam, bX, z, e2);
      s.set_in(idx, z > 0.0 && e2 <= a.thresh2);
    }
  } else {
    for (int idx = lane; idx < Lu; idx += G) s.set_in(idx, true);
  }
  __builtin_amdgcn_wave_barrier();

  // ---- midpoint over S
  double X[3];
  {
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
    int nS = 0;
    for (int idx = lane; idx < Lu; idx += G) {
      if (!s.in(idx)) continue;
      const double *d = s.d + 3 * idx, *c = s.c + 3 * idx;
      const double sc = d[0] * c[0] + d[1] * c[1] + d[2] * c[2];
      A[0] += 1.0 - d[0] * d[0], A[1] += -d[0] * d[1], A[2] += -d[0] * d[2], A[3] += 1.0 - d[1] * d[1], A[4] += -d[1] * d[2], A[5] += 1.0 - d[2] * d[2];
      b[0] += c[0] - d[0] * sc, b[1] += c[1] - d[1] * sc, b[2] += c[2] - d[2] * sc;
      ++nS;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) A[j] = tri_gsum<G>(A[j]);
#pragma unroll
    for (int j = 0; j < 3; ++j) b[j] = tri_gsum<G>(b[j]);
    nS = tri_gsum<G>(nS);
    const double det = tri_solve(A, b, X);
    if (!(det > 1e-12 * (double)nS * (double)nS * (double)nS)) return no_model();
  }

  // ---- guarded Gauss-Newton on the reprojection cost over S
  auto cost_of = [&](const double Y[3], double& cost) -> bool {
    double c = 0.0;
    int neg = 0;
    for (int idx = lane; idx < Lu; idx += G) {
      if (!s.in(idx)) continue;
      TriCam cam;
      cam_of(idx, cam);
      double z, e2;
      tri_reproject(cam, Y, z, e2);
      c += e2;
      neg += !(z > 0.0);
    }
    cost = tri_gsum<G>(c);
    return tri_gsum<G>(neg) == 0;
  };
  if (a.refine_iters > 0) {
    double cost;
    cost_of(X, cost);
    for (int it = 0; it < a.refine_iters; ++it) {
      double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
      for (int idx = lane; idx < Lu; idx += G) {
        if (!s.in(idx)) continue;
        TriCam c;
        cam_of(idx, c);
        const double x = c.R[0] * X[0] + c.R[1] * X[1] + c.R[2] * X[2] + c.t[0];
        const double y = c.R[3] * X[0] + c.R[4] * X[1] + c.R[5] * X[2] + c.t[1];
        const double z = c.R[6] * X[0] + c.R[7] * X[1] + c.R[8] * X[2] + c.t[2];
        const double xz = x / z, yz = y / z, ru = c.fx * xz + c.cx - c.u, rv = c.fy * yz + c.cy - c.v;
        double ju[3], jv[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) ju[j] = c.fx * (c.R[j] - xz * c.R[6 + j]) / z, jv[j] = c.fy * (c.R[3 + j] - yz * c.R[6 + j]) / z;
        A[0] += ju[0] * ju[0] + jv[0] * jv[0], A[1] += ju[0] * ju[1] + jv[0] * jv[1], A[2] += ju[0] * ju[2] + jv[0] * jv[2];
        A[3] += ju[1] * ju[1] + jv[1] * jv[1], A[4] += ju[1] * ju[2] + jv[1] * jv[2], A[5] += ju[2] * ju[2] + jv[2] * jv[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) g[j] += -(ju[j] * ru + jv[j] * rv);
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) A[j] = tri_gsum<G>(A[j]);
#pragma unroll
      for (int j = 0; j < 3; ++j) g[j] = tri_gsum<G>(g[j]);
      double step[3];
      const double det = tri_solve(A, g, step);
      if (!(det > 0.0)) break;
      const double Y[3] = {X[0] + step[0], X[1] + step[1], X[2] + step[2]};
      double cost_y;
      const bool front = cost_of(Y, cost_y);
      if (!(front && cost_y < cost)) break;                    // (a NaN anywhere refuses the round)
      X[0] = Y[0], X[1] = Y[1], X[2] = Y[2], cost = cost_y;
    }
  }

  // ---- classify every usable observation at X
  int n_in = 0, kmin = 0x7fffffff, kmax_neg = 0x7fffffff;
  double sum = 0.0;
  for (int idx = lane; idx < Lu; idx += G) {
    TriCam cam;
    cam_of(idx, cam);
    double z, e2;
    tri_reproject(cam, X, z, e2);
    const bool in = z > 0.0 && e2 <= a.thresh2;
    const double err = sqrt(e2);
    s.set_in(idx, in);
    s.uv[2 * idx] = z > 0.0 && err == err ? (err < (double)FLT_MAX ? (float)err : FLT_MAX) : -1.f;
    if (in) {
      ++n_in, sum += e2;
      const int k = s.k[idx];
      kmin = k < kmin ? k : kmin;
      kmax_neg = -k < kmax_neg ? -k : kmax_neg;
    }
    const double *c = s.c + 3 * idx;                           // the unit vector centre -> X, for the angles below
    const double v0 = X[0] - c[0], v1 = X[1] - c[1], v2 = X[2] - c[2], len = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
    s.d[3 * idx] = v0 / len, s.d[3 * idx + 1] = v1 / len, s.d[3 * idx + 2] = v2 / len;
  }
  n_in = tri_gsum<G>(n_in);
  sum = tri_gsum<G>(sum);
  kmin = tri_gmin<G>(kmin);
  kmax_neg = tri_gmin<G>(kmax_neg);
  __builtin_amdgcn_wave_barrier();
  if (n_in < 2 || kmin == -kmax_neg) return no_model();        // fewer than two inliers, or all of them in one image

  // ---- the largest angle among the final inliers: the pair of the smallest cosine (first pair on a tie), then its angle
  double best = 2.0;
  int pair = 0x7fffffff;
  for (int pi = lane; pi < Lu; pi += G) {
    if (!s.in(pi)) continue;
    const double a0 = s.d[3 * pi], a1 = s.d[3 * pi + 1], a2 = s.d[3 * pi + 2];
    for (int qi = pi + 1; qi < Lu; ++qi) {
      if (!s.in(qi)) continue;
      const double cs = a0 * s.d[3 * qi] + a1 * s.d[3 * qi + 1] + a2 * s.d[3 * qi + 2];
      if (cs < best) best = cs, pair = pi * TRI_MAX_OBS + qi;
    }
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o, G);
    const int op = __shfl_xor(pair, o, G);
    if (ob < best || (ob == best && op < pair)) best = ob, pair = op;
  }
  double angle = 0.0;
  if (pair != 0x7fffffff) angle = tri_angle(X, s.c + 3 * (pair / TRI_MAX_OBS), s.c + 3 * (pair % TRI_MAX_OBS));
  if (!(angle == angle)) angle = 0.0;
  const int status = angle < a.min_angle ? TRI_LOW_ANGLE : 0;

  for (int idx = lane; idx < Lu; idx += G) {
    a.out.obs_error[beg + s.o(idx)] = s.uv[2 * idx];
    a.out.obs_inlier[beg + s.o(idx)] = s.in(idx);
  }
  if (lane == 0) {
    tri_write_track(a.out, t, status, X, (float)angle, (float)sqrt(sum / (double)n_in), n_in);
    atomicAdd(cnt + (status ? TRI_N_LOW_ANGLE : TRI_N_OK), 1);
    atomicAdd(cnt + TRI_N_INLIER_OBS, n_in);
  }
}

// A workgroup of THREADS / G groups walks the tracks of its class by the grid's stride: the short ones by their number (a group whose track
// is of another class steps on), the mid and long ones through the lists of tri_classify_kernel.  The counters are summed in LDS first.
template <int G, int CAP, int THREADS, int CLS>
__global__ __launch_bounds__(THREADS) void tri_track_kernel(TriArgs a) {
  constexpr int GROUPS = THREADS / G;
  __shared__ double s_d[GROUPS * CAP * 3], s_c[GROUPS * CAP * 3];
  __shared__ float s_uv[GROUPS * CAP * 2];
  __shared__ int s_k[GROUPS * CAP], s_cnt[TRI_COUNTERS];
  __shared__ uint16_t s_oi[GROUPS * CAP];
  const int group = threadIdx.x / G, lane = threadIdx.x % G, wave_lane = threadIdx.x & 63;
  if (threadIdx.x < TRI_COUNTERS) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const TriLds s = {s_d + group * CAP * 3, s_c + group * CAP * 3, s_uv + group * CAP * 2, s_k + group * CAP, s_oi + group * CAP};
  int count = a.T;
  const int32_t* list = nullptr;
  if (CLS != TRI_CLS_SHORT) {
    list = CLS == TRI_CLS_MID ? a.out.list_mid : a.out.list_long;
    const int n = a.out.n_list[CLS - TRI_CLS_MID];
    count = n < 0 ? 0 : n < a.T ? n : a.T;
  }
  for (int64_t w = (int64_t)blockIdx.x * GROUPS + group; w < count; w += (int64_t)gridDim.x * GROUPS) {
    int t = (int)w;
    if (CLS != TRI_CLS_SHORT) {
      t = list[w];
      if (t < 0 || t >= a.T) continue;                         // (never: classify wrote it)
    }
    int beg, L;
    const bool mine = tri_range(a, t, beg, L) && (CLS == TRI_CLS_SHORT ? L <= TRI_SHORT : CLS == TRI_CLS_MID ? L > TRI_SHORT && L <= TRI_MID : L > TRI_MID);
    if (mine) tri_track<G, CAP>(a, t, lane, wave_lane, s, s_cnt);
  }
  __syncthreads();
  if (threadIdx.x < TRI_COUNTERS && s_cnt[threadIdx.x]) atomicAdd(a.out.counters + threadIdx.x, s_cnt[threadIdx.x]);
}

// the sizes that lay the buffer out: the op and gims_aux_layout refuse the same values
static int tri_check_sizes(int64_t T, int64_t n_obs) {
  GIMS_CHECK_ARG(T >= 0 && T <= (1 << 30), "triangulate_tracks: T = %lld is out of range (0 .. 2^30)", (long long)T);
  GIMS_CHECK_ARG(n_obs >= 0 && n_obs <= (1 << 30), "triangulate_tracks: n_obs = %lld is out of range (0 .. 2^30)", (long long)n_obs);
  return GIMS_OK;
}

// gims_aux_layout for GIMS_AUX_TRIANGULATE_TRACKS: sizes = {T, n_obs}
int triangulate_tracks_aux_layout(const int64_t* sizes, int n, WsRecord& rec) {
  GIMS_CHECK_ARG(n == 2, "triangulate_tracks: the layout takes 2 sizes {T, n_obs}, not %d", n);
  if (const int rc = tri_check_sizes(sizes[0], sizes[1])) return rc;
  TriOut w;
  rec.bytes = tri_layout(nullptr, sizes[0], sizes[1], w, &rec);
  return GIMS_OK;
}

// GIMS_AUX_TRIANGULATE_TRACKS of gims_run_ops (include/gims_hip.h): every argument check precedes the first HIP call
int triangulate_tracks_aux(const gims_aux_args& x, hipStream_t st) {
  const int64_t T = x.i[0], n_obs = x.i[1], n_images = x.i[2], N = x.i[3], mode = x.i[4];
  const float thresh = x.f[0], min_angle = x.f[1];
  // i[5] is where a later form of this function would be selected: it is read FIRST (see assemble_rows_aux)
  GIMS_CHECK_ARG(x.i[5] == 0, "gims_run_ops: unknown auxiliary function form: triangulate_tracks with i[5] = %lld (i[5] is reserved and must be 0)",
                 (long long)x.i[5]);
  if (const int rc = tri_check_sizes(T, n_obs)) return rc;
  GIMS_CHECK_ARG(n_images >= 0 && n_images <= (1 << 24), "triangulate_tracks: n_images = %lld is out of range (0 .. 2^24)", (long long)n_images);
  GIMS_CHECK_ARG(N >= 0 && N <= (1 << 30), "triangulate_tracks: N = %lld is out of range (0 .. 2^30)", (long long)N);
  const int64_t max_hyp = mode & 0xffff, refine_iters = mode >> 16;
  GIMS_CHECK_ARG(mode >= 0 && refine_iters <= 255,
                 "triangulate_tracks: i[4] = %lld: max_hyp | refine_iters << 16 with max_hyp in 0 .. 65535 and refine_iters in 0 .. 255", (long long)mode);
  GIMS_CHECK_ARG(thresh - thresh == 0.f && thresh > 0.f, "triangulate_tracks: thresh = %g must be finite and > 0", (double)thresh);
  GIMS_CHECK_ARG(min_angle - min_angle == 0.f && min_angle >= 0.f && min_angle < 180.f, "triangulate_tracks: min_angle = %g must be in [0, 180)",
                 (double)min_angle);
  GIMS_CHECK_ARG(x.p[5], "triangulate_tracks: the output buffer is NULL");
  GIMS_CHECK_ARG(T == 0 || (x.p[0] && x.p[1] && x.p[2] && x.p[3] && x.p[4]),
                 "triangulate_tracks: indptr, obs_image, obs_keypoint, kpts or cams is NULL while T = %lld", (long long)T);
  GIMS_CHECK_ARG((((uintptr_t)x.p[4] | (uintptr_t)x.p[5]) & 7) == 0, "triangulate_tracks: cams and the output buffer must be 8-byte aligned");
  GIMS_CHECK_ARG((((uintptr_t)x.p[0] | (uintptr_t)x.p[1] | (uintptr_t)x.p[2] | (uintptr_t)x.p[3]) & 3) == 0,
                 "triangulate_tracks: indptr, obs_image, obs_keypoint and kpts must be 4-byte aligned");

  TriArgs a;
  tri_layout((void*)x.p[5], T, n_obs, a.out);
  GIMS_HIP(hipMemsetAsync(a.out.counters, 0, sizeof(int32_t) * TRI_COUNTERS, st));
  if (T == 0) return GIMS_OK;
  a.indptr = (const int32_t*)x.p[0], a.obs_image = (const int32_t*)x.p[1], a.obs_keypoint = (const int32_t*)x.p[2];
  a.kpts = (const float*)x.p[3], a.cams = (const double*)x.p[4];
  a.T = (int)T, a.n_obs = (int)n_obs, a.n_images = (int)n_images, a.N = N, a.max_hyp = (int)max_hyp, a.refine_iters = (int)refine_iters;
  a.thresh2 = (double)thresh * (double)thresh, a.min_angle = (double)min_angle;
  GIMS_HIP(hipMemsetAsync(a.out.n_list, 0, sizeof(int32_t) * 2, st));
  if (n_obs > 0) {
    GIMS_HIP(hipMemsetD32Async((hipDeviceptr_t)a.out.obs_error, (int)0xBF800000u, (size_t)n_obs, st));      // -1.f
    GIMS_HIP(hipMemsetAsync(a.out.obs_inlier, 0, (size_t)n_obs, st));
  }
  tri_classify_kernel<<<cdiv(T, TRI_THREADS), TRI_THREADS, 0, st>>>(a);
  GIMS_LAUNCH_CHECK();
  const int64_t full = (int64_t)device_cus() * 8;
  auto grid = [&](int64_t blocks, int64_t cap) { return (unsigned)(blocks < cap ? blocks : cap); };
  tri_track_kernel<TRI_SHORT, TRI_SHORT, TRI_THREADS, TRI_CLS_SHORT><<<grid(cdiv(T, TRI_THREADS / TRI_SHORT), full), TRI_THREADS, 0, st>>>(a);
  GIMS_LAUNCH_CHECK();
  tri_track_kernel<64, TRI_MID, TRI_THREADS, TRI_CLS_MID><<<grid(cdiv(T, TRI_THREADS / 64), full), TRI_THREADS, 0, st>>>(a);
  GIMS_LAUNCH_CHECK();
  tri_track_kernel<64, TRI_MAX_OBS, 64, TRI_CLS_LONG><<<grid(T, full / 4), 64, 0, st>>>(a);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

}  // namespace gims
