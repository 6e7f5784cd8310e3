// Bundle adjustment: GIMS_AUX_BUNDLE_ADJUST of gims_run_ops refines the free cameras and the active points of a Tracks /
// Points3D / camera-record set jointly, by Levenberg-Marquardt rounds on the reprojection cost with the Schur complement over the points.
// include/gims_hip.h has the contract; tests/ba_ref.py is the NumPy restatement.  All arithmetic is float64 on the vector ALU, compiled
// without contraction into fused multiply-adds, so the operations are the ones the specification states.
//
// Launches, the same whatever the data (n_free = the cameras of mode 2, counted on the host): memset nodes -> the slot tables (upload_table)
// -> init (copies, the record check) -> classify (a thread per track: active observations and points, cam_obs) -> slots (held cameras, the
// scan of the list sizes) -> fill (a workgroup per slot: its observations in ascending order) -> prep (a thread per track: the moving
// slot of every observation) -> cost + decide (the starting cost) ->
// per round { point (a thread per track: V, g_p, V*^-1, W, W V*^-1) -> camera (a wave per slot: U, g_c, its block row of S in LDS) ->
// solve (one workgroup: Cholesky, the two substitutions, the candidate cameras) -> back (a thread per track: the candidate point, its
// cost) -> decide (one workgroup: the ordered sum of the costs, one thread decides) } -> finish.  camera and solve are left out when
// n_free == 0.  The state (cost, lambda, which of the two buffers is current, the reject count) lives in a block on the device.
// Every floating-point sum has one order: a track's observations ascending in one thread; a camera's observations as the lane's own
// ascending sum and a butterfly over the wave (U, g_c), or one after the other (the block row); the tracks' costs as a thread's own
// ascending sum, a butterfly, then the waves in order.  No order depends on the grid.
// GIMS_AUX_BUNDLE_ADJUST_PCG, further down, shares init, classify, point, back, decide and finish and replaces camera and
// solve by a matrix-free conjugate-gradient iteration, so that the number of free cameras is not bound by a dense reduced system.
// GIMS_AUX_BUNDLE_ADJUST_FOCAL, behind that, is the conjugate-gradient form with one more unknown per focal group: it launches
// the kernels of the two forms above as they are and adds kernels of its own for the group terms.
#include "common.h"

#include <cfloat>
#include <cstring>
#include <vector>

namespace gims {

constexpr int BA_CAM = GIMS_TRI_CAMERA_WORDS;
constexpr int BA_MAX_OBS = GIMS_TRI_MAX_OBS;
constexpr int BA_MAX_FREE = GIMS_BA_MAX_FREE_CAMERAS;
constexpr int BA_MAX_REJECTS = GIMS_BA_MAX_REJECTS;
constexpr int BA_THREADS = 256;
constexpr int BA_SOLVE_THREADS = 1024;
constexpr int BA_REC = 50;                                     // per observation: Ju, Jv [12] | ru, rv [2] | W [6][3] | W V*^-1 [6][3]
constexpr int BA_PT = 9;                                       // per point: V*^-1 (a00 a01 a02 a11 a12 a22) | g_p [3]
enum { BA_N_FREE = 0, BA_N_FIXED, BA_N_HELD, BA_N_POINTS, BA_N_ACTIVE_OBS, BA_N_BAD_OBS, BA_ROUNDS_TAKEN, BA_STATUS, BA_COUNTERS = 8 };
enum { BA_BAD_CAMERA = 1, BA_BAD_START = 2 };
enum { BA_F_IRREGULAR = 1, BA_F_NOT_FINITE = 2, BA_F_BEHIND = 4 };
enum { BA_ABSENT = -1, BA_FIXED = -2 };                        // slot_of: or the slot 0 .. n_free - 1 of a camera of mode 2

struct BaState {                                               // 256 bytes, zeroed by a memset node
  double cost, lambda;
  int32_t cur, rejects, stop, taken, status, flags, n_points, n_act, n_bad, n_held;
  double rho, rho0;                                            // the conjugate-gradient form only, from here on
  int32_t cg_done, cg_used;
};

struct BaOut {
  double *xyz, *cams, *history;                                // xyz and cams are also buffer 0 of the state
  float* obs_error;
  int32_t *cam_obs, *counters;
  uint8_t* taken;
  BaState* st;                                                 // scratch from here on
  int32_t *slot_of, *slot_cam, *slot_ptr, *held, *obs_track, *obs_node, *cam_list, *obs_mslot, *obs_dup;
  double *xyz1, *cams1, *pt_rec, *obs_rec, *trackcost, *S, *rhs;
  uint8_t *pt_act, *obs_act;
  int32_t *cg_used, *list_tmp, *cursor;                        // the conjugate-gradient form only, from here on (rhs is its x, S stays NULL)
  double *cg_res, *y, *slot_rec, *vr, *vz, *vp, *vq;
};
static size_t ba_layout(void* base, int64_t T, int64_t n_obs, int64_t n_images, int64_t iters, int64_t n_free, BaOut& w, WsRecord* rec = nullptr) {
  WsLayout L(base, rec);
  const size_t n = (size_t)(6 * n_free);
  w.xyz = L.take<double>((size_t)T * 3);
  w.cams = L.take<double>((size_t)n_images * BA_CAM);
  w.obs_error = L.take<float>((size_t)n_obs);
  w.cam_obs = L.take<int32_t>((size_t)n_images);
  w.history = L.take<double>((size_t)(iters + 1) * 2);
  w.taken = L.take<uint8_t>((size_t)iters);
  w.counters = L.take<int32_t>(BA_COUNTERS);
  L.scratch_from_here();
  w.st = (BaState*)L.take<double>(32);
  w.slot_of = L.take<int32_t>((size_t)n_images);
  w.slot_cam = L.take<int32_t>((size_t)n_free);
  w.slot_ptr = L.take<int32_t>((size_t)n_free + 1);
  w.held = L.take<int32_t>((size_t)n_free);
  w.xyz1 = L.take<double>((size_t)T * 3);
  w.cams1 = L.take<double>((size_t)n_images * BA_CAM);
  w.pt_act = L.take<uint8_t>((size_t)T);
  w.obs_act = L.take<uint8_t>((size_t)n_obs);
  w.obs_track = L.take<int32_t>((size_t)n_obs);
  w.obs_node = L.take<int32_t>((size_t)n_obs);
  w.cam_list = L.take<int32_t>((size_t)n_obs);
  w.obs_mslot = L.take<int32_t>((size_t)n_obs);
  w.obs_dup = L.take<int32_t>((size_t)n_obs);
  w.pt_rec = L.take<double>((size_t)T * BA_PT);
  w.obs_rec = L.take<double>((size_t)n_obs * BA_REC);
  w.trackcost = L.take<double>((size_t)T);
  w.S = L.take<double>(n * n);
  w.rhs = L.take<double>(n);
  return L.bytes();
}

struct BaArgs {
  const int32_t *indptr, *obs_image, *obs_keypoint;
  const uint8_t *obs_use, *point_use;
  const float* kpts;
  const double *xyz_in, *cams_in;
  BaOut out;
  int T, n_obs, n_images, iters, n_free, n_fixed;
  int64_t N;
  double huber, lambda0;
  int cg_iters;                                                // the conjugate-gradient form only
  double cg_tol2;
};

__device__ __forceinline__ bool ba_finite(double x) { return fabs(x) <= DBL_MAX; }       // (false for a NaN)
__device__ __forceinline__ double* ba_xyz(const BaArgs& a, int which) { return which ? a.out.xyz1 : a.out.xyz; }
__device__ __forceinline__ double* ba_cams(const BaArgs& a, int which) { return which ? a.out.cams1 : a.out.cams; }
__device__ __forceinline__ bool ba_range(const BaArgs& a, int t, int& beg, int& len) {
  const int b = a.indptr[t], e = a.indptr[t + 1];
  beg = b;
  len = e - b;
  return b >= 0 && e >= b && e <= a.n_obs && e - b <= BA_MAX_OBS;
}
// the slot of an observation's camera when that camera moves (mode 2 and not held), else -1; k is in range (the observation is active)
__device__ __forceinline__ int ba_moving_slot(const BaArgs& a, int k) {
  const int s = a.out.slot_of[k];
  return s >= 0 && s < a.n_free && a.out.held[s] == 0 ? s : -1;
}

// residual, depth and, when J is asked for, the Jacobians of one observation: c = the camera record, X the point, (u, v) the pixel
struct BaJac { double ju[6], jv[6], pu[3], pv[3]; };
template <bool JAC>
__device__ __forceinline__ void ba_observe(const double* c, const double* X, double u, double v, double& ru, double& rv, double& z, BaJac* J) {
  const double fx = c[0], fy = c[1], cx = c[2], cy = c[3];
  const double* R = c + 4;
  const double y0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2], y1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2], y2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2];
  const double x = y0 + c[13], y = y1 + c[14];
  z = y2 + c[15];
  ru = fx * x / z + cx - u, rv = fy * y / z + cy - v;
  if (JAC) {
    const double au = fx / z, bu = -fx * x / (z * z), av = fy / z, bv = -fy * y / (z * z);
    J->ju[0] = bu * y1, J->ju[1] = au * y2 - bu * y0, J->ju[2] = -au * y1, J->ju[3] = au, J->ju[4] = 0.0, J->ju[5] = bu;
    J->jv[0] = bv * y1 - av * y2, J->jv[1] = -bv * y0, J->jv[2] = av * y0, J->jv[3] = 0.0, J->jv[4] = av, J->jv[5] = bv;
#pragma unroll
    for (int m = 0; m < 3; ++m) J->pu[m] = au * R[m] + bu * R[6 + m], J->pv[m] = av * R[3 + m] + bv * R[6 + m];
  }
}
// rho(e^2) of the cost
__device__ __forceinline__ double ba_rho(double e2, double huber) {
  if (!(huber > 0.0)) return e2;
  const double e = sqrt(e2);
  return e <= huber ? e2 : 2.0 * huber * e - huber * huber;
}

// ---------------------------------------------------------------------------------------------- init
__global__ __launch_bounds__(BA_THREADS) void ba_init_kernel(BaArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BA_THREADS + threadIdx.x;
  if (i == 0) a.out.st->lambda = a.lambda0;
  if (i < a.n_images) {
    bool good = true;
    for (int j = 0; j < BA_CAM; ++j) {
      const double w = a.cams_in[i * BA_CAM + j];
      a.out.cams[i * BA_CAM + j] = w, a.out.cams1[i * BA_CAM + j] = w;
      good = good && ba_finite(w);
    }
    good = good && a.cams_in[i * BA_CAM] > 0.0 && a.cams_in[i * BA_CAM + 1] > 0.0;
    if (a.out.slot_of[i] != BA_ABSENT && !good) atomicOr(&a.out.st->status, BA_BAD_CAMERA);
    a.out.cam_obs[i] = 0;
  }
  if (i < a.T)
    for (int j = 0; j < 3; ++j) {
      const double w = a.xyz_in[i * 3 + j];
      a.out.xyz[i * 3 + j] = w, a.out.xyz1[i * 3 + j] = w;
    }
}

// ---------------------------------------------------------------------------------------------- classify
__global__ __launch_bounds__(BA_THREADS) void ba_classify_kernel(BaArgs a) {
  const int t = blockIdx.x * BA_THREADS + threadIdx.x;
  if (t >= a.T) return;
  a.out.trackcost[t] = 0.0;
  a.out.pt_act[t] = 0;
  int beg, len;
  if (!ba_range(a, t, beg, len)) return;                       // a bad range, or a track that is too long: it touches no observation
  const double* X = a.xyz_in + (int64_t)3 * t;
  const bool point = a.point_use[t] != 0 && ba_finite(X[0]) && ba_finite(X[1]) && ba_finite(X[2]);
  int n = 0;
  for (int o = beg; o < beg + len; ++o) {
    bool ok = false;
    const int k = a.obs_image[o], i = a.obs_keypoint[o];
    if (point && a.obs_use[o] != 0 && k >= 0 && k < a.n_images && a.out.slot_of[k] != BA_ABSENT) {
      const double* r = a.cams_in + (int64_t)BA_CAM * k;
      bool fin = true;
      for (int j = 0; j < BA_CAM; ++j) fin = fin && ba_finite(r[j]);
      const double node = r[16] + (double)i;
      if (fin && r[0] > 0.0 && r[1] > 0.0 && i >= 0 && (double)i < r[17] && node >= 0.0 && node < (double)a.N) {
        const int64_t g = (int64_t)node;                       // 0 .. N - 1
        if (ba_finite((double)a.kpts[2 * g]) && ba_finite((double)a.kpts[2 * g + 1])) {
          ok = true;
          a.out.obs_node[o] = (int32_t)g;
        }
      }
    }
    a.out.obs_act[o] = ok ? 1 : 0;
    n += ok ? 1 : 0;
  }
  const bool active = n >= 2;
  a.out.pt_act[t] = active ? 1 : 0;
  for (int o = beg; o < beg + len; ++o) {
    if (a.out.obs_act[o] == 0) continue;
    if (!active) {
      a.out.obs_act[o] = 0;
      continue;
    }
    a.out.obs_track[o] = t;
    atomicAdd(a.out.cam_obs + a.obs_image[o], 1);              // integers: the order of the race changes nothing
  }
  if (active) atomicAdd(&a.out.st->n_points, 1), atomicAdd(&a.out.st->n_act, n);
  if (len - (active ? n : 0) > 0) atomicAdd(&a.out.st->n_bad, len - (active ? n : 0));
}

// ---------------------------------------------------------------------------------------------- slots, lists
__global__ __launch_bounds__(BA_MAX_FREE) void ba_slots_kernel(BaArgs a) {
  const int s = threadIdx.x;
  if (s < a.n_free) a.out.held[s] = a.out.cam_obs[a.out.slot_cam[s]] < 4 ? 1 : 0;
  __syncthreads();
  if (s == 0) {
    int at = 0, held = 0;
    for (int j = 0; j < a.n_free; ++j) {
      a.out.slot_ptr[j] = at;
      if (a.out.held[j]) ++held; else at += a.out.cam_obs[a.out.slot_cam[j]];
    }
    a.out.slot_ptr[a.n_free] = at;                             // <= n_obs: every active observation has one camera
    a.out.st->n_held = held;
  }
}

__global__ __launch_bounds__(BA_THREADS) void ba_fill_kernel(BaArgs a) {
  __shared__ int s_w[BA_THREADS / 64];
  const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (a.out.held[s]) return;                                   // (the same for every thread)
  const int cam = a.out.slot_cam[s], first = a.out.slot_ptr[s], cap = a.out.slot_ptr[s + 1] - first;
  int K = 0;
  for (int o0 = 0; o0 < a.n_obs; o0 += BA_THREADS) {
    const int o = o0 + t;
    const bool ok = o < a.n_obs && a.out.obs_act[o] != 0 && a.obs_image[o] == cam;
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) s_w[wave] = __popcll(bal);
    __syncthreads();
    int before = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < BA_THREADS / 64; ++w) {
      before += w < wave ? s_w[w] : 0;
      total += s_w[w];
    }
    const int at = K + before;
    if (ok && at < cap && first >= 0 && first + at < a.n_obs) a.out.cam_list[first + at] = o;
    K += total;
    __syncthreads();
  }
}

// The slot of every observation whose camera moves (-1 otherwise), and how many earlier observations of its track lie in the same slot:
// both hold for the whole call, and the camera kernel orders two observations of one track in one image by the second.
__global__ __launch_bounds__(BA_THREADS) void ba_prep_kernel(BaArgs a) {
  const int t = blockIdx.x * BA_THREADS + threadIdx.x;
  if (t >= a.T || a.out.pt_act[t] == 0) return;
  int beg, len;
  if (!ba_range(a, t, beg, len)) return;                       // (never: the point is active)
  for (int o = beg; o < beg + len; ++o) {
    const int m = a.out.obs_act[o] != 0 ? ba_moving_slot(a, a.obs_image[o]) : -1;
    int dup = 0;
    for (int o2 = beg; o2 < o && m >= 0; ++o2) dup += a.out.obs_mslot[o2] == m ? 1 : 0;
    a.out.obs_mslot[o] = m, a.out.obs_dup[o] = dup;
  }
}

// ---------------------------------------------------------------------------------------------- point
__global__ __launch_bounds__(BA_THREADS) void ba_point_kernel(BaArgs a) {
  const int t = blockIdx.x * BA_THREADS + threadIdx.x;
  const BaState* st = a.out.st;
  if (t >= a.T || st->stop || a.out.pt_act[t] == 0) return;
  int beg, len;
  if (!ba_range(a, t, beg, len)) return;                       // (never: the point is active)
  const double lambda = st->lambda;
  const double* cams = ba_cams(a, st->cur);
  const double* Xp = ba_xyz(a, st->cur) + (int64_t)3 * t;
  const double X[3] = {Xp[0], Xp[1], Xp[2]};
  double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
  for (int o = beg; o < beg + len; ++o) {
    if (a.out.obs_act[o] == 0) continue;
    const int k = a.obs_image[o];
    const int64_t node = a.out.obs_node[o];
    BaJac J;
    double ru, rv, z;
    ba_observe<true>(cams + (int64_t)BA_CAM * k, X, (double)a.kpts[2 * node], (double)a.kpts[2 * node + 1], ru, rv, z, &J);
    if (a.huber > 0.0) {
      const double e = sqrt(ru * ru + rv * rv);
      if (e > a.huber) {
        const double sw = sqrt(a.huber / e);
        ru = ru * sw, rv = rv * sw;
#pragma unroll
        for (int j = 0; j < 6; ++j) J.ju[j] = J.ju[j] * sw, J.jv[j] = J.jv[j] * sw;
#pragma unroll
        for (int j = 0; j < 3; ++j) J.pu[j] = J.pu[j] * sw, J.pv[j] = J.pv[j] * sw;
      }
    }
    V[0] += J.pu[0] * J.pu[0] + J.pv[0] * J.pv[0], V[1] += J.pu[0] * J.pu[1] + J.pv[0] * J.pv[1], V[2] += J.pu[0] * J.pu[2] + J.pv[0] * J.pv[2];
    V[3] += J.pu[1] * J.pu[1] + J.pv[1] * J.pv[1], V[4] += J.pu[1] * J.pu[2] + J.pv[1] * J.pv[2], V[5] += J.pu[2] * J.pu[2] + J.pv[2] * J.pv[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) g[j] += J.pu[j] * ru + J.pv[j] * rv;
    double* rec = a.out.obs_rec + (int64_t)BA_REC * o;
#pragma unroll
    for (int j = 0; j < 6; ++j) rec[j] = J.ju[j], rec[6 + j] = J.jv[j];
    rec[12] = ru, rec[13] = rv;
#pragma unroll
    for (int j = 0; j < 3; ++j) rec[14 + j] = J.pu[j], rec[17 + j] = J.pv[j];      // (until the second pass below)
  }
  V[0] += lambda * fmax(V[0], 1e-6), V[3] += lambda * fmax(V[3], 1e-6), V[5] += lambda * fmax(V[5], 1e-6);
  const double c00 = V[3] * V[5] - V[4] * V[4], c01 = V[2] * V[4] - V[1] * V[5], c02 = V[1] * V[4] - V[2] * V[3];
  const double c11 = V[0] * V[5] - V[2] * V[2], c12 = V[1] * V[2] - V[0] * V[4], c22 = V[0] * V[3] - V[1] * V[1];
  const double det = V[0] * c00 + V[1] * c01 + V[2] * c02;
  if (!(ba_finite(det) && det > 0.0)) atomicOr(&a.out.st->flags, BA_F_IRREGULAR);
  const double I[3][3] = {{c00 / det, c01 / det, c02 / det}, {c01 / det, c11 / det, c12 / det}, {c02 / det, c12 / det, c22 / det}};
  double* pr = a.out.pt_rec + (int64_t)BA_PT * t;
  pr[0] = I[0][0], pr[1] = I[0][1], pr[2] = I[0][2], pr[3] = I[1][1], pr[4] = I[1][2], pr[5] = I[2][2];
  pr[6] = g[0], pr[7] = g[1], pr[8] = g[2];
  if (a.n_free == 0) return;
  for (int o = beg; o < beg + len; ++o) {
    if (a.out.obs_act[o] == 0 || ba_moving_slot(a, a.obs_image[o]) < 0) continue;
    double* rec = a.out.obs_rec + (int64_t)BA_REC * o;
    const double pu[3] = {rec[14], rec[15], rec[16]}, pv[3] = {rec[17], rec[18], rec[19]};
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const double ju = rec[c], jv = rec[6 + c];
      const double w[3] = {ju * pu[0] + jv * pv[0], ju * pu[1] + jv * pv[1], ju * pu[2] + jv * pv[2]};
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        rec[14 + 3 * c + m] = w[m];
        rec[32 + 3 * c + m] = w[0] * I[0][m] + w[1] * I[1][m] + w[2] * I[2][m];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- camera
// One wave per slot.  U and g_c: the lane's own sum over its observations of the list (lane, lane + 64, ...), then a butterfly.  The block
// row of S: the observations of the list one after the other; for each, lane j takes observation j of its track and subtracts its 6 x 6
// block from the column block of its slot (different slots: different entries; the same slot: in turn), lanes 0 .. 5 the right-hand side.
__global__ __launch_bounds__(64) void ba_camera_kernel(BaArgs a) {
  __shared__ double s_row[6 * 6 * BA_MAX_FREE], s_b[6];
  const int s = blockIdx.x, lane = threadIdx.x, n = 6 * a.n_free;
  const BaState* st = a.out.st;
  if (st->stop) return;
  double* Srow = a.out.S + (int64_t)6 * s * n;
  if (a.out.held[s]) {                                         // a held camera does not move: an identity block, a zero right-hand side
    for (int e = lane; e < 6 * n; e += 64) Srow[e] = e % n == 6 * s + e / n ? 1.0 : 0.0;
    if (lane < 6) a.out.rhs[6 * s + lane] = 0.0;
    return;
  }
  const int first = a.out.slot_ptr[s];
  int cnt = a.out.slot_ptr[s + 1] - first;
  if (first < 0 || cnt < 0 || first + cnt > a.n_obs) cnt = 0;   // (never: ba_slots_kernel wrote them)
  const int32_t* list = a.out.cam_list + first;
  double acc[27];
#pragma unroll
  for (int j = 0; j < 27; ++j) acc[j] = 0.0;
  for (int idx = lane; idx < cnt; idx += 64) {
    const int o = list[idx];
    if (o < 0 || o >= a.n_obs) continue;                       // (never)
    const double* rec = a.out.obs_rec + (int64_t)BA_REC * o;
    double ju[6], jv[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) ju[j] = rec[j], jv[j] = rec[6 + j];
    const double ru = rec[12], rv = rec[13];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) acc[k++] += ju[i] * ju[j] + jv[i] * jv[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += ju[i] * ru + jv[i] * rv;
  }
#pragma unroll
  for (int j = 0; j < 27; ++j)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
  for (int e = lane; e < 6 * n; e += 64) s_row[e] = 0.0;
  __syncthreads();
  const double lambda = st->lambda;
  if (lane < 36) {
    const int r = lane / 6, c = lane % 6, i = r < c ? r : c, j = r < c ? c : r;
    double u = 0.0;
    int k = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
      for (int q = p; q < 6; ++q) {
        if (p == i && q == j) u = acc[k];
        ++k;
      }
    if (r == c) u += lambda * fmax(u, 1e-6);
    s_row[r * n + 6 * s + c] = u;
  } else if (lane < 42) {
    double gc = 0.0;
#pragma unroll
    for (int p = 0; p < 6; ++p)
      if (p == lane - 36) gc = acc[21 + p];
    s_b[lane - 36] = -gc;
  }
  __syncthreads();
  for (int idx = 0; idx < cnt; ++idx) {
    const int o = list[idx];
    if (o < 0 || o >= a.n_obs) continue;                       // (never; the same for every lane)
    const int p = a.out.obs_track[o];
    int beg, len;
    if (p < 0 || p >= a.T || !ba_range(a, p, beg, len)) continue;
    const double* rec = a.out.obs_rec + (int64_t)BA_REC * o;
    double y[18];
#pragma unroll
    for (int j = 0; j < 18; ++j) y[j] = rec[32 + j];           // (one address for the wave)
    if (lane < 6) {
      const double* gp = a.out.pt_rec + (int64_t)BA_PT * p + 6;
      double v = 0.0;
#pragma unroll
      for (int r = 0; r < 6; ++r)
        if (r == lane) v = (y[3 * r] * gp[0] + y[3 * r + 1] * gp[1]) + y[3 * r + 2] * gp[2];
      s_b[lane] += v;
    }
    // lane j takes observation j of the track (in passes of 64): its whole 6 x 6 block, into the column block of its own slot; two
    // observations of the track in one slot go in turn, the earlier first (obs_dup), so every entry keeps the order of the specification
    for (int o0 = 0; o0 < len; o0 += 64) {
      const int o2 = beg + o0 + lane;
      const int k2 = o0 + lane < len ? a.out.obs_mslot[o2] : -1;
      const int dup = k2 >= 0 ? a.out.obs_dup[o2] : 0;
      double w[18];
      if (k2 >= 0 && k2 < a.n_free) {
        const double* wr = a.out.obs_rec + (int64_t)BA_REC * o2 + 14;
#pragma unroll
        for (int j = 0; j < 18; ++j) w[j] = wr[j];
      }
      bool pending = k2 >= 0 && k2 < a.n_free;
      for (int rk = 0; __ballot(pending) != 0ull; ++rk) {
        if (pending && dup <= rk) {
          double* dst = s_row + 6 * k2;
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) dst[r * n + c] -= (y[3 * r] * w[3 * c] + y[3 * r + 1] * w[3 * c + 1]) + y[3 * r + 2] * w[3 * c + 2];
          pending = false;
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  __syncthreads();
  for (int e = lane; e < 6 * n; e += 64) Srow[e] = s_row[e];
  if (lane < 6) a.out.rhs[6 * s + lane] = s_b[lane];
}

// ---------------------------------------------------------------------------------------------- solve
// S = L L^T in place (the lower triangle), column by column: the pivot, the column, then the trailing rows; every entry (i, k) loses
// L[i][j] L[k][j] for j ascending, one product at a time.  L y = b by columns (j ascending), L^T d = y by rows (j descending).
__global__ __launch_bounds__(BA_SOLVE_THREADS) void ba_solve_kernel(BaArgs a) {
  __shared__ double s_col[6 * BA_MAX_FREE], s_b[6 * BA_MAX_FREE], s_y[6 * BA_MAX_FREE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, n = 6 * a.n_free;
  BaState* st = a.out.st;
  if (st->stop) return;
  double* S = a.out.S;
  bool regular = (st->flags & BA_F_IRREGULAR) == 0;            // a point's V* was not regular: there is nothing to solve
  for (int i = t; i < n; i += BA_SOLVE_THREADS) s_b[i] = a.out.rhs[i];
  __syncthreads();
  for (int j = 0; j < n && regular; ++j) {
    const double d = S[(int64_t)j * n + j];
    __syncthreads();
    if (!(ba_finite(d) && d > 0.0)) {                          // the same for every thread
      regular = false;
      break;
    }
    const double l = sqrt(d);
    for (int i = j + t; i < n; i += BA_SOLVE_THREADS) {
      const double v = i == j ? l : S[(int64_t)i * n + j] / l;
      S[(int64_t)i * n + j] = v;
      s_col[i] = v;
    }
    __syncthreads();
    for (int i = j + 1 + wave; i < n; i += BA_SOLVE_THREADS / 64) {
      const double li = s_col[i];
      for (int k = j + 1 + lane; k <= i; k += 64) S[(int64_t)i * n + k] -= li * s_col[k];
    }
    __syncthreads();
  }
  if (regular) {
    for (int j = 0; j < n; ++j) {
      const double yj = s_b[j] / S[(int64_t)j * n + j];
      if (t == 0) s_y[j] = yj;
      for (int i = j + 1 + t; i < n; i += BA_SOLVE_THREADS) s_b[i] -= S[(int64_t)i * n + j] * yj;
      __syncthreads();
    }
    for (int j = n - 1; j >= 0; --j) {
      const double xj = s_y[j] / S[(int64_t)j * n + j];
      if (t == 0) s_b[j] = xj;
      for (int k = t; k < j; k += BA_SOLVE_THREADS) s_y[k] -= S[(int64_t)j * n + k] * xj;
      __syncthreads();
    }
  }
  for (int i = t; i < n; i += BA_SOLVE_THREADS) a.out.rhs[i] = regular ? s_b[i] : 0.0;
  if (!regular) {
    if (t == 0) atomicOr(&st->flags, BA_F_IRREGULAR);
    return;
  }
  if (t < a.n_free && a.out.held[t] == 0) {                    // the candidate camera of slot t, into the buffer that is not current
    const int cam = a.out.slot_cam[t];
    const double* cur = ba_cams(a, st->cur) + (int64_t)BA_CAM * cam;
    double* cand = ba_cams(a, st->cur ^ 1) + (int64_t)BA_CAM * cam;
    const double* d = s_b + 6 * t;
    const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], th = sqrt(th2);
    const double ca = th > 1e-8 ? sin(th) / th : 1.0, cb = th > 1e-8 ? (1.0 - cos(th)) / th2 : 0.5;
    const double W[3][3] = {{0.0, -d[2], d[1]}, {d[2], 0.0, -d[0]}, {-d[1], d[0], 0.0}};
    bool fin = true;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double ex[3];
        for (int m = 0; m < 3; ++m) ex[m] = (i == m ? 1.0 : 0.0) + ca * W[i][m] + cb * (W[i][0] * W[0][m] + W[i][1] * W[1][m] + W[i][2] * W[2][m]);
        const double v = ex[0] * cur[4 + j] + ex[1] * cur[7 + j] + ex[2] * cur[10 + j];
        cand[4 + 3 * i + j] = v;
        fin = fin && ba_finite(v);
      }
    for (int i = 0; i < 3; ++i) {
      const double v = cur[13 + i] + d[3 + i];
      cand[13 + i] = v;
      fin = fin && ba_finite(v);
    }
    if (!fin) atomicOr(&st->flags, BA_F_NOT_FINITE);
  }
}

// ---------------------------------------------------------------------------------------------- back substitution, cost
// initial: the cost of the current state.  Otherwise: the candidate point of the track into the buffer that is not current, and the
// candidate's cost over the track's observations.
__global__ __launch_bounds__(BA_THREADS) void ba_back_kernel(BaArgs a, int initial) {
  const int t = blockIdx.x * BA_THREADS + threadIdx.x;
  BaState* st = a.out.st;
  if (t >= a.T || st->stop || a.out.pt_act[t] == 0) return;
  int beg, len;
  if (!ba_range(a, t, beg, len)) return;                       // (never: the point is active)
  const int which = initial ? st->cur : st->cur ^ 1;
  const double* cams = ba_cams(a, which);
  double X[3];
  if (initial) {
    for (int m = 0; m < 3; ++m) X[m] = ba_xyz(a, which)[(int64_t)3 * t + m];
  } else {
    const double* pr = a.out.pt_rec + (int64_t)BA_PT * t;
    double s[3] = {pr[6], pr[7], pr[8]};
    if (a.n_free > 0)
      for (int o = beg; o < beg + len; ++o) {
        if (a.out.obs_act[o] == 0) continue;
        const int k = ba_moving_slot(a, a.obs_image[o]);
        if (k < 0) continue;
        const double *w = a.out.obs_rec + (int64_t)BA_REC * o + 14, *dc = a.out.rhs + 6 * k;
        for (int c = 0; c < 6; ++c)
#pragma unroll
          for (int m = 0; m < 3; ++m) s[m] += w[3 * c + m] * dc[c];
      }
    const double I[3][3] = {{pr[0], pr[1], pr[2]}, {pr[1], pr[3], pr[4]}, {pr[2], pr[4], pr[5]}};
    const double* cur = ba_xyz(a, st->cur) + (int64_t)3 * t;
    bool fin = true;
    for (int m = 0; m < 3; ++m) {
      X[m] = cur[m] + -(I[m][0] * s[0] + I[m][1] * s[1] + I[m][2] * s[2]);
      ba_xyz(a, which)[(int64_t)3 * t + m] = X[m];
      fin = fin && ba_finite(X[m]);
    }
    if (!fin) atomicOr(&st->flags, BA_F_NOT_FINITE);
  }
  double cost = 0.0;
  bool front = true;
  for (int o = beg; o < beg + len; ++o) {
    if (a.out.obs_act[o] == 0) continue;
    const int64_t node = a.out.obs_node[o];
    double ru, rv, z;
    ba_observe<false>(cams + (int64_t)BA_CAM * a.obs_image[o], X, (double)a.kpts[2 * node], (double)a.kpts[2 * node + 1], ru, rv, z, nullptr);
    front = front && z > 0.0;
    cost += ba_rho(ru * ru + rv * rv, a.huber);
  }
  a.out.trackcost[t] = cost;
  if (!front) atomicOr(&st->flags, BA_F_BEHIND);
}

// ---------------------------------------------------------------------------------------------- decide
__global__ __launch_bounds__(BA_THREADS) void ba_decide_kernel(BaArgs a, int round) {
  __shared__ double s_part[BA_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  BaState* st = a.out.st;
  double v = 0.0;
  for (int i = t; i < a.T; i += BA_THREADS) v += a.out.pt_act[i] ? a.out.trackcost[i] : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) s_part[wave] = v;
  __syncthreads();
  if (t != 0) return;
  double total = s_part[0];
  for (int w = 1; w < BA_THREADS / 64; ++w) total += s_part[w];
  if (round < 0) {                                             // the starting cost
    if (st->flags != 0 || !ba_finite(total)) st->status |= BA_BAD_START;
    if (st->status != 0) st->stop = 1;
    st->cost = st->status != 0 ? 0.0 : total;
    st->flags = 0;
    a.out.history[0] = st->cost, a.out.history[1] = st->lambda;
    return;
  }
  int take = 0;
  if (!st->stop) {
    take = st->flags == 0 && ba_finite(total) && (float)total < (float)st->cost ? 1 : 0;
    if (take) {
      st->cost = total, st->cur ^= 1, st->rejects = 0, st->taken += 1;
      st->lambda = fmax(st->lambda / 10.0, 1e-12);
    } else {
      st->lambda = fmin(10.0 * st->lambda, 1e12);
      if (++st->rejects >= BA_MAX_REJECTS) st->stop = 1;
    }
    st->flags = 0;
  }
  a.out.history[2 * (round + 1)] = st->cost, a.out.history[2 * (round + 1) + 1] = st->lambda;
  a.out.taken[round] = (uint8_t)take;
}

// ---------------------------------------------------------------------------------------------- finish
__global__ __launch_bounds__(BA_THREADS) void ba_finish_kernel(BaArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BA_THREADS + threadIdx.x;
  const BaState* st = a.out.st;
  const int cur = st->cur;
  if (i == 0) {
    int32_t* c = a.out.counters;
    c[BA_N_FREE] = a.n_free - st->n_held, c[BA_N_FIXED] = a.n_fixed, c[BA_N_HELD] = st->n_held, c[BA_N_POINTS] = st->n_points;
    c[BA_N_ACTIVE_OBS] = st->n_act, c[BA_N_BAD_OBS] = st->n_bad, c[BA_ROUNDS_TAKEN] = st->taken, c[BA_STATUS] = st->status;
  }
  if (i < a.n_images && cur == 1 && a.out.slot_of[i] >= 0)
    for (int j = 4; j < 16; ++j) a.out.cams[i * BA_CAM + j] = a.out.cams1[i * BA_CAM + j];
  if (i >= a.T || a.out.pt_act[i] == 0) return;
  int beg, len;
  if (!ba_range(a, (int)i, beg, len)) return;                  // (never: the point is active)
  double X[3];
  for (int m = 0; m < 3; ++m) X[m] = ba_xyz(a, cur)[i * 3 + m];
  if (cur == 1)
    for (int m = 0; m < 3; ++m) a.out.xyz[i * 3 + m] = X[m];
  if (st->status != 0) return;                                 // nothing was computed: every obs_error stays -1
  const double* cams = ba_cams(a, cur);                        // (buffer 1 when cur == 1: the copy above touches buffer 0 only)
  for (int o = beg; o < beg + len; ++o) {
    if (a.out.obs_act[o] == 0) continue;
    const int64_t node = a.out.obs_node[o];
    double ru, rv, z;
    ba_observe<false>(cams + (int64_t)BA_CAM * a.obs_image[o], X, (double)a.kpts[2 * node], (double)a.kpts[2 * node + 1], ru, rv, z, nullptr);
    const double err = sqrt(ru * ru + rv * rv);
    a.out.obs_error[o] = z > 0.0 && err == err ? (err < (double)FLT_MAX ? (float)err : FLT_MAX) : -1.f;
  }
}

// ================================================================================================ the conjugate-gradient form
// GIMS_AUX_BUNDLE_ADJUST_PCG: the same rounds, but the camera step d of a round comes from preconditioned conjugate
// gradients on the Schur complement S, which is never formed.  Per round: point (as above) -> pcg_setup (a wave per slot: U*, b, the block
// M_s of the preconditioner and its 6 x 6 Cholesky factor) -> pcg_init (one workgroup: x = 0, z = M^-1 r, p = z, rho_0) -> cg_iters times
// { pcg_y (a thread per track: y = V*^-1 sum W^T p) -> pcg_sp (a wave per slot: q = U* p - sum W y) -> pcg_step (one workgroup: the two dot
// products, x, r, z, the stop test, p) } -> pcg_cand (a thread per slot: the candidate camera) -> back -> decide.  The iterations after
// the stop are launched and return at once: cg_done lives in the state block.  The lists of the slots are built once per call, with cost
// linear in n_obs up to the ordering: slots (held, an exclusive scan of cam_obs) -> fill (a thread per observation, an integer cursor per
// slot: any order) -> sort (BA_SORT_SPLIT workgroups per slot, 256 entries at a time: every entry goes to the place its rank gives it: ascending).
constexpr int BA_PCG_MAX_FREE = GIMS_BA_PCG_MAX_FREE_CAMERAS;
constexpr int BA_PCG_MAX_ITERS = GIMS_BA_PCG_MAX_CG_ITERS;
constexpr int BA_SORT_SPLIT = 16;                              // workgroups that share the ordering of one slot's list, 256 entries at a time
constexpr int BA_SLOT_REC = 42;                                // per slot: U* (the upper triangle by rows, 21) | L of M_s = L L^T (the lower triangle by rows, 21)

static size_t ba_pcg_layout(void* base, int64_t T, int64_t n_obs, int64_t n_images, int64_t iters, int64_t n_free, BaOut& w, WsRecord* rec = nullptr) {
  WsLayout L(base, rec);
  w.xyz = L.take<double>((size_t)T * 3);
  w.cams = L.take<double>((size_t)n_images * BA_CAM);
  w.obs_error = L.take<float>((size_t)n_obs);
  w.cam_obs = L.take<int32_t>((size_t)n_images);
  w.history = L.take<double>((size_t)(iters + 1) * 2);
  w.taken = L.take<uint8_t>((size_t)iters);
  w.counters = L.take<int32_t>(BA_COUNTERS);
  w.cg_used = L.take<int32_t>((size_t)iters);
  w.cg_res = L.take<double>((size_t)iters);
  L.scratch_from_here();
  w.st = (BaState*)L.take<double>(32);
  w.slot_of = L.take<int32_t>((size_t)n_images);
  w.slot_cam = L.take<int32_t>((size_t)n_free);
  w.slot_ptr = L.take<int32_t>((size_t)n_free + 1);
  w.held = L.take<int32_t>((size_t)n_free);
  w.cursor = L.take<int32_t>((size_t)n_free);
  w.xyz1 = L.take<double>((size_t)T * 3);
  w.cams1 = L.take<double>((size_t)n_images * BA_CAM);
  w.pt_act = L.take<uint8_t>((size_t)T);
  w.obs_act = L.take<uint8_t>((size_t)n_obs);
  w.obs_track = L.take<int32_t>((size_t)n_obs);
  w.obs_node = L.take<int32_t>((size_t)n_obs);
  w.cam_list = L.take<int32_t>((size_t)n_obs);
  w.list_tmp = L.take<int32_t>((size_t)n_obs);
  w.pt_rec = L.take<double>((size_t)T * BA_PT);
  w.obs_rec = L.take<double>((size_t)n_obs * BA_REC);
  w.trackcost = L.take<double>((size_t)T);
  w.y = L.take<double>((size_t)T * 3);
  w.slot_rec = L.take<double>((size_t)n_free * BA_SLOT_REC);
  w.rhs = L.take<double>((size_t)n_free * 6);                  // x of the iteration, then the step d that back reads
  w.vr = L.take<double>((size_t)n_free * 6);
  w.vz = L.take<double>((size_t)n_free * 6);
  w.vp = L.take<double>((size_t)n_free * 6);
  w.vq = L.take<double>((size_t)n_free * 6);
  w.obs_mslot = w.obs_dup = nullptr, w.S = nullptr;            // (the dense form's)
  return L.bytes();
}

__device__ __forceinline__ double ba_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the sum over a workgroup of BA_THREADS: a butterfly per wave, then the waves in order; every thread gets the same bits
__device__ __forceinline__ double ba_block_sum(double v, double* s_part) {
  v = ba_wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  double total = s_part[0];
  for (int w = 1; w < BA_THREADS / 64; ++w) total += s_part[w];
  __syncthreads();
  return total;
}
__device__ __forceinline__ double ba_dot6(const double* v, const double* w) {
  return ((((v[0] * w[0] + v[1] * w[1]) + v[2] * w[2]) + v[3] * w[3]) + v[4] * w[4]) + v[5] * w[5];
}
// z = M^-1 r from the factor L (the lower triangle by rows): L y = r by columns (j ascending), L^T z = y by rows (j descending)
__device__ __forceinline__ void ba_msolve(const double* Lf, const double* r, double* z) {
  double L[21], b[6], y[6];
#pragma unroll
  for (int j = 0; j < 21; ++j) L[j] = Lf[j];
#pragma unroll
  for (int j = 0; j < 6; ++j) b[j] = r[j];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    y[j] = b[j] / L[j * (j + 1) / 2 + j];
#pragma unroll
    for (int i = j + 1; i < 6; ++i) b[i] -= L[i * (i + 1) / 2 + j] * y[j];
  }
#pragma unroll
  for (int j = 5; j >= 0; --j) {
    z[j] = y[j] / L[j * (j + 1) / 2 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) y[k] -= L[j * (j + 1) / 2 + k] * z[j];
  }
}

// ---------------------------------------------------------------------------------------------- slots, lists (any number of slots)
__global__ __launch_bounds__(BA_THREADS) void ba_pcg_slots_kernel(BaArgs a) {
  __shared__ int s_sum[BA_THREADS], s_held[BA_THREADS];
  const int t = threadIdx.x, per = (a.n_free + BA_THREADS - 1) / BA_THREADS;
  const int lo = t * per < a.n_free ? t * per : a.n_free, hi = lo + per < a.n_free ? lo + per : a.n_free;
  int sum = 0, held = 0;
  for (int s = lo; s < hi; ++s) {
    const int c = a.out.cam_obs[a.out.slot_cam[s]];
    a.out.held[s] = c < 4 ? 1 : 0, a.out.cursor[s] = 0;
    if (c < 4) ++held; else sum += c;
  }
  s_sum[t] = sum, s_held[t] = held;
  __syncthreads();
  if (t == 0) {
    int at = 0, h = 0;
    for (int j = 0; j < BA_THREADS; ++j) {
      const int v = s_sum[j];
      s_sum[j] = at, at += v, h += s_held[j];
    }
    a.out.slot_ptr[a.n_free] = at;                             // <= n_obs: every active observation has one camera
    a.out.st->n_held = h;
  }
  __syncthreads();
  int at = s_sum[t];
  for (int s = lo; s < hi; ++s) {
    a.out.slot_ptr[s] = at;
    if (a.out.held[s] == 0) at += a.out.cam_obs[a.out.slot_cam[s]];
  }
}

__global__ __launch_bounds__(BA_THREADS) void ba_pcg_fill_kernel(BaArgs a) {
  const int o = blockIdx.x * BA_THREADS + threadIdx.x;
  if (o >= a.n_obs || a.out.obs_act[o] == 0) return;
  const int s = ba_moving_slot(a, a.obs_image[o]);             // (in range: the observation is active)
  if (s < 0) return;
  const int first = a.out.slot_ptr[s], cap = a.out.slot_ptr[s + 1] - first;
  const int at = atomicAdd(a.out.cursor + s, 1);               // integers: the order of the race is undone by the sort
  if (at < cap && first >= 0 && first + at < a.n_obs) a.out.list_tmp[first + at] = o;
}

__global__ __launch_bounds__(BA_THREADS) void ba_pcg_sort_kernel(BaArgs a) {
  __shared__ int s_tile[BA_THREADS];
  const int s = blockIdx.x, t = threadIdx.x, first = a.out.slot_ptr[s];
  int cnt = a.out.slot_ptr[s + 1] - first;
  if (first < 0 || cnt < 0 || first + cnt > a.n_obs) cnt = 0;   // (never: ba_pcg_slots_kernel wrote them)
  const int32_t* src = a.out.list_tmp + first;
  for (int base = blockIdx.y * BA_THREADS; base < cnt; base += BA_SORT_SPLIT * BA_THREADS) {      // (the same trip count for every thread)
    const int mine = base + t < cnt ? src[base + t] : 0x7fffffff;
    int rank = 0;
    for (int tb = 0; tb < cnt; tb += BA_THREADS) {
      __syncthreads();
      s_tile[t] = tb + t < cnt ? src[tb + t] : 0x7fffffff;
      __syncthreads();
      const int m = cnt - tb < BA_THREADS ? cnt - tb : BA_THREADS;
      for (int j = 0; j < m; ++j) rank += s_tile[j] < mine ? 1 : 0;
    }
    if (base + t < cnt && rank < cnt) a.out.cam_list[first + rank] = mine;      // the entries differ: the ranks are 0 .. cnt - 1
  }
}

// ---------------------------------------------------------------------------------------------- setup of a round's system
// One wave per slot.  U, g_c as in the camera kernel; then, in the same order (the lane's own ascending sum, a butterfly), B = sum Y_o g_p
// and the 21 sums of Y_o W_o^T over the slot's own observations.  b = -g_c + B goes into r; M = U* - sum Y W^T is factored in registers.
__global__ __launch_bounds__(64) void ba_pcg_setup_kernel(BaArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  BaState* st = a.out.st;
  if (st->stop) return;
  double* srec = a.out.slot_rec + (int64_t)BA_SLOT_REC * s;
  double* rs = a.out.vr + (int64_t)6 * s;
  if (a.out.held[s]) {                                         // a held camera does not move: identity blocks and a zero right-hand side
    if (lane < BA_SLOT_REC) {
      const int k = lane < 21 ? lane : lane - 21;
      const bool diag = lane < 21 ? (k == 0 || k == 6 || k == 11 || k == 15 || k == 18 || k == 20) : (k == 0 || k == 2 || k == 5 || k == 9 || k == 14 || k == 20);
      srec[lane] = diag ? 1.0 : 0.0;
    }
    if (lane < 6) rs[lane] = 0.0;
    return;
  }
  const int first = a.out.slot_ptr[s];
  int cnt = a.out.slot_ptr[s + 1] - first;
  if (first < 0 || cnt < 0 || first + cnt > a.n_obs) cnt = 0;   // (never)
  const int32_t* list = a.out.cam_list + first;
  double acc[27];
#pragma unroll
  for (int j = 0; j < 27; ++j) acc[j] = 0.0;
  for (int idx = lane; idx < cnt; idx += 64) {
    const int o = list[idx];
    if (o < 0 || o >= a.n_obs) continue;                       // (never)
    const double* rec = a.out.obs_rec + (int64_t)BA_REC * o;
    double ju[6], jv[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) ju[j] = rec[j], jv[j] = rec[6 + j];
    const double ru = rec[12], rv = rec[13];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) acc[k++] += ju[i] * ju[j] + jv[i] * jv[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += ju[i] * ru + jv[i] * rv;
  }
#pragma unroll
  for (int j = 0; j < 27; ++j) acc[j] = ba_wave_sum(acc[j]);
  const double lambda = st->lambda;
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      acc[k] += lambda * fmax(acc[k], 1e-6);                   // the diagonal entry (i, i) leads row i of the triangle
      k += 6 - i;
    }
  }
  double am[27];                                               // the 21 sums of Y W^T (upper triangle), then B
#pragma unroll
  for (int j = 0; j < 27; ++j) am[j] = 0.0;
  for (int idx = lane; idx < cnt; idx += 64) {
    const int o = list[idx];
    if (o < 0 || o >= a.n_obs) continue;                       // (never)
    const int p = a.out.obs_track[o];
    if (p < 0 || p >= a.T) continue;                           // (never)
    const double* rec = a.out.obs_rec + (int64_t)BA_REC * o;
    const double* gp = a.out.pt_rec + (int64_t)BA_PT * p + 6;
    double w[18], y[18];
#pragma unroll
    for (int j = 0; j < 18; ++j) w[j] = rec[14 + j], y[j] = rec[32 + j];
    const double g0 = gp[0], g1 = gp[1], g2 = gp[2];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) am[k++] += (y[3 * i] * w[3 * j] + y[3 * i + 1] * w[3 * j + 1]) + y[3 * i + 2] * w[3 * j + 2];
#pragma unroll
    for (int i = 0; i < 6; ++i) am[21 + i] += (y[3 * i] * g0 + y[3 * i + 1] * g1) + y[3 * i + 2] * g2;
  }
#pragma unroll
  for (int j = 0; j < 27; ++j) am[j] = ba_wave_sum(am[j]);
  double m[6][6];                                              // M, the lower triangle; every lane holds the same bits
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) {
        m[j][i] = acc[k] - am[k];
        ++k;
      }
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double d = m[j][j];
    ok = ok && ba_finite(d) && d > 0.0;
    const double l = sqrt(d);
    m[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) m[i][j] = m[i][j] / l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i)
#pragma unroll
      for (int k = j + 1; k <= i; ++k) m[i][k] -= m[i][j] * m[k][j];
  }
  if (lane != 0) return;
#pragma unroll
  for (int j = 0; j < 21; ++j) srec[j] = acc[j];
  {
    int k = 21;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) srec[k++] = m[i][j];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) rs[i] = -acc[21 + i] + am[21 + i];
  if (!ok) atomicOr(&st->flags, BA_F_IRREGULAR);
}

// ---------------------------------------------------------------------------------------------- the iteration
// One workgroup: thread j takes the slots j, j + BA_THREADS, ...  x = 0, z = M^-1 r, p = z, rho_0 = r . z
__global__ __launch_bounds__(BA_THREADS) void ba_pcg_init_kernel(BaArgs a) {
  __shared__ double s_part[BA_THREADS / 64];
  const int t = threadIdx.x;
  BaState* st = a.out.st;
  if (st->stop) return;
  const bool irregular = (st->flags & BA_F_IRREGULAR) != 0;    // a point's V* or a slot's M was not regular: there is nothing to solve
  double part = 0.0;
  for (int s = t; s < a.n_free; s += BA_THREADS) {
    double z[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) a.out.rhs[6 * s + j] = 0.0;
    if (irregular) continue;
    ba_msolve(a.out.slot_rec + (int64_t)BA_SLOT_REC * s + 21, a.out.vr + 6 * s, z);
#pragma unroll
    for (int j = 0; j < 6; ++j) a.out.vz[6 * s + j] = z[j], a.out.vp[6 * s + j] = z[j];
    part += ba_dot6(a.out.vr + 6 * s, z);
  }
  const double rho = ba_block_sum(part, s_part);
  if (t != 0) return;
  const bool good = !irregular && ba_finite(rho) && rho >= 0.0;
  if (!irregular && !good) atomicOr(&st->flags, BA_F_IRREGULAR);
  st->rho = good ? rho : 0.0, st->rho0 = good ? rho : 0.0;
  st->cg_used = 0, st->cg_done = !good || rho == 0.0 ? 1 : 0;
}

// y = V*^-1 sum W_o^T p_slot(o): a thread per track, its observations ascending, c ascending inside an observation
__global__ __launch_bounds__(BA_THREADS) void ba_pcg_y_kernel(BaArgs a) {
  const int t = blockIdx.x * BA_THREADS + threadIdx.x;
  const BaState* st = a.out.st;
  if (t >= a.T || st->stop || st->cg_done || a.out.pt_act[t] == 0) return;
  int beg, len;
  if (!ba_range(a, t, beg, len)) return;                       // (never: the point is active)
  double s[3] = {0.0, 0.0, 0.0};
  for (int o = beg; o < beg + len; ++o) {
    if (a.out.obs_act[o] == 0) continue;
    const int k = ba_moving_slot(a, a.obs_image[o]);
    if (k < 0) continue;
    const double *w = a.out.obs_rec + (int64_t)BA_REC * o + 14, *pc = a.out.vp + 6 * k;
    for (int c = 0; c < 6; ++c)
#pragma unroll
      for (int m = 0; m < 3; ++m) s[m] += w[3 * c + m] * pc[c];
  }
  const double* pr = a.out.pt_rec + (int64_t)BA_PT * t;
  const double I[3][3] = {{pr[0], pr[1], pr[2]}, {pr[1], pr[3], pr[4]}, {pr[2], pr[4], pr[5]}};
#pragma unroll
  for (int m = 0; m < 3; ++m) a.out.y[(int64_t)3 * t + m] = (I[m][0] * s[0] + I[m][1] * s[1]) + I[m][2] * s[2];
}

// q_s = U*_s p_s - sum W_o y_track(o): a wave per slot, the lane's own ascending sum over the list and a butterfly
__global__ __launch_bounds__(64) void ba_pcg_sp_kernel(BaArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const BaState* st = a.out.st;
  if (st->stop || st->cg_done) return;
  const int first = a.out.slot_ptr[s];
  int cnt = a.out.slot_ptr[s + 1] - first;
  if (first < 0 || cnt < 0 || first + cnt > a.n_obs) cnt = 0;   // (never)
  const int32_t* list = a.out.cam_list + first;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int idx = lane; idx < cnt; idx += 64) {
    const int o = list[idx];
    if (o < 0 || o >= a.n_obs) continue;                       // (never)
    const int p = a.out.obs_track[o];
    if (p < 0 || p >= a.T) continue;                           // (never)
    const double *w = a.out.obs_rec + (int64_t)BA_REC * o + 14, *y = a.out.y + (int64_t)3 * p;
    const double y0 = y[0], y1 = y[1], y2 = y[2];
#pragma unroll
    for (int r = 0; r < 6; ++r) acc[r] += (w[3 * r] * y0 + w[3 * r + 1] * y1) + w[3 * r + 2] * y2;
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) acc[r] = ba_wave_sum(acc[r]);
  if (lane >= 6) return;
  const double *U = a.out.slot_rec + (int64_t)BA_SLOT_REC * s, *pc = a.out.vp + 6 * s;
  double up = 0.0, wy = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
    if (r == lane) wy = acc[r];
  for (int c = 0; c < 6; ++c) {
    const int i = lane < c ? lane : c, j = lane < c ? c : lane;
    const double term = U[i * 6 - i * (i - 1) / 2 + (j - i)] * pc[c];
    up = c == 0 ? term : up + term;
  }
  a.out.vq[6 * s + lane] = up - wy;
}

// One workgroup: alpha = rho / (p . q), x += alpha p, r -= alpha q, z = M^-1 r, rho' = r . z, the stop test, p = z + (rho' / rho) p
__global__ __launch_bounds__(BA_THREADS) void ba_pcg_step_kernel(BaArgs a, int last) {
  __shared__ double s_part[BA_THREADS / 64];
  const int t = threadIdx.x;
  BaState* st = a.out.st;
  if (st->stop || st->cg_done) return;
  const double rho = st->rho, rho0 = st->rho0;
  double part = 0.0;
  for (int s = t; s < a.n_free; s += BA_THREADS) part += ba_dot6(a.out.vp + 6 * s, a.out.vq + 6 * s);
  const double pq = ba_block_sum(part, s_part);
  if (!(ba_finite(pq) && pq > 0.0)) {                          // the same for every thread
    if (t == 0) atomicOr(&st->flags, BA_F_IRREGULAR), st->cg_done = 1, st->cg_used += 1;
    return;
  }
  const double alpha = rho / pq;
  part = 0.0;
  for (int s = t; s < a.n_free; s += BA_THREADS) {
    double r[6], z[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      a.out.rhs[6 * s + j] = a.out.rhs[6 * s + j] + alpha * a.out.vp[6 * s + j];
      r[j] = a.out.vr[6 * s + j] - alpha * a.out.vq[6 * s + j];
      a.out.vr[6 * s + j] = r[j];
    }
    ba_msolve(a.out.slot_rec + (int64_t)BA_SLOT_REC * s + 21, r, z);
#pragma unroll
    for (int j = 0; j < 6; ++j) a.out.vz[6 * s + j] = z[j];
    part += ba_dot6(r, z);
  }
  const double rho1 = ba_block_sum(part, s_part);
  const bool good = ba_finite(rho1) && rho1 >= 0.0;
  const bool done = !good || rho1 <= a.cg_tol2 * rho0 || last != 0;
  if (!done) {
    const double beta = rho1 / rho;
    for (int s = t; s < a.n_free; s += BA_THREADS)
#pragma unroll
      for (int j = 0; j < 6; ++j) a.out.vp[6 * s + j] = a.out.vz[6 * s + j] + beta * a.out.vp[6 * s + j];
  }
  if (t != 0) return;
  if (!good) atomicOr(&st->flags, BA_F_IRREGULAR);
  st->rho = rho1, st->cg_used += 1, st->cg_done = done ? 1 : 0;
}

// The candidate camera of every slot that moves, into the buffer that is not current (the last part of the solve kernel), and the
// round's cg_used and cg_res.  An irregular round has d = 0.
__global__ __launch_bounds__(BA_THREADS) void ba_pcg_cand_kernel(BaArgs a, int round) {
  const int s = blockIdx.x * BA_THREADS + threadIdx.x;
  BaState* st = a.out.st;
  if (st->stop) return;
  const bool regular = (st->flags & BA_F_IRREGULAR) == 0;
  if (s == 0) {
    a.out.cg_used[round] = st->cg_used;
    a.out.cg_res[round] = regular && st->rho0 > 0.0 ? sqrt(st->rho / st->rho0) : 0.0;
  }
  if (s >= a.n_free) return;
  if (!regular) {
#pragma unroll
    for (int j = 0; j < 6; ++j) a.out.rhs[6 * s + j] = 0.0;
    return;
  }
  if (a.out.held[s] != 0) return;
  const int cam = a.out.slot_cam[s];
  const double* cur = ba_cams(a, st->cur) + (int64_t)BA_CAM * cam;
  double* cand = ba_cams(a, st->cur ^ 1) + (int64_t)BA_CAM * cam;
  const double* d = a.out.rhs + 6 * s;
  const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], th = sqrt(th2);
  const double ca = th > 1e-8 ? sin(th) / th : 1.0, cb = th > 1e-8 ? (1.0 - cos(th)) / th2 : 0.5;
  const double W[3][3] = {{0.0, -d[2], d[1]}, {d[2], 0.0, -d[0]}, {-d[1], d[0], 0.0}};
  bool fin = true;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double ex[3];
      for (int m = 0; m < 3; ++m) ex[m] = (i == m ? 1.0 : 0.0) + ca * W[i][m] + cb * (W[i][0] * W[0][m] + W[i][1] * W[1][m] + W[i][2] * W[2][m]);
      const double v = ex[0] * cur[4 + j] + ex[1] * cur[7 + j] + ex[2] * cur[10 + j];
      cand[4 + 3 * i + j] = v;
      fin = fin && ba_finite(v);
    }
  for (int i = 0; i < 3; ++i) {
    const double v = cur[13 + i] + d[3 + i];
    cand[13 + i] = v;
    fin = fin && ba_finite(v);
  }
  if (!fin) atomicOr(&st->flags, BA_F_NOT_FINITE);
}

// the launches of the conjugate-gradient form behind init and classify: 8 + iters (6 + 3 cg_iters) in all, 5 + 3 iters when n_free == 0
static int ba_pcg_launches(const BaArgs& a, unsigned g_all, unsigned g_T, hipStream_t st) {
  const unsigned g_obs = (unsigned)(a.n_obs > 0 ? cdiv((int64_t)a.n_obs, BA_THREADS) : 1), g_slots = (unsigned)cdiv((int64_t)(a.n_free > 0 ? a.n_free : 1), BA_THREADS);
  if (a.n_free > 0) {
    ba_pcg_slots_kernel<<<1, BA_THREADS, 0, st>>>(a);
    GIMS_LAUNCH_CHECK();
    ba_pcg_fill_kernel<<<g_obs, BA_THREADS, 0, st>>>(a);
    GIMS_LAUNCH_CHECK();
    ba_pcg_sort_kernel<<<dim3((unsigned)a.n_free, BA_SORT_SPLIT), BA_THREADS, 0, st>>>(a);
    GIMS_LAUNCH_CHECK();
  }
  ba_back_kernel<<<g_T, BA_THREADS, 0, st>>>(a, 1);
  GIMS_LAUNCH_CHECK();
  ba_decide_kernel<<<1, BA_THREADS, 0, st>>>(a, -1);
  GIMS_LAUNCH_CHECK();
  for (int r = 0; r < a.iters; ++r) {
    ba_point_kernel<<<g_T, BA_THREADS, 0, st>>>(a);
    GIMS_LAUNCH_CHECK();
    if (a.n_free > 0) {
      ba_pcg_setup_kernel<<<(unsigned)a.n_free, 64, 0, st>>>(a);
      GIMS_LAUNCH_CHECK();
      ba_pcg_init_kernel<<<1, BA_THREADS, 0, st>>>(a);
      GIMS_LAUNCH_CHECK();
      for (int it = 0; it < a.cg_iters; ++it) {
        ba_pcg_y_kernel<<<g_T, BA_THREADS, 0, st>>>(a);
        GIMS_LAUNCH_CHECK();
        ba_pcg_sp_kernel<<<(unsigned)a.n_free, 64, 0, st>>>(a);
        GIMS_LAUNCH_CHECK();
        ba_pcg_step_kernel<<<1, BA_THREADS, 0, st>>>(a, it + 1 == a.cg_iters ? 1 : 0);
        GIMS_LAUNCH_CHECK();
      }
      ba_pcg_cand_kernel<<<g_slots, BA_THREADS, 0, st>>>(a, r);
      GIMS_LAUNCH_CHECK();
    }
    ba_back_kernel<<<g_T, BA_THREADS, 0, st>>>(a, 0);
    GIMS_LAUNCH_CHECK();
    ba_decide_kernel<<<1, BA_THREADS, 0, st>>>(a, r);
    GIMS_LAUNCH_CHECK();
  }
  ba_finish_kernel<<<g_all, BA_THREADS, 0, st>>>(a);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

// ================================================================================================ the focal form
// GIMS_AUX_BUNDLE_ADJUST_FOCAL: the conjugate-gradient form with one more unknown per focal group, the relative scale ds of
// the focal lengths of the group's images.  The reduced system has the unknowns [6 words per slot | 1 word per group].  Every posed image
// that is a slot or lies in a group has an ascending list of its active observations ("listed images": the slots first, in slot order, so
// that setup reads a slot's list where it always did; then the others in image order).  Per round: point (as above) -> focal_point (a
// thread per track: Fu, Fv, G, G V*^-1 of the observations of moving groups) -> pcg_setup (as above) -> focal_image (a wave per listed
// image: the image's share of A, g_g, sum G V*^-1 G^T, sum G V*^-1 g_p, and C_s) -> focal_group (a workgroup per group: A*, b_g, M_g) ->
// focal_init -> cg_iters times { focal_y -> focal_sp (a wave per listed image: q_s and the image's share of q_g) -> focal_gq (a workgroup
// per group: q_g) -> focal_step } -> pcg_cand (as above) -> focal_cand (the candidate focal lengths and scales) -> focal_back -> decide.
// The order of every sum: per image, lane l takes the entries l, l + 64, ... of the image's list, then the butterfly; per group, thread j
// of 256 takes the group's images j, j + 256, ... in ascending image index, a butterfly per wave, then the four waves in order; a dot
// product is the slot sum of 4.21, then the group sum by the same scheme over the groups, and the two are added in that order.
constexpr int BA_FREC = 8;                                     // per observation of a moving group: Fu, Fv | G [3] | G V*^-1 [3]
constexpr int BA_IPART = 4;                                    // per image: its share of A, g_g, sum G V*^-1 G^T, sum G V*^-1 g_p

struct BaFocal {                                               // what the focal form has next to BaArgs
  int n_groups, n_lists;
  int32_t *group_of, *list_of, *gimg_ptr, *gimg_list, *gheld, *group_obs;
  double *scale, *scale1;                                      // the product of the taken (1 + ds): the two buffers of the state (scale is the output)
  double *obs_frec, *img_part, *img_q, *cvec, *grec, *gx, *gr, *gz, *gp, *gq;
};

static size_t ba_focal_layout(void* base, int64_t T, int64_t n_obs, int64_t n_images, int64_t iters, int64_t n_free, int64_t n_groups, BaOut& w, BaFocal& f,
                              WsRecord* rec = nullptr) {
  WsLayout L(base, rec);
  w.xyz = L.take<double>((size_t)T * 3);
  w.cams = L.take<double>((size_t)n_images * BA_CAM);
  w.obs_error = L.take<float>((size_t)n_obs);
  w.cam_obs = L.take<int32_t>((size_t)n_images);
  w.history = L.take<double>((size_t)(iters + 1) * 2);
  w.taken = L.take<uint8_t>((size_t)iters);
  w.counters = L.take<int32_t>(BA_COUNTERS);
  w.cg_used = L.take<int32_t>((size_t)iters);
  w.cg_res = L.take<double>((size_t)iters);
  f.scale = L.take<double>((size_t)n_groups);
  f.group_obs = L.take<int32_t>((size_t)n_groups);
  L.scratch_from_here();
  w.st = (BaState*)L.take<double>(32);
  w.slot_of = L.take<int32_t>((size_t)n_images);
  w.slot_cam = L.take<int32_t>((size_t)n_images);              // the image of every list: the slots, then the other listed images
  w.slot_ptr = L.take<int32_t>((size_t)n_images + 1);
  w.held = L.take<int32_t>((size_t)n_free);
  w.cursor = L.take<int32_t>((size_t)n_images);
  w.xyz1 = L.take<double>((size_t)T * 3);
  w.cams1 = L.take<double>((size_t)n_images * BA_CAM);
  w.pt_act = L.take<uint8_t>((size_t)T);
  w.obs_act = L.take<uint8_t>((size_t)n_obs);
  w.obs_track = L.take<int32_t>((size_t)n_obs);
  w.obs_node = L.take<int32_t>((size_t)n_obs);
  w.cam_list = L.take<int32_t>((size_t)n_obs);
  w.list_tmp = L.take<int32_t>((size_t)n_obs);
  w.pt_rec = L.take<double>((size_t)T * BA_PT);
  w.obs_rec = L.take<double>((size_t)n_obs * BA_REC);
  w.trackcost = L.take<double>((size_t)T);
  w.y = L.take<double>((size_t)T * 3);
  w.slot_rec = L.take<double>((size_t)n_free * BA_SLOT_REC);
  w.rhs = L.take<double>((size_t)n_free * 6);
  w.vr = L.take<double>((size_t)n_free * 6);
  w.vz = L.take<double>((size_t)n_free * 6);
  w.vp = L.take<double>((size_t)n_free * 6);
  w.vq = L.take<double>((size_t)n_free * 6);
  f.cvec = L.take<double>((size_t)n_free * 6);
  f.group_of = L.take<int32_t>((size_t)n_images);
  f.list_of = L.take<int32_t>((size_t)n_images);
  f.gimg_list = L.take<int32_t>((size_t)n_images);
  f.img_part = L.take<double>((size_t)n_images * BA_IPART);
  f.img_q = L.take<double>((size_t)n_images * 2);
  f.obs_frec = L.take<double>((size_t)n_obs * BA_FREC);
  f.gimg_ptr = L.take<int32_t>((size_t)n_groups + 1);
  f.gheld = L.take<int32_t>((size_t)n_groups);
  f.scale1 = L.take<double>((size_t)n_groups);
  f.grec = L.take<double>((size_t)n_groups * 2);
  f.gx = L.take<double>((size_t)n_groups);
  f.gr = L.take<double>((size_t)n_groups);
  f.gz = L.take<double>((size_t)n_groups);
  f.gp = L.take<double>((size_t)n_groups);
  f.gq = L.take<double>((size_t)n_groups);
  w.obs_mslot = w.obs_dup = nullptr, w.S = nullptr;            // (the dense form's)
  return L.bytes();
}

// the group of an image when that group moves, else -1; k is in range
__device__ __forceinline__ int ba_moving_group(const BaFocal& f, int k) {
  const int g = f.group_of[k];
  return g >= 0 && g < f.n_groups && f.gheld[g] == 0 ? g : -1;
}

// ---------------------------------------------------------------------------------------------- groups, lists
// a thread per group: the active observations of its images (integers: any order), held or not, the scale 1 in both buffers
__global__ __launch_bounds__(BA_THREADS) void ba_focal_groups_kernel(BaArgs a, BaFocal f) {
  const int g = blockIdx.x * BA_THREADS + threadIdx.x;
  if (g >= f.n_groups) return;
  int beg = f.gimg_ptr[g], end = f.gimg_ptr[g + 1], n = 0;
  if (beg < 0 || end < beg || end > a.n_images) end = beg = 0;  // (never: the host built the table)
  for (int j = beg; j < end; ++j) {
    const int k = f.gimg_list[j];
    n += k >= 0 && k < a.n_images ? a.out.cam_obs[k] : 0;
  }
  f.group_obs[g] = n, f.gheld[g] = n < 4 ? 1 : 0;
  f.scale[g] = 1.0, f.scale1[g] = 1.0;
}

// one workgroup: which slots are held, and the exclusive scan of the list sizes of ALL the listed images (a held camera's observations
// still count for its group)
__global__ __launch_bounds__(BA_THREADS) void ba_focal_lists_kernel(BaArgs a, BaFocal f) {
  __shared__ int s_sum[BA_THREADS], s_held[BA_THREADS];
  const int t = threadIdx.x, L = f.n_lists, per = (L + BA_THREADS - 1) / BA_THREADS;
  const int lo = t * per < L ? t * per : L, hi = lo + per < L ? lo + per : L;
  int sum = 0, held = 0;
  for (int li = lo; li < hi; ++li) {
    const int c = a.out.cam_obs[a.out.slot_cam[li]];
    a.out.cursor[li] = 0;
    if (li < a.n_free) a.out.held[li] = c < 4 ? 1 : 0, held += c < 4 ? 1 : 0;
    sum += c;
  }
  s_sum[t] = sum, s_held[t] = held;
  __syncthreads();
  if (t == 0) {
    int at = 0, h = 0;
    for (int j = 0; j < BA_THREADS; ++j) {
      const int v = s_sum[j];
      s_sum[j] = at, at += v, h += s_held[j];
    }
    a.out.slot_ptr[L] = at;                                    // <= n_obs: every active observation has one camera
    a.out.st->n_held = h;
  }
  __syncthreads();
  int at = s_sum[t];
  for (int li = lo; li < hi; ++li) {
    a.out.slot_ptr[li] = at;
    at += a.out.cam_obs[a.out.slot_cam[li]];
  }
}

__global__ __launch_bounds__(BA_THREADS) void ba_focal_fill_kernel(BaArgs a, BaFocal f) {
  const int o = blockIdx.x * BA_THREADS + threadIdx.x;
  if (o >= a.n_obs || a.out.obs_act[o] == 0) return;
  const int li = f.list_of[a.obs_image[o]];                    // (in range: the observation is active)
  if (li < 0 || li >= f.n_lists) return;
  const int first = a.out.slot_ptr[li], cap = a.out.slot_ptr[li + 1] - first;
  const int at = atomicAdd(a.out.cursor + li, 1);              // integers: the order of the race is undone by the sort
  if (at >= 0 && at < cap && first >= 0 && first + at < a.n_obs) a.out.list_tmp[first + at] = o;
}

// ---------------------------------------------------------------------------------------------- the focal words of a round
// A thread per track, behind ba_point_kernel (which left V*^-1 in pt_rec): Fu = fx x / z, Fv = fy y / z with the Huber factor, G = Fu Pu +
// Fv Pv and G V*^-1, for every active observation whose image lies in a moving group.
__global__ __launch_bounds__(BA_THREADS) void ba_focal_point_kernel(BaArgs a, BaFocal f) {
  const int t = blockIdx.x * BA_THREADS + threadIdx.x;
  const BaState* st = a.out.st;
  if (t >= a.T || st->stop || a.out.pt_act[t] == 0) return;
  int beg, len;
  if (!ba_range(a, t, beg, len)) return;                       // (never: the point is active)
  const double* cams = ba_cams(a, st->cur);
  const double* Xp = ba_xyz(a, st->cur) + (int64_t)3 * t;
  const double X[3] = {Xp[0], Xp[1], Xp[2]};
  const double* pr = a.out.pt_rec + (int64_t)BA_PT * t;
  const double I[3][3] = {{pr[0], pr[1], pr[2]}, {pr[1], pr[3], pr[4]}, {pr[2], pr[4], pr[5]}};
  for (int o = beg; o < beg + len; ++o) {
    if (a.out.obs_act[o] == 0) continue;
    const int k = a.obs_image[o];
    if (ba_moving_group(f, k) < 0) continue;
    const int64_t node = a.out.obs_node[o];
    const double* c = cams + (int64_t)BA_CAM * k;
    BaJac J;
    double ru, rv, z;
    ba_observe<true>(c, X, (double)a.kpts[2 * node], (double)a.kpts[2 * node + 1], ru, rv, z, &J);
    const double* R = c + 4;
    const double x = (R[0] * X[0] + R[1] * X[1] + R[2] * X[2]) + c[13], y = (R[3] * X[0] + R[4] * X[1] + R[5] * X[2]) + c[14];
    double Fu = c[0] * x / z, Fv = c[1] * y / z;
    if (a.huber > 0.0) {
      const double e = sqrt(ru * ru + rv * rv);
      if (e > a.huber) {
        const double sw = sqrt(a.huber / e);
        Fu = Fu * sw, Fv = Fv * sw;
#pragma unroll
        for (int j = 0; j < 3; ++j) J.pu[j] = J.pu[j] * sw, J.pv[j] = J.pv[j] * sw;
      }
    }
    double* fr = f.obs_frec + (int64_t)BA_FREC * o;
    const double G[3] = {Fu * J.pu[0] + Fv * J.pv[0], Fu * J.pu[1] + Fv * J.pv[1], Fu * J.pu[2] + Fv * J.pv[2]};
    fr[0] = Fu, fr[1] = Fv;
#pragma unroll
    for (int m = 0; m < 3; ++m) fr[2 + m] = G[m], fr[5 + m] = (G[0] * I[0][m] + G[1] * I[1][m]) + G[2] * I[2][m];
  }
}

// A wave per listed image whose group moves: the image's share of A = sum Fu^2 + Fv^2, g_g = sum Fu ru + Fv rv, sum G V*^-1 G^T and
// sum G V*^-1 g_p, and, when the image is a slot that moves, C_s[c] = sum Ju[c] Fu + Jv[c] Fv: the lane's own ascending sum, a butterfly.
__global__ __launch_bounds__(64) void ba_focal_image_kernel(BaArgs a, BaFocal f) {
  const int li = blockIdx.x, lane = threadIdx.x;
  const BaState* st = a.out.st;
  if (li >= f.n_lists || st->stop) return;
  const int k = a.out.slot_cam[li];
  if (k < 0 || k >= a.n_images || ba_moving_group(f, k) < 0) return;
  const bool slot = li < a.n_free && a.out.held[li] == 0;
  const int first = a.out.slot_ptr[li];
  int cnt = a.out.slot_ptr[li + 1] - first;
  if (first < 0 || cnt < 0 || first + cnt > a.n_obs) cnt = 0;   // (never)
  const int32_t* list = a.out.cam_list + first;
  double acc[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) acc[j] = 0.0;
  for (int idx = lane; idx < cnt; idx += 64) {
    const int o = list[idx];
    if (o < 0 || o >= a.n_obs) continue;                       // (never)
    const int p = a.out.obs_track[o];
    if (p < 0 || p >= a.T) continue;                           // (never)
    const double *rec = a.out.obs_rec + (int64_t)BA_REC * o, *fr = f.obs_frec + (int64_t)BA_FREC * o, *gp = a.out.pt_rec + (int64_t)BA_PT * p + 6;
    const double Fu = fr[0], Fv = fr[1];
    acc[0] += Fu * Fu + Fv * Fv;
    acc[1] += Fu * rec[12] + Fv * rec[13];
    acc[2] += (fr[5] * fr[2] + fr[6] * fr[3]) + fr[7] * fr[4];
    acc[3] += (fr[5] * gp[0] + fr[6] * gp[1]) + fr[7] * gp[2];
    if (slot) {
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[4 + c] += rec[c] * Fu + rec[6 + c] * Fv;
    }
  }
#pragma unroll
  for (int j = 0; j < 10; ++j) acc[j] = ba_wave_sum(acc[j]);
  if (lane != 0) return;
#pragma unroll
  for (int j = 0; j < BA_IPART; ++j) f.img_part[(int64_t)BA_IPART * k + j] = acc[j];
  if (slot) {
#pragma unroll
    for (int c = 0; c < 6; ++c) f.cvec[6 * li + c] = acc[4 + c];
  }
}

// the sum of v[k] over the images k of group g, by the scheme of the cost sum: thread j takes the images j, j + BA_THREADS, ...
__device__ __forceinline__ double ba_group_sum(const BaFocal& f, int g, const double* v, int stride, int n_images, double* s_part) {
  int beg = f.gimg_ptr[g], end = f.gimg_ptr[g + 1];
  if (beg < 0 || end < beg || end > n_images) end = beg = 0;    // (never)
  double part = 0.0;
  for (int j = beg + (int)threadIdx.x; j < end; j += BA_THREADS) {
    const int k = f.gimg_list[j];
    if (k >= 0 && k < n_images) part += v[(int64_t)stride * k];
  }
  return ba_block_sum(part, s_part);
}

// A workgroup per group: A* = A + lambda max(A, 1e-6), b_g = -g_g + sum G V*^-1 g_p into r, M_g = A* - sum G V*^-1 G^T
__global__ __launch_bounds__(BA_THREADS) void ba_focal_group_kernel(BaArgs a, BaFocal f) {
  __shared__ double s_part[BA_THREADS / 64];
  const int g = blockIdx.x;
  BaState* st = a.out.st;
  if (st->stop) return;
  if (f.gheld[g]) {                                            // a held group does not move: an identity entry, a zero right-hand side
    if (threadIdx.x == 0) f.grec[2 * g] = 1.0, f.grec[2 * g + 1] = 1.0, f.gr[g] = 0.0;
    return;
  }
  const double A = ba_group_sum(f, g, f.img_part, BA_IPART, a.n_images, s_part), gg = ba_group_sum(f, g, f.img_part + 1, BA_IPART, a.n_images, s_part);
  const double E = ba_group_sum(f, g, f.img_part + 2, BA_IPART, a.n_images, s_part), B = ba_group_sum(f, g, f.img_part + 3, BA_IPART, a.n_images, s_part);
  if (threadIdx.x != 0) return;
  const double As = A + st->lambda * fmax(A, 1e-6), M = As - E;
  f.grec[2 * g] = As, f.grec[2 * g + 1] = M, f.gr[g] = -gg + B;
  if (!(ba_finite(M) && M > 0.0)) atomicOr(&st->flags, BA_F_IRREGULAR);
}

// ---------------------------------------------------------------------------------------------- the iteration
__global__ __launch_bounds__(BA_THREADS) void ba_focal_init_kernel(BaArgs a, BaFocal f) {
  __shared__ double s_part[BA_THREADS / 64];
  const int t = threadIdx.x;
  BaState* st = a.out.st;
  if (st->stop) return;
  const bool irregular = (st->flags & BA_F_IRREGULAR) != 0;
  double part = 0.0;
  for (int s = t; s < a.n_free; s += BA_THREADS) {
    double z[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) a.out.rhs[6 * s + j] = 0.0;
    if (irregular) continue;
    ba_msolve(a.out.slot_rec + (int64_t)BA_SLOT_REC * s + 21, a.out.vr + 6 * s, z);
#pragma unroll
    for (int j = 0; j < 6; ++j) a.out.vz[6 * s + j] = z[j], a.out.vp[6 * s + j] = z[j];
    part += ba_dot6(a.out.vr + 6 * s, z);
  }
  const double rho_s = ba_block_sum(part, s_part);
  part = 0.0;
  for (int g = t; g < f.n_groups; g += BA_THREADS) {
    f.gx[g] = 0.0;
    if (irregular) continue;
    const double z = f.gr[g] / f.grec[2 * g + 1];
    f.gz[g] = z, f.gp[g] = z;
    part += f.gr[g] * z;
  }
  const double rho = rho_s + ba_block_sum(part, s_part);
  if (t != 0) return;
  const bool good = !irregular && ba_finite(rho) && rho >= 0.0;
  if (!irregular && !good) atomicOr(&st->flags, BA_F_IRREGULAR);
  st->rho = good ? rho : 0.0, st->rho0 = good ? rho : 0.0;
  st->cg_used = 0, st->cg_done = !good || rho == 0.0 ? 1 : 0;
}

// y = V*^-1 sum (W_o^T p_slot(o) + G_o^T p_group(o)): a thread per track, its observations ascending, the camera term before the group term
__global__ __launch_bounds__(BA_THREADS) void ba_focal_y_kernel(BaArgs a, BaFocal f) {
  const int t = blockIdx.x * BA_THREADS + threadIdx.x;
  const BaState* st = a.out.st;
  if (t >= a.T || st->stop || st->cg_done || a.out.pt_act[t] == 0) return;
  int beg, len;
  if (!ba_range(a, t, beg, len)) return;                       // (never: the point is active)
  double s[3] = {0.0, 0.0, 0.0};
  for (int o = beg; o < beg + len; ++o) {
    if (a.out.obs_act[o] == 0) continue;
    const int k = ba_moving_slot(a, a.obs_image[o]), g = ba_moving_group(f, a.obs_image[o]);
    if (k >= 0) {
      const double *w = a.out.obs_rec + (int64_t)BA_REC * o + 14, *pc = a.out.vp + 6 * k;
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int m = 0; m < 3; ++m) s[m] += w[3 * c + m] * pc[c];
    }
    if (g >= 0) {
      const double *G = f.obs_frec + (int64_t)BA_FREC * o + 2, pg = f.gp[g];
#pragma unroll
      for (int m = 0; m < 3; ++m) s[m] += G[m] * pg;
    }
  }
  const double* pr = a.out.pt_rec + (int64_t)BA_PT * t;
  const double I[3][3] = {{pr[0], pr[1], pr[2]}, {pr[1], pr[3], pr[4]}, {pr[2], pr[4], pr[5]}};
#pragma unroll
  for (int m = 0; m < 3; ++m) a.out.y[(int64_t)3 * t + m] = (I[m][0] * s[0] + I[m][1] * s[1]) + I[m][2] * s[2];
}

// A wave per listed image.  A slot: q_s = (U*_s p_s + C_s p_g) - sum W_o y (without the C_s term when its group does not move).  An
// image of a moving group: its share of q_g, C_s^T p_s (0 when it is no moving slot) and sum G_o y.
__global__ __launch_bounds__(64) void ba_focal_sp_kernel(BaArgs a, BaFocal f) {
  const int li = blockIdx.x, lane = threadIdx.x;
  const BaState* st = a.out.st;
  if (li >= f.n_lists || st->stop || st->cg_done) return;
  const int k = a.out.slot_cam[li];
  if (k < 0 || k >= a.n_images) return;                        // (never)
  const int g = ba_moving_group(f, k);
  const bool is_slot = li < a.n_free, moving = is_slot && a.out.held[li] == 0;
  if (!is_slot && g < 0) return;
  const int first = a.out.slot_ptr[li];
  int cnt = a.out.slot_ptr[li + 1] - first;
  if (first < 0 || cnt < 0 || first + cnt > a.n_obs) cnt = 0;   // (never)
  if (!moving && g < 0) cnt = 0;                               // a held slot outside a moving group: q = p
  const int32_t* list = a.out.cam_list + first;
  double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int idx = lane; idx < cnt; idx += 64) {
    const int o = list[idx];
    if (o < 0 || o >= a.n_obs) continue;                       // (never)
    const int p = a.out.obs_track[o];
    if (p < 0 || p >= a.T) continue;                           // (never)
    const double* y = a.out.y + (int64_t)3 * p;
    const double y0 = y[0], y1 = y[1], y2 = y[2];
    if (moving) {
      const double* w = a.out.obs_rec + (int64_t)BA_REC * o + 14;
#pragma unroll
      for (int r = 0; r < 6; ++r) acc[r] += (w[3 * r] * y0 + w[3 * r + 1] * y1) + w[3 * r + 2] * y2;
    }
    if (g >= 0) {
      const double* G = f.obs_frec + (int64_t)BA_FREC * o + 2;
      acc[6] += (G[0] * y0 + G[1] * y1) + G[2] * y2;
    }
  }
#pragma unroll
  for (int r = 0; r < 7; ++r) acc[r] = ba_wave_sum(acc[r]);
  if (lane == 0 && g >= 0) {
    f.img_q[2 * (int64_t)k] = moving ? ba_dot6(f.cvec + 6 * li, a.out.vp + 6 * li) : 0.0;
    f.img_q[2 * (int64_t)k + 1] = acc[6];
  }
  if (lane >= 6 || !is_slot) return;
  const double *U = a.out.slot_rec + (int64_t)BA_SLOT_REC * li, *pc = a.out.vp + 6 * li;
  double up = 0.0, wy = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
    if (r == lane) wy = acc[r];
  for (int c = 0; c < 6; ++c) {
    const int i = lane < c ? lane : c, j = lane < c ? c : lane;
    const double term = U[i * 6 - i * (i - 1) / 2 + (j - i)] * pc[c];
    up = c == 0 ? term : up + term;
  }
  if (moving && g >= 0) up = up + f.cvec[6 * li + lane] * f.gp[g];
  a.out.vq[6 * li + lane] = up - wy;
}

// A workgroup per group: q_g = (A*_g p_g + sum C_s^T p_s) - sum G_o y, the two sums over the group's images
__global__ __launch_bounds__(BA_THREADS) void ba_focal_gq_kernel(BaArgs a, BaFocal f) {
  __shared__ double s_part[BA_THREADS / 64];
  const int g = blockIdx.x;
  const BaState* st = a.out.st;
  if (st->stop || st->cg_done) return;
  if (f.gheld[g]) {
    if (threadIdx.x == 0) f.gq[g] = f.gp[g];
    return;
  }
  const double cs = ba_group_sum(f, g, f.img_q, 2, a.n_images, s_part), gy = ba_group_sum(f, g, f.img_q + 1, 2, a.n_images, s_part);
  if (threadIdx.x == 0) f.gq[g] = (f.grec[2 * g] * f.gp[g] + cs) - gy;
}

__global__ __launch_bounds__(BA_THREADS) void ba_focal_step_kernel(BaArgs a, BaFocal f, int last) {
  __shared__ double s_part[BA_THREADS / 64];
  const int t = threadIdx.x;
  BaState* st = a.out.st;
  if (st->stop || st->cg_done) return;
  const double rho = st->rho, rho0 = st->rho0;
  double part = 0.0;
  for (int s = t; s < a.n_free; s += BA_THREADS) part += ba_dot6(a.out.vp + 6 * s, a.out.vq + 6 * s);
  const double pq_s = ba_block_sum(part, s_part);
  part = 0.0;
  for (int g = t; g < f.n_groups; g += BA_THREADS) part += f.gp[g] * f.gq[g];
  const double pq = pq_s + ba_block_sum(part, s_part);
  if (!(ba_finite(pq) && pq > 0.0)) {                          // the same for every thread
    if (t == 0) atomicOr(&st->flags, BA_F_IRREGULAR), st->cg_done = 1, st->cg_used += 1;
    return;
  }
  const double alpha = rho / pq;
  part = 0.0;
  for (int s = t; s < a.n_free; s += BA_THREADS) {
    double r[6], z[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      a.out.rhs[6 * s + j] = a.out.rhs[6 * s + j] + alpha * a.out.vp[6 * s + j];
      r[j] = a.out.vr[6 * s + j] - alpha * a.out.vq[6 * s + j];
      a.out.vr[6 * s + j] = r[j];
    }
    ba_msolve(a.out.slot_rec + (int64_t)BA_SLOT_REC * s + 21, r, z);
#pragma unroll
    for (int j = 0; j < 6; ++j) a.out.vz[6 * s + j] = z[j];
    part += ba_dot6(r, z);
  }
  const double rho1_s = ba_block_sum(part, s_part);
  part = 0.0;
  for (int g = t; g < f.n_groups; g += BA_THREADS) {
    f.gx[g] = f.gx[g] + alpha * f.gp[g];
    const double r = f.gr[g] - alpha * f.gq[g], z = r / f.grec[2 * g + 1];
    f.gr[g] = r, f.gz[g] = z;
    part += r * z;
  }
  const double rho1 = rho1_s + ba_block_sum(part, s_part);
  const bool good = ba_finite(rho1) && rho1 >= 0.0;
  const bool done = !good || rho1 <= a.cg_tol2 * rho0 || last != 0;
  if (!done) {
    const double beta = rho1 / rho;
    for (int s = t; s < a.n_free; s += BA_THREADS)
#pragma unroll
      for (int j = 0; j < 6; ++j) a.out.vp[6 * s + j] = a.out.vz[6 * s + j] + beta * a.out.vp[6 * s + j];
    for (int g = t; g < f.n_groups; g += BA_THREADS) f.gp[g] = f.gz[g] + beta * f.gp[g];
  }
  if (t != 0) return;
  if (!good) atomicOr(&st->flags, BA_F_IRREGULAR);
  st->rho = rho1, st->cg_used += 1, st->cg_done = done ? 1 : 0;
}

// Behind ba_pcg_cand_kernel: the candidate fx' = fx (1 + ds), fy' = fy (1 + ds) of every image of a moving group and the candidate scale
// of the group, into the buffers that are not current.  1 + ds <= 0 or a focal length that is not finite: the round is not taken.
__global__ __launch_bounds__(BA_THREADS) void ba_focal_cand_kernel(BaArgs a, BaFocal f) {
  const int i = blockIdx.x * BA_THREADS + threadIdx.x;
  BaState* st = a.out.st;
  if (st->stop) return;
  if ((st->flags & BA_F_IRREGULAR) != 0) {                     // an irregular round has ds = 0 and is not taken
    if (i < f.n_groups) f.gx[i] = 0.0;
    return;
  }
  if (i < f.n_groups && f.gheld[i] == 0) (st->cur ? f.scale : f.scale1)[i] = (st->cur ? f.scale1 : f.scale)[i] * (1.0 + f.gx[i]);
  if (i >= a.n_images) return;
  const int g = ba_moving_group(f, i);
  if (g < 0) return;
  const double* cur = ba_cams(a, st->cur) + (int64_t)BA_CAM * i;
  double* cand = ba_cams(a, st->cur ^ 1) + (int64_t)BA_CAM * i;
  const double f1 = 1.0 + f.gx[g], fx = cur[0] * f1, fy = cur[1] * f1;
  cand[0] = fx, cand[1] = fy;
  if (!(f1 > 0.0 && ba_finite(fx) && ba_finite(fy))) atomicOr(&st->flags, BA_F_NOT_FINITE);
}

// ba_back_kernel(initial = 0) with the group term: s = g_p + sum (W_o^T d_slot(o) + G_o^T ds_group(o)), the observations ascending
__global__ __launch_bounds__(BA_THREADS) void ba_focal_back_kernel(BaArgs a, BaFocal f) {
  const int t = blockIdx.x * BA_THREADS + threadIdx.x;
  BaState* st = a.out.st;
  if (t >= a.T || st->stop || a.out.pt_act[t] == 0) return;
  int beg, len;
  if (!ba_range(a, t, beg, len)) return;                       // (never: the point is active)
  const int which = st->cur ^ 1;
  const double* cams = ba_cams(a, which);
  const double* pr = a.out.pt_rec + (int64_t)BA_PT * t;
  double s[3] = {pr[6], pr[7], pr[8]};
  for (int o = beg; o < beg + len; ++o) {
    if (a.out.obs_act[o] == 0) continue;
    const int k = ba_moving_slot(a, a.obs_image[o]), g = ba_moving_group(f, a.obs_image[o]);
    if (k >= 0) {
      const double *w = a.out.obs_rec + (int64_t)BA_REC * o + 14, *dc = a.out.rhs + 6 * k;
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int m = 0; m < 3; ++m) s[m] += w[3 * c + m] * dc[c];
    }
    if (g >= 0) {
      const double *G = f.obs_frec + (int64_t)BA_FREC * o + 2, dg = f.gx[g];
#pragma unroll
      for (int m = 0; m < 3; ++m) s[m] += G[m] * dg;
    }
  }
  const double I[3][3] = {{pr[0], pr[1], pr[2]}, {pr[1], pr[3], pr[4]}, {pr[2], pr[4], pr[5]}};
  const double* cur = ba_xyz(a, st->cur) + (int64_t)3 * t;
  double X[3];
  bool fin = true;
  for (int m = 0; m < 3; ++m) {
    X[m] = cur[m] + -(I[m][0] * s[0] + I[m][1] * s[1] + I[m][2] * s[2]);
    ba_xyz(a, which)[(int64_t)3 * t + m] = X[m];
    fin = fin && ba_finite(X[m]);
  }
  if (!fin) atomicOr(&st->flags, BA_F_NOT_FINITE);
  double cost = 0.0;
  bool front = true;
  for (int o = beg; o < beg + len; ++o) {
    if (a.out.obs_act[o] == 0) continue;
    const int64_t node = a.out.obs_node[o];
    double ru, rv, z;
    ba_observe<false>(cams + (int64_t)BA_CAM * a.obs_image[o], X, (double)a.kpts[2 * node], (double)a.kpts[2 * node + 1], ru, rv, z, nullptr);
    front = front && z > 0.0;
    cost += ba_rho(ru * ru + rv * rv, a.huber);
  }
  a.out.trackcost[t] = cost;
  if (!front) atomicOr(&st->flags, BA_F_BEHIND);
}

// Behind ba_finish_kernel: the refined fx, fy of the images of moving groups and the scales, when the current buffer is the second
__global__ __launch_bounds__(BA_THREADS) void ba_focal_finish_kernel(BaArgs a, BaFocal f) {
  const int i = blockIdx.x * BA_THREADS + threadIdx.x;
  if (a.out.st->cur != 1) return;
  if (i < f.n_groups) f.scale[i] = f.scale1[i];
  if (i < a.n_images && ba_moving_group(f, i) >= 0) a.out.cams[(int64_t)i * BA_CAM] = a.out.cams1[(int64_t)i * BA_CAM], a.out.cams[(int64_t)i * BA_CAM + 1] = a.out.cams1[(int64_t)i * BA_CAM + 1];
}

// the launches of the focal form behind init and classify, for n_groups > 0: 6 + iters (10 + 4 cg_iters) + 2 when there are slots
static int ba_focal_launches(const BaArgs& a, const BaFocal& f, unsigned g_all, unsigned g_T, hipStream_t st) {
  const unsigned g_obs = (unsigned)(a.n_obs > 0 ? cdiv((int64_t)a.n_obs, BA_THREADS) : 1), g_slots = (unsigned)cdiv((int64_t)(a.n_free > 0 ? a.n_free : 1), BA_THREADS);
  const unsigned g_groups = (unsigned)cdiv((int64_t)f.n_groups, BA_THREADS), L = (unsigned)f.n_lists;
  const int64_t most = a.n_images > f.n_groups ? a.n_images : f.n_groups;
  const unsigned g_ig = (unsigned)cdiv(most, BA_THREADS);
  ba_focal_groups_kernel<<<g_groups, BA_THREADS, 0, st>>>(a, f);
  GIMS_LAUNCH_CHECK();
  if (L > 0) {
    ba_focal_lists_kernel<<<1, BA_THREADS, 0, st>>>(a, f);
    GIMS_LAUNCH_CHECK();
    ba_focal_fill_kernel<<<g_obs, BA_THREADS, 0, st>>>(a, f);
    GIMS_LAUNCH_CHECK();
    ba_pcg_sort_kernel<<<dim3(L, BA_SORT_SPLIT), BA_THREADS, 0, st>>>(a);      // (a list per listed image: slot_ptr has n_lists + 1 entries)
    GIMS_LAUNCH_CHECK();
  }
  ba_back_kernel<<<g_T, BA_THREADS, 0, st>>>(a, 1);
  GIMS_LAUNCH_CHECK();
  ba_decide_kernel<<<1, BA_THREADS, 0, st>>>(a, -1);
  GIMS_LAUNCH_CHECK();
  for (int r = 0; r < a.iters; ++r) {
    ba_point_kernel<<<g_T, BA_THREADS, 0, st>>>(a);
    GIMS_LAUNCH_CHECK();
    ba_focal_point_kernel<<<g_T, BA_THREADS, 0, st>>>(a, f);
    GIMS_LAUNCH_CHECK();
    if (a.n_free > 0) {
      ba_pcg_setup_kernel<<<(unsigned)a.n_free, 64, 0, st>>>(a);
      GIMS_LAUNCH_CHECK();
    }
    if (L > 0) {
      ba_focal_image_kernel<<<L, 64, 0, st>>>(a, f);
      GIMS_LAUNCH_CHECK();
    }
    ba_focal_group_kernel<<<(unsigned)f.n_groups, BA_THREADS, 0, st>>>(a, f);
    GIMS_LAUNCH_CHECK();
    ba_focal_init_kernel<<<1, BA_THREADS, 0, st>>>(a, f);
    GIMS_LAUNCH_CHECK();
    for (int it = 0; it < a.cg_iters; ++it) {
      ba_focal_y_kernel<<<g_T, BA_THREADS, 0, st>>>(a, f);
      GIMS_LAUNCH_CHECK();
      if (L > 0) {
        ba_focal_sp_kernel<<<L, 64, 0, st>>>(a, f);
        GIMS_LAUNCH_CHECK();
      }
      ba_focal_gq_kernel<<<(unsigned)f.n_groups, BA_THREADS, 0, st>>>(a, f);
      GIMS_LAUNCH_CHECK();
      ba_focal_step_kernel<<<1, BA_THREADS, 0, st>>>(a, f, it + 1 == a.cg_iters ? 1 : 0);
      GIMS_LAUNCH_CHECK();
    }
    ba_pcg_cand_kernel<<<g_slots, BA_THREADS, 0, st>>>(a, r);
    GIMS_LAUNCH_CHECK();
    ba_focal_cand_kernel<<<g_ig, BA_THREADS, 0, st>>>(a, f);
    GIMS_LAUNCH_CHECK();
    ba_focal_back_kernel<<<g_T, BA_THREADS, 0, st>>>(a, f);
    GIMS_LAUNCH_CHECK();
    ba_decide_kernel<<<1, BA_THREADS, 0, st>>>(a, r);
    GIMS_LAUNCH_CHECK();
  }
  ba_finish_kernel<<<g_all, BA_THREADS, 0, st>>>(a);
  GIMS_LAUNCH_CHECK();
  ba_focal_finish_kernel<<<g_ig, BA_THREADS, 0, st>>>(a, f);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

// the sizes that lay the buffer out and come as op arguments: the op and gims_aux_layout refuse the same values
static int ba_check_sizes(int64_t T, int64_t n_obs, int64_t n_images) {
  GIMS_CHECK_ARG(T >= 0 && T <= (1 << 30), "bundle_adjust: T = %lld is out of range (0 .. 2^30)", (long long)T);
  GIMS_CHECK_ARG(n_obs >= 0 && n_obs <= (1 << 30), "bundle_adjust: n_obs = %lld is out of range (0 .. 2^30)", (long long)n_obs);
  GIMS_CHECK_ARG(n_images >= 0 && n_images <= (1 << 24), "bundle_adjust: n_images = %lld is out of range (0 .. 2^24)", (long long)n_images);
  return GIMS_OK;
}

// gims_aux_layout for the three forms: sizes = {T, n_obs, n_images, iters, n_free}, the focal form adds n_groups.  iters, n_free and n_groups
// have the bounds of ba_aux below (the op counts n_free from mode and n_groups from group, so each is at most n_images there).
static int ba_aux_layout(const int64_t* sizes, int n, WsRecord& rec, const int form) {
  const bool pcg = form != 0, focal = form == 2;
  GIMS_CHECK_ARG(n == (focal ? 6 : 5), "bundle_adjust: the layout takes %d sizes {T, n_obs, n_images, iters, n_free%s}, not %d", focal ? 6 : 5,
                 focal ? ", n_groups" : "", n);
  const int64_t T = sizes[0], n_obs = sizes[1], n_images = sizes[2], iters = sizes[3], n_free = sizes[4], n_groups = focal ? sizes[5] : 0;
  if (const int rc = ba_check_sizes(T, n_obs, n_images)) return rc;
  GIMS_CHECK_ARG(iters >= 0 && iters <= 255, "bundle_adjust: iters = %lld is out of range (0 .. 255)", (long long)iters);
  GIMS_CHECK_ARG(n_free >= 0 && n_free <= (pcg ? BA_PCG_MAX_FREE : BA_MAX_FREE), "bundle_adjust: %lld free cameras, at most %d", (long long)n_free,
                 pcg ? BA_PCG_MAX_FREE : BA_MAX_FREE);
  GIMS_CHECK_ARG(n_groups >= 0 && n_groups <= (1 << 24), "bundle_adjust: n_groups = %lld is out of range (0 .. 2^24)", (long long)n_groups);
  BaOut w;
  BaFocal f;
  rec.bytes = focal ? ba_focal_layout(nullptr, T, n_obs, n_images, iters, n_free, n_groups, w, f, &rec)
              : pcg ? ba_pcg_layout(nullptr, T, n_obs, n_images, iters, n_free, w, &rec)
                    : ba_layout(nullptr, T, n_obs, n_images, iters, n_free, w, &rec);
  return GIMS_OK;
}
int bundle_adjust_aux_layout(const int64_t* sizes, int n, WsRecord& rec) { return ba_aux_layout(sizes, n, rec, 0); }
int bundle_adjust_pcg_aux_layout(const int64_t* sizes, int n, WsRecord& rec) { return ba_aux_layout(sizes, n, rec, 1); }
int bundle_adjust_focal_aux_layout(const int64_t* sizes, int n, WsRecord& rec) { return ba_aux_layout(sizes, n, rec, 2); }

// GIMS_AUX_BUNDLE_ADJUST, GIMS_AUX_BUNDLE_ADJUST_PCG and GIMS_AUX_BUNDLE_ADJUST_FOCAL of gims_run_ops (include/gims_hip.h): every argument
// check precedes the first HIP call.  form: 0 dense, 1 conjugate gradients, 2 conjugate gradients with focal groups.
static int ba_aux(const gims_aux_args& x, hipStream_t st, const int form) {
  const bool pcg = form != 0, focal = form == 2;
  const int64_t T = x.i[0], n_obs = x.i[1], n_images = x.i[2], N = x.i[3], iters = x.i[4];
  const float huber = x.f[0], lambda0 = x.f[1];
  // i[5] is where a later form of this function (a blocked or iterative reduced solve) would be selected: it is read FIRST
  GIMS_CHECK_ARG(x.i[5] == 0, "gims_run_ops: unknown auxiliary function form: bundle_adjust with i[5] = %lld (i[5] is reserved and must be 0)",
                 (long long)x.i[5]);
  if (const int rc = ba_check_sizes(T, n_obs, n_images)) return rc;
  GIMS_CHECK_ARG(N >= 0 && N <= (1 << 30), "bundle_adjust: N = %lld is out of range (0 .. 2^30)", (long long)N);
  GIMS_CHECK_ARG(iters >= 0 && iters <= 255, "bundle_adjust: iters = %lld is out of range (0 .. 255)", (long long)iters);
  GIMS_CHECK_ARG(huber - huber == 0.f && huber >= 0.f, "bundle_adjust: huber = %g must be finite and >= 0", (double)huber);
  GIMS_CHECK_ARG(lambda0 - lambda0 == 0.f && lambda0 > 0.f, "bundle_adjust: lambda0 = %g must be finite and > 0", (double)lambda0);
  GIMS_CHECK_ARG(x.p[5], "bundle_adjust: the output buffer is NULL");
  GIMS_CHECK_ARG(x.p[0], "bundle_adjust: the table is NULL");
  GIMS_CHECK_ARG(((uintptr_t)x.p[5] & 15) == 0, "bundle_adjust: the output buffer must be 16-byte aligned");
  GIMS_CHECK_ARG((((uintptr_t)x.p[0] | (uintptr_t)x.p[2] | (uintptr_t)x.p[3]) & 7) == 0, "bundle_adjust: the table, xyz and cams must be 8-byte aligned");
  GIMS_CHECK_ARG((((uintptr_t)x.p[1] | (uintptr_t)x.p[4]) & 3) == 0, "bundle_adjust: kpts and mode must be 4-byte aligned");
  const int64_t* tab = (const int64_t*)x.p[0];                 // a HOST array, like the op table itself
  GIMS_CHECK_ARG(pcg || (tab[5] == 0 && tab[6] == 0 && tab[7] == 0), "bundle_adjust: the table words 5 .. 7 are reserved and must be 0");
  GIMS_CHECK_ARG(((tab[0] | tab[1] | tab[2]) & 3) == 0, "bundle_adjust: indptr, obs_image and obs_keypoint must be 4-byte aligned");
  GIMS_CHECK_ARG(T == 0 || (tab[0] && tab[1] && tab[2] && tab[3] && tab[4] && x.p[1] && x.p[2]),
                 "bundle_adjust: indptr, obs_image, obs_keypoint, obs_use, point_use, kpts or xyz is NULL while T = %lld", (long long)T);
  GIMS_CHECK_ARG(n_images == 0 || (x.p[3] && x.p[4]), "bundle_adjust: cams or mode is NULL while n_images = %lld", (long long)n_images);
  const int32_t* mode = (const int32_t*)x.p[4];                // a HOST array too: the number of free cameras sizes the reduced system
  std::vector<int32_t> slot_of((size_t)n_images), slot_cam;
  int64_t n_fixed = 0;
  for (int64_t k = 0; k < n_images; ++k) {
    GIMS_CHECK_ARG(mode[k] >= 0 && mode[k] <= 2, "bundle_adjust: image %lld: mode = %d is out of range (0 absent, 1 fixed, 2 free)", (long long)k, mode[k]);
    slot_of[(size_t)k] = mode[k] == 0 ? BA_ABSENT : mode[k] == 1 ? BA_FIXED : (int32_t)slot_cam.size();
    if (mode[k] == 2) slot_cam.push_back((int32_t)k);
    n_fixed += mode[k] == 1;
  }
  const int64_t n_free = (int64_t)slot_cam.size();
  GIMS_CHECK_ARG(pcg || n_free <= BA_MAX_FREE, "bundle_adjust: %lld free cameras, at most GIMS_BA_MAX_FREE_CAMERAS = %d (a larger set needs the blocked reduced solve)",
                 (long long)n_free, BA_MAX_FREE);
  GIMS_CHECK_ARG(!pcg || n_free <= BA_PCG_MAX_FREE, "bundle_adjust: %lld free cameras, at most GIMS_BA_PCG_MAX_FREE_CAMERAS = %d", (long long)n_free, BA_PCG_MAX_FREE);
  double cg_tol = 0.0;
  if (pcg) {                                                   // the words of this form, behind the checks the two forms share
    memcpy(&cg_tol, tab + 6, sizeof(double));
    GIMS_CHECK_ARG(tab[5] >= 1 && tab[5] <= BA_PCG_MAX_ITERS, "bundle_adjust: cg_iters = %lld (table word 5) is out of range (1 .. %d)", (long long)tab[5], BA_PCG_MAX_ITERS);
    GIMS_CHECK_ARG(cg_tol - cg_tol == 0.0 && cg_tol >= 0.0 && cg_tol < 1.0, "bundle_adjust: cg_tol = %g (table word 6) must be finite with 0 <= cg_tol < 1", cg_tol);
    GIMS_CHECK_ARG(focal || tab[7] == 0, "bundle_adjust: the table word 7 is reserved and must be 0");
  }
  // the focal form: table word 7 is the HOST array group[n_images]; the groups and the listed images are counted here, before any HIP call
  int64_t n_groups = 0;
  std::vector<int32_t> group_of, list_of, gimg_ptr, gimg_list;
  if (focal) {
    GIMS_CHECK_ARG(n_images == 0 || tab[7] != 0, "bundle_adjust: group (table word 7) is NULL while n_images = %lld", (long long)n_images);
    GIMS_CHECK_ARG((tab[7] & 3) == 0, "bundle_adjust: group (table word 7) must be 4-byte aligned");
    const int32_t* group = (const int32_t*)tab[7];
    group_of.assign((size_t)n_images, -1), list_of.assign((size_t)n_images, -1);
    for (int64_t k = 0; k < n_images; ++k) {
      if (mode[k] == 0) continue;                              // an absent image's entry is ignored
      GIMS_CHECK_ARG(group[k] >= -1 && group[k] < n_images, "bundle_adjust: image %lld: group = %d is out of range (-1 fixed intrinsics, 0 .. n_images - 1 = %lld)",
                     (long long)k, group[k], (long long)n_images - 1);
      group_of[(size_t)k] = group[k];
      if (group[k] + 1 > n_groups) n_groups = group[k] + 1;
    }
    gimg_ptr.assign((size_t)n_groups + 1, 0);
    for (int64_t k = 0; k < n_images; ++k)
      if (group_of[(size_t)k] >= 0) ++gimg_ptr[(size_t)group_of[(size_t)k] + 1];
    for (int64_t g = 0; g < n_groups; ++g) gimg_ptr[(size_t)g + 1] += gimg_ptr[(size_t)g];
    gimg_list.resize((size_t)gimg_ptr[(size_t)n_groups]);
    std::vector<int32_t> at(gimg_ptr.begin(), gimg_ptr.end() - 1);
    for (int64_t k = 0; k < n_images; ++k)                     // ascending image index inside every group
      if (group_of[(size_t)k] >= 0) gimg_list[(size_t)at[(size_t)group_of[(size_t)k]]++] = (int32_t)k;
    for (int64_t s = 0; s < n_free; ++s) list_of[(size_t)slot_cam[(size_t)s]] = (int32_t)s;
    for (int64_t k = 0; k < n_images; ++k)                     // the listed images: the slots, then the other images of the groups
      if (mode[k] == 1 && group_of[(size_t)k] >= 0) list_of[(size_t)k] = (int32_t)slot_cam.size(), slot_cam.push_back((int32_t)k);
  }

  BaArgs a;
  BaFocal f;
  memset(&f, 0, sizeof(f));
  if (focal)
    ba_focal_layout((void*)x.p[5], T, n_obs, n_images, iters, n_free, n_groups, a.out, f);
  else if (pcg)
    ba_pcg_layout((void*)x.p[5], T, n_obs, n_images, iters, n_free, a.out);
  else
    ba_layout((void*)x.p[5], T, n_obs, n_images, iters, n_free, a.out);
  a.cg_iters = pcg ? (int)tab[5] : 0, a.cg_tol2 = cg_tol * cg_tol;
  a.indptr = (const int32_t*)tab[0], a.obs_image = (const int32_t*)tab[1], a.obs_keypoint = (const int32_t*)tab[2];
  a.obs_use = (const uint8_t*)tab[3], a.point_use = (const uint8_t*)tab[4];
  a.kpts = (const float*)x.p[1], a.xyz_in = (const double*)x.p[2], a.cams_in = (const double*)x.p[3];
  a.T = (int)T, a.n_obs = (int)n_obs, a.n_images = (int)n_images, a.iters = (int)iters, a.n_free = (int)n_free, a.n_fixed = (int)n_fixed;
  a.N = N, a.huber = (double)huber, a.lambda0 = (double)lambda0;
  GIMS_HIP(hipMemsetAsync(a.out.st, 0, 256, st));
  if (iters > 0) GIMS_HIP(hipMemsetAsync(a.out.taken, 0, (size_t)iters, st));
  if (pcg && iters > 0) {
    GIMS_HIP(hipMemsetAsync(a.out.cg_used, 0, sizeof(int32_t) * (size_t)iters, st));
    GIMS_HIP(hipMemsetAsync(a.out.cg_res, 0, sizeof(double) * (size_t)iters, st));
  }
  if (n_obs > 0) {
    GIMS_HIP(hipMemsetD32Async((hipDeviceptr_t)a.out.obs_error, (int)0xBF800000u, (size_t)n_obs, st));      // -1.f
    GIMS_HIP(hipMemsetAsync(a.out.obs_act, 0, (size_t)n_obs, st));
  }
  if (n_images > 0) {
    const int rc = upload_table(slot_of.data(), sizeof(int32_t) * (size_t)n_images, a.out.slot_of, st);
    if (rc != GIMS_OK) return rc;
  }
  if (!slot_cam.empty()) {
    const int rc = upload_table(slot_cam.data(), sizeof(int32_t) * slot_cam.size(), a.out.slot_cam, st);
    if (rc != GIMS_OK) return rc;
  }
  if (focal && n_groups > 0) {
    f.n_groups = (int)n_groups, f.n_lists = (int)slot_cam.size();
    int rc = upload_table(group_of.data(), sizeof(int32_t) * (size_t)n_images, f.group_of, st);
    if (rc == GIMS_OK) rc = upload_table(list_of.data(), sizeof(int32_t) * (size_t)n_images, f.list_of, st);
    if (rc == GIMS_OK) rc = upload_table(gimg_ptr.data(), sizeof(int32_t) * gimg_ptr.size(), f.gimg_ptr, st);
    if (rc == GIMS_OK && !gimg_list.empty()) rc = upload_table(gimg_list.data(), sizeof(int32_t) * gimg_list.size(), f.gimg_list, st);
    if (rc != GIMS_OK) return rc;
  }
  const int64_t most = T > n_images ? T : n_images;
  const unsigned g_all = (unsigned)(most > 0 ? cdiv(most, BA_THREADS) : 1), g_T = (unsigned)(T > 0 ? cdiv(T, BA_THREADS) : 1);
  ba_init_kernel<<<g_all, BA_THREADS, 0, st>>>(a);
  GIMS_LAUNCH_CHECK();
  ba_classify_kernel<<<g_T, BA_THREADS, 0, st>>>(a);
  GIMS_LAUNCH_CHECK();
  if (focal && n_groups > 0) return ba_focal_launches(a, f, g_all, g_T, st);
  if (pcg) return ba_pcg_launches(a, g_all, g_T, st);             // (the focal form without a group is this form)
  ba_slots_kernel<<<1, BA_MAX_FREE, 0, st>>>(a);
  GIMS_LAUNCH_CHECK();
  if (n_free > 0) {
    ba_fill_kernel<<<(unsigned)n_free, BA_THREADS, 0, st>>>(a);
    GIMS_LAUNCH_CHECK();
    ba_prep_kernel<<<g_T, BA_THREADS, 0, st>>>(a);
    GIMS_LAUNCH_CHECK();
  }
  ba_back_kernel<<<g_T, BA_THREADS, 0, st>>>(a, 1);
  GIMS_LAUNCH_CHECK();
  ba_decide_kernel<<<1, BA_THREADS, 0, st>>>(a, -1);
  GIMS_LAUNCH_CHECK();
  for (int r = 0; r < (int)iters; ++r) {
    ba_point_kernel<<<g_T, BA_THREADS, 0, st>>>(a);
    GIMS_LAUNCH_CHECK();
    if (n_free > 0) {
      ba_camera_kernel<<<(unsigned)n_free, 64, 0, st>>>(a);
      GIMS_LAUNCH_CHECK();
      ba_solve_kernel<<<1, BA_SOLVE_THREADS, 0, st>>>(a);
      GIMS_LAUNCH_CHECK();
    }
    ba_back_kernel<<<g_T, BA_THREADS, 0, st>>>(a, 0);
    GIMS_LAUNCH_CHECK();
    ba_decide_kernel<<<1, BA_THREADS, 0, st>>>(a, r);
    GIMS_LAUNCH_CHECK();
  }
  ba_finish_kernel<<<g_all, BA_THREADS, 0, st>>>(a);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

int bundle_adjust_aux(const gims_aux_args& x, hipStream_t st) { return ba_aux(x, st, 0); }
int bundle_adjust_pcg_aux(const gims_aux_args& x, hipStream_t st) { return ba_aux(x, st, 1); }
int bundle_adjust_focal_aux(const gims_aux_args& x, hipStream_t st) { return ba_aux(x, st, 2); }

}  // namespace gims
