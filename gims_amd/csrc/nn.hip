// Classical descriptor baselines on the device: nearest-neighbour distance ratio (NNDR) and mutual nearest neighbours (MNN).
// replaces: calculate_nndr / calculate_mnn (eval_matches.py:13-67).  Semantics: include/gims_hip.h; design and error bound: DESIGN.md 4.11.
//
// A PROBLEM is one direction of one pair: queries X [nx][d] against the data base Y [ny][d] (A against B, and for MNN also B against A: the
// same kernels through one problem table, one launch per stage for every direction of every pair).
//   norms      float64 |row|^2 of every row, float32 copies for the candidate pass, the largest per matrix (integer max on the bits);
//   candidate  exact-f32 MFMA (v_mfma_f32_32x32x2_f32) tiles of Y X^T.  Y is the ROW operand and X the COLUMN operand, so a lane owns one query
//              (accumulator column) and its 16 registers of an MFMA tile are 16 data-base columns of that query: the 4 smallest approximate scores
//              s^(i,j) = |y_j|^2 - 2 x_i.y_j per query stay in the lane's registers across the column tiles, no cross-lane work in the loop, and
//              no tile of the product is ever stored.  Every (column split, wave column half, lane half) ends with its own list of 4: a query has
//              4 * csplit lists, each over a disjoint column subset;
//   refine     one wave per query: exact float64 distances of the candidates that can still be among the two nearest, then the certificate
//              e2 < |x_i|^2 + T - eps_i  (T = the smallest of the lists' largest kept scores).  A query that fails goes on a device-side list;
//   exhaustive the listed queries against all of Y with the same float64 distance routine (bit-identical to what refine would have written);
//   finish     ratio, threshold, mutual test, matches / scores.
// GUIDED MATCHING (GIMS_AUX_GUIDED_MATCH) is the same sequence under a gate: claim and prologue launches in front (fixed
// rows, the per-row words of the model), then gated instances of candidate and refine (the same bodies, a template parameter), an exhaustive
// pass over the admissible columns only and a finish that keeps the fixed rows.  The ungated kernels compile to what they were.
#include "common.h"

#include <math.h>
#include <string.h>

#include <type_traits>
#include <vector>

namespace gims {

constexpr int NN_K = 4;                    // kept per list
constexpr int NN_T = 128;                  // queries / data-base columns per workgroup tile
constexpr int NN_BK = 32, NN_LD = NN_T + 1;
constexpr int NN_MAXT = 8;                 // d <= 64 * NN_MAXT
constexpr int NN_MAX_N = 32768;
constexpr int NN_TARGET_WGS = 512;         // two workgroups per CU: small problems split their columns until the grid is about this large
constexpr int NN_MAX_SPLIT = 8;

struct NnProb {
  const float* x; const float* y; int64_t ldx, ldy;
  int32_t nx, ny, d, csplit;               // lists per query = 4 * csplit
  int32_t tiles_per, item0, forced, reserved;
  const double* xn; const float* ynf; const uint32_t* ymax_bits;
  float* cs; int32_t* ci;                  // [nx][4 * csplit][NN_K] approximate score / column id (-1: empty slot, score +inf)
  int32_t* nn1; int32_t* nn2; float* d1; float* d2;
  int32_t* fb_rows; int32_t* fb_count;
  float* debug;
};

struct NnPairDev {
  const float* a; const float* b; int64_t lda, ldb;
  int32_t n0, n1, d, mutual;
  float threshold; int32_t forced;
  double* an; double* bn; float* anf; float* bnf; uint32_t* amax; uint32_t* bmax;
  const int32_t* nn1; const float* d1; const float* d2; const int32_t* cnn1;
  float* ratio; uint8_t* match; int64_t* matches0; float* scores0; int64_t* matches1; int32_t* info;
  const int32_t* fb_count0; const int32_t* fb_count1;
};

// Guided matching (GIMS_AUX_GUIDED_MATCH, include/gims_hip.h): the same passes with a GATE.  Every row of A and of B has four
// float64 words, written once by gd_prologue_kernel; admissible(i, j) is one expression of the two rows' words, symmetric in them, so the B
// against A direction runs through the same code.  GdProb [k] goes with NnProb [k].
constexpr int GD_W = 4;
constexpr int GD_NO_CLAIM = 0x7f7f7f7f;    // what a memset of 0x7f leaves: above every row index
struct GdProb {
  const double* qw; const double* cw;      // words of the query rows [nx][GD_W] and of the data-base rows [ny][GD_W]
  int32_t* lcnt;                           // [nx][4 * csplit] admissible columns seen per list
  int32_t* nadm;                           // [nx] n_admissible, or null (the B against A direction)
  double t2; int32_t kind, reserved;
};

struct GdPairDev {
  const float* k0; const float* k1; const float* model; const float* ok;
  const int64_t* prior; const uint8_t* pmask; const float* pscore;
  int32_t n0, n1, kind, mutual, forced; float ratio_thr, max_dist;
  double* wa; double* wb; int32_t* claim; uint8_t* fixed; int32_t* cnt;      // cnt (zeroed): {n_fixed, n_bad_prior, n_dup_prior, no_model}
  int32_t* nn1; int32_t* nn2; float* d1; float* d2; const int32_t* cnn1; const int32_t* fb_count0; const int32_t* fb_count1;
  float* ratio; int64_t* matches0; float* scores0; uint8_t* added0; int64_t* matches1; int32_t* info;
};

// admissible(i, j) of the header on the words of the two rows; q and c may be swapped (every product and square is commutative, the sum of
// the fundamental form keeps its order).  A blocked row (fixed, taken, invalid, no model) holds four NaNs: every comparison is false.
//   fundamental  A row {la, lb, lc, g}, B row {u', v', 1, h}: n = (la u' + lb v') + lc 1;   homography  A row {ax, ay, u, v}, B row {bx, by, u', v'}
// Every product and every sum of the gate is rounded on its own: contraction is switched off inside these two, whatever the file's mode.
__device__ __forceinline__ double gd_mul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double gd_add(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ bool gd_admissible(int kind, double t2, const double (&q)[GD_W], const double (&c)[GD_W]) {
  if (kind == GIMS_VERIFY_MODEL_FUNDAMENTAL) {
    const double n = gd_add(gd_add(gd_mul(q[0], c[0]), gd_mul(q[1], c[1])), gd_mul(q[2], c[2]));
    const double n2 = gd_mul(n, n);
    return (int)(q[3] > 0.0) & (int)(c[3] > 0.0) & (int)(n2 <= gd_mul(t2, q[3])) & (int)(n2 <= gd_mul(t2, c[3]));      // & not &&: no branch between the tests
  }
  const double dx = gd_add(q[0], -c[2]), dy = gd_add(q[1], -c[3]), ex = gd_add(c[0], -q[2]), ey = gd_add(c[1], -q[3]);
  return (int)(gd_add(gd_mul(dx, dx), gd_mul(dy, dy)) <= t2) & (int)(gd_add(gd_mul(ex, ex), gd_mul(ey, ey)) <= t2);
}

// The exact squared distance of include/gims_hip.h: lane l sums k = l, l + 64, ... (square rounded, then added), then the xor butterfly
// 32, 16, 8, 4, 2, 1.  Every lane returns the same value (a + b == b + a).  y == nullptr: the squared norm of x.
__device__ __forceinline__ double nn_exact_d2(const float (&xv)[NN_MAXT], const float* __restrict__ y, int d, int lane) {
  double acc = 0.0;
#pragma unroll
  for (int t = 0; t < NN_MAXT; ++t) {
    const int k = lane + 64 * t;
    if (k < d) {
      const double df = (double)xv[t] - (y ? (double)y[k] : 0.0);
      acc = __dadd_rn(acc, __dmul_rn(df, df));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc = __dadd_rn(acc, __shfl_xor(acc, o, 64));
  return acc;
}
__device__ __forceinline__ void nn_load_row(float (&xv)[NN_MAXT], const float* __restrict__ x, int d, int lane) {
#pragma unroll
  for (int t = 0; t < NN_MAXT; ++t) {
    const int k = lane + 64 * t;
    xv[t] = k < d ? x[k] : 0.f;
  }
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float f32_round_up(double v) {       // smallest float >= v (v >= 0)
  float f = (float)v;
  if ((double)f < v) f = __uint_as_float(__float_as_uint(f) + 1u);
  return f;
}

// (S, j) ordered lexicographically: the two nearest so far.  NaN compares false everywhere and is never taken.
struct NnBest { double e1, e2; int i1, i2; };
__device__ __forceinline__ void nn_best_init(NnBest& b) { b.e1 = b.e2 = INFINITY; b.i1 = b.i2 = 0x7fffffff; }
__device__ __forceinline__ void nn_best_update(NnBest& b, double e, int j) {
  if (e < b.e1 || (e == b.e1 && j < b.i1)) { b.e2 = b.e1; b.i2 = b.i1; b.e1 = e; b.i1 = j; }
  else if (e < b.e2 || (e == b.e2 && j < b.i2)) { b.e2 = e; b.i2 = j; }
}
__device__ __forceinline__ void nn_best_write(const NnProb& P, int i, const NnBest& b) {
  P.nn1[i] = b.i1 == 0x7fffffff ? -1 : b.i1;
  P.nn2[i] = b.i2 == 0x7fffffff ? -1 : b.i2;
  P.d1[i] = (float)sqrt(b.e1);
  P.d2[i] = (float)sqrt(b.e2);
}

// ---------------------------------------------------------------------------------------------- norms
__global__ __launch_bounds__(256) void nn_norms_kernel(const NnPairDev* __restrict__ pairs) {
  const NnPairDev& P = pairs[blockIdx.y];
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= P.n0 + P.n1) return;
  const bool isa = r < P.n0;
  const int i = isa ? r : r - P.n0;
  float xv[NN_MAXT];
  nn_load_row(xv, isa ? P.a + (int64_t)i * P.lda : P.b + (int64_t)i * P.ldb, P.d, lane);
  const double n2 = nn_exact_d2(xv, nullptr, P.d, lane);
  if (lane == 0) {
    (isa ? P.an : P.bn)[i] = n2;
    (isa ? P.anf : P.bnf)[i] = (float)n2;
    atomicMax(isa ? P.amax : P.bmax, __float_as_uint(f32_round_up(n2)));      // non-negative floats order like their bit patterns; NaN sorts above all
    if (!isa && P.mutual) P.matches1[i] = -1;
  }
}

// ---------------------------------------------------------------------------------------------- candidate pass
#define NN_INSERT(IX, S, J)                                                                              \
  do {                                                                                                   \
    if ((S) < ls[IX][3]) {                                                                               \
      float s_ = (S); int j_ = (J);                                                                      \
      ls[IX][3] = s_; lj[IX][3] = j_;                                                                    \
      _Pragma("unroll") for (int q_ = 3; q_ > 0; --q_) {                                                 \
        if (ls[IX][q_] < ls[IX][q_ - 1]) {                                                               \
          const float ts_ = ls[IX][q_]; ls[IX][q_] = ls[IX][q_ - 1]; ls[IX][q_ - 1] = ts_;               \
          const int tj_ = lj[IX][q_]; lj[IX][q_] = lj[IX][q_ - 1]; lj[IX][q_ - 1] = tj_;                 \
        }                                                                                                \
      }                                                                                                  \
    }                                                                                                    \
  } while (0)

// GATED: Wc holds the words of the tile's columns next to Yn (two buffers of [GD_W][NN_T]); an inadmissible entry scores +inf BEFORE the
// insertion, so a list holds admissible columns only, and every list counts the admissible entries it saw.
template <bool GATED>
__device__ __forceinline__ void nn_candidate_body(const NnProb* __restrict__ probs, int np, const GdProb* __restrict__ gates, float* __restrict__ Xs,
                                                  float* __restrict__ Ys, float (*__restrict__ Yn)[NN_T], double* __restrict__ Wc) {
  const int bid = blockIdx.x;
  int lo = 0, hi = np;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (probs[mid].item0 <= bid) lo = mid; else hi = mid;
  }
  const NnProb& P = probs[lo];
  const GdProb* G = GATED ? gates + lo : nullptr;
  const int nx = P.nx, ny = P.ny, csplit = P.csplit, nk = P.d / NN_BK;
  const int local = bid - P.item0, rb = local / csplit, sp = local - rb * csplit;
  const int m0 = rb * NN_T;
  const int tiles_total = (ny + NN_T - 1) / NN_T, t0 = sp * P.tiles_per;
  const int ntl = min(tiles_total, t0 + P.tiles_per) - t0;             // >= 1: the host sizes csplit so that no split is empty
  const float* __restrict__ x = P.x;
  const float* __restrict__ y = P.y;
  const float* __restrict__ ynf = P.ynf;
  const int64_t ldx = P.ldx, ldy = P.ldy;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wy = wave >> 1, wx = wave & 1, li = lane & 31, lh = lane >> 5;

  float ls[2][NN_K];
  int lj[2][NN_K];
#pragma unroll
  for (int ix = 0; ix < 2; ++ix)
#pragma unroll
    for (int q = 0; q < NN_K; ++q) { ls[ix][q] = INFINITY; lj[ix][q] = -1; }

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 rx[4], ry[4];
  float rn = INFINITY;
  // the gate: the words of this lane's two queries, the admissible entries seen, and half a column's words on the way to LDS
  double qw[2][GD_W];
  int seen[2] = {0, 0};
  double2 rw = make_double2(0.0, 0.0);
  double gate_t2 = 0.0;
  int gate_kind = 0;
  if constexpr (GATED) {
    gate_t2 = G->t2;
    gate_kind = G->kind;
#pragma unroll
    for (int ix = 0; ix < 2; ++ix) {
      int row = m0 + (t & 64) + ix * 32 + (t & 31);
      row = row < nx ? row : nx - 1;                                       // a row past the end is computed and not written, like its scores
#pragma unroll
      for (int w = 0; w < GD_W; ++w) qw[ix][w] = G->qw[(int64_t)row * GD_W + w];
    }
  }
  const int total = ntl * nk;
  auto load_tile = [&](int step) {
    const int tl = step / nk, kt = step - tl * nk, k = kt * NN_BK, c0 = (t0 + tl) * NN_T;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int f = t + 256 * it, row = f >> 3, kq = f & 7;
      int xr = m0 + row; xr = xr < nx ? xr : nx - 1;
      int yr = c0 + row; yr = yr < ny ? yr : ny - 1;
      rx[it] = *(const float4*)(x + (int64_t)xr * ldx + k + 4 * kq);
      ry[it] = *(const float4*)(y + (int64_t)yr * ldy + k + 4 * kq);
    }
    if (kt == 0 && t < NN_T) rn = c0 + t < ny ? ynf[c0 + t] : INFINITY;      // a column past the end scores +inf and is never kept
    if constexpr (GATED) {
      if (kt == 0) {                                                        // thread t: words 2 (t & 1), 2 (t & 1) + 1 of column t / 2
        const int c = c0 + (t >> 1);
        rw = c < ny ? *(const double2*)(G->cw + (int64_t)c * GD_W + 2 * (t & 1)) : make_double2(NAN, NAN);      // past the end: blocked
      }
    }
  };
  auto store_tile = [&](int step) {
    const int tl = step / nk, kt = step - tl * nk;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int f = t + 256 * it, row = f >> 3, kq = f & 7;
      float* a = Xs + (4 * kq) * NN_LD + row;
      a[0] = rx[it].x; a[NN_LD] = rx[it].y; a[2 * NN_LD] = rx[it].z; a[3 * NN_LD] = rx[it].w;
      float* b = Ys + (4 * kq) * NN_LD + row;
      b[0] = ry[it].x; b[NN_LD] = ry[it].y; b[2 * NN_LD] = ry[it].z; b[3 * NN_LD] = ry[it].w;
    }
    if (kt == 0 && t < NN_T) Yn[tl & 1][t] = rn;
    if constexpr (GATED) {
      if (kt == 0) {
        double* w = Wc + (tl & 1) * (GD_W * NN_T) + (2 * (t & 1)) * NN_T + (t >> 1);
        w[0] = rw.x; w[NN_T] = rw.y;
      }
    }
  };

  load_tile(0);
  store_tile(0);
  __syncthreads();
  int step = 0;
  for (int tl = 0; tl < ntl; ++tl) {
    for (int kt = 0; kt < nk; ++kt, ++step) {
      if (step + 1 < total) load_tile(step + 1);
#pragma unroll
      for (int s = 0; s < NN_BK / 2; ++s) {
        const float* yp = Ys + (2 * s + lh) * NN_LD + wy * 64 + li;
        const float* xp = Xs + (2 * s + lh) * NN_LD + wx * 64 + li;
        const float y0 = yp[0], y1 = yp[32], x0 = xp[0], x1 = xp[32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(y0, x0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(y0, x1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(y1, x0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(y1, x1, acc[1][1], 0, 0, 0);
      }
      __syncthreads();
      if (step + 1 < total) {
        store_tile(step + 1);
        __syncthreads();
      }
    }
    // the tile's 64 x 64 block of this wave: accumulator row = data-base column, accumulator column (the lane) = query.  The model's kind is
    // the same for the whole workgroup: it selects one of two copies of the gated loop, so the 64 gates of a lane hold no branch.
    const int c0 = (t0 + tl) * NN_T;
    const float* yn = Yn[tl & 1];
    auto tile_lists = [&](auto kind_tag) {
      constexpr int KIND = decltype(kind_tag)::value;
#pragma unroll
      for (int iy = 0; iy < 2; ++iy)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int yl = wy * 64 + iy * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const float ynv = yn[yl];
          float s0 = fmaf(-2.f, acc[iy][0][r], ynv), s1 = fmaf(-2.f, acc[iy][1][r], ynv);
          if constexpr (GATED) {
            const double* w = Wc + (tl & 1) * (GD_W * NN_T) + yl;
            const double cw[GD_W] = {w[0], w[NN_T], w[2 * NN_T], w[3 * NN_T]};
            const bool a0 = gd_admissible(KIND, gate_t2, qw[0], cw), a1 = gd_admissible(KIND, gate_t2, qw[1], cw);
            seen[0] += a0; seen[1] += a1;
            asm volatile("" : "+v"(seen[0]), "+v"(seen[1]));                 // count now: 64 comparison masks kept for one sum at the end spill
            s0 = a0 ? s0 : INFINITY;
            s1 = a1 ? s1 : INFINITY;
          }
          NN_INSERT(0, s0, c0 + yl);
          NN_INSERT(1, s1, c0 + yl);
          acc[iy][0][r] = 0.f;
          acc[iy][1][r] = 0.f;
        }
    };
    if (GATED && gate_kind == GIMS_VERIFY_MODEL_FUNDAMENTAL) tile_lists(std::integral_constant<int, GIMS_VERIFY_MODEL_FUNDAMENTAL>{});
    else tile_lists(std::integral_constant<int, GIMS_VERIFY_MODEL_HOMOGRAPHY>{});
  }
  const int nl = 4 * csplit, list = sp * 4 + wy * 2 + lh;
#pragma unroll
  for (int ix = 0; ix < 2; ++ix) {
    const int row = m0 + wx * 64 + ix * 32 + li;
    if (row < nx) {
      const int64_t o = ((int64_t)row * nl + list) * NN_K;
      *(float4*)(P.cs + o) = make_float4(ls[ix][0], ls[ix][1], ls[ix][2], ls[ix][3]);
      *(int4*)(P.ci + o) = make_int4(lj[ix][0], lj[ix][1], lj[ix][2], lj[ix][3]);
      if constexpr (GATED) G->lcnt[(int64_t)row * nl + list] = seen[ix];
    }
  }
}

__global__ __launch_bounds__(256, 2) void nn_candidate_kernel(const NnProb* __restrict__ probs, int np) {
  __shared__ float Xs[NN_BK * NN_LD];
  __shared__ float Ys[NN_BK * NN_LD];
  __shared__ float Yn[2][NN_T];
  nn_candidate_body<false>(probs, np, nullptr, Xs, Ys, Yn, nullptr);
}

__global__ __launch_bounds__(256, 2) void gd_candidate_kernel(const NnProb* __restrict__ probs, int np, const GdProb* __restrict__ gates) {
  __shared__ float Xs[NN_BK * NN_LD];
  __shared__ float Ys[NN_BK * NN_LD];
  __shared__ float Yn[2][NN_T];
  __shared__ double Wc[2 * GD_W * NN_T];
  nn_candidate_body<true>(probs, np, gates, Xs, Ys, Yn, Wc);
}

// ---------------------------------------------------------------------------------------------- refine and certify
// eps_i >= |s^ - s| for every column: u = 2^-24, gamma = d u / (1 - d u), B2 = max_j |y_j|^2 (rounded up),
//   eps_i = 1.01 * (2 u B2 + 2 (gamma + u) sqrt(|x_i|^2 B2)) + 2^-40 (|x_i|^2 + B2)
// the last term covers the float64 roundings of the exact distance and of the certificate itself.  Non-finite norms give NaN: never certified.
__device__ __forceinline__ double nn_eps(double xn, double b2, int d) {
  const double u = 5.9604644775390625e-08, g = d * u / (1.0 - d * u);
  return 1.01 * (2.0 * u * b2 + 2.0 * (g + u) * sqrt(xn * b2)) + 9.094947017729282e-13 * (xn + b2);
}

// GATED: the lists hold admissible columns only, and one rule is added: a row ALL of whose lists are short (last slot +inf, T = +inf) has every
// admissible column listed and is certified without the inequality -- with finite norms only, like the inequality: a column whose
// approximate score is NaN is in no list, and the exhaustive pass may still take it.  n_admissible is the integer sum of the lists' counts.
template <bool GATED>
__device__ __forceinline__ void nn_refine_body(const NnProb* __restrict__ probs, const GdProb* __restrict__ gates) {
  const NnProb& P = probs[blockIdx.y];
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= P.nx) return;
  if constexpr (GATED) {
    const GdProb& G = gates[blockIdx.y];
    const int nl = 4 * P.csplit;
    int seen = 0;
    for (int l = lane; l < nl; l += 64) seen += G.lcnt[(int64_t)i * nl + l];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) seen += __shfl_xor(seen, o, 64);
    if (lane == 0 && G.nadm) G.nadm[i] = seen;
  }
  float xv[NN_MAXT];
  nn_load_row(xv, P.x + (int64_t)i * P.ldx, P.d, lane);
  const double xn = P.xn[i];
  const int nc = 4 * P.csplit * NN_K;
  const float* __restrict__ cs = P.cs + (int64_t)i * nc;
  const int32_t* __restrict__ ci = P.ci + (int64_t)i * nc;
  // the two smallest approximate scores of the row, and T
  float m1 = INFINITY, m2 = INFINITY, T = INFINITY;
  for (int c0 = 0; c0 < nc; c0 += 64) {
    const int c = c0 + lane;
    const float s = c < nc ? cs[c] : INFINITY;
    T = fminf(T, wave_min((c < nc && (c & (NN_K - 1)) == NN_K - 1) ? s : INFINITY));
    const float a = wave_min(s);
    const unsigned long long at = __ballot(s == a);
    const int first = at ? __ffsll((long long)at) - 1 : 0;
    const float b = wave_min(lane == first ? INFINITY : s);
    m2 = fminf(fmaxf(m1, a), fminf(m2, b));
    m1 = fminf(m1, a);
  }
  const double eps = nn_eps(xn, (double)__uint_as_float(*P.ymax_bits), P.d);
  // a candidate whose approximate score exceeds the second smallest by more than 2 eps is strictly farther than two others: not evaluated
  const bool dbg = P.debug != nullptr;
  const double cut = dbg ? (double)INFINITY : (double)m2 + 2.0 * eps;
  NnBest best;
  nn_best_init(best);
  double maxerr = 0.0;
  float s_nn1 = __uint_as_float(0x7fc00000u);
  for (int c0 = 0; c0 < nc; c0 += 64) {
    const int c = c0 + lane;
    const float s = c < nc ? cs[c] : INFINITY;
    const int j = c < nc ? ci[c] : -1;
    unsigned long long mask = __ballot(j >= 0 && (double)s <= cut);
    while (mask) {
      const int src = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int jj = __shfl(j, src, 64);
      const double e = nn_exact_d2(xv, P.y + (int64_t)jj * P.ldy, P.d, lane);
      const int before = best.i1;
      nn_best_update(best, e, jj);
      if (dbg) {
        const float sj = __shfl(s, src, 64);
        maxerr = fmax(maxerr, fabs((double)sj - (e - xn)));
        if (best.i1 != before) s_nn1 = sj;
      }
    }
  }
  const bool certified = best.e2 < xn + (double)T - eps || (GATED && T == INFINITY && eps < (double)INFINITY);
  if (dbg && lane == 0) {
    float* g = P.debug + 4 * (int64_t)i;
    g[0] = f32_round_up(eps); g[1] = f32_round_up(maxerr); g[2] = s_nn1; g[3] = T;
  }
  if (lane == 0) {
    if (certified) nn_best_write(P, i, best);
    else P.fb_rows[atomicAdd(P.fb_count, 1)] = i;         // integer counter: the ORDER of the list varies, what is written per row does not
  }
}

__global__ __launch_bounds__(256) void nn_refine_kernel(const NnProb* __restrict__ probs) { nn_refine_body<false>(probs, nullptr); }
__global__ __launch_bounds__(256) void gd_refine_kernel(const NnProb* __restrict__ probs, const GdProb* __restrict__ gates) {
  nn_refine_body<true>(probs, gates);
}

// ---------------------------------------------------------------------------------------------- exhaustive fallback
__global__ __launch_bounds__(256) void nn_exhaustive_kernel(const NnProb* __restrict__ probs) {
  const NnProb& P = probs[blockIdx.y];
  const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
  const int cnt = P.forced ? P.nx : min(*P.fb_count, P.nx);
  for (int r = w; r < cnt; r += nw) {
    const int i = P.forced ? r : P.fb_rows[r];
    float xv[NN_MAXT];
    nn_load_row(xv, P.x + (int64_t)i * P.ldx, P.d, lane);
    NnBest best;
    nn_best_init(best);
    for (int j = 0; j < P.ny; ++j) nn_best_update(best, nn_exact_d2(xv, P.y + (int64_t)j * P.ldy, P.d, lane), j);
    if (lane == 0) nn_best_write(P, i, best);
  }
}

// the same over the ADMISSIBLE columns only: the lanes gate 64 columns at a time, the wave evaluates the distances of those that passed
__global__ __launch_bounds__(256) void gd_exhaustive_kernel(const NnProb* __restrict__ probs, const GdProb* __restrict__ gates) {
  const NnProb& P = probs[blockIdx.y];
  const GdProb& G = gates[blockIdx.y];
  const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
  const int cnt = P.forced ? P.nx : min(*P.fb_count, P.nx);
  for (int r = w; r < cnt; r += nw) {
    const int i = P.forced ? r : P.fb_rows[r];
    float xv[NN_MAXT];
    nn_load_row(xv, P.x + (int64_t)i * P.ldx, P.d, lane);
    double qw[GD_W];
#pragma unroll
    for (int k = 0; k < GD_W; ++k) qw[k] = G.qw[(int64_t)i * GD_W + k];
    NnBest best;
    nn_best_init(best);
    int seen = 0;
    for (int j0 = 0; j0 < P.ny; j0 += 64) {
      const int j = j0 + lane;
      bool adm = false;
      if (j < P.ny) {
        const double cw[GD_W] = {G.cw[(int64_t)j * GD_W], G.cw[(int64_t)j * GD_W + 1], G.cw[(int64_t)j * GD_W + 2], G.cw[(int64_t)j * GD_W + 3]};
        adm = gd_admissible(G.kind, G.t2, qw, cw);
      }
      unsigned long long mask = __ballot(adm);
      seen += __popcll(mask);
      while (mask) {
        const int jj = j0 + __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        nn_best_update(best, nn_exact_d2(xv, P.y + (int64_t)jj * P.ldy, P.d, lane), jj);
      }
    }
    if (lane == 0) {
      nn_best_write(P, i, best);
      if (G.nadm) G.nadm[i] = seen;
    }
  }
}

// ---------------------------------------------------------------------------------------------- finish
__global__ __launch_bounds__(256) void nn_finish_kernel(const NnPairDev* __restrict__ pairs) {
  const NnPairDev& P = pairs[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    P.info[0] = P.forced ? P.n0 : *P.fb_count0;
    P.info[1] = P.mutual ? (P.forced ? P.n1 : *P.fb_count1) : 0;
    P.info[2] = 0; P.info[3] = 0;
  }
  if (i >= P.n0) return;
  const float ratio = P.d1[i] / P.d2[i];
  const int j = P.nn1[i];
  bool m = ratio < P.threshold;
  if (P.mutual) m = m && j >= 0 && P.cnn1[j] == i;
  P.ratio[i] = ratio;
  P.match[i] = m ? 1 : 0;
  P.matches0[i] = m ? (int64_t)j : (int64_t)-1;
  P.scores0[i] = m ? 1.f - ratio : 0.f;
  if (m && P.mutual) P.matches1[j] = i;            // the mutual test makes j's partner unique
}

// ---------------------------------------------------------------------------------------------- guided matching: claim, prologue, finish
// FIXED rows, step 1: every row whose prior is in the image claims that column; the integer minimum over the claimants keeps the lowest row
__global__ __launch_bounds__(256) void gd_claim_kernel(const GdPairDev* __restrict__ pairs) {
  const GdPairDev& P = pairs[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P.n0 || !P.prior || (P.pmask && P.pmask[i] == 0)) return;
  const int64_t p = P.prior[i];
  if (p >= 0 && p < P.n1) atomicMin(P.claim + p, i);
  else if (p != -1) atomicAdd(P.cnt + 1, 1);
}

__device__ __forceinline__ double gd_lin(double a, double x, double b, double y, double c) {      // (a x + b y) + c
  return gd_add(gd_add(gd_mul(a, x), gd_mul(b, y)), c);
}
__device__ __forceinline__ double gd_cof(double a, double b, double c, double d) { return gd_add(gd_mul(a, b), -gd_mul(c, d)); }      // a b - c d

// step 2 and the per-row words: computed ONCE, read by every later pass.  Row r < n0 is row r of A, the others are rows of B.
__global__ __launch_bounds__(256) void gd_prologue_kernel(const GdPairDev* __restrict__ pairs) {
  const GdPairDev& P = pairs[blockIdx.y];
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= P.n0 + P.n1) return;
  double M[9];
  bool has_model = !P.ok || *P.ok != 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float m = P.model[k];
    has_model = has_model && isfinite(m);
    M[k] = (double)m;
  }
  if (r == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) P.info[k] = 0;            // n_added is counted into info[6] by the finish pass
    P.cnt[3] = has_model ? 0 : 1;
  }
  const bool isa = r < P.n0;
  const int i = isa ? r : r - P.n0;
  bool blocked;
  if (isa) {
    bool fixed = false;
    if (P.prior && !(P.pmask && P.pmask[i] == 0)) {
      const int64_t p = P.prior[i];
      if (p >= 0 && p < P.n1) {
        fixed = P.claim[p] == i;
        atomicAdd(P.cnt + (fixed ? 0 : 2), 1);
      }
    }
    P.fixed[i] = fixed ? 1 : 0;
    blocked = fixed;
  } else {
    blocked = P.claim[i] != GD_NO_CLAIM;                  // TAKEN
  }
  const float* kp = (isa ? P.k0 : P.k1) + 2 * (int64_t)i;
  const double u = (double)kp[0], v = (double)kp[1];
  double w[GD_W];
  if (P.kind == GIMS_VERIFY_MODEL_FUNDAMENTAL) {
    if (isa) {
      w[0] = gd_lin(M[0], u, M[1], v, M[2]); w[1] = gd_lin(M[3], u, M[4], v, M[5]); w[2] = gd_lin(M[6], u, M[7], v, M[8]);
      w[3] = gd_add(gd_mul(w[0], w[0]), gd_mul(w[1], w[1]));
    } else {
      const double ma = gd_lin(M[0], u, M[3], v, M[6]), mb = gd_lin(M[1], u, M[4], v, M[7]);
      w[0] = u; w[1] = v; w[2] = 1.0;
      w[3] = gd_add(gd_mul(ma, ma), gd_mul(mb, mb));
    }
  } else {
    double px, py, pw;
    if (isa) {
      px = gd_lin(M[0], u, M[1], v, M[2]); py = gd_lin(M[3], u, M[4], v, M[5]); pw = gd_lin(M[6], u, M[7], v, M[8]);
    } else {                                              // the cofactors of H, transposed: H^-1 up to the determinant
      px = gd_lin(gd_cof(M[4], M[8], M[5], M[7]), u, gd_cof(M[2], M[7], M[1], M[8]), v, gd_cof(M[1], M[5], M[2], M[4]));
      py = gd_lin(gd_cof(M[5], M[6], M[3], M[8]), u, gd_cof(M[0], M[8], M[2], M[6]), v, gd_cof(M[2], M[3], M[0], M[5]));
      pw = gd_lin(gd_cof(M[3], M[7], M[4], M[6]), u, gd_cof(M[1], M[6], M[0], M[7]), v, gd_cof(M[0], M[4], M[1], M[3]));
    }
    blocked = blocked || !(fabs(pw) > 0.0);
    w[0] = px / pw; w[1] = py / pw; w[2] = u; w[3] = v;
  }
  blocked = blocked || !has_model;
  double* out = (isa ? P.wa : P.wb) + (int64_t)i * GD_W;
#pragma unroll
  for (int k = 0; k < GD_W; ++k) out[k] = blocked ? (double)NAN : w[k];
}

__global__ __launch_bounds__(256) void gd_finish_kernel(const GdPairDev* __restrict__ pairs) {
  const GdPairDev& P = pairs[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    P.info[0] = P.forced ? P.n0 : *P.fb_count0;
    P.info[1] = P.mutual ? (P.forced ? P.n1 : *P.fb_count1) : 0;
    P.info[2] = P.cnt[0]; P.info[3] = P.cnt[1]; P.info[4] = P.cnt[2]; P.info[5] = P.cnt[3];
  }
  bool m = false;
  if (i < P.n0) {
    if (P.fixed[i]) {
      const int64_t p = P.prior[i];
      P.nn1[i] = (int32_t)p; P.nn2[i] = -1;
      P.d1[i] = INFINITY; P.d2[i] = INFINITY; P.ratio[i] = NAN;
      P.matches0[i] = p; P.scores0[i] = P.pscore ? P.pscore[i] : 1.f; P.added0[i] = 0;
      if (P.mutual) P.matches1[p] = i;                    // one fixed row per column, and no searching row reaches a taken column
    } else {
      const float d1 = P.d1[i], ratio = d1 / P.d2[i];
      const int j = P.nn1[i];
      m = ratio < P.ratio_thr && d1 <= P.max_dist;
      if (P.mutual) m = m && j >= 0 && P.cnn1[j] == i;
      P.ratio[i] = ratio;
      P.added0[i] = m ? 1 : 0;
      P.matches0[i] = m ? (int64_t)j : (int64_t)-1;
      P.scores0[i] = m ? 1.f - ratio : 0.f;
      if (m && P.mutual) P.matches1[j] = i;
    }
  }
  const unsigned long long added = __ballot(m);
  if ((threadIdx.x & 63) == 0 && added) atomicAdd(P.info + 6, __popcll(added));
}

// ---------------------------------------------------------------------------------------------- host
// guided: the rules of GIMS_AUX_GUIDED_MATCH, where a row may have one admissible column or none and n1 = 1 (or n0 = 1 with mutual) is served
static const char* nn_rows_why(int64_t n0, int64_t n1, bool mutual, bool guided) {      // the row counts, which are what lays the workspace out
  if (guided && (n0 < 1 || n1 < 1)) return "needs n0 >= 1 and n1 >= 1";
  if (!guided && (n0 < 1 || n1 < 2)) return "needs n0 >= 1 and n1 >= 2 (a second neighbour in B)";
  if (!guided && mutual && n0 < 2) return "the mutual test needs n0 >= 2 (a second neighbour in A)";
  if (n0 > NN_MAX_N || n1 > NN_MAX_N) return "more than 32768 rows";
  return nullptr;
}
static bool nn_pair_ok(const gims_nn_pair& p, int i, bool report, bool guided = false) {
  const char* why = nullptr;
  if (p.d < 32 || p.d > 64 * NN_MAXT || p.d % 32 != 0) why = "d must be a multiple of 32 in [32, 512]";
  else if ((why = nn_rows_why(p.n0, p.n1, p.mutual != 0, guided))) ;
  else if (!p.a || !p.b || !p.nn1 || !p.nn2 || !p.d1 || !p.d2 || !p.ratio || !p.match || !p.matches0 || !p.scores0 || !p.info) why = "null pointer";
  else if (p.mutual && !p.matches1) why = "null matches1 with mutual set";
  else if (p.lda < p.d || p.ldb < p.d || p.lda % 4 != 0 || p.ldb % 4 != 0) why = "row pitch below d or not a multiple of 4";
  else if (((uintptr_t)p.a | (uintptr_t)p.b) & 15) why = "a / b not 16-byte aligned";
  if (why && report) set_error("%s: pair %d (n0 = %d, n1 = %d, d = %d): %s", guided ? "guided_match" : "gims_nn_match", i, p.n0, p.n1, p.d, why);
  return why == nullptr;
}

// The workspace: the two descriptor tables, then the words that must start at zero (four per pair), then per-pair arrays.  probs / pd null
// (with L on a null base): sizing only.
struct NnWs { NnProb* dprobs; NnPairDev* dpairs; uint32_t* zero; size_t zero_bytes; int n_items; };
static NnWs nn_layout(const gims_nn_pair* pairs, int n_pairs, int flags, WsLayout& L, std::vector<NnProb>* probs, std::vector<NnPairDev>* pd) {
  const bool forced = (flags & GIMS_NN_EXHAUSTIVE) != 0;
  int np = 0;
  int64_t rbs = 0;
  for (int i = 0; i < n_pairs; ++i) {
    np += pairs[i].mutual ? 2 : 1;
    rbs += cdiv(pairs[i].n0, NN_T) + (pairs[i].mutual ? cdiv(pairs[i].n1, NN_T) : 0);
  }
  int want = (int)((NN_TARGET_WGS + rbs - 1) / rbs);
  want = want < 1 ? 1 : (want > NN_MAX_SPLIT ? NN_MAX_SPLIT : want);
  NnWs w{};
  w.dprobs = L.take<NnProb>(np);
  w.dpairs = L.take<NnPairDev>(n_pairs);
  w.zero = L.take<uint32_t>(4 * (size_t)n_pairs);
  w.zero_bytes = al256(16 * (size_t)n_pairs);
  for (int i = 0; i < n_pairs; ++i) {
    const gims_nn_pair& p = pairs[i];
    uint32_t* z = w.zero ? w.zero + 4 * (size_t)i : nullptr;                  // {amax bits, bmax bits, fb_count0, fb_count1}
    NnPairDev D;
    memset(&D, 0, sizeof(D));
    D.a = p.a; D.b = p.b; D.lda = p.lda; D.ldb = p.ldb; D.n0 = p.n0; D.n1 = p.n1; D.d = p.d; D.mutual = p.mutual ? 1 : 0;
    D.threshold = p.threshold; D.forced = forced;
    D.an = L.take<double>(p.n0);
    D.bn = L.take<double>(p.n1);
    D.anf = L.take<float>(p.n0);
    D.bnf = L.take<float>(p.n1);
    D.nn1 = p.nn1; D.d1 = p.d1; D.d2 = p.d2;
    D.ratio = p.ratio; D.match = p.match; D.matches0 = p.matches0; D.scores0 = p.scores0; D.matches1 = p.matches1; D.info = p.info;
    if (z) { D.amax = z; D.bmax = z + 1; D.fb_count0 = (const int32_t*)(z + 2); D.fb_count1 = (const int32_t*)(z + 3); }
    for (int dir = 0; dir < (p.mutual ? 2 : 1); ++dir) {
      NnProb Q;
      memset(&Q, 0, sizeof(Q));
      Q.x = dir ? p.b : p.a; Q.y = dir ? p.a : p.b; Q.ldx = dir ? p.ldb : p.lda; Q.ldy = dir ? p.lda : p.ldb;
      Q.nx = dir ? p.n1 : p.n0; Q.ny = dir ? p.n0 : p.n1; Q.d = p.d;
      const int tiles_total = cdiv(Q.ny, NN_T);
      int cs = want < tiles_total ? want : tiles_total;
      Q.tiles_per = cdiv(tiles_total, cs);
      Q.csplit = cdiv(tiles_total, Q.tiles_per);                               // no empty split
      Q.item0 = w.n_items; Q.forced = forced;
      w.n_items += cdiv(Q.nx, NN_T) * Q.csplit;
      Q.xn = dir ? D.bn : D.an; Q.ynf = dir ? D.anf : D.bnf; Q.ymax_bits = dir ? D.amax : D.bmax;
      const size_t nc = (size_t)Q.nx * 4 * Q.csplit * NN_K;
      if (!forced) {
        Q.cs = L.take<float>(nc);
        Q.ci = L.take<int32_t>(nc);
      }
      Q.fb_rows = L.take<int32_t>(Q.nx);
      Q.fb_count = z ? (int32_t*)(z + 2 + dir) : nullptr;
      if (dir == 0) {
        Q.nn1 = p.nn1; Q.nn2 = p.nn2; Q.d1 = p.d1; Q.d2 = p.d2; Q.debug = forced ? nullptr : p.debug;
      } else {
        Q.nn1 = p.cnn1 ? p.cnn1 : L.take<int32_t>(Q.nx);
        Q.nn2 = L.take<int32_t>(Q.nx);
        Q.d1 = L.take<float>(Q.nx);
        Q.d2 = L.take<float>(Q.nx);
        D.cnn1 = Q.nn1;
      }
      if (probs) probs->push_back(Q);
    }
    if (pd) pd->push_back(D);
  }
  return w;
}

// The workspace of GIMS_AUX_GUIDED_MATCH: nn_layout's for the same sizes (match = added0), then the regions of the gate.  probs and pd are
// filled as nn_layout fills them, on a null base too.
struct GdWs {
  NnWs nn;
  GdProb* dgates;
  GdPairDev* dgpairs;
  int32_t *cnt, *claim;
  size_t claims;
  std::vector<double*> wa, wb;       // per pair
  std::vector<uint8_t*> fixed;       // per pair
  std::vector<int32_t*> lcnt;        // per problem (null with GIMS_NN_EXHAUSTIVE)
};
static GdWs gd_layout(const gims_nn_pair* pairs, int np, int flags, WsLayout& L, std::vector<NnProb>& probs, std::vector<NnPairDev>& pd) {
  const bool forced = (flags & GIMS_NN_EXHAUSTIVE) != 0;
  GdWs w;
  w.nn = nn_layout(pairs, np, flags, L, &probs, &pd);
  w.dgates = L.take<GdProb>(probs.size());
  w.dgpairs = L.take<GdPairDev>((size_t)np);
  w.cnt = L.take<int32_t>(4 * (size_t)np);
  w.claims = 0;
  for (int i = 0; i < np; ++i) w.claims += (size_t)pairs[i].n1;
  w.claim = L.take<int32_t>(w.claims);
  size_t k = 0;
  for (int i = 0; i < np; ++i) {
    const gims_nn_pair& p = pairs[i];
    w.wa.push_back(L.take<double>((size_t)GD_W * p.n0));
    w.wb.push_back(L.take<double>((size_t)GD_W * p.n1));
    w.fixed.push_back(L.take<uint8_t>((size_t)p.n0));
    for (int dir = 0; dir < (p.mutual ? 2 : 1); ++dir, ++k)
      w.lcnt.push_back(forced ? nullptr : L.take<int32_t>((size_t)probs[k].nx * 4 * probs[k].csplit));
  }
  return w;
}

// GIMS_AUX_GUIDED_MATCH of gims_run_ops (include/gims_hip.h): every argument check precedes the first HIP call.
enum { GD_A, GD_B, GD_LDA, GD_LDB, GD_N0, GD_N1, GD_D, GD_KPTS0, GD_KPTS1, GD_MODEL, GD_KIND, GD_OK, GD_PRIOR, GD_PMASK, GD_PSCORE, GD_MUTUAL,
       GD_NN1, GD_NN2, GD_D1, GD_D2, GD_RATIO, GD_NADM, GD_MATCHES0, GD_SCORES0, GD_ADDED0, GD_CNN1, GD_MATCHES1, GD_INFO, GD_THRESH, GD_RATIO_THR,
       GD_MAX_DIST, GD_RESERVED };
static_assert(GD_RESERVED + 1 == GIMS_GUIDED_TABLE_WORDS, "the table of GIMS_AUX_GUIDED_MATCH");
static_assert(sizeof(GdProb) == 48 && sizeof(GdPairDev) == 232 && sizeof(NnProb) == 160 && sizeof(NnPairDev) == 200,
              "the workspace formula of include/gims_hip.h");
static float gd_float(int64_t word) {
  const uint32_t b = (uint32_t)word;
  float f;
  memcpy(&f, &b, 4);
  return f;
}

// the number of pairs of one call and its flags: the op and gims_aux_layout refuse the same values
static int gd_check_call(int64_t n, int64_t flags) {
  GIMS_CHECK_ARG(n >= 1 && (size_t)n * 2 * sizeof(NnProb) <= ((size_t)1 << 20), "guided_match: %lld pairs in one call (1 .. %zu)", (long long)n,
                 ((size_t)1 << 20) / (2 * sizeof(NnProb)));
  GIMS_CHECK_ARG((flags & ~(int64_t)GIMS_NN_EXHAUSTIVE) == 0, "guided_match: unknown flag bits 0x%llx", (long long)flags);
  return GIMS_OK;
}

// gims_aux_layout for GIMS_AUX_GUIDED_MATCH: sizes = {flags, P, (n0, n1, mutual) x P}, the workspace
int guided_match_aux_layout(const int64_t* sizes, int n, WsRecord& rec) {
  GIMS_CHECK_ARG(n >= 2 && sizes[1] >= 0 && (int64_t)n - 2 == 3 * sizes[1], "guided_match: the layout takes 2 + 3 P sizes {flags, P, (n0, n1, mutual) x P}, not %d", n);
  const int64_t flags = sizes[0], np = sizes[1];
  if (const int rc = gd_check_call(np, flags)) return rc;
  std::vector<gims_nn_pair> pairs((size_t)np);
  for (int64_t i = 0; i < np; ++i) {
    const int64_t n0 = sizes[2 + 3 * i], n1 = sizes[3 + 3 * i], mutual = sizes[4 + 3 * i];
    const char* why = mutual != 0 && mutual != 1 ? "mutual must be 0 or 1" : nn_rows_why(n0, n1, mutual != 0, true);
    GIMS_CHECK_ARG(!why, "guided_match: pair %lld (n0 = %lld, n1 = %lld): %s", (long long)i, (long long)n0, (long long)n1, why);
    gims_nn_pair& p = pairs[(size_t)i];
    memset(&p, 0, sizeof(p));
    p.n0 = (int32_t)n0, p.n1 = (int32_t)n1, p.mutual = (int32_t)mutual;
    p.cnn1 = mutual ? (int32_t*)&p : nullptr;                  // the op refuses a mutual pair without the caller's cnn1: nn_layout takes none (never read here)
  }
  std::vector<NnProb> probs;
  std::vector<NnPairDev> pd;
  WsLayout L(nullptr, &rec);
  gd_layout(pairs.data(), (int)np, (int)flags, L, probs, pd);
  rec.bytes = L.bytes();
  return GIMS_OK;
}

int guided_match_aux(const gims_aux_args& x, hipStream_t st) {
  // i[5] is where a later form of this function would be selected: it is read FIRST (see assemble_rows_aux)
  GIMS_CHECK_ARG(x.i[5] == 0, "gims_run_ops: unknown auxiliary function form: guided_match with i[5] = %lld (i[5] is reserved and must be 0)",
                 (long long)x.i[5]);
  const int64_t n = x.i[0], flags = x.i[1], work_bytes = x.i[2];
  if (const int rc = gd_check_call(n, flags)) return rc;
  GIMS_CHECK_ARG(x.i[3] == 0 && x.i[4] == 0 && !x.p[2] && !x.p[3] && !x.p[4] && !x.p[5] && x.f[0] == 0.f && x.f[1] == 0.f,
                 "guided_match: a reserved word of the call is not 0 (i[3], i[4], p[2] .. p[5], f[0], f[1])");
  GIMS_CHECK_ARG(x.p[0] && x.p[1], "guided_match: the table or the workspace is NULL");
  GIMS_CHECK_ARG(((uintptr_t)x.p[0] & 7) == 0, "guided_match: the table must be 8-byte aligned");
  GIMS_CHECK_ARG(((uintptr_t)x.p[1] & 255) == 0, "guided_match: the workspace must be 256-byte aligned");
  const int64_t* tab = (const int64_t*)x.p[0];                 // HOST memory
  const int np = (int)n;
  std::vector<gims_nn_pair> pairs((size_t)np);
  for (int i = 0; i < np; ++i) {
    const int64_t* e = tab + (int64_t)GIMS_GUIDED_TABLE_WORDS * i;
    GIMS_CHECK_ARG(e[GD_RESERVED] == 0 && (e[GD_THRESH] >> 32) == 0 && (e[GD_RATIO_THR] >> 32) == 0 && (e[GD_MAX_DIST] >> 32) == 0,
                   "guided_match: pair %d: a reserved word of the table is not 0 (word 31, the high halves of words 28 .. 30)", i);
    GIMS_CHECK_ARG(e[GD_N0] >= 0 && e[GD_N0] <= 0x7fffffff && e[GD_N1] >= 0 && e[GD_N1] <= 0x7fffffff && e[GD_D] >= 0 && e[GD_D] <= 0x7fffffff,
                   "guided_match: pair %d: n0 = %lld, n1 = %lld or d = %lld is out of range", i, (long long)e[GD_N0], (long long)e[GD_N1], (long long)e[GD_D]);
    gims_nn_pair& p = pairs[(size_t)i];
    memset(&p, 0, sizeof(p));
    p.a = (const float*)e[GD_A]; p.b = (const float*)e[GD_B]; p.lda = e[GD_LDA]; p.ldb = e[GD_LDB];
    p.n0 = (int32_t)e[GD_N0]; p.n1 = (int32_t)e[GD_N1]; p.d = (int32_t)e[GD_D]; p.mutual = e[GD_MUTUAL] != 0;
    p.threshold = gd_float(e[GD_RATIO_THR]);
    p.nn1 = (int32_t*)e[GD_NN1]; p.nn2 = (int32_t*)e[GD_NN2]; p.d1 = (float*)e[GD_D1]; p.d2 = (float*)e[GD_D2]; p.ratio = (float*)e[GD_RATIO];
    p.match = (uint8_t*)e[GD_ADDED0]; p.matches0 = (int64_t*)e[GD_MATCHES0]; p.scores0 = (float*)e[GD_SCORES0];
    p.cnn1 = p.mutual ? (int32_t*)e[GD_CNN1] : nullptr; p.matches1 = p.mutual ? (int64_t*)e[GD_MATCHES1] : nullptr; p.info = (int32_t*)e[GD_INFO];
    if (!nn_pair_ok(p, i, true, true)) return GIMS_EINVAL;
    GIMS_CHECK_ARG(e[GD_KPTS0] && e[GD_KPTS1] && e[GD_MODEL] && e[GD_NADM] && (!p.mutual || e[GD_CNN1]),
                   "guided_match: pair %d: null pointer (kpts0, kpts1, model, n_admissible, or cnn1 with mutual set)", i);
    GIMS_CHECK_ARG(e[GD_KIND] == GIMS_VERIFY_MODEL_HOMOGRAPHY || e[GD_KIND] == GIMS_VERIFY_MODEL_FUNDAMENTAL,
                   "guided_match: pair %d: unknown kind %lld (homography 0 or fundamental 1)", i, (long long)e[GD_KIND]);
    const float thresh = gd_float(e[GD_THRESH]), maxd = gd_float(e[GD_MAX_DIST]);
    GIMS_CHECK_ARG(thresh > 0.f && thresh <= 3.402823466e38f, "guided_match: pair %d: thresh must be finite and > 0", i);
    GIMS_CHECK_ARG(maxd >= 0.f, "guided_match: pair %d: max_distance must be >= 0 (+inf for none) and not NaN", i);
  }
  std::vector<NnProb> probs;
  std::vector<NnPairDev> pd;
  WsLayout L((void*)x.p[1]);
  const int iflags = (int)flags;
  const GdWs W = gd_layout(pairs.data(), np, iflags, L, probs, pd);
  const NnWs& w = W.nn;
  const bool forced = (flags & GIMS_NN_EXHAUSTIVE) != 0;
  const int nprob = (int)probs.size();
  GdProb* dgates = W.dgates;
  GdPairDev* dgpairs = W.dgpairs;
  int32_t *cnt = W.cnt, *claim = W.claim;
  const size_t claims = W.claims;
  std::vector<GdProb> gates;
  std::vector<GdPairDev> gp;
  int k = 0, max_rows = 0, max_nx = 0, max_n0 = 0;
  for (int i = 0; i < np; ++i) {
    const int64_t* e = tab + (int64_t)GIMS_GUIDED_TABLE_WORDS * i;
    const gims_nn_pair& p = pairs[(size_t)i];
    GdPairDev D;
    memset(&D, 0, sizeof(D));
    D.k0 = (const float*)e[GD_KPTS0]; D.k1 = (const float*)e[GD_KPTS1]; D.model = (const float*)e[GD_MODEL]; D.ok = (const float*)e[GD_OK];
    D.prior = (const int64_t*)e[GD_PRIOR]; D.pmask = (const uint8_t*)e[GD_PMASK]; D.pscore = (const float*)e[GD_PSCORE];
    D.n0 = p.n0; D.n1 = p.n1; D.kind = (int32_t)e[GD_KIND]; D.mutual = p.mutual ? 1 : 0; D.forced = forced;
    D.ratio_thr = p.threshold; D.max_dist = gd_float(e[GD_MAX_DIST]);
    D.wa = W.wa[(size_t)i], D.wb = W.wb[(size_t)i], D.fixed = W.fixed[(size_t)i];
    D.claim = claim; claim += p.n1;
    D.cnt = cnt + 4 * (size_t)i;
    D.nn1 = p.nn1; D.nn2 = p.nn2; D.d1 = p.d1; D.d2 = p.d2; D.cnn1 = pd[(size_t)i].cnn1;
    D.fb_count0 = pd[(size_t)i].fb_count0; D.fb_count1 = pd[(size_t)i].fb_count1;
    D.ratio = p.ratio; D.matches0 = p.matches0; D.scores0 = p.scores0; D.added0 = p.match; D.matches1 = p.matches1; D.info = p.info;
    const double t = (double)gd_float(e[GD_THRESH]);
    for (int dir = 0; dir < (p.mutual ? 2 : 1); ++dir, ++k) {
      GdProb G;
      memset(&G, 0, sizeof(G));
      G.qw = dir ? D.wb : D.wa; G.cw = dir ? D.wa : D.wb;
      G.lcnt = W.lcnt[(size_t)k];
      G.nadm = dir ? nullptr : (int32_t*)e[GD_NADM];
      G.t2 = t * t; G.kind = D.kind;
      gates.push_back(G);
    }
    gp.push_back(D);
    const int r = p.n0 + p.n1, m = p.mutual ? (p.n0 > p.n1 ? p.n0 : p.n1) : p.n0;
    max_rows = r > max_rows ? r : max_rows;
    max_nx = m > max_nx ? m : max_nx;
    max_n0 = p.n0 > max_n0 ? p.n0 : max_n0;
  }
  GIMS_CHECK_ARG(work_bytes >= 0 && (size_t)work_bytes >= L.bytes(), "guided_match: work_bytes = %lld is below the %zu bytes that this call needs",
                 (long long)work_bytes, L.bytes());

  int rc = upload_table(probs.data(), sizeof(NnProb) * (size_t)nprob, w.dprobs, st);
  if (rc != GIMS_OK) return rc;
  rc = upload_table(pd.data(), sizeof(NnPairDev) * (size_t)np, w.dpairs, st);
  if (rc != GIMS_OK) return rc;
  rc = upload_table(gates.data(), sizeof(GdProb) * (size_t)nprob, dgates, st);
  if (rc != GIMS_OK) return rc;
  rc = upload_table(gp.data(), sizeof(GdPairDev) * (size_t)np, dgpairs, st);
  if (rc != GIMS_OK) return rc;
  GIMS_HIP(hipMemsetAsync(w.zero, 0, w.zero_bytes, st));
  GIMS_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * 4 * (size_t)np, st));
  GIMS_HIP(hipMemsetAsync(gp[0].claim, 0x7f, sizeof(int32_t) * claims, st));
  const NnProb* dp = w.dprobs;
  gd_claim_kernel<<<dim3(cdiv(max_n0, 256), np), 256, 0, st>>>(dgpairs);
  gd_prologue_kernel<<<dim3(cdiv(max_rows, 256), np), 256, 0, st>>>(dgpairs);
  nn_norms_kernel<<<dim3(cdiv(max_rows, 4), np), 256, 0, st>>>(w.dpairs);
  if (!forced) {
    gd_candidate_kernel<<<dim3(w.n_items), 256, 0, st>>>(dp, nprob, dgates);
    gd_refine_kernel<<<dim3(cdiv(max_nx, 4), nprob), 256, 0, st>>>(dp, dgates);
  }
  const int gx = forced ? cdiv(max_nx, 4) : (cdiv(max_nx, 4) < 64 ? cdiv(max_nx, 4) : 64);
  gd_exhaustive_kernel<<<dim3(gx, nprob), 256, 0, st>>>(dp, dgates);
  gd_finish_kernel<<<dim3(cdiv(max_n0, 256), np), 256, 0, st>>>(dgpairs);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

}  // namespace gims

extern "C" size_t gims_nn_workspace_bytes(const gims_nn_pair* pairs, int32_t n_pairs, int32_t flags) {
  using namespace gims;
  if (!pairs || n_pairs <= 0 || (flags & ~GIMS_NN_EXHAUSTIVE)) return 0;
  for (int i = 0; i < n_pairs; ++i)
    if (!nn_pair_ok(pairs[i], i, false)) return 0;
  WsLayout L(nullptr);
  nn_layout(pairs, n_pairs, flags, L, nullptr, nullptr);
  return L.bytes();
}

extern "C" int gims_nn_match(const gims_nn_pair* pairs, int32_t n_pairs, int32_t flags, void* work, size_t work_bytes, void* stream) {
  using namespace gims;
  GIMS_CHECK_ARG(pairs && n_pairs > 0, "gims_nn_match: null / empty pair array");
  GIMS_CHECK_ARG((flags & ~GIMS_NN_EXHAUSTIVE) == 0, "gims_nn_match: unknown flag bits 0x%x", flags);
  GIMS_CHECK_ARG((size_t)n_pairs * 2 * sizeof(NnProb) <= ((size_t)1 << 20), "gims_nn_match: %d pairs in one call (the descriptor table is limited to 1 MiB)", n_pairs);
  for (int i = 0; i < n_pairs; ++i)
    if (!nn_pair_ok(pairs[i], i, true)) return GIMS_EINVAL;
  GIMS_CHECK_ARG(work && ((uintptr_t)work & 255) == 0, "gims_nn_match: null or misaligned workspace");
  std::vector<NnProb> probs;
  std::vector<NnPairDev> pd;
  WsLayout L(work);
  const NnWs w = nn_layout(pairs, n_pairs, flags, L, &probs, &pd);
  GIMS_CHECK_ARG(work_bytes >= L.bytes(), "gims_nn_match: workspace too small (%zu bytes given, %zu needed)", work_bytes, L.bytes());
  hipStream_t s = (hipStream_t)stream;
  const int np = (int)probs.size(), n_items = w.n_items;
  NnProb* dprobs = w.dprobs;
  NnPairDev* dpairs = w.dpairs;
  int rc = upload_table(probs.data(), sizeof(NnProb) * (size_t)np, dprobs, s);
  if (rc != GIMS_OK) return rc;
  rc = upload_table(pd.data(), sizeof(NnPairDev) * (size_t)n_pairs, dpairs, s);
  if (rc != GIMS_OK) return rc;
  GIMS_HIP(hipMemsetAsync(w.zero, 0, w.zero_bytes, s));
  int max_rows = 0, max_nx = 0, max_n0 = 0;
  for (int i = 0; i < n_pairs; ++i) {
    const int r = pairs[i].n0 + pairs[i].n1, m = pairs[i].mutual ? (pairs[i].n0 > pairs[i].n1 ? pairs[i].n0 : pairs[i].n1) : pairs[i].n0;
    max_rows = r > max_rows ? r : max_rows;
    max_nx = m > max_nx ? m : max_nx;
    max_n0 = pairs[i].n0 > max_n0 ? pairs[i].n0 : max_n0;
  }
  const bool forced = (flags & GIMS_NN_EXHAUSTIVE) != 0;
  hipLaunchKernelGGL(nn_norms_kernel, dim3(cdiv(max_rows, 4), n_pairs), dim3(256), 0, s, (const NnPairDev*)dpairs);
  if (!forced) {
    hipLaunchKernelGGL(nn_candidate_kernel, dim3(n_items), dim3(256), 0, s, (const NnProb*)dprobs, np);
    hipLaunchKernelGGL(nn_refine_kernel, dim3(cdiv(max_nx, 4), np), dim3(256), 0, s, (const NnProb*)dprobs);
  }
  // the list of uncertified rows is only known on the device: a fixed grid of waves walks it (empty lists cost one load per wave)
  const int gx = forced ? cdiv(max_nx, 4) : (cdiv(max_nx, 4) < 64 ? cdiv(max_nx, 4) : 64);
  hipLaunchKernelGGL(nn_exhaustive_kernel, dim3(gx, np), dim3(256), 0, s, (const NnProb*)dprobs);
  hipLaunchKernelGGL(nn_finish_kernel, dim3(cdiv(max_n0, 256), n_pairs), dim3(256), 0, s, (const NnPairDev*)dpairs);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}
