// Log-domain Sinkhorn optimal transport + mutual-argmax selection (gmatcher.py:41-69, 284-294).
//
// HBM-bound: the reference reads (and re-materialises) the (N+1)x(M+1) matrix twice per iteration.
// Here the iteration is run in the absorbed-potential form
//     P_ij = exp(Z_ij + u_i + v_j)
//     row:  r_i = sum_j P_ij ;  u_i += log mu_i - log r_i        (== log mu - LSE_j(Z + v))
//     col:  c_j = sum_i P_ij ;  v_j += log nu_j - log c_j        (== log nu - LSE_i(Z + u))
// and ONE sweep over Z serves a row update and the following column update: a workgroup owns a slab of
// 8 rows, keeps e_ij = exp(Z_ij + u_i + v_j) in registers, reduces the row sums, then accumulates the
// column sums of the *updated* matrix as e_ij * (mu_i / r_i) straight from registers.  Column sums are
// written as per-workgroup partials and folded by a tiny second kernel (fixed order -> deterministic).
// After the first row normalisation every P_ij <= 1, so no running max is needed; the start potentials
// u0_i = -max_j Z_ij make the first sweep safe as well (the recurrence does not depend on u0).
// The dustbin row / column (all = alpha) are handled analytically; Z stays the inner N x M block.
// Traffic per iteration: N*M*4 bytes of Z + 2 * G*(M+1)*4 bytes of partials (G <= 512 workgroups).
#include "common.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

namespace gims {

constexpr int OT_R = 8;  // rows per slab

struct OtDev {
  const float* z; int64_t ld; int n, m;
  float* u; float* v;            // [n+1], [m+1]
  float* partial;                // [G][m+1]
  float* cbest_val; int* cbest_idx;  // [G][m]
  float* max0; int* idx0;        // [n]
  float* max1; int* idx1;        // [m]
  int64_t* matches0; int64_t* matches1; float* mscores0; float* mscores1;
  float* status;                 // 1 word: 0 ok / 1 numeric guard
  int G;
  float norm, log_mu_bin, log_nu_bin;  // norm = -log(n+m); log(m)+norm; log(n)+norm
  float* hist;                   // gims_sinkhorn_history: potentials after iteration k go to hist + k * (n + m + 2); else null
};

struct OtBwd {                    // one problem of the backward sweep
  const float* z; int64_t ld; int n, m;
  const float* hist; int64_t hstride;     // potentials after iteration k at hist + k * hstride: u [n+1] then v [m+1]; k = 0 .. iters (slot 0 unused)
  float* dz;                               // [(n+1)][(m+1)], holds G on entry, dL/dZc on exit
  float* gu; float* gv; float* gv2;        // [n+1], [m+1], [m+1]
  float* colpart;                          // [ceil((n+1)/8)][m+1] per-slab column partials of the fused sweep
  float* gu_rec; float* gv_rec;            // low-rank sweep: gu_k [iters + 1][n+1], gv_k [iters + 1][m+1] (slot k; gv_rec[iters] = column sums of G)
  float* fp; float* fq;                    // factor matrices P [n+1][2 iters], Q [m+1][2 iters]
  float* tmat;                             // P Q^T, [(n+1)][ldt]
  int64_t ldt; int iters;
  float* dalpha;
  float norm, log_mu_bin, log_nu_bin;
};

// Reduce R (= 8, 4 or 2) per-lane values over the 64 lanes of a wave with a reduce-scatter butterfly:
// log2(R) exchange steps halve the number of live values, the rest fold the single survivor -- R-1 + (6-log2 R)
// cross-lane moves instead of 6*R.  On return lane l holds the total of row
// ((l>>5)&1)*R/2 + ((l>>4)&1)*R/4 + ... ; lanes with the low (6 - log2 R) bits clear are the writers.
template <int R>
__device__ __forceinline__ float wave_reduce_rows(float (&v)[R], int lane, int& row_out) {
  float cur[R];
#pragma unroll
  for (int i = 0; i < R; ++i) cur[i] = v[i];
  int n = R, bit = 32, row = 0;
#pragma unroll
  for (; n > 1; n >>= 1, bit >>= 1) {
    const bool up = lane & bit;
    const int h = n >> 1;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const float send = up ? cur[i] : cur[i + h];
      const float mine = up ? cur[i + h] : cur[i];
      cur[i] = mine + __shfl_xor(send, bit, 64);
    }
    row += up ? h : 0;
  }
  float x = cur[0];
#pragma unroll
  for (; bit > 0; bit >>= 1) x += __shfl_xor(x, bit, 64);
  row_out = row;
  return x;
}

// The same butterfly for (value, index) pairs under "larger value, then smaller index wins": on return lane l holds the winner of row
// ((l>>5)&1)*R/2 + ((l>>4)&1)*R/4 + ...; lanes with the low (6 - log2 R) bits clear are the writers.
template <int R>
__device__ __forceinline__ void wave_argmax_rows(float (&v)[R], int (&ix)[R], int lane, int& row_out, float& v_out, int& i_out) {
  float cv[R];
  int ci[R];
#pragma unroll
  for (int i = 0; i < R; ++i) { cv[i] = v[i]; ci[i] = ix[i]; }
  int n = R, bit = 32, row = 0;
#pragma unroll
  for (; n > 1; n >>= 1, bit >>= 1) {
    const bool up = lane & bit;
    const int h = n >> 1;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const float sv = up ? cv[i] : cv[i + h];
      const int si = up ? ci[i] : ci[i + h];
      const float mv = up ? cv[i + h] : cv[i];
      const int mi = up ? ci[i + h] : ci[i];
      const float ov = __shfl_xor(sv, bit, 64);
      const int oi = __shfl_xor(si, bit, 64);
      const bool take = ov > mv || (ov == mv && oi < mi);
      cv[i] = take ? ov : mv;
      ci[i] = take ? oi : mi;
    }
    row += up ? h : 0;
  }
  float x = cv[0];
  int xi = ci[0];
#pragma unroll
  for (; bit > 0; bit >>= 1) {
    const float ov = __shfl_xor(x, bit, 64);
    const int oi = __shfl_xor(xi, bit, 64);
    if (ov > x || (ov == x && oi < xi)) { x = ov; xi = oi; }
  }
  row_out = row;
  v_out = x;
  i_out = xi;
}

// ---------------------------------------------------------------------------------------------- init
// rescue = 1 (the streamed re-solve of a given-up on-chip solve, see ot_rescue_begin_kernel): only problems whose status word is 3
// are touched, and the status word is left alone
__global__ void ot_init_kernel(const OtDev* __restrict__ probs, float alpha, int zero_init, int rescue) {
  const OtDev p = probs[blockIdx.y];
  if (rescue && p.status[0] != 3.f) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (blockIdx.x == 0) {
    for (int j = threadIdx.x; j <= p.m; j += blockDim.x) p.v[j] = 0.f;
    if (threadIdx.x == 0) { p.u[p.n] = zero_init ? 0.f : -alpha; if (!rescue) p.status[0] = 0.f; }
  }
  if (row >= p.n) return;
  const float* zr = p.z + (int64_t)row * p.ld;
  float mx = alpha;
  for (int j = lane; j < p.m; j += 64) mx = fmaxf(mx, zr[j]);
  mx = wave_max(mx);
  if (lane == 0) p.u[row] = zero_init ? 0.f : -mx;   // iters == 0: the reference returns Z + 0 + 0 - norm
}

// status words only (the 2-D on-chip kernel forms the start potentials itself)
__global__ void ot_status0_kernel(const OtDev* __restrict__ probs, int np) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < np) probs[i].status[0] = 0.f;
}

// ---------------------------------------------------------------------------------------------- fused iteration
template <int CPT, int R>
__global__ __launch_bounds__(1024) void ot_iter_kernel(const OtDev* __restrict__ probs, float alpha, int rescue) {
  __shared__ float red[16][R];
  __shared__ float fac[R];
  const OtDev p = probs[blockIdx.y];
  if ((int)blockIdx.x >= p.G) return;
  if (rescue && p.status[0] != 3.f && p.status[0] != 4.f) return;
  const float guard_code = rescue ? 4.f : 1.f;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nw = blockDim.x >> 6;

  // owned columns: quads q = t + blockDim*s
  float4 vq[CPT], acc[CPT];
#pragma unroll
  for (int s = 0; s < CPT; ++s) {
    const int c0 = 4 * (t + blockDim.x * s);
    vq[s].x = c0 + 0 < p.m ? p.v[c0 + 0] : 0.f;
    vq[s].y = c0 + 1 < p.m ? p.v[c0 + 1] : 0.f;
    vq[s].z = c0 + 2 < p.m ? p.v[c0 + 2] : 0.f;
    vq[s].w = c0 + 3 < p.m ? p.v[c0 + 3] : 0.f;
    acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float vbin = p.v[p.m];
  float accbin = 0.f;

  // ---- dustbin row (all entries alpha), handled once by workgroup 0
  if (blockIdx.x == 0) {
    const float ub = p.u[p.n];
    float4 e[CPT];
    float rs = 0.f;
#pragma unroll
    for (int s = 0; s < CPT; ++s) {
      const int c0 = 4 * (t + blockDim.x * s);
      e[s].x = c0 + 0 < p.m ? __expf(alpha + ub + vq[s].x) : 0.f;
      e[s].y = c0 + 1 < p.m ? __expf(alpha + ub + vq[s].y) : 0.f;
      e[s].z = c0 + 2 < p.m ? __expf(alpha + ub + vq[s].z) : 0.f;
      e[s].w = c0 + 3 < p.m ? __expf(alpha + ub + vq[s].w) : 0.f;
      rs += (e[s].x + e[s].y) + (e[s].z + e[s].w);
    }
    rs = wave_sum(rs);
    if (lane == 0) red[wave][0] = rs;
    __syncthreads();
    if (t == 0) {
      float tot = 0.f;
      for (int w = 0; w < nw; ++w) tot += red[w][0];
      const float corner = __expf(alpha + ub + vbin);
      tot += corner;
      if (!(tot > 0.f) || !(tot < 3.0e38f)) ot_raise_status(p.status, guard_code);
      const float du = p.log_mu_bin - logf(tot);
      p.u[p.n] = ub + du;
      const float f = __expf(du);
      fac[0] = f;
      accbin += corner * f;
    }
    __syncthreads();
    const float f = fac[0];
#pragma unroll
    for (int s = 0; s < CPT; ++s) {
      acc[s].x += e[s].x * f; acc[s].y += e[s].y * f; acc[s].z += e[s].z * f; acc[s].w += e[s].w * f;
    }
    __syncthreads();
  }

  // ---- slabs of R rows.  The Z rows of the NEXT slab are requested before the current slab is reduced, so
  // the HBM stream keeps running through the barrier-separated reduce / rescale phases (one workgroup per CU).
  const int n_slabs = (p.n + R - 1) / R;
  float4 zn[R][CPT];
  float un[R];
  // branch-free loads: rows are clamped, column quads past m are redirected to column 0 and masked by value
  // (scores rows are padded to a multiple of 4 floats, so a quad that starts inside the row ends inside it)
  int cl[CPT];
  bool cm[CPT][4];
#pragma unroll
  for (int s = 0; s < CPT; ++s) {
    const int c0 = 4 * (t + blockDim.x * s);
    cl[s] = c0 < p.m ? c0 : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cm[s][k] = c0 + k < p.m;
  }
  const float* __restrict__ zbase = p.z;
  const float* __restrict__ ubase = p.u;
  auto load_slab = [&](int slab) {
    const int r0 = slab * R;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int row = r0 + r < p.n ? r0 + r : p.n - 1;
      un[r] = ubase[row];
      const float* zr = zbase + (int64_t)row * p.ld;
#pragma unroll
      for (int s = 0; s < CPT; ++s) {   // streamed once per launch: non-temporal
        const f32x4 z = __builtin_nontemporal_load((const f32x4*)(zr + cl[s]));
        zn[r][s] = make_float4(z[0], z[1], z[2], z[3]);
      }
    }
  };
  if ((int)blockIdx.x < n_slabs) load_slab(blockIdx.x);
  for (int slab = blockIdx.x; slab < n_slabs; slab += p.G) {
    const int r0 = slab * R;
    float4 e[R][CPT];
    float rs[R], ucur[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      ucur[r] = un[r];
#pragma unroll
      for (int s = 0; s < CPT; ++s) e[r][s] = zn[r][s];
    }
    if (slab + p.G < n_slabs) load_slab(slab + p.G);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool live = r0 + r < p.n;
      const float ui = ucur[r];
      rs[r] = 0.f;
#pragma unroll
      for (int s = 0; s < CPT; ++s) {
        const float4 z = e[r][s];
        float4 x;
        x.x = (live && cm[s][0]) ? __expf(z.x + ui + vq[s].x) : 0.f;
        x.y = (live && cm[s][1]) ? __expf(z.y + ui + vq[s].y) : 0.f;
        x.z = (live && cm[s][2]) ? __expf(z.z + ui + vq[s].z) : 0.f;
        x.w = (live && cm[s][3]) ? __expf(z.w + ui + vq[s].w) : 0.f;
        e[r][s] = x;
        rs[r] += (x.x + x.y) + (x.z + x.w);
      }
    }
    {
      int rrow;
      const float w = wave_reduce_rows<R>(rs, lane, rrow);
      if ((lane & (64 / R - 1)) == 0) red[wave][rrow] = w;
    }
    __syncthreads();
    if (t < R) {
      const int row = r0 + t;
      float f = 0.f;
      if (row < p.n) {
        float tot = 0.f;
        for (int w = 0; w < nw; ++w) tot += red[w][t];
        const float ui = p.u[row];
        const float ebin = __expf(alpha + ui + vbin);
        tot += ebin;
        if (!(tot > 0.f) || !(tot < 3.0e38f)) ot_raise_status(p.status, guard_code);
        const float du = p.norm - logf(tot);
        p.u[row] = ui + du;
        f = __expf(du);
        red[0][t] = ebin * f;   // this row's share of the dustbin column (read by thread 0 below)
      } else {
        red[0][t] = 0.f;
      }
      fac[t] = f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float f = fac[r];
#pragma unroll
      for (int s = 0; s < CPT; ++s) {
        acc[s].x += e[r][s].x * f; acc[s].y += e[r][s].y * f; acc[s].z += e[r][s].z * f; acc[s].w += e[r][s].w * f;
      }
    }
    if (t == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) accbin += red[0][r];
    }
    __syncthreads();
  }

  float* pp = p.partial + (int64_t)blockIdx.x * (p.m + 1);
#pragma unroll
  for (int s = 0; s < CPT; ++s) {
    const int c0 = 4 * (t + blockDim.x * s);
    if (c0 + 0 < p.m) pp[c0 + 0] = acc[s].x;
    if (c0 + 1 < p.m) pp[c0 + 1] = acc[s].y;
    if (c0 + 2 < p.m) pp[c0 + 2] = acc[s].z;
    if (c0 + 3 < p.m) pp[c0 + 3] = acc[s].w;
  }
  if (t == 0) pp[p.m] = accbin;
}

// v_j += log nu_j - log(sum of partials)    block = 64 columns x 16 partial groups; every thread issues its
// (<= 32) loads back to back so the fold is one memory round trip, not a dependent chain
__global__ __launch_bounds__(1024) void ot_colreduce_kernel(const OtDev* __restrict__ probs, int slot, int rescue) {
  __shared__ float red[16][64];
  const OtDev p = probs[blockIdx.y];
  if (rescue && p.status[0] != 3.f && p.status[0] != 4.f) return;
  const float guard_code = rescue ? 4.f : 1.f;
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  if (blockIdx.x * 64 > p.m) return;
  float s = 0.f;
  if (col <= p.m) {
    const float* pp = p.partial + col;
    const int64_t st = p.m + 1;
    for (int b0 = g; b0 < p.G; b0 += 128) {   // 8 independent loads per trip
      float x[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int b = b0 + 16 * q;
        x[q] = b < p.G ? pp[(int64_t)b * st] : 0.f;
      }
      s += ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));
    }
  }
  red[g][cl] = s;
  __syncthreads();
  if (g == 0 && col <= p.m) {
    float c = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) c += red[q][cl];
    if (!(c > 0.f) || !(c < 3.0e38f)) ot_raise_status(p.status, guard_code);
    const float lognu = col < p.m ? p.norm : p.log_nu_bin;
    const float nv = p.v[col] + (lognu - logf(c));
    p.v[col] = nv;
    if (p.hist && slot >= 0) p.hist[(int64_t)slot * (p.n + p.m + 2) + p.n + 1 + col] = nv;       // recorded solve: v after this iteration
  }
  if (p.hist && slot >= 0 && g == 1) {                      // ... and u (final since the row kernel of this iteration)
    float* hu = p.hist + (int64_t)slot * (p.n + p.m + 2);
    // striped over THIS problem's live blocks (blockIdx.x <= m / 64): the grid is sized for the largest m of the call, and the
    // blocks beyond a smaller problem's columns have returned above
    for (int i = blockIdx.x * 64 + cl; i <= p.n; i += (p.m / 64 + 1) * 64) hu[i] = p.u[i];
  }
}

// ---------------------------------------------------------------------------------------------- selection
// t_ij = ((Z_ij + u_i) + v_j) - norm on the inner block (gmatcher.py:47,68,284): row max/argmax directly,
// column max/argmax through per-workgroup partials (rows visited in ascending order; ties -> lower index).
template <int CPT, int RS = OT_R>      // RS rows per slab (8; 2 for the 8-quad instance of problems wider than 16 384 columns: registers)
__global__ __launch_bounds__(1024) void ot_select_kernel(const OtDev* __restrict__ probs) {
  __shared__ float rv[16][RS];
  __shared__ int ri[16][RS];
  const OtDev p = probs[blockIdx.y];
  if ((int)blockIdx.x >= p.G) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nw = blockDim.x >> 6;
  float4 vq[CPT], cb[CPT];
  int4 cbi[CPT];
#pragma unroll
  for (int s = 0; s < CPT; ++s) {
    const int c0 = 4 * (t + blockDim.x * s);
    vq[s].x = c0 + 0 < p.m ? p.v[c0 + 0] : 0.f;
    vq[s].y = c0 + 1 < p.m ? p.v[c0 + 1] : 0.f;
    vq[s].z = c0 + 2 < p.m ? p.v[c0 + 2] : 0.f;
    vq[s].w = c0 + 3 < p.m ? p.v[c0 + 3] : 0.f;
    cb[s] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    cbi[s] = make_int4(0, 0, 0, 0);
  }
  const int n_slabs = (p.n + RS - 1) / RS;
  // all RS x CPT row pieces of a slab are requested before the first one is used (clamped rows: unconditional loads), and the NEXT slab's
  // pieces are requested before this slab's reductions: row by row the kernel paid one HBM latency per row (12.8 us per 8-row slab, 2.7 TB/s)
  float4 zs[RS][CPT], zn[RS][CPT];
  float us[RS], un[RS];
  auto request = [&](int slab, float4 (&zd)[RS][CPT], float (&ud)[RS]) __attribute__((always_inline)) {
    const int r0 = slab * RS;
#pragma unroll
    for (int r = 0; r < RS; ++r) {
      int rowc = r0 + r < p.n ? r0 + r : p.n - 1;
      rowc = rowc < 0 ? 0 : rowc;
      ud[r] = p.u[rowc];
#pragma unroll
      for (int s = 0; s < CPT; ++s) {
        const int c0 = 4 * (t + blockDim.x * s);
        zd[r][s] = *(const float4*)(p.z + (int64_t)rowc * p.ld + (c0 < p.m ? c0 : 0));     // rows are padded to 4 floats: in bounds
      }
    }
  };
  if ((int)blockIdx.x < n_slabs) request(blockIdx.x, zn, un);
  for (int slab = blockIdx.x; slab < n_slabs; slab += p.G) {
    const int r0 = slab * RS;
#pragma unroll
    for (int r = 0; r < RS; ++r) {
      us[r] = un[r];
#pragma unroll
      for (int s = 0; s < CPT; ++s) zs[r][s] = zn[r][s];
    }
    if (slab + p.G < n_slabs) request(slab + p.G, zn, un);
    float rbv[RS];
    int rbi[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) {
      const int row = r0 + r;
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      if (row < p.n) {
        const float ui = us[r];
#pragma unroll
        for (int s = 0; s < CPT; ++s) {
          const int c0 = 4 * (t + blockDim.x * s);
          const float4 z = zs[r][s];
          const float zz[4] = {z.x, z.y, z.z, z.w};
          const float vv[4] = {vq[s].x, vq[s].y, vq[s].z, vq[s].w};
          float* cbp = (float*)&cb[s];
          int* cip = (int*)&cbi[s];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (c0 + k < p.m) {
              const float tv = ((zz[k] + ui) + vv[k]) - p.norm;
              if (tv > bv) { bv = tv; bi = c0 + k; }
              if (tv > cbp[k]) { cbp[k] = tv; cip[k] = row; }
            }
          }
        }
      }
      rbv[r] = bv;
      rbi[r] = bi;
    }
    // wave argmax of all RS rows at once (ties -> lower column; the comparison is a strict total order, so the result does not depend on the
    // combination order): a reduce-scatter butterfly -- log2 RS steps halve the rows a lane still carries, the rest fold the survivor --
    // RS - 1 + (6 - log2 RS) exchanges of a (value, index) pair instead of RS x (4 DPP steps + 3 readlane folds): the per-row form was 30 of
    // this kernel's 158 us at 8 x 4096^2.
    {
      int rrow;
      float fv;
      int fi;
      wave_argmax_rows<RS>(rbv, rbi, lane, rrow, fv, fi);
      if ((lane & (64 / RS - 1)) == 0) { rv[wave][rrow] = fv; ri[wave][rrow] = fi; }
    }
    __syncthreads();
    if (t < RS && r0 + t < p.n) {
      float bv = rv[0][t];
      int bi = ri[0][t];
      for (int w = 1; w < nw; ++w) {
        const float ov = rv[w][t];
        const int oi = ri[w][t];
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      p.max0[r0 + t] = bv;
      p.idx0[r0 + t] = bi;
    }
    __syncthreads();
  }
  float* pv = p.cbest_val + (int64_t)blockIdx.x * p.m;
  int* pi = p.cbest_idx + (int64_t)blockIdx.x * p.m;
#pragma unroll
  for (int s = 0; s < CPT; ++s) {
    const int c0 = 4 * (t + blockDim.x * s);
    const float* cbp = (const float*)&cb[s];
    const int* cip = (const int*)&cbi[s];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k < p.m) { pv[c0 + k] = cbp[k]; pi[c0 + k] = cip[k]; }
  }
}

// column maxima over the row slabs' partial results: 32 columns x 8 slab groups per workgroup (one thread per column walking all
// G slabs was a serial chain of 512 dependent loads: 89 us for one 4096 x 4096 pair); ties go to the smaller row index, in any
// combination order
__global__ __launch_bounds__(256) void ot_colbest_kernel(const OtDev* __restrict__ probs) {
  const OtDev p = probs[blockIdx.y];
  __shared__ float sv[8][32];
  __shared__ int si[8][32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, col = blockIdx.x * 32 + tx;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  if (col < p.m)
    for (int b = ty; b < p.G; b += 8) {
      const float ov = p.cbest_val[(int64_t)b * p.m + col];
      const int oi = p.cbest_idx[(int64_t)b * p.m + col];
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
  sv[ty][tx] = bv;
  si[ty][tx] = bi;
  __syncthreads();
  if (ty == 0 && col < p.m) {
#pragma unroll
    for (int q = 1; q < 8; ++q) {
      const float ov = sv[q][tx];
      const int oi = si[q][tx];
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    p.max1[col] = bv;
    p.idx1[col] = bi;
  }
}

// gmatcher.py:286-294
__global__ __launch_bounds__(256) void ot_mutual_kernel(const OtDev* __restrict__ probs, float thr) {
  const OtDev p = probs[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool bad = p.status[0] != 0.f;
  if (i < p.n) {
    const int j = p.idx0[i];
    const bool mutual = (unsigned)j < (unsigned)p.m && p.idx1[j] == i;
    const float sc = mutual ? expf(p.max0[i]) : 0.f;
    p.mscores0[i] = sc;
    p.matches0[i] = (!bad && mutual && sc > thr) ? (int64_t)j : (int64_t)-1;
  }
  if (i < p.m) {
    const int r = p.idx1[i];
    const bool rok = (unsigned)r < (unsigned)p.n;
    const bool mutual1 = rok && p.idx0[r] == i;
    // mscores1 = where(mutual1, mscores0[idx1], 0); valid1 = mutual1 & valid0[idx1]
    const int jr = rok ? p.idx0[r] : -1;
    const bool mutual0_r = rok && (unsigned)jr < (unsigned)p.m && p.idx1[jr] == r;
    const float sc0 = mutual0_r ? expf(p.max0[r]) : 0.f;
    p.mscores1[i] = mutual1 ? sc0 : 0.f;
    const bool valid0_r = mutual0_r && sc0 > thr;
    p.matches1[i] = (!bad && mutual1 && valid0_r) ? (int64_t)r : (int64_t)-1;
  }
}

__global__ void ot_matrix_kernel(const float* __restrict__ z, int64_t ld, int n, int m, float alpha,
                                 const float* __restrict__ uv, float* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = blockIdx.y;
  if (j > m || i > n) return;
  const float norm = -logf((float)n + (float)m);
  const float zz = (i < n && j < m) ? z[(int64_t)i * ld + j] : alpha;
  out[(int64_t)i * (m + 1) + j] = ((zz + uv[i]) + uv[n + 1 + j]) - norm;
}

// ---------------------------------------------------------------------------------------------- training loss (forward)
// forward_train's loss on top of the solved potentials (gmatcher.py:333-386): the (N+1)x(M+1) OT matrix is not materialised,
// the ground-truth cells are gathered as (Z_ij + u_i) + v_j - norm.
//   phase 1 (one thread per ground-truth row (b, i0, i1), ORIGINAL keypoint ids): remap through the sorted kept lists
//   (gmatcher.py:340-367; binary search instead of the reference's dicts), a row whose i0 / i1 is -1 or was dropped by the
//   adaptive graph becomes (b, -1, -1) -- which the reference's indexing reads as the CORNER cell scores[b, -1, -1] = OT[N, M]
//   (gmatcher.py:372) -- and is a negative; clamp to [-100, 0], negate (373-376).
//   phase 2 (one wave per batch element, fixed order): scatter_mean of the positive / negative losses by batch element
//   (380), then the batch means times the weights (383-385).
__device__ __forceinline__ int kept_find(const int32_t* kept, int n, int64_t orig) {
  int lo = 0, hi = n - 1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const int v = kept[mid];
    if (v == orig) return mid;
    if (v < orig) lo = mid + 1; else hi = mid - 1;
  }
  return -1;
}

__global__ void train_loss_gather_kernel(const gims_loss_pair* __restrict__ pairs, int n_pairs, const int64_t* __restrict__ gt, int K,
                                         float alpha, float* __restrict__ loss_vec, int32_t* __restrict__ tag) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const int64_t b = gt[3 * k], i0 = gt[3 * k + 1], i1 = gt[3 * k + 2];
  if (b < 0 || b >= n_pairs) { tag[k] = -1; loss_vec[k] = 0.f; return; }      // the reference would raise IndexError; ignored here
  const gims_loss_pair p = pairs[b];
  int r0 = -1, r1 = -1;
  if (i0 != -1 && i1 != -1) {
    r0 = kept_find(p.kept0, p.n, i0);
    r1 = kept_find(p.kept1, p.m, i1);
  }
  const bool neg = r0 < 0 || r1 < 0;
  const float norm = -logf((float)p.n + (float)p.m);
  const float* u = p.uv;
  const float* v = p.uv + p.n + 1;
  float x = neg ? ((alpha + u[p.n]) + v[p.m]) - norm : ((p.scores[(int64_t)r0 * p.ld + r1] + u[r0]) + v[r1]) - norm;
  x = fminf(fmaxf(x, -100.f), 0.f);
  loss_vec[k] = -x;
  tag[k] = (int32_t)b | (neg ? (int32_t)0x40000000 : 0);
}

__global__ __launch_bounds__(1024) void train_loss_reduce_kernel(const float* __restrict__ loss_vec, int32_t* __restrict__ tag, int K,
                                                                 int n_pairs, float pos_w, float neg_w, float* __restrict__ out3) {
  __shared__ float pos_mean[1024], neg_mean[1024];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < n_pairs; b += 16) {
    float ps = 0.f, ns = 0.f, pc = 0.f, nc = 0.f;
    for (int k = lane; k < K; k += 64) {
      const int32_t t = tag[k];
      if (t < 0 || (t & 0x3fffffff) != b) continue;
      if (t & 0x40000000) { ns += loss_vec[k]; nc += 1.f; } else { ps += loss_vec[k]; pc += 1.f; }
    }
    ps = wave_sum(ps); ns = wave_sum(ns); pc = wave_sum(pc); nc = wave_sum(nc);
    if (lane == 0) {
      pos_mean[b] = ps / fmaxf(pc, 1.f); neg_mean[b] = ns / fmaxf(nc, 1.f);    // scatter_mean: empty groups give 0
      tag[K + 2 * b] = (int32_t)pc; tag[K + 2 * b + 1] = (int32_t)nc;          // group sizes, for gims_train_loss_grad
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ps = 0.f, ns = 0.f;
    for (int b = 0; b < n_pairs; ++b) { ps += pos_mean[b]; ns += neg_mean[b]; }
    const float pl = pos_w * (ps / (float)n_pairs), nl = neg_w * (ns / (float)n_pairs);
    out3[0] = pl + nl; out3[1] = pl; out3[2] = nl;
  }
}

// ---------------------------------------------------------------------------------------------- backward through the Sinkhorn iterations
// d loss / d scores and d loss / d bin_score for forward_train: reverse mode through the UNROLLED iterations of
// log_sinkhorn_iterations (gmatcher.py:41-47), which is what autograd does in the reference.  With Zc the (n+1) x (m+1)
// couplings (scores + the alpha border), out = Zc + u_I + v_I - norm and
//     u_k = log mu - LSE_j(Zc + v_{k-1}),      v_k = log nu - LSE_i(Zc + u_k),      u_0 = v_0 = 0,
// the softmax weights of the two LSEs are  R^k_ij = exp(Zc_ij + u_k[i] + v_{k-1}[j] - log mu_i)  and
// C^k_ij = exp(Zc_ij + u_k[i] + v_k[j] - log nu_j).  Reverse sweep, k = I .. 1, with gu = dL/du_k, gv = dL/dv_k:
//     dZc -= gv[j] C^k_ij ;  gu[i] -= sum_j gv[j] C^k_ij ;   then   dZc -= gu[i] R^k_ij ;  gv'[j] = - sum_i gu[i] R^k_ij
// starting from dZc = G = dL/dout, gu = row sums of G, gv = column sums of G.  The potentials of every iteration come from
// a recorded forward solve (gims_sinkhorn_history).  Fixed summation order throughout.
//
// The fused sweep: ONE pass over Z and one read-modify-write of dZc per iteration.  A workgroup owns a slab of 8 rows, a
// thread the columns j = t, t + 256, ...: phase 1 reduces sum_j gv[j] C_ij per row over the workgroup (gu_k[i] is final right
// after its own row's reduction); phase 2 recomputes C, adds the row-step term gu_k[i] R_ij, updates dZc once and keeps the
// column sums of the row-step terms of its 8 rows -> colpart[slab][j]; ot_bwd_colsum_kernel folds the slabs in order -> gv_{k-1}.
constexpr int BW_ROWS = 4;
template <bool INIT>
__global__ __launch_bounds__(256) void ot_bwd_fused_kernel(const OtBwd* __restrict__ probs, float alpha, int k, int first) {
  const OtBwd p = probs[blockIdx.y];
  const int r0 = blockIdx.x * BW_ROWS;
  if (r0 > p.n) return;
  const int nr = min(BW_ROWS, p.n + 1 - r0);
  const int ldz = p.m + 1, tid = threadIdx.x;
  __shared__ float red[4][BW_ROWS];
  __shared__ float gnew[BW_ROWS];
  float acc[BW_ROWS];
#pragma unroll
  for (int r = 0; r < BW_ROWS; ++r) acc[r] = 0.f;
  if constexpr (INIT) {           // gu = row sums of G, colpart = per-slab column sums of G
    for (int j = tid; j <= p.m; j += 256) {
      float cs = 0.f;
#pragma unroll
      for (int r = 0; r < BW_ROWS; ++r)
        if (r < nr) {
          const float g = p.dz[(int64_t)(r0 + r) * ldz + j];
          acc[r] += g;
          cs += g;
        }
      p.colpart[(int64_t)blockIdx.x * ldz + j] = cs;
    }
  } else {
    const float* uk = p.hist + (int64_t)k * p.hstride;
    const float* vk = uk + p.n + 1;
    const float* vprev = p.hist + (int64_t)(k - 1) * p.hstride + p.n + 1;
    float ui[BW_ROWS];
#pragma unroll
    for (int r = 0; r < BW_ROWS; ++r) ui[r] = r < nr ? uk[r0 + r] : 0.f;
    for (int j = tid; j <= p.m; j += 256) {
      const float w = vk[j] - (j < p.m ? p.norm : p.log_nu_bin), gvj = p.gv[j];
#pragma unroll
      for (int r = 0; r < BW_ROWS; ++r)
        if (r < nr) {
          const int i = r0 + r;
          const float z = (i < p.n && j < p.m) ? p.z[(int64_t)i * p.ld + j] : alpha;
          acc[r] += gvj * __expf(z + ui[r] + w);
        }
    }
#pragma unroll
    for (int r = 0; r < BW_ROWS; ++r) acc[r] = wave_sum(acc[r]);
    if ((tid & 63) == 0)
#pragma unroll
      for (int r = 0; r < BW_ROWS; ++r) red[tid >> 6][r] = acc[r];
    __syncthreads();
    if (tid < BW_ROWS) gnew[tid] = ((first && tid < nr) ? p.gu[r0 + tid] : 0.f) - ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]));
    __syncthreads();
    for (int j = tid; j <= p.m; j += 256) {
      const float w = vk[j] - (j < p.m ? p.norm : p.log_nu_bin), gvj = p.gv[j];
      const float vp = k > 1 ? vprev[j] : 0.f;
      float cs = 0.f;
#pragma unroll
      for (int r = 0; r < BW_ROWS; ++r)
        if (r < nr) {
          const int i = r0 + r;
          const float z = (i < p.n && j < p.m) ? p.z[(int64_t)i * p.ld + j] : alpha;
          const float t = gvj * __expf(z + ui[r] + w);
          const float t2 = gnew[r] * __expf(z + ui[r] + vp - (i < p.n ? p.norm : p.log_mu_bin));
          p.dz[(int64_t)i * ldz + j] -= t + t2;
          cs += t2;
        }
      p.colpart[(int64_t)blockIdx.x * ldz + j] = cs;
    }
    return;
  }
  // INIT: row sums -> gu
#pragma unroll
  for (int r = 0; r < BW_ROWS; ++r) acc[r] = wave_sum(acc[r]);
  if ((tid & 63) == 0)
#pragma unroll
    for (int r = 0; r < BW_ROWS; ++r) red[tid >> 6][r] = acc[r];
  __syncthreads();
  if (tid < nr) p.gu[r0 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// gv[j] = sign * sum over slabs of colpart[slab][j]: 32 columns x 8 slab groups per workgroup, fixed order
__global__ __launch_bounds__(256) void ot_bwd_colsum_kernel(const OtBwd* __restrict__ probs, float sign) {
  const OtBwd p = probs[blockIdx.y];
  __shared__ float red[8][32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, j = blockIdx.x * 32 + tx;
  const int ns = (p.n + BW_ROWS) / BW_ROWS, ldz = p.m + 1;
  float s = 0.f;
  if (j <= p.m)
    for (int b = ty; b < ns; b += 8) s += p.colpart[(int64_t)b * ldz + j];
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && j <= p.m) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += red[i][tx];
    p.gv[j] = sign * t;
  }
}

// The same sweep for m + 1 <= 512 * CPT columns with the slab's Z values held in registers between the two phases (one read of Z);
// 512 threads: two workgroups fit on a CU, so the one-row slab of the dustbin row does not cost a second round.
template <int CPT>
__global__ __launch_bounds__(512) void ot_bwd_fused_reg_kernel(const OtBwd* __restrict__ probs, float alpha, int k, int first) {
  const OtBwd p = probs[blockIdx.y];
  const int r0 = blockIdx.x * BW_ROWS;
  if (r0 > p.n) return;
  const int nr = min(BW_ROWS, p.n + 1 - r0);
  const int ldz = p.m + 1, tid = threadIdx.x;
  __shared__ float red[8][BW_ROWS];
  __shared__ float gnew[BW_ROWS];
  const float* uk = p.hist + (int64_t)k * p.hstride;
  const float* vk = uk + p.n + 1;
  const float* vprev = p.hist + (int64_t)(k - 1) * p.hstride + p.n + 1;
  float ui[BW_ROWS], acc[BW_ROWS], zc[CPT][BW_ROWS], w[CPT], gvj[CPT];
#pragma unroll
  for (int r = 0; r < BW_ROWS; ++r) {
    ui[r] = r < nr ? uk[r0 + r] : 0.f;
    acc[r] = 0.f;
  }
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int j = tid + 512 * c;
    const bool on = j <= p.m;
    w[c] = on ? vk[j] - (j < p.m ? p.norm : p.log_nu_bin) : 0.f;
    gvj[c] = on ? p.gv[j] : 0.f;
#pragma unroll
    for (int r = 0; r < BW_ROWS; ++r) {
      const int i = r0 + r;
      float z = alpha;
      if (on && r < nr && i < p.n && j < p.m) z = p.z[(int64_t)i * p.ld + j];
      zc[c][r] = z;
      if (on && r < nr) acc[r] += gvj[c] * __expf(z + ui[r] + w[c]);
    }
  }
#pragma unroll
  for (int r = 0; r < BW_ROWS; ++r) acc[r] = wave_sum(acc[r]);
  if ((tid & 63) == 0)
#pragma unroll
    for (int r = 0; r < BW_ROWS; ++r) red[tid >> 6][r] = acc[r];
  __syncthreads();
  if (tid < BW_ROWS)
    gnew[tid] = ((first && tid < nr) ? p.gu[r0 + tid] : 0.f) -
                (((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) + ((red[4][tid] + red[5][tid]) + (red[6][tid] + red[7][tid])));
  __syncthreads();
  float gn[BW_ROWS];
#pragma unroll
  for (int r = 0; r < BW_ROWS; ++r) gn[r] = gnew[r];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int j = tid + 512 * c;
    if (j > p.m) continue;
    const float vp = k > 1 ? vprev[j] : 0.f;
    float cs = 0.f;
#pragma unroll
    for (int r = 0; r < BW_ROWS; ++r)
      if (r < nr) {
        const int i = r0 + r;
        const float t = gvj[c] * __expf(zc[c][r] + ui[r] + w[c]);
        const float t2 = gn[r] * __expf(zc[c][r] + ui[r] + vp - (i < p.n ? p.norm : p.log_mu_bin));
        p.dz[(int64_t)i * ldz + j] -= t + t2;
        cs += t2;
      }
    p.colpart[(int64_t)blockIdx.x * ldz + j] = cs;
  }
}

// LOW-RANK form of the sweep (default): every term subtracted from dZc factorises,
//     gv_k[j] C^k_ij = e^{Zc_ij} * e^{u_k[i]} * (gv_k[j] e^{v_k[j] - log nu_j}),    gu_k[i] R^k_ij = e^{Zc_ij} * (gu_k[i] e^{u_k[i] - log mu_i}) * e^{v_{k-1}[j]},
// so  dZc = G - e^{Zc} o (P Q^T)  with P = [e^{u_k} | gu_k e^{u_k - log mu}] ((n+1) x 2I) and Q = [gv_k e^{v_k - log nu} | e^{v_{k-1}}] ((m+1) x 2I):
// the per-iteration kernels only run the two reductions (gu_k, gv_{k-1}) and RECORD them -- Z is read once per iteration (17 MB at
// 2048^2, L2 / MALL resident) and dZc is never touched (its read-modify-write was 34 of the 50 MB per iteration) --, and one K = 2I
// product at the end (gims_gemm_f32, bf16x6) rebuilds all I updates at once.  Potentials stay within e^{+-20}: no range problem in f32.
template <int CPT>
__global__ __launch_bounds__(512) void ot_bwd_reduce_kernel(const OtBwd* __restrict__ probs, float alpha, int k, int first) {
  const OtBwd p = probs[blockIdx.y];
  const int r0 = blockIdx.x * BW_ROWS;
  if (r0 > p.n) return;
  const int nr = min(BW_ROWS, p.n + 1 - r0);
  const int ldz = p.m + 1, tid = threadIdx.x;
  __shared__ float red[8][BW_ROWS];
  __shared__ float gnew[BW_ROWS];
  const float* uk = p.hist + (int64_t)k * p.hstride;
  const float* vk = uk + p.n + 1;
  const float* vprev = p.hist + (int64_t)(k - 1) * p.hstride + p.n + 1;
  const float* gvk = p.gv_rec + (int64_t)k * ldz;               // gv entering iteration k
  float ui[BW_ROWS], acc[BW_ROWS], zc[CPT][BW_ROWS];
#pragma unroll
  for (int r = 0; r < BW_ROWS; ++r) {
    ui[r] = r < nr ? uk[r0 + r] : 0.f;
    acc[r] = 0.f;
  }
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int j = tid + 512 * c;
    const bool on = j <= p.m;
    const float w = on ? vk[j] - (j < p.m ? p.norm : p.log_nu_bin) : 0.f;
    const float gvj = on ? gvk[j] : 0.f;
#pragma unroll
    for (int r = 0; r < BW_ROWS; ++r) {
      const int i = r0 + r;
      float z = alpha;
      if (on && r < nr && i < p.n && j < p.m) z = p.z[(int64_t)i * p.ld + j];
      zc[c][r] = z;
      if (on && r < nr) acc[r] += gvj * __expf(z + ui[r] + w);
    }
  }
#pragma unroll
  for (int r = 0; r < BW_ROWS; ++r) acc[r] = wave_sum(acc[r]);
  if ((tid & 63) == 0)
#pragma unroll
    for (int r = 0; r < BW_ROWS; ++r) red[tid >> 6][r] = acc[r];
  __syncthreads();
  if (tid < BW_ROWS) {
    const float gn = ((first && tid < nr) ? p.gu[r0 + tid] : 0.f) -
                     (((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) + ((red[4][tid] + red[5][tid]) + (red[6][tid] + red[7][tid])));
    gnew[tid] = gn;
    if (tid < nr) p.gu_rec[(int64_t)k * (p.n + 1) + r0 + tid] = gn;
  }
  __syncthreads();
  float gn[BW_ROWS];
#pragma unroll
  for (int r = 0; r < BW_ROWS; ++r) gn[r] = gnew[r];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int j = tid + 512 * c;
    if (j > p.m) continue;
    const float vp = k > 1 ? vprev[j] : 0.f;
    float cs = 0.f;
#pragma unroll
    for (int r = 0; r < BW_ROWS; ++r)
      if (r < nr) cs += gn[r] * __expf(zc[c][r] + ui[r] + vp - (r0 + r < p.n ? p.norm : p.log_mu_bin));
    p.colpart[(int64_t)blockIdx.x * ldz + j] = cs;
  }
}

// gv_rec[slot][j] = sign * sum over slabs of colpart[slab][j].  16 columns x 64 slab groups per workgroup: every thread issues its (<= 8 per trip)
// loads back to back, so the fold of ~500 slabs is one memory round trip (32 columns x 8 groups walked 16 dependent trips: 8.4 us per launch
// once the slabs were 4 rows), and the grid has m / 16 workgroups instead of m / 32.
__global__ __launch_bounds__(1024) void ot_bwd_colsum_rec_kernel(const OtBwd* __restrict__ probs, float sign, int slot) {
  const OtBwd p = probs[blockIdx.y];
  __shared__ float red[64][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, j = blockIdx.x * 16 + tx;
  if (blockIdx.x * 16 > p.m) return;
  const int ns = (p.n + BW_ROWS) / BW_ROWS, ldz = p.m + 1;
  float s = 0.f;
  if (j <= p.m)
    for (int b0 = ty; b0 < ns; b0 += 512) {
      float x[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) x[q] = b0 + 64 * q < ns ? p.colpart[(int64_t)(b0 + 64 * q) * ldz + j] : 0.f;
      s += ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));
    }
  red[ty][tx] = s;
  __syncthreads();
  float a = 0.f;                                             // 64 groups -> 16 -> 1, fixed order
  if (ty < 16) a = (red[ty][tx] + red[ty + 16][tx]) + (red[ty + 32][tx] + red[ty + 48][tx]);
  __syncthreads();                                           // (every thread reaches both barriers: none sits in a divergent branch)
  if (ty < 16) red[ty][tx] = a;
  __syncthreads();
  if (ty == 0 && j <= p.m) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += red[i][tx];
    p.gv_rec[(int64_t)slot * ldz + j] = sign * t;
  }
}

// per-row / per-column shifts of the factorisation: a_i = max_k u_k[i] (-> p.gu), b_j = max over the v_k[j] that occur (k = 0 .. I, v_0 = 0;
// -> p.gv2).  With them every factor is <= 1 in magnitude times the recorded gradient: the potentials of a peaked problem span more
// than the 88 nats e^x covers in f32, their differences from the running maximum do not matter below e^-88.
__global__ __launch_bounds__(256) void ot_bwd_shift_kernel(const OtBwd* __restrict__ probs) {
  const OtBwd p = probs[blockIdx.y];
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t <= p.n) {
    float a = -INFINITY;
    for (int k = 1; k <= p.iters; ++k) a = fmaxf(a, p.hist[(int64_t)k * p.hstride + t]);
    p.gu[t] = a;
  }
  if (t <= p.m) {
    float b = 0.f;                                          // v_0 = 0
    for (int k = 1; k <= p.iters; ++k) b = fmaxf(b, p.hist[(int64_t)k * p.hstride + p.n + 1 + t]);
    p.gv2[t] = b;
  }
}

// factor matrices: P[i][k-1] = e^{u_k[i] - a_i}, P[i][I + k-1] = gu_k[i] e^{u_k[i] - log mu_i - a_i};
//                  Q[j][k-1] = gv_k[j] e^{v_k[j] - log nu_j - b_j}, Q[j][I + k-1] = e^{v_{k-1}[j] - b_j}
__global__ __launch_bounds__(256) void ot_bwd_factor_kernel(const OtBwd* __restrict__ probs) {
  const OtBwd p = probs[blockIdx.y];
  const int I = p.iters, ld = 2 * I;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t np_ = (int64_t)(p.n + 1) * I, nq = (int64_t)(p.m + 1) * I;
  if (idx < np_) {
    const int i = (int)(idx / I), k = (int)(idx - (int64_t)i * I) + 1;
    const float u = p.hist[(int64_t)k * p.hstride + i] - p.gu[i];
    p.fp[(int64_t)i * ld + k - 1] = __expf(u);
    p.fp[(int64_t)i * ld + I + k - 1] = p.gu_rec[(int64_t)k * (p.n + 1) + i] * __expf(u - (i < p.n ? p.norm : p.log_mu_bin));
  } else if (idx < np_ + nq) {
    const int64_t e = idx - np_;
    const int j = (int)(e / I), k = (int)(e - (int64_t)j * I) + 1;
    const float b = p.gv2[j];
    const float v = p.hist[(int64_t)k * p.hstride + p.n + 1 + j] - b;
    const float vp = (k > 1 ? p.hist[(int64_t)(k - 1) * p.hstride + p.n + 1 + j] : 0.f) - b;
    p.fq[(int64_t)j * ld + k - 1] = p.gv_rec[(int64_t)k * (p.m + 1) + j] * __expf(v - (j < p.m ? p.norm : p.log_nu_bin));
    p.fq[(int64_t)j * ld + I + k - 1] = __expf(vp);
  }
}

// dZc = G - e^{Zc + a_i + b_j} o T
__global__ __launch_bounds__(256) void ot_bwd_combine_kernel(const OtBwd* __restrict__ probs, float alpha) {
  const OtBwd p = probs[blockIdx.z];
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (i > p.n || j > p.m) return;
  const float t = p.tmat[(int64_t)i * p.ldt + j];
  if (t == 0.f) return;
  const float z = (i < p.n && j < p.m) ? p.z[(int64_t)i * p.ld + j] : alpha;
  p.dz[(int64_t)i * (p.m + 1) + j] -= __expf(z + p.gu[i] + p.gv2[j]) * t;
}

// d alpha = sum of dZc over the border cells (dustbin row, dustbin column, corner once)
__global__ __launch_bounds__(256) void ot_bwd_alpha_kernel(const OtBwd* __restrict__ probs) {
  const OtBwd p = probs[blockIdx.x];
  __shared__ float red[4];
  const int ldz = p.m + 1;
  float s = 0.f;
  for (int j = threadIdx.x; j <= p.m; j += 256) s += p.dz[(int64_t)p.n * ldz + j];
  for (int i = threadIdx.x; i < p.n; i += 256) s += p.dz[(int64_t)i * ldz + p.m];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) p.dalpha[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

// G = dL/dout scattered into the zeroed dZc: the loss is  sum_b [ w_pos/(B cnt_pos_b) sum_pos (-x) + w_neg/(B cnt_neg_b) sum_neg (-x) ]
// with x = clamp(out, -100, 0): d/d out = -w / (B cnt) inside the clamp, 0 outside (gmatcher.py:372-385).
__global__ void train_loss_grad_kernel(const gims_loss_pair* __restrict__ pairs, int n_pairs, const int64_t* __restrict__ gt, int K, float alpha,
                                       const int32_t* __restrict__ tag, float pos_w, float neg_w, float* const* __restrict__ dz_ptrs) {
  // one thread per ground-truth row; the group sizes per (batch element, sign) were left behind the tags by gims_train_loss
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const int32_t t = tag[k];
  if (t < 0) return;
  const int b = t & 0x3fffffff;
  const bool neg = (t & 0x40000000) != 0;
  const int cnt = tag[K + 2 * b + (neg ? 1 : 0)];
  const gims_loss_pair p = pairs[b];
  int r0 = p.n, r1 = p.m;                                   // negatives: the corner cell
  if (!neg) { r0 = kept_find(p.kept0, p.n, gt[3 * k + 1]); r1 = kept_find(p.kept1, p.m, gt[3 * k + 2]); }
  const float norm = -logf((float)p.n + (float)p.m);
  const float* u = p.uv;
  const float* v = p.uv + p.n + 1;
  const float x = neg ? ((alpha + u[p.n]) + v[p.m]) - norm : ((p.scores[(int64_t)r0 * p.ld + r1] + u[r0]) + v[r1]) - norm;
  if (!(x >= -100.f && x <= 0.f)) return;                    // clamped: zero gradient (torch.clamp's backward passes it on [min, max], bounds included)
  const float g = -(neg ? neg_w : pos_w) / ((float)n_pairs * (float)cnt);
  atomicAdd(dz_ptrs[b] + (int64_t)r0 * (p.m + 1) + r1, g);   // equal addends per cell group: the sum does not depend on the order
}

// ---------------------------------------------------------------------------------------------- rescue
// The on-chip kernel needs its 256 workgroups co-resident; when a bounded wait runs out (another process's kernels on the
// GPU, a straggling workgroup) it leaves status 2 and no potentials.  This kernel is enqueued right after the resident
// launches of every call and costs one empty launch when nothing happened: a workgroup looks at its problem's status word
// and returns unless it is 2.  Otherwise it re-solves THAT problem, alone, with no cross-workgroup dependency at all
// (one workgroup per problem walks the matrix twice per iteration: slow -- ~0.25 s for a 4096^2 problem -- but it cannot
// stall, and the batch leaves with valid matches instead of -1s).  Same recurrence as the streamed kernels
// (u = log mu - LSE_j(Z + v); v = log nu - LSE_i(Z + u), gmatcher.py:41-47), fixed summation order.
__global__ __launch_bounds__(1024) void ot_rescue_kernel(const OtDev* __restrict__ probs, float alpha, int iters, int force, int* __restrict__ counter) {
  const OtDev p = probs[blockIdx.x];
  if (!force && p.status[0] != 2.f) return;
  if (threadIdx.x == 0 && counter) atomicAdd(counter, 1);
  __shared__ float wsum[16];
  __shared__ int bad;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) bad = 0;
  // start potentials like ot_init_kernel: u = -max(alpha, row max), v = 0
  for (int j = t; j <= p.m; j += 1024) p.v[j] = 0.f;
  for (int i = wave; i < p.n; i += 16) {
    const float* zr = p.z + (int64_t)i * p.ld;
    float mx = alpha;
    for (int j = lane; j < p.m; j += 64) mx = fmaxf(mx, zr[j]);
    mx = wave_max(mx);
    if (lane == 0) p.u[i] = -mx;
  }
  if (t == 0) p.u[p.n] = -alpha;
  __threadfence_block();
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    // ---- rows: one wave per row (coalesced along the row); the dustbin row is row n
    const float vbin = p.v[p.m];
    for (int i = wave; i <= p.n; i += 16) {
      const float ui = p.u[i];
      float sacc = 0.f;
      if (i < p.n) {
        const float* zr = p.z + (int64_t)i * p.ld;
        for (int j = lane; j < p.m; j += 64) sacc += __expf(zr[j] + ui + p.v[j]);
      } else {
        for (int j = lane; j < p.m; j += 64) sacc += __expf(alpha + ui + p.v[j]);
      }
      sacc = wave_sum(sacc) + __expf(alpha + ui + vbin);
      if (lane == 0) {
        if (!(sacc > 0.f) || !(sacc < 3.0e38f)) bad = 1;
        p.u[i] = ui + (i < p.n ? p.norm : p.log_mu_bin) - logf(sacc);
      }
    }
    __threadfence_block();
    __syncthreads();
    // ---- columns: one thread per column (coalesced across the threads of a row visit); the dustbin column by wave 0 last
    const float ubin = p.u[p.n];
    for (int j = t; j < p.m; j += 1024) {
      const float vj = p.v[j];
      float sacc = 0.f;
      for (int i = 0; i < p.n; ++i) sacc += __expf(p.z[(int64_t)i * p.ld + j] + p.u[i] + vj);
      sacc += __expf(alpha + ubin + vj);
      if (!(sacc > 0.f) || !(sacc < 3.0e38f)) bad = 1;
      p.v[j] = vj + p.norm - logf(sacc);
    }
    {
      float sacc = 0.f;
      for (int i = t; i <= p.n; i += 1024) sacc += __expf(alpha + p.u[i] + vbin);
      sacc = wave_sum(sacc);
      if (lane == 0) wsum[wave] = sacc;
      __syncthreads();
      if (t == 0) {
        float tot = 0.f;
        for (int w = 0; w < 16; ++w) tot += wsum[w];
        if (!(tot > 0.f) || !(tot < 3.0e38f)) bad = 1;
        p.v[p.m] = vbin + p.log_nu_bin - logf(tot);
      }
    }
    __threadfence_block();
    __syncthreads();
  }
  if (t == 0) p.status[0] = bad ? 1.f : 0.f;
}

// test hook (GIMS_OT_FORCE_FAIL=1): what a timed-out resident solve leaves behind -- status 2 and garbage potentials
__global__ void ot_poison_kernel(const OtDev* __restrict__ probs) {
  const OtDev p = probs[blockIdx.x];
  for (int i = threadIdx.x; i <= p.n; i += blockDim.x) p.u[i] = __uint_as_float(0x7fc00000u);
  for (int j = threadIdx.x; j <= p.m; j += blockDim.x) p.v[j] = __uint_as_float(0x7fc00000u);
  if (threadIdx.x == 0) ot_raise_status(p.status, 2.f);
}

// ---- rescue by the streamed kernels (no cross-workgroup waits, full-chip parallelism: ~ the cost of a streamed solve).  All of its
// launches look at the problem's status word first and return at once unless the solve gave up: begin (2 -> 3 "being re-solved",
// counted), start potentials, `iters` x (ot_iter_kernel + ot_colreduce_kernel) with rescue = 1 (numeric guard raises 4), end (3 -> 0,
// 4 -> 1).  2 * iters + 3 near-empty launches when nothing happened, so the host enqueues the sequence only while the device is
// MARGINAL -- a give-up was seen during the last OT_MARGINAL_CALLS calls (the counter is read back lazily, without a synchronisation
// of its own) -- and the one-workgroup ot_rescue_kernel stays behind it as the last resort for the first give-up ever seen.
__global__ void ot_rescue_begin_kernel(const OtDev* __restrict__ probs, int np, int* __restrict__ counter) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np || probs[i].status[0] != 2.f) return;
  probs[i].status[0] = 3.f;
  atomicAdd(counter, 1);
}
__global__ void ot_rescue_end_kernel(const OtDev* __restrict__ probs, int np) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  const float st = probs[i].status[0];
  if (st == 3.f) probs[i].status[0] = 0.f;
  else if (st == 4.f) probs[i].status[0] = 1.f;
}

// ---- host side of the on-chip path
static int ot_cus() {
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, current_device()) != hipSuccess) n = 0;
  return n;
}

// Give-up bookkeeping, per device: a device counter of re-solved problems (bumped by the rescue kernels), mirrored into pinned host
// memory by an asynchronous copy at the end of every on-chip call; the copy of call k is looked at by call k + 1.
constexpr int OT_MARGINAL_CALLS = 256;
struct OtRescueState {
  int* d_count; volatile int* h_count; hipEvent_t ev;
  long calls, last_giveup_call; int seen;
};
static std::mutex g_rescue_mu;
static OtRescueState* ot_rescue_state() {
  static std::map<int, OtRescueState> states;
  const int dev = current_device();
  std::lock_guard<std::mutex> lock(g_rescue_mu);
  auto it = states.find(dev);
  if (it != states.end()) return &it->second;
  OtRescueState st{};
  st.d_count = (int*)device_once("ot_rescue_count", 256, nullptr);
  st.h_count = (volatile int*)pinned_once("ot_rescue_count", 256);
  if (!st.d_count || !st.h_count || hipEventCreateWithFlags(&st.ev, hipEventDisableTiming) != hipSuccess) return nullptr;
  st.last_giveup_call = -(long)OT_MARGINAL_CALLS - 1;
  return &states.emplace(dev, st).first->second;
}

// The on-chip kernel (2-D decomposition, sinkhorn2d.hip) is used whenever every problem has a geometry (n, m <= 4096) and the device has
// the 256 CUs its workgroups need; GIMS_OT_RESIDENT=0 / GIMS_OT_STREAMED select the streamed kernels.
static OtR2Plan ot_res2_choose(const gims_ot_problem* pr, int np, int iters, int flags) {
  OtR2Plan none{};
  if ((flags & GIMS_OT_STREAMED) || !env_int("GIMS_OT_RESIDENT", 1) || iters < 1 || ot_cus() < 256) return none;
  // (no size gate: measured down to one problem of 128^2 the 2-D kernel's ~5.5 us per iteration beats the two launches per
  // iteration of the streamed kernels -- 0.60 vs 0.75 ms per 100 iterations)
  std::vector<OtR2Host> h(np);
  for (int i = 0; i < np; ++i) { h[i] = OtR2Host{}; h[i].n = pr[i].n; h[i].m = pr[i].m; }
  return ot_res2_plan(h.data(), np, iters);
}

// The instances of the streamed kernels by column quads per thread: ot_iter_kernel<CPT, R> sweeps slabs of R rows, ot_select_kernel<CPT, RS>
// of RS rows.  f is called with the constants of the instance that serves cpt (the launches check cpt <= 8 first; sizing may ask beyond it).
template <int CPT_, int R_, int RS_> struct OtInst { static constexpr int CPT = CPT_, R = R_, RS = RS_; };
template <typename F>
static auto ot_instance(int cpt, F&& f) {
  if (cpt == 1) return f(OtInst<1, OT_R, OT_R>{});
  if (cpt == 2) return f(OtInst<2, 4, 4>{});      // (select: four-row slabs: eight staged 364 B of the row pieces in scratch)
  // (select: two rows per slab for the 4- and 8-quad instances: with eight, the two slabs' worth of staged rows are 256-512 registers per lane: 1.1 KB of scratch)
  if (cpt <= 4) return f(OtInst<4, 2, 2>{});
  return f(OtInst<8, 1, 2>{});                    // 16 384 < m <= 32 768 (round 5: the graph build's limit)
}
// The register-resident sweeps of the backward pass by column pieces per thread (cpt <= 9)
template <typename F>
static void ot_bwd_instance(int cpt, F&& f) {
  if (cpt <= 1) f(std::integral_constant<int, 1>{});
  else if (cpt <= 3) f(std::integral_constant<int, 3>{});
  else if (cpt <= 5) f(std::integral_constant<int, 5>{});
  else f(std::integral_constant<int, 9>{});
}

static void ot_launch_shape(const gims_ot_problem* pr, int np, int& threads, int& cpt, int& maxn, int& maxm) {
  maxn = 0; maxm = 0;
  for (int i = 0; i < np; ++i) { maxn = pr[i].n > maxn ? pr[i].n : maxn; maxm = pr[i].m > maxm ? pr[i].m : maxm; }
  const int quads = (maxm + 3) / 4;
  threads = ((quads + 63) / 64) * 64;
  if (threads > 1024) threads = 1024;
  if (threads < 64) threads = 64;
  cpt = (quads + threads - 1) / threads;
}
// workgroups per problem.  Large workgroups (one resident per CU) run persistent-style: ~256 in total, each
// walking several slabs with the prefetch above; small workgroups want ~4 per CU for latency hiding.
static int ot_G(int n, int np, int threads, int cpt) {
  const int rows = ot_instance(cpt, [](auto inst) { return decltype(inst)::R; });   // rows per slab of ot_iter_kernel<CPT, R>
  const int total = threads >= 1024 ? 256 : (threads >= 512 ? 512 : 1024);
  int cap = total / (np > 0 ? np : 1);
  if (cap < 4) cap = 4;
  int g = (n + rows - 1) / rows;
  return g < cap ? g : cap;
}
static void ot_fill_common(const gims_ot_problem& q, float& norm, float& log_mu_bin, float& log_nu_bin) {
  const float ms = (float)q.n, ns = (float)q.m;            // gmatcher.py:53 (m rows, n cols there)
  norm = -logf(ms + ns);
  log_mu_bin = logf(ns) + norm;                            // gmatcher.py:63
  log_nu_bin = logf(ms) + norm;                            // gmatcher.py:64
}

// The workspace of gims_sinkhorn_match and gims_sinkhorn_history (which leaves the selection buffers and the on-chip region unused): the OtDev
// table, the buffers of the streamed kernels problem by problem, then the region of the on-chip kernel (0 bytes when that path is off or does
// not fit).  recs == nullptr: sizing only (nothing of a problem but n and m is looked at); otherwise the records are filled, hist left null.
struct OtWs { int threads, cpt, maxn, maxm, maxG; OtR2Plan plan2; char* onchip; };
static OtWs ot_layout(const gims_ot_problem* pr, int np, int flags, WsLayout& L, OtDev* recs) {
  OtWs w{};
  ot_launch_shape(pr, np, w.threads, w.cpt, w.maxn, w.maxm);
  L.take<OtDev>(np);
  for (int i = 0; i < np; ++i) {
    const gims_ot_problem& q = pr[i];
    OtDev d{};
    d.G = ot_G(q.n, np, w.threads, w.cpt);
    w.maxG = d.G > w.maxG ? d.G : w.maxG;
    d.partial = L.take<float>((size_t)d.G * (q.m + 1));
    d.cbest_val = L.take<float>((size_t)d.G * q.m);
    d.cbest_idx = L.take<int>((size_t)d.G * q.m);
    d.max0 = L.take<float>(q.n);
    d.idx0 = L.take<int>(q.n);
    d.max1 = L.take<float>(q.m);
    d.idx1 = L.take<int>(q.m);
    if (!recs) continue;
    d.z = q.scores; d.ld = q.ld; d.n = q.n; d.m = q.m;
    d.u = q.uv; d.v = q.uv + q.n + 1; d.status = q.uv + q.n + 1 + q.m + 1;
    d.matches0 = q.matches0; d.matches1 = q.matches1; d.mscores0 = q.mscores0; d.mscores1 = q.mscores1;
    ot_fill_common(q, d.norm, d.log_mu_bin, d.log_nu_bin);
    recs[i] = d;
  }
  w.plan2 = ot_res2_choose(pr, np, 1, flags);      // (the plan of one iteration is the plan of any number: the size does not depend on the count)
  w.onchip = L.take<char>(w.plan2.bytes);
  return w;
}

// one iteration of the streamed kernels: the row sweep (instance by column quads per thread), then the column reduction, which also writes
// u and v into slot hist_slot of the history (-1: none)
static void ot_streamed_iteration(const OtWs& w, const OtDev* dp, int np, float alpha, int rescue, int hist_slot, hipStream_t s) {
  const dim3 gi(w.maxG, np), gc(cdiv(w.maxm + 1, 64), np), bt(w.threads);
  ot_instance(w.cpt, [&](auto inst) { using I = decltype(inst); hipLaunchKernelGGL((ot_iter_kernel<I::CPT, I::R>), gi, bt, 0, s, dp, alpha, rescue); });
  hipLaunchKernelGGL(ot_colreduce_kernel, gc, dim3(1024), 0, s, dp, hist_slot, rescue);
}

}  // namespace gims

extern "C" int gims_sinkhorn_plan(const gims_ot_problem* pr, int32_t np, int32_t iters, int32_t flags) {
  using namespace gims;
  if (!pr || np <= 0) return 0;
  const OtR2Plan p2 = ot_res2_choose(pr, np, iters, flags);
  return p2.ok ? p2.ngroups : 0;
}

extern "C" int gims_sinkhorn_match(const gims_ot_problem* pr, int32_t np, float alpha, int32_t iters, float match_threshold, void* work,
                                   size_t work_bytes, int32_t flags, void* stream) {
  using namespace gims;
  hipStream_t s = (hipStream_t)stream;
  GIMS_CHECK_ARG(pr && np > 0 && work, "gims_sinkhorn_match: null / empty arguments");
  GIMS_CHECK_ARG(iters >= 0, "gims_sinkhorn_match: iters < 0");
  for (int i = 0; i < np; ++i) {
    const gims_ot_problem& q = pr[i];
    GIMS_CHECK_ARG(q.n > 0 && q.m > 0 && q.scores && q.uv && q.matches0 && q.matches1 && q.mscores0 && q.mscores1,
                   "gims_sinkhorn_match: problem %d has empty shape or null pointer", i);
    GIMS_CHECK_ARG((q.ld % 4) == 0 && (((uintptr_t)q.scores) & 15) == 0, "gims_sinkhorn_match: scores must be 16-byte aligned with ld %% 4 == 0");
  }
  std::vector<OtDev> hprob(np);
  WsLayout L(work);
  const OtWs w = ot_layout(pr, np, flags, L, hprob.data());
  GIMS_CHECK_ARG(work_bytes >= L.bytes(), "gims_sinkhorn_match: workspace too small (%zu < %zu)", work_bytes, L.bytes());
  GIMS_CHECK_ARG(w.cpt <= 8, "gims_sinkhorn_match: m=%d too large (max 32768 columns: a thread of the streamed kernels owns at most 8 column quads)", w.maxm);
  const int threads = w.threads, cpt = w.cpt, maxn = w.maxn, maxm = w.maxm;
  {
    const int rc = upload_table(hprob.data(), sizeof(OtDev) * (size_t)np, work, s);   // by kernel arguments: no sync
    if (rc != GIMS_OK) return rc;
  }
  const OtDev* dp = (const OtDev*)work;
  const bool onchip = w.plan2.ok && iters >= 1;
  // the 2-D on-chip kernel forms the start potentials itself (GIMS_OT_R2_INIT=0: the separate sweep, for cross-checks)
  const int init_inside = onchip && env_int("GIMS_OT_R2_INIT", 1) ? 1 : 0;
  if (init_inside) hipLaunchKernelGGL(ot_status0_kernel, dim3(cdiv(np, 256)), dim3(256), 0, s, dp, np);
  else hipLaunchKernelGGL(ot_init_kernel, dim3(cdiv(maxn, 4), np), dim3(256), 0, s, dp, alpha, iters == 0 ? 1 : 0, 0);
  const dim3 gi(w.maxG, np);
  if (onchip) {     // whole iteration loop on chip, 2-D decomposition (sinkhorn2d.hip)
    std::vector<OtR2Host> h2(np);
    for (int i = 0; i < np; ++i) {
      const OtDev& d = hprob[i];
      h2[i] = OtR2Host{d.z, d.ld, d.n, d.m, d.u, d.v, d.status, d.norm, d.log_mu_bin, d.log_nu_bin};
    }
    const int rc = ot_res2_run(w.plan2, h2.data(), np, alpha, iters, init_inside, w.onchip, s);
    if (rc != GIMS_OK) return rc;
    const int force_fail = env_int("GIMS_OT_FORCE_FAIL", 0);       // test hook: pretend every on-chip solve timed out
    if (force_fail) hipLaunchKernelGGL(ot_poison_kernel, dim3(np), dim3(256), 0, s, dp);
    // Problems whose on-chip solve gave up (status 2) are re-solved here, before the selection kernels read u and v.
    OtRescueState* rs = ot_rescue_state();
    if (!rs) { set_error("gims_sinkhorn_match: no rescue state on this device"); return GIMS_EHIP; }
    const int mode = env_int("GIMS_OT_RESCUE", -1);                // 0: one-workgroup kernel only, 1: streamed always, default: streamed while marginal
    bool marginal;
    {
      std::lock_guard<std::mutex> lock(g_rescue_mu);
      rs->calls += 1;
      if (*rs->h_count != rs->seen) { rs->seen = *rs->h_count; rs->last_giveup_call = rs->calls; }
      marginal = mode == 1 || (mode != 0 && rs->calls - rs->last_giveup_call <= OT_MARGINAL_CALLS);
    }
    if (marginal) {
      hipLaunchKernelGGL(ot_rescue_begin_kernel, dim3(cdiv(np, 256)), dim3(256), 0, s, dp, np, rs->d_count);
      hipLaunchKernelGGL(ot_init_kernel, dim3(cdiv(maxn, 4), np), dim3(256), 0, s, dp, alpha, 0, 1);
      for (int it = 0; it < iters; ++it) ot_streamed_iteration(w, dp, np, alpha, 1, -1, s);
      hipLaunchKernelGGL(ot_rescue_end_kernel, dim3(cdiv(np, 256)), dim3(256), 0, s, dp, np);
    }
    // last resort (and the only rescue while the device is not marginal): an empty launch unless a status word still reads 2
    hipLaunchKernelGGL(ot_rescue_kernel, dim3(np), dim3(1024), 0, s, dp, alpha, iters, 0, rs->d_count);
    if (hipEventQuery(rs->ev) != hipErrorNotReady) {              // the previous read-back has landed: start the next one
      GIMS_HIP(hipMemcpyAsync((void*)rs->h_count, rs->d_count, sizeof(int), hipMemcpyDeviceToHost, s));
      GIMS_HIP(hipEventRecord(rs->ev, s));
    }
  } else {
    for (int it = 0; it < iters; ++it) ot_streamed_iteration(w, dp, np, alpha, 0, -1, s);
  }
  ot_instance(cpt, [&](auto inst) { using I = decltype(inst); hipLaunchKernelGGL((ot_select_kernel<I::CPT, I::RS>), gi, dim3(threads), 0, s, dp); });
  hipLaunchKernelGGL(ot_colbest_kernel, dim3(cdiv(maxm, 32), np), dim3(256), 0, s, dp);
  const int mx = maxn > maxm ? maxn : maxm;
  hipLaunchKernelGGL(ot_mutual_kernel, dim3(cdiv(mx, 256), np), dim3(256), 0, s, dp, match_threshold);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

extern "C" size_t gims_sinkhorn_workspace_bytes(const gims_ot_problem* pr, int32_t np) {
  using namespace gims;
  if (!pr || np <= 0) return 0;
  WsLayout L(nullptr);
  ot_layout(pr, np, 0, L, nullptr);
  return L.bytes();
}

extern "C" int64_t gims_sinkhorn_rescues(void) {
  using namespace gims;
  OtRescueState* rs = ot_rescue_state();
  int n = 0;
  if (!rs || hipDeviceSynchronize() != hipSuccess || hipMemcpy(&n, rs->d_count, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) {
    set_error("gims_sinkhorn_rescues: the counter of the current device could not be read");
    return -1;
  }
  return n;
}

extern "C" int gims_ot_matrix(const float* scores, int64_t ld, int32_t n, int32_t m, float alpha, const float* uv,
                              float* out, void* stream) {
  using namespace gims;
  GIMS_CHECK_ARG(scores && uv && out && n > 0 && m > 0, "gims_ot_matrix: bad arguments");
  hipLaunchKernelGGL(ot_matrix_kernel, dim3(cdiv(m + 1, 256), n + 1), dim3(256), 0, (hipStream_t)stream, scores, ld, n, m,
                     alpha, uv, out);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

extern "C" int gims_train_loss(const gims_loss_pair* dev_pairs, int32_t n_pairs, const int64_t* gt, int32_t n_gt, float alpha,
                               float pos_weight, float neg_weight, float* loss_vec, int32_t* tag, float* out3, void* stream) {
  using namespace gims;
  GIMS_CHECK_ARG(dev_pairs && n_pairs > 0 && n_pairs <= 1024 && out3 && n_gt >= 0 && (n_gt == 0 || (gt && loss_vec && tag)),
                 "gims_train_loss: bad arguments (1 <= n_pairs <= 1024)");
  if (n_gt > 0) hipLaunchKernelGGL(train_loss_gather_kernel, dim3(cdiv(n_gt, 256)), dim3(256), 0, (hipStream_t)stream, dev_pairs, n_pairs, gt, n_gt, alpha,
                                   loss_vec, tag);
  hipLaunchKernelGGL(train_loss_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, loss_vec, tag, n_gt, n_pairs, pos_weight, neg_weight, out3);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

// ---- recorded forward solve + backward sweep (forward_train gradients w.r.t. scores and bin_score)
extern "C" size_t gims_sinkhorn_history_floats(int32_t n, int32_t m, int32_t iters) {
  return (size_t)(iters + 1) * (size_t)(n + m + 2);
}

extern "C" int gims_sinkhorn_history(const gims_ot_problem* pr, int32_t np, float alpha, int32_t iters, float* const* h_hist, void* work,
                                     size_t work_bytes, void* stream) {
  using namespace gims;
  GIMS_CHECK_ARG(pr && np > 0 && work && h_hist && iters >= 1, "gims_sinkhorn_history: null / empty arguments");
  for (int i = 0; i < np; ++i) {
    const gims_ot_problem& q = pr[i];
    GIMS_CHECK_ARG(q.n > 0 && q.m > 0 && q.scores && q.uv && h_hist[i], "gims_sinkhorn_history: problem %d has empty shape or null pointer", i);
    GIMS_CHECK_ARG((q.ld % 4) == 0 && (((uintptr_t)q.scores) & 15) == 0, "gims_sinkhorn_history: scores must be 16-byte aligned with ld %% 4 == 0");
  }
  std::vector<OtDev> hprob(np);
  WsLayout L(work);
  const OtWs w = ot_layout(pr, np, 0, L, hprob.data());      // the layout of gims_sinkhorn_match: the caller sized the buffer with its query
  GIMS_CHECK_ARG(work_bytes >= L.bytes(), "gims_sinkhorn_history: workspace too small (%zu < %zu)", work_bytes, L.bytes());
  GIMS_CHECK_ARG(w.cpt <= 4, "gims_sinkhorn_history: m=%d too large (max 16384)", w.maxm);
  for (int i = 0; i < np; ++i) hprob[i].hist = h_hist[i];
  hipStream_t s = (hipStream_t)stream;
  const int rc = upload_table(hprob.data(), sizeof(OtDev) * (size_t)np, work, s);
  if (rc != GIMS_OK) return rc;
  const OtDev* dp = (const OtDev*)work;
  // (Round 5 measured the recorded solve on chip -- ot_res2_kernel writing u and v after every iteration, 3 launches instead of 2 x iters --
  // and took it out again: its potentials are consistent with the K it ROUNDED at the last derivation, the reverse sweep recomputes
  // exp(Z + u_k + v_k-1) afresh, and that 1e-5 inconsistency per iteration is amplified by the cancellation in d loss / d bin_score:
  // 7.9e-2 on the 2 x 2048 fixture against a bar of 2e-2; every other gradient was unaffected.)
  hipLaunchKernelGGL(ot_init_kernel, dim3(cdiv(w.maxn, 4), np), dim3(256), 0, s, dp, alpha, 0, 0);
  // the streamed kernels, one iteration at a time; the column reduction writes u, v of this iteration into the history itself
  for (int it = 0; it < iters; ++it) ot_streamed_iteration(w, dp, np, alpha, 0, it + 1, s);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

namespace gims {
// The workspace of gims_sinkhorn_backward: the OtBwd table, then per problem the sweep vectors and the low-rank sweep's gu_rec, gv_rec, P, Q, T.
// The low-rank buffers always have the capacity of OT_BWD_MAX_ITERS iterations (the workspace query does not know the iteration count; a
// shorter solve uses their front, a longer one falls back to the in-place sweep and leaves them alone).  recs == nullptr: sizing only.
constexpr int OT_BWD_MAX_ITERS = 128;
static void ot_bwd_layout(const gims_ot_problem* pr, int np, WsLayout& L, OtBwd* recs) {
  constexpr size_t cap = OT_BWD_MAX_ITERS;
  L.take<OtBwd>(np);
  for (int i = 0; i < np; ++i) {
    const size_t n1 = (size_t)pr[i].n + 1, m1 = (size_t)pr[i].m + 1, ldt = (m1 + 3) & ~(size_t)3;
    OtBwd b{};
    b.gu = L.take<float>(n1);
    b.gv = L.take<float>(m1);
    b.gv2 = L.take<float>(m1);
    b.colpart = L.take<float>((size_t)((pr[i].n + BW_ROWS) / BW_ROWS) * m1);
    b.gu_rec = L.take<float>((cap + 1) * n1);
    b.gv_rec = L.take<float>((cap + 1) * m1);
    b.fp = L.take<float>(n1 * 2 * cap);
    b.fq = L.take<float>(m1 * 2 * cap);
    b.tmat = L.take<float>(n1 * ldt);
    b.ldt = (int64_t)ldt;
    if (recs) recs[i] = b;
  }
}
}  // namespace gims

extern "C" size_t gims_sinkhorn_backward_workspace_bytes(const gims_ot_problem* pr, int32_t np) {
  using namespace gims;
  if (!pr || np <= 0) return 0;
  WsLayout L(nullptr);
  ot_bwd_layout(pr, np, L, nullptr);
  return L.bytes();
}

extern "C" int gims_sinkhorn_backward(const gims_ot_problem* pr, int32_t np, float alpha, int32_t iters, const float* const* h_hist,
                                      float* const* h_dz, float* dalpha /* device [np] */, void* work, size_t work_bytes, void* stream) {
  using namespace gims;
  GIMS_CHECK_ARG(pr && np > 0 && h_hist && h_dz && dalpha && work && iters >= 1, "gims_sinkhorn_backward: null / empty arguments");
  for (int i = 0; i < np; ++i)
    GIMS_CHECK_ARG(pr[i].n > 0 && pr[i].m > 0 && pr[i].scores && h_hist[i] && h_dz[i], "gims_sinkhorn_backward: problem %d has empty shape or null pointer", i);
  std::vector<OtBwd> hp(np);
  WsLayout L(work);
  ot_bwd_layout(pr, np, L, hp.data());
  GIMS_CHECK_ARG(work_bytes >= L.bytes(), "gims_sinkhorn_backward: workspace too small (%zu < %zu)", work_bytes, L.bytes());
  hipStream_t s = (hipStream_t)stream;
  int maxn = 0, maxm = 0;
  for (int i = 0; i < np; ++i) {
    const gims_ot_problem& q = pr[i];
    OtBwd& b = hp[i];
    b.z = q.scores; b.ld = q.ld; b.n = q.n; b.m = q.m;
    b.hist = h_hist[i]; b.hstride = q.n + q.m + 2;
    b.dz = h_dz[i];
    b.iters = iters;
    b.dalpha = dalpha + i;
    ot_fill_common(q, b.norm, b.log_mu_bin, b.log_nu_bin);
    maxn = q.n > maxn ? q.n : maxn; maxm = q.m > maxm ? q.m : maxm;
  }
  const int rc = upload_table(hp.data(), sizeof(OtBwd) * (size_t)np, work, s);
  if (rc != GIMS_OK) return rc;
  const OtBwd* dp = (const OtBwd*)work;
  const int mx = maxn > maxm ? maxn : maxm;
  if (iters <= OT_BWD_MAX_ITERS && cdiv(maxm + 1, 512) <= 9 && !env_int("GIMS_OT_BWD_INPLACE", 0)) {
    // low-rank form: reductions only per iteration, one K = 2 iters product at the end
    const dim3 gs(cdiv(maxn + 1, BW_ROWS), np), gc(cdiv(maxm + 1, 16), np);
    const int cpt = cdiv(maxm + 1, 512);
    hipLaunchKernelGGL(ot_bwd_fused_kernel<true>, gs, dim3(256), 0, s, dp, alpha, 0, 0);
    hipLaunchKernelGGL(ot_bwd_colsum_rec_kernel, gc, dim3(1024), 0, s, dp, 1.f, iters);
    for (int k = iters; k >= 1; --k) {
      const int first = k == iters ? 1 : 0;
      ot_bwd_instance(cpt, [&](auto n) { hipLaunchKernelGGL((ot_bwd_reduce_kernel<decltype(n)::value>), gs, dim3(512), 0, s, dp, alpha, k, first); });
      hipLaunchKernelGGL(ot_bwd_colsum_rec_kernel, gc, dim3(1024), 0, s, dp, -1.f, k - 1);
    }
    const int64_t fmax = (int64_t)(maxn + 1 + maxm + 1) * iters;
    hipLaunchKernelGGL(ot_bwd_shift_kernel, dim3(cdiv(mx + 1, 256), np), dim3(256), 0, s, dp);          // (gu, gv2 are free after the loop)
    hipLaunchKernelGGL(ot_bwd_factor_kernel, dim3((unsigned)cdiv(fmax, 256), np), dim3(256), 0, s, dp);
    GIMS_LAUNCH_CHECK();
    for (int i = 0; i < np; ++i) {
      gims_gemm g{};
      g.a = hp[i].fp; g.b = hp[i].fq; g.c = hp[i].tmat;
      g.lda = 2 * iters; g.ldb = 2 * iters; g.ldc = hp[i].ldt;
      g.m = hp[i].n + 1; g.n = hp[i].m + 1; g.k = 2 * iters; g.batch = 1;
      g.alpha = 1.f; g.beta = 0.f; g.act = GIMS_ACT_NONE; g.precision = GIMS_PREC_BF16X6;
      const int rcg = gims_gemm_f32(&g, stream);
      if (rcg != GIMS_OK) return rcg;
    }
    hipLaunchKernelGGL(ot_bwd_combine_kernel, dim3(cdiv(maxm + 1, 256), maxn + 1, np), dim3(256), 0, s, dp, alpha);
  } else {
    const dim3 gs(cdiv(maxn + 1, BW_ROWS), np), gc(cdiv(maxm + 1, 32), np);
    const int cpt = cdiv(maxm + 1, 512);
    hipLaunchKernelGGL(ot_bwd_fused_kernel<true>, gs, dim3(256), 0, s, dp, alpha, 0, 0);
    hipLaunchKernelGGL(ot_bwd_colsum_kernel, gc, dim3(256), 0, s, dp, 1.f);
    for (int k = iters; k >= 1; --k) {
      const int first = k == iters ? 1 : 0;
      if (cpt <= 9) ot_bwd_instance(cpt, [&](auto n) { hipLaunchKernelGGL((ot_bwd_fused_reg_kernel<decltype(n)::value>), gs, dim3(512), 0, s, dp, alpha, k, first); });
      else hipLaunchKernelGGL((ot_bwd_fused_kernel<false>), gs, dim3(256), 0, s, dp, alpha, k, first);
      hipLaunchKernelGGL(ot_bwd_colsum_kernel, gc, dim3(256), 0, s, dp, -1.f);
    }
  }
  hipLaunchKernelGGL(ot_bwd_alpha_kernel, dim3(np), dim3(256), 0, s, dp);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

extern "C" int gims_train_loss_grad(const gims_loss_pair* dev_pairs, int32_t n_pairs, const int64_t* gt, int32_t n_gt, float alpha, const int32_t* tag,
                                    float pos_weight, float neg_weight, float* const* dev_dz_ptrs, void* stream) {
  using namespace gims;
  GIMS_CHECK_ARG(dev_pairs && n_pairs > 0 && dev_dz_ptrs && n_gt >= 0 && (n_gt == 0 || (gt && tag)), "gims_train_loss_grad: bad arguments");
  if (n_gt > 0)
    hipLaunchKernelGGL(train_loss_grad_kernel, dim3(cdiv(n_gt, 256)), dim3(256), 0, (hipStream_t)stream, dev_pairs, n_pairs, gt, n_gt, alpha, tag, pos_weight,
                       neg_weight, dev_dz_ptrs);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}
