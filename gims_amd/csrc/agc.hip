// Adaptive graph construction on the GPU -- models/agc.py:682-709 (live subset) for one image.
//
//   K1 cosine similarity  S = Dn Dn^T                      (agc.py:382-391)
//   K2 exact percentile threshold over the strict upper triangle (agc.py:367-380, 439-440)
//        round 4: APPROXIMATE everywhere, EXACT only where it decides.  The N x N matrix is formed once in IEEE half on the matrix cores
//        (one MFMA pass, |error| <= AGC_EPS by Cauchy-Schwarz on unit rows); a 12-bit histogram of it brackets the k-th value; only the
//        entries inside a rigorous error band around that bracket (~0.3 %) and the radius candidates (~19 k per image) are re-evaluated
//        exactly (f32 operands, float64 accumulation in a fixed order), and the exact k-th value is selected among the band entries
//        with the exact count below the band.  (The flow of rounds 1-3 -- all N^2 similarities at f32-GEMM accuracy, radix select over the
//        whole matrix -- left the library in round 5; the reference goldens and the CPU restatement in the tests are the cross-check.)
//   K3 radius candidates (float64, inclusive) AND sim >= thr  (agc.py:435-447) -> adjacency BIT MATRIX
//   K4 connect_isolated_nodes, sequential semantics           (agc.py:476-495)
//   K5 connected components (min-label union-find in LDS) + small-component removal (agc.py:497-516)
//   K6 fast_connect_components, one round                     (agc.py:518-565)
//   K7 sorted relabel + bidirectional CSR                     (dgl.from_networkx, agc.py:704)
//
// Everything here is integer / byte / latency-bound work (N <= 32768 nodes, a few 10^4 edges) except K1/K2,
// which stream the N x N similarity matrix (HBM-bound).  The adjacency lives in an N x N bit matrix so that
// the sequential fix-ups only flip bits and the CSR falls out of popcounts in ascending neighbour order.
#include "common.h"

#include <cstring>
#include <vector>

namespace gims {

// Largest image: 32768 keypoints (the reference has no limit -- agc.py:413-449 is NumPy -- and publishes runs with up to 21 163 kept
// keypoints, tools/files/rgbd1/record.txt:635).  What bounds it here: a pair of node ids is packed into one 32-bit word (i << 16 | j), the
// sequential isolated-node walk keeps its ordered list in LDS (4 bytes per node + a bit: 135 KB of the 160 KB at 32768), and the band list
// reserves one word per pair of the strict upper triangle (2 GB per image at 32768).  Up to AGC_CC_LDS_N nodes the component search runs in LDS,
// above it in global memory (slower, same labels).
constexpr int AGC_MAX_N = 32768;
constexpr int AGC_PK_SHIFT = 16;
constexpr uint32_t AGC_PK_MASK = 0xffffu;
constexpr int AGC_CC_LDS_N = 16384;
constexpr int AGC_NB = 16384;  // hash buckets of the keypoint grid

struct AgcWs {
  float* dnf;           // [n][d] normalised descriptors in f32: operands of the exact evaluations
  uint16_t* dn16;       // [n][d] the same rounded to IEEE half: operands of the approximate similarity GEMM
  uint16_t* S16;        // [n][lds16] approximate similarities in half; tiles that touch the upper triangle are valid
  uint32_t* list;       // band entries: packed (i << 16 | j), overwritten in place by the order-preserving keys of their exact values
  uint32_t* band;       // [4]: first and last 12-bit bin of the band, pad
  uint32_t* clist;      // radius candidates, packed (i << 16 | j) with i < j; ckey: the order-preserving keys of their exact similarities
  uint32_t* ckey;
  uint32_t list_cap, clist_cap; int lds16;
  int32_t* cellptr;     // [AGC_NB + 1] bucket offsets of the keypoint grid (radius search); cellidx [n]: point ids sorted by bucket
  int32_t* cellidx;
  uint64_t* bits;       // [n][nw]
  uint32_t* hist;       // [4096] histogram of the current radix digit
  uint32_t* sel;        // [4]: prefix, k_lo, k_hi, pad
  int32_t* deg;         // [n]
  int32_t* nn;          // [n]
  int32_t* label;       // [n]
  int32_t* alive;       // [n]
  int32_t* newid;       // [n]
  int32_t* crank;       // [n] component rank of a root (ascending root id), -1 otherwise
  int32_t* coff;        // [n+1]
  int32_t* members;     // [n]
  int32_t* nnc;         // [n]
  int32_t* link;        // [n][2]
  double* cent;         // [n][2]
  int32_t* ptr0;        // [n+1] CSR of the pre-removal graph (original ids)
  int32_t* idx0;        // [cap]
  int32_t* esrc;        // [cap] source row of every entry of idx0 (the component search walks the edge list, not the rows)
  int32_t* counters;    // [16] scratch counters: 0 coarse directed edges, 1 components, 2 pre-removal directed edges
  int32_t* coff2;       // [n+1] component offsets (scan of sizes)
  int32_t* degk;        // [n] degree by kept id
  // per-image inputs / outputs (caller-owned)
  const float* kpts; const float* desc; int64_t ldd;
  int32_t* kept; int32_t* indptr; int32_t* indices; int32_t* info;
  int64_t krank;        // percentile rank k (agc.py:378-379)
  int n, d, nw, cap, max_edges_dir;
  // the image's own graph parameters (gims_agc_params): min_size of the component removal, squared radius, inverse cell side of the keypoint grid
  int min_size;
  double r2, inv_side;
};

// per-image reset of the select state and counters (descriptors are already in device memory, see upload_table)
__global__ void agc_init_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  if (threadIdx.x == 0) {
    w.sel[0] = 0u; w.sel[1] = (uint32_t)(w.krank & 0xffffffffll); w.sel[2] = (uint32_t)(w.krank >> 32); w.sel[3] = 0u;
    for (int i = 0; i < 8; ++i) w.info[i] = 0;
    for (int i = 0; i < 16; ++i) w.counters[i] = 0;
    for (int i = 0; i < 4; ++i) w.band[i] = 0u;
  }
  for (int i = threadIdx.x; i < 4096; i += blockDim.x) w.hist[i] = 0u;
}

// ---------------------------------------------------------------------------------------------- K1 prologue
__global__ __launch_bounds__(256) void agc_normalize_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  const int n = w.n, d = w.d;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= n) return;
  const float* x = w.desc + (int64_t)row * w.ldd;
  float s = 0.f;
  for (int j = lane; j < d; j += 64) s = fmaf(x[j], x[j], s);
  s = wave_sum(s);
  const float nrm = fmaxf(sqrtf(s), 1e-12f);   // F.normalize: x / max(||x||, eps)
  // the f32 quotient (exact evaluations) and its rounding to half (approximate GEMM)
  // ... and the 2-norm of the row's rounding error (kept per row in deg, as float bits): the measured half of the error bound of the approximate
  // similarities (agc_window_kernel, agc_band_kernel).  A half that is subnormal counts as flushed to zero (some matrix cores do): the bound
  // holds either way.
  float e2 = 0.f;
  for (int j = lane; j < d; j += 64) {
    const float v = x[j] / nrm;
    const uint16_t hb = (uint16_t)(pack_h2_sat(v, 0.f) & 0xffffu);
    w.dnf[(int64_t)row * d + j] = v;
    w.dn16[(int64_t)row * d + j] = hb;
    const float back = (float)__builtin_bit_cast(_Float16, hb);
    float e = fabsf(v - back);
    if ((hb & 0x7c00u) == 0u) e = fmaxf(e, fabsf(v));
    e2 = fmaf(e, e, e2);
  }
  e2 = wave_sum(e2);
  if (lane == 0) w.deg[row] = (int32_t)__float_as_uint(sqrtf(e2) * 1.0001f);      // (deg is free until the adjacency exists; the window / band kernels take the maximum)
}

// ---------------------------------------------------------------------------------------------- K2 radix select
// Exact k-th smallest among the listed keys (the exact similarities of the band / window entries) by radix select on order-preserving keys
// in THREE digits (12 + 12 + 8 bits): one histogram pass over the list per digit, restricted to the keys that share the prefix selected so far.
__global__ __launch_bounds__(256) void agc_hist_kernel(const AgcWs* __restrict__ ws, int shift, int bits) {
  const AgcWs& w = ws[blockIdx.y];
  __shared__ uint32_t h[4096];
  const int nb = 1 << bits;
  for (int i = threadIdx.x; i < nb; i += 256) h[i] = 0;
  __syncthreads();
  const uint32_t prefix = w.sel[0];
  const uint32_t himask = shift + bits >= 32 ? 0u : (0xffffffffu << (shift + bits));
  const uint32_t dmask = (uint32_t)nb - 1u;
  const uint32_t nlist = w.sel[3] < w.list_cap ? w.sel[3] : w.list_cap;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nlist; i += gridDim.x * 256) {
    const uint32_t k = w.list[i];
    if ((k & himask) == (prefix & himask)) atomicAdd(&h[(k >> shift) & dmask], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += 256)
    if (h[i]) atomicAdd(&w.hist[i], h[i]);
}

// the bin holding rank k: parallel inclusive scan of the counts (thread t owns nb / 256 consecutive bins)
__global__ __launch_bounds__(256) void agc_pick_kernel(const AgcWs* __restrict__ ws, int shift, int bits) {
  const AgcWs& w = ws[blockIdx.y];
  __shared__ uint64_t wsum[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nb = 1 << bits, per = nb >> 8;             // bits >= 8
  uint64_t v = 0;
  for (int q = 0; q < per; ++q) v += w.hist[t * per + q];
  uint64_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  for (int q = 0; q < wave; ++q) incl += wsum[q];
  const uint64_t k = (uint64_t)w.sel[1] | ((uint64_t)w.sel[2] << 32);
  uint64_t excl = incl - v;
  // first bin b < nb - 1 with cum(b) + h[b] > k, else nb - 1 (the reference walk): the owning thread walks its own bins
  const bool mine = t < 255 ? (excl <= k && k < incl) : excl <= k;
  __syncthreads();                      // every thread has read sel[1..2]
  if (mine) {
    int b = t * per;
    for (int q = 0; q < per; ++q, ++b) {
      const uint64_t c = w.hist[b];
      if (k < excl + c || b == nb - 1) break;
      excl += c;
    }
    const uint64_t r = k - excl;
    w.sel[0] |= ((uint32_t)b) << shift;
    w.sel[1] = (uint32_t)r;
    w.sel[2] = (uint32_t)(r >> 32);
  }
  __syncthreads();
  for (int q = 0; q < per; ++q) w.hist[t * per + q] = 0;
  for (int i = nb + t; i < 4096; i += 256) w.hist[i] = 0;
}

// ---------------------------------------------------------------------------------------------- K1/K2, band-limited flow (round 4)
// |S - S16| <= AGC_EPS for unit rows: operands rounded to half (unit roundoff 2^-11 each: <= 2 * 2^-11 + 2^-22 by Cauchy-Schwarz;
// elements below 2^-14 go subnormal at an absolute 2^-25, < 2^-21 over 256 of them), products exact in f32, 256 f32 additions
// (< 2e-5), result rounded to half (<= 2^-11 for |S| <= 2).  0.000977 + 0.00002 + 0.00049 < 0.0016.
// Placement of per-image work that re-reads the image's rows (similarity tiles, gathered exact dot products): block b runs on XCD b % 8
// (observed; a speed assumption only), and the eight XCDs take the (image, part) units q = xcd, xcd + 8, ... in turn, with
// nparts = 8 / gcd(n_images, 8) parts per image -- an image's rows are fetched into ONE XCD's 4-MB L2 (16 images: two per XCD, one after the
// other) instead of into all eight.  Grids of these kernels are 1-D multiples of 8.
__device__ __forceinline__ int agc_nparts(int n_images) {
  int g = n_images & -n_images;
  g = g > 8 ? 8 : g;
  return 8 / g;
}
typedef _Float16 agc_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 agc_h2 __attribute__((ext_vector_type(2)));
typedef float agc_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t h16_key(uint16_t h) { return (h & 0x8000u) ? (uint32_t)(uint16_t)~h : (uint32_t)(h | 0x8000u); }
__device__ __forceinline__ float h16_val(uint32_t key) {      // inverse of h16_key, as f32
  const uint16_t h = (key & 0x8000u) ? (uint16_t)(key & 0x7fffu) : (uint16_t)~key;
  return (float)__builtin_bit_cast(_Float16, h);
}

// The exact evaluation of one similarity (both the threshold and the edge tests go through it: decisions are self-consistent).
// dot(a, b) of two f32 rows in FLOAT64, fixed order: partial q (0..7) takes the 4-element pieces q, q + 8, q + 16 ... in ascending
// order; the partials are combined as ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)) and the sum is rounded to f32 once.  Eight lanes per pair
// (lane q = partial q, xor-butterfly: every lane of the group ends with the same bits); d % 32 == 0.
__device__ __forceinline__ float agc_exact_sim8(const float* __restrict__ a, const float* __restrict__ b, int d, int q) {
  double acc = 0.0;
  if (d == 256) {                 // the descriptor size of the path: all sixteen 16-byte loads of the lane in flight before the first fma
    float4 x[8], y[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) { x[t] = *(const float4*)(a + 4 * q + 32 * t); y[t] = *(const float4*)(b + 4 * q + 32 * t); }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      acc = fma((double)x[t].x, (double)y[t].x, acc);
      acc = fma((double)x[t].y, (double)y[t].y, acc);
      acc = fma((double)x[t].z, (double)y[t].z, acc);
      acc = fma((double)x[t].w, (double)y[t].w, acc);
    }
  } else {
    for (int k = 4 * q; k < d; k += 32) {
      const float4 x = *(const float4*)(a + k), y = *(const float4*)(b + k);
      acc = fma((double)x.x, (double)y.x, acc);
      acc = fma((double)x.y, (double)y.y, acc);
      acc = fma((double)x.z, (double)y.z, acc);
      acc = fma((double)x.w, (double)y.w, acc);
    }
  }
  acc += __shfl_xor(acc, 1, 64);
  acc += __shfl_xor(acc, 2, 64);
  acc += __shfl_xor(acc, 4, 64);
  return (float)acc;
}

// Robust flow.  S16 = Dn16 Dn16^T, 128 x 128 tiles that touch the upper triangle, one MFMA pass on v_mfma_f32_32x32x16_f16.  4 waves (2 x 2),
// 64 x 64 per wave; K in chunks of 128 (operands by LDS-DMA: 2 x 32 KB, 16-byte chunks XOR-swizzled with row & 15 on the source side); two
// workgroups per CU take turns loading and multiplying.  The tile leaves in half as whole 256-byte row pieces through an LDS transpose and the
// strict upper triangle is histogrammed on the 12-bit half key.
constexpr int S16_T = 128, S16_KC = 128, S16_EP = 136;        // tile, K chunk, epilogue pitch (halves)
constexpr int S16_LDS_BYTES = 2 * S16_T * S16_KC * 2 + 4096 * 4;    // operand chunks (64 KB) + the workgroup's histogram / staging buffer (16 KB): two workgroups per CU
__global__ __launch_bounds__(256, 2) void agc_sim16_kernel(const AgcWs* __restrict__ ws, int n_images) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];        // A chunk | B chunk (epilogue: [128][136] halves) | histogram
  uint16_t* As = lds;
  uint16_t* Bs = lds + S16_T * S16_KC;
  uint32_t* hist = (uint32_t*)(lds + 2 * S16_T * S16_KC);
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wi = wave >> 1, wj = wave & 1, li = lane & 31, lh = lane >> 5;
  for (int i = t; i < 4096; i += 256) hist[i] = 0u;
  const int nparts = agc_nparts(n_images);
  for (int q = blockIdx.x & 7; q < n_images * nparts; q += 8) {
  const AgcWs& w = ws[q / nparts];
  const int n = w.n, d = w.d, T = (n + S16_T - 1) / S16_T;
  const int ntiles = T * (T + 1) / 2;
  // persistent over its share of the image's tiles: what this workgroup found for the image is folded into the image's ONCE
  for (int tile = q % nparts + nparts * (int)(blockIdx.x >> 3); tile < ntiles; tile += nparts * (int)(gridDim.x >> 3)) {
  // linear index -> (ti <= tj): rows of the upper triangle hold T, T - 1, ... tiles
  int rem = tile, ti = 0;
  while (rem >= T - ti) { rem -= T - ti; ++ti; }
  const int tj = ti + rem;
  const int i0 = ti * S16_T, j0 = tj * S16_T;
  f32x16 acc[2][2];        // [jb][ib]: lane holds S[i = wi*64 + ib*32 + li][j = wj*64 + jb*32 + (r&3) + 8*(r>>2) + 4*lh]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  __syncthreads();                                             // (the previous tile's epilogue is done with the operand buffers)
  for (int k0 = 0; k0 < d; k0 += S16_KC) {
    const int kc = d - k0 < S16_KC ? d - k0 : S16_KC;       // multiple of 32
    const int cpr = kc / 8;                                  // 16-byte chunks per row of this K chunk (<= 16)
    // 64 pieces of 1 KiB (A rows then B rows, 4 rows of 256 bytes per piece), 16 per wave; short chunks leave the row tails untouched
#pragma unroll 4
    for (int pc = 0; pc < 16; ++pc) {
      const int piece = wave * 16 + pc;                      // wave-uniform
      const bool is_b = piece >= 32;
      const int row = 4 * (piece & 31) + (lane >> 4), pos = lane & 15, ch = pos ^ (row & 15);
      int gr = (is_b ? j0 : i0) + row;
      gr = gr < n ? gr : n - 1;
      const uint16_t* src = w.dn16 + (int64_t)gr * d + k0 + 8 * (ch < cpr ? ch : 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)((is_b ? Bs : As) + (piece & 31) * 512), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int s = 0; s < kc / 16; ++s) {
      bf16x8 af[2], bf[2];
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) {
        const int row = wi * 64 + ib * 32 + li;
        af[ib] = *(const bf16x8*)(As + row * S16_KC + (((2 * s + lh) ^ (row & 15)) << 3));
      }
#pragma unroll
      for (int jb = 0; jb < 2; ++jb) {
        const int row = wj * 64 + jb * 32 + li;
        bf[jb] = *(const bf16x8*)(Bs + row * S16_KC + (((2 * s + lh) ^ (row & 15)) << 3));
      }
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
          acc[jb][ib] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(agc_h8, bf[jb]), __builtin_bit_cast(agc_h8, af[ib]), acc[jb][ib], 0, 0, 0);
    }
    __syncthreads();
  }
  // ---- epilogue: half values -> LDS [row i][col j] (pitch 136 halves), then whole row pieces out; the strict upper triangle is histogrammed
  uint16_t* es = lds;
#pragma unroll
  for (int jb = 0; jb < 2; ++jb)
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = wi * 64 + ib * 32 + li, j = wj * 64 + jb * 32 + 8 * g + 4 * lh;
        const uint32_t lo = pack_h2_sat(acc[jb][ib][4 * g], acc[jb][ib][4 * g + 1]), hi = pack_h2_sat(acc[jb][ib][4 * g + 2], acc[jb][ib][4 * g + 3]);
        *(uint2*)(es + i * S16_EP + j) = make_uint2(lo, hi);
        const int gi = i0 + i, gj = j0 + j;
        if (gi < n) {
          if (gj + 0 > gi && gj + 0 < n) atomicAdd(&hist[h16_key((uint16_t)(lo & 0xffffu)) >> 4], 1u);
          if (gj + 1 > gi && gj + 1 < n) atomicAdd(&hist[h16_key((uint16_t)(lo >> 16)) >> 4], 1u);
          if (gj + 2 > gi && gj + 2 < n) atomicAdd(&hist[h16_key((uint16_t)(hi & 0xffffu)) >> 4], 1u);
          if (gj + 3 > gi && gj + 3 < n) atomicAdd(&hist[h16_key((uint16_t)(hi >> 16)) >> 4], 1u);
        }
      }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int i = 16 * it + (t >> 4), c = t & 15;            // 16 lanes per row: 16 x 16 bytes = the row's 128 columns
    const int gi = i0 + i, gj = j0 + 8 * c;
    if (gi < n && gj < w.lds16) *(uint4*)(w.S16 + (int64_t)gi * w.lds16 + gj) = *(const uint4*)(es + i * S16_EP + 8 * c);
  }
  }
  __syncthreads();
  for (int i = t; i < 4096; i += 256)
    if (hist[i]) { atomicAdd(&w.hist[i], hist[i]); hist[i] = 0u; }
  }
}

// Window flow: the approximate similarities (half operands, f32 MFMA accumulation) are looked at, never stored.  A workgroup of 4 waves (2 x 2,
// 64 x 64 per wave) takes a unit = up to eight (sample pass: three) consecutive 128 x 128 tiles of one tile row.  Every wave keeps the MFMA fragments of ITS 64
// rows for the whole K in REGISTERS for the unit (128 VGPRs): with both operands read from LDS a 64 x 64 wave tile needs exactly the LDS
// bandwidth the CU has (1 KB per MFMA), and the column ring's DMA writes and the epilogue come on top; with the rows in registers it is half.
// Only the column operand goes through LDS: K chunks of 64 in a two-buffer ring by LDS-DMA, the next chunk in flight under the MFMAs of the
// current one.  48 KB of LDS and <= 256 VGPRs: two independent workgroups per CU, so one's epilogue runs under the other's MFMAs.  Units are
// handed out by a per-image counter; an image's units run on ONE XCD (agc_nparts).  d % 64 == 0, d <= 256.
//   SIM_SAMPLE   the rows i % stride == 0 against all columns: histogram of the strict upper triangle on 4096 LINEAR bins over [-1, 1) (stride 1 =
//                every pair: small images);
//   SIM_COLLECT  every pair: entries below the window [band[0], band[1]] are counted (counters[5]), entries inside it are appended to the list as
//                (i << 16 | j) (LDS-staged: one global reservation per flush).
constexpr int SIM_SAMPLE = 1, SIM_COLLECT = 2, SIM_STAGE = 4096;
constexpr int AGC_SAMPLE_STRIDE = 8, AGC_SAMPLE_MIN_N = 1536;      // images of at most that many rows are "sampled" in full: their window is rigorous
__host__ __device__ __forceinline__ int agc_sample_stride(int n) { return n > AGC_SAMPLE_MIN_N ? AGC_SAMPLE_STRIDE : 1; }
__device__ __forceinline__ int agc_linear_bin(float v) {
  int b = (int)((v + 1.f) * 2048.f);
  b = b < 0 ? 0 : (b > 4095 ? 4095 : b);
  return v == v ? b : 4095;
}
// LDS accesses of the epilogues as raw instructions: in front of every LDS access it can see, the compiler waits for ALL outstanding LDS-DMA
// loads (vmcnt(0): it cannot tell that the column ring and the staging buffer do not overlap) -- that is the next tile's first chunk, in flight
// on purpose -- and it turns an atomicAdd of per-lane counts on one address into a scalar loop over the lanes.
__device__ __forceinline__ uint32_t lds_off(const void* p) { return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p; }
__device__ __forceinline__ uint32_t lds_add_rtn_raw(uint32_t off, uint32_t v) {
  uint32_t r;
  asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r) : "v"(off), "v"(v) : "memory");
  return r;
}
__device__ __forceinline__ void lds_add_raw(uint32_t off, uint32_t v) { asm volatile("ds_add_u32 %0, %1" ::"v"(off), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_write_raw(uint32_t off, uint32_t v) { asm volatile("ds_write_b32 %0, %1" ::"v"(off), "v"(v) : "memory"); }
__device__ __forceinline__ uint32_t lds_read_raw(uint32_t off) {
  uint32_t r;
  asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r) : "v"(off) : "memory");
  return r;
}
constexpr int SW_T = 128, SW_KC = 64, SW_KMAX = 256;
// tiles per unit: loading a unit's row fragments costs about one tile's time (205 us per collect pass at one tile per unit, 120 at eight); the
// sample pass has few tile rows and wants more, shorter units
template <int MODE> constexpr int sw_seg() { return MODE == 1 ? 3 : 8; }
constexpr int SW_RING = 3;                                                 // column chunks in LDS: one under the MFMAs, two in flight (an L2 round trip is longer than a chunk's MFMAs)
constexpr int SW_LDS_BYTES = SW_RING * SW_T * SW_KC * 2 + 4096 * 4;     // column ring 3 x 16 KB + histogram / staging 16 KB
template <int MODE>
__global__ __launch_bounds__(256, 2) void agc_simw_kernel(const AgcWs* __restrict__ ws, int n_images) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  uint16_t* Bs = lds;                                  // SW_RING x [128][64] halves, 16-byte chunks at position chunk ^ ((row >> 1) & 7)
  uint32_t* hist = (uint32_t*)(lds + SW_RING * SW_T * SW_KC);
  __shared__ int s_unit;
  __shared__ uint32_t nst, gbase;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wi = wave >> 1, wj = wave & 1, li = lane & 31, lh = lane >> 5;
  const uint32_t hist_off = lds_off(hist), nst_off = lds_off(&nst);
  if (MODE == SIM_SAMPLE)
    for (int i = t; i < 4096; i += 256) hist[i] = 0u;
  if (t == 0) nst = 0u;
  const int nparts = agc_nparts(n_images);
  for (int q = blockIdx.x & 7; q < n_images * nparts; q += 8) {
    const AgcWs& w = ws[q / nparts];
    const int n = w.n, d = w.d, T = (n + 127) / 128, kpc = d / SW_KC;
    const int stride = MODE == SIM_SAMPLE ? agc_sample_stride(n) : 1;
    int nunits = 0;                                     // tile row ti holds the tiles stride * ti .. T - 1, in segments of sw_seg<MODE>()
    for (int ti = 0; T - stride * ti > 0; ++ti) nunits += (T - stride * ti + sw_seg<MODE>() - 1) / sw_seg<MODE>();
    // window [band[0], band[1]] as centre and squared half width (an empty or NaN window lists next to nothing: agc_finish_kernel reports the
    // miss; what is tested is |v - centre|^2 <= half^2 in f32, a few ulps off the interval -- the verification's slack is a hundred times that)
    agc_f2 vC2 = {0.f, 0.f}, hsq2 = {0.f, 0.f};
    if (MODE == SIM_COLLECT) {
      const float vL = __uint_as_float(w.band[0]), vU = __uint_as_float(w.band[1]), hw = 0.5f * (vU - vL), vC = 0.5f * (vL + vU);
      vC2 = agc_f2{vC, vC};
      hsq2 = hw >= 0.f ? agc_f2{hw * hw, hw * hw} : agc_f2{-1.f, -1.f};
    }
    uint32_t below = 0u;
    auto flush = [&]() __attribute__((always_inline)) {        // (called by the whole workgroup)
      __syncthreads();
      const uint32_t cnt = nst < (uint32_t)SIM_STAGE ? nst : (uint32_t)SIM_STAGE;
      if (t == 0) gbase = cnt ? atomicAdd(&w.sel[3], cnt) : 0u;
      __syncthreads();
      const uint32_t base = gbase;
      for (uint32_t i = t; i < cnt; i += 256)
        if (base + i < w.list_cap) w.list[base + i] = hist[i];
      __syncthreads();
      if (t == 0) nst = 0u;
      __syncthreads();
    };
    while (true) {
      __syncthreads();                                  // (the previous unit is done with s_unit)
      if (t == 0) s_unit = atomicAdd(&w.counters[MODE == SIM_SAMPLE ? 8 : 9], 1);
      __syncthreads();
      int rem = s_unit;
      if (rem >= nunits) break;
      int ti = 0, m_row = 0;
      for (;; ++ti) {
        m_row = T - stride * ti;
        const int segs = (m_row + sw_seg<MODE>() - 1) / sw_seg<MODE>();
        if (rem < segs) break;
        rem -= segs;
      }
      const int t0 = rem * sw_seg<MODE>(), ntl = m_row - t0 < sw_seg<MODE>() ? m_row - t0 : sw_seg<MODE>();
      const int i0 = ti * SW_T, jbase = (stride * ti + t0) * SW_T;
      // column chunk (tile tl, K chunk kc) -> ring buffer: 16 pieces of 1 KiB (8 rows of 128 bytes), 4 per wave
      auto issue_b = [&](int tl, int kc, int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int pc = 0; pc < 4; ++pc) {
          const int piece = wave * 4 + pc;
          const int row = 8 * piece + (lane >> 3), ch = (lane & 7) ^ ((row >> 1) & 7);
          int gr = jbase + tl * SW_T + row;
          gr = gr < n ? gr : n - 1;
          const uint16_t* src = w.dn16 + (int64_t)gr * d + kc * SW_KC + 8 * ch;
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                           (__attribute__((address_space(3))) void*)(Bs + buf * (SW_T * SW_KC) + piece * 512), 16, 0, 0);
        }
      };
      // the wave's rows as MFMA fragments, whole K: lane (li, lh) holds for k step s the 8 halves at k = 16 s + 8 lh of rows ib * 32 + li
      bf16x8 af[2][SW_KMAX / 16];
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) {
        int gr = stride * (i0 + wi * 64 + ib * 32 + li);
        gr = gr < n ? gr : n - 1;
        const __attribute__((address_space(1))) uint16_t* src = (const __attribute__((address_space(1))) uint16_t*)(w.dn16 + (int64_t)gr * d + 8 * lh);
#pragma unroll
        for (int s = 0; s < SW_KMAX / 16; ++s) af[ib][s] = *(const __attribute__((address_space(1))) bf16x8*)(src + (16 * s < d ? 16 * s : 0));   // (32 loads in flight)
      }
      const int nchunks = ntl * kpc;
      issue_b(0, 0, 0);
      if (nchunks > 1) issue_b(kpc > 1 ? 0 : 1, kpc > 1 ? 1 : 0, 1);
      // (the fragments are "used" here: the compiler's wait for their loads lands in front of the tile loop, once per unit, instead of in front
      // of the first MFMA of every tile, where it would also wait for the chunks in flight)
#pragma unroll
      for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int s = 0; s < SW_KMAX / 16; ++s) asm volatile("" : "+v"(af[ib][s]));
      f32x16 acc[2][2];        // [jb][ib]: lane holds S[i = wi*64 + ib*32 + li][j = wj*64 + jb*32 + (r&3) + 8*(r>>2) + 4*lh]
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
      int par = 0, cidx = 0;                            // ring slot and index of the chunk under the MFMAs
      int tl2 = kpc > 2 ? 0 : (kpc == 2 ? 1 : 2), kc2 = kpc > 2 ? 2 : 0;       // (tile, K chunk) of chunk cidx + 2
      for (int tl = 0; tl < ntl; ++tl) {
#pragma unroll
        for (int kc = 0; kc < SW_KMAX / SW_KC; ++kc) {
          if (kc >= kpc) break;
          // chunk cidx has landed when at most the 4 loads of chunk cidx + 1 are outstanding
          if (cidx + 1 < nchunks) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();                 // ... for every wave; every wave is done with chunk cidx - 1: its slot takes chunk cidx + 2
                                                        // (the bare barrier: __syncthreads() would wait for the chunks in flight as well)
          if (MODE == SIM_COLLECT && kc == 0 && tl > 0) {     // room for a dense tile.  nst is read by every wave between two barriers with no epilogue
            const uint32_t cur = lds_read_raw(nst_off);       // in between: with kpc > 1 the next one is the barrier of chunk kc = 1; with a single K chunk
            if (kpc == 1) __builtin_amdgcn_s_barrier();       // per tile the next barrier would come AFTER this tile's epilogue, so one is added here
            if (cur > (uint32_t)SIM_STAGE / 2) flush();       // (uniform: flush() holds barriers)
          }
          if (cidx + 2 < nchunks) issue_b(tl2, kc2, par >= 1 ? par - 1 : 2);
          if (++kc2 == kpc) { kc2 = 0; ++tl2; }
          ++cidx;
          const uint16_t* Bb = Bs + par * (SW_T * SW_KC);
          par = par == SW_RING - 1 ? 0 : par + 1;
#pragma unroll
          for (int s = 0; s < SW_KC / 16; ++s) {
            bf16x8 bf[2];
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
              const int row = wj * 64 + jb * 32 + li;
              bf[jb] = *(const bf16x8*)(Bb + row * SW_KC + (((2 * s + lh) ^ ((row >> 1) & 7)) << 3));
            }
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
              for (int ib = 0; ib < 2; ++ib)
                acc[jb][ib] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(agc_h8, bf[jb]), __builtin_bit_cast(agc_h8, af[ib][kc * (SW_KC / 16) + s]),
                                                                     acc[jb][ib], 0, 0, 0);
          }
        }
        // ---- the tile is complete (the first chunk of the next one is in flight).  The epilogue is written for instruction count: it runs
        // 16 384 times per image of 4096 on every wave.
        const int j0 = jbase + tl * SW_T;
        const bool interior = stride * (i0 + SW_T - 1) < j0 && stride * (i0 + SW_T - 1) < n && j0 + SW_T <= n;      // every entry a pair i < j < n
        const int jl = j0 + wj * 64 + 4 * lh;
        if (MODE == SIM_SAMPLE) {
#pragma unroll
          for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int ib = 0; ib < 2; ++ib) {
              const int gi = stride * (i0 + wi * 64 + ib * 32 + li);
              // pairs that do not exist (j <= i, or past n):  0 <= gj - gi - 1 < n - gi - 1  in one unsigned compare
              const uint32_t span = gi < n ? (uint32_t)(n - gi - 1) : 0u;
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const float v = acc[jb][ib][r];
                acc[jb][ib][r] = 0.f;
                if (interior || (uint32_t)(jl + jb * 32 + (r & 3) + 8 * (r >> 2) - gi - 1) < span) lds_add_raw(hist_off + 4u * (uint32_t)agc_linear_bin(v), 1u);
              }
            }
        } else {
          // u = v - vC, t = h^2 - u^2 (vC, h = centre and half width of the window): inside iff t >= 0, below iff outside and u < 0, above
          // otherwise -- a partition whatever the rounding.  Only SIGN BITS are needed: two packed instructions per PAIR of entries
          // (v_pk_add_f32, v_pk_fma_f32) and one v_alignbit per entry and mask that shifts the bit into a per-lane word; no compare.
          uint32_t sgn[2] = {0u, 0u}, out[2] = {0u, 0u};      // entry 16 * ib + r of word jb sits at bit 31 - (16 * ib + r)
          auto classify2 = [&](float v0, float v1, int jb) __attribute__((always_inline)) {
            const agc_f2 u = agc_f2{v0, v1} - vC2;
            const agc_f2 tt = __builtin_elementwise_fma(-u, u, hsq2);
            sgn[jb] = __builtin_amdgcn_alignbit(sgn[jb], __float_as_uint(u[0]), 31);
            sgn[jb] = __builtin_amdgcn_alignbit(sgn[jb], __float_as_uint(u[1]), 31);
            out[jb] = __builtin_amdgcn_alignbit(out[jb], __float_as_uint(tt[0]), 31);
            out[jb] = __builtin_amdgcn_alignbit(out[jb], __float_as_uint(tt[1]), 31);
          };
          if (interior) {
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
              for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                  classify2(acc[jb][ib][r], acc[jb][ib][r + 1], jb);
                  acc[jb][ib][r] = 0.f; acc[jb][ib][r + 1] = 0.f;
                }
          } else {
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
              for (int ib = 0; ib < 2; ++ib) {
                const int gi = stride * (i0 + wi * 64 + ib * 32 + li);
                const uint32_t span = gi < n ? (uint32_t)(n - gi - 1) : 0u;
#pragma unroll
                for (int r = 0; r < 16; r += 2) {    // (a pair that does not exist is +inf: above every window)
                  const int jo = jl + jb * 32 + (r & 3) + 8 * (r >> 2) - gi - 1;
                  classify2((uint32_t)jo < span ? acc[jb][ib][r] : __builtin_inff(), (uint32_t)(jo + 1) < span ? acc[jb][ib][r + 1] : __builtin_inff(), jb);
                  acc[jb][ib][r] = 0.f; acc[jb][ib][r + 1] = 0.f;
                }
              }
          }
          below += (uint32_t)(__builtin_popcount(sgn[0] & out[0]) + __builtin_popcount(sgn[1] & out[1]));
          // the hits of this lane (a fifth of the lanes hold one per tile, almost none three): ONE reservation per lane that has any -- a single
          // LDS instruction for the wave -- then the lane writes its entries
          uint64_t m = (uint64_t)(~out[0]) | ((uint64_t)(~out[1]) << 32);
          if (m != 0ull) {
            uint32_t slot = lds_add_rtn_raw(nst_off, (uint32_t)__popcll(m));
            do {
              const int b6 = __builtin_ctzll(m);
              m &= m - 1ull;
              const int e = 31 - (b6 & 31), r = e & 15, ib = e >> 4, jb = b6 >> 5;
              const uint32_t gi = (uint32_t)(stride * (i0 + wi * 64 + ib * 32 + li));
              const uint32_t packed = (gi << AGC_PK_SHIFT) | (uint32_t)(jl + jb * 32 + (r & 3) + 8 * (r >> 2));
              if (slot < (uint32_t)SIM_STAGE) lds_write_raw(hist_off + 4u * slot, packed);
              else {                                          // staging buffer full inside one tile: straight to the list (degenerate inputs)
                const uint32_t g = atomicAdd(&w.sel[3], 1u);
                if (g < w.list_cap) w.list[g] = packed;
              }
              ++slot;
            } while (m != 0ull);
          }
        }
      }
    }
    if (MODE == SIM_COLLECT) {
      flush();
      for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o, 64);
      if (lane == 0 && below) atomicAdd((uint32_t*)&w.counters[5], below);
    } else {
      __syncthreads();
      for (int i = t; i < 4096; i += 256)
        if (hist[i]) { atomicAdd(&w.hist[i], hist[i]); hist[i] = 0u; }
    }
  }
}

// Window flow: from the sample histogram (4096 linear bins, agc_simw_kernel<SIM_SAMPLE>) to the window of approximate values that must hold
// the k-th smallest.  Sample ranks r_lo / r_hi bracket rank k by 3 % and five standard deviations of the sample count (none when the sample is
// the whole triangle); the window is the span of their bins widened by 2 eps on either side, eps = the bound of |approximate - exact|:
//   | sum a16 b16 (f32 MFMA accumulation) - fl32(sum a b in f64) |  <=  2 dmax + dmax^2  +  256 * 2^-24  +  2^-24,   dmax = the image's largest
// row rounding error (band[3], agc_normalize_kernel; Cauchy-Schwarz on unit rows).  band = {vL, vU, eps_check, dmax}; the histogram, the list
// length and the below-window counter are cleared.  The window is only a PREDICTION: agc_finish_kernel verifies
// vL + eps <= threshold <= vU - eps and that rank k fell inside the list, else info[7] |= 2 and the caller repeats the build with the robust flow.
__global__ __launch_bounds__(256) void agc_window_kernel(const AgcWs* __restrict__ ws, float test_shift) {
  const AgcWs& w = ws[blockIdx.y];
  __shared__ uint64_t wsum[4];
  __shared__ uint64_t ranks[2];
  __shared__ int bsel[2];
  __shared__ int s_open[2];
  __shared__ uint32_t s_dmax;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  constexpr int per = 16;
  uint64_t v = 0;
  for (int q = 0; q < per; ++q) v += w.hist[t * per + q];
  uint64_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wsum[wave] = incl;
  if (t == 0) { bsel[0] = 0; bsel[1] = 4095; s_dmax = 0u; }
  __syncthreads();
  for (int q = 0; q < wave; ++q) incl += wsum[q];
  if (t == 255) {
    const uint64_t ns = incl, k = (uint64_t)w.sel[1] | ((uint64_t)w.sel[2] << 32);
    const uint64_t L = (uint64_t)w.n * (uint64_t)(w.n - 1) / 2;
    uint64_t rlo = k, rhi = k;
    if (ns != L) {
      const double f = (double)ns / (double)L, p = ((double)k + 0.5) / (double)L;
      const double sd = sqrt((double)ns * p * (1.0 - p));
      const double lo = f * (double)k * 0.97 - 5.0 * sd - 1.0, hi = f * (double)(k + 1) * 1.03 + 5.0 * sd + 1.0;
      rlo = lo > 0.0 ? (uint64_t)lo : 0ull;
      rhi = (uint64_t)hi;
    }
    const uint64_t last = ns ? ns - 1 : 0;
    s_open[0] = ns != L && rlo == 0;
    s_open[1] = ns != L && rhi >= last;
    ranks[0] = rlo < last ? rlo : last;
    ranks[1] = rhi < last ? rhi : last;
  }
  __syncthreads();
  const uint64_t excl0 = incl - v;
  for (int e = 0; e < 2; ++e) {
    const uint64_t r = ranks[e];
    if (t < 255 ? (excl0 <= r && r < incl) : excl0 <= r) {
      uint64_t excl = excl0;
      int b = t * per;
      for (int q = 0; q < per; ++q, ++b) {
        const uint64_t c = w.hist[b];
        if (r < excl + c || b == 4095) break;
        excl += c;
      }
      bsel[e] = b;
    }
  }
  __syncthreads();
  {    // dmax = the largest row rounding error (positive floats order like their bits; a NaN row poisons the window: nothing lands in it -> miss)
    uint32_t m = 0u;
    for (int i = t; i < w.n; i += 256) { const uint32_t b = (uint32_t)w.deg[i]; m = b > m ? b : m; }
    for (int o = 32; o > 0; o >>= 1) { const uint32_t y = (uint32_t)__shfl_xor((int)m, o, 64); m = y > m ? y : m; }
    if (lane == 0) atomicMax(&s_dmax, m);
  }
  __syncthreads();
  if (t == 0) {
    const float dmax = __uint_as_float(s_dmax);
    w.band[3] = s_dmax;
    const float eps = 2.02f * dmax + dmax * dmax + 6e-5f, eps_check = 2.01f * dmax + dmax * dmax + 4e-5f;
    float vL = ((float)bsel[0] / 2048.f - 1.f) - 2.f * eps + test_shift, vU = ((float)(bsel[1] + 1) / 2048.f - 1.f) + 2.f * eps + test_shift;
    // a bracket that ran into the end of the sample bounds nothing on that side (percentiles next to 0 or 100): the window is open there
    if (s_open[0]) vL = -4.f + test_shift;
    if (s_open[1]) vU = 4.f + test_shift;
    w.band[0] = __float_as_uint(vL); w.band[1] = __float_as_uint(vU); w.band[2] = __float_as_uint(eps_check);
    w.sel[3] = 0u;
    w.counters[5] = 0;
  }
  for (int q = 0; q < per; ++q) w.hist[t * per + q] = 0;
}

// 12-bit histogram (top bits of the 16-bit order-preserving key) of the strict upper triangle of S16 (collect == 0), or, collect == 1, the packed
// indices (i << 16 | j) of the entries whose bin lies in the band [band[0], band[1]] appended to the list (LDS-staged: one global reservation per
// flush).  Rows are walked with 16-byte loads (8 entries), four in flight per thread.
constexpr int AGC_STAGE = 4096;
__global__ __launch_bounds__(256) void agc_sweep16_kernel(const AgcWs* __restrict__ ws, int collect) {
  const AgcWs& w = ws[blockIdx.y];
  __shared__ uint32_t h[4096];               // histogram, or the staging buffer of the collect pass
  __shared__ uint32_t nst, gbase;
  for (int i = threadIdx.x; i < 4096; i += 256) h[i] = 0;
  if (threadIdx.x == 0) nst = 0;
  __syncthreads();
  const uint32_t blo = collect ? w.band[0] : 0u, bhi = collect ? w.band[1] : 0u;
  auto flush = [&]() __attribute__((always_inline)) {        // (called by the whole workgroup)
    __syncthreads();
    const uint32_t cnt = nst < (uint32_t)AGC_STAGE ? nst : (uint32_t)AGC_STAGE;
    if (threadIdx.x == 0) gbase = atomicAdd(&w.sel[3], cnt);
    __syncthreads();
    const uint32_t base = gbase;
    for (uint32_t i = threadIdx.x; i < cnt; i += 256)
      if (base + i < w.list_cap) w.list[base + i] = h[i];
    __syncthreads();
    if (threadIdx.x == 0) nst = 0;
    __syncthreads();
  };
  // Work unit = the row pair (a, n - 1 - a): its two strict-upper-triangle pieces together hold n - 1 entries whatever a is, so every unit
  // is the same amount of work (single rows run from n - 1 entries down to none).  The unit's 16-byte chunks (row a's, then row b's) are
  // dealt round-robin to the threads, four loads in flight per thread.
  const int n = w.n, half = (n + 1) / 2;
  for (int a = blockIdx.x; a < half; a += gridDim.x) {
    const int b = n - 1 - a;
    const int ca0 = (a + 1) >> 3, cb0 = (b + 1) >> 3, cend = (n + 7) >> 3;          // first chunk of each row piece; chunks per full row
    const int na = cend - ca0, nb = b > a ? cend - cb0 : 0;
    for (int c0 = threadIdx.x; c0 < na + nb; c0 += 4 * 256) {
      uint4 v[4];
      int ri[4], cj[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = c0 + u * 256;
        const bool first = c < na;
        ri[u] = first ? a : b;
        cj[u] = first ? ca0 + c : cb0 + (c - na);
        v[u] = c < na + nb ? *(const uint4*)(w.S16 + (int64_t)ri[u] * w.lds16 + 8 * cj[u]) : make_uint4(0, 0, 0, 0);
        if (c >= na + nb) cj[u] = -1;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (cj[u] < 0) continue;
        const int i = ri[u], j8 = 8 * cj[u];
        const uint32_t x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int j = j8 + q;
          if (j > i && j < n) {
            const uint32_t bin = h16_key((uint16_t)(x[q >> 1] >> (16 * (q & 1)))) >> 4;
            if (!collect) atomicAdd(&h[bin], 1u);
            else if (bin >= blo && bin <= bhi) {
              const uint32_t slot = atomicAdd(&nst, 1u);
              const uint32_t packed = ((uint32_t)i << AGC_PK_SHIFT) | (uint32_t)j;
              if (slot < (uint32_t)AGC_STAGE) h[slot] = packed;
              else {                                          // staging buffer full inside one unit: straight to the list (rare)
                const uint32_t g = atomicAdd(&w.sel[3], 1u);
                if (g < w.list_cap) w.list[g] = packed;
              }
            }
          }
        }
      }
    }
    if (collect) {                                            // between units: keep room for a dense one.  The decision is taken on ONE value of nst:
      __syncthreads();                                        // every thread reads it between two barriers (a wave that ran ahead into the next unit
      const uint32_t cur = nst;                               // would bump it under the others' eyes, and flush() holds barriers)
      __syncthreads();
      if (cur > (uint32_t)AGC_STAGE / 2) flush();
    }
  }
  if (collect) { flush(); return; }
  __syncthreads();
  for (int i = threadIdx.x; i < 4096; i += 256)
    if (h[i]) atomicAdd(&w.hist[i], h[i]);
}

// The bin b* that holds rank k of the approximate matrix, the band of bins whose values can be within 2 AGC_EPS of b*'s, the exact count below the
// band -> band[0..1], sel = {prefix 0, k - count below (64 bit), list length 0}; histogram cleared for the digit passes over the list.
__global__ __launch_bounds__(256) void agc_band_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  __shared__ uint64_t wsum[4];
  __shared__ int bstar;
  __shared__ unsigned int s_lo, s_hi, s_dmax;
  __shared__ unsigned long long below;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  constexpr int per = 16;
  uint64_t v = 0;
  for (int q = 0; q < per; ++q) v += w.hist[t * per + q];
  uint64_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wsum[wave] = incl;
  if (t == 0) { s_lo = 4095u; s_hi = 0u; below = 0ull; bstar = 4095; s_dmax = 0u; }
  __syncthreads();
  for (int q = 0; q < wave; ++q) incl += wsum[q];
  const uint64_t k = (uint64_t)w.sel[1] | ((uint64_t)w.sel[2] << 32);
  uint64_t excl = incl - v;
  if (t < 255 ? (excl <= k && k < incl) : excl <= k) {
    int b = t * per;
    for (int q = 0; q < per; ++q, ++b) {
      const uint64_t c = w.hist[b];
      if (k < excl + c || b == 4095) break;
      excl += c;
    }
    bstar = b;
  }
  {    // dmax = the largest row rounding error of the image (agc_normalize_kernel; positive floats order like their bits)
    uint32_t m = 0u;
    for (int i = t; i < w.n; i += 256) { const uint32_t b = (uint32_t)w.deg[i]; m = b > m ? b : m; }
    for (int o = 32; o > 0; o >>= 1) { const uint32_t y = (uint32_t)__shfl_xor((int)m, o, 64); m = y > m ? y : m; }
    if (lane == 0) atomicMax(&s_dmax, m);
  }
  __syncthreads();
  const int bs = bstar;
  // |S16 - exact| <= eps: operand rounding 2 dmax + dmax^2 (Cauchy-Schwarz on unit rows, MEASURED -- subnormal halves counted as flushed),
  // 256 f32 additions + the final rounding of the exact value (< 6e-5), the stored result rounded to half (|S| < 2: <= 2^-11)
  const float dmax = __uint_as_float(s_dmax);
  const float eps = 2.02f * dmax + dmax * dmax + 6e-5f + 0.0005f;
  const float lo_val = h16_val((uint32_t)bs << 4) - 2.f * eps, hi_val = h16_val(((uint32_t)bs << 4) | 15u) + 2.f * eps;
  // a bin belongs to the band iff its value range [v(b << 4), v(b << 4 | 15)] meets [lo_val, hi_val]; NaN bins (keys past the infinities) never do
  unsigned long long mybelow = 0;
  unsigned int mlo = 4095u, mhi = 0u;
  bool any = false;
  for (int q = 0; q < per; ++q) {
    const uint32_t b = (uint32_t)(t * per + q);
    const float vlo = h16_val(b << 4), vhi = h16_val((b << 4) | 15u);
    const bool in = (vhi >= lo_val && vlo <= hi_val) || (int)b == bs;
    if (in) { mlo = b < mlo ? b : mlo; mhi = b > mhi ? b : mhi; any = true; }
  }
  if (any) { atomicMin(&s_lo, mlo); atomicMax(&s_hi, mhi); }
  __syncthreads();
  const unsigned int blo = s_lo, bhi = s_hi;
  for (int q = 0; q < per; ++q) {
    const uint32_t b = (uint32_t)(t * per + q);
    if (b < blo) mybelow += w.hist[b];
  }
  if (mybelow) atomicAdd(&below, mybelow);
  __syncthreads();
  if (t == 0) {
    const uint64_t r = k - below;
    w.band[0] = blo; w.band[1] = bhi;
    // the k-th exact value lies within eps of the k-th approximate one, i.e. of bin b*'s range: agc_finish_kernel checks the selected threshold
    // against [band[2], band[3]] (NaN bounds -- a NaN row -- fail the check)
    w.band[2] = __float_as_uint(h16_val((uint32_t)bs << 4) - eps); w.band[3] = __float_as_uint(h16_val(((uint32_t)bs << 4) | 15u) + eps);
    w.sel[0] = 0u; w.sel[1] = (uint32_t)r; w.sel[2] = (uint32_t)(r >> 32); w.sel[3] = 0u;
  }
  __syncthreads();
  for (int q = 0; q < per; ++q) w.hist[t * per + q] = 0;
}

// list[e] = (i << 16 | j)  ->  the order-preserving key of the exact similarity of rows i and j (in place); the same for the radius candidates
// (clist -> ckey).  Eight lanes per entry.
__global__ __launch_bounds__(256) void agc_exact_kernel(const AgcWs* __restrict__ ws, int n_images, int window) {
  const int nparts = agc_nparts(n_images);
  for (int u = blockIdx.x & 7; u < n_images * nparts; u += 8) {
  const AgcWs& w = ws[u / nparts];
  if (window && u % nparts == 0 && (blockIdx.x >> 3) == 0 && threadIdx.x == 0) {
    // window flow: rank of the threshold AMONG the listed entries = k - (entries below the window); a rank outside the list is a missed window
    const uint64_t k = (uint64_t)w.krank, below = (uint32_t)w.counters[5], nl0 = w.sel[3];
    const bool hit = k >= below && k < below + nl0;
    const uint64_t r = hit ? k - below : 0ull;
    if (!hit) w.counters[7] = 1;
    w.sel[0] = 0u; w.sel[1] = (uint32_t)r; w.sel[2] = (uint32_t)(r >> 32);
  }
  if (!window && u % nparts == 0 && (blockIdx.x >> 3) == 0 && threadIdx.x == 0) {
    // robust flow: the rank among the band entries (agc_band_kernel) must fall inside the collected list, and the list must have fitted
    const uint64_t r = (uint64_t)w.sel[1] | ((uint64_t)w.sel[2] << 32);
    if (!(r < (uint64_t)w.sel[3]) || w.sel[3] > w.list_cap) w.counters[7] = 1;
  }
  const uint32_t nl = w.sel[3] < w.list_cap ? w.sel[3] : w.list_cap;
  const uint32_t nc = (uint32_t)w.counters[4] < w.clist_cap ? (uint32_t)w.counters[4] : w.clist_cap;
  const uint32_t nlp = (nl + 31u) & ~31u, total = nlp + ((nc + 31u) & ~31u);       // (whole waves stay in the loop: shuffles)
  const int q = threadIdx.x & 7;
  const uint32_t slot = (uint32_t)(u % nparts) + (uint32_t)nparts * (blockIdx.x >> 3), nslots = (uint32_t)nparts * (gridDim.x >> 3);
  for (uint32_t e = (slot * 256 + threadIdx.x) >> 3; e < total; e += (nslots * 256) >> 3) {
    const bool band = e < nlp;
    const uint32_t idx = band ? e : e - nlp;
    const bool live = band ? idx < nl : idx < nc;
    const uint32_t pk = live ? (band ? w.list[idx] : w.clist[idx]) : 0u;
    const int i = (int)(pk >> AGC_PK_SHIFT), j = (int)(pk & AGC_PK_MASK);
    const float sim = agc_exact_sim8(w.dnf + (int64_t)i * w.d, w.dnf + (int64_t)j * w.d, w.d, q);
    if (live && q == 0) (band ? w.list : w.ckey)[idx] = f32_key(sim);
  }
  }
}

// ---------------------------------------------------------------------------------------------- K3, band-limited flow
constexpr int RAD_STAGE = 2048;
// Keypoint grid for the radius search: cells of side 1.001 r (cell index = floor(x / side) in float64: two points within r of each other sit in
// the same or in adjacent cells whatever the rounding), hashed into AGC_NB buckets; one workgroup per image counts, scans and scatters in LDS.
__device__ __forceinline__ int agc_cell(float x, double inv_side) {
  const double c = floor((double)x * inv_side);
  return x == x ? (int)fmin(fmax(c, -1073741824.0), 1073741824.0) : 0;
}
__device__ __forceinline__ uint32_t agc_cell_hash(int cx, int cy) {
  uint32_t h = (uint32_t)cx * 73856093u ^ (uint32_t)cy * 19349663u;
  h ^= h >> 15;
  return h & (uint32_t)(AGC_NB - 1);
}
__global__ __launch_bounds__(1024) void agc_grid_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  const double inv_side = w.inv_side;
  extern __shared__ int cnt[];                  // [AGC_NB] counts, then running fill positions
  __shared__ int wsum[16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, n = w.n;
  for (int b = t; b < AGC_NB; b += 1024) cnt[b] = 0;
  __syncthreads();
  for (int i = t; i < n; i += 1024) atomicAdd(&cnt[agc_cell_hash(agc_cell(w.kpts[2 * i], inv_side), agc_cell(w.kpts[2 * i + 1], inv_side))], 1);
  __syncthreads();
  constexpr int per = AGC_NB / 1024;
  int v = 0;
  for (int q = 0; q < per; ++q) v += cnt[t * per + q];
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  for (int q = 0; q < wave; ++q) incl += wsum[q];
  int excl = incl - v;
  for (int q = 0; q < per; ++q) {
    const int c = cnt[t * per + q];
    w.cellptr[t * per + q] = excl;
    cnt[t * per + q] = excl;
    excl += c;
  }
  if (t == 1023) w.cellptr[AGC_NB] = excl;
  __syncthreads();
  for (int i = t; i < n; i += 1024) {
    const int pos = atomicAdd(&cnt[agc_cell_hash(agc_cell(w.kpts[2 * i], inv_side), agc_cell(w.kpts[2 * i + 1], inv_side))], 1);
    w.cellidx[pos] = i;
  }
}

// Radius candidates through the grid (agc.py:435-447: ||xi - xj||^2 <= r^2 in float64, inclusive): point i looks at the buckets of its own and
// the eight adjacent cells and takes the points j > i of exactly that cell (two cells may share a bucket: no pair twice) that pass the float64
// test -- the same predicate on the same pairs as the all-pairs kernel below, which stays for degenerate radii.  A workgroup also clears the
// adjacency rows of its points.  Candidates are staged in LDS (one global reservation per workgroup).
__global__ __launch_bounds__(288) void agc_radius_grid_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  const double r2 = w.r2, inv_side = w.inv_side;
  const float* __restrict__ kpts = w.kpts;
  __shared__ uint32_t st[RAD_STAGE];
  __shared__ uint32_t nst, gbase;
  if (threadIdx.x == 0) nst = 0;
  __syncthreads();
  // 32 points per workgroup, one thread per (point, cell of its 3 x 3 neighbourhood): the search is a chain of dependent loads (bucket bounds ->
  // point id -> coordinates), so what it needs is many short chains in flight, not few long ones
  const int n = w.n, i0 = blockIdx.x * 32, i = i0 + (int)threadIdx.x / 9, c = (int)threadIdx.x % 9;
  {  // the adjacency rows of the workgroup's points start empty (one contiguous piece of 32 nw words)
    const int64_t r0 = (int64_t)i0 * w.nw, rend = (int64_t)(n < i0 + 32 ? n : i0 + 32) * w.nw;
    for (int64_t k = r0 + threadIdx.x; k < rend; k += 288) w.bits[k] = 0ull;
  }
  if (i < n) {
    const float xi = kpts[2 * i], yi = kpts[2 * i + 1];
    const int nx = agc_cell(xi, inv_side) + c % 3 - 1, ny = agc_cell(yi, inv_side) + c / 3 - 1;
    const uint32_t h = agc_cell_hash(nx, ny);
    const int e0 = w.cellptr[h], e1 = w.cellptr[h + 1];
    for (int e = e0; e < e1; ++e) {
      const int j = w.cellidx[e];
      if (j <= i) continue;
      const float xj = kpts[2 * j], yj = kpts[2 * j + 1];
      if (agc_cell(xj, inv_side) != nx || agc_cell(yj, inv_side) != ny) continue;
      const double ddx = (double)xi - (double)xj, ddy = (double)yi - (double)yj;
      if (!(ddx * ddx + ddy * ddy <= r2)) continue;
      const uint32_t packed = ((uint32_t)i << AGC_PK_SHIFT) | (uint32_t)j;
      const uint32_t slot = atomicAdd(&nst, 1u);
      if (slot < (uint32_t)RAD_STAGE) st[slot] = packed;
      else {
        const uint32_t g = atomicAdd((uint32_t*)&w.counters[4], 1u);
        if (g < w.clist_cap) w.clist[g] = packed;
      }
    }
  }
  __syncthreads();
  const uint32_t cnt = nst < (uint32_t)RAD_STAGE ? nst : (uint32_t)RAD_STAGE;
  if (threadIdx.x == 0) gbase = cnt ? atomicAdd((uint32_t*)&w.counters[4], cnt) : 0u;
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < cnt; k += 288)
    if (gbase + k < w.clist_cap) w.clist[gbase + k] = st[k];
}

// adjacency bits of the candidates whose exact similarity reaches the threshold (the reference tests sim_matrix[i, j] >= thr, agc.py:445-446)
__global__ __launch_bounds__(256) void agc_apply_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  const float thr = key_f32(w.sel[0]);
  const uint32_t nc = (uint32_t)w.counters[4] < w.clist_cap ? (uint32_t)w.counters[4] : w.clist_cap;
  for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < nc; e += gridDim.x * 256) {
    if (!(key_f32(w.ckey[e]) >= thr)) continue;
    const uint32_t pk = w.clist[e];
    const int i = (int)(pk >> AGC_PK_SHIFT), j = (int)(pk & AGC_PK_MASK);
    atomicOr((unsigned long long*)&w.bits[(int64_t)i * w.nw + (j >> 6)], 1ull << (j & 63));
    atomicOr((unsigned long long*)&w.bits[(int64_t)j * w.nw + (i >> 6)], 1ull << (i & 63));
  }
}

// ---------------------------------------------------------------------------------------------- degrees
__global__ __launch_bounds__(256) void agc_deg_kernel(const AgcWs* __restrict__ ws, int count_total) {
  const AgcWs& w = ws[blockIdx.y];
  int32_t* deg = w.deg;
  int32_t* total = count_total ? w.counters + 0 : nullptr;
  // sixteen lanes per row (four rows per wave, sixteen per workgroup): at 4096 points a row is 64 words, four per lane
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, sub = lane & 15;
  const int i = blockIdx.x * 16 + wave * 4 + (lane >> 4);
  int c = 0;
  if (i < w.n)
    for (int k = sub; k < w.nw; k += 16) c += __popcll(w.bits[(int64_t)i * w.nw + k]);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (sub == 0 && i < w.n) deg[i] = c;
  if (total) {                          // one atomic per workgroup, not per row
    __shared__ int part[4];
    int cw = sub == 0 ? c : 0;
    cw += __shfl_xor(cw, 16, 64);
    cw += __shfl_xor(cw, 32, 64);
    if (lane == 0) part[wave] = cw;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int sum = part[0] + part[1] + part[2] + part[3];
      if (sum) atomicAdd(total, sum);
    }
  }
}

// ---------------------------------------------------------------------------------------------- K4 isolated nodes
__global__ __launch_bounds__(256) void agc_iso_nn_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  const float* __restrict__ kpts = w.kpts;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + wave;
  if (i >= w.n) return;
  if (w.deg[i] != 0) {
    if (lane == 0) w.nn[i] = -1;
    return;
  }
  const double xi = kpts[2 * i], yi = kpts[2 * i + 1];
  double bd = 1e300;
  int bj = 0x7fffffff;
  for (int j = lane; j < w.n; j += 64) {
    if (j == i) continue;
    const double dx = (double)kpts[2 * j] - xi, dy = (double)kpts[2 * j + 1] - yi;
    const double dd = dx * dx + dy * dy;
    if (dd < bd) { bd = dd; bj = j; }   // ascending j: first minimum kept
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(bd, o, 64);
    const int oj = __shfl_xor(bj, o, 64);
    if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
  }
  if (lane == 0) w.nn[i] = bj;
}

// sequential semantics of agc.py:489-494: ascending node order; a node is still isolated at its turn iff it
// started isolated and no earlier isolated node attached to it.  Only the (few) initially isolated nodes
// are walked, from an ordered compaction held in LDS.
__global__ __launch_bounds__(1024) void agc_iso_seq_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  int32_t* info = w.info;
  extern __shared__ int32_t sm[];
  int32_t* list = sm;                       // [n] ordered isolated ids
  uint32_t* touched = (uint32_t*)(sm + w.n);  // [n/32+1]
  __shared__ int wcount[17];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int total_dir = w.counters[0];
  for (int k = t; k < (w.n + 31) / 32; k += 1024) touched[k] = 0;
  if (t == 0) wcount[16] = 0;
  __syncthreads();
  int n_added = 0;
  if (total_dir != 0 && w.n > 1) {       // agc.py:486 early return when the graph has no edges
    for (int base = 0; base < w.n; base += 1024) {
      const int i = base + t;
      const bool iso = i < w.n && w.deg[i] == 0;
      const uint64_t m = __ballot(iso);
      if (lane == 0) wcount[wave] = __popcll(m);
      __syncthreads();
      int off = wcount[16];
      for (int q = 0; q < wave; ++q) off += wcount[q];
      if (iso) list[off + __popcll(m & ((1ull << lane) - 1))] = i;
      __syncthreads();
      if (t == 0) {
        int s = 0;
        for (int q = 0; q < 16; ++q) s += wcount[q];
        wcount[16] += s;
      }
      __syncthreads();
    }
    if (t == 0) {
      const int cnt = wcount[16];
      for (int q = 0; q < cnt; ++q) {
        const int i = list[q];
        if (touched[i >> 5] & (1u << (i & 31))) continue;
        const int j = w.nn[i];
        w.bits[(int64_t)i * w.nw + (j >> 6)] |= 1ull << (j & 63);
        w.bits[(int64_t)j * w.nw + (i >> 6)] |= 1ull << (i & 63);
        touched[j >> 5] |= 1u << (j & 31);
        ++n_added;
      }
    }
  }
  if (t == 0) info[3] = n_added;
}

// ---------------------------------------------------------------------------------------------- bits -> CSR
// exclusive scan, one workgroup per image.  mode 0: deg -> ptr0 (total -> counters[2]);
// mode 1: component sizes (coff) -> coff2; mode 2: degk -> indptr (total -> info[1])
__global__ __launch_bounds__(1024) void agc_scan_kernel(const AgcWs* __restrict__ ws, int mode) {
  const AgcWs& w = ws[blockIdx.y];
  const int n = w.n;
  const int32_t* deg = mode == 0 ? w.deg : (mode == 1 ? w.coff : w.degk);
  int32_t* ptr = mode == 0 ? w.ptr0 : (mode == 1 ? w.coff2 : w.indptr);
  int32_t* total_out = mode == 0 ? w.counters + 2 : (mode == 1 ? nullptr : w.info + 1);
  __shared__ int wsum[16];
  __shared__ int carry;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int i = base + t;
    int v = i < n ? deg[i] : 0;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int off = carry;
    for (int q = 0; q < wave; ++q) off += wsum[q];
    if (i < n) ptr[i] = off + x - v;
    __syncthreads();
    if (t == 0) {
      int s = 0;
      for (int q = 0; q < 16; ++q) s += wsum[q];
      carry += s;
    }
    __syncthreads();
  }
  if (t == 0) {
    ptr[n] = carry;
    if (total_out) *total_out = carry;
  }
}

// row i of the bit matrix -> idx[ptr[i] ...] ascending; optional relabel through newid (rows with newid<0 skipped)
__global__ __launch_bounds__(256) void agc_fill_kernel(const AgcWs* __restrict__ ws, int final_pass) {
  const AgcWs& w = ws[blockIdx.y];
  const int32_t* __restrict__ ptr_by_row = final_pass ? w.indptr : w.ptr0;
  const int32_t* __restrict__ newid = final_pass ? w.newid : nullptr;
  int32_t* __restrict__ idx = final_pass ? w.indices : w.idx0;
  const int cap = final_pass ? w.max_edges_dir : w.cap;
  // sixteen lanes per row (four rows per wave): lane `sub` owns the words [sub * wpl, (sub + 1) * wpl) of the row, so the neighbours leave in
  // ascending order; an exclusive scan of the lanes' counts places them
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, sub = lane & 15;
  const int i = blockIdx.x * 16 + wave * 4 + (lane >> 4);
  const bool live = i < w.n && !(newid && newid[i] < 0);
  const int wpl = (w.nw + 15) / 16, k0 = sub * wpl, k1 = k0 + wpl < w.nw ? k0 + wpl : w.nw;
  int c = 0;
  if (live)
    for (int k = k0; k < k1; ++k) c += __popcll(w.bits[(int64_t)i * w.nw + k]);
  int x = c;
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const int y = __shfl_up(x, o, 16);
    if (sub >= o) x += y;
  }
  if (!live) return;
  int pos = ptr_by_row[newid ? newid[i] : i] + x - c;
  for (int k = k0; k < k1; ++k) {
    uint64_t m = w.bits[(int64_t)i * w.nw + k];
    while (m) {
      const int b = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int j = k * 64 + b;
      if (pos < cap) {
        idx[pos] = newid ? newid[j] : j;
        if (!final_pass) w.esrc[pos] = i;
      }
      ++pos;
    }
  }
}

// ---------------------------------------------------------------------------------------------- K5 components
// single workgroup; parent[n], count[n] in LDS -- or, GLOBAL (images of more than AGC_CC_LDS_N nodes), in the members / nnc arrays, which are free
// until the linking step: every access to them is then a device-scope atomic or a volatile access (the workgroup's L1 is never trusted)
template <bool GLOBAL>
__global__ __launch_bounds__(1024) void agc_cc_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  const int min_size = w.min_size;
  int32_t* __restrict__ kept = w.kept;
  int32_t* info = w.info;
  extern __shared__ int32_t sm[];
  int32_t* parent = GLOBAL ? w.members : sm;
  int32_t* count = GLOBAL ? w.nnc : sm + w.n;
  auto cnt_of = [&](int x) { return __hip_atomic_load(&count[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  __shared__ int wsum[16];
  __shared__ int carry[2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = w.n;
  for (int u = t; u < n; u += 1024) {
    __hip_atomic_store(&parent[u], u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&count[u], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  volatile int32_t* vp = parent;
  auto find = [&](int x) {
    for (;;) {
      const int p = vp[x];
      if (p == x) return x;
      const int g = vp[p];
      if (g != p) vp[x] = g;   // path compression step (benign race: g is always an ancestor of x)
      x = p;
    }
  };
  // ONE pass over the edges: a lock-free union (hook the larger root under the smaller one by compare-and-swap, retry when the root was taken
  // meanwhile).  Roots only ever move to smaller indices, so a component's final root is its smallest node whatever the interleaving -- the
  // labels are the same as the min-label propagation this replaces, which rescanned all edges until a pass changed nothing (three scans of
  // ~50 us each at 4096 nodes: 160 -> 65 us).
  // ... over the EDGE LIST (source row, neighbour), four entries per thread and step with their loads in flight together: walking the rows
  // (ptr0 -> idx0 -> union, a chain of dependent global loads per edge) was 80 us per image of 4096, most of it memory latency
  {
    const int E = w.ptr0[n] < w.cap ? w.ptr0[n] : w.cap;
    for (int e0 = t; e0 < E; e0 += 4 * 1024) {
      int us[4], vs[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = e0 + q * 1024;
        us[q] = e < E ? w.esrc[e] : 0;
        vs[q] = e < E ? w.idx0[e] : 0;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int u = us[q], v = vs[q];
        if (v <= u) continue;   // each undirected edge once (and the padding of the last step)
        for (;;) {
          const int ru = find(u), rv = find(v);
          if (ru == rv) break;
          const int hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
          if (atomicCAS(&parent[hi], hi, lo) == hi) break;     // hi was still a root: hooked
        }
      }
    }
  }
  __syncthreads();
  for (int u = t; u < n; u += 1024) {
    const int x = find(u);
    w.label[u] = x;
    atomicAdd(&count[x], 1);
  }
  __syncthreads();
  // ordered compaction of alive nodes (kept) and of alive roots (component ranks)
  if (t == 0) { carry[0] = 0; carry[1] = 0; }
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int u = base + t;
    bool al = false, root = false;
    if (u < n) {
      const int l = w.label[u];
      al = cnt_of(l) >= min_size;
      root = al && l == u;
      w.alive[u] = al ? 1 : 0;
    }
    const uint64_t ma = __ballot(al), mr = __ballot(root);
    const uint64_t lt = (1ull << lane) - 1;
    if (lane == 0) wsum[wave] = __popcll(ma) | (__popcll(mr) << 16);
    __syncthreads();
    int offa = carry[0], offr = carry[1];
    for (int q = 0; q < wave; ++q) { offa += wsum[q] & 0xffff; offr += wsum[q] >> 16; }
    if (u < n) {
      const int id = al ? offa + __popcll(ma & lt) : -1;
      w.newid[u] = id;
      if (al) kept[id] = u;
      w.crank[u] = root ? offr + __popcll(mr & lt) : -1;
    }
    __syncthreads();
    if (t == 0) {
      int sa = 0, sr = 0;
      for (int q = 0; q < 16; ++q) { sa += wsum[q] & 0xffff; sr += wsum[q] >> 16; }
      carry[0] += sa; carry[1] += sr;
    }
    __syncthreads();
  }
  // component offsets (size of each alive component, in rank order)
  for (int u = t; u < n; u += 1024) {
    const int r = w.crank[u];
    if (r >= 0) w.coff[r] = cnt_of(u);   // temporarily sizes
  }
  if (t == 0) {
    info[0] = carry[0];
    info[4] = carry[1];
    w.counters[1] = carry[1];
  }
}

// ---------------------------------------------------------------------------------------------- K6 linking
// members of each alive component in ascending node order + float64 centroid (one wave per component)
template <int NWV>      // waves per workgroup: 4 up to 16384 nodes, 8 above (a wave's share is at most 64 chunks of 64 nodes: one mask word)
__global__ __launch_bounds__(64 * NWV) void agc_members_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  const float* __restrict__ kpts = w.kpts;
  const int32_t* __restrict__ coff = w.coff2;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int C = w.counters[1];
  // One WORKGROUP per component (there are usually one to a handful; a small grid walks them): the four waves take one quarter of the node range
  // each -- a single wave walking all nodes with three dependent loads per chunk (alive -> label -> rank) was 67 us of pure latency per image.
  // Pass 1 finds the members of the quarter (kept as one bit per chunk and lane) and counts them, the counts give every wave its offset, pass 2
  // writes the members in ascending order and sums their coordinates in float64.
  __shared__ int wcnt[NWV];
  __shared__ double part[NWV][2];
  const int per = ((w.n + NWV - 1) / NWV + 63) & ~63;         // nodes per wave, a multiple of 64 (<= 4096: at most 64 chunks)
  const int u0 = wave * per, u1 = (u0 + per < w.n) ? u0 + per : w.n;
  for (int c = blockIdx.x; c < C; c += gridDim.x) {
    uint64_t mine = 0;                                         // bit k: node u0 + 64 k + lane belongs to component c
    int cnt = 0;
    for (int base = u0, k = 0; base < u1; base += 256, k += 4) {
      bool mem[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {                            // four chunks in flight
        const int u = base + 64 * q + lane;
        int lab = 0;
        const bool al = u < u1 && w.alive[u] != 0;
        if (al) lab = w.label[u];
        mem[q] = al && w.crank[lab] == c;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (mem[q]) mine |= 1ull << (k + q);
        cnt += __popcll(__ballot(mem[q]));
      }
    }
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    int off = coff[c];
    for (int q = 0; q < wave; ++q) off += wcnt[q];
    int total = 0;
#pragma unroll
    for (int q = 0; q < NWV; ++q) total += wcnt[q];
    double sx = 0.0, sy = 0.0;
    for (int base = u0, k = 0; base < u1; base += 64, ++k) {
      const bool mem = (mine >> k) & 1ull;
      const uint64_t m = __ballot(mem);
      if (mem) {
        const int u = base + lane;
        w.members[off + __popcll(m & ((1ull << lane) - 1))] = u;
        sx += (double)kpts[2 * u];
        sy += (double)kpts[2 * u + 1];
      }
      off += __popcll(m);
    }
    sx = wave_sum_f64(sx);
    sy = wave_sum_f64(sy);
    if (lane == 0) { part[wave][0] = sx; part[wave][1] = sy; }
    __syncthreads();
    if (threadIdx.x == 0) {
      double sx4 = part[0][0], sy4 = part[0][1];          // left to right
#pragma unroll
      for (int q = 1; q < NWV; ++q) { sx4 += part[q][0]; sy4 += part[q][1]; }
      w.cent[2 * c] = sx4 / (double)total;
      w.cent[2 * c + 1] = sy4 / (double)total;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void agc_nnc_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + wave;
  const int C = w.counters[1];
  if (c >= C) return;
  const double cx = w.cent[2 * c], cy = w.cent[2 * c + 1];
  double bd = 1e300;
  int bj = 0x7fffffff;
  for (int j = lane; j < C; j += 64) {
    if (j == c) continue;
    const double dx = w.cent[2 * j] - cx, dy = w.cent[2 * j + 1] - cy;
    const double dd = dx * dx + dy * dy;
    if (dd < bd) { bd = dd; bj = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(bd, o, 64);
    const int oj = __shfl_xor(bj, o, 64);
    if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
  }
  if (lane == 0) w.nnc[c] = bj;
}

// one workgroup per component i: closest (v in comp nn(i), u in comp i) pair, lexicographic (d2, v, u)
__global__ __launch_bounds__(256) void agc_link_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  const float* __restrict__ kpts = w.kpts;
  const int32_t* __restrict__ coff = w.coff2;
  __shared__ double sd[256];
  __shared__ int sv[256], su[256];
  const int t = threadIdx.x;
  const int C = w.counters[1];
  if (C <= 1) return;
  for (int i = blockIdx.x; i < C; i += gridDim.x) {      // (a workgroup per POSSIBLE component was 65 k workgroups that only exited: 70 us)
  const int j = w.nnc[i];
  // agc.py:550-552: skip when the reverse pair was linked earlier (j < i and nn(j) == i)
  if (j < i && w.nnc[j] == i) {
    if (t == 0) { w.link[2 * i] = -1; w.link[2 * i + 1] = -1; }
    continue;
  }
  const int ai = coff[i], na = coff[i + 1] - ai;
  const int aj = coff[j], nb = coff[j + 1] - aj;
  double bd = 1e300;
  int bv = 0x7fffffff, bu = 0x7fffffff;
  // every (v, u) pair once; the lexicographic minimum of (d2, v, u) does not depend on the visiting order.  The LARGER member list runs across the
  // threads (its points loaded once per thread and kept), the smaller one is walked by every thread -- no index arithmetic per pair (a flat
  // pair index cost a 64-bit division and four dependent loads per pair: 63 us for one 4000 x 10 product)
  const bool swap = nb > na;
  const int big0 = swap ? aj : ai, nbig = swap ? nb : na, small0 = swap ? ai : aj, nsmall = swap ? na : nb;
  for (int p = t; p < nbig; p += 256) {
    const int pb = w.members[big0 + p];
    const double bx = (double)kpts[2 * pb], by = (double)kpts[2 * pb + 1];
    for (int q = 0; q < nsmall; ++q) {
      const int ps = w.members[small0 + q];
      const double dx = bx - (double)kpts[2 * ps], dy = by - (double)kpts[2 * ps + 1];
      const double dd = dx * dx + dy * dy;                   // (u - v)^2 == (v - u)^2 bit for bit: the roles of the two lists do not matter
      const int v = swap ? pb : ps, u = swap ? ps : pb;
      if (dd < bd || (dd == bd && (v < bv || (v == bv && u < bu)))) { bd = dd; bv = v; bu = u; }
    }
  }
  sd[t] = bd; sv[t] = bv; su[t] = bu;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      const double od = sd[t + s];
      const int ov = sv[t + s], ou = su[t + s];
      if (od < sd[t] || (od == sd[t] && (ov < sv[t] || (ov == sv[t] && ou < su[t])))) { sd[t] = od; sv[t] = ov; su[t] = ou; }
    }
    __syncthreads();
  }
  if (t == 0) { w.link[2 * i] = su[0]; w.link[2 * i + 1] = sv[0]; }
  __syncthreads();
  }
}

__global__ __launch_bounds__(256) void agc_link_apply_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  int32_t* info = w.info;
  const int C = w.counters[1];
  if (C <= 1) { if (threadIdx.x == 0 && blockIdx.x == 0) info[5] = 0; return; }
  int added = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < C; i += gridDim.x * 256) {
    const int u = w.link[2 * i], v = w.link[2 * i + 1];
    if (u < 0) continue;
    atomicOr((unsigned long long*)&w.bits[(int64_t)u * w.nw + (v >> 6)], 1ull << (v & 63));
    atomicOr((unsigned long long*)&w.bits[(int64_t)v * w.nw + (u >> 6)], 1ull << (u & 63));
    ++added;
  }
  if (added) atomicAdd(&info[5], added);
}

__global__ void agc_finish_kernel(const AgcWs* __restrict__ ws, int window) {
  const AgcWs& w = ws[blockIdx.y];
  int32_t* info = w.info;
  const int max_edges_dir = w.max_edges_dir;
  info[2] = w.counters[0] / 2;
  info[6] = (int32_t)__float_as_uint(key_f32(w.sel[0]));
  info[7] = (info[1] > max_edges_dir || w.counters[0] > w.cap || w.counters[2] > w.cap) ? 1 : 0;
  if ((uint32_t)w.counters[4] > w.clist_cap) {       // more radius candidates than the list holds: like an edge overflow (the caller
    info[7] = 1;                                                // repeats the build with larger buffers), sized from the candidate count
    info[2] = w.counters[4];
  }
  if (window) {       // the window was a prediction (agc_window_kernel): the threshold it produced stands only if the window provably held rank k
    const float thr = key_f32(w.sel[0]), vL = __uint_as_float(w.band[0]), vU = __uint_as_float(w.band[1]), eps = __uint_as_float(w.band[2]);
    if (w.counters[7] || !(thr >= vL + eps && thr <= vU - eps)) info[7] |= 2;
  } else {            // robust flow: the same post-check against the measured error bound (agc_band_kernel); a failure here is an error, not a retry
    const float thr = key_f32(w.sel[0]);
    if (w.counters[7] || !(thr >= __uint_as_float(w.band[2]) && thr <= __uint_as_float(w.band[3]))) info[7] |= 2;
  }
}

// degree by kept id (rows past n_kept get 0 so that the scan over n entries ends at the edge total)
__global__ __launch_bounds__(256) void agc_kept_deg_kernel(const AgcWs* __restrict__ ws) {
  const AgcWs& w = ws[blockIdx.y];
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= w.n) return;
  const int id = w.newid[u];
  if (id >= 0) w.degk[id] = w.deg[u];
  if (u >= w.info[0]) w.degk[u] = 0;
}

// The scratch CSR of the pre-removal graph gets the capacity the caller gives the final one (gims_agc_image::max_edges_dir,
// at least 64 directed edges per node): a caller that sees the overflow flag repeats the build with larger output buffers.
constexpr int AGC_MIN_CAP_PER_NODE = 64;

// One image's part of the workspace (sizing: L on a null base, w a scratch record)
static void agc_layout(int n, int d, int max_edges_dir, bool with_s16, WsLayout& L, AgcWs& w) {
  const int nw = (n + 63) / 64, lds16 = (n + 7) & ~7;
  const int cap = max_edges_dir > n * AGC_MIN_CAP_PER_NODE ? max_edges_dir : n * AGC_MIN_CAP_PER_NODE;
  // descriptors: [n][d] f32 followed by [n][d] half
  char* dn = L.take<char>((size_t)n * d * 6);
  w.dnf = (float*)dn;
  w.dn16 = dn ? (uint16_t*)(dn + (size_t)n * d * 4) : nullptr;
  // approximate similarities in half [n][lds16] (robust flow only: the window flow never stores them), the radius candidates and their keys, and the
  // band list (one u32 per pair of the strict upper triangle at most)
  const size_t list_cap = (size_t)n * (n - 1) / 2 + 64;
  w.S16 = with_s16 ? L.take<uint16_t>((size_t)n * lds16) : nullptr;
  w.clist = L.take<uint32_t>(cap);
  w.ckey = L.take<uint32_t>(cap);
  w.list = L.take<uint32_t>(list_cap);
  w.list_cap = (uint32_t)list_cap;
  w.clist_cap = (uint32_t)cap;
  w.lds16 = lds16;
  w.cellptr = L.take<int32_t>(AGC_NB + 1);
  w.cellidx = L.take<int32_t>(n);
  w.bits = L.take<uint64_t>((size_t)n * nw);
  w.hist = L.take<uint32_t>(4096);
  w.sel = L.take<uint32_t>(4);
  w.band = L.take<uint32_t>(4);
  w.deg = L.take<int32_t>(n);
  w.nn = L.take<int32_t>(n);
  w.label = L.take<int32_t>(n);
  w.alive = L.take<int32_t>(n);
  w.newid = L.take<int32_t>(n);
  w.crank = L.take<int32_t>(n);
  w.coff = L.take<int32_t>(n + 1);
  w.members = L.take<int32_t>(n);
  w.nnc = L.take<int32_t>(n);
  w.link = L.take<int32_t>((size_t)n * 2);
  w.cent = L.take<double>((size_t)n * 2);
  w.ptr0 = L.take<int32_t>(n + 1);
  w.idx0 = L.take<int32_t>(cap);
  w.esrc = L.take<int32_t>(cap);
  w.counters = L.take<int32_t>(16);
  w.coff2 = L.take<int32_t>(n + 1);
  w.degk = L.take<int32_t>(n);
  w.n = n; w.d = d; w.nw = nw; w.cap = cap;
}

// The whole workspace: the AgcWs table, then image after image.  recs == nullptr: sizing only.
static void agc_batch_layout(const gims_agc_image* images, int n_images, bool robust, WsLayout& L, AgcWs* recs) {
  L.take<AgcWs>(n_images);
  AgcWs scratch;
  for (int i = 0; i < n_images; ++i) agc_layout(images[i].n, images[i].d, images[i].max_edges_dir, robust, L, recs ? recs[i] : scratch);
}

}  // namespace gims

// which flow a call takes: the robust one when asked for (flag or GIMS_AGC_ROBUST=1) or when an image's descriptor width does not fit the
// window kernels (they keep a tile row's whole K in registers); only that flow stores the half similarity matrix
static bool agc_takes_robust_flow(const gims_agc_image* images, int n_images, int flags) {
  bool robust = (flags & GIMS_AGC_ROBUST) != 0 || gims::env_int("GIMS_AGC_ROBUST", 0) != 0;          // read per call: the tests switch flows
  for (int i = 0; i < n_images; ++i) robust = robust || images[i].d % gims::SW_KC != 0 || images[i].d > gims::SW_KMAX;
  return robust;
}

extern "C" size_t gims_agc_workspace_bytes(const gims_agc_image* images, int32_t n_images, int32_t flags) {
  using namespace gims;
  if (!images || n_images <= 0) return 0;
  const bool robust = agc_takes_robust_flow(images, n_images, flags);
  WsLayout L(nullptr);
  agc_batch_layout(images, n_images, robust, L, nullptr);
  return L.bytes();
}

extern "C" int32_t gims_agc_max_keypoints(void) { return gims::AGC_MAX_N; }

// n_params == 1: one (radius, percentile, min_size) for every image; n_params == n_images: params[i] belongs to images[i]
extern "C" int gims_agc_build(const gims_agc_image* images, int32_t n_images, const gims_agc_params* params, int32_t n_params, int32_t flags,
                              void* work, size_t work_bytes, void* stream) {
  using namespace gims;
  GIMS_CHECK_ARG(images && n_images > 0 && work, "gims_agc_build: null / empty arguments");
  GIMS_CHECK_ARG(params && (n_params == 1 || n_params == n_images), "gims_agc_build: h_params is null or n_params=%d is neither 1 nor n_images=%d",
                 n_params, n_images);
  // GIMS_AGC_ROBUST=1 / GIMS_AGC_WINDOW_SHIFT=<x> (read per call: the tests switch flows and force a missed window)
  const bool robust = agc_takes_robust_flow(images, n_images, flags);
  const char* env_shift = getenv("GIMS_AGC_WINDOW_SHIFT");
  const float window_test_shift = env_shift ? (float)atof(env_shift) : 0.f;
  for (int i = 0; i < n_images; ++i) {
    const gims_agc_image& im = images[i];
    GIMS_CHECK_ARG(im.kpts && im.desc && im.kept && im.indptr && im.indices && im.info, "gims_agc_build: image %d has a null pointer", i);
    GIMS_CHECK_ARG(im.n >= 2 && im.n <= AGC_MAX_N, "gims_agc_build: image %d: n=%d out of range [2, %d] (gims_agc_max_keypoints)", i, im.n, AGC_MAX_N);
    static_assert(AGC_MAX_N <= (1 << AGC_PK_SHIFT), "the band list packs a pair as i << 16 | j");
    GIMS_CHECK_ARG(im.d > 0 && (im.d % 32) == 0 && (im.ldd % 4) == 0, "gims_agc_build: image %d: d=%d must be a multiple of 32 (ldd %% 4 == 0)", i, im.d);
  }
  std::vector<AgcWs> hws(n_images);
  WsLayout lay(work);
  agc_batch_layout(images, n_images, robust, lay, hws.data());
  GIMS_CHECK_ARG(work_bytes >= lay.bytes(), "gims_agc_build: workspace too small (%zu bytes; gims_agc_workspace_bytes asks for %zu for the %s flow)", work_bytes,
                 lay.bytes(), robust ? "robust" : "window");
  hipStream_t s = (hipStream_t)stream;
  AgcWs* dws = (AgcWs*)work;
  int maxn = 0, maxnw = 0;
  for (int i = 0; i < n_images; ++i) {
    const gims_agc_image& im = images[i];
    AgcWs* w = &hws[i];
    w->kpts = im.kpts; w->desc = im.desc; w->ldd = im.ldd; w->kept = im.kept; w->indptr = im.indptr; w->indices = im.indices;
    w->info = im.info; w->max_edges_dir = im.max_edges_dir;
    const gims_agc_params& pm = params[n_params == 1 ? 0 : i];
    // K2 rank: k = int(L * p / 100), clamped (agc.py:378-379)
    const int64_t L = (int64_t)im.n * (im.n - 1) / 2;
    int64_t k = (int64_t)(((double)L * pm.percentile) / 100.0);
    if (k >= L) k = L - 1;
    if (k < 0) k = 0;
    w->krank = k;
    // radius candidates go through a keypoint grid of cell side 1.001 |r|, never below 1e-3 (a larger cell only costs tests); an infinite radius
    // puts every point into one cell (every pair is tested: what the predicate asks for), a NaN radius keeps no pair (agc.py:443: d2 <= r2 is False)
    double side = fabs(pm.radius) * 1.001;
    if (!(side >= 1e-3)) side = 1e-3;
    w->r2 = pm.radius * pm.radius;
    w->inv_side = 1.0 / side;
    w->min_size = pm.min_size;
    maxn = im.n > maxn ? im.n : maxn;
    maxnw = w->nw > maxnw ? w->nw : maxnw;
  }
  // (every argument is validated before the first call into the HIP runtime)
  GIMS_LDS_ATTR((const void*)agc_cc_kernel<false>, AGC_CC_LDS_N * 8);
  GIMS_LDS_ATTR((const void*)agc_iso_seq_kernel, AGC_MAX_N * 4 + (AGC_MAX_N / 32 + 2) * 4);
  const int B = n_images;
  {
    const int rc = upload_table(hws.data(), sizeof(AgcWs) * (size_t)B, dws, s);
    if (rc != GIMS_OK) return rc;
    hipLaunchKernelGGL(agc_init_kernel, dim3(1, B), dim3(256), 0, s, dws);
  }
  const dim3 gw(cdiv(maxn, 4), B), g1(1, B);
  // K1
  hipLaunchKernelGGL(agc_normalize_kernel, gw, dim3(256), 0, s, dws);
  {
    const int T = cdiv(maxn, S16_T), ntiles = T * (T + 1) / 2;
    if (robust) {
      // approximate matrix (half, one MFMA pass, every entry histogrammed) -> bracket of the k-th value -> band entries
      GIMS_LDS_ATTR((const void*)agc_sim16_kernel, S16_LDS_BYTES);
      // two workgroups per CU, the images dealt to the XCDs (agc_nparts); a small batch of small images takes fewer workgroups
      const int nparts = 8 / (((B & -B) > 8) ? 8 : (B & -B)), per_xcd = cdiv(B * nparts, 8) * cdiv(ntiles, nparts);
      const int sgrid = 8 * (per_xcd < 2 * (device_cus() / 8) ? per_xcd : 2 * (device_cus() / 8));
      // ~4096 workgroups in total for the sweep: each folds its LDS staging buffer into the global list
      int hgrid = 4096 / B;
      hgrid = hgrid < 16 ? 16 : (hgrid > 1024 ? 1024 : hgrid);
      hgrid = hgrid < maxn ? hgrid : maxn;
      hipLaunchKernelGGL(agc_sim16_kernel, dim3(sgrid), dim3(256), S16_LDS_BYTES, s, dws, B);
      hipLaunchKernelGGL(agc_band_kernel, g1, dim3(256), 0, s, dws);
      hipLaunchKernelGGL(agc_sweep16_kernel, dim3(hgrid, B), dim3(256), 0, s, dws, 1);
    } else {
      // a sample of the approximate similarities predicts the window that holds the k-th value; ONE pass over all of them counts what lies
      // below it and lists what lies inside it; nothing of the N x N matrix is ever stored.  Two workgroups per CU.
      GIMS_LDS_ATTR((const void*)agc_simw_kernel<SIM_SAMPLE>, SW_LDS_BYTES);
      GIMS_LDS_ATTR((const void*)agc_simw_kernel<SIM_COLLECT>, SW_LDS_BYTES);
      const int wgrid = 8 * 2 * (device_cus() / 8);
      hipLaunchKernelGGL(agc_simw_kernel<SIM_SAMPLE>, dim3(wgrid), dim3(256), SW_LDS_BYTES, s, dws, B);
      hipLaunchKernelGGL(agc_window_kernel, g1, dim3(256), 0, s, dws, window_test_shift);
      hipLaunchKernelGGL(agc_simw_kernel<SIM_COLLECT>, dim3(wgrid), dim3(256), SW_LDS_BYTES, s, dws, B);
    }
    // radius candidates through each image's keypoint grid (cell side and squared radius: in its record)
    GIMS_LDS_ATTR((const void*)agc_grid_kernel, AGC_NB * 4);
    hipLaunchKernelGGL(agc_grid_kernel, g1, dim3(1024), AGC_NB * 4, s, dws);
    hipLaunchKernelGGL(agc_radius_grid_kernel, dim3(cdiv(maxn, 32), B), dim3(288), 0, s, dws);
    // the exact values of the listed entries and of the radius candidates, then the exact k-th among the former
    hipLaunchKernelGGL(agc_exact_kernel, dim3(8 * 4 * (device_cus() / 8)), dim3(256), 0, s, dws, B, robust ? 0 : 1);
    const int lgrid = 1024 / B < 4 ? 4 : (1024 / B > 64 ? 64 : 1024 / B);
    hipLaunchKernelGGL(agc_hist_kernel, dim3(lgrid, B), dim3(256), 0, s, dws, 20, 12);
    hipLaunchKernelGGL(agc_pick_kernel, g1, dim3(256), 0, s, dws, 20, 12);
    hipLaunchKernelGGL(agc_hist_kernel, dim3(lgrid, B), dim3(256), 0, s, dws, 8, 12);
    hipLaunchKernelGGL(agc_pick_kernel, g1, dim3(256), 0, s, dws, 8, 12);
    hipLaunchKernelGGL(agc_hist_kernel, dim3(lgrid, B), dim3(256), 0, s, dws, 0, 8);
    hipLaunchKernelGGL(agc_pick_kernel, g1, dim3(256), 0, s, dws, 0, 8);
  }
  // K3
  hipLaunchKernelGGL(agc_apply_kernel, dim3(16, B), dim3(256), 0, s, dws);
  hipLaunchKernelGGL(agc_deg_kernel, dim3(cdiv(maxn, 16), B), dim3(256), 0, s, dws, 1);
  // K4
  hipLaunchKernelGGL(agc_iso_nn_kernel, gw, dim3(256), 0, s, dws);
  const size_t iso_lds = (size_t)maxn * 4 + ((size_t)(maxn + 31) / 32 + 1) * 4;
  hipLaunchKernelGGL(agc_iso_seq_kernel, g1, dim3(1024), iso_lds, s, dws);
  // CSR of the pre-removal graph (original ids) for the component search
  hipLaunchKernelGGL(agc_deg_kernel, dim3(cdiv(maxn, 16), B), dim3(256), 0, s, dws, 0);
  hipLaunchKernelGGL(agc_scan_kernel, g1, dim3(1024), 0, s, dws, 0);
  hipLaunchKernelGGL(agc_fill_kernel, dim3(cdiv(maxn, 16), B), dim3(256), 0, s, dws, 0);
  // K5
  if (maxn <= AGC_CC_LDS_N) hipLaunchKernelGGL(agc_cc_kernel<false>, g1, dim3(1024), (size_t)maxn * 8, s, dws);
  else hipLaunchKernelGGL(agc_cc_kernel<true>, g1, dim3(1024), 0, s, dws);
  // K6: component sizes -> offsets; members, centroids, nearest component, links
  hipLaunchKernelGGL(agc_scan_kernel, g1, dim3(1024), 0, s, dws, 1);
  if (maxn <= 16384) hipLaunchKernelGGL(agc_members_kernel<4>, dim3(32, B), dim3(256), 0, s, dws);
  else hipLaunchKernelGGL(agc_members_kernel<8>, dim3(32, B), dim3(512), 0, s, dws);
  hipLaunchKernelGGL(agc_nnc_kernel, gw, dim3(256), 0, s, dws);
  hipLaunchKernelGGL(agc_link_kernel, dim3(maxn < 256 ? maxn : 256, B), dim3(256), 0, s, dws);
  hipLaunchKernelGGL(agc_link_apply_kernel, dim3(cdiv(maxn, 256), B), dim3(256), 0, s, dws);
  // K7: final CSR over the kept nodes, relabelled in sorted order
  hipLaunchKernelGGL(agc_deg_kernel, dim3(cdiv(maxn, 16), B), dim3(256), 0, s, dws, 0);
  hipLaunchKernelGGL(agc_kept_deg_kernel, dim3(cdiv(maxn, 256), B), dim3(256), 0, s, dws);
  hipLaunchKernelGGL(agc_scan_kernel, g1, dim3(1024), 0, s, dws, 2);
  hipLaunchKernelGGL(agc_fill_kernel, dim3(cdiv(maxn, 16), B), dim3(256), 0, s, dws, 1);
  hipLaunchKernelGGL(agc_finish_kernel, g1, dim3(1), 0, s, dws, robust ? 0 : 1);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}
