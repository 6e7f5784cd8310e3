// Which image pairs to match: GIMS_AUX_SELECT_PAIRS of gims_run_ops pre-matches a few hundred int8-quantised descriptors of
// every image against those of every other image, lets every row vote (Lowe's ratio test on the two smallest squared distances, in
// integers) and keeps, per image, the k partners with the most votes.  include/gims_hip.h has the contract; tests/pairs_ref.py is the NumPy
// restatement.  Every decision is an integer one: the outputs are a function of the inputs alone, whatever the order of the sums.
//
// Stages, each a launch of its own on the stream:  table upload -> maxabs (without a given scale) -> quantise (gather the selected rows into
// the pooled int8 matrix Q and |q|^2) -> vote (the hot path: i8 MFMA, two smallest per (row, image), one integer add per (32 rows, image)) ->
// select (top k of a row of S = votes + votes^T, marks in an N x N byte map) -> row counts -> scan -> fill.
//
// The pool.  Image i owns P_i = m_i rounded up to 32 rows at pstart_i = P_0 + ... + P_(i-1); the pool ends on a multiple of 128 rows.  A block
// of 32 pooled rows therefore belongs to ONE image (blk_img, -1 behind the last image), which makes the self test and the vote count
// wave-uniform.  A row that is padding, or whose selected index is out of range, is all zeros with |q|^2 = PAIRS_NO_ROW = 2^30: as a neighbour
// its distance exceeds every real one (<= 4 * 127^2 * 1024 < 2^26), as a query it is recognised by that norm and does not vote.
#include "common.h"

#include <math.h>
#include <string.h>

#include <vector>

namespace gims {

constexpr int PRS_THREADS = 256;                               // 4 waves
constexpr int PRS_BLOCK = 32;                                  // pooled rows per MFMA block: one image per block
constexpr int PRS_TILE = GIMS_PAIRS_QUERY_TILE;                // pooled rows per workgroup of the vote kernel: a block per wave
constexpr int PRS_WORDS = GIMS_PAIRS_TABLE_WORDS;              // int64 words per table entry
constexpr int PRS_NO_ROW = 1 << 30;                            // |q|^2 of a row that does not exist
constexpr int PRS_NO_DIST = 1 << 29;                           // a (distance - |q_r|^2) at or above this involves a row that does not exist
constexpr int PRS_VOTE_GROUPS = 2048;                          // the vote grid aims at this many workgroups (a constant: the launch is a host fact)
constexpr int PRS_SCAN_THREADS = 1024;
constexpr int PRS_MAXABS_ROWS = 8;                             // pooled rows per wave of the maxabs kernel
static_assert(PRS_TILE == PRS_BLOCK * (PRS_THREADS / 64), "a query tile is one block of 32 rows per wave");
enum { PRS_N_PAIRS = 0, PRS_N_ROWS, PRS_N_SHORT, PRS_N_BAD_ROWS, PRS_N_NONFINITE, PRS_COUNTERS = 8 };

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

static inline int64_t prs_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
static inline int prs_dp(int d) { int p = 32; while (p < d) p <<= 1; return p; }        // the channel count of Q: D up to a power of two, zeros behind D
// the rows of the pooled matrix: every image's m (m[0], m[stride], ...) up to a whole block, the whole up to a query tile (at least one)
static inline int64_t prs_pool(const int64_t* m, int64_t stride, int64_t n) {
  int64_t pool = 0;
  for (int64_t i = 0; i < n; ++i) pool += prs_up(m[stride * i], PRS_BLOCK);
  return prs_up(pool > 0 ? pool : 1, PRS_TILE);
}

// The workspace (the formula of include/gims_hip.h; gims_aux_layout reports this routine's offsets)
struct PrsWs {
  uint32_t* head;              // {maxabs bits, scale bits, n_bad_rows, 0, non-finite count lo, hi}
  int64_t* tab;                // [N][8]: the caller's table with word 5 = pstart_i and word 6 = P_i
  int32_t* blk_img;            // [pool / 32]
  int8_t* q;                   // [pool][Dp]
  int32_t* norms;              // [pool]
  uint8_t* map;                // [N][N]
  int32_t *rowcnt, *rowoff;    // [N]
};
static size_t prs_layout(void* base, int64_t n, int64_t pool, int dp, PrsWs& w, WsRecord* rec = nullptr) {
  WsLayout L(base, rec);
  w.head = L.take<uint32_t>(8);
  w.tab = L.take<int64_t>((size_t)n * PRS_WORDS);
  w.blk_img = L.take<int32_t>((size_t)(pool / PRS_BLOCK));
  w.q = L.take<int8_t>((size_t)pool * dp);
  w.norms = L.take<int32_t>((size_t)pool);
  w.map = L.take<uint8_t>((size_t)n * n);
  w.rowcnt = L.take<int32_t>((size_t)n);
  w.rowoff = L.take<int32_t>((size_t)n);
  return L.bytes();
}

__device__ __forceinline__ int prs_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the source row of pooled row `row`: nullptr when the row is padding or its selected index is outside its image (bad = true then)
__device__ __forceinline__ const float* prs_source(const int64_t* __restrict__ tab, const int32_t* __restrict__ blk_img, int row, bool& bad) {
  bad = false;
  const int img = blk_img[row / PRS_BLOCK];
  if (img < 0) return nullptr;
  const int64_t* e = tab + (int64_t)PRS_WORDS * img;
  const int local = row - (int)e[5];
  if (local >= (int)e[4]) return nullptr;
  const int32_t* idx = (const int32_t*)(uintptr_t)e[3];
  const int64_t src = idx ? (int64_t)idx[local] : (int64_t)local;
  if (src < 0 || src >= e[2]) {
    bad = true;
    return nullptr;
  }
  return (const float*)(uintptr_t)e[0] + src * e[1];
}

// ---------------------------------------------------------------------------------------------- maxabs
// A wave per PRS_MAXABS_ROWS pooled rows, a workgroup per block of 32.  The largest |x| over the finite selected values as an integer maximum on
// the float bits (positive floats order like their bit patterns), as nn_norms_kernel does.  One atomic per workgroup, and only when it can
// raise the value: the word only grows, so a stale read costs an atomic that changes nothing, never a missed maximum.
__global__ __launch_bounds__(PRS_THREADS) void pairs_maxabs_kernel(const int64_t* __restrict__ tab, const int32_t* __restrict__ blk_img, int pool, int d,
                                                                  uint32_t* head) {
  __shared__ uint32_t part[PRS_THREADS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t m = 0;
  for (int k = 0; k < PRS_MAXABS_ROWS; ++k) {
    const int row = (blockIdx.x * (PRS_THREADS / 64) + w) * PRS_MAXABS_ROWS + k;
    if (row >= pool) break;
    bool bad;
    const float* src = prs_source(tab, blk_img, row, bad);
    if (!src) continue;
    for (int c = lane; c < d; c += 64) {
      const uint32_t a = __float_as_uint(src[c]) & 0x7fffffffu;
      if (a < 0x7f800000u) m = a > m ? a : m;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t x = (uint32_t)__shfl_xor((int)m, o, 64);
    m = x > m ? x : m;
  }
  if (lane == 0) part[w] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < PRS_THREADS / 64; ++k) m = part[k] > m ? part[k] : m;
    if (m > __hip_atomic_load(head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(head + 0, m);
  }
}

// ---------------------------------------------------------------------------------------------- quantise
// A wave per pooled row, a lane per four channels: q = clamp(rintf(x * s), -127, 127), non-finite x as 0; |q|^2; the counters of what was
// not usable.  s = the given scale, or 127.0f / maxabs (0 when maxabs is 0); it is kept in head[1].
__global__ __launch_bounds__(PRS_THREADS) void pairs_quantise_kernel(const int64_t* __restrict__ tab, const int32_t* __restrict__ blk_img, int pool, int d,
                                                                    int dp, int scale_given, float scale, uint32_t* head, int8_t* __restrict__ q,
                                                                    int32_t* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (PRS_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= pool) return;
  float s = scale;
  if (!scale_given) {
    const uint32_t mb = head[0];                               // (final: the launch that raised it precedes this one)
    s = mb ? 127.0f / __uint_as_float(mb) : 0.0f;
  }
  if (row == 0 && lane == 0) head[1] = __float_as_uint(s);
  bool bad;
  const float* src = prs_source(tab, blk_img, row, bad);
  uint32_t* out = (uint32_t*)(q + (int64_t)row * dp);
  int norm = 0, nonfinite = 0;
  for (int c4 = lane; c4 < dp / 4; c4 += 64) {
    uint32_t word = 0;
    if (src) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = 4 * c4 + k;
        int v = 0;
        if (c < d) {
          const float x = src[c];
          if ((__float_as_uint(x) & 0x7fffffffu) >= 0x7f800000u) {
            ++nonfinite;
          } else {
            float p = rintf(x * s);
            p = p == p ? p : 0.0f;                             // (0 * inf, when 127 / maxabs overflows: nothing)
            p = fminf(fmaxf(p, -127.0f), 127.0f);
            v = (int)p;
          }
        }
        norm += v * v;
        word |= (uint32_t)(v & 0xff) << (8 * k);
      }
    }
    out[c4] = word;
  }
  norm = prs_wave_sum(norm);
  nonfinite = prs_wave_sum(nonfinite);
  if (lane == 0) {
    norms[row] = src ? norm : PRS_NO_ROW;
    if (bad) atomicAdd(head + 2, 1u);
    if (nonfinite) atomicAdd((unsigned long long*)(head + 4), (unsigned long long)nonfinite);
  }
}

// ---------------------------------------------------------------------------------------------- vote
// The hot path.  A workgroup takes a query tile of 128 pooled rows, a wave one block of 32 (one image i), and walks the database images j =
// blockIdx.y, blockIdx.y + gridDim.y, ...  The queries are the COLUMN operand of v_mfma_i32_32x32x32_i8 and the database rows the ROW operand
// (the orientation of nn_candidate_kernel): lane l owns query l & 31, and its 16 accumulators are 16 database rows
// ((reg & 3) + 8 (reg >> 2) + 4 (l >> 5)) of THAT query, so the running two smallest of a query are two registers of the lane and the loop
// holds no cross-lane traffic.  The wave's query fragments stay in registers (4 per 32 channels) for all of its images; the database rows of a
// step, 32 at a time with their norms, go through LDS and are shared by the four waves.
//   Operand map.  Lane (r = l & 31, h = l >> 5) supplies bytes 16 h .. 16 h + 15 of every 32-channel slice of row r, for both operands.  WHICH k
// of the instruction a byte lands on is the same function of (h, byte) for A and for B, and the product sums over all k: any such map gives
// the dot product.  What the exact tests check is the rest: that A indexes rows, B columns, and the accumulator rows are the ones stated.
//   LDS rows are Dp + 16 bytes apart: the 16-byte reads of 32 rows then fall 16 bytes apart modulo the bank width instead of on one bank.
template <int KS>
__global__ __launch_bounds__(PRS_THREADS) void pairs_vote_kernel(const int8_t* __restrict__ q, const int32_t* __restrict__ norms,
                                                                const int32_t* __restrict__ blk_img, const int64_t* __restrict__ tab, int n_images, int rq,
                                                                int32_t* votes) {
  constexpr int DP = KS * 32, LD = DP + 16, CHUNKS = PRS_BLOCK * DP / 16;
  __shared__ __attribute__((aligned(16))) int8_t rows[PRS_BLOCK * LD];
  __shared__ __attribute__((aligned(16))) int32_t rnorm[PRS_BLOCK];
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int qb = blockIdx.x * (PRS_TILE / PRS_BLOCK) + w;
  const int img = __builtin_amdgcn_readfirstlane(blk_img[qb]);
  i32x4 bq[KS];
  {
    const int8_t* src = q + ((int64_t)qb * PRS_BLOCK + r) * DP + 16 * h;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bq[ks] = *(const i32x4*)(src + 32 * ks);
  }
  const int nq = norms[qb * PRS_BLOCK + r];
  for (int j = blockIdx.y; j < n_images; j += gridDim.y) {
    const int64_t* e = tab + (int64_t)PRS_WORDS * j;
    const int pstart = (int)e[5], nblk = (int)e[6] / PRS_BLOCK;
    const bool active = img >= 0 && img != j;                  // (wave-uniform: a block is one image's)
    int d1 = 0x7fffffff, d2 = 0x7fffffff;
    for (int b = 0; b < nblk; ++b) {
      const int64_t first = (int64_t)pstart + (int64_t)b * PRS_BLOCK;
      __syncthreads();                                         // (the reads of the step before)
      for (int c = threadIdx.x; c < CHUNKS; c += PRS_THREADS) {
        const int row = c / (DP / 16), col = c % (DP / 16);
        *(i32x4*)(rows + row * LD + 16 * col) = *(const i32x4*)(q + (first + row) * DP + 16 * col);
      }
      if (threadIdx.x < PRS_BLOCK) rnorm[threadIdx.x] = norms[first + threadIdx.x];
      __syncthreads();
      if (!active) continue;
      i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      const int8_t* a = rows + r * LD + 16 * h;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const i32x4*)(a + 32 * ks), bq[ks], acc, 0, 0, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const i32x4 nc = *(const i32x4*)(rnorm + 8 * g + 4 * h);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int v = nc[t] - 2 * acc[4 * g + t];            // d^2 - |q_r|^2
          const int lo = v < d1 ? v : d1;
          d2 = v < d1 ? d1 : (v < d2 ? v : d2);                // the median of (d1, d2, v)
          d1 = lo;
        }
      }
    }
    if (!active) continue;
    // the other half of the database rows of this query sits in lane l ^ 32: the two smallest of the union of two pairs
    const int o1 = __shfl_xor(d1, 32, 64), o2 = __shfl_xor(d2, 32, 64);
    const int m1 = d1 < o1 ? d1 : o1, x1 = d1 < o1 ? o1 : d1, y2 = d2 < o2 ? d2 : o2;
    const int m2 = x1 < y2 ? x1 : y2;
    bool vote = false;
    if (h == 0 && nq != PRS_NO_ROW && m2 < PRS_NO_DIST) {       // (m2 real: image j holds two rows or more)
      const long long e1 = (long long)m1 + nq, e2 = (long long)m2 + nq;
      vote = e1 * 65536ll < (long long)rq * e2;
    }
    const int cnt = __popcll(__ballot(vote));
    if (lane == 0 && cnt) atomicAdd(votes + (int64_t)img * n_images + j, cnt);
  }
}

// ---------------------------------------------------------------------------------------------- select
template <int THREADS>
__device__ __forceinline__ int prs_block_sum(int v, int* lds /* THREADS / 64 */) {
  v = prs_wave_sum(v);
  __syncthreads();                                             // (lds may still be read from the call before)
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  int all = 0;
#pragma unroll
  for (int k = 0; k < THREADS / 64; ++k) all += lds[k];
  return all;
}

// A workgroup per image i.  S[j] = votes[i][j] + votes[j][i] for the eligible j (j != i, S >= min_votes), -1 otherwise, in LDS.  The k-th
// largest value T by bisection on the value (S <= 2 * 4096); everything above T is taken, and of the ties at T the first ones by j.
__global__ __launch_bounds__(PRS_THREADS) void pairs_select_kernel(const int32_t* __restrict__ votes, int n, int k, int min_votes, uint8_t* map) {
  extern __shared__ int s[];                                   // [n] + the sums
  int* sums = s + n;
  const int i = blockIdx.x, tid = threadIdx.x;
  int eligible = 0, top = 0;
  for (int j = tid; j < n; j += PRS_THREADS) {
    int v = -1;
    if (j != i) {
      const int sv = votes[(int64_t)i * n + j] + votes[(int64_t)j * n + i];
      if (sv >= min_votes) v = sv;
    }
    s[j] = v;
    eligible += v >= 0;
    top = v > top ? v : top;
  }
  eligible = prs_block_sum<PRS_THREADS>(eligible, sums);       // (its barriers also publish s)
  if (eligible == 0) return;
  int T = 0, take_ties = eligible;                             // eligible <= k: everything with S >= 0
  if (eligible > k) {
    int lo = 0, hi = 2 * GIMS_PAIRS_MAX_ROWS + 1;              // count(S >= lo) >= k > count(S >= hi)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      int c = 0;
      for (int j = tid; j < n; j += PRS_THREADS) c += s[j] >= mid;
      c = prs_block_sum<PRS_THREADS>(c, sums);
      if (c >= k) lo = mid; else hi = mid;
    }
    T = lo;
    int above = 0;
    for (int j = tid; j < n; j += PRS_THREADS) above += s[j] > T;
    above = prs_block_sum<PRS_THREADS>(above, sums);
    take_ties = k - above;
  }
  int carry = 0;                                               // ties at T in front of this chunk
  for (int base = 0; base < n; base += PRS_THREADS) {
    const int j = base + tid;
    const int v = j < n ? s[j] : -1;
    const int tie = v == T && v >= 0;
    // the rank of a tie among the ties: those of the waves before, then of the lanes before
    const unsigned long long bal = __ballot(tie);
    const int before_lane = __popcll(bal & ((1ull << (tid & 63)) - 1ull));
    __syncthreads();
    if ((tid & 63) == 0) sums[tid >> 6] = __popcll(bal);
    __syncthreads();
    int before = carry, all = 0;
#pragma unroll
    for (int x = 0; x < PRS_THREADS / 64; ++x) {
      before += x < (tid >> 6) ? sums[x] : 0;
      all += sums[x];
    }
    carry += all;
    const bool taken = v >= 0 && (v > T || (tie && before + before_lane < take_ties));
    if (taken) {
      const int a = i < j ? i : j, b = i < j ? j : i;
      map[(int64_t)a * n + b] = 1;                             // (every writer writes the same 1)
    }
  }
}

// ---------------------------------------------------------------------------------------------- compaction
// a wave per row of the map: the marks of the row
__global__ __launch_bounds__(PRS_THREADS) void pairs_count_kernel(const uint8_t* __restrict__ map, int n, int32_t* __restrict__ rowcnt) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (PRS_THREADS / 64) + (threadIdx.x >> 6);
  if (i >= n) return;
  int c = 0;
  for (int j = i + 1 + lane; j < n; j += 64) c += map[(int64_t)i * n + j] != 0;
  c = prs_wave_sum(c);
  if (lane == 0) rowcnt[i] = c;
}

// one workgroup: the exclusive scan of the row counts, 1024 at a time with a carry, and the counters
__global__ __launch_bounds__(PRS_SCAN_THREADS) void pairs_scan_kernel(const int32_t* __restrict__ rowcnt, int n, int32_t* __restrict__ rowoff,
                                                                     const uint32_t* __restrict__ head, int n_rows, int n_short,
                                                                     int32_t* __restrict__ counters) {
  __shared__ int lds[PRS_SCAN_THREADS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += PRS_SCAN_THREADS) {
    const int i = base + (int)threadIdx.x;
    const int v = i < n ? rowcnt[i] : 0;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    __syncthreads();
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int x = 0; x < PRS_SCAN_THREADS / 64; ++x) {
      const int sx = lds[x];
      before += x < w ? sx : 0;
      all += sx;
    }
    if (i < n) rowoff[i] = carry + before + inc - v;
    carry += all;
  }
  if (threadIdx.x == 0) {
    const unsigned long long nf = *(const unsigned long long*)(head + 4);
    counters[PRS_N_PAIRS] = carry;
    counters[PRS_N_ROWS] = n_rows;
    counters[PRS_N_SHORT] = n_short;
    counters[PRS_N_BAD_ROWS] = (int32_t)head[2];
    counters[PRS_N_NONFINITE] = nf > 0x7fffffffull ? 0x7fffffff : (int32_t)nf;
    counters[5] = counters[6] = counters[7] = 0;
  }
}

// a wave per row of the map: the marked (i, j), j ascending, from rowoff[i] on
__global__ __launch_bounds__(PRS_THREADS) void pairs_fill_kernel(const uint8_t* __restrict__ map, const int32_t* __restrict__ votes,
                                                                const int32_t* __restrict__ rowoff, int n, int64_t cap, int32_t* __restrict__ pairs,
                                                                int32_t* __restrict__ pair_votes) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (PRS_THREADS / 64) + (threadIdx.x >> 6);
  if (i >= n) return;
  int64_t at = rowoff[i];
  for (int base = i + 1; base < n; base += 64) {
    const int j = base + lane;
    const bool on = j < n && map[(int64_t)i * n + j] != 0;
    const unsigned long long bal = __ballot(on);
    const int64_t slot = at + __popcll(bal & ((1ull << lane) - 1ull));
    if (on && slot < cap) {                                    // (always: a row of S gives at most k marks, and there are no more pairs than pairs)
      pairs[2 * slot] = i;
      pairs[2 * slot + 1] = j;
      pair_votes[slot] = votes[(int64_t)i * n + j] + votes[(int64_t)j * n + i];
    }
    at += __popcll(bal);
  }
}

template <int KS>
static int prs_vote_launch(const PrsWs& w, int n, int pool, int rq, int32_t* votes, hipStream_t st) {
  const int tiles = pool / PRS_TILE;
  int gy = cdiv(PRS_VOTE_GROUPS, tiles);
  gy = gy < 1 ? 1 : (gy > n ? n : gy);
  pairs_vote_kernel<KS><<<dim3(tiles, gy), PRS_THREADS, 0, st>>>(w.q, w.norms, w.blk_img, w.tab, n, rq, votes);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

// the sizes that lay the workspace out (with every image's m): the op and gims_aux_layout refuse the same values
static int prs_check_sizes(int64_t n, int64_t d) {
  GIMS_CHECK_ARG(n >= 2 && n <= GIMS_PAIRS_MAX_IMAGES, "select_pairs: N = %lld is out of range (2 .. %d)", (long long)n, GIMS_PAIRS_MAX_IMAGES);
  GIMS_CHECK_ARG(d >= 32 && d <= GIMS_PAIRS_MAX_D && d % 32 == 0, "select_pairs: D = %lld is not served (a multiple of 32 in 32 .. %d)", (long long)d,
                 GIMS_PAIRS_MAX_D);
  return GIMS_OK;
}

// gims_aux_layout for GIMS_AUX_SELECT_PAIRS: sizes = {D, N, m_0 .. m_{N-1}}, the workspace
int select_pairs_aux_layout(const int64_t* sizes, int n, WsRecord& rec) {
  GIMS_CHECK_ARG(n >= 2 && sizes[1] == (int64_t)n - 2, "select_pairs: the layout takes 2 + N sizes {D, N, m_0 .. m_{N-1}}, not %d", n);
  const int64_t d = sizes[0], n_img = sizes[1];
  if (const int rc = prs_check_sizes(n_img, d)) return rc;
  for (int64_t i = 0; i < n_img; ++i)
    GIMS_CHECK_ARG(sizes[2 + i] >= 0 && sizes[2 + i] <= GIMS_PAIRS_MAX_ROWS, "select_pairs: image %lld: m = %lld is outside 0 .. %d", (long long)i,
                   (long long)sizes[2 + i], GIMS_PAIRS_MAX_ROWS);
  PrsWs w;
  rec.bytes = prs_layout(nullptr, n_img, prs_pool(sizes + 2, 1, n_img), prs_dp((int)d), w, &rec);
  return GIMS_OK;
}

// GIMS_AUX_SELECT_PAIRS of gims_run_ops (include/gims_hip.h): every argument check precedes the first HIP call
int select_pairs_aux(const gims_aux_args& x, hipStream_t st) {
  const int64_t n = x.i[0], d = x.i[1], per_image = x.i[2], k = x.i[3], min_votes = x.i[4];
  const float scale = x.f[0];
  // i[5] is where a later form of this function would be selected: it is read FIRST (see assemble_rows_aux)
  GIMS_CHECK_ARG(x.i[5] == 0, "gims_run_ops: unknown auxiliary function form: select_pairs with i[5] = %lld (i[5] is reserved and must be 0)",
                 (long long)x.i[5]);
  if (const int rc = prs_check_sizes(n, d)) return rc;
  GIMS_CHECK_ARG(per_image >= 0 && per_image <= GIMS_PAIRS_MAX_ROWS, "select_pairs: per_image = %lld is out of range (0 .. %d)", (long long)per_image,
                 GIMS_PAIRS_MAX_ROWS);
  GIMS_CHECK_ARG(k >= 1, "select_pairs: k = %lld must be at least 1", (long long)k);
  GIMS_CHECK_ARG(min_votes >= 0, "select_pairs: min_votes = %lld is negative", (long long)min_votes);
  GIMS_CHECK_ARG(x.p[0] && x.p[1] && x.p[2] && x.p[3] && x.p[4], "select_pairs: the table, votes, the output buffer, the counters or the workspace are NULL");
  GIMS_CHECK_ARG(x.p[5] == nullptr, "select_pairs: p[5] is reserved and must be NULL");
  GIMS_CHECK_ARG(((uintptr_t)x.p[0] & 7) == 0, "select_pairs: the table must be 8-byte aligned");
  GIMS_CHECK_ARG((((uintptr_t)x.p[1] | (uintptr_t)x.p[2] | (uintptr_t)x.p[3]) & 3) == 0,
                 "select_pairs: votes, the output buffer and the counters must be 4-byte aligned");
  GIMS_CHECK_ARG(((uintptr_t)x.p[4] & 15) == 0, "select_pairs: the workspace must be 16-byte aligned");
  const int64_t* tab = (const int64_t*)x.p[0];                 // HOST memory: N image entries, then the entry of the call
  const int64_t* call = tab + PRS_WORDS * n;
  const int64_t rq = call[0], flags = call[1], work_bytes = call[2];
  GIMS_CHECK_ARG(rq >= 0 && rq <= 65536, "select_pairs: rq = %lld is out of range (0 .. 65536: ratio^2 * 65536 for a ratio in [0, 1])", (long long)rq);
  GIMS_CHECK_ARG((flags & ~(int64_t)GIMS_PAIRS_SCALE_GIVEN) == 0 && call[3] == 0 && call[4] == 0 && call[5] == 0 && call[6] == 0 && call[7] == 0,
                 "select_pairs: a reserved word of the table's last entry is not 0 (GIMS_PAIRS_SCALE_GIVEN is the only flag)");
  const bool scale_given = (flags & GIMS_PAIRS_SCALE_GIVEN) != 0;
  GIMS_CHECK_ARG(!scale_given || (scale >= 0.0f && scale <= 3.402823466e38f), "select_pairs: scale must be finite and >= 0");
  int64_t n_rows = 0, n_short = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t* e = tab + PRS_WORDS * i;
    GIMS_CHECK_ARG(e[4] >= 0 && e[4] <= per_image, "select_pairs: image %lld: m = %lld is outside 0 .. per_image = %lld", (long long)i, (long long)e[4],
                   (long long)per_image);
    GIMS_CHECK_ARG(e[0] != 0 || e[4] == 0, "select_pairs: image %lld: the descriptor pointer is NULL", (long long)i);
    GIMS_CHECK_ARG((e[0] & 3) == 0 && (e[3] & 3) == 0, "select_pairs: image %lld: the descriptors and the index list must be 4-byte aligned", (long long)i);
    GIMS_CHECK_ARG(e[1] >= d, "select_pairs: image %lld: the row stride %lld is below D = %lld", (long long)i, (long long)e[1], (long long)d);
    GIMS_CHECK_ARG(e[2] >= 0 && e[2] <= 0x7fffffff, "select_pairs: image %lld: n = %lld is out of range", (long long)i, (long long)e[2]);
    GIMS_CHECK_ARG(e[5] == 0 && e[6] == 0 && e[7] == 0, "select_pairs: image %lld: a reserved word of the table is not 0", (long long)i);
    n_rows += e[4];
    n_short += e[4] < 2;
  }
  const int64_t pool = prs_pool(tab + 4, PRS_WORDS, n);
  const int dp = prs_dp((int)d);
  PrsWs w;
  const size_t need = prs_layout(nullptr, n, pool, dp, w);
  GIMS_CHECK_ARG(work_bytes >= 0 && (size_t)work_bytes >= need, "select_pairs: work_bytes = %lld is below the %zu bytes that this call needs",
                 (long long)work_bytes, need);

  prs_layout((void*)x.p[4], n, pool, dp, w);
  int32_t* votes = (int32_t*)x.p[1];
  int32_t* out = (int32_t*)x.p[2];
  int32_t* counters = (int32_t*)x.p[3];
  const int nn = (int)n, kk = (int)(k < n - 1 ? k : n - 1), np = (int)pool;
  const int64_t cap = n * kk < n * (n - 1) / 2 ? n * kk : n * (n - 1) / 2;       // = min(N k, N (N - 1) / 2)

  std::vector<int64_t> dev_tab((size_t)n * PRS_WORDS);
  std::vector<int32_t> blk((size_t)(pool / PRS_BLOCK), -1);
  int64_t at = 0;
  for (int64_t i = 0; i < n; ++i) {
    memcpy(&dev_tab[(size_t)i * PRS_WORDS], tab + PRS_WORDS * i, sizeof(int64_t) * PRS_WORDS);
    const int64_t p = prs_up(tab[PRS_WORDS * i + 4], PRS_BLOCK);
    dev_tab[(size_t)i * PRS_WORDS + 5] = at;
    dev_tab[(size_t)i * PRS_WORDS + 6] = p;
    for (int64_t b = 0; b < p / PRS_BLOCK; ++b) blk[(size_t)(at / PRS_BLOCK + b)] = (int32_t)i;
    at += p;
  }
  int rc = upload_table(dev_tab.data(), dev_tab.size() * sizeof(int64_t), w.tab, st);
  if (rc != GIMS_OK) return rc;
  rc = upload_table(blk.data(), blk.size() * sizeof(int32_t), w.blk_img, st);
  if (rc != GIMS_OK) return rc;
  GIMS_HIP(hipMemsetAsync(w.head, 0, sizeof(uint32_t) * 8, st));
  GIMS_HIP(hipMemsetAsync(votes, 0, sizeof(int32_t) * (size_t)n * (size_t)n, st));
  GIMS_HIP(hipMemsetAsync(w.map, 0, (size_t)n * (size_t)n, st));

  const int row_blocks = cdiv(pool, PRS_THREADS / 64);
  if (!scale_given) {
    pairs_maxabs_kernel<<<cdiv(pool, PRS_MAXABS_ROWS * (PRS_THREADS / 64)), PRS_THREADS, 0, st>>>(w.tab, w.blk_img, np, (int)d, w.head);
    GIMS_LAUNCH_CHECK();
  }
  pairs_quantise_kernel<<<row_blocks, PRS_THREADS, 0, st>>>(w.tab, w.blk_img, np, (int)d, dp, scale_given ? 1 : 0, scale, w.head, w.q, w.norms);
  GIMS_LAUNCH_CHECK();
  switch (dp / 32) {
    case 1: rc = prs_vote_launch<1>(w, nn, np, (int)rq, votes, st); break;
    case 2: rc = prs_vote_launch<2>(w, nn, np, (int)rq, votes, st); break;
    case 4: rc = prs_vote_launch<4>(w, nn, np, (int)rq, votes, st); break;
    case 8: rc = prs_vote_launch<8>(w, nn, np, (int)rq, votes, st); break;
    case 16: rc = prs_vote_launch<16>(w, nn, np, (int)rq, votes, st); break;
    default: rc = prs_vote_launch<32>(w, nn, np, (int)rq, votes, st); break;
  }
  if (rc != GIMS_OK) return rc;
  pairs_select_kernel<<<nn, PRS_THREADS, sizeof(int) * (size_t)(nn + PRS_THREADS / 64), st>>>(votes, nn, kk, (int)min_votes, w.map);
  GIMS_LAUNCH_CHECK();
  pairs_count_kernel<<<cdiv(n, PRS_THREADS / 64), PRS_THREADS, 0, st>>>(w.map, nn, w.rowcnt);
  GIMS_LAUNCH_CHECK();
  pairs_scan_kernel<<<1, PRS_SCAN_THREADS, 0, st>>>(w.rowcnt, nn, w.rowoff, w.head, (int)n_rows, (int)n_short, counters);
  GIMS_LAUNCH_CHECK();
  pairs_fill_kernel<<<cdiv(n, PRS_THREADS / 64), PRS_THREADS, 0, st>>>(w.map, votes, w.rowoff, nn, cap, out, out + 2 * cap);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

}  // namespace gims
