// Multi-view tracks from image-set matches: GIMS_AUX_BUILD_TRACKS of gims_run_ops merges the pairwise matches of a set of
// images into the connected components of the match graph, flags the components that hold two keypoints of one image, and writes the kept
// ones in canonical order.  include/gims_hip.h has the contract; tests/tracks_ref.py is the NumPy restatement.  Integer work throughout:
// every output is a function of the edge set alone.
//
// Stages, each a launch of its own on the stream (a kernel boundary makes the stage before it visible, so only the union launch needs atomics
// for its reads):  init (parent[g] = g, image of g) -> union (lock-free, hooks the larger root under the smaller: the root of a component is
// its smallest member) -> flatten + component sizes -> scan of the sizes (segment starts) -> claim (members into their segment, any order) ->
// rank (position of every member among its component's ids by counting, conflict flag; the huge components by a prefix count over the nodes
// instead) -> keep flags -> scans of the keep flags (track number) and of the kept sizes (indptr) -> write.
#include "common.h"

namespace gims {

constexpr int TRK_THREADS = 256;                               // 4 waves
constexpr int TRK_TILE = GIMS_TRACKS_SCAN_TILE;                // elements per workgroup of the three-phase scan
constexpr int TRK_ITEMS = TRK_TILE / TRK_THREADS;              // consecutive elements per thread
constexpr int TRK_SHORT = GIMS_TRACKS_SHORT_SEGMENT;           // components up to this size are ranked by one lane, larger ones by a wave
constexpr int TRK_WORDS = GIMS_TRACKS_TABLE_WORDS;             // int64 words per table entry
constexpr int TRK_LONG = GIMS_TRACKS_LONG_SEGMENT;             // ... and components above max(this, N / 1024) nodes, "huge", by a scan over the nodes
constexpr int TRK_SUMS_THREADS = 1024;
static_assert(TRK_TILE % TRK_THREADS == 0, "a scan tile is a whole number of elements per thread");
enum { TRK_N_TRACKS = 0, TRK_N_OBS, TRK_N_CONFLICTING, TRK_N_EDGES, TRK_N_BAD, TRK_STATUS, TRK_COUNTERS = 8 };

// A component of more than trk_huge(n) nodes is huge; there are at most trk_cap_huge(n) <= 1024 of them
static inline int64_t trk_huge(int64_t n) { return n / 1024 > TRK_LONG ? n / 1024 : TRK_LONG; }
static inline int64_t trk_cap_huge(int64_t n) { return n / (trk_huge(n) + 1); }
// The workspace (the formula of include/gims_hip.h; gims_aux_layout reports this routine's offsets): twelve int32 [N] arrays, the tile sums of the scan, the
// per-tile member counts of the huge components and one counter
struct TrkWs {
  int32_t *parent, *root, *size, *off, *members, *img, *pos, *keep, *ksize, *tid, *kofs, *confl, *sums, *hcnt, *n_huge;
  int32_t* cursor() const { return parent; }                   // the claim counters: parent is dead once root is written
};
static size_t trk_layout(void* base, int64_t n, TrkWs& w, WsRecord* rec = nullptr) {
  WsLayout L(base, rec);
  int32_t** a[12] = {&w.parent, &w.root, &w.size, &w.off, &w.members, &w.img, &w.pos, &w.keep, &w.ksize, &w.tid, &w.kofs, &w.confl};
  for (auto p : a) *p = L.take<int32_t>((size_t)n);
  w.sums = L.take<int32_t>((size_t)(n / TRK_TILE + 2));
  w.hcnt = L.take<int32_t>((size_t)((trk_cap_huge(n) + 1) * (n / TRK_TILE + 1)));
  w.n_huge = L.take<int32_t>(1);
  return L.bytes();
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------- init
// parent[g] = g; img[g] = the image of node g: the number of entries of start[1 .. n_images] that are <= g (images without keypoints have
// equal starts and are stepped over), clamped, so that a start table that is not ascending still gives an image that exists
__global__ __launch_bounds__(TRK_THREADS) void trk_init_kernel(const int32_t* __restrict__ start, int n_images, int n, int32_t* __restrict__ parent,
                                                               int32_t* __restrict__ img) {
  const int g = blockIdx.x * TRK_THREADS + threadIdx.x;
  if (g >= n) return;
  int lo = 0, hi = n_images;                                   // the first k in 0 .. n_images with start[k + 1] > g (n_images: none)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (start[mid + 1] <= g) lo = mid + 1; else hi = mid;
  }
  parent[g] = g;
  img[g] = lo < n_images ? lo : n_images - 1;
}

// ---------------------------------------------------------------------------------------------- union
// The one launch in which workgroups on different XCDs read what the others write.  Per-XCD L2s are not coherent with each other and a CU's L1
// is never refreshed by another CU's stores, so EVERY access to parent here is an agent-scope atomic (the loads bypass L1 and are served by
// memory-side coherent L2 traffic): a plain or volatile load could show a stale parent for ever, and the retry loop below would spin on it.
__device__ __forceinline__ int32_t trk_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x.  A non-root's parent is always a smaller id (init writes parent[g] = g, a hook puts the larger root under the smaller, the
// compression replaces a parent by an ancestor), so every step moves to a strictly smaller id: at most x steps.  Anything else -- it cannot
// happen -- ends the walk with bad = true instead of following it.
__device__ __forceinline__ int32_t trk_find(int32_t* parent, int32_t x, bool& bad) {
  for (;;) {
    const int32_t p = trk_load(parent + x);
    if (p == x) return x;
    if (p < 0 || p > x) { bad = true; return x; }
    const int32_t gp = trk_load(parent + p);
    if (gp < 0 || gp > p) { bad = true; return x; }
    if (gp != p) __hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // halve the path: parent only ever decreases
    x = gp;
  }
}

// Join the components of a and b.  A failed compare-and-swap means that another thread's hook of that root succeeded in between; there are at
// most n - 1 successful hooks in all, so n retries cannot run out -- and if they do the row gives up and raises the status word.
__device__ __forceinline__ bool trk_unite(int32_t* parent, int32_t a, int32_t b, int n) {
  bool bad = false;
  for (int it = 0; it <= n; ++it) {
    a = trk_find(parent, a, bad);
    b = trk_find(parent, b, bad);
    if (bad) return false;
    if (a == b) return true;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    int32_t expect = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return true;                                             // hi was still a root: hooked
  }
  return false;
}

// Work items are the rows of all pairs, 64 consecutive rows per wave and step.  tab: [n_pairs + 1][8] = {matches0, scores, mask, n_a, n_b,
// start_a, start_b, first row}; entry n_pairs holds the total number of rows.  The pair of a wave's first row is a binary search over the
// first rows (wave-uniform: scalar loads and compares); a lane whose row lies in a later pair steps forward from there.
__global__ __launch_bounds__(TRK_THREADS) void trk_union_kernel(const int64_t* __restrict__ tab, int n_pairs, int n, float min_score,
                                                                int32_t* parent, int32_t* counters) {
  const int lane = threadIdx.x & 63;
  const int64_t total = tab[(int64_t)TRK_WORDS * n_pairs + 7];
  const int64_t n_waves = (int64_t)gridDim.x * (TRK_THREADS / 64);
  const int64_t wave = (int64_t)blockIdx.x * (TRK_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  int n_edges = 0, n_bad = 0, gave_up = 0;
  for (int64_t base = wave * 64; base < total; base += n_waves * 64) {
    int lo = 0, hi = n_pairs;                                  // the last pair whose first row is <= base (first row of pair 0 is 0)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tab[(int64_t)TRK_WORDS * mid + 7] <= base) lo = mid; else hi = mid;
    }
    const int64_t row = base + lane;
    if (row >= total) continue;
    int p = lo;
    while (p + 1 < n_pairs && tab[(int64_t)TRK_WORDS * (p + 1) + 7] <= row) ++p;
    const int64_t* e = tab + (int64_t)TRK_WORDS * p;
    const int64_t i = row - e[7], n_a = e[3], n_b = e[4];
    if (i < 0 || i >= n_a) continue;                           // (a table whose first rows do not ascend: the row belongs to nobody)
    const int64_t j = ((const int64_t*)(uintptr_t)e[0])[i];
    if (j == -1) continue;
    const int64_t ga = e[5] + i, gb = e[6] + j;
    if (j < 0 || j >= n_b || ga < 0 || ga >= n || gb < 0 || gb >= n) {      // never an index
      ++n_bad;
      continue;
    }
    const float* score = (const float*)(uintptr_t)e[1];
    if (score && !(score[i] >= min_score)) continue;           // (a NaN score is no edge)
    const uint8_t* mask = (const uint8_t*)(uintptr_t)e[2];
    if (mask && mask[i] == 0) continue;
    ++n_edges;
    if (ga != gb && !trk_unite(parent, (int32_t)ga, (int32_t)gb, n)) gave_up = 1;
  }
  n_edges = wave_sum_i32(n_edges);
  n_bad = wave_sum_i32(n_bad);
  gave_up = wave_sum_i32(gave_up);
  if (lane == 0) {
    if (n_edges) atomicAdd(counters + TRK_N_EDGES, n_edges);
    if (n_bad) atomicAdd(counters + TRK_N_BAD, n_bad);
    if (gave_up) atomicOr(counters + TRK_STATUS, 1);
  }
}

// ---------------------------------------------------------------------------------------------- flatten, sizes
__global__ __launch_bounds__(TRK_THREADS) void trk_flatten_kernel(const int32_t* __restrict__ parent, int n, int32_t* __restrict__ root,
                                                                  int32_t* __restrict__ size, int32_t* counters) {
  const int g = blockIdx.x * TRK_THREADS + threadIdx.x;
  if (g >= n) return;
  int x = g;
  for (;;) {
    const int p = parent[x];
    if (p == x) break;
    if (p < 0 || p > x) {                                      // (cannot happen, see trk_find)
      atomicOr(counters + TRK_STATUS, 2);
      break;
    }
    x = p;
  }
  root[g] = x;
  atomicAdd(size + x, 1);
}

// ---------------------------------------------------------------------------------------------- exclusive scan over n elements, three phases
// thread t of a workgroup takes elements TRK_ITEMS t .. TRK_ITEMS t + TRK_ITEMS - 1 of the workgroup's tile
template <int THREADS>
__device__ __forceinline__ int block_exclusive_scan(int v, int* lds /* THREADS / 64 + 1 */, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();                                             // (lds may still be read from the call before)
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < THREADS / 64; ++k) {
    const int s = lds[k];
    before += k < w ? s : 0;
    all += s;
  }
  total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(TRK_THREADS) void trk_scan_sums_kernel(const int32_t* __restrict__ in, int n, int32_t* __restrict__ sums) {
  __shared__ int lds[TRK_THREADS / 64 + 1];
  const int64_t first = (int64_t)blockIdx.x * TRK_TILE + (int64_t)threadIdx.x * TRK_ITEMS;
  int v = 0;
#pragma unroll
  for (int k = 0; k < TRK_ITEMS; ++k) v += first + k < n ? in[first + k] : 0;
  int total;
  block_exclusive_scan<TRK_THREADS>(v, lds, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0 .. n_tiles) -> their exclusive scan in place; the grand total to sums[n_tiles] and, when given, to *total_out
__global__ __launch_bounds__(TRK_SUMS_THREADS) void trk_scan_tiles_kernel(int32_t* __restrict__ sums, int n_tiles, int32_t* __restrict__ total_out) {
  __shared__ int lds[TRK_SUMS_THREADS / 64 + 1];
  int carry = 0;
  for (int base = 0; base < n_tiles; base += TRK_SUMS_THREADS) {
    const int k = base + (int)threadIdx.x;
    const int v = k < n_tiles ? sums[k] : 0;
    int total;
    const int ex = block_exclusive_scan<TRK_SUMS_THREADS>(v, lds, total);
    if (k < n_tiles) sums[k] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    sums[n_tiles] = carry;
    if (total_out) *total_out = carry;
  }
}

__global__ __launch_bounds__(TRK_THREADS) void trk_scan_apply_kernel(const int32_t* __restrict__ in, int n, const int32_t* __restrict__ sums,
                                                                     int32_t* __restrict__ out) {
  __shared__ int lds[TRK_THREADS / 64 + 1];
  const int64_t first = (int64_t)blockIdx.x * TRK_TILE + (int64_t)threadIdx.x * TRK_ITEMS;
  int x[TRK_ITEMS], v = 0;
#pragma unroll
  for (int k = 0; k < TRK_ITEMS; ++k) {
    x[k] = first + k < n ? in[first + k] : 0;
    v += x[k];
  }
  int total;
  int run = sums[blockIdx.x] + block_exclusive_scan<TRK_THREADS>(v, lds, total);
#pragma unroll
  for (int k = 0; k < TRK_ITEMS; ++k) {
    if (first + k < n) out[first + k] = run;
    run += x[k];
  }
}

static int trk_scan(const int32_t* in, int n, int32_t* sums, int32_t* out, int32_t* total_out, hipStream_t st) {
  const int n_tiles = cdiv(n, TRK_TILE);
  trk_scan_sums_kernel<<<n_tiles, TRK_THREADS, 0, st>>>(in, n, sums);
  GIMS_LAUNCH_CHECK();
  trk_scan_tiles_kernel<<<1, TRK_SUMS_THREADS, 0, st>>>(sums, n_tiles, total_out);
  GIMS_LAUNCH_CHECK();
  trk_scan_apply_kernel<<<n_tiles, TRK_THREADS, 0, st>>>(in, n, sums, out);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

// ---------------------------------------------------------------------------------------------- claim
// every member of a component of two or more -- but not of a huge one -- takes a slot of its component's segment; which slot is decided by the
// race and forgotten by the ranking below.  The root of a huge component takes the component's row of the huge table instead (any order: the
// row is scratch), and keeps its number where its claim counter would be.
__global__ __launch_bounds__(TRK_THREADS) void trk_claim_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                                const int32_t* __restrict__ off, int n, int huge, int cap_huge, int32_t* cursor,
                                                                int32_t* __restrict__ members, int32_t* n_huge) {
  const int g = blockIdx.x * TRK_THREADS + threadIdx.x;
  if (g >= n) return;
  const int r = root[g], s = size[r];
  if (s < 2) return;
  if (s > huge) {
    if (g == r) {
      const int c = atomicAdd(n_huge, 1);
      cursor[g] = c < cap_huge ? c : -1;                       // (always a row: more than cap_huge components of more than `huge` nodes exceed n)
    }
    return;
  }
  const int slot = atomicAdd(cursor + r, 1);
  const int64_t at = (int64_t)off[r] + slot;
  if (slot < s && at < n) members[at] = g;                     // (always: the sizes were counted over the same roots)
}

// ---------------------------------------------------------------------------------------------- rank, conflict, keep
// pos[e] = the number of members of e's component with a smaller id: rank by counting, which needs no order among the claimed slots.  A
// component conflicts when two of its members lie in one image.  One thread per node; the thread of a root owns its component: it ranks a
// short one alone, and the wave takes the long ones of its 64 nodes one after the other, a lane per member.
__global__ __launch_bounds__(TRK_THREADS) void trk_rank_kernel(const int32_t* __restrict__ size, const int32_t* __restrict__ off,
                                                               const int32_t* __restrict__ members, const int32_t* __restrict__ img, int n, int huge,
                                                               int32_t* __restrict__ pos, int32_t* __restrict__ confl) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * TRK_THREADS + threadIdx.x;
  int s = g < n ? size[g] : 0;                                 // (non-roots hold 0)
  if (s > huge) s = 0;                                         // (the huge ones are ranked by trk_huge_*_kernel)
  const int o = g < n ? off[g] : 0;
  bool c = false;
  if (s >= 2 && s <= TRK_SHORT) {
    for (int a = 0; a < s; ++a) {
      const int e = members[o + a], ie = img[e];
      int rank = 0;
      for (int b = 0; b < s; ++b) {
        const int x = members[o + b];
        rank += x < e;
        c |= x != e && img[x] == ie;
      }
      pos[e] = rank;
    }
  }
  unsigned long long todo = __ballot(s > TRK_SHORT);
  while (todo) {
    const int src = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int S = __shfl(s, src, 64), O = __shfl(o, src, 64);
    bool cc = false;
    for (int a = lane; a < S; a += 64) {
      const int e = members[O + a], ie = img[e];
      int rank = 0;
      for (int b = 0; b < S; ++b) {
        const int x = members[O + b];
        rank += x < e;
        cc |= x != e && img[x] == ie;
      }
      pos[e] = rank;
    }
    const bool any = __ballot(cc) != 0ull;
    if (lane == src) c = any;
  }
  if (g < n) confl[g] = c;
}

// ---------------------------------------------------------------------------------------------- huge components
// Rank by counting costs s^2 / 64 steps per component: fine up to a thousand nodes, not for the one component of 10^5 that a few percent of wrong
// matches glue together.  For a huge component the rank of a member is a prefix count over the NODES instead: members per scan tile (hcnt
// [component][tile], counted by atomics), an exclusive scan of every row, and inside a tile the number of earlier nodes of the same component.
__global__ __launch_bounds__(TRK_THREADS) void trk_huge_count_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                                     const int32_t* __restrict__ cursor, int n, int huge, int n_tiles, int32_t* hcnt) {
  const int g = blockIdx.x * TRK_THREADS + threadIdx.x;
  if (g >= n) return;
  const int r = root[g];
  if (size[r] <= huge) return;
  const int c = cursor[r];
  if (c >= 0) atomicAdd(hcnt + (int64_t)c * n_tiles + g / TRK_TILE, 1);
}

// one workgroup per row of the table: the row's exclusive scan in place
__global__ __launch_bounds__(TRK_SUMS_THREADS) void trk_huge_scan_kernel(int32_t* __restrict__ hcnt, int n_tiles, const int32_t* __restrict__ n_huge) {
  __shared__ int lds[TRK_SUMS_THREADS / 64 + 1];
  if ((int)blockIdx.x >= *n_huge) return;
  int32_t* row = hcnt + (int64_t)blockIdx.x * n_tiles;
  int carry = 0;
  for (int base = 0; base < n_tiles; base += TRK_SUMS_THREADS) {
    const int k = base + (int)threadIdx.x;
    const int v = k < n_tiles ? row[k] : 0;
    int total;
    const int ex = block_exclusive_scan<TRK_SUMS_THREADS>(v, lds, total);
    if (k < n_tiles) row[k] = carry + ex;
    carry += total;
  }
}

// one workgroup per tile: key[i] = the table row of node i's component, or -1; a member's rank is its row's count in front of the tile plus the
// earlier nodes of the tile with its key.  The member goes to that place of its component's segment: the segment in ascending order.
__global__ __launch_bounds__(TRK_THREADS) void trk_huge_rank_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                                    const int32_t* __restrict__ off, const int32_t* __restrict__ cursor,
                                                                    const int32_t* __restrict__ hcnt, int n, int huge, int n_tiles,
                                                                    int32_t* __restrict__ pos, int32_t* __restrict__ members) {
  __shared__ int key[TRK_TILE];
  const int first = blockIdx.x * TRK_TILE;
  int mine = 0;
#pragma unroll
  for (int k = 0; k < TRK_ITEMS; ++k) {
    const int i = k * TRK_THREADS + (int)threadIdx.x, g = first + i;
    int c = -1;
    if (g < n) {
      const int r = root[g];
      if (size[r] > huge) c = cursor[r];
    }
    key[i] = c;
    mine |= c >= 0;
  }
  if (!__syncthreads_or(mine)) return;
#pragma unroll 1
  for (int k = 0; k < TRK_ITEMS; ++k) {
    const int i = k * TRK_THREADS + (int)threadIdx.x, g = first + i;
    const int c = key[i];
    if (c < 0) continue;
    int before = 0;
    for (int h = 0; h < i; ++h) before += key[h] == c;
    const int r = root[g], rank = hcnt[(int64_t)c * n_tiles + blockIdx.x] + before;
    pos[g] = rank;
    if (rank < size[r]) members[off[r] + rank] = g;            // (always)
  }
}

// a huge component conflicts when a member and the member in front of it lie in one image (the nodes of an image are contiguous)
__global__ __launch_bounds__(TRK_THREADS) void trk_huge_conflict_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                                        const int32_t* __restrict__ off, const int32_t* __restrict__ cursor,
                                                                        const int32_t* __restrict__ pos, const int32_t* __restrict__ members,
                                                                        const int32_t* __restrict__ img, int n, int huge, int32_t* confl) {
  const int g = blockIdx.x * TRK_THREADS + threadIdx.x;
  if (g >= n) return;
  const int r = root[g];
  if (size[r] <= huge || cursor[r] < 0) return;
  const int rank = pos[g];
  if (rank <= 0 || rank >= size[r]) return;
  const int prev = members[off[r] + rank - 1];
  if (prev >= 0 && prev < n && img[prev] == img[g]) confl[r] = 1;          // (every writer writes the same 1)
}

// ---------------------------------------------------------------------------------------------- keep
__global__ __launch_bounds__(TRK_THREADS) void trk_keep_kernel(const int32_t* __restrict__ size, const int32_t* __restrict__ confl, int n, int min_length,
                                                               int keep_conflicting, int32_t* __restrict__ keep, int32_t* __restrict__ ksize,
                                                               int32_t* counters) {
  const int g = blockIdx.x * TRK_THREADS + threadIdx.x;
  if (g >= n) return;
  const int s = size[g], c = confl[g];                         // (non-roots: 0 and 0)
  const bool kept = s >= min_length && (keep_conflicting || !c);
  keep[g] = kept;
  ksize[g] = kept ? s : 0;
  if (c) atomicAdd(counters + TRK_N_CONFLICTING, 1);
}

// ---------------------------------------------------------------------------------------------- write
__global__ __launch_bounds__(TRK_THREADS) void trk_write_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ keep,
                                                                const int32_t* __restrict__ tid, const int32_t* __restrict__ kofs,
                                                                const int32_t* __restrict__ pos, const int32_t* __restrict__ img,
                                                                const int32_t* __restrict__ confl, const int32_t* __restrict__ start, int n,
                                                                const int32_t* __restrict__ counters, int32_t* __restrict__ track_of,
                                                                int32_t* __restrict__ indptr, int32_t* __restrict__ obs_image,
                                                                int32_t* __restrict__ obs_keypoint, uint8_t* __restrict__ conflict) {
  const int g = blockIdx.x * TRK_THREADS + threadIdx.x;
  if (g >= n) return;
  const int cap_t = n / 2;
  if (g == 0) {
    const int t = counters[TRK_N_TRACKS];
    if (t >= 0 && t <= cap_t) indptr[t] = counters[TRK_N_OBS];
  }
  const int r = root[g];
  int t = -1;
  if (keep[r]) {
    t = tid[r];
    const int64_t q = (int64_t)kofs[r] + pos[g];
    if (t < 0 || t >= cap_t || q < 0 || q >= n) {              // (cannot happen: a kept component has two members or more, and they add up to <= n)
      t = -1;
    } else {
      const int k = img[g];
      obs_image[q] = k;
      obs_keypoint[q] = g - start[k];
      if (g == r) {
        indptr[t] = kofs[r];
        conflict[t] = (uint8_t)confl[r];
      }
    }
  }
  track_of[g] = t;
}

// gims_aux_layout for GIMS_AUX_BUILD_TRACKS: sizes = {N}, the workspace; the bound is the op's below
int build_tracks_aux_layout(const int64_t* sizes, int n, WsRecord& rec) {
  GIMS_CHECK_ARG(n == 1, "build_tracks: the layout takes 1 size {N}, not %d", n);
  GIMS_CHECK_ARG(sizes[0] >= 0 && sizes[0] <= (1 << 30), "build_tracks: N = %lld is out of range (0 .. 2^30)", (long long)sizes[0]);
  TrkWs w;
  rec.bytes = trk_layout(nullptr, sizes[0], w, &rec);
  return GIMS_OK;
}

// GIMS_AUX_BUILD_TRACKS of gims_run_ops (include/gims_hip.h): every argument check precedes the first HIP call
int build_tracks_aux(const gims_aux_args& x, hipStream_t st) {
  const int64_t n_pairs = x.i[0], n_images = x.i[1], n = x.i[2], mode = x.i[3], work_bytes = x.i[4];
  const float min_score = x.f[0];
  // i[5] is where a later form of this function would be selected: it is read FIRST (see assemble_rows_aux)
  GIMS_CHECK_ARG(x.i[5] == 0, "gims_run_ops: unknown auxiliary function form: build_tracks with i[5] = %lld (i[5] is reserved and must be 0)",
                 (long long)x.i[5]);
  GIMS_CHECK_ARG(n_pairs >= 0 && n_pairs <= (1 << 24), "build_tracks: n_pairs = %lld is out of range (0 .. 2^24)", (long long)n_pairs);
  GIMS_CHECK_ARG(n_images >= 1 && n_images <= (1 << 24), "build_tracks: n_images = %lld is out of range (1 .. 2^24)", (long long)n_images);
  GIMS_CHECK_ARG(n >= 0 && n <= (1 << 30), "build_tracks: N = %lld is out of range (0 .. 2^30)", (long long)n);
  const int64_t min_length = mode & ~(int64_t)GIMS_TRACKS_KEEP_CONFLICTING;
  GIMS_CHECK_ARG(mode >= 0 && min_length >= 2 && min_length <= (1 << 24),
                 "build_tracks: i[3] = %lld: min_length must be 2 .. 2^24, and GIMS_TRACKS_KEEP_CONFLICTING is the only flag", (long long)mode);
  GIMS_CHECK_ARG(min_score == min_score, "build_tracks: min_score is NaN");
  GIMS_CHECK_ARG(x.p[1] && x.p[3] && x.p[4], "build_tracks: start, the output buffer or the counters are NULL");
  GIMS_CHECK_ARG(x.p[0] || n_pairs == 0, "build_tracks: the pair table is NULL while n_pairs = %lld", (long long)n_pairs);
  GIMS_CHECK_ARG((x.p[2] && x.p[5]) || n == 0, "build_tracks: track_of or the workspace is NULL while N = %lld", (long long)n);
  GIMS_CHECK_ARG(((uintptr_t)x.p[0] & 7) == 0, "build_tracks: the pair table must be 8-byte aligned");
  GIMS_CHECK_ARG((((uintptr_t)x.p[1] | (uintptr_t)x.p[2] | (uintptr_t)x.p[3] | (uintptr_t)x.p[4]) & 3) == 0,
                 "build_tracks: start, track_of, the output buffer and the counters must be 4-byte aligned");
  GIMS_CHECK_ARG(((uintptr_t)x.p[5] & 15) == 0, "build_tracks: the workspace must be 16-byte aligned");
  TrkWs w;
  const size_t need = trk_layout(nullptr, n, w);
  GIMS_CHECK_ARG(n == 0 || (work_bytes >= 0 && (size_t)work_bytes >= need), "build_tracks: work_bytes = %lld is below the %zu bytes that N = %lld needs",
                 (long long)work_bytes, need, (long long)n);

  int32_t* counters = (int32_t*)x.p[4];
  int32_t* out = (int32_t*)x.p[3];
  GIMS_HIP(hipMemsetAsync(counters, 0, sizeof(int32_t) * TRK_COUNTERS, st));
  GIMS_HIP(hipMemsetAsync(out, 0, sizeof(int32_t), st));       // indptr[0]
  if (n == 0 || n_pairs == 0) return GIMS_OK;

  trk_layout((void*)x.p[5], n, w);
  const int32_t* start = (const int32_t*)x.p[1];
  int32_t* track_of = (int32_t*)x.p[2];
  const int cap_t = (int)(n / 2);
  int32_t* indptr = out;
  int32_t* obs_image = indptr + cap_t + 1;
  int32_t* obs_keypoint = obs_image + n;
  uint8_t* conflict = (uint8_t*)(obs_keypoint + n);
  const int nn = (int)n, blocks = cdiv(n, TRK_THREADS);

  trk_init_kernel<<<blocks, TRK_THREADS, 0, st>>>(start, (int)n_images, nn, w.parent, w.img);
  GIMS_LAUNCH_CHECK();
  // rows <= n_pairs * N; a workgroup takes 256 rows per step and walks on by the grid's stride
  const int64_t row_blocks = (n_pairs * n + TRK_THREADS - 1) / TRK_THREADS, full = (int64_t)device_cus() * 8;
  trk_union_kernel<<<(unsigned)(row_blocks < full ? row_blocks : full), TRK_THREADS, 0, st>>>((const int64_t*)x.p[0], (int)n_pairs, nn, min_score,
                                                                                              w.parent, counters);
  GIMS_LAUNCH_CHECK();
  GIMS_HIP(hipMemsetAsync(w.size, 0, sizeof(int32_t) * (size_t)n, st));
  trk_flatten_kernel<<<blocks, TRK_THREADS, 0, st>>>(w.parent, nn, w.root, w.size, counters);
  GIMS_LAUNCH_CHECK();
  GIMS_HIP(hipMemsetAsync(w.cursor(), 0, sizeof(int32_t) * (size_t)n, st));
  int rc = trk_scan(w.size, nn, w.sums, w.off, nullptr, st);
  if (rc != GIMS_OK) return rc;
  const int huge = (int)trk_huge(n), cap_huge = (int)trk_cap_huge(n), n_tiles = cdiv(n, TRK_TILE);
  GIMS_HIP(hipMemsetAsync(w.hcnt, 0, sizeof(int32_t) * (size_t)(cap_huge + 1) * (size_t)n_tiles, st));
  GIMS_HIP(hipMemsetAsync(w.n_huge, 0, sizeof(int32_t), st));
  GIMS_HIP(hipMemsetAsync(w.members, 0, sizeof(int32_t) * (size_t)n, st));       // (every slot that is read is claimed; a slot is a node index all the same)
  trk_claim_kernel<<<blocks, TRK_THREADS, 0, st>>>(w.root, w.size, w.off, nn, huge, cap_huge, w.cursor(), w.members, w.n_huge);
  GIMS_LAUNCH_CHECK();
  trk_rank_kernel<<<blocks, TRK_THREADS, 0, st>>>(w.size, w.off, w.members, w.img, nn, huge, w.pos, w.confl);
  GIMS_LAUNCH_CHECK();
  if (cap_huge > 0) {                                          // (a set too small to hold a huge component: a function of N, not of the data)
    trk_huge_count_kernel<<<blocks, TRK_THREADS, 0, st>>>(w.root, w.size, w.cursor(), nn, huge, n_tiles, w.hcnt);
    GIMS_LAUNCH_CHECK();
    trk_huge_scan_kernel<<<cap_huge, TRK_SUMS_THREADS, 0, st>>>(w.hcnt, n_tiles, w.n_huge);
    GIMS_LAUNCH_CHECK();
    trk_huge_rank_kernel<<<n_tiles, TRK_THREADS, 0, st>>>(w.root, w.size, w.off, w.cursor(), w.hcnt, nn, huge, n_tiles, w.pos, w.members);
    GIMS_LAUNCH_CHECK();
    trk_huge_conflict_kernel<<<blocks, TRK_THREADS, 0, st>>>(w.root, w.size, w.off, w.cursor(), w.pos, w.members, w.img, nn, huge, w.confl);
    GIMS_LAUNCH_CHECK();
  }
  trk_keep_kernel<<<blocks, TRK_THREADS, 0, st>>>(w.size, w.confl, nn, (int)min_length, (mode & GIMS_TRACKS_KEEP_CONFLICTING) != 0, w.keep, w.ksize,
                                                  counters);
  GIMS_LAUNCH_CHECK();
  rc = trk_scan(w.keep, nn, w.sums, w.tid, counters + TRK_N_TRACKS, st);
  if (rc != GIMS_OK) return rc;
  rc = trk_scan(w.ksize, nn, w.sums, w.kofs, counters + TRK_N_OBS, st);
  if (rc != GIMS_OK) return rc;
  trk_write_kernel<<<blocks, TRK_THREADS, 0, st>>>(w.root, w.keep, w.tid, w.kofs, w.pos, w.img, w.confl, start, nn, counters, track_of, indptr,
                                                   obs_image, obs_keypoint, conflict);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

}  // namespace gims
