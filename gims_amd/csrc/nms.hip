// DIoU-NMS keypoint thinning on the device: the reference's process_diou_nms / diou_nms (utils/common.py:720-807)
// restated index for index.  include/gims_hip.h, GIMS_AUX_DIOU_NMS, has the arithmetic; tests/nms_ref.py is the NumPy restatement.
//
// One workgroup of 1024 threads per image does everything, so nothing crosses workgroups:
//   1. boxes of the image's keypoints in PROCESSING order (position j of the segment holds row order[off0 + j]), the largest box side;
//   2. a uniform grid over (x1, y1) whose cell side exceeds that side + 1, so that every pair that can interact lies within 3 x 3 cells;
//      a counting sort of the positions by cell (counts, a workgroup scan, a scatter);
//   3. rounds: an undecided position is SUPPRESSED once an earlier partner it does not survive is KEPT, KEPT once all such partners are
//      SUPPRESSED.  Decisions are final and read earlier positions only, so the update is in place; the earliest undecided position is
//      decided in every round, so at most m rounds are needed (a chain of overlapping boxes needs them all).  A position that found an
//      undecided partner remembers the earliest one and does not scan again before that partner is decided;
//   4. the kept positions, compacted in processing order, each mapped back to the lowest row with the same four corners.
// All float32 arithmetic of the pair test goes through the __f*_rn intrinsics: one rounding per operation, nothing contracted.
#include "common.h"

#include <math.h>

namespace gims {

namespace {

constexpr int NMS_THREADS = 1024;
constexpr int NMS_LDS_STATUS = 32768;     // images of up to this many keypoints keep their status bytes in LDS
constexpr int NMS_CELL_SLACK = 64;        // an image of m keypoints may use up to 2 m + NMS_CELL_SLACK grid cells
enum : uint8_t { NMS_UNDECIDED = 0, NMS_KEPT = 1, NMS_SUPPRESSED = 2 };

// The workspace of GIMS_AUX_DIOU_NMS (the formula of include/gims_hip.h; gims_aux_layout reports this routine's offsets)
struct NmsWs {
  float4* box;        // [n] x1, y1, x2, y2 of position j
  float4* aux;        // [n] area, cx, cy, row (int bits)
  int32_t* cell;      // [n] grid cell of position j
  int32_t* items;     // [n] positions sorted by cell
  int32_t* wait;      // [n] the undecided earlier partner position j was last seen to depend on, or -1
  int32_t* cells;     // [2 n + NMS_CELL_SLACK * n_images] per image: the END of every cell's range in items
  uint8_t* status;    // [n] for images that do not fit NMS_LDS_STATUS
};

NmsWs nms_layout(WsLayout& L, int64_t n, int64_t n_images) {
  NmsWs w;
  w.box = L.take<float4>((size_t)n);
  w.aux = L.take<float4>((size_t)n);
  w.cell = L.take<int32_t>((size_t)n);
  w.items = L.take<int32_t>((size_t)n);
  w.wait = L.take<int32_t>((size_t)n);
  w.cells = L.take<int32_t>((size_t)(2 * n + NMS_CELL_SLACK * n_images));
  w.status = L.take<uint8_t>((size_t)n);
  return w;
}

// false: o does not survive i (the test is symmetric in its two boxes)
__device__ __forceinline__ bool nms_survives(const float4 bi, const float4 ai, const float4 bo, const float4 ao, float thr) {
  const float w = fmaxf(0.f, __fadd_rn(__fsub_rn(fminf(bi.z, bo.z), fmaxf(bi.x, bo.x)), 1.f));
  const float h = fmaxf(0.f, __fadd_rn(__fsub_rn(fminf(bi.w, bo.w), fmaxf(bi.y, bo.y)), 1.f));
  const float inter = __fmul_rn(w, h);
  const float iou = __fdiv_rn(inter, __fsub_rn(__fadd_rn(ai.x, ao.x), inter));
  const float ex = __fsub_rn(fmaxf(bi.z, bo.z), fminf(bi.x, bo.x)), ey = __fsub_rn(fmaxf(bi.w, bo.w), fminf(bi.y, bo.y));
  const float diag = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
  const float dx = __fsub_rn(ai.y, ao.y), dy = __fsub_rn(ai.z, ao.z);
  const float cd = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
  const float diou = __fsub_rn(iou, __fdiv_rn(cd, __fadd_rn(diag, 1e-10f)));
  return diou <= thr;
}

// Exclusive prefix of `mine` over the workgroup's threads; *total gets the sum.  scan: NMS_THREADS ints of LDS, free on entry.
__device__ __forceinline__ int nms_block_scan(int mine, int* scan, int* total) {
  const int t = threadIdx.x;
  scan[t] = mine;
  __syncthreads();
  for (int d = 1; d < NMS_THREADS; d <<= 1) {
    const int v = t >= d ? scan[t - d] : 0;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  const int incl = scan[t];
  *total = scan[NMS_THREADS - 1];
  __syncthreads();
  return incl - mine;
}

__device__ __forceinline__ int nms_cell_axis(float v, double cs, int cells) {
  const double q = floor((double)v / cs);          // monotone in v; the clamp keeps neighbours within one cell
  return q < 0.0 ? 0 : (q > (double)(cells - 1) ? cells - 1 : (int)q);
}

__global__ __launch_bounds__(NMS_THREADS) void diou_nms_kernel(const float* __restrict__ kp4, const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ offsets, int32_t* __restrict__ keep,
                                                               int32_t* __restrict__ count, NmsWs W, int n, int n_images, int height, int width,
                                                               float radius, float thr) {
  __shared__ uint8_t lds_status[NMS_LDS_STATUS];
  __shared__ int s_scan[NMS_THREADS];
  __shared__ unsigned s_maxside, s_maxx, s_maxy;
  __shared__ int s_bad, s_nx, s_ny;
  __shared__ double s_cs;
  const int b = blockIdx.x, t = threadIdx.x;
  const int off0 = min(max(offsets[b], 0), n);
  const int off1 = max(off0, min(max(offsets[b + 1], 0), n));
  const int m = off1 - off0;                       // the same for every thread: the early return is uniform
  if (m == 0) {
    if (t == 0) count[b] = 0;
    return;
  }
  uint8_t* st = m <= NMS_LDS_STATUS ? lds_status : W.status + off0;
  float4* box = W.box + off0;
  float4* aux = W.aux + off0;
  int32_t* cell = W.cell + off0;
  int32_t* items = W.items + off0;
  int32_t* wait = W.wait + off0;
  int32_t* cend = W.cells + 2 * (int64_t)off0 + (int64_t)NMS_CELL_SLACK * b;       // up to 2 m + NMS_CELL_SLACK entries are this image's
  if (t == 0) { s_maxside = s_maxx = s_maxy = 0u; s_bad = 0; }
  __syncthreads();

  // 1. boxes in processing order
  const bool size_mode = radius == 0.f;
  {
    float side = 0.f, mx = 0.f, my = 0.f;
    int bad = 0;
    for (int j = t; j < m; j += NMS_THREADS) {
      const int r = order[off0 + j];
      bool ok = r >= off0 && r < off1;
      float x = 0.f, y = 0.f, size = 0.f;
      if (ok) {
        const float* k = kp4 + 4 * (int64_t)r;
        x = k[0]; y = k[1]; size = k[2];
        ok = isfinite(x) && isfinite(y) && isfinite(size) && !(size_mode && size < 0.f);
      }
      if (ok) {
        const double half = (size_mode ? (double)size : (double)radius) / 2;
        const float x1 = (float)((double)x - half), y1 = (float)((double)y - half), x2 = (float)((double)x + half), y2 = (float)((double)y + half);
        const float sx = __fsub_rn(x2, x1), sy = __fsub_rn(y2, y1);
        box[j] = make_float4(x1, y1, x2, y2);
        aux[j] = make_float4(__fmul_rn(__fadd_rn(sx, 1.f), __fadd_rn(sy, 1.f)), __fdiv_rn(__fadd_rn(x1, x2), 2.f), __fdiv_rn(__fadd_rn(y1, y2), 2.f),
                             __int_as_float(r));
        side = fmaxf(side, fmaxf(sx, sy));
        mx = fmaxf(mx, x1);
        my = fmaxf(my, y1);
        st[j] = NMS_UNDECIDED;
        wait[j] = -1;
      } else {
        st[j] = NMS_SUPPRESSED;                    // never kept, never a partner, never binned
        ++bad;
      }
    }
    if (side > 0.f) atomicMax(&s_maxside, __float_as_uint(side));       // all three are >= 0: their bits order like the values
    if (mx > 0.f) atomicMax(&s_maxx, __float_as_uint(mx));
    if (my > 0.f) atomicMax(&s_maxy, __float_as_uint(my));
    if (bad) atomicAdd(&s_bad, bad);
  }
  __syncthreads();

  // 2. the grid: cell side above (largest side + 1), doubled until the cells fit the image's share of the workspace.  It covers the stated
  // extent or the corners that are there, whichever is smaller: an extent far too large costs nothing
  if (t == 0) {
    const double ew = fmin((double)width, (double)__uint_as_float(s_maxx) + 1.0), eh = fmin((double)height, (double)__uint_as_float(s_maxy) + 1.0);
    double cs = ((double)__uint_as_float(s_maxside) * (1.0 + 1.0 / 1048576.0) + 1.0) * 1.001;
    const double budget = 2.0 * m + (NMS_CELL_SLACK - 1);
    double fx = ceil(ew / cs), fy = ceil(eh / cs);
    while (fx * fy > budget) {
      cs *= 2.0;
      fx = ceil(ew / cs);
      fy = ceil(eh / cs);
    }
    s_cs = cs;
    s_nx = fx < 1.0 ? 1 : (int)fx;
    s_ny = fy < 1.0 ? 1 : (int)fy;
  }
  __syncthreads();
  const double cs = s_cs;
  const int nx = s_nx, ny = s_ny, ncell = nx * ny;
  for (int c = t; c < ncell; c += NMS_THREADS) cend[c] = 0;
  __syncthreads();
  for (int j = t; j < m; j += NMS_THREADS) {
    if (st[j] != NMS_UNDECIDED) continue;
    const float4 bj = box[j];
    const int c = nms_cell_axis(bj.y, cs, ny) * nx + nms_cell_axis(bj.x, cs, nx);
    cell[j] = c;
    atomicAdd(&cend[c], 1);
  }
  __syncthreads();
  {
    const int ch = (ncell + NMS_THREADS - 1) / NMS_THREADS, lo = min(t * ch, ncell), hi = min(lo + ch, ncell);
    int sum = 0, total;
    for (int c = lo; c < hi; ++c) sum += cend[c];
    int run = nms_block_scan(sum, s_scan, &total);
    for (int c = lo; c < hi; ++c) { const int v = cend[c]; cend[c] = run; run += v; }
  }
  __syncthreads();
  for (int j = t; j < m; j += NMS_THREADS) {
    if (st[j] != NMS_UNDECIDED) continue;
    items[atomicAdd(&cend[cell[j]], 1)] = j;       // the start of every cell moves to its end: cell c is items[c ? cend[c-1] : 0 .. cend[c])
  }
  __syncthreads();

  // 3. rounds.  A position that found an undecided partner waits for THAT partner's decision before it looks again: decisions are final
  // and the earliest undecided position never waits on an undecided one, so this only skips evaluations that could not have decided it
  for (int round = 0; round <= m; ++round) {
    int undecided = 0;
    for (int j = t; j < m; j += NMS_THREADS) {
      if (st[j] != NMS_UNDECIDED) continue;
      const int wq = wait[j];
      if (wq >= 0 && st[wq] == NMS_UNDECIDED) { undecided = 1; continue; }
      const float4 bj = box[j], aj = aux[j];
      const int c = cell[j], cx = c % nx, cy = c / nx;
      bool suppressed = false;
      int pending = m;                             // the earliest undecided partner, m: none
      for (int yy = max(cy - 1, 0); yy <= min(cy + 1, ny - 1) && !suppressed; ++yy) {
        for (int xx = max(cx - 1, 0); xx <= min(cx + 1, nx - 1) && !suppressed; ++xx) {
          const int cc = yy * nx + xx;
          const int hi = cend[cc];
          for (int p = cc ? cend[cc - 1] : 0; p < hi; ++p) {
            const int q = items[p];
            if (q >= j) continue;
            const uint8_t sq = st[q];
            if (sq == NMS_SUPPRESSED) continue;
            const float4 bq = box[q];
            // boxes that do not overlap (w == 0 or h == 0) give diou <= 0 < thr: the test below would say "survives"
            if (!(__fadd_rn(__fsub_rn(fminf(bq.z, bj.z), fmaxf(bq.x, bj.x)), 1.f) > 0.f) ||
                !(__fadd_rn(__fsub_rn(fminf(bq.w, bj.w), fmaxf(bq.y, bj.y)), 1.f) > 0.f))
              continue;
            if (nms_survives(bq, aux[q], bj, aj, thr)) continue;
            if (sq == NMS_KEPT) { suppressed = true; break; }
            pending = min(pending, q);
          }
        }
      }
      if (suppressed) st[j] = NMS_SUPPRESSED;
      else if (pending == m) st[j] = NMS_KEPT;
      else { wait[j] = pending; undecided = 1; }
    }
    if (!__syncthreads_or(undecided)) break;
  }

  // 4. compaction in processing order, with the map-back to the lowest row of equal corners (equal corners share a cell)
  {
    const int ch = (m + NMS_THREADS - 1) / NMS_THREADS, lo = min(t * ch, m), hi = min(lo + ch, m);
    int kept = 0, total;
    for (int j = lo; j < hi; ++j) kept += st[j] == NMS_KEPT;
    int at = nms_block_scan(kept, s_scan, &total);
    for (int j = lo; j < hi; ++j) {
      if (st[j] != NMS_KEPT) continue;
      const float4 bj = box[j];
      int row = __float_as_int(aux[j].w);
      const int c = cell[j], end = cend[c];
      for (int p = c ? cend[c - 1] : 0; p < end; ++p) {
        const int q = items[p];
        const float4 bq = box[q];
        if (bq.x == bj.x && bq.y == bj.y && bq.z == bj.z && bq.w == bj.w) row = min(row, __float_as_int(aux[q].w));
      }
      keep[off0 + at++] = row;
    }
    for (int k = total + t; k < m; k += NMS_THREADS) keep[off0 + k] = -1;
    if (t == 0) {
      count[b] = total;
      if (s_bad) atomicAdd(&count[n_images], s_bad);
    }
  }
}

}  // namespace

// the sizes that lay the workspace out: the op and gims_aux_layout refuse the same values
static int nms_check_sizes(int64_t n, int64_t n_images) {
  GIMS_CHECK_ARG(n >= 0 && n <= (1 << 29), "diou_nms: n = %lld is out of range (0 .. 2^29)", (long long)n);
  GIMS_CHECK_ARG(n_images >= 1 && n_images <= (1 << 20), "diou_nms: n_images = %lld (1 .. 2^20)", (long long)n_images);
  return GIMS_OK;
}

// gims_aux_layout for GIMS_AUX_DIOU_NMS: sizes = {n, n_images}, the workspace
int diou_nms_aux_layout(const int64_t* sizes, int n, WsRecord& rec) {
  GIMS_CHECK_ARG(n == 2, "diou_nms: the layout takes 2 sizes {n, n_images}, not %d", n);
  if (const int rc = nms_check_sizes(sizes[0], sizes[1])) return rc;
  WsLayout L(nullptr, &rec);
  nms_layout(L, sizes[0], sizes[1]);
  rec.bytes = L.bytes();
  return GIMS_OK;
}

int diou_nms_aux(const gims_aux_args& x, hipStream_t st) {
  const int64_t n = x.i[0], n_images = x.i[1], h = x.i[2], w = x.i[3], work_bytes = x.i[4];
  const float radius = x.f[0], thr = x.f[1];
  if (const int rc = nms_check_sizes(n, n_images)) return rc;
  GIMS_CHECK_ARG(h >= 1 && w >= 1 && h <= INT32_MAX && w <= INT32_MAX, "diou_nms: extent %lld x %lld (height and width are at least 1)", (long long)h,
                 (long long)w);
  GIMS_CHECK_ARG(isfinite(radius) && radius >= 0.f, "diou_nms: radius = %g (finite, > 0 for fixed boxes, 0 for boxes from the size)", (double)radius);
  GIMS_CHECK_ARG(isfinite(thr) && thr > 0.f && thr < 1.f, "diou_nms: iou_thresh = %g is outside (0, 1)", (double)thr);
  GIMS_CHECK_ARG(x.i[5] == 0, "diou_nms: i[5] is reserved and must be 0");
  WsLayout sizing(nullptr);
  nms_layout(sizing, n, n_images);
  GIMS_CHECK_ARG(work_bytes >= 0 && (uint64_t)work_bytes >= sizing.bytes(), "diou_nms: workspace of %lld bytes, %lld needed", (long long)work_bytes,
                 (long long)sizing.bytes());
  if (n == 0) return GIMS_OK;
  GIMS_CHECK_ARG(x.p[0] && x.p[1] && x.p[2] && x.p[3] && x.p[4] && x.p[5], "diou_nms: kp4, order, offsets, keep, count and work must not be NULL");
  GIMS_CHECK_ARG(((uintptr_t)x.p[5] & 15) == 0, "diou_nms: work must be 16-byte aligned");
  WsLayout L(const_cast<void*>(x.p[5]));
  const NmsWs W = nms_layout(L, n, n_images);
  int32_t* count = (int32_t*)const_cast<void*>(x.p[4]);
  GIMS_HIP(hipMemsetAsync(count + n_images, 0, sizeof(int32_t), st));
  diou_nms_kernel<<<(unsigned)n_images, NMS_THREADS, 0, st>>>((const float*)x.p[0], (const int32_t*)x.p[1], (const int32_t*)x.p[2],
                                                              (int32_t*)const_cast<void*>(x.p[3]), count, W, (int)n, (int)n_images, (int)h, (int)w, radius,
                                                              thr);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

}  // namespace gims
