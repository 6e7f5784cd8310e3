// Delaunay graph construction on the GPU (D-GIMS: the reference's build_graph_from_keypoints_Delaunay, models/agc.py:718-751) for a
// batch of images, every stage one launch for all images (blockIdx.y = image), no host synchronisation.
//
//   K1 grid    per image: bounding box, a uniform grid of about 2 points per cell filled by counting sort, every cell sorted by
//              (x, y, id); of a group of identical coordinates only the lowest id is a vertex, the others stay isolated (degree 0)
//   K2 star    one thread per vertex, in cell order: its Delaunay star, computed on its own.  The nearest neighbour is always a Delaunay
//              edge; from an edge p -> q the next neighbour is the point left of it whose circle through p and q holds no other such point
//              (a replacement scan over grid rings, bounded by the current circle); the walk ends where it closes, or at a hull edge (no
//              point to the left), after which it walks the other way from the nearest neighbour.  Two passes: degrees, then (after the
//              scan) the same walk writes the neighbours, sorted ascending.  Filter-only predicates (delaunay_pred.h): a point whose walk
//              meets a predicate the float64 filter cannot decide goes to the image's fallback list instead
//   K3 fallback  the listed points' stars again, with the exact predicates (the only kernel whose exact expansions live in scratch);
//              every decision the filter can make is the same in both, so the stars of all points agree
//   K4 scan    degrees -> indptr; kept = 0..n-1
//   K5 check   every edge must be present in both directions (a set bit becomes an exception on the host, never a silent result)
//
// The graph is the unique Delaunay triangulation under the tie rule of delaunay_pred.h (symbolic perturbation of the lift by id).
#include "common.h"
#include "delaunay_pred.h"

#include <vector>

namespace gims {

constexpr int DT_MAX_N = 32768;          // the library's per-image limit (gims_agc_max_keypoints)
constexpr int DT_INFO_OVERFLOW = 1, DT_INFO_DEGENERATE = 4, DT_INFO_ASYMMETRIC = 8;
enum { DT_C_FALLBACK = 0, DT_C_HULL = 1, DT_C_DUP = 2, DT_C_TRI = 3, DT_C_FLAGS = 4 };
constexpr int DT_UND = dpred::DP_UNDECIDED;

struct DtGrid {
  double minx, miny, side, inv, tol;     // cell (cx, cy) covers [minx + cx side, minx + (cx + 1) side) x ..., up to `tol`
  int gx, gy, bad, pad;                  // bad: a non-finite coordinate
};

struct DtWs {
  const float* kpts; int32_t* kept; int32_t* indptr; int32_t* indices; int32_t* info;
  int n, max_edges_dir, ncell_cap, pad;
  int32_t* cstart;   // [ncell_cap + 1] cell offsets into cid / cpt
  int32_t* ccnt;     // [ncell_cap] vertices of the cell: they lead its segment, its duplicates (stored as ~id) follow
  int32_t* cfill;    // [ncell_cap]
  int32_t* csort;    // [n]
  int32_t* cid;      // [n]
  float2* cpt;       // [n] coordinates in cid order
  int32_t* deg;      // [n] by id
  int32_t* fb;       // [n] the fallback list
  int32_t* fbmark;   // [n] by id
  int32_t* cnt;      // [16] counters (DT_C_*)
  DtGrid* grid;
};

__device__ __forceinline__ void dt_cell_of(const DtGrid& g, double x, double y, int& cx, int& cy) {
  cx = (int)((x - g.minx) * g.inv);
  cy = (int)((y - g.miny) * g.inv);
  cx = cx < 0 ? 0 : (cx >= g.gx ? g.gx - 1 : cx);
  cy = cy < 0 ? 0 : (cy >= g.gy ? g.gy - 1 : cy);
}

// exclusive scan of v[0..m) in place by one 1024-thread block; returns the total
__device__ int dt_block_scan(int32_t* v, int m, int* part) {
  const int tid = threadIdx.x, per = (m + 1023) / 1024, s = tid * per, e = min(s + per, m);
  int sum = 0;
  for (int i = s; i < e; ++i) sum += v[i];
  part[tid] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int t = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += t;
    __syncthreads();
  }
  int run = part[tid] - sum;
  for (int i = s; i < e; ++i) {
    const int c = v[i];
    v[i] = run;
    run += c;
  }
  const int total = part[1023];
  __syncthreads();
  return total;
}

__device__ __forceinline__ bool dt_less(float ax, float ay, int ia, float bx, float by, int ib) {
  return ax < bx || (ax == bx && (ay < by || (ay == by && ia < ib)));
}

// K1: one 1024-thread block per image
__global__ __launch_bounds__(1024) void dt_grid_kernel(const DtWs* __restrict__ wss) {
  const DtWs& w = wss[blockIdx.y];
  const int n = w.n, tid = threadIdx.x;
  __shared__ float red[4][16];
  __shared__ int part[1024];
  __shared__ int sbad, sdup;
  __shared__ DtGrid sg;
  if (tid == 0) { sbad = 0; sdup = 0; }
  float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
  int bad = 0;
  for (int i = tid; i < n; i += 1024) {
    const float x = w.kpts[2 * i], y = w.kpts[2 * i + 1];
    if (!(isfinite(x) && isfinite(y))) { bad = 1; continue; }
    mnx = fminf(mnx, x); mny = fminf(mny, y); mxx = fmaxf(mxx, x); mxy = fmaxf(mxy, y);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mnx = fminf(mnx, __shfl_xor(mnx, o, 64)); mny = fminf(mny, __shfl_xor(mny, o, 64));
    mxx = fmaxf(mxx, __shfl_xor(mxx, o, 64)); mxy = fmaxf(mxy, __shfl_xor(mxy, o, 64));
  }
  __syncthreads();
  if (bad) atomicOr(&sbad, 1);
  if ((tid & 63) == 0) { red[0][tid >> 6] = mnx; red[1][tid >> 6] = mny; red[2][tid >> 6] = mxx; red[3][tid >> 6] = mxy; }
  if (tid < 16) w.cnt[tid] = 0;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < 16; ++i) {
      mnx = fminf(mnx, red[0][i]); mny = fminf(mny, red[1][i]); mxx = fmaxf(mxx, red[2][i]); mxy = fmaxf(mxy, red[3][i]);
    }
    DtGrid g;
    g.bad = sbad || n == 0;
    g.pad = 0;
    if (g.bad) {
      g.minx = g.miny = 0.0; g.side = g.inv = 1.0; g.tol = 0.0; g.gx = g.gy = 1;
      w.cnt[DT_C_FLAGS] = DT_INFO_DEGENERATE;
    } else {
      const double W = (double)mxx - mnx, H = (double)mxy - mny, T = n / 2 > 1 ? n / 2 : 1;
      double side = fmax(sqrt(W * H / T), fmax(W, H) / T);
      if (!(side > 0.0)) side = 1.0;
      int gx, gy;
      for (;;) {            // (W / side + 1)(H / side + 1) <= 3 T + 1 <= ncell_cap; the loop only absorbs rounding
        gx = (int)(W / side) + 1;
        gy = (int)(H / side) + 1;
        if ((int64_t)gx * gy <= w.ncell_cap) break;
        side *= 1.01;
      }
      g.minx = mnx; g.miny = mny; g.side = side; g.inv = 1.0 / side; g.gx = gx; g.gy = gy;
      g.tol = 1e-9 * (fabs((double)mnx) + fabs((double)mny) + W + H + side);
    }
    sg = g;
    *w.grid = g;
  }
  __syncthreads();
  const DtGrid g = sg;
  const int ncell = g.gx * g.gy;
  for (int c = tid; c < ncell; c += 1024) w.cfill[c] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 1024) {
    w.deg[i] = 0;
    w.fbmark[i] = 0;
    w.kept[i] = i;
    int cx = 0, cy = 0;
    if (!g.bad) dt_cell_of(g, w.kpts[2 * i], w.kpts[2 * i + 1], cx, cy);
    atomicAdd(&w.cfill[cy * g.gx + cx], 1);
  }
  __syncthreads();
  const int total = dt_block_scan(w.cfill, ncell, part);
  if (tid == 0) w.cstart[ncell] = total;
  for (int c = tid; c < ncell; c += 1024) w.cstart[c] = w.cfill[c];
  __syncthreads();
  for (int i = tid; i < n; i += 1024) {
    int cx = 0, cy = 0;
    if (!g.bad) dt_cell_of(g, w.kpts[2 * i], w.kpts[2 * i + 1], cx, cy);
    const int c = cy * g.gx + cx;
    w.csort[atomicAdd(&w.cfill[c], 1)] = i;           // cfill now holds the running end of each cell
  }
  __syncthreads();
  int dups = 0;
  for (int c = tid; c < ncell; c += 1024) {
    const int s = w.cstart[c], e = w.cstart[c + 1];
    for (int j = s + 1; j < e; ++j) {                 // insertion sort by (x, y, id): a few points per cell
      const int id = w.csort[j];
      const float x = w.kpts[2 * id], y = w.kpts[2 * id + 1];
      int t = j - 1;
      while (t >= s) {
        const int o = w.csort[t];
        if (!dt_less(x, y, id, w.kpts[2 * o], w.kpts[2 * o + 1], o)) break;
        w.csort[t + 1] = o;
        --t;
      }
      w.csort[t + 1] = id;
    }
    int nv = 0;
    for (int j = s; j < e; ++j) {                     // vertices first (the lowest id of each coordinate group) ...
      const int id = w.csort[j];
      const float x = w.kpts[2 * id], y = w.kpts[2 * id + 1];
      if (j > s && w.kpts[2 * w.csort[j - 1]] == x && w.kpts[2 * w.csort[j - 1] + 1] == y) continue;
      w.cid[s + nv] = id;
      w.cpt[s + nv] = make_float2(x, y);
      ++nv;
    }
    int nd = nv;
    for (int j = s + 1; j < e; ++j) {                 // ... then the duplicates
      const int id = w.csort[j];
      const float x = w.kpts[2 * id], y = w.kpts[2 * id + 1];
      if (w.kpts[2 * w.csort[j - 1]] == x && w.kpts[2 * w.csort[j - 1] + 1] == y) {
        w.cid[s + nd] = ~id;
        w.cpt[s + nd] = make_float2(x, y);
        ++nd;
      }
    }
    w.ccnt[c] = nv;
    dups += e - s - nv;
  }
  if (dups) atomicAdd(&sdup, dups);
  __syncthreads();
  if (tid == 0) w.cnt[DT_C_DUP] = sdup;
}

// calls f(cell) for every cell of the square ring at Chebyshev distance k around (cx, cy) that lies in the grid; false from f stops
template <class F>
__device__ __forceinline__ bool dt_ring(const DtGrid& g, int cx, int cy, int k, F&& f) {
  const int y0 = cy - k, y1 = cy + k;
  for (int y = max(y0, 0); y <= min(y1, g.gy - 1); ++y) {
    if (y == y0 || y == y1) {
      for (int x = max(cx - k, 0); x <= min(cx + k, g.gx - 1); ++x)
        if (!f(x, y)) return false;
    } else {
      if (cx - k >= 0 && !f(cx - k, y)) return false;
      if (cx + k < g.gx && !f(cx + k, y)) return false;
    }
  }
  return true;
}

struct DtPoint { double x, y; int id; };

// nearest vertex to p (lowest id among the nearest); 0, or DT_UND
template <bool EXACT>
__device__ int dt_nearest(const DtWs& w, const DtGrid& g, const DtPoint& p, int cx, int cy, int kmax, DtPoint& q) {
  q.id = -1;
  double best = 0.0;
  bool und = false;
  for (int k = 0; k <= kmax; ++k) {
    if (q.id >= 0) {
      const double dmin = (k - 1) * g.side - g.tol;
      if (dmin > 0.0 && dmin * dmin > best * (1.0 + 1e-9)) break;
    }
    dt_ring(g, cx, cy, k, [&](int x, int y) {
      const int c = y * g.gx + x, s = w.cstart[c], e = s + w.ccnt[c];
      for (int j = s; j < e; ++j) {
        const int sid = w.cid[j];
        if (sid == p.id) continue;
        const float2 sp = w.cpt[j];
        int cmp = -1;
        if (q.id >= 0) {
          cmp = dpred::dist_cmp<EXACT>(p.x, p.y, sp.x, sp.y, q.x, q.y);
          if (cmp == DT_UND) { und = true; return false; }
          if (cmp == 0) cmp = sid < q.id ? -1 : 1;
        }
        if (cmp < 0) {
          q.id = sid; q.x = sp.x; q.y = sp.y;
          const double dx = q.x - p.x, dy = q.y - p.y;
          best = dx * dx + dy * dy;
        }
      }
      return true;
    });
    if (und) return DT_UND;
  }
  return 0;
}

// the vertex r left of a -> b whose circle through a, b holds no other vertex left of a -> b (r.id = -1: none, a -> b is a hull edge);
// grid rings around the cell (cx, cy) of o, o = a or b; 0, or DT_UND
template <bool EXACT>
__device__ int dt_third(const DtWs& w, const DtGrid& g, const DtPoint& a, const DtPoint& b, const DtPoint& o, int cx, int cy, int kmax,
                        DtPoint& r) {
  r.id = -1;
  double ccx = 0.0, ccy = 0.0, rad = INFINITY, reach = INFINITY;
  const double ux = b.x - a.x, uy = b.y - a.y, ulen = sqrt(ux * ux + uy * uy);
  const double half_diag = 0.70711 * g.side + g.tol;
  bool und = false;
  auto circle = [&]() {        // a safe enclosing disc of the circle through a, b, r (float64 centre, inflated by its error bound)
    const double rx = r.x - a.x, ry = r.y - a.y;
    const double t1 = ux * ry, t2 = uy * rx, D = 2.0 * (t1 - t2);
    const double errD = 32.0 * dpred::DP_EPS * (fabs(t1) + fabs(t2));
    if (!(D > 0.0) || errD > 1e-3 * D) { rad = INFINITY; reach = INFINITY; return; }
    const double rel = errD / D + 1e-13;
    const double b2 = ux * ux + uy * uy, r2 = rx * rx + ry * ry;
    const double ox = (ry * b2 - uy * r2) / D, oy = (ux * r2 - rx * b2) / D;
    ccx = a.x + ox; ccy = a.y + oy;
    rad = sqrt(ox * ox + oy * oy) * (1.0 + 8.0 * rel) + g.tol;
    const double dx = o.x - ccx, dy = o.y - ccy;
    reach = sqrt(dx * dx + dy * dy) * (1.0 + 1e-12) + rad;
    if (!isfinite(reach)) { rad = INFINITY; reach = INFINITY; }
  };
  for (int k = 0; k <= kmax; ++k) {
    if (r.id >= 0 && (k - 1) * g.side - g.tol > reach) break;
    dt_ring(g, cx, cy, k, [&](int x, int y) {
      const double x0 = g.minx + x * g.side, y0 = g.miny + y * g.side;
      if (r.id < 0) {            // the open half-plane left of a -> b
        const double mx = x0 + 0.5 * g.side - a.x, my = y0 + 0.5 * g.side - a.y;
        if (ux * my - uy * mx < -half_diag * ulen * (1.0 + 1e-12)) return true;
      } else if (rad < INFINITY) {
        const double ddx = fmax(fmax(x0 - ccx, ccx - (x0 + g.side)), 0.0), ddy = fmax(fmax(y0 - ccy, ccy - (y0 + g.side)), 0.0);
        if (ddx * ddx + ddy * ddy > rad * rad) return true;
      }
      const int c = y * g.gx + x, s = w.cstart[c], e = s + w.ccnt[c];
      for (int j = s; j < e; ++j) {
        const int sid = w.cid[j];
        if (sid == a.id || sid == b.id) continue;
        const float2 sp = w.cpt[j];
        const int ori = dpred::orient<EXACT>(a.x, a.y, b.x, b.y, sp.x, sp.y);
        if (ori == DT_UND) { und = true; return false; }
        if (ori <= 0) continue;
        if (r.id >= 0) {
          const int ic = dpred::incircle_sos<EXACT>(a.x, a.y, a.id, b.x, b.y, b.id, r.x, r.y, r.id, sp.x, sp.y, sid);
          if (ic == DT_UND) { und = true; return false; }
          if (ic <= 0) continue;
        }
        r.id = sid; r.x = sp.x; r.y = sp.y;
        circle();
      }
      return true;
    });
    if (und) return DT_UND;
  }
  return 0;
}

// the star of p: 0 (deg, hull, tri set), DT_UND, or -1 (a walk that did not end: inconsistent input to the walk)
template <bool EXACT, bool FILL>
__device__ int dt_walk(const DtWs& w, const DtGrid& g, const DtPoint& p, int32_t* out, int cap, int& deg, int& hull, int& tri) {
  deg = 0; hull = 0; tri = 0;
  int cx, cy;
  dt_cell_of(g, p.x, p.y, cx, cy);
  const int kmax = max(max(cx, g.gx - 1 - cx), max(cy, g.gy - 1 - cy));
  DtPoint q0, q, r;
  if (dt_nearest<EXACT>(w, g, p, cx, cy, kmax, q0) == DT_UND) return DT_UND;
  if (q0.id < 0) return 0;                      // the only vertex of its image
  auto emit = [&](int v) {
    if (FILL && deg < cap) out[deg] = v;
    ++deg;
  };
  emit(q0.id);
  q = q0;
  bool closed = false;
  int steps = 0;
  for (; steps < w.n; ++steps) {                // counter-clockwise around p
    if (dt_third<EXACT>(w, g, p, q, p, cx, cy, kmax, r) == DT_UND) return DT_UND;
    if (r.id < 0) { hull = 1; break; }
    tri = 1;
    if (r.id == q0.id) { closed = true; break; }
    emit(r.id);
    q = r;
  }
  if (!closed) {
    q = q0;
    for (; steps < w.n; ++steps) {              // clockwise from the nearest neighbour, to the other hull edge
      if (dt_third<EXACT>(w, g, q, p, p, cx, cy, kmax, r) == DT_UND) return DT_UND;
      if (r.id < 0) break;
      tri = 1;
      emit(r.id);
      q = r;
    }
  }
  return steps < w.n ? 0 : -1;
}

template <bool EXACT, bool FILL>
__device__ void dt_point(const DtWs& w, const DtGrid& g, int pid) {
  const DtPoint p = {w.kpts[2 * pid], w.kpts[2 * pid + 1], pid};
  int deg, hull, tri;
  int32_t* out = nullptr;
  int cap = 0;
  if (FILL) {
    out = w.indices + w.indptr[pid];
    cap = w.indptr[pid + 1] - w.indptr[pid];
  }
  const int rc = dt_walk<EXACT, FILL>(w, g, p, out, cap, deg, hull, tri);
  if (rc == DT_UND) {
    if (EXACT || FILL) atomicOr(&w.cnt[DT_C_FLAGS], DT_INFO_ASYMMETRIC);     // cannot happen: a point the filter failed on is listed in pass 0
    else { w.fbmark[pid] = 1; w.fb[atomicAdd(&w.cnt[DT_C_FALLBACK], 1)] = pid; }
    return;
  }
  if (rc != 0) { atomicOr(&w.cnt[DT_C_FLAGS], DT_INFO_ASYMMETRIC); return; }
  if (!FILL) {
    w.deg[pid] = deg;
    if (hull) atomicAdd(&w.cnt[DT_C_HULL], 1);
    if (tri) atomicOr(&w.cnt[DT_C_TRI], 1);
    return;
  }
  if (deg != cap) { atomicOr(&w.cnt[DT_C_FLAGS], DT_INFO_ASYMMETRIC); return; }
  for (int j = 1; j < deg; ++j) {               // ascending ids (the adaptive build's CSR convention)
    const int v = out[j];
    int t = j - 1;
    while (t >= 0 && out[t] > v) { out[t + 1] = out[t]; --t; }
    out[t + 1] = v;
  }
}

// K2: thread per vertex in cell order; filter-only (no scratch)
template <bool FILL>
__global__ __launch_bounds__(256) void dt_star_kernel(const DtWs* __restrict__ wss) {
  const DtWs& w = wss[blockIdx.y];
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= w.n) return;
  const DtGrid g = *w.grid;
  if (g.bad) return;
  const int pid = w.cid[k];
  if (pid < 0) return;
  if (FILL && (w.fbmark[pid] || (w.cnt[DT_C_FLAGS] & DT_INFO_OVERFLOW))) return;
  dt_point<false, FILL>(w, g, pid);
}

// K3: the fallback list, exact predicates
template <bool FILL>
__global__ __launch_bounds__(64) void dt_fallback_kernel(const DtWs* __restrict__ wss) {
  const DtWs& w = wss[blockIdx.y];
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= w.cnt[DT_C_FALLBACK] || j >= w.n) return;
  if (FILL && (w.cnt[DT_C_FLAGS] & DT_INFO_OVERFLOW)) return;
  const DtGrid g = *w.grid;
  dt_point<true, FILL>(w, g, w.fb[j]);
}

// K4: indptr = exclusive scan of the degrees; overflow when the edges do not fit the caller's buffer
__global__ __launch_bounds__(1024) void dt_scan_kernel(const DtWs* __restrict__ wss) {
  const DtWs& w = wss[blockIdx.y];
  __shared__ int part[1024];
  const int n = w.n;
  for (int i = threadIdx.x; i < n; i += 1024) w.indptr[i] = w.deg[i];
  __syncthreads();
  const int total = dt_block_scan(w.indptr, n, part);
  if (threadIdx.x == 0) {
    w.indptr[n] = total;
    if (total > w.max_edges_dir) atomicOr(&w.cnt[DT_C_FLAGS], DT_INFO_OVERFLOW);
  }
}

// K5: every list ascending, no self loop, every edge present both ways
__global__ __launch_bounds__(256) void dt_check_kernel(const DtWs* __restrict__ wss) {
  const DtWs& w = wss[blockIdx.y];
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= w.n || (w.cnt[DT_C_FLAGS] & (DT_INFO_OVERFLOW | DT_INFO_DEGENERATE))) return;
  const int s = w.indptr[u], e = w.indptr[u + 1];
  bool ok = true;
  for (int t = s; t < e && ok; ++t) {
    const int v = w.indices[t];
    if (v < 0 || v >= w.n || v == u || (t > s && w.indices[t - 1] >= v)) { ok = false; break; }
    int lo = w.indptr[v], hi = w.indptr[v + 1];
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (w.indices[mid] < u) lo = mid + 1;
      else hi = mid;
    }
    ok = lo < w.indptr[v + 1] && w.indices[lo] == u;
  }
  if (!ok) atomicOr(&w.cnt[DT_C_FLAGS], DT_INFO_ASYMMETRIC);
}

__global__ void dt_info_kernel(const DtWs* __restrict__ wss) {
  const DtWs& w = wss[blockIdx.y];
  if (threadIdx.x != 0) return;
  int flags = w.cnt[DT_C_FLAGS];
  const int distinct = w.n - w.cnt[DT_C_DUP];
  if (distinct < 3 || w.cnt[DT_C_TRI] == 0) flags |= DT_INFO_DEGENERATE;
  const int e = w.indptr[w.n];
  const int v[8] = {w.n, e, e / 2, w.cnt[DT_C_DUP], w.cnt[DT_C_HULL], w.cnt[DT_C_FALLBACK], 0, flags};
  for (int i = 0; i < 8; ++i) w.info[i] = v[i];
}

// One image's part of the workspace (sizing: L on a null base, w a scratch record)
static void dt_layout(int n, WsLayout& L, DtWs& w) {
  const int T = n / 2 > 1 ? n / 2 : 1, ncap = 3 * T + 2;
  w.cstart = L.take<int32_t>(ncap + 1);
  w.ccnt = L.take<int32_t>(ncap);
  w.cfill = L.take<int32_t>(ncap);
  w.csort = L.take<int32_t>(n);
  w.cid = L.take<int32_t>(n);
  w.cpt = L.take<float2>(n);
  w.deg = L.take<int32_t>(n);
  w.fb = L.take<int32_t>(n);
  w.fbmark = L.take<int32_t>(n);
  w.cnt = L.take<int32_t>(16);
  w.grid = L.take<DtGrid>(1);
  w.n = n; w.ncell_cap = ncap; w.pad = 0;
}

// The whole workspace: the DtWs table, then image after image.  recs == nullptr: sizing only.
static void dt_batch_layout(const gims_agc_image* images, int n_images, WsLayout& L, DtWs* recs) {
  L.take<DtWs>(n_images);
  DtWs scratch;
  for (int i = 0; i < n_images; ++i) dt_layout(images[i].n > 0 ? images[i].n : 0, L, recs ? recs[i] : scratch);
}

}  // namespace gims

extern "C" size_t gims_delaunay_workspace_bytes(const gims_agc_image* images, int32_t n_images) {
  using namespace gims;
  if (!images || n_images <= 0) return 0;
  WsLayout L(nullptr);
  dt_batch_layout(images, n_images, L, nullptr);
  return L.bytes();
}

extern "C" int gims_delaunay_build(const gims_agc_image* images, int32_t n_images, void* work, size_t work_bytes, void* stream) {
  using namespace gims;
  GIMS_CHECK_ARG(images && n_images > 0 && work, "gims_delaunay_build: null / empty arguments");
  for (int i = 0; i < n_images; ++i) {
    const gims_agc_image& im = images[i];
    GIMS_CHECK_ARG(im.kpts && im.kept && im.indptr && im.indices && im.info, "gims_delaunay_build: image %d has a null pointer", i);
    GIMS_CHECK_ARG(im.n >= 1 && im.n <= DT_MAX_N, "gims_delaunay_build: image %d: n=%d out of range [1, %d] (gims_agc_max_keypoints)", i, im.n,
                   DT_MAX_N);
    GIMS_CHECK_ARG(im.max_edges_dir >= 0, "gims_delaunay_build: image %d: max_edges_dir=%d < 0", i, im.max_edges_dir);
  }
  std::vector<DtWs> hws(n_images);
  WsLayout L(work);
  dt_batch_layout(images, n_images, L, hws.data());
  GIMS_CHECK_ARG(work_bytes >= L.bytes(), "gims_delaunay_build: workspace too small (%zu bytes; gims_delaunay_workspace_bytes asks for %zu)", work_bytes,
                 L.bytes());
  hipStream_t s = (hipStream_t)stream;
  DtWs* dws = (DtWs*)work;
  int maxn = 0;
  for (int i = 0; i < n_images; ++i) {
    const gims_agc_image& im = images[i];
    DtWs* w = &hws[i];
    w->kpts = im.kpts; w->kept = im.kept; w->indptr = im.indptr; w->indices = im.indices; w->info = im.info;
    w->max_edges_dir = im.max_edges_dir;
    maxn = im.n > maxn ? im.n : maxn;
  }
  const int B = n_images;
  const int rc = upload_table(hws.data(), sizeof(DtWs) * (size_t)B, dws, s);
  if (rc != GIMS_OK) return rc;
  const dim3 g1(1, B), gp(cdiv(maxn, 256), B), gf(cdiv(maxn, 64), B);
  hipLaunchKernelGGL(dt_grid_kernel, g1, dim3(1024), 0, s, dws);
  hipLaunchKernelGGL(dt_star_kernel<false>, gp, dim3(256), 0, s, dws);
  hipLaunchKernelGGL(dt_fallback_kernel<false>, gf, dim3(64), 0, s, dws);
  hipLaunchKernelGGL(dt_scan_kernel, g1, dim3(1024), 0, s, dws);
  hipLaunchKernelGGL(dt_star_kernel<true>, gp, dim3(256), 0, s, dws);
  hipLaunchKernelGGL(dt_fallback_kernel<true>, gf, dim3(64), 0, s, dws);
  hipLaunchKernelGGL(dt_check_kernel, gp, dim3(256), 0, s, dws);
  hipLaunchKernelGGL(dt_info_kernel, g1, dim3(64), 0, s, dws);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}
