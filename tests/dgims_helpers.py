"""Shared helpers of the D-GIMS (Delaunay graph) tests and of tools/gen_golden_delaunay.py: the input generators of the dgims_* fixtures
(built on gims_amd.synth, so the fixtures store seeds) and an exact Delaunay checker in Python integers (float32 coordinates are dyadic
rationals: one common power-of-two scale turns them into integers)."""
import numpy as np

from gims_amd import synth


# ---------------------------------------------------------------- inputs
def uniform_points(n, seed):
    """The keypoints0 of synth.make_pair(n, seed) (same streams, without the descriptors)."""
    w, h = synth.canvas_for(n)
    return np.stack([synth.uniform(seed, 1, n) * w, synth.uniform(seed, 2, n) * h], axis=1).astype(np.float32)


def cluster_points(n, seed, k=8, sigma=0.05):
    """Gaussian-clustered keypoints: k centres uniform on the canvas, spread sigma * canvas width."""
    w, h = synth.canvas_for(n)
    cent = np.stack([synth.uniform(seed, 21, k) * w, synth.uniform(seed, 22, k) * h], axis=1)
    lab = (synth.uniform(seed, 23, n) * k).astype(np.int64)
    xy = cent[lab] + sigma * w * synth.normal(seed, 24, 2 * n).reshape(n, 2)
    return xy.astype(np.float32)


def with_duplicates(xy, seed, frac=0.15):
    """SIFT-like: `frac` of the keypoints repeat the exact coordinates of another keypoint (one location, several orientations)."""
    xy = xy.copy()
    n = len(xy)
    m = int(n * frac)
    dst = synth.permutation(seed, 31, n)[:m]
    src = (synth.uniform(seed, 32, m) * n).astype(np.int64)
    xy[dst] = xy[src]
    return xy


def fixture_points(kind, n, seed):
    if kind == "uniform":
        return uniform_points(n, seed)
    if kind == "cluster":
        return cluster_points(n, seed)
    if kind == "sift":
        return with_duplicates(uniform_points(n, seed), seed)
    raise ValueError(kind)


def e2e_pair(meta):
    """The input pair of a dgims_e2e_* fixture from its meta = [seed, weight seed, iterations, duplicates, n0, n1]: synth.make_pair (or
    make_pair_unbalanced with 700 common keypoints when n0 != n1), with SIFT-like duplicates in both images when asked for."""
    seed, _, _, dup, n0, n1 = (int(v) for v in meta)
    pair = synth.make_pair(n0, seed) if n0 == n1 else synth.make_pair_unbalanced(n0, n1, 700, seed)
    if dup:
        for k, s in enumerate(("0", "1")):
            pair["keypoints" + s] = with_duplicates(pair["keypoints" + s][0], seed + 17 * k)[None].copy()
    return pair


def lowest_id_map(xy):
    """rep[i] = the lowest id with exactly the coordinates of i."""
    xy = np.asarray(xy, dtype=np.float32)
    order = np.lexsort((np.arange(len(xy)), xy[:, 1], xy[:, 0]))
    s = xy[order]
    new = np.ones(len(xy), dtype=bool)
    new[1:] = (s[1:] != s[:-1]).any(axis=1)
    first = order[np.maximum.accumulate(np.where(new, np.arange(len(xy)), 0))]
    rep = np.empty(len(xy), dtype=np.int64)
    rep[order] = first
    return rep


def canon_edges(e):
    """(E, 2) undirected edges -> unique (min, max) rows, sorted."""
    e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
    e = np.stack([e.min(axis=1), e.max(axis=1)], axis=1)
    e = e[e[:, 0] != e[:, 1]]
    return np.unique(e, axis=0)


def csr_edges(indptr, indices):
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    src = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return src, indices


# ---------------------------------------------------------------- exact arithmetic
def exact_ints(xy):
    """float32 coordinates -> Python ints (object array) at one common power-of-two scale (exact)."""
    a = np.asarray(xy, dtype=np.float32).astype(np.float64)
    m, e = np.frexp(a)
    M = (m * 2.0 ** 24).astype(np.int64)
    E = e.astype(np.int64) - 24
    nz = M != 0
    s = int(-E[nz].min()) if nz.any() else 0
    flat = [int(mi) << int(ei + s) if mi != 0 else 0 for mi, ei in zip(M.ravel().tolist(), E.ravel().tolist())]
    return np.array(flat, dtype=object).reshape(a.shape)


def orient_int(ax, ay, bx, by, cx, cy):
    return (ax - cx) * (by - cy) - (ay - cy) * (bx - cx)


def incircle_int(ax, ay, bx, by, cx, cy, dx, dy):
    adx, ady, bdx, bdy, cdx, cdy = ax - dx, ay - dy, bx - dx, by - dy, cx - dx, cy - dy
    return ((adx * adx + ady * ady) * (bdx * cdy - cdx * bdy) + (bdx * bdx + bdy * bdy) * (cdx * ady - adx * cdy)
            + (cdx * cdx + cdy * cdy) * (adx * bdy - bdx * ady))


def _sgn(v):
    return np.array([(x > 0) - (x < 0) for x in np.asarray(v, dtype=object).ravel()], dtype=np.int64)


def hull_boundary(P, ids):
    """Ids of the distinct points on the convex hull's boundary (collinear boundary points included), exact; and twice the hull's area."""
    pts = sorted((P[i, 0], P[i, 1], i) for i in ids)

    def chain(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and orient_int(out[-2][0], out[-2][1], out[-1][0], out[-1][1], p[0], p[1]) < 0:
                out.pop()
            out.append(p)
        return out
    lo, up = chain(pts), chain(pts[::-1])
    strict = []
    for seq in (pts, pts[::-1]):                        # strict hull for the area
        out = []
        for p in seq:
            while len(out) >= 2 and orient_int(out[-2][0], out[-2][1], out[-1][0], out[-1][1], p[0], p[1]) <= 0:
                out.pop()
            out.append(p)
        strict += out[:-1]
    area2 = sum(strict[i][0] * strict[(i + 1) % len(strict)][1] - strict[(i + 1) % len(strict)][0] * strict[i][1] for i in range(len(strict)))
    return {p[2] for p in lo} | {p[2] for p in up}, area2


def check_delaunay(xy, edges):
    """Exact check that `edges` (undirected, original ids) is a Delaunay triangulation of the float32 points `xy` under the D-GIMS contract:
    only the lowest id of a group of identical coordinates is a vertex; the faces (from the angular order around every vertex) are
    counter-clockwise, cover the convex hull exactly (areas), number 2 n' - 2 - h with 3 n' - 3 - h edges (h: points on the hull's boundary),
    and every interior edge is locally Delaunay (the opposite vertex not strictly inside the circle of a face): hence globally Delaunay.
    Returns dict(n_distinct, hull, n_edges, n_faces)."""
    xy = np.asarray(xy, dtype=np.float32)
    n = len(xy)
    e = canon_edges(edges)
    rep = lowest_id_map(xy)
    verts = np.nonzero(rep == np.arange(n))[0]
    assert (rep[e] == e).all(), "an edge touches a non-lowest duplicate"
    P = exact_ints(xy)
    hull, hull_area2 = hull_boundary(P, verts.tolist())
    nd, h = len(verts), len(hull)
    assert len(e) == 3 * nd - 3 - h, f"{len(e)} edges, a triangulation of {nd} points with {h} on the hull has {3 * nd - 3 - h}"
    # faces from the angular order of the neighbours of every vertex
    src = np.concatenate([e[:, 0], e[:, 1]])
    dst = np.concatenate([e[:, 1], e[:, 0]])
    xd = xy.astype(np.float64)
    ang = np.arctan2(xd[dst, 1] - xd[src, 1], xd[dst, 0] - xd[src, 0])
    o = np.lexsort((ang, src))
    src, dst = src[o], dst[o]
    start = np.searchsorted(src, src, side="left")
    end = np.searchsorted(src, src, side="right")
    nxt_i = np.arange(len(src)) + 1
    nxt_i = np.where(nxt_i == end, start, nxt_i)
    a, b, c = src, dst, dst[nxt_i]
    key = set((e[:, 0] * n + e[:, 1]).tolist())
    lo_, hi_ = np.minimum(b, c), np.maximum(b, c)
    adj = np.array([k in key for k in (lo_ * n + hi_).tolist()], dtype=bool) & (b != c)
    a, b, c = a[adj], b[adj], c[adj]
    ori = _sgn(orient_int(P[a, 0], P[a, 1], P[b, 0], P[b, 1], P[c, 0], P[c, 1]))
    a, b, c = a[ori > 0], b[ori > 0], c[ori > 0]
    tri = np.stack([a, b, c], axis=1)
    r = np.argmin(tri, axis=1)                          # canonical rotation: lowest id first
    tri = np.stack([tri[np.arange(len(tri)), r], tri[np.arange(len(tri)), (r + 1) % 3], tri[np.arange(len(tri)), (r + 2) % 3]], axis=1)
    faces, cnt = np.unique(tri, axis=0, return_counts=True)
    assert (cnt == 3).all(), "a face is not seen from all three of its corners"
    assert len(faces) == 2 * nd - 2 - h, f"{len(faces)} faces, expected {2 * nd - 2 - h}"
    fa, fb, fc = faces[:, 0], faces[:, 1], faces[:, 2]
    area2 = sum(orient_int(P[fa, 0], P[fa, 1], P[fb, 0], P[fb, 1], P[fc, 0], P[fc, 1]).tolist())
    assert area2 == hull_area2, "the faces do not tile the convex hull"
    # local Delaunay: every directed face edge (u, v) with the opposite face's apex
    de_u = np.concatenate([fa, fb, fc])
    de_v = np.concatenate([fb, fc, fa])
    de_w = np.concatenate([fc, fa, fb])
    opp = dict(zip((de_u * n + de_v).tolist(), de_w.tolist()))
    x = np.array([opp.get(k, -1) for k in (de_v * n + de_u).tolist()], dtype=np.int64)
    m = x >= 0
    assert (len(m) - m.sum()) == h, "hull edges do not number h"
    u, v, w, x = de_u[m], de_v[m], de_w[m], x[m]
    ic = _sgn(incircle_int(P[u, 0], P[u, 1], P[v, 0], P[v, 1], P[w, 0], P[w, 1], P[x, 0], P[x, 1]))
    assert (ic <= 0).all(), f"{int((ic > 0).sum())} edges are not locally Delaunay"
    return dict(n_distinct=nd, hull=h, n_edges=len(e), n_faces=len(faces))


def edges_of_graph(g):
    """Undirected (min, max) edges of a GraphHandle / DGL-like graph."""
    src, dst = g.edges()
    return canon_edges(np.stack([np.asarray(src.cpu()), np.asarray(dst.cpu())], axis=1))
