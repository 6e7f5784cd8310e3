"""NumPy restatement of the calibrated relative-pose model of gims_verify_pairs (model 3; specification: include/gims_hip.h) -- TEST
INFRASTRUCTURE.

Stage 1 (the five-point hypotheses) is written batched over the hypotheses of a set, one array operation per step of the specification:
the sampler, the 5 x 9 Gauss-Jordan elimination with complete pivoting, the ten cubic constraints as a 10 x 20 matrix built from products
of the linear forms, its row-pivoted Gauss-Jordan elimination with the hidden variable pivoted, the 3 x 3 matrix of polynomials in z, its degree-10 determinant and the
real roots of that by bisection between the roots of successive derivatives.  No call into ``np.linalg`` or ``np.roots``.  Stages 2 and 3
(guarded local optimisation, projection onto the essential manifold, the four decompositions and the cheirality vote) run per set on the
helpers of tests/fundamental_ref.py.

Besides the expected outputs, ``verify`` returns what a GPU test needs to be allowed to compare index sets exactly: the smallest margin
of every inlier decision (in px^2: normalised margin * f_mean^2), the gap between the two best hypothesis scores, the gap between the
two best pose votes, the smallest depth numerator of a vote, and `stab`: over every hypothesis within 2 of the best score, how far its
polynomial is from gaining or losing a real root (see ``real_roots``) -- 0 when a model of such a hypothesis moves by more than SPREAD
(a quarter of the GPU test's tolerance) under a perturbation of the sample's coordinates by 64 units in the last place, which is how
the restatement measures what a different order of the same sums, or fused multiply-adds, may do to a badly conditioned sample.

Scenes: random 3-D points in front of two calibrated pinhole cameras (800 x 600, focal lengths around 600): a general motion, a forward
motion whose epipole lies inside the image, a sideways translation with R = I, a plane-dominated scene (7 of 8 points on one plane) and
a purely planar one."""
import functools
import math

import numpy as np

from tests import fundamental_ref as RF

F32 = np.float32
HB = 16
KS = (0, 4, 5, 6, 63, 64, 65, 255, 257, 1025)
ITERS = (1, HB - 1, HB, HB + 1, 500)
LO_ITERS = (0, 8)
CONFIGS = ("general", "forward", "sideways", "plane7of8")
CANVAS = (800, 600)
THRESH = 1.0
MARGIN = 1e-6                                      # px^2: smallest allowed |r^2 - thresh^2| f_mean^2 of any inlier decision compared exactly
STAB = 1e-9                                        # smallest allowed relative |p(c)| at a critical point c (real_roots)
DEPTH = 1e-6                                       # smallest allowed |depth numerator| / D of a vote
WIGGLE = 2.0 ** -46                                # relative perturbation of a sample's coordinates (64 units in the last place) ...
SPREAD = 2.0 ** -24                                # ... under which no model of a hypothesis near the best may move by more than this
BISECTIONS = 80
SWEEPS = RF.SWEEPS
_M64 = 0xFFFFFFFFFFFFFFFF

# column of the monomial x^a y^b z^c in the 10 x 20 matrix: BASE[a][b] + (3 - a - b - c)
#   x^3 y^3 x^2y xy^2 | x^2z x^2 | y^2z y^2 | xyz xy | xz^2 xz x | yz^2 yz y | z^3 z^2 z 1
BASE = ((16, 13, 6, 1), (10, 8, 3, -1), (4, 2, -1, -1), (0, -1, -1, -1))


def _col(i, j, k):
    """Column of the product of the variables i, j, k (0: x, 1: y, 2: z, 3: the constant 1)."""
    a, b, c = [sum(1 for v in (i, j, k) if v == w) for w in (0, 1, 2)]
    return BASE[a][b] + (3 - a - b - c)


_P = np.zeros((64, 20))
for _i in range(4):
    for _j in range(4):
        for _k in range(4):
            _P[16 * _i + 4 * _j + _k, _col(_i, _j, _k)] = 1.0


# ------------------------------------------------------------------------------------------------ the sampler and the coordinates
def sample5(seed, hyp, k):
    """Five DISTINCT indices in [0, k): the stream of oracle.eval_oracle.ransac_sample for (seed, hyp), continued."""
    out, state = [], (seed ^ (hyp * 0xD1342543DE82EF95)) & _M64
    while len(out) < 5:
        state = RF._splitmix(state)
        idx = state % k
        if idx not in out:
            out.append(idx)
    return np.asarray(out)


def intr8(K0, K1):
    """fx0, fy0, cx0, cy0, fx1, fy1, cx1, cy1 as the library stores them: float32."""
    K0, K1 = np.asarray(K0, dtype=np.float64), np.asarray(K1, dtype=np.float64)
    return np.array([K0[0, 0], K0[1, 1], K0[0, 2], K0[1, 2], K1[0, 0], K1[1, 1], K1[0, 2], K1[1, 2]], dtype=F32)


def normalise(p0, p1, intr):
    """Camera coordinates of float32 pixel coordinates: (x - cx) / fx, (y - cy) / fy in float64."""
    i = intr.astype(np.float64)
    p0, p1 = p0.astype(np.float64), p1.astype(np.float64)
    q0 = np.stack([(p0[:, 0] - i[2]) / i[0], (p0[:, 1] - i[3]) / i[1]], 1)
    q1 = np.stack([(p1[:, 0] - i[6]) / i[4], (p1[:, 1] - i[7]) / i[5]], 1)
    return q0, q1


def f_mean(intr):
    return (float(intr[0]) + float(intr[5])) / 2.0


# ------------------------------------------------------------------------------------------------ stage 1, batched over hypotheses
def null5x9(A):
    """[H, 5, 9] -> (basis [H, 4, 9], ok [H]): Gauss-Jordan with complete pivoting, five pivots; basis vector j has free column j
    (ascending) at 1 and the other free columns at 0."""
    A = A.copy()
    H = len(A)
    ar = np.arange(H)
    rfree, cfree, ok = np.ones((H, 5), bool), np.ones((H, 9), bool), np.ones(H, bool)
    piv = []
    with np.errstate(all="ignore"):
        for _ in range(5):
            mag = np.where(rfree[:, :, None] & cfree[:, None, :], np.abs(A), -1.0)
            mag = np.where(np.isnan(mag), -1.0, mag)
            flat = np.argmax(mag.reshape(H, 45), 1)                  # the first largest entry: lowest row, then lowest column
            pr, pc = flat // 9, flat % 9
            best = mag[ar, pr, pc]
            ok &= (best > 0.0) & np.isfinite(best)
            rfree[ar, pr], cfree[ar, pc] = False, False
            piv.append((pr, pc))
            m = A[ar, :, pc] / A[ar, pr, pc][:, None]
            m[ar, pr] = 0.0
            A = A - m[:, :, None] * A[ar, pr][:, None, :]
        fc = np.argsort(~cfree, axis=1, kind="stable")[:, :4]
        B = np.zeros((H, 4, 9))
        for j in range(4):
            B[ar, j, fc[:, j]] = 1.0
            for pr, pc in piv:
                B[ar, j, pc] = -A[ar, pr, fc[:, j]] / A[ar, pr, pc]
    return B, ok & np.isfinite(B).all((1, 2))


def constraints(B):
    """[H, 4, 9] basis (X, Y, Z, W) -> the [H, 10, 20] coefficients of det E and of the nine entries of 2 E E^T E - tr(E E^T) E."""
    H = len(B)
    L = B.transpose(0, 2, 1).reshape(H, 3, 3, 4)                      # L[h, i, j]: the linear form E_ij in (x, y, z, 1)
    ll = lambda a, b: np.einsum("hi,hj->hij", a, b)
    ql = lambda q, l: np.einsum("hij,hk->hijk", q, l)
    rows = [ql(ll(L[:, 1, 1], L[:, 2, 2]) - ll(L[:, 1, 2], L[:, 2, 1]), L[:, 0, 0])
            - ql(ll(L[:, 1, 0], L[:, 2, 2]) - ll(L[:, 1, 2], L[:, 2, 0]), L[:, 0, 1])
            + ql(ll(L[:, 1, 0], L[:, 2, 1]) - ll(L[:, 1, 1], L[:, 2, 0]), L[:, 0, 2])]
    G = [[sum(ll(L[:, i, k], L[:, j, k]) for k in range(3)) for j in range(3)] for i in range(3)]
    T = G[0][0] + G[1][1] + G[2][2]
    for i in range(3):
        for j in range(3):
            rows.append(2.0 * sum(ql(G[i][k], L[:, k, j]) for k in range(3)) - ql(T, L[:, i, j]))
    return np.stack(rows, 1).reshape(H, 10, 64) @ _P


def eliminate10(M):
    """Gauss-Jordan over the columns 0 .. 9 of [H, 10, 20], pivot = the largest entry of the column among the rows without a pivot (the
    first such); returns the rows of the pivots of the columns 4 .. 9 divided by their pivots [H, 6, 20], ok [H] and the smallest pivot
    magnitude [H] (-1 where the elimination fails)."""
    M = M.copy()
    H = len(M)
    ar = np.arange(H)
    rfree, ok, quality = np.ones((H, 10), bool), np.ones(H, bool), np.full(H, np.inf)
    prow = []
    with np.errstate(all="ignore"):
        for c in range(10):
            mag = np.where(rfree, np.abs(M[:, :, c]), -1.0)
            mag = np.where(np.isnan(mag), -1.0, mag)
            pr = np.argmax(mag, 1)
            best = mag[ar, pr]
            ok &= (best > 0.0) & np.isfinite(best)
            quality = np.minimum(quality, best)
            rfree[ar, pr] = False
            prow.append(pr)
            m = M[:, :, c] / M[ar, pr, c][:, None]
            m[ar, pr] = 0.0
            M = M - m[:, :, None] * M[ar, pr][:, None, :]
        out = np.stack([M[ar, prow[c]] / M[ar, prow[c], c][:, None] for c in range(4, 10)], 1)
    return out, ok, np.where(ok, quality, -1.0)


ORDERS = ((0, 1, 2, 3), (0, 2, 1, 3), (2, 1, 0, 3))                # (X, Y, Z, W) among the basis vectors: the hidden variable is pivoted


def pivoted_elimination(B):
    """Of the three ORDERS of the basis the one whose elimination has the largest smallest pivot (the first such): the basis in that
    order [H, 4, 9], its six rows [H, 6, 20], ok [H]."""
    cands = [(B[:, list(o)],) + eliminate10(constraints(B[:, list(o)])) for o in ORDERS]
    pick = np.argmax(np.stack([c[3] for c in cands], 1), 1)
    ar = np.arange(len(B))
    return (np.stack([c[0] for c in cands], 1)[ar, pick], np.stack([c[1] for c in cands], 1)[ar, pick],
            np.stack([c[2] for c in cands], 1)[ar, pick])


def zmatrix(R6):
    """The rows <x^2 z> - z <x^2>, <y^2 z> - z <y^2>, <x y z> - z <x y> as polynomials in z multiplying x, y and 1: [H, 3, 3, 5],
    ascending powers (the x and y columns have degree 3)."""
    H = len(R6)
    Bz = np.zeros((H, 3, 3, 5))
    for r in range(3):
        a, b = R6[:, 2 * r], R6[:, 2 * r + 1]
        for v, o in ((0, 10), (1, 13)):
            Bz[:, r, v, 0] = a[:, o + 2]
            Bz[:, r, v, 1] = a[:, o + 1] - b[:, o + 2]
            Bz[:, r, v, 2] = a[:, o] - b[:, o + 1]
            Bz[:, r, v, 3] = -b[:, o]
        Bz[:, r, 2, 0] = a[:, 19]
        Bz[:, r, 2, 1] = a[:, 18] - b[:, 19]
        Bz[:, r, 2, 2] = a[:, 17] - b[:, 18]
        Bz[:, r, 2, 3] = a[:, 16] - b[:, 17]
        Bz[:, r, 2, 4] = -b[:, 16]
    return Bz


def _pmul(a, b):
    out = np.zeros((len(a), a.shape[1] + b.shape[1] - 1))
    for i in range(a.shape[1]):
        out[:, i:i + b.shape[1]] += a[:, i:i + 1] * b
    return out


def zdet(Bz):
    """det of the 3 x 3 matrix of polynomials, expanded along its first row: [H, 11]."""
    x, y, w = lambda r: Bz[:, r, 0, :4], lambda r: Bz[:, r, 1, :4], lambda r: Bz[:, r, 2]
    return (_pmul(x(0), _pmul(y(1), w(2)) - _pmul(w(1), y(2))) - _pmul(y(0), _pmul(x(1), w(2)) - _pmul(w(1), x(2)))
            + _pmul(w(0), _pmul(x(1), y(2)) - _pmul(y(1), x(2))))


def _horner(c, z):
    """c [H, n] ascending, z [H, m] -> [H, m]."""
    v = np.zeros_like(z) + c[:, -1:]
    for i in range(c.shape[1] - 2, -1, -1):
        v = v * z + c[:, i:i + 1]
    return v


def real_roots(c):
    """c [H, 11] -> (roots [H, 10] ascending and padded with the bound, count [H], ok [H], stab [H]).

    bound = 1 + max |c_i / c_10|.  For d = 1 .. 10, q = the (10 - d)-th derivative of p; its real roots inside (-bound, bound) are sought
    in the intervals between -bound, the roots of the derivative before it and bound: an interval [a, b] holds a root iff (q(a) > 0) !=
    (q(b) > 0), found by BISECTIONS halvings (m = (a + b) / 2 replaces the end whose sign it shares), the root is the last midpoint.
    stab = the smallest |p(e)| / sum |c_i| |e|^i over the interval ends e of the last level: small when p is about to gain or lose roots."""
    H = len(c)
    with np.errstate(all="ignore"):
        ok = (c[:, 10] != 0.0) & np.isfinite(c).all(1)
        bound = 1.0 + np.max(np.abs(c[:, :10] / c[:, 10:11]), 1)
        ok &= np.isfinite(bound)
        bound = np.where(ok, bound, 1.0)
        c = np.where(ok[:, None], c, 1.0)
        roots, stab = np.repeat(bound[:, None], 0, 1), None
        for d in range(1, 11):
            k = 10 - d
            q = np.stack([c[:, i + k] * (math.factorial(i + k) // math.factorial(i)) for i in range(d + 1)], 1)
            ends = np.concatenate([-bound[:, None], roots, bound[:, None]], 1)         # [H, d + 1]
            fe = _horner(q, ends)
            if d == 10:
                stab = np.min(np.abs(fe) / _horner(np.abs(q), np.abs(ends)), 1)
            a, b = ends[:, :-1].copy(), ends[:, 1:].copy()
            sa, has = fe[:, :-1] > 0.0, (fe[:, :-1] > 0.0) != (fe[:, 1:] > 0.0)
            for _ in range(BISECTIONS):
                m = 0.5 * (a + b)
                same = (_horner(q, m) > 0.0) == sa
                a, b = np.where(same, m, a), np.where(same, b, m)
            r = np.where(has, 0.5 * (a + b), bound[:, None])
            order = np.argsort(~has, axis=1, kind="stable")
            roots = np.take_along_axis(r, order, 1)
        count = has.sum(1)
    return roots, np.where(ok, count, 0), ok, stab


def models_at(Bz, B, roots, count):
    """E of every root: (x, y, 1) is the cross product of two rows of the matrix at z -- of the three pairs (0,1), (0,2), (1,2) the one
    whose third component is largest in magnitude (the first such) --; E = unit(x X + y Y + z Z + W).  [H, 10, 9], valid [H, 10]."""
    H = len(B)
    E, valid = np.zeros((H, 10, 9)), np.zeros((H, 10), bool)
    with np.errstate(all="ignore"):
        for r in range(10):
            z = roots[:, r]
            M = np.stack([np.stack([_horner(Bz[:, i, j], z[:, None])[:, 0] for j in range(3)], 1) for i in range(3)], 1)
            n = np.stack([np.cross(M[:, 0], M[:, 1]), np.cross(M[:, 0], M[:, 2]), np.cross(M[:, 1], M[:, 2])], 1)
            mag = np.where(np.isnan(n[:, :, 2]), -1.0, np.abs(n[:, :, 2]))
            pick = np.argmax(mag, 1)
            nn = n[np.arange(H), pick]
            x, y = nn[:, 0] / nn[:, 2], nn[:, 1] / nn[:, 2]
            e = x[:, None] * B[:, 0] + y[:, None] * B[:, 1] + z[:, None] * B[:, 2] + B[:, 3]
            n2 = np.zeros(H)
            for q in range(9):
                n2 = n2 + e[:, q] * e[:, q]
            nrm = np.sqrt(n2)
            e = e / nrm[:, None]
            E[:, r] = e
            valid[:, r] = (r < count) & (nn[:, 2] != 0.0) & (nrm > 0.0) & np.isfinite(nrm) & np.isfinite(e).all(1)
    return np.where(valid[:, :, None], E, 0.0), valid


def five_point(q0, q1):
    """q0, q1 [H, 5, 2] camera coordinates -> (E [H, 10, 9] in ascending root order with the models without a finite E removed,
    n_models [H], stab [H])."""
    x, y, u, v = q0[:, :, 0], q0[:, :, 1], q1[:, :, 0], q1[:, :, 1]
    A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], 2)
    B, ok = null5x9(A)
    B = np.where(ok[:, None, None], B, 0.0)
    with np.errstate(all="ignore"):
        B, R6, ok2 = pivoted_elimination(B)
        ok &= ok2 & np.isfinite(R6).all((1, 2))
        R6 = np.where(ok[:, None, None], R6, 0.0)
        Bz = zmatrix(R6)
        roots, count, ok3, stab = real_roots(zdet(Bz))
    ok &= ok3
    count = np.where(ok, count, 0)
    E, valid = models_at(Bz, B, roots, count)
    order = np.argsort(~valid, axis=1, kind="stable")
    E = np.take_along_axis(E, order[:, :, None], 1)
    return E, valid.sum(1), np.where(ok, stab, np.inf)


def stage1_scores(p0, p1, intr, seed, iters, thresh=THRESH):
    """Per hypothesis: score (-1: no model), the index of its best model, that model [9], the smallest decision margin over all its
    models (normalised units), stab."""
    k = len(p0)
    t2 = (float(thresh) / f_mean(intr)) ** 2
    scores, which = np.full(iters, -1, dtype=np.int64), np.zeros(iters, dtype=np.int64)
    models, margins, stab = np.zeros((iters, 9)), np.full(iters, np.inf), np.full(iters, np.inf)
    if k < 5:
        return scores, which, models, margins, stab
    q0, q1 = normalise(p0, p1, intr)
    idx = np.stack([sample5(seed, h, k) for h in range(iters)])
    E, nm, stab = five_point(q0[idx], q1[idx])
    # the same samples with their coordinates moved by up to 64 units in the last place: how far the models move
    r = np.random.default_rng(12345)
    E2, nm2, _ = five_point(q0[idx] * (1.0 + WIGGLE * (2.0 * r.random(q0[idx].shape) - 1.0)), q1[idx] * (1.0 + WIGGLE * (2.0 * r.random(q0[idx].shape) - 1.0)))
    moved = np.where(nm == nm2, np.abs(E - E2).max((1, 2)), np.inf)
    stab = np.where(moved <= SPREAD, stab, 0.0)                    # reported through `stab`: 0 fails every fixture that needs the hypothesis
    for h in range(iters):
        for r in range(int(nm[h])):
            mask, mg = RF.decisions(E[h, r].reshape(3, 3), q0, q1, t2)
            margins[h] = min(margins[h], mg)
            if int(mask.sum()) > scores[h]:
                scores[h], which[h], models[h] = int(mask.sum()), r, E[h, r]
    return scores, which, models, margins, stab


# ------------------------------------------------------------------------------------------------ stages 2 and 3
def jacobi_full(S):
    """RF.jacobi with all of its result: (diagonal, V)."""
    S = np.array(S, dtype=np.float64)
    n = len(S)
    V = np.eye(n)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = S[p, q]
                    if apq == 0.0:
                        continue
                    d, b = S[q, q] - S[p, p], 2.0 * apq
                    t = (b if d >= 0.0 else -b) / (abs(d) + math.hypot(d, b))
                    c = 1.0 / math.sqrt(t * t + 1.0)
                    s = t * c
                    kp, kq = S[:, p].copy(), S[:, q].copy()
                    S[:, p], S[:, q] = c * kp - s * kq, s * kp + c * kq
                    pk, qk = S[p].copy(), S[q].copy()
                    S[p], S[q] = c * pk - s * qk, s * pk + c * qk
                    S[p, q] = S[q, p] = 0.0
                    vp, vq = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
    return np.diag(S).copy(), V


def svd_parts(E):
    """v1, v2, v3 (v3 at the smallest eigenvalue of E^T E, the first such; v1, v2 the other columns in ascending index), w1 = E v1,
    w2 = E v2 and their lengths."""
    G = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            G[i, j] = E[0, i] * E[0, j] + E[1, i] * E[1, j] + E[2, i] * E[2, j]
    d, V = jacobi_full(G)
    m = 0
    for k in range(1, 3):
        if d[k] < d[m]:
            m = k
    a, b = [k for k in range(3) if k != m]
    v1, v2, v3 = V[:, a], V[:, b], V[:, m]
    w1 = E[:, 0] * v1[0] + E[:, 1] * v1[1] + E[:, 2] * v1[2]
    w2 = E[:, 0] * v2[0] + E[:, 1] * v2[1] + E[:, 2] * v2[2]
    return v1, v2, v3, w1, w2, math.sqrt(w1[0] * w1[0] + w1[1] * w1[1] + w1[2] * w1[2]), math.sqrt(w2[0] * w2[0] + w2[1] * w2[1] + w2[2] * w2[2])


def ess(E):
    """Projection onto the essential manifold: singular values (1, 1, 0), then unit(); E itself when that fails."""
    v1, v2, _, w1, w2, s1, s2 = svd_parts(E)
    with np.errstate(all="ignore"):
        out = RF.unit(np.outer(w1, v1) / s1 + np.outer(w2, v2) / s2) if s1 > 0.0 and s2 > 0.0 else None
    return E if out is None else out


def lo_round(E_prev, q0, q1, t2, reverse=False):
    mask, _ = RF.decisions(E_prev, q0, q1, t2)
    if mask.sum() < 8:
        return None
    c0, s0 = RF.similarity(q0[mask], reverse)
    c1, s1 = RF.similarity(q1[mask], reverse)
    a = RF._rows((q0[mask] - c0) * s0, (q1[mask] - c1) * s1)
    S = np.empty((9, 9))
    for i in range(9):
        for j in range(i, 9):
            S[i, j] = S[j, i] = RF._ssum(a[:, i] * a[:, j], reverse)
    with np.errstate(all="ignore"):
        Ed = RF.unit(RF.denormalise(RF.jacobi(S), c0, s0, c1, s1))
    return None if Ed is None else ess(Ed)


def decompose(E):
    """The four (R, t) in the specification's order, det R = +1, |t| = 1; None when E has no two non-zero singular values."""
    v1, v2, v3, w1, w2, s1, s2 = svd_parts(E)
    if not (s1 > 0.0 and s2 > 0.0):
        return None
    u1, u2 = w1 / s1, w2 / s2
    u3 = np.array([u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]])
    n3 = math.sqrt(u3[0] * u3[0] + u3[1] * u3[1] + u3[2] * u3[2])
    if not n3 > 0.0:
        return None
    u3 = u3 / n3
    c = np.array([v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]])
    if c[0] * v3[0] + c[1] * v3[1] + c[2] * v3[2] < 0.0:
        v3 = -v3
    # U W V^T and U W^T V^T for W = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    Ra = np.outer(u2, v1) - np.outer(u1, v2) + np.outer(u3, v3)
    Rb = np.outer(u1, v2) - np.outer(u2, v1) + np.outer(u3, v3)
    return [(Ra, u3), (Ra, -u3), (Rb, u3), (Rb, -u3)]


def depth_numerators(Rm, t, q0, q1):
    """Least-squares depths of l1 x1 = l0 R x0 + t: (numerator of l0, numerator of l1, D); the depths are the numerators / D."""
    x0 = np.concatenate([q0, np.ones((len(q0), 1))], 1)
    x1 = np.concatenate([q1, np.ones((len(q1), 1))], 1)
    a = x0[:, 0:1] * Rm[:, 0][None] + x0[:, 1:2] * Rm[:, 1][None] + x0[:, 2:3] * Rm[:, 2][None]
    dot = lambda p, q: p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1] + p[:, 2] * q[:, 2]
    tt = np.broadcast_to(t, a.shape)
    aa, bb, ab, at, bt = dot(a, a), dot(x1, x1), dot(x1, a), dot(a, tt), dot(x1, tt)
    return ab * bt - bb * at, bt * aa - ab * at, bb * aa - ab * ab


def votes(E, q0, q1, mask):
    """(votes [4], smallest |numerator| / D over the inliers and the two rotations)."""
    dec = decompose(E)
    if dec is None:
        return None, None, np.inf
    out, small = np.zeros(4, dtype=np.int64), np.inf
    for r in (0, 2):
        n0, n1, D = depth_numerators(dec[r][0], dec[r][1], q0[mask], q1[mask])
        out[r] = int(((D > 0.0) & (n0 > 0.0) & (n1 > 0.0)).sum())
        out[r + 1] = int(((D > 0.0) & (n0 < 0.0) & (n1 < 0.0)).sum())
        with np.errstate(all="ignore"):
            s = np.minimum(np.abs(n0), np.abs(n1)) / D
        s = s[np.isfinite(s)]
        small = min(small, float(s.min()) if len(s) else np.inf)
    return dec, out, small


def verify(p0, p1, intr, seed, iters, thresh=THRESH, lo_iters=8, stage1=None, reverse=False):
    """The specification on K correspondences p0[i] <-> p1[i] (float32 [K, 2]) and float32 intrinsics intr [8]."""
    k = len(p0)
    none = dict(ok=0, E=None, R=None, t=None, n_front=0, root=0, mask=np.zeros(k, bool), n_inliers=0, best_hyp=0, best_hyp_inliers=0,
                lo_rounds=0, n_valid=k, margin=np.inf, gap=np.inf, stab=np.inf, vote_gap=np.inf, depth=np.inf, votes=None)
    if k < 5 or iters == 0:
        return none
    fm = f_mean(intr)
    t2 = (float(thresh) / fm) ** 2
    scores, which, models, margins, stab = stage1 if stage1 is not None else stage1_scores(p0, p1, intr, seed, iters, thresh)
    scores, which, models, margins, stab = scores[:iters], which[:iters], models[:iters], margins[:iters], stab[:iters]
    if scores.max() < 0:
        return none
    best = int(np.argmax(scores))
    q0, q1 = normalise(p0, p1, intr)
    E = models[best].reshape(3, 3)
    mask, _ = RF.decisions(E, q0, q1, t2)
    margin, rounds = float(margins.min()), 0
    others = np.delete(scores, best)
    gap = int(scores[best] - others.max()) if len(others) else np.inf
    near = scores >= scores[best] - 2
    if lo_iters > 0:
        for _ in range(lo_iters):
            Ec = lo_round(E, q0, q1, t2, reverse)
            if Ec is None:
                break
            new, mg = RF.decisions(Ec, q0, q1, t2)
            margin = min(margin, mg)
            if new.sum() < mask.sum():
                break
            same = bool((new == mask).all())
            E, mask, rounds = Ec, new, rounds + 1
            if same:
                break
    if rounds == 0:
        E = ess(E)
        mask, mg = RF.decisions(E, q0, q1, t2)
        margin = min(margin, mg)
    E = RF.canonical(E)
    dec, vt, depth = votes(E, q0, q1, mask)
    if dec is None:
        Rm, t, nf, vote_gap = np.zeros((3, 3)), np.zeros(3), 0, np.inf
    else:
        w = int(np.argmax(vt))
        Rm, t, nf = dec[w][0], dec[w][1], int(vt[w])
        vote_gap = int(vt[w] - np.delete(vt, w).max())
    return dict(ok=1, E=E, R=Rm, t=t, n_front=nf, root=int(which[best]), mask=mask, n_inliers=int(mask.sum()), best_hyp=best,
                best_hyp_inliers=int(scores[best]), lo_rounds=rounds, n_valid=k, margin=margin * fm * fm, gap=gap, stab=float(stab[near].min()),
                vote_gap=vote_gap, depth=depth, votes=vt)


# ------------------------------------------------------------------------------------------------ scenes
def _rot(rx, ry, rz):
    Rx = np.array([[1, 0, 0], [0, math.cos(rx), -math.sin(rx)], [0, math.sin(rx), math.cos(rx)]])
    Ry = np.array([[math.cos(ry), 0, math.sin(ry)], [0, 1, 0], [-math.sin(ry), 0, math.cos(ry)]])
    Rz = np.array([[math.cos(rz), -math.sin(rz), 0], [math.sin(rz), math.cos(rz), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def cameras(config):
    """(K0, K1, R, t): x1 ~ K1 (R X + t) for a point X in the frame of camera 0."""
    w, h = CANVAS
    K0 = np.array([[600.0, 0, w / 2.0 - 7.0], [0, 610.0, h / 2.0 + 4.0], [0, 0, 1.0]])
    K1 = np.array([[590.0, 0, w / 2.0 + 5.0], [0, 605.0, h / 2.0 - 3.0], [0, 0, 1.0]])
    if config == "forward":
        return K0, K1, _rot(0.02, 0.03, -0.02), np.array([0.05, -0.03, 1.0])
    if config == "sideways":
        return K0, K1, np.eye(3), np.array([-0.8, 0.0, 0.0])
    if config in ("planar", "plane7of8"):
        return K0, K1, _rot(0.05, math.radians(12.0), -0.03), np.array([0.7, 0.2, 0.35])
    return K0, K1, _rot(0.04, -0.09, 0.03), np.array([0.7, 0.15, 0.3])


def T_0to1(config):
    _, _, Rm, t = cameras(config)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, t
    return T


def planted_E(config):
    _, _, Rm, t = cameras(config)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ Rm
    return E / np.linalg.norm(E)


def project_pair(config, n, rng):
    """n scene points seen by both cameras: exact projections [n, 2], [n, 2] in float64, and on_plane [n].  Depth 4 .. 12; for 'planar'
    every point lies on the plane z = 8 + 0.3 x - 0.2 y, for 'plane7of8' seven of every eight do."""
    K0, K1, Rm, t = cameras(config)
    w, h = CANVAS
    pix = rng.random((n, 2)) * [w, h]
    d = np.stack([(pix[:, 0] - K0[0, 2]) / K0[0, 0], (pix[:, 1] - K0[1, 2]) / K0[1, 1], np.ones(n)], 1)
    z = 4.0 + 8.0 * rng.random(n)
    on = np.zeros(n, bool)
    if config in ("planar", "plane7of8"):
        on = np.ones(n, bool) if config == "planar" else (np.arange(n) % 8 != 7)
        zp = 8.0 / (1.0 - 0.3 * d[:, 0] + 0.2 * d[:, 1])
        z = np.where(on, zp, z)
    Y = (d * z[:, None]) @ Rm.T + t
    q = Y @ K1.T
    return pix, q[:, :2] / q[:, 2:3], on


@functools.lru_cache(maxsize=None)
def planted_spec(K, config, outlier_frac=0.3, noise=0.5):
    """(kp0 [n0, 2], kp1 [n1, 2], matches0 [n0], intr [8]): as tests/fundamental_ref.planted_spec (no outliers with K <= 6)."""
    r = np.random.default_rng(9100 + K + 100000 * CONFIGS.index(config) + 1000000 * SCENES.get((K, config), 0))
    w, h = CANVAS
    n0 = K + K // 4 + 3
    n1 = n0 + 3
    a, b, _ = project_pair(config, n0, r)
    b = b + noise * r.standard_normal((n0, 2))
    rows = np.sort(r.permutation(n0)[:K])
    wrong = rows[r.random(K) < outlier_frac] if K > 6 else rows[:0]
    b[wrong] = r.random((len(wrong), 2)) * [w, h]
    perm = r.permutation(n1)
    kp1 = np.zeros((n1, 2), dtype=F32)
    kp1[perm[:n0]] = b.astype(F32)
    kp1[perm[n0:]] = (r.random((n1 - n0, 2)) * [w, h]).astype(F32)
    m0 = np.full(n0, -1, dtype=np.int64)
    m0[rows] = perm[rows]
    K0, K1, _, _ = cameras(config)
    return a.astype(F32), kp1, m0, intr8(K0, K1)


def clean_pairs(config, n=64, seed=1):
    """Noise-free correspondences of the scene, rounded to float32, and which of them lie on the plane."""
    a, b, on = project_pair(config, n, np.random.default_rng(seed))
    return a.astype(F32), b.astype(F32), on


def correspondences(spec):
    kp0, kp1, m0 = spec[:3]
    valid = m0 > -1
    return np.ascontiguousarray(kp0[valid]), np.ascontiguousarray(kp1[m0[valid]])


def pose_errors(T, Rm, t):
    """(rotation error, translation error) in degrees, the translation up to sign; atan2 of float64 values."""
    Rg, tg = T[:3, :3], T[:3, 3]
    D = Rm.T @ Rg
    ax = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    err_r = math.degrees(math.atan2(np.linalg.norm(ax), np.trace(D) - 1.0))
    err_t = math.degrees(math.atan2(np.linalg.norm(np.cross(t, tg)), abs(float(t @ tg))))
    return err_r, err_t


# three fixtures met the conditions with none of the seeds of search_seed(K, config, 1, 300) on their first scene: their SCENE, not
# only their seed, is drawn from another stream (the lowest stream that has a seed below 80)
SCENES = {(63, "sideways"): 1, (65, "general"): 1, (5, "plane7of8"): 1}

# RANSAC seed of every fixture (K, config): the lowest seed >= 1 that meets every condition of fixture_ok (search_seed below)
SEEDS = {(5, 'general'): 1, (5, 'forward'): 1, (5, 'sideways'): 1, (5, 'plane7of8'): 1, (6, 'general'): 1, (6, 'forward'): 1, (6, 'sideways'): 1,
         (6, 'plane7of8'): 179, (63, 'general'): 54, (63, 'forward'): 16, (63, 'sideways'): 2, (63, 'plane7of8'): 12, (64, 'general'): 2,
         (64, 'forward'): 237, (64, 'sideways'): 15, (64, 'plane7of8'): 41, (65, 'general'): 3, (65, 'forward'): 69, (65, 'sideways'): 87,
         (65, 'plane7of8'): 30, (255, 'general'): 3, (255, 'forward'): 6, (255, 'sideways'): 12, (255, 'plane7of8'): 5, (257, 'general'): 1,
         (257, 'forward'): 1, (257, 'sideways'): 4, (257, 'plane7of8'): 5, (1025, 'general'): 3, (1025, 'forward'): 1, (1025, 'sideways'): 1,
         (1025, 'plane7of8'): 4}


def seed_of(K, config):
    return SEEDS.get((K, config), 1)


@functools.lru_cache(maxsize=None)
def fixture_stage1(K, config, seed):
    spec = planted_spec(K, config)
    p0, p1 = correspondences(spec)
    return stage1_scores(p0, p1, spec[3], seed, max(ITERS))


@functools.lru_cache(maxsize=None)
def fixture_expected(K, config, iters, lo_iters, seed=None, reverse=False):
    spec = planted_spec(K, config)
    p0, p1 = correspondences(spec)
    seed = seed_of(K, config) if seed is None else seed
    return verify(p0, p1, spec[3], seed, iters, THRESH, lo_iters, stage1=fixture_stage1(K, config, seed) if K >= 5 else None, reverse=reverse)


def fixture_problems(K, config, seed=None):
    """Every reason why a GPU run of the fixture could not be compared exactly (empty: none).  With K <= 6 every sample holds all or all
    but one of the correspondences, so the best scores tie by construction and four or five votes cannot win by two: there the lowest
    hypothesis among equals is compared (every score is exact under MARGIN) and the vote has to be won by one."""
    bad = []
    for it in ITERS:
        for lo in LO_ITERS:
            v = fixture_expected(K, config, it, lo, seed)
            if not v["ok"]:
                bad.append((it, lo, "no model"))
                continue
            if v["margin"] < MARGIN:
                bad.append((it, lo, "margin", v["margin"]))
            if it > 1 and v["gap"] < 2 and K > 6:
                bad.append((it, lo, "gap", v["gap"]))
            if v["stab"] < STAB:
                bad.append((it, lo, "stab", v["stab"]))
            if v["vote_gap"] < (2 if K > 6 else 1) or v["depth"] < DEPTH:
                bad.append((it, lo, "votes", v["vote_gap"], v["depth"]))
    return bad


def search_seed(K, config, first=1, last=200):
    """How SEEDS was found."""
    for seed in range(first, last):
        if not fixture_problems(K, config, seed):
            return seed
    raise AssertionError(f"no RANSAC seed in range fits K = {K}, {config}")
