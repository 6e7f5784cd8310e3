"""NumPy float64 restatement of GIMS_AUX_RESECT_IMAGES, written from the specification in include/gims_hip.h (not from the kernel), and the
planted scenes the tests and tools/resect_bench.py share -- TEST INFRASTRUCTURE.

Stage 1 (the P3P hypotheses) is batched over the hypotheses of an entry, one array operation per step of the specification: the sampler,
the bearings, the quartic built by polynomial products, its real roots by bisection between the roots of successive derivatives, the
models from the two triangle frames, the integer scores.  Stage 2 and the final sweep run per entry.  No call into ``np.linalg`` or
``np.roots`` in the solver.  Every floating-point sum over correspondences goes through ``_acc``, forward or in reverse: the difference
between the two is the restatement's own sensitivity to summation order, from which the tests derive TOL_POSE.

Besides the outputs, every entry carries what a GPU test needs to be allowed to compare decisions exactly (``margins``):
  inlier   the smallest |e^2 / thresh^2 - 1| of every inlier decision that reaches an output: of the models of every hypothesis within
           two of the best score, of every model stage 2 evaluated, of the final sweep
  depth    the smallest |z| among the same decisions
  gap      best score minus the best score of any OTHER hypothesis (0: a tie, decided by the smaller h -- integers, so still exact)
  root     over the hypotheses within two of the best score: how far the quartic is from gaining or losing a real root (the smallest
           |p(e)| / sum |c_i| |e|^i over the interval ends e of the last level, as tests/pose_ref.py real_roots) and how far every sign
           condition (u > 0, v > 0, |D(u)| > 1e-12 a, the triangle bound) is from flipping, relative
  stab     the largest movement of a word of those models when the sample's coordinates move by 64 units in the last place
  lead     over the stage-2 comparisons of two costs at equal counts (they are compared as float32): the smallest relative distance of a
           cost from a float64 that rounds to another float32 (inf when no such comparison was made)"""
import numpy as np

from tests import triangulate_ref as TR

COUNTERS = ("n_ok", "n_failed", "n_corr_total", "n_inlier_total")
CAMERA_WORDS, HB, BISECTIONS = 6, 16, 80
WIGGLE = 2.0 ** -46                                # relative perturbation of a sample's coordinates: 64 units in the last place
_M64 = 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------------ the sampler
def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def sample3(seed, hyp, k):
    """Three DISTINCT indices in [0, k): the stream of the verification sampler for (seed, hyp)."""
    out, state = [], (seed ^ (hyp * 0xD1342543DE82EF95)) & _M64
    while len(out) < 3:
        state = _splitmix(state)
        idx = state % k
        if idx not in out:
            out.append(idx)
    return out


def _acc(terms, order):
    """The sum of the rows of terms [n, ...], one after the other."""
    terms = np.asarray(terms, dtype=np.float64)
    out = np.zeros(terms.shape[1:])
    for row in (terms if order == "forward" else terms[::-1]):
        out = out + row
    return out


# ------------------------------------------------------------------------------------------------ stage 1, batched over hypotheses
def _pmul(a, b):
    out = np.zeros((len(a), a.shape[1] + b.shape[1] - 1))
    for i in range(a.shape[1]):
        out[:, i:i + b.shape[1]] += a[:, i:i + 1] * b
    return out


def _horner(c, z):
    """c [H, n] ascending, z [H, m] -> [H, m]."""
    v = np.zeros_like(z) + c[:, -1:]
    for i in range(c.shape[1] - 2, -1, -1):
        v = v * z + c[:, i:i + 1]
    return v


def real_roots4(c):
    """c [H, 5] -> (roots [H, 4] ascending and padded with the bound, count [H], stab [H]); count 0 when c_4 == 0 or a coefficient is not
    finite.  The method of the specification: bisection between the roots of successive derivatives inside 1 + max |c_i / c_4|."""
    fact = (1, 1, 2, 6, 24)
    with np.errstate(all="ignore"):
        ok = (c[:, 4] != 0.0) & np.isfinite(c).all(1)
        bound = 1.0 + np.max(np.abs(c[:, :4] / c[:, 4:5]), 1)
        ok &= np.isfinite(bound)
        bound = np.where(ok, bound, 1.0)
        c = np.where(ok[:, None], c, 1.0)
        roots, stab, has = np.repeat(bound[:, None], 0, 1), None, None
        for d in range(1, 5):
            k = 4 - d
            q = np.stack([c[:, i + k] * float(fact[i + k] // fact[i]) for i in range(d + 1)], 1)
            ends = np.concatenate([-bound[:, None], roots, bound[:, None]], 1)
            fe = _horner(q, ends)
            if d == 4:
                stab = np.min(np.abs(fe) / _horner(np.abs(q), np.abs(ends)), 1)
            a, b = ends[:, :-1].copy(), ends[:, 1:].copy()
            sa, has = fe[:, :-1] > 0.0, (fe[:, :-1] > 0.0) != (fe[:, 1:] > 0.0)
            for _ in range(BISECTIONS):
                m = 0.5 * (a + b)
                same = (_horner(q, m) > 0.0) == sa
                a, b = np.where(same, m, a), np.where(same, b, m)
            r = np.where(has, 0.5 * (a + b), bound[:, None])
            roots = np.take_along_axis(r, np.argsort(~has, axis=1, kind="stable"), 1)
        count = has.sum(1)
    return roots, np.where(ok, count, 0), stab


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _frame(P1, P2, P3):
    """The frames of H triangles: (E [H, 3, 3] with e1, e2, e3 as ROWS, |e1 x (P3 - P1)|^2 [H])."""
    with np.errstate(all="ignore"):
        d = P2 - P1
        e1 = d / np.sqrt((d * d).sum(1))[:, None]
        n = _cross(e1, P3 - P1)
        nn = (n * n).sum(1)
        e3 = n / np.sqrt(nn)[:, None]
        return np.stack([e1, _cross(e3, e1), e3], 1), nn


def p3p(X, uv, cam):
    """X [H, 3, 3] world points and uv [H, 3, 2] pixels of H samples in the camera cam = (fx, fy, cx, cy)
    -> (models [H, 4, 12] = {R row-major, t} per root, valid [H, 4], root [H]: the hypothesis's distance from a change of its model set)."""
    fx, fy, cx, cy = cam
    H = len(X)
    with np.errstate(all="ignore"):
        x = np.stack([(uv[:, :, 0] - cx) / fx, (uv[:, :, 1] - cy) / fy, np.ones((H, 3))], 2)
        f = x / np.sqrt((x * x).sum(2))[:, :, None]
        c12, c13, c23 = (f[:, 0] * f[:, 1]).sum(1), (f[:, 0] * f[:, 2]).sum(1), (f[:, 1] * f[:, 2]).sum(1)
        d2 = lambda p, q: ((p - q) * (p - q)).sum(1)      # noqa: E731
        a, b, c = d2(X[:, 0], X[:, 1]), d2(X[:, 0], X[:, 2]), d2(X[:, 1], X[:, 2])
        EX, nnX = _frame(X[:, 0], X[:, 1], X[:, 2])
        tri = (a > 0.0) & (nnX > 1e-18 * b)
        one = np.ones(H)
        q = np.stack([one, -2.0 * c12, one], 1)
        N = np.stack([(b - c) - a, -2.0 * c12 * (b - c), (b - c) + a], 1)
        D = np.stack([-2.0 * a * c13, 2.0 * a * c23], 1)
        D2 = _pmul(D, D)
        qD2, N2, ND = _pmul(q, D2), _pmul(N, N), _pmul(N, D)
        pad = lambda p: np.concatenate([p, np.zeros((H, 5 - p.shape[1]))], 1)      # noqa: E731
        P = b[:, None] * qD2 - a[:, None] * (pad(D2) + N2 - 2.0 * c13[:, None] * pad(ND))
        roots, count, stab = real_roots4(P)
        models, valid = np.zeros((H, 4, 12)), np.zeros((H, 4), bool)
        near = np.where(tri, np.minimum(stab, np.abs(nnX / (1e-18 * b) - 1.0)), np.inf)
        for j in range(4):
            u = roots[:, j]
            have = tri & (j < count)
            Du, Nu, qu = _horner(D, u[:, None])[:, 0], _horner(N, u[:, None])[:, 0], _horner(q, u[:, None])[:, 0]
            v = Nu / Du
            ok = have & (u > 0.0) & (np.abs(Du) > 1e-12 * a) & (qu > 0.0) & (v > 0.0)
            s1 = np.sqrt(a / qu)
            Y = np.stack([s1[:, None] * f[:, 0], (u * s1)[:, None] * f[:, 1], (v * s1)[:, None] * f[:, 2]], 1)
            EY, _ = _frame(Y[:, 0], Y[:, 1], Y[:, 2])
            Rm = np.einsum("hkr,hks->hrs", EY, EX)                                   # R = E_Y E_X^T with the frames as columns
            t = Y[:, 0] - np.einsum("hrs,hs->hr", Rm, X[:, 0])
            M = np.concatenate([Rm.reshape(H, 9), t], 1)
            ok &= np.isfinite(M).all(1)
            models[:, j], valid[:, j] = np.where(ok[:, None], M, 0.0), ok
            # the sign conditions of a root that exists: relative distances from zero of u, D(u) (against its bound) and v
            scale_u = 1.0 + np.abs(u)
            cond = np.minimum(np.minimum(np.abs(u) / scale_u, np.abs(np.abs(Du) / (1e-12 * a) - 1.0)), np.abs(v) / (1.0 + np.abs(v)))
            cond = np.where(np.isnan(cond), 0.0, cond)
            near = np.where(have, np.minimum(near, cond), near)
    return models, valid, near


def _reproject(M, cam, X, uv):
    """-> (z [K], e2 [K]) of the K correspondences under the model M [12]."""
    fx, fy, cx, cy = cam
    Rm, t = M[:9].reshape(3, 3), M[9:]
    with np.errstate(all="ignore"):
        xc = X @ Rm.T + t
        z = xc[:, 2]
        ru, rv = fx * xc[:, 0] / z + cx - uv[:, 0], fy * xc[:, 1] / z + cy - uv[:, 1]
        return z, ru * ru + rv * rv


def _reproject_many(M, cam, X, uv):
    """M [n, 12] -> (z [n, K], e2 [n, K])."""
    fx, fy, cx, cy = cam
    with np.errstate(all="ignore"):
        xc = np.einsum("nrs,ks->nkr", M[:, :9].reshape(-1, 3, 3), X) + M[:, None, 9:]
        z = xc[:, :, 2]
        ru, rv = fx * xc[:, :, 0] / z + cx - uv[None, :, 0], fy * xc[:, :, 1] / z + cy - uv[None, :, 1]
        return z, ru * ru + rv * rv


def stage1(X, uv, cam, seed, iters, thresh2):
    """-> dict(score [iters, 4] (-1 without a model), models, valid, near, idx [iters, 3], z, e2 [iters, 4, K])."""
    K = len(X)
    idx = np.array([sample3(seed, h, K) for h in range(iters)], dtype=np.int64).reshape(iters, 3)
    models, valid, near = p3p(X[idx], uv[idx], cam)
    z, e2 = _reproject_many(models.reshape(-1, 12), cam, X, uv)
    inl = (z > 0.0) & (e2 <= thresh2)
    score = np.where(valid, inl.sum(1).reshape(iters, 4), -1)
    return dict(score=score, models=models, valid=valid, near=near, idx=idx, z=z.reshape(iters, 4, K), e2=e2.reshape(iters, 4, K))


# ------------------------------------------------------------------------------------------------ stage 2
def solve6(sums):
    """The 27 sums -> (d [6], regular): the elimination of the specification."""
    A = np.zeros((6, 7))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = sums[k]
            k += 1
    A[:, 6] = sums[21:27]
    diag = np.abs(np.diag(A[:, :6])).max()
    if not np.isfinite(diag):
        return None, False
    for c in range(6):
        piv = c + int(np.argmax(np.abs(A[c:, c])))                 # the first row of the largest magnitude
        if not np.abs(A[piv, c]) > 1e-12 * diag:
            return None, False
        if piv != c:
            A[[c, piv]] = A[[piv, c]]
        for r in range(c + 1, 6):
            fct = A[r, c] / A[c, c]
            A[r, c:] = A[r, c:] - fct * A[c, c:]
    d = np.zeros(6)
    for c in range(5, -1, -1):
        s = A[c, 6]
        for j in range(c + 1, 6):
            s = s - A[c, j] * d[j]
        d[c] = s / A[c, c]
    return d, True


def _evaluate(M, cam, X, uv, thresh2, order, note):
    z, e2 = _reproject(M, cam, X, uv)
    note(z, e2)
    inl = (z > 0.0) & (e2 <= thresh2)
    return int(inl.sum()), float(_acc(e2[inl], order)) if inl.any() else 0.0, inl


def _f32_lead(c):
    """How far the float64 c is from a number that rounds to another float32 than it does, relative to c."""
    f = np.float32(c)
    if not np.isfinite(f) or c <= 0.0:
        return 0.0
    lo, hi = (float(f) + float(np.nextafter(f, np.float32(-np.inf)))) / 2.0, (float(f) + float(np.nextafter(f, np.float32(np.inf)))) / 2.0
    return min(c - lo, hi - c) / c


def lo_round(M, inl, cam, X, uv, order):
    """One Gauss-Newton round over the inliers inl of the model M -> the candidate [12], or None when the solve is not regular or a word
    is not finite."""
    fx, fy, cx, cy = cam
    Rm, t = M[:9].reshape(3, 3), M[9:]
    with np.errstate(all="ignore"):
        Xi, uvi = X[inl], uv[inl]
        y = Xi @ Rm.T
        xc = y + t
        z = xc[:, 2]
        ru, rv = fx * xc[:, 0] / z + cx - uvi[:, 0], fy * xc[:, 1] / z + cy - uvi[:, 1]
        au, bu, av, bv = fx / z, -fx * xc[:, 0] / (z * z), fy / z, -fy * xc[:, 1] / (z * z)
        zero = np.zeros_like(z)
        ju = np.stack([bu * y[:, 1], au * y[:, 2] - bu * y[:, 0], -au * y[:, 1], au, zero, bu], 1)
        jv = np.stack([bv * y[:, 1] - av * y[:, 2], -bv * y[:, 0], av * y[:, 0], zero, av, bv], 1)
        terms = [ju[:, i] * ju[:, j] + jv[:, i] * jv[:, j] for i in range(6) for j in range(i, 6)]
        terms += [-(ju[:, i] * ru + jv[:, i] * rv) for i in range(6)]
        sums = _acc(np.stack(terms, 1), order)
        d, regular = solve6(sums)
        if not regular:
            return None
        th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        th = np.sqrt(th2)
        ca, cb = (np.sin(th) / th, (1.0 - np.cos(th)) / th2) if th > 1e-8 else (1.0, 0.5)
        W = np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
        W2 = np.array([[W[i, 0] * W[0, j] + W[i, 1] * W[1, j] + W[i, 2] * W[2, j] for j in range(3)] for i in range(3)])
        Ex = np.eye(3) + ca * W + cb * W2
        Rn = np.array([[Ex[i, 0] * Rm[0, j] + Ex[i, 1] * Rm[1, j] + Ex[i, 2] * Rm[2, j] for j in range(3)] for i in range(3)])
        cand = np.concatenate([Rn.reshape(9), t + d[3:]])
    return cand if np.isfinite(cand).all() else None


# ------------------------------------------------------------------------------------------------ the op
def gather(track_of, xyz, use, kpts, rec):
    """The dense list of one entry -> (X [K, 3], uv [K, 2] float64, keypoint index [K])."""
    N, T = len(track_of), len(use)
    n_k = int(rec[5])
    good = bool(np.isfinite(rec[:5]).all() and rec[0] > 0 and rec[1] > 0)
    keep = []
    for i in range(n_k if good else 0):
        g = rec[4] + float(i)
        if not 0 <= g < N:
            continue
        g = int(g)
        t = int(track_of[g])
        if not 0 <= t < T or use[t] == 0:
            continue
        if not (np.isfinite(xyz[t]).all() and np.isfinite(kpts[g]).all()):
            continue
        keep.append((i, g, t))
    if not keep:
        return np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0, np.int64)
    i, g, t = (np.array(v, dtype=np.int64) for v in zip(*keep))
    return xyz[t].astype(np.float64), kpts[g].astype(np.float64), i


def resect_entry(X, uv, cam, thresh=4.0, iters=1024, lo_iters=8, min_inliers=12, seed=0, order="forward", st1=None):
    """One entry from its dense list -> dict of the op's outputs for it (kp_* over the DENSE list) plus sens and margins."""
    K = len(X)
    thresh2 = float(np.float32(thresh)) ** 2
    out = dict(pose=np.zeros(12), n_corr=K, ok=0, n_inliers=0, best_hyp=-1, best_hyp_inliers=0, lo_rounds=0, rms_error=np.float32(0), root=-1,
               inlier=np.zeros(K, np.uint8), error=np.full(K, -1, np.float32), sens=np.zeros(K), final=np.zeros(12),
               margins=dict(inlier=np.inf, depth=np.inf, gap=np.inf, root=np.inf, stab=0.0, lead=np.inf))
    mg = out["margins"]
    if K < 3 or iters == 0:
        return out
    s = st1 if st1 is not None else stage1(X, uv, cam, seed, iters, thresh2)
    score = s["score"]
    flat = int(np.argmax(score))                                    # the first largest: the smallest h, then the smallest root
    bh, bj, best = flat // 4, flat % 4, int(score.reshape(-1)[flat])
    if best < 0:
        return out

    def note(z, e2):
        with np.errstate(all="ignore"):
            r = np.abs(e2 / thresh2 - 1.0)
        r, zz = r[np.isfinite(r)], np.abs(z[np.isfinite(z)])
        mg["inlier"] = min(mg["inlier"], float(r.min()) if len(r) else np.inf)
        mg["depth"] = min(mg["depth"], float(zz.min()) if len(zz) else np.inf)

    hyp_best = score.max(1)
    others = np.delete(hyp_best, bh)
    mg["gap"] = float(best - others.max()) if len(others) else np.inf
    close = np.nonzero(hyp_best >= best - 2)[0]
    for h in close:
        for j in np.nonzero(s["valid"][h])[0]:
            note(s["z"][h, j], s["e2"][h, j])
    mg["root"] = float(s["near"][close].min())
    wig = np.random.default_rng(12345)
    Xs, us = X[s["idx"][close]], uv[s["idx"][close]]
    m2, v2, _ = p3p(Xs * (1.0 + WIGGLE * wig.choice([-1.0, 1.0], Xs.shape)), us * (1.0 + WIGGLE * wig.choice([-1.0, 1.0], us.shape)), cam)
    same = (v2 == s["valid"][close]).all()
    mg["stab"] = float(np.abs(m2 - s["models"][close]).max()) if same else np.inf

    cur = s["models"][bh, bj].copy()
    n, c, inl = _evaluate(cur, cam, X, uv, thresh2, order, note)
    rounds = 0
    for _ in range(lo_iters):
        if n < 4:
            break
        cand = lo_round(cur, inl, cam, X, uv, order)
        if cand is None:
            break
        n2, c2, inl2 = _evaluate(cand, cam, X, uv, thresh2, order, note)
        if n2 == n:
            mg["lead"] = min(mg["lead"], _f32_lead(c), _f32_lead(c2))
        if not (n2 > n or (n2 == n and np.float32(c2) < np.float32(c))):
            break
        cur, n, c, inl, rounds = cand, n2, c2, inl2, rounds + 1
    z, e2 = _reproject(cur, cam, X, uv)
    note(z, e2)
    inl = (z > 0.0) & (e2 <= thresh2)
    n_in = int(inl.sum())
    out.update(best_hyp=bh, best_hyp_inliers=best, lo_rounds=rounds, root=bj, final=cur)
    if n_in < max(min_inliers, 4):
        return out
    with np.errstate(all="ignore"):
        err = np.where(z > 0, np.minimum(np.sqrt(e2), np.finfo(np.float32).max), -1.0)
        fx, fy = cam[0], cam[1]
        xc = X @ cur[:9].reshape(3, 3).T + cur[9:]
        ju = np.sqrt((fx / xc[:, 2]) ** 2 + (fx * xc[:, 0] / xc[:, 2] ** 2) ** 2)
        jv = np.sqrt((fy / xc[:, 2]) ** 2 + (fy * xc[:, 1] / xc[:, 2] ** 2) ** 2)
        # |d error| <= |d r / d x_c| |d x_c|, and a word of R or t moving by eps moves a component of x_c by at most eps (|X|_1 + 1)
        out["sens"] = np.sqrt(ju * ju + jv * jv) * np.sqrt(3.0) * (np.abs(X).sum(1) + 1.0)
    out.update(pose=cur, ok=1, n_inliers=n_in, rms_error=np.float32(np.sqrt(float(_acc(e2[inl], order)) / n_in)), inlier=inl.astype(np.uint8),
               error=err.astype(np.float32))
    return out


def resect(track_of, xyz, use, kpts, cams, thresh=4.0, iters=1024, lo_iters=8, min_inliers=12, seed=0, order="forward"):
    """The whole op -> dict(pose [m, 12], n_corr, ok, n_inliers, best_hyp, best_hyp_inliers, lo_rounds, rms_error [m], kp_inlier, kp_error [S],
    stats; and, not outputs of the op: root [m], kp_sens [S], slots [m + 1], margins [list of dicts])."""
    track_of, use = np.asarray(track_of, dtype=np.int64), np.asarray(use, dtype=np.uint8)
    xyz, kpts = np.asarray(xyz, dtype=np.float64).reshape(-1, 3), np.asarray(kpts, dtype=np.float32).reshape(-1, 2)
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, CAMERA_WORDS)
    m = len(cams)
    slots = np.concatenate([[0], np.cumsum(cams[:, 5].astype(np.int64))]) if m else np.zeros(1, np.int64)
    S = int(slots[-1])
    out = dict(pose=np.zeros((m, 12)), rms_error=np.zeros(m, np.float32), kp_inlier=np.zeros(S, np.uint8), kp_error=np.full(S, -1, np.float32),
               kp_sens=np.zeros(S), slots=slots, root=np.zeros(m, np.int64), margins=[])
    for k in ("n_corr", "ok", "n_inliers", "best_hyp", "best_hyp_inliers", "lo_rounds"):
        out[k] = np.zeros(m, np.int32)
    for e in range(m):
        X, uv, idx = gather(track_of, xyz, use, kpts, cams[e])
        r = resect_entry(X, uv, cams[e, :4], thresh, iters, lo_iters, min_inliers, seed, order)
        for k in ("pose", "n_corr", "ok", "n_inliers", "best_hyp", "best_hyp_inliers", "lo_rounds", "rms_error", "root"):
            out[k][e] = r[k]
        out["kp_inlier"][slots[e] + idx], out["kp_error"][slots[e] + idx], out["kp_sens"][slots[e] + idx] = r["inlier"], r["error"], r["sens"]
        out["margins"].append(r["margins"])
    out["stats"] = dict(n_ok=int(out["ok"].sum()), n_failed=int(m - out["ok"].sum()), n_corr_total=int(out["n_corr"].sum()),
                        n_inlier_total=int(out["n_inliers"].sum()))
    return out


# ------------------------------------------------------------------------------------------------ planted scenes
def pose_errors(M, Rp, tp):
    """The largest |R - R_planted| and |t - t_planted| of a model M [12]."""
    return float(np.abs(M[:9].reshape(3, 3) - Rp).max()), float(np.abs(M[9:] - tp).max())


def planted_set(seed, n, noise=0.0, wrong=0.0, planar=False, cam=3, n_cams=8, size=(1024, 768)):
    """n world points (a plane through the scene when planar) seen by arc camera `cam`: every point a track of its own
    -> dict(track_of, xyz, use, kpts, cams [1, 6], K, R, t, wrong)."""
    rng = np.random.default_rng(seed)
    K, R, t = TR.arc_cameras(n_cams, size=size)
    X = rng.uniform(-0.5, 0.5, (n, 3))
    if planar:
        X[:, 2] = 0.3 * X[:, 0] - 0.2 * X[:, 1] + 0.05
    uv = np.array([TR.project(K[cam], R[cam], t[cam], x) for x in X]).reshape(n, 2) + noise * rng.standard_normal((n, 2))
    bad = rng.random(n) < wrong
    uv[bad] = rng.uniform([0, 0], size, (int(bad.sum()), 2))
    rec = np.array([[K[cam, 0, 0], K[cam, 1, 1], K[cam, 0, 2], K[cam, 1, 2], 0.0, float(n)]])
    return dict(track_of=np.arange(n, dtype=np.int32), xyz=X, use=np.ones(n, np.uint8), kpts=uv.astype(np.float32), cams=rec, K=K[cam], R=R[cam], t=t[cam],
                wrong=bad)
