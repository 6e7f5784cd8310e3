"""NumPy restatement of the fundamental-matrix estimator of gims_verify_pairs (specification: include/gims_hip.h) -- TEST INFRASTRUCTURE.

Written with the loops of the specification: the sampler, the similarity normalisation, the Gauss-Jordan null vector, the Jacobi
eigenvector and the rank-2 step are spelled out here, none of them is a call into ``np.linalg``.  Sums over inliers run in the order of the
correspondences (``reverse=True``: in the opposite order, which is how the spread quoted in tests/test_fundamental_gpu.py was measured --
the device adds per-wave partial sums, so its order is neither).  oracle/eval_oracle.py holds the 4-point sampler; the 8-point one is its
continuation and is restated here.

Besides the expected outputs, ``verify`` returns the smallest |r^2 - thresh^2| over every inlier decision a GPU test compares: those of
every scored hypothesis and of every model of stage 2.  tests/test_fundamental_cpu.py asserts it for every committed (K, seed).

Scenes: random 3-D points in front of two pinhole cameras (800 x 600, focal length 700), a general motion or a pure x-translation (whose
F has F[2][2] = 0), pixel noise on image 1, 30 % outliers drawn uniformly, unmatched rows in between, coordinates rounded to float32."""
import functools
import math

import numpy as np

F32 = np.float32
HB = 16                                            # hypotheses per workgroup of the scoring kernel (csrc/verify.hip VF_HB)
KS = (0, 7, 8, 9, 63, 64, 65, 255, 257, 1025, 2049)          # wave, 256-thread tile and 1024-row chunk borders, each crossed by one
ITERS = (1, HB - 1, HB, HB + 1, 500)
LO_ITERS = (0, 8)
CONFIGS = ("general", "xtrans")
CANVAS = (800, 600)
FOCAL = 700.0
THRESH = 3.0
MARGIN = 1e-6                                      # px^2: smallest allowed |r^2 - thresh^2| of any inlier decision a GPU test compares
SWEEPS = 12                                        # csrc/verify.hip VF_JACOBI_SWEEPS
_M64 = 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------------ the estimator
def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def sample8(seed, hyp, k):
    """Eight DISTINCT indices in [0, k): the stream of oracle.eval_oracle.ransac_sample for (seed, hyp), continued."""
    out, state = [], (seed ^ (hyp * 0xD1342543DE82EF95)) & _M64
    while len(out) < 8:
        state = _splitmix(state)
        idx = state % k
        if idx not in out:
            out.append(idx)
    return np.asarray(out)


def _ssum(a, reverse=False):
    """Sum over axis 0, one term after the other."""
    a = np.asarray(a, dtype=np.float64)
    if len(a) == 0:
        return np.zeros(a.shape[1:])
    return np.cumsum(a[::-1] if reverse else a, axis=0)[-1]


def similarity(p, reverse=False):
    """(centroid, scale) of the specification's similarity(points)."""
    p = p.astype(np.float64)
    n = float(len(p))
    c = _ssum(p, reverse) / n
    m = _ssum(np.sqrt((p[:, 0] - c[0]) * (p[:, 0] - c[0]) + (p[:, 1] - c[1]) * (p[:, 1] - c[1])), reverse) / n
    return c, (1.0 if m == 0.0 else math.sqrt(2.0) / m)


def _rows(q0, q1):
    """[n, 9]: (u x, u y, u, v x, v y, v, x, y, 1) per normalised pair."""
    x, y, u, v = q0[:, 0], q0[:, 1], q1[:, 0], q1[:, 1]
    return np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], 1)


def null8x9(A):
    """Null vector of the 8 x 9 system by Gauss-Jordan elimination with complete pivoting (None: a zero or non-finite pivot)."""
    A = A.copy()
    rfree, cfree = np.ones(8, bool), np.ones(9, bool)
    piv = []
    with np.errstate(all="ignore"):
        for _ in range(8):
            mag = np.where(rfree[:, None] & cfree[None, :], np.abs(A), -1.0)
            mag = np.where(np.isnan(mag), -1.0, mag)
            flat = int(np.argmax(mag))                             # the first largest entry: lowest row, then lowest column
            pr, pc = divmod(flat, 9)
            best = mag[pr, pc]
            if not best > 0.0 or not np.isfinite(best):
                return None
            rfree[pr], cfree[pc] = False, False
            piv.append((pr, pc))
            m = A[:, pc] / A[pr, pc]
            m[pr] = 0.0
            A = A - m[:, None] * A[pr][None, :]
        fc = int(np.nonzero(cfree)[0][0])
        f = np.ones(9)
        for pr, pc in piv:
            f[pc] = -A[pr, fc] / A[pr, pc]
    return f if np.isfinite(f).all() else None


def unit(F):
    with np.errstate(all="ignore"):
        n2 = 0.0
        for c in F.reshape(9):
            n2 = n2 + c * c
        n = math.sqrt(n2) if n2 >= 0 else float("nan")
        if not n > 0.0 or not math.isfinite(n):
            return None
        F = F / n
    return F if np.isfinite(F).all() else None


def denormalise(fn, c0, s0, c1, s1):
    Fn = fn.reshape(3, 3)
    M = np.empty((3, 3))
    M[:, 0] = Fn[:, 0] * s0
    M[:, 1] = Fn[:, 1] * s0
    M[:, 2] = Fn[:, 2] - s0 * (Fn[:, 0] * c0[0] + Fn[:, 1] * c0[1])
    F = np.empty((3, 3))
    F[0] = s1 * M[0]
    F[1] = s1 * M[1]
    F[2] = M[2] - s1 * (c1[0] * M[0] + c1[1] * M[1])
    return F


def minimal_model(p0, p1):
    """F_h through eight pairs (None: no model)."""
    c0, s0 = similarity(p0)
    c1, s1 = similarity(p1)
    A = _rows((p0.astype(np.float64) - c0) * s0, (p1.astype(np.float64) - c1) * s1)
    f = null8x9(A)
    if f is None:
        return None
    with np.errstate(all="ignore"):
        return unit(denormalise(f, c0, s0, c1, s1))


def sampson(F, p0, p1):
    """(e^2, den) per correspondence; the squared Sampson distance is e^2 / den."""
    x, y = p0[:, 0].astype(np.float64), p0[:, 1].astype(np.float64)
    u, v = p1[:, 0].astype(np.float64), p1[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        a0 = F[0, 0] * x + F[0, 1] * y + F[0, 2]
        a1 = F[1, 0] * x + F[1, 1] * y + F[1, 2]
        a2 = F[2, 0] * x + F[2, 1] * y + F[2, 2]
        g0 = F[0, 0] * u + F[1, 0] * v + F[2, 0]
        g1 = F[0, 1] * u + F[1, 1] * v + F[2, 1]
        e = u * a0 + v * a1 + a2
        return e * e, a0 * a0 + a1 * a1 + g0 * g0 + g1 * g1


def decisions(F, p0, p1, t2):
    """(inlier mask, smallest |r^2 - thresh^2|)."""
    e2, den = sampson(F, p0, p1)
    with np.errstate(all="ignore"):
        mask = (den > 0.0) & (e2 <= t2 * den)
        margin = np.abs(e2 / den - t2)
    margin = margin[np.isfinite(margin)]
    return mask, (float(margin.min()) if len(margin) else np.inf)


def jacobi(S):
    """Eigenvector of the smallest eigenvalue of the symmetric S by cyclic Jacobi rotations, as the specification orders them."""
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
    m = 0
    for k in range(1, n):
        if S[k, k] < S[m, m]:
            m = k
    return V[:, m].copy()


def rank2(F):
    G = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            G[i, j] = F[0, i] * F[0, j] + F[1, i] * F[1, j] + F[2, i] * F[2, j]
    v = jacobi(G)
    fv = F[:, 0] * v[0] + F[:, 1] * v[1] + F[:, 2] * v[2]
    with np.errstate(all="ignore"):
        out = unit(F - fv[:, None] * v[None, :])
    return F if out is None else out


def lo_round(F_prev, p0, p1, t2, reverse=False):
    """One round of the local optimisation from the accepted model: the candidate F' (None: the round stops without one)."""
    mask, _ = decisions(F_prev, p0, p1, t2)
    if mask.sum() < 8:
        return None
    c0, s0 = similarity(p0[mask], reverse)
    c1, s1 = similarity(p1[mask], reverse)
    a = _rows((p0[mask].astype(np.float64) - c0) * s0, (p1[mask].astype(np.float64) - c1) * s1)
    S = np.empty((9, 9))
    for i in range(9):
        for j in range(i, 9):
            S[i, j] = S[j, i] = _ssum(a[:, i] * a[:, j], reverse)
    with np.errstate(all="ignore"):
        Fd = unit(denormalise(jacobi(S), c0, s0, c1, s1))
    return None if Fd is None else rank2(Fd)


def canonical(F):
    """The returned form: unit Frobenius norm (already), the entry of largest magnitude (the first such) positive."""
    f = F.reshape(9)
    m = 0
    for c in range(1, 9):
        if abs(f[c]) > abs(f[m]):
            m = c
    return -F if f[m] < 0.0 else F


def stage1_scores(p0, p1, seed, iters, thresh=THRESH):
    """Score of every hypothesis (-1: no model), its model, and the smallest margin of its decisions."""
    k, t2 = len(p0), float(thresh) ** 2
    scores, models, margins = np.full(iters, -1, dtype=np.int64), [None] * iters, np.full(iters, np.inf)
    if k < 8:
        return scores, models, margins
    for h in range(iters):
        s = sample8(seed, h, k)
        F = minimal_model(p0[s], p1[s])
        if F is None:
            continue
        mask, margins[h] = decisions(F, p0, p1, t2)
        scores[h] = int(mask.sum())
        models[h] = F
    return scores, models, margins


def verify(p0, p1, seed, iters, thresh=THRESH, lo_iters=8, stage1=None, reverse=False):
    """The specification on K correspondences p0[i] <-> p1[i] (float32 [K, 2]).  Returns ok, F (canonical form), mask [K] bool, n_inliers,
    best_hyp, best_hyp_inliers, lo_rounds, n_valid and `margin`: the smallest |r^2 - thresh^2| over the decisions of all `iters` hypotheses and
    of every model of stage 2.  stage1: stage1_scores() of at least `iters` hypotheses."""
    k, t2 = len(p0), float(thresh) ** 2
    none = dict(ok=0, F=None, mask=np.zeros(k, bool), n_inliers=0, best_hyp=0, best_hyp_inliers=0, lo_rounds=0, n_valid=k, margin=np.inf)
    if k < 8 or iters == 0:
        return none
    scores, models, margins = stage1 if stage1 is not None else stage1_scores(p0, p1, seed, iters, thresh)
    scores, models, margins = scores[:iters], models[:iters], margins[:iters]
    if scores.max() < 0:
        return none
    best = int(np.argmax(scores))                                  # first maximum: the lowest h among equals
    F = models[best]
    mask, _ = decisions(F, p0, p1, t2)
    margin, rounds = float(margins.min()), 0
    if lo_iters > 0:
        for _ in range(lo_iters):
            Fc = lo_round(F, p0, p1, t2, reverse)
            if Fc is None:
                break
            new, mg = decisions(Fc, p0, p1, t2)
            margin = min(margin, mg)
            if new.sum() < mask.sum():
                break
            same = bool((new == mask).all())
            F, mask, rounds = Fc, new, rounds + 1
            if same:
                break
    if rounds == 0:                                                # lo_iters == 0, or no accepted round: the best hypothesis made rank 2
        F = rank2(F)
        mask, mg = decisions(F, p0, p1, t2)
        margin = min(margin, mg)
    return dict(ok=1, F=canonical(F), mask=mask, n_inliers=int(mask.sum()), best_hyp=best, best_hyp_inliers=int(scores[best]), lo_rounds=rounds,
                n_valid=k, margin=margin)


# ------------------------------------------------------------------------------------------------ scenes
def cameras(config):
    """(Kmat, R, t) of the second camera; the first is Kmat [I | 0]."""
    w, h = CANVAS
    Kmat = np.array([[FOCAL, 0, w / 2.0], [0, FOCAL, h / 2.0], [0, 0, 1.0]])
    if config == "xtrans":
        return Kmat, np.eye(3), np.array([-0.8, 0.0, 0.0])
    rx, ry, rz = 0.04, -0.09, 0.03
    Rx = np.array([[1, 0, 0], [0, math.cos(rx), -math.sin(rx)], [0, math.sin(rx), math.cos(rx)]])
    Ry = np.array([[math.cos(ry), 0, math.sin(ry)], [0, 1, 0], [-math.sin(ry), 0, math.cos(ry)]])
    Rz = np.array([[math.cos(rz), -math.sin(rz), 0], [math.sin(rz), math.cos(rz), 0], [0, 0, 1]])
    return Kmat, Rz @ Ry @ Rx, np.array([0.7, 0.15, 0.3])


def planted_F(config):
    """F with x1^T F x0 = 0 for the two cameras: Kmat^-T [t]x R Kmat^-1."""
    Kmat, R, t = cameras(config)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(Kmat)
    return Ki.T @ tx @ R @ Ki


def project_pair(config, n, rng):
    """n scene points at depth 4 .. 12 seen by both cameras: exact projections [n, 2], [n, 2] in float64."""
    Kmat, R, t = cameras(config)
    w, h = CANVAS
    pix = rng.random((n, 2)) * [w, h]
    z = 4.0 + 8.0 * rng.random(n)
    X = np.concatenate([(pix - Kmat[:2, 2]) / FOCAL, np.ones((n, 1))], 1) * z[:, None]
    Y = X @ R.T + t
    q = Y @ Kmat.T
    return pix, q[:, :2] / q[:, 2:3]


@functools.lru_cache(maxsize=None)
def planted_spec(K, config, outlier_frac=0.3, noise=0.5):
    """(kp0 [n0, 2], kp1 [n1, 2], matches0 [n0], F_planted): K correspondences among n0 = K + K // 4 + 3 rows (the rest unmatched, spread
    through the array), image 1 permuted and three points longer; `noise` px of Gaussian noise on image 1; `outlier_frac` of the matched
    points of image 1 are replaced by points drawn uniformly over the canvas (none with K <= 9: the model takes eight)."""
    r = np.random.default_rng(7300 + K + (100000 if config == "xtrans" else 0))
    w, h = CANVAS
    n0 = K + K // 4 + 3
    n1 = n0 + 3
    a, b = project_pair(config, n0, r)
    b = b + noise * r.standard_normal((n0, 2))
    rows = np.sort(r.permutation(n0)[:K])
    wrong = rows[r.random(K) < outlier_frac] if K > 9 else rows[:0]
    b[wrong] = r.random((len(wrong), 2)) * [w, h]
    perm = r.permutation(n1)
    kp1 = np.zeros((n1, 2), dtype=F32)
    kp1[perm[:n0]] = b.astype(F32)
    kp1[perm[n0:]] = (r.random((n1 - n0, 2)) * [w, h]).astype(F32)
    m0 = np.full(n0, -1, dtype=np.int64)
    m0[rows] = perm[rows]
    return a.astype(F32), kp1, m0, planted_F(config)


def clean_pairs(config, n=64, seed=1):
    """Noise-free correspondences of the scene, rounded to float32."""
    a, b = project_pair(config, n, np.random.default_rng(seed))
    return a.astype(F32), b.astype(F32)


def correspondences(spec):
    kp0, kp1, m0 = spec[:3]
    valid = m0 > -1
    return np.ascontiguousarray(kp0[valid]), np.ascontiguousarray(kp1[m0[valid]])


# RANSAC seed of every fixture (K, config): the lowest seed >= 1 whose run meets MARGIN at every hypothesis count of ITERS and every
# lo_iters of LO_ITERS (search_seed below).  K < 8 has no model and no decisions.
SEEDS = {(K, config): 1 for K in (8, 9, 63, 64, 65, 255, 257, 1025, 2049) for config in CONFIGS}       # seed 1 fits every fixture


def seed_of(K, config):
    return SEEDS.get((K, config), 1)


@functools.lru_cache(maxsize=None)
def fixture_stage1(K, config, seed):
    p0, p1 = correspondences(planted_spec(K, config))
    return stage1_scores(p0, p1, seed, max(ITERS))


@functools.lru_cache(maxsize=None)
def fixture_expected(K, config, iters, lo_iters, seed=None, reverse=False):
    """verify() of the planted fixture at `iters` hypotheses; cached, read-only."""
    p0, p1 = correspondences(planted_spec(K, config))
    seed = seed_of(K, config) if seed is None else seed
    return verify(p0, p1, seed, iters, THRESH, lo_iters, stage1=fixture_stage1(K, config, seed) if K >= 8 else None, reverse=reverse)


def fixture_margin(K, config, seed=None):
    """The smallest margin over every run of the fixture that a GPU test compares."""
    return min(fixture_expected(K, config, it, lo, seed)["margin"] for it in ITERS for lo in LO_ITERS)


def search_seed(K, config, first=1, last=200):
    """How SEEDS was found."""
    for seed in range(first, last):
        if fixture_margin(K, config, seed) >= MARGIN:
            return seed
    raise AssertionError(f"no RANSAC seed in range fits K = {K}, {config}")
