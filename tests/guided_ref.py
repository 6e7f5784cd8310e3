"""Float64 NumPy restatement of guided matching (include/gims_hip.h, GIMS_AUX_GUIDED_MATCH) and the fixtures it is tested on.

Every product and every sum of the gate is one NumPy operation on float64 arrays, in the header's order; NumPy does not contract them.
The distance is ``nn_ref.exact_sq``, unchanged.  To stay fast only the admissible columns that can be among a row's two nearest are
evaluated in that order, preselected by a float64 BLAS product as in ``nn_ref.two_nearest``."""
import numpy as np

from gims_amd import synth
from tests import fundamental_ref as FR
from tests.nn_ref import exact_sq

HOMOGRAPHY, FUNDAMENTAL = 0, 1
INFO = ("fallback_rows0", "fallback_rows1", "n_fixed", "n_bad_prior", "n_dup_prior", "no_model", "n_added")
F32 = np.float32


def has_model(model, ok=None):
    with np.errstate(over="ignore"):
        return (ok is None or float(ok) != 0.0) and bool(np.isfinite(np.asarray(model, F32)).all())


def fixed_rows(prior, mask, n0, n1):
    """-> fixed bool [n0], taken bool [n1], n_bad_prior, n_dup_prior (step 2 of the header)."""
    fixed, taken = np.zeros(n0, bool), np.zeros(n1, bool)
    if prior is None:
        return fixed, taken, 0, 0
    prior = np.asarray(prior, np.int64)
    on = np.ones(n0, bool) if mask is None else np.asarray(mask) != 0
    claims = on & (prior >= 0) & (prior < n1)
    n_bad = int((on & ~claims & (prior != -1)).sum())
    owner = np.full(n1, n0, np.int64)
    np.minimum.at(owner, prior[claims], np.nonzero(claims)[0])
    rows = np.nonzero(claims)[0]
    fixed[rows] = owner[prior[rows]] == rows
    taken[prior[fixed]] = True
    return fixed, taken, n_bad, int(claims.sum() - fixed.sum())


def _lin(a, x, b, y, c):
    return (a * x + b * y) + c


def row_words(kind, model, kp0, kp1):
    """The per-row words of step 3 in float64: (A rows [n0, 4], B rows [n1, 4]).  fundamental: {la, lb, lc, g} and {u', v', 1, h};
    homography: {ax, ay, u, v} and {bx, by, u', v'}, NaN in a row that is not valid."""
    M = np.asarray(model, F32).astype(np.float64).reshape(9)
    u, v = kp0[:, 0].astype(np.float64), kp0[:, 1].astype(np.float64)
    s, t = kp1[:, 0].astype(np.float64), kp1[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        if kind == FUNDAMENTAL:
            la, lb, lc = _lin(M[0], u, M[1], v, M[2]), _lin(M[3], u, M[4], v, M[5]), _lin(M[6], u, M[7], v, M[8])
            ma, mb = _lin(M[0], s, M[3], t, M[6]), _lin(M[1], s, M[4], t, M[7])
            return np.stack([la, lb, lc, la * la + lb * lb], 1), np.stack([s, t, np.ones_like(s), ma * ma + mb * mb], 1)
        px, py, pw = _lin(M[0], u, M[1], v, M[2]), _lin(M[3], u, M[4], v, M[5]), _lin(M[6], u, M[7], v, M[8])
        cof = lambda a, b, c, d: M[a] * M[b] - M[c] * M[d]                     # noqa: E731
        C = [cof(4, 8, 5, 7), cof(2, 7, 1, 8), cof(1, 5, 2, 4), cof(5, 6, 3, 8), cof(0, 8, 2, 6), cof(2, 3, 0, 5), cof(3, 7, 4, 6), cof(1, 6, 0, 7),
             cof(0, 4, 1, 3)]
        qx, qy, qw = _lin(C[0], s, C[1], t, C[2]), _lin(C[3], s, C[4], t, C[5]), _lin(C[6], s, C[7], t, C[8])
        wa = np.stack([px / pw, py / pw, u, v], 1)
        wb = np.stack([qx / qw, qy / qw, s, t], 1)
        wa[~(np.abs(pw) > 0)] = np.nan
        wb[~(np.abs(qw) > 0)] = np.nan
    return wa, wb


def admissible(kind, thresh, wa, wb, fixed=None, taken=None):
    """bool [n0, n1]: step 4.  A comparison with a NaN is false."""
    t2 = float(F32(thresh)) * float(F32(thresh))
    a = [wa[:, k][:, None] for k in range(4)]
    b = [wb[:, k][None, :] for k in range(4)]
    with np.errstate(all="ignore"):
        if kind == FUNDAMENTAL:
            n = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
            n2 = n * n
            adm = (a[3] > 0) & (b[3] > 0) & (n2 <= t2 * a[3]) & (n2 <= t2 * b[3])
        else:
            dx, dy, ex, ey = a[0] - b[2], a[1] - b[3], b[0] - a[2], b[1] - a[3]
            adm = (dx * dx + dy * dy <= t2) & (ex * ex + ey * ey <= t2)
    if fixed is not None:
        adm = adm & ~fixed[:, None]
    if taken is not None:
        adm = adm & ~taken[None, :]
    return adm


def two_nearest(a, b, adm):
    """a [n0, d], b [n1, d] float32, adm bool [n0, n1] -> nn1, nn2 (int64, -1: none), s1, s2 (float64 exact squared distances, +inf: none)."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    approx = (a64 * a64).sum(1)[:, None] + (b64 * b64).sum(1)[None, :] - 2.0 * (a64 @ b64.T)
    approx = np.where(adm, approx, np.inf)
    n0 = a.shape[0]
    second = np.partition(approx, 1, axis=1)[:, 1] if b.shape[0] > 1 else np.full(n0, np.inf)
    nn1, nn2 = -np.ones(n0, np.int64), -np.ones(n0, np.int64)
    s1, s2 = np.full(n0, np.inf), np.full(n0, np.inf)
    for i in range(n0):
        lim = second[i] + 1e-9 * (1.0 + abs(second[i])) if np.isfinite(second[i]) else np.inf
        cols = np.nonzero(adm[i] & (approx[i] <= lim))[0]
        if len(cols) == 0:
            continue
        s = exact_sq(a[i], b[cols])
        order = np.lexsort((cols, s))
        nn1[i], s1[i] = cols[order[0]], s[order[0]]
        if len(cols) > 1:
            nn2[i], s2[i] = cols[order[1]], s[order[1]]
    return nn1, nn2, s1, s2


def solve(a, b, kp0, kp1, model, kind, *, ok=None, prior=None, mask=None, scores=None, thresh=3.0, ratio=0.8, max_distance=None, mutual=True):
    """a [n0, d], b [n1, d] float32 point-major -> dict of the header's outputs (float32 where the header says so) and float64 helpers for
    the margins: ratio64, and d1_64 = sqrt(S1)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    kp0, kp1 = np.asarray(kp0, F32), np.asarray(kp1, F32)
    n0, n1 = a.shape[0], b.shape[0]
    fixed, taken, n_bad, n_dup = fixed_rows(prior, mask, n0, n1)
    model_ok = has_model(model, ok)
    if model_ok:
        wa, wb = row_words(kind, model, kp0, kp1)
        adm = admissible(kind, thresh, wa, wb, fixed, taken)
    else:
        adm = np.zeros((n0, n1), bool)
    nn1, nn2, s1, s2 = two_nearest(a, b, adm)
    maxd = F32(np.inf) if max_distance is None else F32(max_distance)
    with np.errstate(divide="ignore", invalid="ignore"):
        d1, d2 = np.sqrt(s1).astype(F32), np.sqrt(s2).astype(F32)
        rat = (d1 / d2).astype(F32)
        ratio64 = np.sqrt(s1) / np.sqrt(s2)
        match = (rat < F32(ratio)) & (d1 <= maxd)
    out = dict(n_admissible=adm.sum(1).astype(np.int32), ratio64=ratio64, d1_64=np.sqrt(s1), adm=adm, fixed=fixed, taken=taken)
    if mutual:
        c1, _, _, _ = two_nearest(b, a, np.ascontiguousarray(adm.T))
        match = match & (nn1 >= 0) & (c1[np.maximum(nn1, 0)] == np.arange(n0))
        out["cnn1"] = c1.astype(np.int32)
    match = match & ~fixed
    pr = np.asarray(prior, np.int64) if prior is not None else np.zeros(n0, np.int64)
    sc = np.asarray(scores, F32) if scores is not None else np.ones(n0, F32)
    out["nn1"] = np.where(fixed, pr, nn1).astype(np.int32)
    out["nn2"] = np.where(fixed, -1, nn2).astype(np.int32)
    out["d1"] = np.where(fixed, F32(np.inf), d1).astype(F32)
    out["d2"] = np.where(fixed, F32(np.inf), d2).astype(F32)
    out["ratio"] = np.where(fixed, F32(np.nan), rat).astype(F32)
    out["added0"] = match.astype(np.uint8)
    out["matches0"] = np.where(fixed, pr, np.where(match, nn1, -1)).astype(np.int64)
    out["scores0"] = np.where(fixed, sc, np.where(match, F32(1) - rat, F32(0))).astype(F32)
    if mutual:
        m1 = -np.ones(n1, np.int64)
        rows = np.nonzero(out["matches0"] >= 0)[0]
        m1[out["matches0"][rows]] = rows
        out["matches1"] = m1
    out["info"] = np.array([0, 0, int(fixed.sum()), n_bad, n_dup, 0 if model_ok else 1, int(match.sum()), 0], np.int32)
    return out


def margins(ref, ratio, max_distance=None):
    """(smallest |float64 ratio - threshold| over the searching rows with two admissible columns, smallest distance in float32 ulps of d1 to
    max_distance): what a fixture must keep away from a decision's edge.  No row is ever excluded from a comparison."""
    r = ref["ratio64"][np.isfinite(ref["ratio64"]) & ~ref["fixed"]]
    near = float(np.abs(r - float(F32(ratio))).min()) if len(r) else np.inf
    if max_distance is None:
        return near, np.inf
    d = ref["d1_64"][np.isfinite(ref["d1_64"]) & ~ref["fixed"]]
    m = float(F32(max_distance))
    ulps = float((np.abs(d - m) / np.spacing(F32(m)).astype(np.float64)).min()) if len(d) else np.inf
    return near, ulps


# ------------------------------------------------------------------------------------------------ fixtures
def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)


def noisy(rng, x, sigma):
    y = x.astype(np.float64) + sigma * rng.standard_normal(x.shape)
    return (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(F32)


def planted_descriptors(K, config, d=128, sigma=0.03, seed=0):
    """Descriptors for ``fundamental_ref.planted_spec(K, config)``: row i of A and the column the fixture built as its partner (matched,
    unmatched and geometric-outlier rows alike) share a descriptor up to ``sigma`` per channel.  Then, as repeated structure does, the true
    partners -- rows of matches0 that are admissible under the planted F --, every second one at the most, are given a near-copy of their
    descriptor ELSEWHERE in image 1: on the columns that are nobody's match in the fixture, as far as those go.
    -> (A [n0, d], B [n1, d], kp0, kp1, matches0, F float32 [9], true rows)."""
    kp0, kp1, m0, F = FR.planted_spec(K, config)
    n0, n1 = len(kp0), len(kp1)
    rng = np.random.default_rng(91000 + K + (7 if config == "xtrans" else 0) + 1000003 * seed)
    A = unit_rows(rng, n0, d)
    B = unit_rows(rng, n1, d)
    # the column of row i, matched or not: invert the fixture's construction through the keypoints it wrote
    r = np.random.default_rng(7300 + K + (100000 if config == "xtrans" else 0))
    FR.project_pair(config, n0, r)
    r.standard_normal((n0, 2))
    rows = np.sort(r.permutation(n0)[:K])
    wrong = rows[r.random(K) < 0.3] if K > 9 else rows[:0]
    r.random((len(wrong), 2))
    perm = r.permutation(n1)
    assert (m0[rows] == perm[rows]).all()
    B[perm[:n0]] = noisy(rng, A, sigma)
    Ff = (F / np.linalg.norm(F)).astype(F32).reshape(9)
    wa, wb = row_words(FUNDAMENTAL, Ff, kp0, kp1)
    adm = admissible(FUNDAMENTAL, 3.0, wa, wb)
    true = np.array([i for i in rows if adm[i, m0[i]]], np.int64)
    free = np.concatenate([perm[np.setdiff1d(np.arange(n0), rows)], perm[n0:]])
    twins = true[::2][:len(free)]
    B[free[:len(twins)]] = noisy(rng, A[twins], sigma)
    return A, B, kp0, kp1, m0, Ff, true


def homography_fixture(n=300, seed=5, sigma=0.03, d=128):
    """``synth.make_homography_pair`` with descriptors of its own dimension cut to d and renormalised, every second true pair twinned on an
    outlier column.  -> (A, B, kp0, kp1, gt int64 [n0], H float32 [9])."""
    pair, H = synth.make_homography_pair(n, seed)
    kp0, kp1, gt = pair["keypoints0"][0].astype(F32), pair["keypoints1"][0].astype(F32), pair["gt_perm"].astype(np.int64)
    rng = np.random.default_rng(92000 + n + 31 * seed)
    A = unit_rows(rng, n, d)
    B = unit_rows(rng, len(kp1), d)
    has = gt >= 0
    B[gt[has]] = noisy(rng, A[has], sigma)
    free = np.setdiff1d(np.arange(len(kp1)), gt[has])
    twins = np.nonzero(has)[0][::2][:len(free)]
    B[free[:len(twins)]] = noisy(rng, A[twins], sigma)
    return A, B, kp0, kp1, gt, np.asarray(H, F32).reshape(9)


def plain_mutual(a, b, ratio=0.8):
    """The plain mutual ratio test (nn_ref.solve's MNN) as matches0."""
    from tests import nn_ref
    return nn_ref.solve(np.ascontiguousarray(a.T), np.ascontiguousarray(b.T), ratio, True)["matches0"]
