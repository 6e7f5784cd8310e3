"""NumPy float64 restatement of GIMS_AUX_TRIANGULATE_TRACKS, written from the specification in include/gims_hip.h (not from the kernel), and
the planted scenes the tests and tools/triangulate_bench.py share.

``triangulate`` walks the tracks one by one.  Every sum over observations goes through ``_acc``, which adds the terms one after the other in
track order (``order='forward'``) or from the last to the first (``'reverse'``): the difference between the two is the restatement's own
sensitivity to summation order, from which the tests derive TOL_X.  ``trace``, when given a dict, collects what the fixture-margin tests
look at: every inlier decision (e^2 / thresh^2 and the depth), every angle that was compared with min_angle, and the lead of the best
hypothesis over the next one of equal count."""
import numpy as np

COUNTERS = ("n_ok", "n_low_angle", "n_no_model", "n_too_short", "n_too_long", "n_bad_obs", "n_inlier_obs")
TOO_SHORT, NO_MODEL, LOW_ANGLE, TOO_LONG = 1, 2, 4, 8
MAX_OBS, CAMERA_WORDS = 1024, 18


def camera_records(K, R, t, counts):
    """float64 [n, 18] = {fx, fy, cx, cy, R row-major, t, first node, n_k}."""
    K, R, t = (np.asarray(x, dtype=np.float64) for x in (K, R, t))
    n = len(counts)
    start = np.concatenate([[0], np.cumsum(counts)])
    rec = np.zeros((n, CAMERA_WORDS))
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    rec[:, 4:13] = R.reshape(n, 9)
    rec[:, 13:16] = t.reshape(n, 3)
    rec[:, 16], rec[:, 17] = start[:-1], counts
    return rec


def _acc(terms, order):
    """The sum of the rows of terms [n, ...], one after the other."""
    terms = np.asarray(terms, dtype=np.float64)
    out = np.zeros(terms.shape[1:])
    for row in (terms if order == "forward" else terms[::-1]):
        out = out + row
    return out


def solve_sym(A, b):
    """adj(A) b / det A for a symmetric 3 x 3 A, by cofactors -> (X, det)."""
    a00, a01, a02, a11, a12, a22 = A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = a00 * c00 + a01 * c01 + a02 * c02
    adj = np.array([[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]])
    with np.errstate(all="ignore"):
        return adj @ b / det, det


def angle_deg(X, Cp, Cq):
    a, b = X - Cp, X - Cq
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b)))


def _midpoint(d, C, order):
    P = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
    return solve_sym(_acc(P, order), _acc(np.einsum("nij,nj->ni", P, C), order))


def _reproject(X, f, c, R, t, uv):
    """-> (z [n], e2 [n]) of X in n observations."""
    xc = np.einsum("nij,j->ni", R, X) + t
    with np.errstate(all="ignore"):
        z = xc[:, 2]
        r = f * xc[:, :2] / z[:, None] + c - uv
        return z, (r * r).sum(axis=1)


def _note(trace, key, values):
    if trace is not None:
        trace.setdefault(key, []).extend(np.atleast_1d(values).tolist())


def triangulate(indptr, obs_image, obs_keypoint, kpts, cams, thresh=4.0, min_angle=1.5, max_hyp=64, refine_iters=10, order="forward", trace=None):
    indptr, obs_image, obs_keypoint = (np.asarray(x, dtype=np.int64) for x in (indptr, obs_image, obs_keypoint))
    kpts = np.asarray(kpts, dtype=np.float32).reshape(-1, 2)
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, CAMERA_WORDS)
    T, n_obs, n_images, N = len(indptr) - 1, len(obs_image), len(cams), len(kpts)
    thresh2, min_angle = float(np.float32(thresh)) ** 2, float(np.float32(min_angle))
    out = dict(xyz=np.zeros((T, 3)), max_angle=np.zeros(T, np.float32), rms_error=np.zeros(T, np.float32), n_inliers=np.zeros(T, np.int32),
               obs_error=np.full(n_obs, -1, np.float32), status=np.zeros(T, np.uint8), obs_inlier=np.zeros(n_obs, np.uint8))
    out["obs_sens"], out["min_dist"], out["track_bad"] = np.zeros(n_obs), np.ones(T), np.zeros(T, np.int64)      # (not outputs of the op)
    n_bad = 0
    cam_ok = np.isfinite(cams).all(axis=1) & (cams[:, 0] > 0) & (cams[:, 1] > 0) if n_images else np.zeros(0, bool)
    for tr in range(T):
        beg, end = int(indptr[tr]), int(indptr[tr + 1])
        if not 0 <= beg <= end <= n_obs:
            out["status"][tr] = TOO_SHORT
            continue
        L = end - beg
        if L > MAX_OBS:
            out["status"][tr] = TOO_LONG
            continue
        use, node = [], []
        for o in range(L):
            k, i = int(obs_image[beg + o]), int(obs_keypoint[beg + o])
            if not (0 <= k < n_images and cam_ok[k]):
                continue
            g = cams[k, 16] + float(i)
            if not (i >= 0 and i < cams[k, 17] and 0 <= g < N):
                continue
            if not np.isfinite(kpts[int(g)]).all():
                continue
            use.append(o)
            node.append(int(g))
        n_bad += L - len(use)
        out["track_bad"][tr] = L - len(use)
        Lu = len(use)
        if Lu < 2:
            out["status"][tr] = TOO_SHORT
            continue
        use = np.array(use)
        ks = obs_image[beg + use]
        rec = cams[ks]
        f, c, R, t = rec[:, 0:2], rec[:, 2:4], rec[:, 4:13].reshape(-1, 3, 3), rec[:, 13:16]
        uv = kpts[node].astype(np.float64)
        x = np.concatenate([(uv - c) / f, np.ones((Lu, 1))], axis=1)
        d = np.einsum("nji,nj->ni", R, x) / np.linalg.norm(x, axis=1, keepdims=True)
        C = -np.einsum("nji,nj->ni", R, t)

        if max_hyp >= 1:
            E = Lu * (Lu - 1) // 2
            H = min(E, max_hyp)
            pairs = [(p, q) for p in range(Lu) for q in range(p + 1, Lu)] if E <= 4096 else None
            best, scored = None, []
            for h in range(H):
                e = h * E // H
                if pairs is not None:
                    p, q = pairs[e]
                else:
                    p = 0
                    while (p + 1) * (2 * Lu - p - 2) // 2 <= e:
                        p += 1
                    q = p + 1 + e - p * (2 * Lu - p - 1) // 2
                X, det = _midpoint(d[[p, q]], C[[p, q]], order)
                if not det > 1e-12 * 8:
                    continue
                ang = angle_deg(X, C[p], C[q])
                _note(trace, "angles", ang)
                if not ang >= min_angle:
                    continue
                z, e2 = _reproject(X, f, c, R, t, uv)
                _note(trace, "e2_over_thresh2", e2 / thresh2)
                _note(trace, "depths", z)
                inl = (z > 0) & (e2 <= thresh2)
                n_h, c_h = int(inl.sum()), float(_acc(e2[inl], order)) if inl.any() else 0.0
                scored.append((n_h, c_h))
                if n_h >= 2 and (best is None or n_h > best[0] or (n_h == best[0] and c_h < best[1])):
                    best = (n_h, c_h, inl)
            if best is None:
                out["status"][tr] = NO_MODEL
                continue
            same = sorted(c_h for n_h, c_h in scored if n_h == best[0])
            if len(same) > 1:
                _note(trace, "cost_lead", (same[1] - same[0]) / max(same[0], 1e-300))
            S = best[2]
        else:
            S = np.ones(Lu, bool)

        X, det = _midpoint(d[S], C[S], order)
        if not det > 1e-12 * float(S.sum()) ** 3:
            out["status"][tr] = NO_MODEL
            continue
        fS, cS, RS, tS, uvS = f[S], c[S], R[S], t[S], uv[S]

        def cost_of(Y):
            z, e2 = _reproject(Y, fS, cS, RS, tS, uvS)
            return float(_acc(e2, order)), bool((z > 0).all())

        if refine_iters > 0:
            cost, _ = cost_of(X)
            for _ in range(refine_iters):
                with np.errstate(all="ignore"):
                    xc = np.einsum("nij,j->ni", RS, X) + tS
                    z = xc[:, 2:3]
                    r = fS * xc[:, :2] / z + cS - uvS
                    ju = fS[:, 0:1] * (RS[:, 0] - xc[:, 0:1] / z * RS[:, 2]) / z
                    jv = fS[:, 1:2] * (RS[:, 1] - xc[:, 1:2] / z * RS[:, 2]) / z
                    JtJ = _acc(ju[:, :, None] * ju[:, None, :] + jv[:, :, None] * jv[:, None, :], order)
                    g = _acc(-(ju * r[:, 0:1] + jv * r[:, 1:2]), order)
                    step, det = solve_sym(JtJ, g)
                if not det > 0:
                    break
                cost_y, front = cost_of(X + step)
                if not (front and cost_y < cost):
                    break
                X, cost = X + step, cost_y

        z, e2 = _reproject(X, f, c, R, t, uv)
        _note(trace, "e2_over_thresh2", e2 / thresh2)
        _note(trace, "depths", z)
        inl = (z > 0) & (e2 <= thresh2)
        n_in = int(inl.sum())
        if n_in < 2 or len(set(ks[inl].tolist())) < 2:
            out["status"][tr] = NO_MODEL
            continue
        a = X - C[inl]                                      # angle_deg over all pairs of inliers at once
        cr = np.linalg.norm(np.cross(a[:, None, :], a[None, :, :]), axis=2)
        ang = float(np.degrees(np.arctan2(cr, a @ a.T))[np.triu_indices(n_in, 1)].max())
        _note(trace, "angles", ang)
        with np.errstate(all="ignore"):
            err = np.where(z > 0, np.minimum(np.sqrt(e2), np.finfo(np.float32).max), -1.0)
        with np.errstate(all="ignore"):                     # for the tests' error bars: |d error / d X| per observation, the nearest inlier centre
            xc = np.einsum("nij,j->ni", R, X) + t
            ju = f[:, 0:1] * (R[:, 0] - xc[:, 0:1] / xc[:, 2:3] * R[:, 2]) / xc[:, 2:3]
            jv = f[:, 1:2] * (R[:, 1] - xc[:, 1:2] / xc[:, 2:3] * R[:, 2]) / xc[:, 2:3]
            out["obs_sens"][beg + use] = np.sqrt((ju * ju).sum(axis=1) + (jv * jv).sum(axis=1))
        out["min_dist"][tr] = np.linalg.norm(X - C[inl], axis=1).min()
        out["xyz"][tr], out["max_angle"][tr], out["n_inliers"][tr] = X, ang, n_in
        out["rms_error"][tr] = np.sqrt(float(_acc(e2[inl], order)) / n_in)
        out["obs_error"][beg + use] = err
        out["obs_inlier"][beg + use] = inl
        out["status"][tr] = LOW_ANGLE if ang < min_angle else 0
    st = out["status"]
    out["stats"] = dict(n_ok=int((st == 0).sum()), n_low_angle=int((st == LOW_ANGLE).sum()), n_no_model=int((st == NO_MODEL).sum()),
                        n_too_short=int((st == TOO_SHORT).sum()), n_too_long=int((st == TOO_LONG).sum()), n_bad_obs=n_bad,
                        n_inlier_obs=int(out["n_inliers"].sum()))
    return out


# ------------------------------------------------------------------------------------------------ planted scenes
def look_at(centre, target):
    """R (world to camera, z forward) of a camera at centre looking at target, and t = -R centre."""
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x = x / np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ centre


def arc_cameras(n, radius=4.0, span=np.pi, focal=800.0, size=(1024, 768), jitter=None):
    """n cameras on an arc of `span` radians around the origin, looking at it: K [n, 3, 3], R [n, 3, 3], t [n, 3]."""
    K = np.tile(np.array([[focal, 0, size[0] / 2], [0, focal, size[1] / 2], [0, 0, 1.0]]), (n, 1, 1))
    Rs, ts = [], []
    for j in range(n):
        a = span * (j + 0.5) / n - span / 2
        cen = radius * np.array([np.sin(a), 0.15 * np.cos(3 * a), -np.cos(a)])
        if jitter is not None:
            cen = cen + jitter[j]
        R, t = look_at(cen, np.zeros(3))
        Rs.append(R)
        ts.append(t)
    return K, np.array(Rs), np.array(ts)


def project(K, R, t, X):
    xc = R @ X + t
    return np.array([K[0, 0] * xc[0] / xc[2] + K[0, 2], K[1, 1] * xc[1] / xc[2] + K[1, 2]])


def planted_tracks(seed, lengths, n_cams=12, noise=0.5, p_wrong=0.2, min_len_wrong=4, size=(1024, 768)):
    """Tracks of the given lengths over n_cams arc cameras around points in the cube [-0.5, 0.5]^3 (scene extent 1): every observation is a
    keypoint of its own.  A track of up to n_cams observations takes distinct cameras; a longer one walks round them.  On tracks of at
    least min_len_wrong observations each observation is replaced, with probability p_wrong, by a random pixel.
    -> dict(indptr, obs_image, obs_keypoint, kpts float32 [N, 2], K, R, t, counts, cams float64 [n, 18], points [T, 3], wrong bool [n_obs])."""
    rng = np.random.default_rng(seed)
    K, R, t = arc_cameras(n_cams, size=size)
    per_image = [[] for _ in range(n_cams)]
    obs_image, obs_slot, wrong, points, indptr = [], [], [], [], [0]
    for L in lengths:
        X = rng.uniform(-0.5, 0.5, 3)
        points.append(X)
        ks = rng.permutation(n_cams)[:L] if L <= n_cams else (rng.integers(0, n_cams) + np.arange(L)) % n_cams
        ks = np.sort(ks) if L <= n_cams else ks
        for k in ks:
            w = L >= min_len_wrong and rng.random() < p_wrong
            px = rng.uniform([0, 0], size) if w else project(K[k], R[k], t[k], X) + noise * rng.standard_normal(2)
            obs_image.append(int(k))
            obs_slot.append(len(per_image[k]))
            per_image[k].append(px)
            wrong.append(w)
        indptr.append(len(obs_image))
    counts = [len(p) for p in per_image]
    kpts = np.concatenate([np.array(p, dtype=np.float64).reshape(-1, 2) for p in per_image]).astype(np.float32)
    return dict(indptr=np.array(indptr, np.int32), obs_image=np.array(obs_image, np.int32), obs_keypoint=np.array(obs_slot, np.int32), kpts=kpts,
                K=K, R=R, t=t, counts=counts, cams=camera_records(K, R, t, counts), points=np.array(points).reshape(-1, 3), wrong=np.array(wrong, bool))


def planted_matches(seed, n_cams, n_points, n_kp, noise=0.5, w_wrong=0.03, neighbours=3, size=(1024, 768), span=np.pi):
    """An image set as match_features would hand it over: n_cams arc cameras, n_points planted points, every image sees the points that
    project inside it (at most n_kp of them, in random order); pairs (k, k + j), j = 1 .. neighbours; matches0 of a pair = the planted
    correspondences, a fraction w_wrong of the rows pointed at a random keypoint instead.
    -> dict(counts, kpts [list of float32 [n_k, 2]], point_of [list of int arrays], pairs, matches [list of int64], K, R, t, points)."""
    rng = np.random.default_rng(seed)
    K, R, t = arc_cameras(n_cams, size=size, span=span)
    X = rng.uniform(-0.5, 0.5, (n_points, 3))
    kpts, point_of = [], []
    for k in range(n_cams):
        xc = X @ R[k].T + t[k]
        uv = np.stack([K[k, 0, 0] * xc[:, 0] / xc[:, 2] + K[k, 0, 2], K[k, 1, 1] * xc[:, 1] / xc[:, 2] + K[k, 1, 2]], axis=1)
        seen = np.nonzero((xc[:, 2] > 0) & (uv[:, 0] >= 0) & (uv[:, 0] < size[0]) & (uv[:, 1] >= 0) & (uv[:, 1] < size[1]))[0]
        seen = rng.permutation(seen)[:n_kp]
        kpts.append((uv[seen] + noise * rng.standard_normal((len(seen), 2))).astype(np.float32))
        point_of.append(seen)
    pairs, matches = [], []
    for a in range(n_cams):
        for j in range(1, neighbours + 1):
            b = a + j
            if b >= n_cams:
                continue
            where = np.full(n_points, -1, np.int64)
            where[point_of[b]] = np.arange(len(point_of[b]))
            m = where[point_of[a]]
            bad = rng.random(len(m)) < w_wrong
            m[bad] = rng.integers(0, max(len(point_of[b]), 1), int(bad.sum()))
            pairs.append((a, b))
            matches.append(m)
    return dict(counts=[len(p) for p in point_of], kpts=kpts, point_of=point_of, pairs=pairs, matches=matches, K=K, R=R, t=t, points=X)
