"""NumPy float64 restatement of GIMS_AUX_BUNDLE_ADJUST, written from the specification in include/gims_hip.h (not from the kernel), and the
planted scenes the tests and tools/ba_bench.py share.

``adjust`` performs the operations of the specification one at a time, in its association and order (``order='forward'``): elementwise
NumPy arithmetic on float64 is the same IEEE operation the device performs, so what separates the two is the last bit of sin / cos in the
exponential map.  ``order='reverse'`` takes every sum over observations, and the sum of the points' costs, from the last term to the first:
the difference between the two is the restatement's own sensitivity to summation order, from which the tests derive TOL_BA.  The result
also carries what the fixture-margin tests look at (``margins``) and a per-observation bound on |d error / d parameter| (``obs_sens``).

``dense_step`` solves the full damped normal equations of one round without the Schur complement; ``residuals`` evaluates the cost function
for central differences."""
import numpy as np

from tests import triangulate_ref as TR

COUNTERS = ("n_free", "n_fixed", "n_held", "n_points", "n_active_obs", "n_bad_obs", "rounds_taken", "status")
MAX_OBS, CAMERA_WORDS, MAX_FREE, MAX_REJECTS = 1024, 18, 128, 5
BAD_CAMERA, BAD_START = 1, 2


def out_layout(T, n_obs, n_images, iters, n_free):
    """The byte offsets of the op's buffer by the formula of the header."""
    al = lambda x: (x + 255) & ~255      # noqa: E731
    n = 6 * n_free
    sizes = [("xyz", 24 * T), ("cams", 144 * n_images), ("obs_error", 4 * n_obs), ("cam_obs", 4 * n_images), ("history", 16 * (iters + 1)), ("taken", iters),
             ("counters", 32)]
    off, at = {}, 0
    for name, size in sizes:
        off[name] = at
        at += al(size)
    off["outputs"] = off["scratch"] = at
    scratch = [256, 4 * n_images, 4 * n_free, 4 * n_free + 4, 4 * n_free, 24 * T, 144 * n_images, T, n_obs, 4 * n_obs, 4 * n_obs, 4 * n_obs, 4 * n_obs, 4 * n_obs, 72 * T, 400 * n_obs,
               8 * T, 8 * n * n, 8 * n]
    off["bytes"] = at + sum(al(s) for s in scratch)
    return off


# ------------------------------------------------------------------------------------------------ activity
def classify(indptr, obs_image, obs_keypoint, obs_use, point_use, kpts, xyz, cams, mode):
    """-> dict(pt_act [T], obs_act [n_obs], obs_track, obs_node, cam_obs [n_images], n_bad, status bit 1)."""
    T, n_obs, n_images, N = len(indptr) - 1, len(obs_image), len(cams), len(kpts)
    cam_ok = (np.isfinite(cams).all(axis=1) & (cams[:, 0] > 0) & (cams[:, 1] > 0)) if n_images else np.zeros(0, bool)
    status = BAD_CAMERA if ((mode != 0) & ~cam_ok).any() else 0
    pt_act, obs_act = np.zeros(T, bool), np.zeros(n_obs, bool)
    obs_track, obs_node = np.full(n_obs, -1, np.int64), np.full(n_obs, -1, np.int64)
    n_bad = 0
    for t in range(T):
        beg, end = int(indptr[t]), int(indptr[t + 1])
        if not (0 <= beg <= end <= n_obs) or end - beg > MAX_OBS:
            continue
        point = bool(point_use[t]) and bool(np.isfinite(xyz[t]).all())
        cand = []
        for o in range(beg, end):
            k, i = int(obs_image[o]), int(obs_keypoint[o])
            if not (point and obs_use[o] and 0 <= k < n_images and mode[k] != 0 and cam_ok[k]):
                continue
            g = cams[k, 16] + float(i)
            if not (0 <= i < cams[k, 17] and 0 <= g < N) or not np.isfinite(kpts[int(g)]).all():
                continue
            cand.append((o, int(g)))
        if len(cand) >= 2:
            pt_act[t] = True
            for o, g in cand:
                obs_act[o], obs_track[o], obs_node[o] = True, t, g
            n_bad += (end - beg) - len(cand)
        else:
            n_bad += end - beg
    cam_obs = np.bincount(obs_image[obs_act], minlength=n_images).astype(np.int32) if n_images else np.zeros(0, np.int32)
    return dict(pt_act=pt_act, obs_act=obs_act, obs_track=obs_track, obs_node=obs_node, cam_obs=cam_obs, n_bad=n_bad, status=status)


# ------------------------------------------------------------------------------------------------ the model
def observe(cams, X, k, uv, jac=True):
    """Residuals, depth and Jacobians of observations: cams [n_images, 18], X [m, 3] the point of every observation, k [m] its image, uv
    [m, 2] its pixel -> ru, rv, z (and Ju [m, 6], Jv [m, 6], Pu [m, 3], Pv [m, 3]).  The association of the header."""
    c = cams[k]
    fx, fy, cx, cy = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    R = c[:, 4:13]
    with np.errstate(all="ignore"):
        y0 = R[:, 0] * X[:, 0] + R[:, 1] * X[:, 1] + R[:, 2] * X[:, 2]
        y1 = R[:, 3] * X[:, 0] + R[:, 4] * X[:, 1] + R[:, 5] * X[:, 2]
        y2 = R[:, 6] * X[:, 0] + R[:, 7] * X[:, 1] + R[:, 8] * X[:, 2]
        x, y, z = y0 + c[:, 13], y1 + c[:, 14], y2 + c[:, 15]
        ru, rv = fx * x / z + cx - uv[:, 0], fy * y / z + cy - uv[:, 1]
        if not jac:
            return ru, rv, z
        au, bu, av, bv = fx / z, -fx * x / (z * z), fy / z, -fy * y / (z * z)
        zero = np.zeros_like(au)
        Ju = np.stack([bu * y1, au * y2 - bu * y0, -au * y1, au, zero, bu], axis=1)
        Jv = np.stack([bv * y1 - av * y2, -bv * y0, av * y0, zero, av, bv], axis=1)
        Pu = np.stack([au * R[:, m] + bu * R[:, 6 + m] for m in range(3)], axis=1)
        Pv = np.stack([av * R[:, 3 + m] + bv * R[:, 6 + m] for m in range(3)], axis=1)
    return ru, rv, z, Ju, Jv, Pu, Pv


def rho(e2, huber):
    if not huber > 0.0:
        return e2
    with np.errstate(all="ignore"):
        e = np.sqrt(e2)
        return np.where(e <= huber, e2, 2.0 * huber * e - huber * huber)


def expmap(w):
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    th = np.sqrt(th2)
    ca, cb = (np.sin(th) / th, (1.0 - np.cos(th)) / th2) if th > 1e-8 else (1.0, 0.5)
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    E = np.zeros((3, 3))
    for i in range(3):
        for m in range(3):
            E[i, m] = (1.0 if i == m else 0.0) + ca * W[i, m] + cb * (W[i, 0] * W[0, m] + W[i, 1] * W[1, m] + W[i, 2] * W[2, m])
    return E


def _by_rank(groups, n_groups, terms, reverse, start=None):
    """Sums of terms [m, ...] per group, the members of a group added one after the other in the order they are listed (from the last to
    the first when reverse).  groups [m]: the group of every term.  start [n_groups, ...]: what the sums start from (default zeros)."""
    out = np.zeros((n_groups,) + terms.shape[1:]) if start is None else start.copy()
    if len(groups) == 0:
        return out
    order = np.argsort(groups, kind="stable")
    g = groups[order]
    first = np.searchsorted(g, g, side="left")
    rank = np.arange(len(g)) - first
    if reverse:
        count = np.bincount(g, minlength=n_groups)
        rank = count[g] - 1 - rank
    for r in range(int(rank.max()) + 1):
        sel = order[rank == r]
        out[groups[sel]] = out[groups[sel]] + terms[sel]
    return out


def _butterfly(v):
    """The sum of the 64 rows of v by the butterfly of a wave (offsets 32 .. 1); every lane ends with the same bits."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lane ^ o]
    return v[0]


def _lane_sum(terms, reverse):
    """terms [cnt, ...]: lane l of 64 adds the terms l, l + 64, ... in order, then the butterfly (reverse: one after the other, last first)."""
    if reverse:
        out = np.zeros(terms.shape[1:])
        for row in terms[::-1]:
            out = out + row
        return out
    part = np.zeros((64,) + terms.shape[1:])
    for i0 in range(0, len(terms), 64):
        chunk = terms[i0:i0 + 64]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    return _butterfly(part)


def total_cost(pt_cost, reverse):
    """The sum of the points' costs: thread j of 256 adds the points j, j + 256, ..., a butterfly per wave, the four waves in order."""
    if reverse:
        out = 0.0
        for v in pt_cost[::-1]:
            out = out + v
        return float(out)
    part = np.zeros(256)
    for i0 in range(0, len(pt_cost), 256):
        chunk = pt_cost[i0:i0 + 256]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    waves = [_butterfly(part[64 * w:64 * w + 64]) for w in range(4)]
    out = waves[0]
    for w in waves[1:]:
        out = out + w
    return float(out)


def cholesky_solve(S, b):
    """S = L L^T in place, then the two substitutions, in the order of the header -> (d, regular, the pivots relative to their entries)."""
    n = len(b)
    S, b = S.copy(), b.copy()
    diag0 = np.diag(S).copy()
    piv = np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(n):
            d = S[j, j]
            if not (np.isfinite(d) and d > 0.0):
                return np.zeros(n), False, piv[:j]
            piv[j] = d / diag0[j] if diag0[j] > 0 else 0.0
            el = np.sqrt(d)
            S[j + 1:, j] = S[j + 1:, j] / el
            S[j, j] = el
            col = S[j + 1:, j]
            S[j + 1:, j + 1:] = S[j + 1:, j + 1:] - col[:, None] * col[None, :]      # (the upper triangle is carried along and never read)
        y = np.zeros(n)
        for j in range(n):
            y[j] = b[j] / S[j, j]
            b[j + 1:] = b[j + 1:] - S[j + 1:, j] * y[j]
        d = np.zeros(n)
        for j in range(n - 1, -1, -1):
            d[j] = y[j] / S[j, j]
            y[:j] = y[:j] - S[j, :j] * d[j]
    return d, True, piv


def _tie_margin(a, b):
    """How far the comparison (float32) a < (float32) b is from changing when a and b move: the relative gap when the two are more than four
    float32 steps apart, else the relative distance of either from the nearest float32 rounding boundary."""
    if not (np.isfinite(a) and np.isfinite(b)):
        return np.inf
    big = max(abs(a), abs(b), 1e-300)
    if abs(a - b) / big > 2.0 ** -21:
        return abs(a - b) / big
    m = np.inf
    for v in (a, b):
        f = np.float32(v)
        for nb in (np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
            m = min(m, abs(v - 0.5 * (float(f) + float(nb))) / big)
    return m


# ------------------------------------------------------------------------------------------------ the op
def adjust(indptr, obs_image, obs_keypoint, obs_use, point_use, kpts, xyz, cams, mode, iters=20, huber=0.0, lambda0=1e-4, order="forward", rounds_out=None):
    indptr, obs_image, obs_keypoint = (np.asarray(x, dtype=np.int64) for x in (indptr, obs_image, obs_keypoint))
    obs_use, point_use = np.asarray(obs_use).astype(bool), np.asarray(point_use).astype(bool)
    kpts = np.asarray(kpts, dtype=np.float32).reshape(-1, 2)
    xyz0 = np.array(xyz, dtype=np.float64).reshape(-1, 3)
    cams0 = np.array(cams, dtype=np.float64).reshape(-1, CAMERA_WORDS)
    mode = np.asarray(mode, dtype=np.int64).reshape(-1)
    T, n_obs, n_images = len(indptr) - 1, len(obs_image), len(cams0)
    huber, lam = float(np.float32(huber)), float(np.float32(lambda0))
    rev = order == "reverse"
    cl = classify(indptr, obs_image, obs_keypoint, obs_use, point_use, kpts, xyz0, cams0, mode)
    slot_cam = np.flatnonzero(mode == 2)
    n_slots = len(slot_cam)
    assert n_slots <= MAX_FREE
    held = cl["cam_obs"][slot_cam] < 4
    slot_of = np.full(n_images, -1, np.int64)
    slot_of[slot_cam[~held]] = np.flatnonzero(~held)
    n = 6 * n_slots
    ao = np.flatnonzero(cl["obs_act"])                                          # the active observations, ascending
    ot, ok_ = cl["obs_track"][ao], obs_image[ao]
    uv = kpts[cl["obs_node"][ao]].astype(np.float64)
    oslot = slot_of[ok_] if len(ao) else np.zeros(0, np.int64)                  # the slot of a moving camera, else -1
    mov = oslot >= 0
    out = dict(xyz=xyz0.copy(), cams=cams0.copy(), obs_error=np.full(n_obs, -1, np.float32), cam_obs=cl["cam_obs"], history=np.zeros((iters + 1, 2)),
               taken=np.zeros(iters, np.uint8), obs_sens=np.zeros(n_obs))
    margins = dict(lead=np.inf, depth=np.inf, pivot=np.inf, det=np.inf)
    stats = dict(n_free=int((~held).sum()), n_fixed=int((mode == 1).sum()), n_held=int(held.sum()), n_points=int(cl["pt_act"].sum()), n_active_obs=len(ao),
                 n_bad_obs=int(cl["n_bad"]), rounds_taken=0, status=cl["status"])

    def cost_of(X, C):
        ru, rv, z = observe(C, X[ot], ok_, uv, jac=False)
        with np.errstate(all="ignore"):
            terms = rho(ru * ru + rv * rv, huber)
        pt = _by_rank(ot, T, terms, rev)
        return total_cost(pt, rev), z

    X, C = xyz0.copy(), cams0.copy()
    status = cl["status"]
    cost, z = cost_of(X, C) if len(ao) else (0.0, np.zeros(0))
    if not status and ((len(z) and not (z > 0).all()) or not np.isfinite(cost)):
        status |= BAD_START
    stats["status"] = status
    if status:
        out["history"][:, 1] = lam
        out.update(stats=stats, margins=margins)
        return out
    if len(z):
        margins["depth"] = float(z.min())
    out["history"][0] = cost, lam
    rejects, stop = 0, False
    for r in range(iters):
        if stop:
            out["history"][r + 1] = cost, lam
            continue
        ru, rv, z, Ju, Jv, Pu, Pv = observe(C, X[ot], ok_, uv)
        if huber > 0.0:
            e = np.sqrt(ru * ru + rv * rv)
            sw = np.where(e > huber, np.sqrt(huber / np.where(e > huber, e, 1.0)), 1.0)
            ru, rv = np.where(e > huber, ru * sw, ru), np.where(e > huber, rv * sw, rv)
            big = (e > huber)[:, None]
            Ju, Jv, Pu, Pv = (np.where(big, J * sw[:, None], J) for J in (Ju, Jv, Pu, Pv))
        tri = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        Vt = np.stack([Pu[:, i] * Pu[:, j] + Pv[:, i] * Pv[:, j] for i, j in tri], axis=1)
        gt = np.stack([Pu[:, m] * ru + Pv[:, m] * rv for m in range(3)], axis=1)
        V, gp = _by_rank(ot, T, Vt, rev), _by_rank(ot, T, gt, rev)
        for d in (0, 3, 5):
            V[:, d] = V[:, d] + lam * np.maximum(V[:, d], 1e-6)
        with np.errstate(all="ignore"):
            c00, c01, c02 = V[:, 3] * V[:, 5] - V[:, 4] * V[:, 4], V[:, 2] * V[:, 4] - V[:, 1] * V[:, 5], V[:, 1] * V[:, 4] - V[:, 2] * V[:, 3]
            c11, c12, c22 = V[:, 0] * V[:, 5] - V[:, 2] * V[:, 2], V[:, 1] * V[:, 2] - V[:, 0] * V[:, 4], V[:, 0] * V[:, 3] - V[:, 1] * V[:, 1]
            det = V[:, 0] * c00 + V[:, 1] * c01 + V[:, 2] * c02
            I = np.stack([c00 / det, c01 / det, c02 / det, c01 / det, c11 / det, c12 / det, c02 / det, c12 / det, c22 / det], axis=1).reshape(-1, 3, 3)
        act = cl["pt_act"]
        regular = bool((np.isfinite(det[act]) & (det[act] > 0)).all())
        if act.any():
            with np.errstate(all="ignore"):
                margins["det"] = min(margins["det"], float((det[act] / (V[act, 0] * V[act, 3] * V[act, 5])).min()))
        d = np.zeros(n)
        Wm = np.zeros((len(ao), 6, 3))
        if n and regular:
            Wm = Ju[:, :, None] * Pu[:, None, :] + Jv[:, :, None] * Pv[:, None, :]
            Io = I[ot]
            Y = Wm[:, :, 0, None] * Io[:, None, 0, :] + Wm[:, :, 1, None] * Io[:, None, 1, :] + Wm[:, :, 2, None] * Io[:, None, 2, :]
            S, b = np.zeros((n, n)), np.zeros(n)
            for s in np.flatnonzero(held):
                S[6 * s:6 * s + 6, 6 * s:6 * s + 6] = np.eye(6)
            for s in np.flatnonzero(~held):
                mine = np.flatnonzero(oslot == s)
                terms = np.concatenate([np.stack([Ju[mine, i] * Ju[mine, j] + Jv[mine, i] * Jv[mine, j] for i in range(6) for j in range(i, 6)], axis=1),
                                        np.stack([Ju[mine, i] * ru[mine] + Jv[mine, i] * rv[mine] for i in range(6)], axis=1)], axis=1)
                tot = _lane_sum(terms, rev)
                U, k = np.zeros((6, 6)), 0
                for i in range(6):
                    for j in range(i, 6):
                        U[i, j] = U[j, i] = tot[k]
                        k += 1
                for i in range(6):
                    U[i, i] = U[i, i] + lam * max(U[i, i], 1e-6)
                S[6 * s:6 * s + 6, 6 * s:6 * s + 6] = U
                b[6 * s:6 * s + 6] = -tot[21:]
            # the block rows: the pairs (o, o') of moving observations of one point, ordered by (slot of o, o, o')
            midx = np.flatnonzero(mov)
            bt = Y[midx, :, 0] * gp[ot[midx], 0, None] + Y[midx, :, 1] * gp[ot[midx], 1, None] + Y[midx, :, 2] * gp[ot[midx], 2, None]
            keys = np.lexsort((midx, oslot[midx]))
            b = _by_rank(oslot[midx][keys], n_slots, bt[keys], rev, start=b.reshape(n_slots, 6)).reshape(n)
            by_track = {}
            for j in midx:
                by_track.setdefault(int(ot[j]), []).append(int(j))
            pa, pb = [], []
            for members in by_track.values():
                for a_ in members:
                    for b_ in members:
                        pa.append(a_)
                        pb.append(b_)
            pa, pb = np.array(pa, np.int64), np.array(pb, np.int64)
            if len(pa):
                keys = np.lexsort((pb, pa, oslot[pa]))
                pa, pb = pa[keys], pb[keys]
                v = (Y[pa][:, :, None, 0] * Wm[pb][:, None, :, 0] + Y[pa][:, :, None, 1] * Wm[pb][:, None, :, 1]) + Y[pa][:, :, None, 2] * Wm[pb][:, None, :, 2]
                blocks = S.reshape(n_slots, 6, n_slots, 6).transpose(0, 2, 1, 3).reshape(n_slots * n_slots, 6, 6)
                blocks = _by_rank(oslot[pa] * n_slots + oslot[pb], n_slots * n_slots, -v, rev, start=blocks)
                S = blocks.reshape(n_slots, n_slots, 6, 6).transpose(0, 2, 1, 3).reshape(n, n)
            if rounds_out is not None:
                rounds_out.append(dict(S=S.copy(), b=b.copy(), V=V.copy(), gp=gp.copy(), lam=lam, Ju=Ju, Jv=Jv, Pu=Pu, Pv=Pv, ru=ru, rv=rv, X=X.copy(), C=C.copy(),
                                       ao=ao, ot=ot, oslot=oslot, held=held))
            d, regular, piv = cholesky_solve(S, b)
            if len(piv):
                margins["pivot"] = min(margins["pivot"], float(piv.min()))
        elif rounds_out is not None:
            rounds_out.append(dict(V=V.copy(), gp=gp.copy(), lam=lam, Ju=Ju, Jv=Jv, Pu=Pu, Pv=Pv, ru=ru, rv=rv, X=X.copy(), C=C.copy(), ao=ao, ot=ot, oslot=oslot, held=held))
        take = False
        if regular:
            s = gp.copy()
            if n:
                midx = np.flatnonzero(mov)
                dc = d.reshape(n_slots, 6)[oslot[midx]]
                # s[m] += W[c][m] d[c]: the observations of a point by rank, c ascending inside an observation
                terms = Wm[midx] * dc[:, :, None]                              # [m, 6, 3]
                order_ = np.argsort(ot[midx], kind="stable")
                g = ot[midx][order_]
                first = np.searchsorted(g, g, side="left")
                rank = np.arange(len(g)) - first
                if rev:
                    rank = np.bincount(g, minlength=T)[g] - 1 - rank
                for rk in range(int(rank.max()) + 1 if len(rank) else 0):
                    sel = order_[rank == rk]
                    for c in (range(5, -1, -1) if rev else range(6)):
                        s[ot[midx][sel]] = s[ot[midx][sel]] + terms[sel, c]
            with np.errstate(all="ignore"):
                dX = -((I[:, :, 0] * s[:, 0, None] + I[:, :, 1] * s[:, 1, None]) + I[:, :, 2] * s[:, 2, None])
            Xc = X.copy()
            Xc[act] = X[act] + dX[act]
            Cc = C.copy()
            for sl in np.flatnonzero(~held):
                k = slot_cam[sl]
                w = d[6 * sl:6 * sl + 6]
                E, Rk = expmap(w[:3]), C[k, 4:13].reshape(3, 3)
                Rn = np.zeros((3, 3))
                for i in range(3):
                    for j in range(3):
                        Rn[i, j] = E[i, 0] * Rk[0, j] + E[i, 1] * Rk[1, j] + E[i, 2] * Rk[2, j]
                Cc[k, 4:13], Cc[k, 13:16] = Rn.reshape(9), C[k, 13:16] + w[3:]
            finite = bool(np.isfinite(Xc[act]).all() and np.isfinite(Cc[slot_cam[~held]]).all())
            cand, zc = cost_of(Xc, Cc)
            front = bool((zc > 0).all())
            if len(zc) and finite:
                margins["depth"] = min(margins["depth"], float(np.abs(zc).min()))
            if finite and front:
                margins["lead"] = min(margins["lead"], _tie_margin(cand, cost))
            take = finite and front and bool(np.isfinite(cand)) and bool(np.float32(cand) < np.float32(cost))
        if take:
            X, C, cost, rejects = Xc, Cc, cand, 0
            lam = max(lam / 10.0, 1e-12)
            stats["rounds_taken"] += 1
        else:
            lam = min(10.0 * lam, 1e12)
            rejects += 1
            stop = rejects >= MAX_REJECTS
        out["history"][r + 1] = cost, lam
        out["taken"][r] = 1 if take else 0
    out["xyz"], out["cams"] = X, C
    if len(ao):
        ru, rv, z, Ju, Jv, Pu, Pv = observe(C, X[ot], ok_, uv)
        err = np.sqrt(ru * ru + rv * rv)
        out["obs_error"][ao] = np.where(z > 0, np.minimum(err, np.finfo(np.float32).max), -1).astype(np.float32)
        scale = max(1.0, float(np.abs(X[cl["pt_act"]]).max()), float(np.abs(C[:, 4:16][mode != 0]).max()))
        out["obs_sens"][ao] = scale * (np.abs(Ju).sum(axis=1) + np.abs(Jv).sum(axis=1) + np.abs(Pu).sum(axis=1) + np.abs(Pv).sum(axis=1))
    out.update(stats=stats, margins=margins)
    return out


# ------------------------------------------------------------------------------------------------ checks of the restatement itself
def residuals(xyz, cams, ao, ot, ok_, uv):
    """The stacked residuals (ru, rv per active observation) at a state, for central differences."""
    ru, rv, _ = observe(cams, xyz[ot], ok_, uv, jac=False)
    return np.stack([ru, rv], axis=1).reshape(-1)


def apply_step(X, C, slot_cam, held, act, dc, dp):
    """The state after the update (dc [n_slots, 6] in the order (w, dt), dp [T, 3])."""
    Xn, Cn = X.copy(), C.copy()
    Xn[act] = X[act] + dp[act]
    for sl in np.flatnonzero(~held):
        k = slot_cam[sl]
        Cn[k, 4:13] = (expmap(dc[sl, :3]) @ C[k, 4:13].reshape(3, 3)).reshape(9)
        Cn[k, 13:16] = C[k, 13:16] + dc[sl, 3:]
    return Xn, Cn


def dense_step(rd, T, n_slots):
    """The step of one round from the full damped normal equations, by a dense solve without the Schur complement -> (dc [n_slots, 6],
    dp [T, 3]) for the round record rd of adjust(rounds_out=...)."""
    Ju, Jv, Pu, Pv, ru, rv, ot, oslot, lam = (rd[k] for k in ("Ju", "Jv", "Pu", "Pv", "ru", "rv", "ot", "oslot", "lam"))
    nc, npt = 6 * n_slots, 3 * T
    H, g = np.zeros((nc + npt, nc + npt)), np.zeros(nc + npt)
    for j in range(len(ot)):
        rows = np.zeros((2, nc + npt))
        if oslot[j] >= 0:
            rows[0, 6 * oslot[j]:6 * oslot[j] + 6], rows[1, 6 * oslot[j]:6 * oslot[j] + 6] = Ju[j], Jv[j]
        rows[0, nc + 3 * ot[j]:nc + 3 * ot[j] + 3], rows[1, nc + 3 * ot[j]:nc + 3 * ot[j] + 3] = Pu[j], Pv[j]
        H += rows.T @ rows
        g += rows.T @ np.array([ru[j], rv[j]])
    used = np.flatnonzero(np.diag(H) > 0)
    Hd = H[np.ix_(used, used)]
    Hd = Hd + lam * np.diag(np.maximum(np.diag(Hd), 1e-6))
    step = np.zeros(nc + npt)
    step[used] = np.linalg.solve(Hd, -g[used])
    return step[:nc].reshape(n_slots, 6), step[nc:].reshape(T, 3)


# ------------------------------------------------------------------------------------------------ planted scenes
def rot(w):
    return expmap(np.asarray(w, dtype=np.float64))


def planted_scene(seed, lengths, n_cams, noise=0.5, fixed=(0, 1), pert_cam=0.0, pert_pt=0.0, span=np.pi):
    """Tracks of the given lengths over n_cams arc cameras (TR.planted_tracks without wrong matches), the cameras outside `fixed` turned by
    pert_cam radians and moved by pert_cam, the points moved by pert_pt (uniform in [-1, 1] times that).
    -> dict(indptr, obs_image, obs_keypoint, obs_use, point_use, kpts, xyz (the start), cams (the start), mode, planted_xyz, planted_cams, counts)."""
    sc = TR.planted_tracks(seed, lengths, n_cams=n_cams, noise=noise, p_wrong=0.0)
    rng = np.random.default_rng(seed + 77)
    cams = sc["cams"].copy()
    mode = np.full(n_cams, 2, np.int32)
    mode[list(fixed)] = 1
    for k in range(n_cams):
        if mode[k] == 2 and pert_cam > 0:
            E = rot(pert_cam * rng.uniform(-1, 1, 3))
            cams[k, 4:13] = (E @ cams[k, 4:13].reshape(3, 3)).reshape(9)
            cams[k, 13:16] = cams[k, 13:16] + pert_cam * rng.uniform(-1, 1, 3)
    xyz = sc["points"] + pert_pt * rng.uniform(-1, 1, sc["points"].shape)
    n_obs, T = len(sc["obs_image"]), len(lengths)
    return dict(indptr=sc["indptr"], obs_image=sc["obs_image"], obs_keypoint=sc["obs_keypoint"], obs_use=np.ones(n_obs, np.uint8), point_use=np.ones(T, np.uint8),
                kpts=sc["kpts"], xyz=xyz, cams=cams, mode=mode, planted_xyz=sc["points"], planted_cams=sc["cams"], counts=sc["counts"])


ARGS = ("indptr", "obs_image", "obs_keypoint", "obs_use", "point_use", "kpts", "xyz", "cams", "mode")


def run(sc, **kw):
    return adjust(*(sc[k] for k in ARGS), **kw)


def errors(out, sc):
    """The largest |X - planted|, |R - planted|, |t - planted| over the active points and the posed cameras."""
    posed = sc["mode"] != 0
    pc = sc["planted_cams"]
    return (float(np.abs(out["xyz"] - sc["planted_xyz"]).max()), float(np.abs(out["cams"][posed, 4:13] - pc[posed, 4:13]).max()),
            float(np.abs(out["cams"][posed, 13:16] - pc[posed, 13:16]).max()))
