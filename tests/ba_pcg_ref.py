"""NumPy float64 restatement of GIMS_AUX_BUNDLE_ADJUST_PCG, written from the specification in include/gims_hip.h (not from the kernel).

The model, the activity rules, the Levenberg-Marquardt schedule and the helpers are those of tests/ba_ref.py, which this file imports and
does not change; what is restated here is the round's camera step: preconditioned conjugate gradients on the Schur complement, applied
matrix-free, with the block-Jacobi preconditioner M.  ``adjust`` performs the operations one at a time in the association and order of
the header (``order='forward'``); ``order='reverse'`` takes every sum over observations, over the slots of a dot product and over the
points' costs from the last term to the first, and the c of the point sums descending: the difference between the two is the
restatement's own sensitivity to summation order, from which the tests derive TOL_PCG.

The result carries ``cg_used`` and ``cg_res`` next to the outputs of ba_ref.adjust, and ``margins`` gains ``cg_stop`` (every stop
comparison rho' <= cg_tol^2 rho_0, relative to the larger side), ``pq`` (every p . q relative to the sum of the magnitudes of its
products) and ``m_pivot`` (every pivot of every M_s relative to the diagonal entry it started as)."""
import numpy as np

from tests import ba_ref as B

MAX_FREE, MAX_CG_ITERS = 65536, 256
TRI = [(i, j) for i in range(6) for j in range(i, 6)]                                # the upper triangle by rows


def out_layout(T, n_obs, n_images, iters, n_free):
    """The byte offsets of the op's buffer by the formula of the header."""
    al = lambda x: (x + 255) & ~255      # noqa: E731
    sizes = [("xyz", 24 * T), ("cams", 144 * n_images), ("obs_error", 4 * n_obs), ("cam_obs", 4 * n_images), ("history", 16 * (iters + 1)), ("taken", iters),
             ("counters", 32), ("cg_used", 4 * iters), ("cg_res", 8 * iters)]
    off, at = {}, 0
    for name, size in sizes:
        off[name] = at
        at += al(size)
    off["outputs"] = off["scratch"] = at
    scratch = [256, 4 * n_images, 4 * n_free, 4 * n_free + 4, 4 * n_free, 4 * n_free, 24 * T, 144 * n_images, T, n_obs, 4 * n_obs, 4 * n_obs, 4 * n_obs, 4 * n_obs, 72 * T,
               400 * n_obs, 8 * T, 24 * T, 336 * n_free] + [48 * n_free] * 5
    off["bytes"] = at + sum(al(s) for s in scratch)
    return off


class _Sums:
    """The fixed summation orders of one call: the lists of the slots and the moving observations of the points do not change."""

    def __init__(self, ot, oslot, T, n_slots, rev):
        self.T, self.n_slots, self.rev = T, n_slots, rev
        self.midx = np.flatnonzero(oslot >= 0)                                      # the observations whose camera moves, ascending in o
        self.mslot, self.mtrack = oslot[self.midx], ot[self.midx]
        # the slot's order: place number l of the slot's list (ascending o) belongs to lane l % 64
        order = np.argsort(self.mslot, kind="stable")
        place = np.zeros(len(self.midx), np.int64)
        g = self.mslot[order]
        place[order] = np.arange(len(g)) - np.searchsorted(g, g, side="left")
        self.lane_group = self.mslot * 64 + place % 64
        # the point's order: rank of the moving observation inside its track
        order = np.argsort(self.mtrack, kind="stable")
        g = self.mtrack[order]
        rank = np.arange(len(g)) - np.searchsorted(g, g, side="left")
        if rev and len(g):
            rank = np.bincount(g, minlength=T)[g] - 1 - rank
        self.t_order, self.t_rank = order, rank

    def slots(self, terms):
        """terms [m, k] per moving observation -> [n_slots, k]: lane l adds its places l, l + 64, ... in order, then the butterfly."""
        if self.rev:
            return B._by_rank(self.mslot, self.n_slots, terms, True)
        part = B._by_rank(self.lane_group, self.n_slots * 64, terms, False).reshape(self.n_slots, 64, -1)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            part = part + part[:, lane ^ o]
        return part[:, 0]

    def points(self, terms):
        """terms [m, 6, 3] per moving observation -> s [T, 3]: the observations of a point by rank, c ascending inside an observation."""
        return _points_from(self, np.zeros((self.T, 3)), terms)

    def dot(self, v, w):
        """v . w over [n_slots, 6]: per slot ((((v0 w0 + v1 w1) + v2 w2) + ...) + v5 w5, the slots by the scheme of the cost."""
        d = v[:, 0] * w[:, 0]
        for c in range(1, 6):
            d = d + v[:, c] * w[:, c]
        return B.total_cost(d, self.rev)


def cholesky6(M):
    """M [n_slots, 6, 6] -> (L in the lower triangles, the pivots relative to their entries [n_slots, 6], regular): the Cholesky of the header."""
    L = M.copy()
    diag0 = np.stack([M[:, j, j] for j in range(6)], axis=1)
    piv = np.zeros((len(M), 6))
    regular = True
    with np.errstate(all="ignore"):
        for j in range(6):
            d = L[:, j, j].copy()
            regular = regular and bool((np.isfinite(d) & (d > 0)).all())
            piv[:, j] = np.where(diag0[:, j] > 0, d / diag0[:, j], 0.0)
            el = np.sqrt(d)
            L[:, j, j] = el
            for i in range(j + 1, 6):
                L[:, i, j] = L[:, i, j] / el
            for i in range(j + 1, 6):
                for k in range(j + 1, i + 1):
                    L[:, i, k] = L[:, i, k] - L[:, i, j] * L[:, k, j]
    return L, piv, regular


def msolve(L, r):
    """z = M^-1 r per slot from the factor: L y = r by columns, L^T z = y by rows."""
    b, y, z = r.copy(), np.zeros_like(r), np.zeros_like(r)
    with np.errstate(all="ignore"):
        for j in range(6):
            y[:, j] = b[:, j] / L[:, j, j]
            for i in range(j + 1, 6):
                b[:, i] = b[:, i] - L[:, i, j] * y[:, j]
        for j in range(5, -1, -1):
            z[:, j] = y[:, j] / L[:, j, j]
            for k in range(j):
                y[:, k] = y[:, k] - L[:, j, k] * z[:, j]
    return z


def round_system(sums, held, lam, Ju, Jv, ru, rv, Wm, Y, I, gp):
    """U*, b, M of one round and the product v -> S v -> dict(U [n_slots, 6, 6], b [n_slots, 6], M [n_slots, 6, 6], Sp)."""
    n_slots, mi = sums.n_slots, sums.midx
    with np.errstate(all="ignore"):
        terms = np.concatenate([np.stack([Ju[mi, i] * Ju[mi, j] + Jv[mi, i] * Jv[mi, j] for i, j in TRI], axis=1),
                                np.stack([Ju[mi, i] * ru[mi] + Jv[mi, i] * rv[mi] for i in range(6)], axis=1)], axis=1)
        tot = sums.slots(terms)
        g0, g1, g2 = (gp[sums.mtrack, m] for m in range(3))
        more = np.concatenate([np.stack([(Y[mi, i, 0] * Wm[mi, j, 0] + Y[mi, i, 1] * Wm[mi, j, 1]) + Y[mi, i, 2] * Wm[mi, j, 2] for i, j in TRI], axis=1),
                               np.stack([(Y[mi, i, 0] * g0 + Y[mi, i, 1] * g1) + Y[mi, i, 2] * g2 for i in range(6)], axis=1)], axis=1)
        tot2 = sums.slots(more)
    U, M = np.zeros((n_slots, 6, 6)), np.zeros((n_slots, 6, 6))
    for k, (i, j) in enumerate(TRI):
        u = tot[:, k]
        if i == j:
            u = u + lam * np.maximum(u, 1e-6)
        U[:, i, j] = U[:, j, i] = u
        M[:, i, j] = M[:, j, i] = u - tot2[:, k]
    b = -tot[:, 21:] + tot2[:, 21:]
    U[held], M[held], b[held] = np.eye(6), np.eye(6), 0.0

    def Sp(v):
        with np.errstate(all="ignore"):
            s = sums.points(Wm[mi] * v[sums.mslot][:, :, None])
            y = (I[:, :, 0] * s[:, 0, None] + I[:, :, 1] * s[:, 1, None]) + I[:, :, 2] * s[:, 2, None]
            yo = y[sums.mtrack]
            wy = sums.slots(np.stack([(Wm[mi, r, 0] * yo[:, 0] + Wm[mi, r, 1] * yo[:, 1]) + Wm[mi, r, 2] * yo[:, 2] for r in range(6)], axis=1))
            up = U[:, :, 0] * v[:, 0, None]
            for c in range(1, 6):
                up = up + U[:, :, c] * v[:, c, None]
        return up - wy

    return dict(U=U, b=b, M=M, Sp=Sp)


def pcg(sys_, sums, cg_iters, tol2, margins):
    """-> (d [n_slots, 6], regular, cg_used, cg_res) by the iteration of the header."""
    n_slots = sums.n_slots
    zero = np.zeros((n_slots, 6))
    L, piv, regular = cholesky6(sys_["M"])
    if len(piv):
        margins["m_pivot"] = min(margins["m_pivot"], float(piv.min()))
    if not regular:
        return zero, False, 0, 0.0
    x, r = zero.copy(), sys_["b"].copy()
    z = msolve(L, r)
    p = z.copy()
    rho0 = rho = sums.dot(r, z)
    if not (np.isfinite(rho0) and rho0 >= 0.0):
        return zero, False, 0, 0.0
    if rho0 == 0.0:
        return zero, True, 0, 0.0
    used = 0
    with np.errstate(all="ignore"):
        for it in range(1, cg_iters + 1):
            q = sys_["Sp"](p)
            pq = sums.dot(p, q)
            used += 1
            if not (np.isfinite(pq) and pq > 0.0):
                return zero, False, used, 0.0
            margins["pq"] = min(margins["pq"], pq / max(float(np.abs(p * q).sum()), 1e-300))
            alpha = rho / pq
            x = x + alpha * p
            r = r - alpha * q
            z = msolve(L, r)
            rho1 = sums.dot(r, z)
            if not (np.isfinite(rho1) and rho1 >= 0.0):
                return zero, False, used, 0.0
            thr = tol2 * rho0
            margins["cg_stop"] = min(margins["cg_stop"], abs(rho1 - thr) / max(rho1, thr, 1e-300))
            if rho1 <= thr or it == cg_iters:
                rho = rho1
                break
            p = z + (rho1 / rho) * p
            rho = rho1
    return x, True, used, float(np.sqrt(rho / rho0))


# ------------------------------------------------------------------------------------------------ the op
def adjust(indptr, obs_image, obs_keypoint, obs_use, point_use, kpts, xyz, cams, mode, iters=20, huber=0.0, lambda0=1e-4, cg_iters=64, cg_tol=1e-6,
           order="forward", rounds_out=None):
    indptr, obs_image, obs_keypoint = (np.asarray(x, dtype=np.int64) for x in (indptr, obs_image, obs_keypoint))
    obs_use, point_use = np.asarray(obs_use).astype(bool), np.asarray(point_use).astype(bool)
    kpts = np.asarray(kpts, dtype=np.float32).reshape(-1, 2)
    xyz0 = np.array(xyz, dtype=np.float64).reshape(-1, 3)
    cams0 = np.array(cams, dtype=np.float64).reshape(-1, B.CAMERA_WORDS)
    mode = np.asarray(mode, dtype=np.int64).reshape(-1)
    T, n_obs, n_images = len(indptr) - 1, len(obs_image), len(cams0)
    huber, lam = float(np.float32(huber)), float(np.float32(lambda0))
    cg_tol = float(cg_tol)
    assert 1 <= cg_iters <= MAX_CG_ITERS and np.isfinite(cg_tol) and 0.0 <= cg_tol < 1.0
    tol2 = cg_tol * cg_tol
    rev = order == "reverse"
    cl = B.classify(indptr, obs_image, obs_keypoint, obs_use, point_use, kpts, xyz0, cams0, mode)
    slot_cam = np.flatnonzero(mode == 2)
    n_slots = len(slot_cam)
    assert n_slots <= MAX_FREE
    held = cl["cam_obs"][slot_cam] < 4
    slot_of = np.full(n_images, -1, np.int64)
    slot_of[slot_cam[~held]] = np.flatnonzero(~held)
    ao = np.flatnonzero(cl["obs_act"])                                          # the active observations, ascending
    ot, ok_ = cl["obs_track"][ao], obs_image[ao]
    uv = kpts[cl["obs_node"][ao]].astype(np.float64)
    oslot = slot_of[ok_] if len(ao) else np.zeros(0, np.int64)                  # the slot of a moving camera, else -1
    sums = _Sums(ot, oslot, T, n_slots, rev)
    out = dict(xyz=xyz0.copy(), cams=cams0.copy(), obs_error=np.full(n_obs, -1, np.float32), cam_obs=cl["cam_obs"], history=np.zeros((iters + 1, 2)),
               taken=np.zeros(iters, np.uint8), obs_sens=np.zeros(n_obs), cg_used=np.zeros(iters, np.int32), cg_res=np.zeros(iters))
    margins = dict(lead=np.inf, depth=np.inf, det=np.inf, m_pivot=np.inf, pq=np.inf, cg_stop=np.inf)
    stats = dict(n_free=int((~held).sum()), n_fixed=int((mode == 1).sum()), n_held=int(held.sum()), n_points=int(cl["pt_act"].sum()), n_active_obs=len(ao),
                 n_bad_obs=int(cl["n_bad"]), rounds_taken=0, status=cl["status"])

    def cost_of(X, C):
        ru, rv, z = B.observe(C, X[ot], ok_, uv, jac=False)
        with np.errstate(all="ignore"):
            terms = B.rho(ru * ru + rv * rv, huber)
        return B.total_cost(B._by_rank(ot, T, terms, rev), rev), z

    X, C = xyz0.copy(), cams0.copy()
    status = cl["status"]
    cost, z = cost_of(X, C) if len(ao) else (0.0, np.zeros(0))
    if not status and ((len(z) and not (z > 0).all()) or not np.isfinite(cost)):
        status |= B.BAD_START
    stats["status"] = status
    if status:
        out["history"][:, 1] = lam
        out.update(stats=stats, margins=margins)
        return out
    if len(z):
        margins["depth"] = float(z.min())
    out["history"][0] = cost, lam
    rejects, stop = 0, False
    act = cl["pt_act"]
    for r in range(iters):
        if stop:
            out["history"][r + 1] = cost, lam
            continue
        ru, rv, z, Ju, Jv, Pu, Pv = B.observe(C, X[ot], ok_, uv)
        if huber > 0.0:
            e = np.sqrt(ru * ru + rv * rv)
            sw = np.where(e > huber, np.sqrt(huber / np.where(e > huber, e, 1.0)), 1.0)
            ru, rv = np.where(e > huber, ru * sw, ru), np.where(e > huber, rv * sw, rv)
            big = (e > huber)[:, None]
            Ju, Jv, Pu, Pv = (np.where(big, J * sw[:, None], J) for J in (Ju, Jv, Pu, Pv))
        tri = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        Vt = np.stack([Pu[:, i] * Pu[:, j] + Pv[:, i] * Pv[:, j] for i, j in tri], axis=1)
        gt = np.stack([Pu[:, m] * ru + Pv[:, m] * rv for m in range(3)], axis=1)
        V, gp = B._by_rank(ot, T, Vt, rev), B._by_rank(ot, T, gt, rev)
        for d_ in (0, 3, 5):
            V[:, d_] = V[:, d_] + lam * np.maximum(V[:, d_], 1e-6)
        with np.errstate(all="ignore"):
            c00, c01, c02 = V[:, 3] * V[:, 5] - V[:, 4] * V[:, 4], V[:, 2] * V[:, 4] - V[:, 1] * V[:, 5], V[:, 1] * V[:, 4] - V[:, 2] * V[:, 3]
            c11, c12, c22 = V[:, 0] * V[:, 5] - V[:, 2] * V[:, 2], V[:, 1] * V[:, 2] - V[:, 0] * V[:, 4], V[:, 0] * V[:, 3] - V[:, 1] * V[:, 1]
            det = V[:, 0] * c00 + V[:, 1] * c01 + V[:, 2] * c02
            I = np.stack([c00 / det, c01 / det, c02 / det, c01 / det, c11 / det, c12 / det, c02 / det, c12 / det, c22 / det], axis=1).reshape(-1, 3, 3)
        regular = bool((np.isfinite(det[act]) & (det[act] > 0)).all())
        if act.any():
            with np.errstate(all="ignore"):
                margins["det"] = min(margins["det"], float((det[act] / (V[act, 0] * V[act, 3] * V[act, 5])).min()))
        d = np.zeros((n_slots, 6))
        Wm = np.zeros((len(ao), 6, 3))
        if n_slots and regular:
            with np.errstate(all="ignore"):
                Wm = Ju[:, :, None] * Pu[:, None, :] + Jv[:, :, None] * Pv[:, None, :]
                Io = I[ot]
                Y = Wm[:, :, 0, None] * Io[:, None, 0, :] + Wm[:, :, 1, None] * Io[:, None, 1, :] + Wm[:, :, 2, None] * Io[:, None, 2, :]
            sys_ = round_system(sums, held, lam, Ju, Jv, ru, rv, Wm, Y, I, gp)
            if rounds_out is not None:
                rounds_out.append(dict(sys_, lam=lam, oslot=oslot, held=held, ot=ot))
            d, regular, out["cg_used"][r], out["cg_res"][r] = pcg(sys_, sums, cg_iters, tol2, margins)
        take = False
        if regular:
            s = _points_from(sums, gp, Wm[sums.midx] * d[sums.mslot][:, :, None]) if n_slots else gp.copy()
            with np.errstate(all="ignore"):
                dX = -((I[:, :, 0] * s[:, 0, None] + I[:, :, 1] * s[:, 1, None]) + I[:, :, 2] * s[:, 2, None])
            Xc = X.copy()
            Xc[act] = X[act] + dX[act]
            Cc = C.copy()
            for sl in np.flatnonzero(~held):
                k = slot_cam[sl]
                w = d[sl]
                E, Rk = B.expmap(w[:3]), C[k, 4:13].reshape(3, 3)
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
                margins["lead"] = min(margins["lead"], B._tie_margin(cand, cost))
            take = finite and front and bool(np.isfinite(cand)) and bool(np.float32(cand) < np.float32(cost))
        if take:
            X, C, cost, rejects = Xc, Cc, cand, 0
            lam = max(lam / 10.0, 1e-12)
            stats["rounds_taken"] += 1
        else:
            lam = min(10.0 * lam, 1e12)
            rejects += 1
            stop = rejects >= B.MAX_REJECTS
        out["history"][r + 1] = cost, lam
        out["taken"][r] = 1 if take else 0
    out["xyz"], out["cams"] = X, C
    if len(ao):
        ru, rv, z, Ju, Jv, Pu, Pv = B.observe(C, X[ot], ok_, uv)
        err = np.sqrt(ru * ru + rv * rv)
        out["obs_error"][ao] = np.where(z > 0, np.minimum(err, np.finfo(np.float32).max), -1).astype(np.float32)
        scale = max(1.0, float(np.abs(X[cl["pt_act"]]).max()), float(np.abs(C[:, 4:16][mode != 0]).max()))
        out["obs_sens"][ao] = scale * (np.abs(Ju).sum(axis=1) + np.abs(Jv).sum(axis=1) + np.abs(Pu).sum(axis=1) + np.abs(Pv).sum(axis=1))
    out.update(stats=stats, margins=margins)
    return out


def _points_from(sums, start, terms):
    """The back substitution's sum: s = g_p, then the moving observations of the point by rank, c ascending inside an observation."""
    s = start.copy()
    for rk in range(int(sums.t_rank.max()) + 1 if len(sums.t_rank) else 0):
        sel = sums.t_order[sums.t_rank == rk]
        for c in (range(5, -1, -1) if sums.rev else range(6)):
            s[sums.mtrack[sel]] = s[sums.mtrack[sel]] + terms[sel, c]
    return s


def run(sc, **kw):
    return adjust(*(sc[k] for k in B.ARGS), **kw)
