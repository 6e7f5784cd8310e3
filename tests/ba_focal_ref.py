"""NumPy float64 restatement of GIMS_AUX_BUNDLE_ADJUST_FOCAL, written from the specification in include/gims_hip.h (not from the kernel).

The model, the activity rules and the Levenberg-Marquardt schedule are those of tests/ba_ref.py, the slot part of a round's system (U*, b,
M_s, the Cholesky of M_s) is that of tests/ba_pcg_ref.py; both are imported and not changed.  What is restated here is what a focal group
adds: the Jacobian words Fu, Fv and G of an observation, A*, b_g, M_g and C_s, the product S v, the dot products and the iteration on the
unknowns [6 words per slot | 1 word per group], the back-substitution with the group term and the multiplicative update of fx, fy.

``order='forward'`` takes every sum in the association and order of the header; ``order='reverse'`` takes every sum over observations,
over the images of a group, over the slots and the groups of a dot product and over the points' costs from the last term to the first
(and inside an observation the group term before the camera term, c descending): the difference between the two is the restatement's own
sensitivity to summation order, from which the tests derive TOL_FOCAL.

The result carries ``focal_scale`` and ``group_obs`` next to the outputs of ba_pcg_ref.adjust, and ``margins`` gains ``mg_pivot`` (every
M_g relative to its A*_g) and ``f1`` (the smallest |1 + ds| of a candidate: how far the comparison 1 + ds <= 0 is from changing)."""
import numpy as np

from tests import ba_pcg_ref as P
from tests import ba_ref as B


def out_layout(T, n_obs, n_images, iters, n_free, n_groups):
    """The byte offsets of the op's buffer by the formula of the header."""
    al = lambda x: (x + 255) & ~255      # noqa: E731
    sizes = [("xyz", 24 * T), ("cams", 144 * n_images), ("obs_error", 4 * n_obs), ("cam_obs", 4 * n_images), ("history", 16 * (iters + 1)), ("taken", iters),
             ("counters", 32), ("cg_used", 4 * iters), ("cg_res", 8 * iters), ("focal_scale", 8 * n_groups), ("group_obs", 4 * n_groups)]
    off, at = {}, 0
    for name, size in sizes:
        off[name] = at
        at += al(size)
    off["outputs"] = off["scratch"] = at
    scratch = ([256, 4 * n_images, 4 * n_images, 4 * n_images + 4, 4 * n_free, 4 * n_images, 24 * T, 144 * n_images, T, n_obs] + [4 * n_obs] * 4
               + [72 * T, 400 * n_obs, 8 * T, 24 * T, 336 * n_free] + [48 * n_free] * 6 + [4 * n_images] * 3 + [32 * n_images, 16 * n_images, 64 * n_obs,
                                                                                                                 4 * n_groups + 4, 4 * n_groups, 8 * n_groups, 16 * n_groups]
               + [8 * n_groups] * 5)
    off["bytes"] = at + sum(al(s) for s in scratch)
    return off


def focal_words(cams, X, k):
    """Fu = fx x_c[0] / z, Fv = fy x_c[1] / z of observations (before the Huber factor), in the association of the residual."""
    c = cams[k]
    R = c[:, 4:13]
    with np.errstate(all="ignore"):
        x = (R[:, 0] * X[:, 0] + R[:, 1] * X[:, 1] + R[:, 2] * X[:, 2]) + c[:, 13]
        y = (R[:, 3] * X[:, 0] + R[:, 4] * X[:, 1] + R[:, 5] * X[:, 2]) + c[:, 14]
        z = (R[:, 6] * X[:, 0] + R[:, 7] * X[:, 1] + R[:, 8] * X[:, 2]) + c[:, 15]
        return c[:, 0] * x / z, c[:, 1] * y / z


class _PointSums:
    """The sums of a point over its active observations in ascending o: per observation the camera term (c ascending) when its camera
    moves, then the group term when its group moves."""

    def __init__(self, ot, oslot, ogrp, rev):
        self.ot, self.oslot, self.ogrp, self.rev = ot, oslot, ogrp, rev
        idx = np.flatnonzero((oslot >= 0) | (ogrp >= 0))
        order = np.argsort(ot[idx], kind="stable")
        g = ot[idx][order]
        rank = np.arange(len(g)) - np.searchsorted(g, g, side="left")
        if rev and len(g):
            rank = np.bincount(g)[g] - 1 - rank
        self.by_rank = [idx[order[rank == r]] for r in range(int(rank.max()) + 1 if len(rank) else 0)]

    def run(self, start, cam_terms, grp_terms):
        """start [T, 3]; cam_terms [m, 6, 3] and grp_terms [m, 3] per active observation (read where the camera / the group moves)."""
        s = start.copy()
        for sel in self.by_rank:
            cam, grp = sel[self.oslot[sel] >= 0], sel[self.ogrp[sel] >= 0]
            for part in (("g", "c") if self.rev else ("c", "g")):
                if part == "c":
                    for c in (range(5, -1, -1) if self.rev else range(6)):
                        s[self.ot[cam]] = s[self.ot[cam]] + cam_terms[cam, c]
                else:
                    s[self.ot[grp]] = s[self.ot[grp]] + grp_terms[grp]
        return s


def _dot6(v, w):
    d = v[:, 0] * w[:, 0]
    for c in range(1, 6):
        d = d + v[:, c] * w[:, c]
    return d


def round_system(ctx, lam, Ju, Jv, ru, rv, Pu, Pv, Fu, Fv, I, gp):
    """The system of one round -> dict(U, b, M (the slots, of ba_pcg_ref), As, bg, Mg [n_groups], Cs [n_slots, 6], G, Wm, Sp, dot)."""
    sums, isums, psums, rev = ctx["sums"], ctx["isums"], ctx["psums"], ctx["rev"]
    ot, oslot, ogrp, held, gheld, slot_cam, mgroup = (ctx[k] for k in ("ot", "oslot", "ogrp", "held", "gheld", "slot_cam", "mgroup"))
    n_slots, n_groups, n_images = len(held), len(gheld), len(mgroup)
    with np.errstate(all="ignore"):
        Wm = Ju[:, :, None] * Pu[:, None, :] + Jv[:, :, None] * Pv[:, None, :]
        Io = I[ot]
        Y = Wm[:, :, 0, None] * Io[:, None, 0, :] + Wm[:, :, 1, None] * Io[:, None, 1, :] + Wm[:, :, 2, None] * Io[:, None, 2, :]
        G = Fu[:, None] * Pu + Fv[:, None] * Pv
        GI = np.stack([(G[:, 0] * Io[:, 0, m] + G[:, 1] * Io[:, 1, m]) + G[:, 2] * Io[:, 2, m] for m in range(3)], axis=1)
    slot_sys = (P.round_system(sums, held, lam, Ju, Jv, ru, rv, Wm, Y, I, gp) if n_slots else
                dict(U=np.zeros((0, 6, 6)), b=np.zeros((0, 6)), M=np.zeros((0, 6, 6))))      # (poses fixed: the groups alone)
    gi = isums.midx
    gpo = gp[ot]
    with np.errstate(all="ignore"):
        terms = np.stack([Fu[gi] * Fu[gi] + Fv[gi] * Fv[gi], Fu[gi] * ru[gi] + Fv[gi] * rv[gi],
                          (GI[gi, 0] * G[gi, 0] + GI[gi, 1] * G[gi, 1]) + GI[gi, 2] * G[gi, 2],
                          (GI[gi, 0] * gpo[gi, 0] + GI[gi, 1] * gpo[gi, 1]) + GI[gi, 2] * gpo[gi, 2]]
                         + [Ju[gi, c] * Fu[gi] + Jv[gi, c] * Fv[gi] for c in range(6)], axis=1)
        ipart = isums.slots(terms)                                                  # [n_images, 10]
    As, Mg, bg = np.ones(n_groups), np.ones(n_groups), np.zeros(n_groups)
    for g in np.flatnonzero(~gheld):
        imgs = ctx["gimgs"][g]
        A, gg, E, Bs = (B.total_cost(ipart[imgs, j], rev) for j in range(4))
        with np.errstate(all="ignore"):
            As[g] = A + lam * max(A, 1e-6)
            Mg[g], bg[g] = As[g] - E, -gg + Bs
    coupled = np.array([(not held[s]) and mgroup[slot_cam[s]] >= 0 for s in range(n_slots)], bool)      # the slot moves and so does its group
    sgrp = np.where(coupled, mgroup[slot_cam], 0) if n_slots else np.zeros(0, np.int64)
    Cs = np.zeros((n_slots, 6))
    Cs[coupled] = ipart[slot_cam[coupled], 4:]
    U = slot_sys["U"]
    mi = sums.midx
    cam_img = np.zeros(n_images, bool)
    cam_img[slot_cam[coupled]] = True

    def Sp(vs, vg):
        with np.errstate(all="ignore"):
            cam_terms = np.zeros((len(ot), 6, 3))
            cam_terms[mi] = Wm[mi] * vs[sums.mslot][:, :, None]
            grp_terms = G * np.where(ogrp >= 0, vg[np.maximum(ogrp, 0)], 0.0)[:, None] if n_groups else np.zeros((len(ot), 3))
            s = psums.run(np.zeros((ctx["T"], 3)), cam_terms, grp_terms)
            y = (I[:, :, 0] * s[:, 0, None] + I[:, :, 1] * s[:, 1, None]) + I[:, :, 2] * s[:, 2, None]
            yo = y[ot]
            wy = np.zeros((0, 6)) if n_slots == 0 else sums.slots(np.stack([(Wm[mi, r, 0] * yo[mi, 0] + Wm[mi, r, 1] * yo[mi, 1]) + Wm[mi, r, 2] * yo[mi, 2] for r in range(6)], axis=1))
            up = U[:, :, 0] * vs[:, 0, None]
            for c in range(1, 6):
                up = up + U[:, :, c] * vs[:, c, None]
            up[coupled] = up[coupled] + Cs[coupled] * vg[sgrp[coupled]][:, None]
            qs = up - wy
            gy = isums.slots(((G[gi, 0] * yo[gi, 0] + G[gi, 1] * yo[gi, 1]) + G[gi, 2] * yo[gi, 2])[:, None])[:, 0]      # [n_images]
            cs = np.zeros(n_images)
            cs[slot_cam[coupled]] = _dot6(Cs[coupled], vs[coupled])
            qg = vg.copy()
            for g in np.flatnonzero(~gheld):
                imgs = ctx["gimgs"][g]
                qg[g] = (As[g] * vg[g] + B.total_cost(cs[imgs], rev)) - B.total_cost(gy[imgs], rev)
        return qs, qg

    def dot(vs, vg, ws, wg):
        with np.errstate(all="ignore"):
            return sums.dot(vs, ws) + B.total_cost(vg * wg, rev)

    return dict(slot_sys, As=As, bg=bg, Mg=Mg, Cs=Cs, G=G, Wm=Wm, Sp=Sp, dot=dot)


def pcg(sys_, ctx, cg_iters, tol2, margins):
    """-> (d [n_slots, 6], ds [n_groups], regular, cg_used, cg_res) by the iteration of the header."""
    n_slots, gheld = len(ctx["held"]), ctx["gheld"]
    zs, zg = np.zeros((n_slots, 6)), np.zeros(len(gheld))
    L, piv, regular = P.cholesky6(sys_["M"])
    if len(piv):
        margins["m_pivot"] = min(margins["m_pivot"], float(piv.min()))
    Mg = sys_["Mg"]
    regular = regular and bool((np.isfinite(Mg) & (Mg > 0)).all())
    if (~gheld).any():
        with np.errstate(all="ignore"):
            margins["mg_pivot"] = min(margins["mg_pivot"], float((Mg / sys_["As"])[~gheld].min()))
    if not regular:
        return zs, zg, False, 0, 0.0
    dot, Sp = sys_["dot"], sys_["Sp"]
    xs, xg, rs, rg = zs.copy(), zg.copy(), sys_["b"].copy(), sys_["bg"].copy()
    with np.errstate(all="ignore"):
        z_s, z_g = P.msolve(L, rs), rg / Mg
    ps, pg = z_s.copy(), z_g.copy()
    rho0 = rho = dot(rs, rg, z_s, z_g)
    if not (np.isfinite(rho0) and rho0 >= 0.0):
        return zs, zg, False, 0, 0.0
    if rho0 == 0.0:
        return zs, zg, True, 0, 0.0
    used = 0
    with np.errstate(all="ignore"):
        for it in range(1, cg_iters + 1):
            qs, qg = Sp(ps, pg)
            pq = dot(ps, pg, qs, qg)
            used += 1
            if not (np.isfinite(pq) and pq > 0.0):
                return zs, zg, False, used, 0.0
            margins["pq"] = min(margins["pq"], pq / max(float(np.abs(ps * qs).sum() + np.abs(pg * qg).sum()), 1e-300))
            alpha = rho / pq
            xs, xg = xs + alpha * ps, xg + alpha * pg
            rs, rg = rs - alpha * qs, rg - alpha * qg
            z_s, z_g = P.msolve(L, rs), rg / Mg
            rho1 = dot(rs, rg, z_s, z_g)
            if not (np.isfinite(rho1) and rho1 >= 0.0):
                return zs, zg, False, used, 0.0
            thr = tol2 * rho0
            margins["cg_stop"] = min(margins["cg_stop"], abs(rho1 - thr) / max(rho1, thr, 1e-300))
            if rho1 <= thr or it == cg_iters:
                rho = rho1
                break
            ps, pg = z_s + (rho1 / rho) * ps, z_g + (rho1 / rho) * pg
            rho = rho1
    return xs, xg, True, used, float(np.sqrt(rho / rho0))


# ------------------------------------------------------------------------------------------------ the op
def adjust(indptr, obs_image, obs_keypoint, obs_use, point_use, kpts, xyz, cams, mode, group, iters=20, huber=0.0, lambda0=1e-4, cg_iters=64, cg_tol=1e-6,
           order="forward", rounds_out=None):
    indptr, obs_image, obs_keypoint = (np.asarray(x, dtype=np.int64) for x in (indptr, obs_image, obs_keypoint))
    obs_use, point_use = np.asarray(obs_use).astype(bool), np.asarray(point_use).astype(bool)
    kpts = np.asarray(kpts, dtype=np.float32).reshape(-1, 2)
    xyz0 = np.array(xyz, dtype=np.float64).reshape(-1, 3)
    cams0 = np.array(cams, dtype=np.float64).reshape(-1, B.CAMERA_WORDS)
    mode = np.asarray(mode, dtype=np.int64).reshape(-1)
    T, n_obs, n_images = len(indptr) - 1, len(obs_image), len(cams0)
    group = np.where(mode != 0, np.asarray(group, dtype=np.int64).reshape(-1), -1) if n_images else np.zeros(0, np.int64)      # an absent image's entry is ignored
    assert len(group) == n_images and (group >= -1).all() and (group < max(n_images, 1)).all()
    n_groups = int(group.max()) + 1 if n_images else 0
    huber, lam = float(np.float32(huber)), float(np.float32(lambda0))
    cg_tol = float(cg_tol)
    assert 1 <= cg_iters <= P.MAX_CG_ITERS and np.isfinite(cg_tol) and 0.0 <= cg_tol < 1.0
    tol2 = cg_tol * cg_tol
    rev = order == "reverse"
    cl = B.classify(indptr, obs_image, obs_keypoint, obs_use, point_use, kpts, xyz0, cams0, mode)
    slot_cam = np.flatnonzero(mode == 2)
    n_slots = len(slot_cam)
    assert n_slots <= P.MAX_FREE
    held = cl["cam_obs"][slot_cam] < 4
    slot_of = np.full(n_images, -1, np.int64)
    slot_of[slot_cam[~held]] = np.flatnonzero(~held)
    gimgs = [np.flatnonzero(group == g) for g in range(n_groups)]                   # the posed images of every group, ascending
    group_obs = np.array([int(cl["cam_obs"][im].sum()) for im in gimgs], np.int32).reshape(n_groups)
    gheld = group_obs < 4
    mgroup = np.where((group >= 0) & ~gheld[np.maximum(group, 0)], group, -1) if n_groups else np.full(n_images, -1, np.int64)
    ao = np.flatnonzero(cl["obs_act"])                                          # the active observations, ascending
    ot, ok_ = cl["obs_track"][ao], obs_image[ao]
    uv = kpts[cl["obs_node"][ao]].astype(np.float64)
    oslot = slot_of[ok_] if len(ao) else np.zeros(0, np.int64)                  # the slot of a moving camera, else -1
    ogrp = mgroup[ok_] if len(ao) else np.zeros(0, np.int64)                    # the group that moves, else -1
    ctx = dict(sums=P._Sums(ot, oslot, T, n_slots, rev), isums=P._Sums(ot, np.where(ogrp >= 0, ok_, -1), T, n_images, rev), psums=_PointSums(ot, oslot, ogrp, rev),
               rev=rev, ot=ot, oslot=oslot, ogrp=ogrp, held=held, gheld=gheld, slot_cam=slot_cam, mgroup=mgroup, gimgs=gimgs, T=T)
    out = dict(xyz=xyz0.copy(), cams=cams0.copy(), obs_error=np.full(n_obs, -1, np.float32), cam_obs=cl["cam_obs"], history=np.zeros((iters + 1, 2)),
               taken=np.zeros(iters, np.uint8), obs_sens=np.zeros(n_obs), cg_used=np.zeros(iters, np.int32), cg_res=np.zeros(iters),
               focal_scale=np.ones(n_groups), group_obs=group_obs, ds=np.zeros((iters, n_groups)))
    margins = dict(lead=np.inf, depth=np.inf, det=np.inf, m_pivot=np.inf, pq=np.inf, cg_stop=np.inf, mg_pivot=np.inf, f1=np.inf)
    stats = dict(n_free=int((~held).sum()), n_fixed=int((mode == 1).sum()), n_held=int(held.sum()), n_points=int(cl["pt_act"].sum()), n_active_obs=len(ao),
                 n_bad_obs=int(cl["n_bad"]), rounds_taken=0, status=cl["status"])

    def cost_of(X, C):
        ru, rv, z = B.observe(C, X[ot], ok_, uv, jac=False)
        with np.errstate(all="ignore"):
            terms = B.rho(ru * ru + rv * rv, huber)
        return B.total_cost(B._by_rank(ot, T, terms, rev), rev), z

    X, C, scale = xyz0.copy(), cams0.copy(), np.ones(n_groups)
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
    in_group = np.flatnonzero(mgroup >= 0)
    for r in range(iters):
        if stop:
            out["history"][r + 1] = cost, lam
            continue
        ru, rv, z, Ju, Jv, Pu, Pv = B.observe(C, X[ot], ok_, uv)
        Fu, Fv = focal_words(C, X[ot], ok_)
        if huber > 0.0:
            e = np.sqrt(ru * ru + rv * rv)
            sw = np.where(e > huber, np.sqrt(huber / np.where(e > huber, e, 1.0)), 1.0)
            ru, rv = np.where(e > huber, ru * sw, ru), np.where(e > huber, rv * sw, rv)
            Fu, Fv = np.where(e > huber, Fu * sw, Fu), np.where(e > huber, Fv * sw, Fv)
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
        d, dg = np.zeros((n_slots, 6)), np.zeros(n_groups)
        Wm, G = np.zeros((len(ao), 6, 3)), np.zeros((len(ao), 3))
        if (n_slots or n_groups) and regular:
            sys_ = round_system(ctx, lam, Ju, Jv, ru, rv, Pu, Pv, Fu, Fv, I, gp)
            Wm, G = sys_["Wm"], sys_["G"]
            if rounds_out is not None:
                rounds_out.append(dict(sys_, lam=lam, oslot=oslot, ogrp=ogrp, held=held, gheld=gheld, ot=ot, Ju=Ju, Jv=Jv, Pu=Pu, Pv=Pv, Fu=Fu, Fv=Fv, ru=ru, rv=rv,
                                       X=X.copy(), C=C.copy(), ok=ok_, uv=uv))
            d, dg, regular, out["cg_used"][r], out["cg_res"][r] = pcg(sys_, ctx, cg_iters, tol2, margins)
        take = False
        if regular:
            cam_terms = np.zeros((len(ao), 6, 3))
            mi = ctx["sums"].midx
            with np.errstate(all="ignore"):
                cam_terms[mi] = Wm[mi] * d[ctx["sums"].mslot][:, :, None]
                grp_terms = G * np.where(ogrp >= 0, dg[np.maximum(ogrp, 0)], 0.0)[:, None] if n_groups else np.zeros((len(ao), 3))
                s = ctx["psums"].run(gp, cam_terms, grp_terms)
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
            with np.errstate(all="ignore"):
                f1 = 1.0 + dg
                Cc[in_group, 0], Cc[in_group, 1] = C[in_group, 0] * f1[mgroup[in_group]], C[in_group, 1] * f1[mgroup[in_group]]
                scale_c = np.where(gheld, scale, scale * f1)
            lens = bool((f1[~gheld] > 0).all() and np.isfinite(Cc[in_group, :2]).all())
            if (~gheld).any():
                margins["f1"] = min(margins["f1"], float(np.abs(f1[~gheld]).min()))
            out["ds"][r] = dg
            finite = bool(np.isfinite(Xc[act]).all() and np.isfinite(Cc[slot_cam[~held]]).all()) and lens
            cand, zc = cost_of(Xc, Cc)
            front = bool((zc > 0).all())
            if len(zc) and finite:
                margins["depth"] = min(margins["depth"], float(np.abs(zc).min()))
            if finite and front:
                margins["lead"] = min(margins["lead"], B._tie_margin(cand, cost))
            take = finite and front and bool(np.isfinite(cand)) and bool(np.float32(cand) < np.float32(cost))
        if take:
            X, C, cost, rejects, scale = Xc, Cc, cand, 0, scale_c
            lam = max(lam / 10.0, 1e-12)
            stats["rounds_taken"] += 1
        else:
            lam = min(10.0 * lam, 1e12)
            rejects += 1
            stop = rejects >= B.MAX_REJECTS
        out["history"][r + 1] = cost, lam
        out["taken"][r] = 1 if take else 0
    out["xyz"], out["cams"], out["focal_scale"] = X, C, scale
    if len(ao):
        ru, rv, z, Ju, Jv, Pu, Pv = B.observe(C, X[ot], ok_, uv)
        Fu, Fv = focal_words(C, X[ot], ok_)
        err = np.sqrt(ru * ru + rv * rv)
        out["obs_error"][ao] = np.where(z > 0, np.minimum(err, np.finfo(np.float32).max), -1).astype(np.float32)
        sc_ = max(1.0, float(np.abs(X[cl["pt_act"]]).max()), float(np.abs(C[:, 4:16][mode != 0]).max()))
        out["obs_sens"][ao] = sc_ * (np.abs(Ju).sum(axis=1) + np.abs(Jv).sum(axis=1) + np.abs(Pu).sum(axis=1) + np.abs(Pv).sum(axis=1)) + np.abs(Fu) + np.abs(Fv)
    out.update(stats=stats, margins=margins)
    return out


def run(sc, group, **kw):
    return adjust(*(sc[k] for k in B.ARGS), group, **kw)
