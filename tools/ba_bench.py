"""Bundle adjustment on the device against the host route: the scene of tools/resect_bench.py -- --images + 2 cameras on an
arc around 8192 planted points, every image sees 4096 of them with 0.5 px of noise, the matches of the pairs (k, k + 1 .. k + --neighbours)
are the planted correspondences with a fraction --wrong of the rows pointed at a random keypoint.  Images 0 and 1 are posed and stay fixed;
build_tracks, triangulate_tracks (the points of the posed pair), resect_images for the others, triangulate_tracks (all), then
bundle_adjust with every resected camera free.  Reports
  device_op       GIMS_AUX_BUNDLE_ADJUST alone, by device events around the op (gims_run_ops_timed): median, min, max of --runs runs; the
                  same with iters = 0 (`setup_ms`: what is not a round) and the difference per round (`per_round_ms`)
  bundle_adjust   the whole gims_amd.bundle_adjust call on the host clock, to the end of the device work (and the enqueue alone)
  host_route      what a caller does without the op: read tracks, masks, points and all keypoints back, then adjust on the host -- the NumPy
                  restatement, run for --host-rounds rounds and scaled to --iters of them (`extrapolated_ms`: an EXTRAPOLATION, the
                  restatement was not run to the end), and scipy.optimize.least_squares (trf, sparse analytic Jacobian, at most --iters
                  evaluations) when scipy imports (`scipy`: null otherwise)
and what the adjustment did: rms reprojection error and the worst |R - planted|, |t - planted| before and after.  One JSON line, ms.
--solver pcg runs GIMS_AUX_BUNDLE_ADJUST_PCG with --cg-iters and --cg-tol and adds `cg_used` per round; the restatement of
the host route is then tests/ba_pcg_ref.py.  The dense solver takes at most 128 free cameras; the scene above that cap is the same
generator with more images at the same spacing, the arc wound round the scene (--images 254 --span-pi 5 --solver pcg: 256 images, 254
of them free; on an arc of pi the first two of 256 images would be too close to triangulate from).
--refine-focal shared|per_image (with --solver pcg) runs GIMS_AUX_BUNDLE_ADJUST_FOCAL: the focal lengths are unknowns, one
relative scale for all posed images or one per image; --focal-error 0.05 plants a starting focal that much too long in the K the whole
chain is given (with or without --refine-focal: without it the run shows the floor a wrong K leaves).  Adds `focal_scale` (the first
eight) and `focal_error` (the worst |focal_scale (1 + error) - 1|, the recovered focal against the planted one); the restatement of the
host route is then tests/ba_focal_ref.py and scipy is given the scales as unknowns.
gims_run_ops_timed times whole ops, so the split of a round by kernel is taken from a kernel trace of this tool.

Usage: python tools/ba_bench.py [--images 48] [--points 8192] [--kpts 4096] [--iters 20] [--runs 10] [--host-rounds 2 (0: the device side only)] [--no-scipy]
                               [--solver dense|pcg] [--cg-iters 64] [--cg-tol 1e-6] [--span-pi 1] [--no-restatement]
                               [--refine-focal shared|per_image] [--focal-error 0.05]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gims_amd  # noqa: E402
from gims_amd import hip  # noqa: E402
from tests import ba_focal_ref as F  # noqa: E402
from tests import ba_pcg_ref as P  # noqa: E402
from tests import ba_ref as B  # noqa: E402
from tests import triangulate_ref as R  # noqa: E402

DEV = "cuda"


def op_alone(dev, mode, iters, runs, warmup, solver="dense", cg_iters=64, cg_tol=1e-6, group=None):
    T, n_obs, n = dev["indptr"].numel() - 1, dev["obs_image"].numel(), dev["kpts"].shape[0]
    n_free = int((mode == 2).sum())
    pcg = solver == "pcg"
    layout, make_op, make_views = (hip.ba_pcg_out_layout, hip.op_bundle_adjust_pcg, hip.ba_pcg_views) if pcg else (hip.ba_out_layout, hip.op_bundle_adjust, hip.ba_views)
    if group is not None:                                        # the focal form: one more size, the group array in the table
        n_groups = hip.ba_focal_groups(mode, group)
        layout, make_op = (lambda *a_: hip.ba_focal_out_layout(*a_, n_groups)), hip.op_bundle_adjust_focal
        make_views = lambda *a_: hip.ba_focal_views(*a_, n_groups)      # noqa: E731
    out = torch.empty(layout(T, n_obs, len(mode), iters, n_free)["bytes"], dtype=torch.uint8, device=DEV)
    table = hip.ba_table(*(dev[k] for k in ("indptr", "obs_image", "obs_keypoint", "obs_use", "point_use")), **(dict(cg_iters=cg_iters, cg_tol=cg_tol) if pcg else {}),
                         **({} if group is None else dict(group=group)))
    ops = hip.make_ops([make_op(table, dev["kpts"], dev["xyz"], dev["cams"], mode, out, T, n_obs, n, iters, 0.0, 1e-4)])
    ev = hip.EventPool(2)
    ms = []
    for it in range(warmup + runs):
        hip.run_ops_timed(ops, ev)
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(ev.elapsed_ms()[0])
    views = make_views(out, T, n_obs, len(mode), iters, n_free)
    res = {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4), "runs": len(ms),
           "stats": dict(zip(hip.BA_COUNTERS, views["counters"].tolist())), "taken": views["taken"].tolist(), "scratch_mb": round(out.numel() / 2 ** 20, 1)}
    if pcg:
        res["cg_used"], res["cg_res_max"] = views["cg_used"].tolist(), float(views["cg_res"].max()) if iters else 0.0
    return res


def scipy_route(host, mode, iters, group=None):
    """scipy.optimize.least_squares on the same cost (squared loss), the same parameters (w, dt per free camera; with `group` a relative
    focal scale per group; the points), a sparse analytic Jacobian from the restatement's model."""
    from scipy.optimize import least_squares
    from scipy.sparse import csr_matrix
    cl = B.classify(*(host[k] for k in B.ARGS[:5]), host["kpts"], host["xyz"], host["cams"], mode)
    ao = np.flatnonzero(cl["obs_act"])
    ot, ok_ = cl["obs_track"][ao], host["obs_image"][ao].astype(np.int64)
    uv = host["kpts"][cl["obs_node"][ao]].astype(np.float64)
    slot_cam = np.flatnonzero(mode == 2)
    held = cl["cam_obs"][slot_cam] < 4
    slot_of = np.full(len(mode), -1, np.int64)
    slot_of[slot_cam[~held]] = np.flatnonzero(~held)
    oslot, T, ns = slot_of[ok_], len(host["xyz"]), len(slot_cam)
    X0, C0, act = host["xyz"], host["cams"], cl["pt_act"]
    gid = np.full(len(mode), -1, np.int64) if group is None else np.where(mode != 0, group, -1)
    ng = int(gid.max()) + 1 if len(gid) else 0
    ogrp, in_group = gid[ok_], np.flatnonzero(gid >= 0)

    def state(p):
        X, C = B.apply_step(X0, C0, slot_cam, held, act, p[:6 * ns].reshape(ns, 6), p[6 * ns + ng:].reshape(T, 3))
        C[in_group, 0], C[in_group, 1] = C[in_group, 0] * (1.0 + p[6 * ns + gid[in_group]]), C[in_group, 1] * (1.0 + p[6 * ns + gid[in_group]])
        return X, C

    def fun(p):
        return B.residuals(*state(p), ao, ot, ok_, uv)

    def jac(p):
        # (the camera Jacobian of the model is taken at the current rotation: exact at w = 0, first order in w elsewhere)
        X, C = state(p)
        _, _, _, Ju, Jv, Pu, Pv = B.observe(C, X[ot], ok_, uv)
        rows, cols, vals = [], [], []
        for half, (Jc, Jp) in enumerate(((Ju, Pu), (Jv, Pv))):
            r = 2 * np.arange(len(ao)) + half
            mv = oslot >= 0
            for c in range(6):
                rows.append(r[mv]), cols.append(6 * oslot[mv] + c), vals.append(Jc[mv, c])
            for m_ in range(3):
                rows.append(r), cols.append(6 * ns + ng + 3 * ot + m_), vals.append(Jp[:, m_])
        if ng:                                                   # d r / d s at the current scale: F / (1 + s)
            gv = ogrp >= 0
            for half, Fw in enumerate(F.focal_words(C, X[ot], ok_)):
                rows.append(2 * np.flatnonzero(gv) + half), cols.append(6 * ns + ogrp[gv]), vals.append(Fw[gv] / (1.0 + p[6 * ns + ogrp[gv]]))
        return csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * len(ao), 6 * ns + ng + 3 * T))

    t = time.perf_counter()
    res = least_squares(fun, np.zeros(6 * ns + ng + 3 * T), jac=jac, method="trf", tr_solver="lsmr", x_scale="jac", max_nfev=iters)
    got = {"ms": round((time.perf_counter() - t) * 1e3, 1), "nfev": int(res.nfev), "rms": round(float(np.sqrt(2 * res.cost / len(ao))), 5)}
    if ng:
        got["focal_scale"] = [round(float(1.0 + v), 7) for v in res.x[6 * ns:6 * ns + min(ng, 8)]]
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--kpts", type=int, default=4096)
    ap.add_argument("--neighbours", type=int, default=6)
    ap.add_argument("--wrong", type=float, default=0.0005)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-restatement", action="store_true", help="the host route by scipy only (the NumPy restatement takes minutes on a large scene)")
    ap.add_argument("--span-pi", type=float, default=1.0, help="the arc of the cameras in units of pi (more than 2: the arc winds round the scene)")
    ap.add_argument("--solver", choices=("dense", "pcg"), default="dense")
    ap.add_argument("--cg-iters", type=int, default=64)
    ap.add_argument("--cg-tol", type=float, default=1e-6)
    ap.add_argument("--refine-focal", choices=("shared", "per_image"), default=None, help="refine the focal lengths too (needs --solver pcg)")
    ap.add_argument("--focal-error", type=float, default=0.0, help="the starting focal lengths are this much too long (0.05: 5 %%)")
    a = ap.parse_args()
    if a.refine_focal and a.solver != "pcg":
        ap.error("--refine-focal needs --solver pcg")
    solve = dict(solver=a.solver, cg_iters=a.cg_iters, cg_tol=a.cg_tol)
    torch.set_grad_enabled(False)
    n_images = a.images + 2
    m = R.planted_matches(1, n_images, a.points, a.kpts, noise=0.5, w_wrong=a.wrong, neighbours=a.neighbours, span=a.span_pi * np.pi)
    m["K"] = m["K"].copy()
    m["K"][:, 0, 0], m["K"][:, 1, 1] = m["K"][:, 0, 0] * (1.0 + a.focal_error), m["K"][:, 1, 1] * (1.0 + a.focal_error)      # the K the chain is given
    kpts = [torch.from_numpy(k).to(DEV) for k in m["kpts"]]
    outs = [{"matches0": torch.from_numpy(x).to(DEV)[None]} for x in m["matches"]]
    Rn, tn = m["R"].copy(), m["t"].copy()
    Rn[2:], tn[2:] = np.nan, np.nan
    out = {"images": a.images, "points": a.points, "kpts": a.kpts, "pairs": len(m["pairs"]), "wrong": a.wrong, "iters": a.iters, "solver": a.solver}
    if a.solver == "pcg":
        out.update(cg_iters=a.cg_iters, cg_tol=a.cg_tol)
    out.update(refine_focal=a.refine_focal, focal_error_planted=a.focal_error)

    tracks = gims_amd.build_tracks(m["counts"], m["pairs"], outs)
    first = gims_amd.triangulate_tracks(tracks, kpts, (m["K"], Rn, tn))
    poses = gims_amd.resect_images(first, tracks, kpts, m["K"], list(range(2, n_images)), seed=0)
    cams = poses.cameras(m["K"], Rn, tn)
    pts = gims_amd.triangulate_tracks(tracks, kpts, cams)
    out["scene"] = {"n_tracks": tracks.n_tracks, "n_obs": int(tracks.obs_image.numel()), "valid": int(pts.valid.sum()), "resected": poses.stats["n_ok"]}
    posed = np.isfinite(cams[1]).all(axis=(1, 2))
    mode = np.where(posed, 2, 0).astype(np.int32)
    mode[:2] = 1
    rec = hip.triangulate_cameras(*cams, m["counts"])
    dev = dict(indptr=tracks.indptr.contiguous(), obs_image=tracks.obs_image.contiguous(), obs_keypoint=tracks.obs_keypoint.contiguous(),
               obs_use=pts.obs_inlier.contiguous(), point_use=pts.valid.view(torch.uint8).contiguous(), kpts=torch.cat(kpts).contiguous(), xyz=pts.xyz.contiguous(),
               cams=torch.from_numpy(rec).to(DEV))
    group = None
    if a.refine_focal:
        group = np.where(posed, 0 if a.refine_focal == "shared" else np.cumsum(posed) - 1, -1).astype(np.int32)
    out["device_op"] = op_alone(dev, mode, a.iters, a.runs, a.warmup, group=group, **solve)
    out["device_op"]["setup_ms"] = op_alone(dev, mode, 0, a.runs, a.warmup, group=group, **solve)["median_ms"]
    out["device_op"]["per_round_ms"] = round((out["device_op"]["median_ms"] - out["device_op"]["setup_ms"]) / max(a.iters, 1), 4)

    if a.refine_focal:
        solve["refine_focal"] = a.refine_focal
    gims_amd.bundle_adjust(pts, tracks, kpts, cams, iters=a.iters, **solve)
    torch.cuda.synchronize()
    t = time.perf_counter()
    adj = gims_amd.bundle_adjust(pts, tracks, kpts, cams, iters=a.iters, **solve)
    t_enq = time.perf_counter()
    torch.cuda.synchronize()
    out["bundle_adjust"] = {"wall_ms": round((time.perf_counter() - t) * 1e3, 3), "enqueue_ms": round((t_enq - t) * 1e3, 3)}
    stats, hist = adj.stats, adj.history.cpu().numpy()
    out["stats"] = stats
    n_act = max(stats["n_active_obs"], 1)
    Ka, Ra, ta = adj.cameras()
    out["rms_px"] = {"before": round(float(np.sqrt(hist[0, 0] / n_act)), 5), "after": round(float(np.sqrt(hist[-1, 0] / n_act)), 5)}
    out["worst_dR"] = {"before": round(float(np.abs(cams[1] - m["R"])[posed].max()), 6), "after": round(float(np.abs(Ra - m["R"])[posed].max()), 6)}
    if a.refine_focal:
        scale = adj.focal_scale.cpu().numpy()
        moved = adj.group_obs.cpu().numpy() >= 4
        out["focal_scale"] = [round(float(v), 7) for v in scale[:8]]
        out["focal_error"] = round(float(np.abs(scale[moved] * (1.0 + a.focal_error) - 1.0).max()), 7) if moved.any() else None
    out["worst_dt"] = {"before": round(float(np.abs(cams[2] - m["t"])[posed].max()), 6), "after": round(float(np.abs(ta - m["t"])[posed].max()), 6)}

    if a.host_rounds <= 0:                                       # the device side only (for a kernel trace)
        print(json.dumps(out))
        return
    torch.cuda.synchronize()
    t = time.perf_counter()
    host = {k: v.cpu().numpy() for k, v in dev.items()}
    t_read = time.perf_counter()
    rounds = max(1, min(a.host_rounds, max(a.iters, 1)))
    if a.no_restatement:
        out["host_route"] = {"readback_ms": round((t_read - t) * 1e3, 2)}
        out["scipy"] = None
        if not a.no_scipy:
            try:
                import scipy
                out["scipy"] = dict(scipy_route(host, mode, a.iters, group), version=scipy.__version__, readback_ms=out["host_route"]["readback_ms"])
            except ImportError:
                pass
        print(json.dumps(out))
        return
    want = (F.adjust(*(host[k] for k in B.ARGS[:8]), mode, group, iters=rounds, cg_iters=a.cg_iters, cg_tol=a.cg_tol) if group is not None
            else P.adjust(*(host[k] for k in B.ARGS[:8]), mode, iters=rounds, cg_iters=a.cg_iters, cg_tol=a.cg_tol) if a.solver == "pcg"
            else B.adjust(*(host[k] for k in B.ARGS[:8]), mode, iters=rounds))
    rest_ms = (time.perf_counter() - t_read) * 1e3
    out["host_route"] = {"readback_ms": round((t_read - t) * 1e3, 2), "restatement_ms": round(rest_ms, 1), "restatement_rounds": rounds,
                         "extrapolated_ms": round((t_read - t) * 1e3 + rest_ms * a.iters / rounds, 1)}
    out["results_equal"] = bool(np.array_equal(want["taken"], adj.taken.cpu().numpy()[:rounds]))
    out["max_cost_diff"] = float(np.abs(want["history"][:, 0] - hist[:rounds + 1, 0]).max() / max(hist[0, 0], 1.0))
    out["host_over_device"] = round(out["host_route"]["extrapolated_ms"] / out["device_op"]["median_ms"], 1)
    out["scipy"] = None
    if not a.no_scipy:
        try:
            import scipy
            out["scipy"] = dict(scipy_route(host, mode, a.iters, group), version=scipy.__version__, readback_ms=out["host_route"]["readback_ms"])
        except ImportError:
            pass
    print(json.dumps(out))


if __name__ == "__main__":
    main()
