"""Resection on the device against the host route: --images + 2 cameras on an arc around 8192 planted points, every image
sees 4096 of them with 0.5 px of noise; the matches of the pairs (k, k + 1 .. k + --neighbours) are the planted correspondences with a
fraction --wrong of the rows pointed at a random keypoint (tests/triangulate_ref.py planted_matches).  Images 0 and 1 are posed, the others
hold NaN poses: build_tracks, triangulate_tracks (the points of the posed pair), then resect_images for the --images others.  Reports
  device_op       GIMS_AUX_RESECT_IMAGES alone, by device events around the op (gims_run_ops_timed): median, min, max of --runs runs
  resect_images   the whole gims_amd.resect_images call on the host clock, to the end of the device work (and the enqueue alone)
  host_route      what a caller does without the op: read track_of, the points, their mask and all keypoints back, then a PnP RANSAC per
                  image -- the NumPy restatement, run on the first --host-images entries and scaled to all of them (`extrapolated_ms`; 0:
                  all entries), and cv2.solvePnPRansac with the same threshold and iteration count when cv2 imports (`cv2`: null otherwise)
and compares the device result with the restatement's on the entries the host route ran (`results_equal`: ok, n_inliers, best_hyp,
kp_inlier; `max_pose_diff`) and with the planted cameras (`worst_dR`, `worst_dt` over the entries with a pose).  One JSON line, ms.

Usage: python tools/resect_bench.py [--images 48] [--points 8192] [--kpts 4096] [--iters 1024] [--runs 10] [--host-images 4]
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
from tests import resect_ref as RR  # noqa: E402
from tests import triangulate_ref as R  # noqa: E402

DEV = "cuda"


def op_alone(track_of, xyz, use, kpts, cams, runs, warmup, **kw):
    out = torch.empty(hip.resect_out_layout(cams, kw["iters"])["bytes"], dtype=torch.uint8, device=DEV)
    ops = hip.make_ops([hip.op_resect_images(track_of, xyz, use, kpts, cams, out, track_of.numel(), use.numel(), **kw)])
    ev = hip.EventPool(2)
    ms = []
    for it in range(warmup + runs):
        hip.run_ops_timed(ops, ev)
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(ev.elapsed_ms()[0])
    views = hip.resect_views(out, cams, kw["iters"])
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4), "runs": len(ms),
            "entries": len(cams), "keypoints": views["slots"][-1], "stats": dict(zip(hip.RESECT_COUNTERS, views["counters"].tolist()[:4]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--kpts", type=int, default=4096)
    ap.add_argument("--neighbours", type=int, default=6)
    ap.add_argument("--wrong", type=float, default=0.0005)
    ap.add_argument("--iters", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-images", type=int, default=4)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    n_images = a.images + 2
    m = R.planted_matches(1, n_images, a.points, a.kpts, noise=0.5, w_wrong=a.wrong, neighbours=a.neighbours)
    kpts = [torch.from_numpy(k).to(DEV) for k in m["kpts"]]
    outs = [{"matches0": torch.from_numpy(x).to(DEV)[None]} for x in m["matches"]]
    Rn, tn = m["R"].copy(), m["t"].copy()
    Rn[2:], tn[2:] = np.nan, np.nan
    which = list(range(2, n_images))
    kw = dict(thresh=4.0, iters=a.iters, lo_iters=8, min_inliers=12, seed=0)
    out = {"images": a.images, "points": a.points, "kpts": a.kpts, "pairs": len(m["pairs"]), "wrong": a.wrong, "iters": a.iters}

    tracks = gims_amd.build_tracks(m["counts"], m["pairs"], outs)
    pts = gims_amd.triangulate_tracks(tracks, kpts, (m["K"], Rn, tn))
    out["points3d"] = {"n_tracks": tracks.n_tracks, "valid": int(pts.valid.sum())}
    allk = torch.cat(kpts).contiguous()
    cams = hip.resect_cameras(m["K"], m["counts"], which)
    use = pts.valid.view(torch.uint8)
    out["device_op"] = op_alone(tracks.track_of, pts.xyz, use, allk, cams, a.runs, a.warmup, **kw)

    gims_amd.resect_images(pts, tracks, kpts, m["K"], which, **kw)
    torch.cuda.synchronize()
    t = time.perf_counter()
    poses = gims_amd.resect_images(pts, tracks, kpts, m["K"], which, **kw)
    t_enq = time.perf_counter()
    torch.cuda.synchronize()
    out["resect_images"] = {"wall_ms": round((time.perf_counter() - t) * 1e3, 3), "enqueue_ms": round((t_enq - t) * 1e3, 3)}
    out["stats"] = poses.stats
    got = {k: getattr(poses, k).cpu().numpy() for k in ("ok", "n_inliers", "best_hyp", "kp_inlier", "R", "t", "n_corr")}
    errs = [(float(np.abs(got["R"][e] - m["R"][k]).max()), float(np.abs(got["t"][e] - m["t"][k]).max())) for e, k in enumerate(which) if got["ok"][e]]
    out["worst_dR"], out["worst_dt"] = (round(max(x[0] for x in errs), 6), round(max(x[1] for x in errs), 6)) if errs else (None, None)
    out["n_corr"] = {"min": int(got["n_corr"].min()), "median": int(np.median(got["n_corr"])), "max": int(got["n_corr"].max())}

    torch.cuda.synchronize()
    t = time.perf_counter()
    h_track, h_xyz, h_use, h_kpts = tracks.track_of.cpu().numpy(), pts.xyz.cpu().numpy(), use.cpu().numpy(), allk.cpu().numpy()
    t_read = time.perf_counter()
    n_host = len(which) if a.host_images <= 0 else min(a.host_images, len(which))
    want = RR.resect(h_track, h_xyz, h_use, h_kpts, cams[:n_host], **kw)
    t_done = time.perf_counter()
    rest_ms = (t_done - t_read) * 1e3
    out["host_route"] = {"readback_ms": round((t_read - t) * 1e3, 2), "restatement_ms": round(rest_ms, 1), "restatement_entries": n_host,
                         "extrapolated_ms": round((t_read - t) * 1e3 + rest_ms * len(which) / max(n_host, 1), 1)}
    n_slots = int(want["slots"][-1])
    out["results_equal"] = bool(all(np.array_equal(got[k][:n_host], want[k]) for k in ("ok", "n_inliers", "best_hyp"))
                                and np.array_equal(got["kp_inlier"][:n_slots], want["kp_inlier"]))
    pose = np.concatenate([got["R"].reshape(-1, 9), got["t"]], axis=1)
    out["max_pose_diff"] = float(np.abs(pose[:n_host] - want["pose"]).max()) if n_host else 0.0
    out["host_over_device"] = round(out["host_route"]["extrapolated_ms"] / out["device_op"]["median_ms"], 1)

    out["cv2"] = None
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        t = time.perf_counter()
        n_ok = 0
        for e, k in enumerate(which):
            X, uv, _ = RR.gather(h_track, h_xyz, h_use, h_kpts, cams[e])
            if len(X) >= 4:
                ok, _, _, _ = cv2.solvePnPRansac(X, uv, m["K"][k], None, iterationsCount=a.iters, reprojectionError=4.0, flags=cv2.SOLVEPNP_P3P)
                n_ok += int(bool(ok))
        out["cv2"] = {"ms": round((time.perf_counter() - t) * 1e3 + out["host_route"]["readback_ms"], 1), "n_ok": n_ok, "version": cv2.__version__}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
