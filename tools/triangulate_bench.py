"""Track triangulation on the device against the host route: 50 cameras on an arc around 8192 planted points, every image
sees 4096 of them with 0.5 px of noise; the matches of the pairs (k, k + 1 .. k + --neighbours) are the planted correspondences with a
fraction --wrong of the rows pointed at a random keypoint (tests/triangulate_ref.py planted_matches).  The flow is build_tracks, then
triangulate_tracks.  Reports
  device_op           GIMS_AUX_TRIANGULATE_TRACKS alone, by device events around the op (gims_run_ops_timed): median, min, max of --iters runs
  triangulate_tracks  the whole gims_amd.triangulate_tracks call on the host clock, to the end of the device work (and the enqueue alone)
  host_route          what a caller does without the op: read the Tracks and all keypoints back, then the NumPy restatement -- run on the
                      first --host-tracks tracks and scaled to all of them by the number of observations (`extrapolated_ms`; 0: all tracks)
  short_tracks        a second scene of --short-tracks tracks of 2 - 4 observations (generated directly), the op alone
and compares the device result with the restatement's on the tracks the host route ran (`results_equal`: status, n_inliers, obs_inlier;
`max_xyz_diff`).  One JSON line, ms.

Usage: python tools/triangulate_bench.py [--images 50] [--points 8192] [--kpts 4096] [--iters 10] [--host-tracks 512] [--short-tracks 1000000]
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
from tests import triangulate_ref as R  # noqa: E402

DEV = "cuda"


def op_alone(indptr, obs_image, obs_keypoint, kpts, cams, iters, warmup, **kw):
    T, n_obs = indptr.numel() - 1, obs_image.numel()
    out = torch.empty(hip.triangulate_out_layout(T, n_obs)["bytes"], dtype=torch.uint8, device=DEV)
    ops = hip.make_ops([hip.op_triangulate_tracks(indptr, obs_image, obs_keypoint, kpts, cams, out, T, n_obs, cams.shape[0], kpts.shape[0], **kw)])
    ev = hip.EventPool(2)
    ms = []
    for it in range(warmup + iters):
        hip.run_ops_timed(ops, ev)
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(ev.elapsed_ms()[0])
    views = hip.triangulate_views(out, T, n_obs)
    res = {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4), "runs": len(ms),
           "tracks": T, "observations": n_obs, "stats": dict(zip(hip.TRI_COUNTERS, views["counters"].tolist()[:7]))}
    return res, views


def short_scene(seed, n_tracks, n_cams, noise=0.5):
    """n_tracks tracks of 2 - 4 observations in distinct cameras, every observation a keypoint of its own: device tensors for the op."""
    rng = np.random.default_rng(seed)
    K, Rm, t = R.arc_cameras(n_cams)
    X = rng.uniform(-0.5, 0.5, (n_tracks, 3))
    lengths = rng.integers(2, 5, n_tracks)
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    track = np.repeat(np.arange(n_tracks), lengths)
    slot = np.arange(indptr[-1]) - indptr[track]
    cam = (rng.integers(0, n_cams, n_tracks)[track] + slot * rng.integers(1, (n_cams - 1) // 3 + 1, n_tracks)[track]) % n_cams
    xc = np.einsum("nij,nj->ni", Rm[cam], X[track]) + t[cam]
    uv = np.stack([K[cam, 0, 0] * xc[:, 0] / xc[:, 2] + K[cam, 0, 2], K[cam, 1, 1] * xc[:, 1] / xc[:, 2] + K[cam, 1, 2]], axis=1)
    uv += noise * rng.standard_normal(uv.shape)
    order = np.argsort(cam, kind="stable")                        # the keypoints of an image are its observations, in track order
    counts = np.bincount(cam, minlength=n_cams)
    start = np.concatenate([[0], np.cumsum(counts)])
    kp = np.empty(len(cam), dtype=np.int64)
    kp[order] = np.arange(len(cam)) - start[cam[order]]
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(DEV)      # noqa: E731
    return dict(indptr=dev(indptr, np.int32), obs_image=dev(cam, np.int32), obs_keypoint=dev(kp, np.int32), kpts=dev(uv[order], np.float32),
                cams=dev(R.camera_records(K, Rm, t, counts.tolist()), np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=50)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--kpts", type=int, default=4096)
    ap.add_argument("--neighbours", type=int, default=6)
    ap.add_argument("--wrong", type=float, default=0.0005)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-tracks", type=int, default=512)
    ap.add_argument("--short-tracks", type=int, default=1000000)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    m = R.planted_matches(1, a.images, a.points, a.kpts, noise=0.5, w_wrong=a.wrong, neighbours=a.neighbours)
    kpts = [torch.from_numpy(k).to(DEV) for k in m["kpts"]]
    outs = [{"matches0": torch.from_numpy(x).to(DEV)[None]} for x in m["matches"]]
    cameras = (m["K"], m["R"], m["t"])
    out = {"images": a.images, "points": a.points, "kpts": a.kpts, "pairs": len(m["pairs"]), "wrong": a.wrong}

    tracks = gims_amd.build_tracks(m["counts"], m["pairs"], outs)
    lengths = tracks.lengths().cpu().numpy()
    out["tracks"] = {"n_tracks": tracks.n_tracks, "n_obs": tracks.n_obs, "longest": int(lengths.max()) if len(lengths) else 0,
                     "short": int((lengths <= hip.TRI_SHORT_TRACK).sum()), "up_to_64": int(((lengths > hip.TRI_SHORT_TRACK) & (lengths <= 64)).sum()),
                     "above_64": int((lengths > 64).sum())}
    allk = torch.cat(kpts).contiguous()
    cams = torch.from_numpy(hip.triangulate_cameras(*cameras, m["counts"])).to(DEV)
    out["device_op"], views = op_alone(tracks.indptr, tracks.obs_image, tracks.obs_keypoint, allk, cams, a.iters, a.warmup)

    gims_amd.triangulate_tracks(tracks, kpts, cameras)
    torch.cuda.synchronize()
    t = time.perf_counter()
    pts = gims_amd.triangulate_tracks(tracks, kpts, cameras)
    t_enq = time.perf_counter()
    torch.cuda.synchronize()
    out["triangulate_tracks"] = {"wall_ms": round((time.perf_counter() - t) * 1e3, 3), "enqueue_ms": round((t_enq - t) * 1e3, 3)}
    out["stats"] = pts.stats

    torch.cuda.synchronize()
    t = time.perf_counter()
    h_ptr, h_img, h_kp, h_kpts = tracks.indptr.cpu().numpy(), tracks.obs_image.cpu().numpy(), tracks.obs_keypoint.cpu().numpy(), allk.cpu().numpy()
    t_read = time.perf_counter()
    n_host = tracks.n_tracks if a.host_tracks <= 0 else min(a.host_tracks, tracks.n_tracks)
    n_host_obs = int(h_ptr[n_host])
    want = R.triangulate(h_ptr[:n_host + 1], h_img[:n_host_obs], h_kp[:n_host_obs], h_kpts, hip.triangulate_cameras(*cameras, m["counts"]))
    t_done = time.perf_counter()
    rest_ms = (t_done - t_read) * 1e3
    out["host_route"] = {"readback_ms": round((t_read - t) * 1e3, 2), "restatement_ms": round(rest_ms, 1), "restatement_tracks": n_host,
                         "extrapolated_ms": round((t_read - t) * 1e3 + rest_ms * tracks.n_obs / max(n_host_obs, 1), 1)}
    got = {k: getattr(pts, k).cpu().numpy() for k in ("status", "n_inliers", "obs_inlier", "xyz")}
    out["results_equal"] = bool(np.array_equal(got["status"][:n_host], want["status"]) and np.array_equal(got["n_inliers"][:n_host], want["n_inliers"])
                                and np.array_equal(got["obs_inlier"][:n_host_obs], want["obs_inlier"]))
    out["max_xyz_diff"] = float(np.abs(got["xyz"][:n_host] - want["xyz"]).max()) if n_host else 0.0
    out["host_over_device"] = round(out["host_route"]["extrapolated_ms"] / out["device_op"]["median_ms"], 1)

    sh = short_scene(2, a.short_tracks, a.images)
    out["short_tracks"], _ = op_alone(sh["indptr"], sh["obs_image"], sh["obs_keypoint"], sh["kpts"], sh["cams"], a.iters, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
