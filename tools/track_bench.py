"""Multi-view tracks on the device against the host route: 50 images of 4096 keypoints, all 1225 pairs, matches from the
synthetic scene generator of the tests (tests/tracks_ref.py: 8192 scene points, every image sees 4096 of them, 80 % of the common points
matched, 0.05 % of the unmatched rows matched wrongly: about 1 500 wrong edges that merge some of the 8192 true tracks into conflicting
ones).  `glued` repeats the op alone with 2 % wrong rows, which glue everything into ONE conflicting component of all nodes.  Reports
  device_op      GIMS_AUX_BUILD_TRACKS alone, by device events around the op (gims_run_ops_timed), median of --iters runs
  build_tracks   the whole gims_amd.build_tracks call on the host clock: table build and upload, the op, the one read-back of the counters
  host_route     what a caller does without the op: read every matches0 back, then the NumPy restatement (sequential union-find plus a sort)
  match_features the time GMatcher.match_features takes for the same number of pairs at the same keypoint count on the same build, in
                 sub-batches of --batch pairs over a pool of encoded synthetic images (encode_images is not part of the figure)
and the op's share of the match_features time.  The device result is compared with the restatement's (results_equal).  One JSON line, ms.

Usage: python tools/track_bench.py [--images 50] [--kpts 4096] [--iters 10] [--batch 8] [--wrong 0.0005] [--glued 0.02] [--skip-matcher]
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
from gims_amd import GMatcher, hip, synth  # noqa: E402
from tests import tracks_ref as R  # noqa: E402

DEV = "cuda"
GRAPH = dict(radius=15, percentile=2, min_size=7)


def op_alone(counts, pairs, dev_matches, iters, warmup):
    entries = [(a, b, m, None, None) for (a, b), m in zip(pairs, dev_matches)]
    n = int(sum(counts))
    table = hip.upload_large(hip.tracks_table(entries, counts, DEV), DEV)
    start = hip.upload(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), DEV)
    track_of = torch.empty(n, dtype=torch.int32, device=DEV)
    out = torch.empty(hip.tracks_out_layout(n)[-1], dtype=torch.int32, device=DEV)
    counters = torch.empty(8, dtype=torch.int32, device=DEV)
    work = torch.empty(hip.tracks_work_bytes(len(pairs), len(counts), n), dtype=torch.uint8, device=DEV)
    ops = hip.make_ops([hip.op_build_tracks(table, start, track_of, out, counters, work, len(pairs), len(counts), n)])
    ev = hip.EventPool(2)
    ms = []
    for it in range(warmup + iters):
        hip.run_ops_timed(ops, ev)
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(ev.elapsed_ms()[0])
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4), "runs": len(ms),
            "work_mib": round(work.numel() / 2 ** 20, 1)}


def matcher_time(kpts, n_pairs, batch):
    model = GMatcher({}).eval()
    model.load_state_dict(synth.make_state_dict(123))
    pool = []
    for pid in range(8):
        pair = synth.make_pair(kpts, 1000 + pid)
        for s in "01":
            pool.append({"keypoints": torch.from_numpy(pair["keypoints" + s]).to(DEV), "descriptors": torch.from_numpy(pair["descriptors" + s]).to(DEV),
                         "scores": torch.from_numpy(pair["scores" + s]).to(DEV), "image": pair["image" + s]})
    feats = model.encode_images(pool, **GRAPH)
    every = R.all_pairs(len(pool))
    todo = [every[k % len(every)] for k in range(n_pairs)]
    for _ in range(3):
        model.match_features(feats, todo[:batch])
    torch.cuda.synchronize()
    t = time.perf_counter()
    for o in range(0, n_pairs, batch):
        model.match_features(feats, todo[o:o + batch])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) * 1e3
    return {"total_ms": round(ms, 1), "pairs": n_pairs, "batch": batch, "ms_per_pair": round(ms / n_pairs, 4), "kept_keypoints": [f.n for f in feats[:2]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=50)
    ap.add_argument("--kpts", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--wrong", type=float, default=0.0005)
    ap.add_argument("--glued", type=float, default=0.02)
    ap.add_argument("--skip-matcher", action="store_true")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    counts, pairs, matches = R.scene(1, 2 * a.kpts, a.images, 0.5, 0.8, a.wrong, n_seen=a.kpts)
    dev_matches = [torch.from_numpy(m).to(DEV) for m in matches]
    out = {"images": a.images, "kpts": a.kpts, "pairs": len(pairs), "nodes": int(sum(counts)), "rows": int(sum(counts[i] for i, _ in pairs)), "wrong": a.wrong}
    out["device_op"] = op_alone(counts, pairs, dev_matches, a.iters, a.warmup)

    outs = [{"matches0": m[None]} for m in dev_matches]
    gims_amd.build_tracks(counts, pairs, outs)
    torch.cuda.synchronize()
    t = time.perf_counter()
    tracks = gims_amd.build_tracks(counts, pairs, outs)
    out["build_tracks"] = {"wall_ms": round((time.perf_counter() - t) * 1e3, 3)}
    out["stats"] = tracks.stats
    out["longest_track"] = int(tracks.lengths().max()) if tracks.n_tracks else 0

    torch.cuda.synchronize()
    t = time.perf_counter()
    host = [m.cpu().numpy() for m in dev_matches]
    t_read = time.perf_counter()
    want = R.build(counts, pairs, host)
    t_done = time.perf_counter()
    out["host_route"] = {"readback_ms": round((t_read - t) * 1e3, 1), "restatement_ms": round((t_done - t_read) * 1e3, 1), "total_ms": round((t_done - t) * 1e3, 1)}
    got = {k: getattr(tracks, k).cpu().numpy() for k in ("track_of", "indptr", "obs_image", "obs_keypoint", "conflict")}
    out["results_equal"] = bool(all(np.array_equal(got[k], want[k]) for k in got) and tracks.stats == want["stats"])
    out["host_over_device"] = round(out["host_route"]["total_ms"] / out["device_op"]["median_ms"], 1)
    out["faster_than_host_route"] = bool(out["device_op"]["median_ms"] < out["host_route"]["total_ms"]
                                         and out["build_tracks"]["wall_ms"] < out["host_route"]["total_ms"])
    # the worst case for the op: enough wrong matches (2 % of the unmatched rows) to glue all tracks into one conflicting component
    g_counts, g_pairs, g_matches = R.scene(2, 2 * a.kpts, a.images, 0.5, 0.8, a.glued, n_seen=a.kpts)
    g_dev = [torch.from_numpy(m).to(DEV) for m in g_matches]
    out["glued"] = {"wrong": a.glued, "device_op": op_alone(g_counts, g_pairs, g_dev, a.iters, a.warmup)}
    g_tracks = gims_amd.build_tracks(g_counts, g_pairs, [{"matches0": m[None]} for m in g_dev], conflicts="keep")
    out["glued"]["stats"] = g_tracks.stats
    out["glued"]["longest_track"] = int(g_tracks.lengths().max()) if g_tracks.n_tracks else 0
    g_want = R.build(g_counts, g_pairs, g_matches, conflicts="keep")
    out["glued"]["results_equal"] = bool(all(np.array_equal(getattr(g_tracks, k).cpu().numpy(), g_want[k]) for k in got) and g_tracks.stats == g_want["stats"])
    if not a.skip_matcher:
        out["match_features"] = matcher_time(a.kpts, len(pairs), a.batch)
        out["op_share_of_match_features"] = round(out["device_op"]["median_ms"] / out["match_features"]["total_ms"], 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
