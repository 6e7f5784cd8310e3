#!/usr/bin/env python3
"""One image pair matched under every (radius, percentile, min_size) of a grid -- the command line of the reference's
tools/parameter_search.py (``-r``, ``-t``, ``-m`` ranges as ``start,end`` inclusive, ``-k``) on ``GMatcher.sweep``: the pair is ingested once
and the settings run as batch entries, not as one ``forward`` per setting.

Input: a synthetic pair (``--synth N,SEED[,W,H]``, gims_amd.synth.make_pair) or saved keypoint tensors (``--pair FILE``: a ``torch.save``d dict
with keypoints0/1 (1, N, 2), descriptors0/1 (1, 256, N), scores0/1 (1, N) and image0/image1 -- arrays or just their (1, H, W, 3) shapes).
``-k`` keeps the K highest-scoring keypoints of each image.  Weights: ``-w`` a state dict, else synth.make_state_dict(123).  The model
settings are the reference tool's: sinkhorn_iterations=20, match_threshold=0.02.

Output: ``<output>/record.txt`` with one line per setting in the reference's format

    [r, t, m, correct_matches, total_matches, time]

* ``total_matches`` = len(matches0), the number of kept keypoints of image 0, as the reference writes it (parameter_search.py:162-165);
  a setting under which an image keeps nothing gives ``[r, t, m, 0, 0, time]``, as there.
* ``correct_matches`` = the inlier count of THIS LIBRARY's RANSAC homography (``sweep(verify=...)``: gims_verify_pairs on the sweep's outputs,
  one batched call per sub-batch), NOT of OpenCV's ``cv2.findHomography(..., cv2.USAC_DEFAULT)`` as in the reference: the two estimators
  differ, so these counts are comparable among themselves and not with a record.txt of the reference (parity unpinned).  The estimator
  (include/gims_hip.h): 3000 hypotheses, 3 px, best 4-point model, then ``--lo-iters`` rounds of local optimisation.  ``--lo-iters 0``
  (default) is one plain refit, the estimator of gims_eval_pairs, which this tool used before: its counts stay what they were.
* ``time`` = the wall time of the whole sweep divided by the number of settings (the settings are not timed one by one: they run together).
  The file's first line, a comment, says so.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gims_amd import GMatcher, synth  # noqa: E402


def str_to_range(s):
    start, end = (int(v) for v in s.split(","))
    return list(range(start, end + 1))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="GIMS parameter sweep on the device")
    ap.add_argument("-r", "--r-range", default="10,30", help="range of the radius (start,end)")
    ap.add_argument("-t", "--t-range", default="0,10", help="range of the percentile (start,end)")
    ap.add_argument("-m", "--m-range", default="0,10", help="range of min_size (start,end)")
    ap.add_argument("-k", "--max-keypoints", type=int, default=-1, help="keep the K highest-scoring keypoints per image")
    ap.add_argument("-c", "--cuda", default="cuda:0")
    ap.add_argument("-w", "--weights", default=None, help="state dict of the matcher (default: synth.make_state_dict(123))")
    ap.add_argument("-o", "--output", default="./exp_gims_search")
    ap.add_argument("--synth", default="1024,2001,800,600", help="N,SEED[,W,H] of a synthetic pair")
    ap.add_argument("--pair", default=None, help="torch-saved dict of keypoint tensors (overrides --synth)")
    ap.add_argument("--rows", type=int, default=None, help="keypoint rows per sub-batch (default: config['sweep_rows'])")
    ap.add_argument("--lo-iters", type=int, default=0, help="rounds of local optimisation of the RANSAC homography (0: one plain refit)")
    return ap.parse_args(argv)


def load_pair(args, device):
    if args.pair:
        raw = torch.load(args.pair, map_location="cpu")
    else:
        v = [int(x) for x in args.synth.split(",")]
        raw = synth.make_pair(v[0], v[1], canvas=(v[2], v[3]) if len(v) == 4 else None)
    data = {}
    for side in ("0", "1"):
        kp, de, sc = (torch.as_tensor(np.asarray(raw[k + side])).float() for k in ("keypoints", "descriptors", "scores"))
        if 0 < args.max_keypoints < kp.shape[1]:
            top = torch.sort(sc[0], descending=True, stable=True)[1][:args.max_keypoints]
            kp, de, sc = kp[:, top], de[:, :, top], sc[:, top]
        data["keypoints" + side], data["descriptors" + side], data["scores" + side] = kp.to(device), de.contiguous().to(device), sc.to(device)
        im = raw["image" + side]
        data["image" + side] = im if hasattr(im, "shape") else np.zeros(tuple(im), dtype=np.uint8)
    data["device"] = device
    return data


def records_to_lines(recs, inliers, per_setting_s):
    """record.txt lines of a sweep's records; inliers: one RANSAC inlier count per record (ignored where the record is an error)."""
    lines = []
    for rec, inl in zip(recs, inliers):
        row = [rec["radius"], rec["percentile"], rec["min_size"]]
        row += [0, 0] if rec["error"] is not None else [int(inl), int(rec["kept0"])]
        lines.append(str(row + [per_setting_s]))
    return lines


def main(argv=None):
    args = parse_args(argv)
    device = torch.device(args.cuda)
    torch.cuda.set_device(device)
    grid = [(r, t, m) for r in str_to_range(args.r_range) for t in str_to_range(args.t_range) for m in str_to_range(args.m_range)]
    model = GMatcher({"sinkhorn_iterations": 20, "match_threshold": 0.02}).eval()
    model.load_state_dict(torch.load(args.weights, map_location="cpu") if args.weights else synth.make_state_dict(123))
    data = load_pair(args, device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    recs = model.sweep(data, grid, rows=args.rows, outputs="matches", verify=dict(thresh=3.0, iters=3000, lo_iters=args.lo_iters, seed=0))
    live = [r for r in recs if r["error"] is None]
    counts = torch.stack([r["correct_matches"] for r in live]).cpu().numpy().tolist() if live else []       # one read for the whole grid
    inliers = dict(zip(map(id, live), counts))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    os.makedirs(args.output, exist_ok=True)
    path = os.path.join(args.output, "record.txt")
    with open(path, "w") as f:
        f.write(f"# [r, t, m, correct_matches, total_matches, time]; time = sweep wall time {dt:.3f} s / {len(grid)} settings (RANSAC included); "
                f"correct_matches = inliers of gims_verify_pairs' RANSAC (lo_iters={args.lo_iters}), not OpenCV USAC_DEFAULT\n")
        f.write("\n".join(records_to_lines(recs, [inliers.get(id(r), 0) for r in recs], dt / len(grid))) + "\n")
    st = model.sweep_stats_last
    print(f"{len(grid)} settings in {dt:.3f} s ({len(grid) / dt:.1f} settings/s), {st['sub_batches']} sub-batches, "
          f"{sum(r['error'] is not None for r in recs)} settings kept nothing -> {path}")


if __name__ == "__main__":
    main()
