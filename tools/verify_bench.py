#!/usr/bin/env python3
"""Device time of geometric verification on a batch of matcher-sized sets: the route through ``evalh.evaluate_pairs`` with an identity
ground truth (what tools/parameter_sweep.py did before ``verify_pairs`` existed) against ``verify_pairs`` without and with the local
optimisation.  Numbers for DESIGN.md 4.12.

Workload: ``--sets`` (512) synthetic sets, each a planted homography on an 800 x 600 canvas with ``--points`` (2300) keypoints per image,
about 2000 of them matched, 30 % of the matches wrong, 1 px of noise; 3000 hypotheses, 3 px.

Variants, alternating inside one process, ``--warmup`` rounds unmeasured, then ``--reps`` (>= 20) measured rounds:
  eval        evaluate_pairs(h_gt = identity): GT matching (3 rounds) + one wave per hypothesis + one refit       -- the parent's route
  eval_nogt   the same with n_iters = 0: the RANSAC kernels of gims_eval_pairs almost alone (the warp and the counts kernel remain)
  verify_lo0  verify_pairs(lo_iters=0): the same estimator through the gather / shared-model scoring / finish kernels
  verify_lo8  verify_pairs(lo_iters=8): with the local optimisation

Timing: HIP events around each call.  The host needs milliseconds to pack 512 descriptors, during which an idle GPU would make the
events measure the host; so every measured call is preceded by a matrix product long enough to keep the GPU busy until the call's
launches are queued (the start event is reached when that product ends).  What is reported is device time of the call's own launches.

``--model fundamental`` measures the fundamental-matrix model instead: the same number of sets, points, matches and wrong matches, but
of a two-view scene (random 3-D points at depth 4 .. 12 in front of two pinhole cameras, a rotation of a few degrees and a translation),
variants ``fundamental_lo0`` and ``fundamental_lo8``; the evaluation route has no such model and is left out.

``--model pose`` measures the calibrated relative-pose model on the same two-view scenes (focal length 700, principal point at the
centre of the canvas), variants ``pose_lo0`` and ``pose_lo8``, with the threshold of the fundamental run (3 px).

Prints one JSON line (median, min, max in ms per variant, and the inlier totals of the two verify variants)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gims_amd import evalh, synth, verify_pairs  # noqa: E402
from gims_amd.verify import RECORD_FIELDS  # noqa: E402

CANVAS = (800, 600)


def make_sets(n_sets, n_points, seed, device):
    datas, outs = [], []
    w, h = CANVAS
    for s in range(n_sets):
        r = np.random.default_rng(seed + s)
        H = synth.make_homography(seed + s, CANVAS).astype(np.float64)
        kp0 = (r.random((n_points, 2)) * [w, h]).astype(np.float32)
        q = np.concatenate([kp0.astype(np.float64), np.ones((n_points, 1))], 1) @ H.T
        warped = q[:, :2] / q[:, 2:3] + r.standard_normal((n_points, 2))
        perm = r.permutation(n_points)
        kp1 = np.zeros((n_points, 2), dtype=np.float32)
        kp1[perm] = warped.astype(np.float32)
        m0 = perm.astype(np.int64)
        m0[r.random(n_points) < 0.13] = -1
        wrong = np.nonzero((m0 > -1) & (r.random(n_points) < 0.3))[0]
        m0[wrong] = perm[np.roll(wrong, 1)]
        sc = r.random(n_points).astype(np.float32)
        datas.append(dict(keypoints0=torch.from_numpy(kp0).to(device)[None], keypoints1=torch.from_numpy(kp1).to(device)[None],
                          image0=np.zeros((h, w, 3), dtype=np.uint8)))
        outs.append(dict(matches0=torch.from_numpy(m0).to(device)[None], matching_scores0=torch.from_numpy(sc).to(device)[None]))
    return datas, outs


def make_two_view_sets(n_sets, n_points, seed, device):
    """As make_sets, the correspondences those of a camera that moved through a 3-D scene."""
    datas, outs = [], []
    w, h = CANVAS
    f = 700.0
    for s in range(n_sets):
        r = np.random.default_rng(seed + s)
        ang = 0.1 * (r.random(3) - 0.5)
        cx, cy, cz = np.cos(ang)
        sx, sy, sz = np.sin(ang)
        R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        t = np.array([0.8, 0.2, 0.3]) * (r.random(3) + 0.5)
        kp0 = (r.random((n_points, 2)) * [w, h]).astype(np.float32)
        z = 4.0 + 8.0 * r.random(n_points)
        X = np.concatenate([(kp0.astype(np.float64) - [w / 2, h / 2]) / f, np.ones((n_points, 1))], 1) * z[:, None]
        Y = X @ R.T + t
        seen = Y[:, :2] / Y[:, 2:3] * f + [w / 2, h / 2] + r.standard_normal((n_points, 2))
        perm = r.permutation(n_points)
        kp1 = np.zeros((n_points, 2), dtype=np.float32)
        kp1[perm] = seen.astype(np.float32)
        m0 = perm.astype(np.int64)
        m0[r.random(n_points) < 0.13] = -1
        wrong = np.nonzero((m0 > -1) & (r.random(n_points) < 0.3))[0]
        m0[wrong] = perm[np.roll(wrong, 1)]
        datas.append(dict(keypoints0=torch.from_numpy(kp0).to(device)[None], keypoints1=torch.from_numpy(kp1).to(device)[None],
                          image0=np.zeros((h, w, 3), dtype=np.uint8)))
        outs.append(dict(matches0=torch.from_numpy(m0).to(device)[None]))
    return datas, outs


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sets", type=int, default=512)
    ap.add_argument("--points", type=int, default=2300)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7000)
    ap.add_argument("--model", choices=("homography", "fundamental", "pose"), default="homography")
    ap.add_argument("-o", "--output", default=None, help="also write the JSON record to this file")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    two_view = args.model in ("fundamental", "pose")
    datas, outs = (make_two_view_sets if two_view else make_sets)(args.sets, args.points, args.seed, dev)
    cam = np.array([[700.0, 0, CANVAS[0] / 2], [0, 700.0, CANVAS[1] / 2], [0, 0, 1]])
    eye = [np.eye(3, dtype=np.float32)] * args.sets
    variants = {
        "pose_lo0": lambda: verify_pairs(datas, outs, thresh=3.0, iters=args.iters, lo_iters=0, seed=0, model="pose", intrinsics=(cam, cam)),
        "pose_lo8": lambda: verify_pairs(datas, outs, thresh=3.0, iters=args.iters, lo_iters=8, seed=0, model="pose", intrinsics=(cam, cam)),
    } if args.model == "pose" else {
        "fundamental_lo0": lambda: verify_pairs(datas, outs, thresh=3.0, iters=args.iters, lo_iters=0, seed=0, model="fundamental"),
        "fundamental_lo8": lambda: verify_pairs(datas, outs, thresh=3.0, iters=args.iters, lo_iters=8, seed=0, model="fundamental"),
    } if two_view else {
        "eval": lambda: evalh.evaluate_pairs(datas, outs, eye, ransac_thresh=3.0, ransac_iters=args.iters, seed=0),
        "eval_nogt": lambda: evalh.evaluate_pairs(datas, outs, eye, n_iters=0, ransac_thresh=3.0, ransac_iters=args.iters, seed=0),
        "verify_lo0": lambda: verify_pairs(datas, outs, thresh=3.0, iters=args.iters, lo_iters=0, seed=0),
        "verify_lo8": lambda: verify_pairs(datas, outs, thresh=3.0, iters=args.iters, lo_iters=8, seed=0),
    }
    a = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    # how long the host takes to issue a call, and how long one blocker product runs on the device
    host_ms = {}
    for name, fn in variants.items():
        t0 = time.perf_counter()
        keep = fn()
        host_ms[name] = 1e3 * (time.perf_counter() - t0)
        torch.cuda.synchronize()
        del keep
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(4):
        a @ a
    e1.record()
    torch.cuda.synchronize()
    mm_ms = e0.elapsed_time(e1) / 4
    times = {k: [] for k in variants}
    last = {}
    for rep in range(args.warmup + args.reps):
        for name, fn in variants.items():
            for _ in range(int(2.0 * host_ms[name] / mm_ms) + 2):
                a @ a
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last[name] = fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    col = RECORD_FIELDS.index("n_inliers")
    res = dict(model=args.model, sets=args.sets, points=args.points, iters=args.iters, reps=args.reps, host_issue_ms={k: round(v, 2) for k, v in host_ms.items()},
               correspondences_mean=float(np.mean([int((o["matches0"] > -1).sum()) for o in outs[:16]])),
               ms={k: dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3)) for k, v in times.items()},
               inliers_total={k: int(last[k]["records"][:, col].sum().item()) for k in variants if k not in ("eval", "eval_nogt")})
    if two_view:
        res["lo_rounds_mean"] = float(last[args.model + "_lo8"]["records"][:, RECORD_FIELDS.index("lo_rounds")].mean().item())
        if args.model == "pose":
            res["n_front_total"] = {k: int(last[k]["n_front"].sum().item()) for k in variants}
    else:
        res["inliers_total_eval"] = int(last["eval"]["records"][:, evalh.RECORD_FIELDS.index("n_inliers")].sum().item())
    line = json.dumps(res)
    print(line)
    if args.output:
        os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
        with open(args.output, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
