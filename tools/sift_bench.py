"""Time the device SIFT detector (gims_amd/csrc/sift.hip): HIP events around whole sift_detect calls (the final host read of
the count included), median of --iters calls after --warmup, for boat1 (850 x 680) alone and for a pair batch (boat1 and its
mirror image).  Prints one JSON line: ms per image and keypoints per second.

Usage: python tools/sift_bench.py [--iters 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gims_amd import hip  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
    img = np.load(os.path.join(root, "sift_boat1.npz"))["img"]
    one = torch.from_numpy(img)[None].cuda()
    pair = torch.from_numpy(np.stack([img, np.ascontiguousarray(img[:, ::-1])])).cuda()
    t1, o1 = timed(lambda: hip.sift_detect(one), a.iters, a.warmup)
    t2, o2 = timed(lambda: hip.sift_detect(pair), a.iters, a.warmup)
    n1, n2 = len(o1[0]["pt"]), sum(len(o["pt"]) for o in o2)
    print(json.dumps({"boat1_ms": round(t1, 3), "boat1_keypoints": n1, "pair_ms_per_image": round(t2 / 2, 3), "pair_keypoints": n2,
                      "keypoints_per_s": round(n2 / (t2 / 1e3)), "iters": a.iters}))


if __name__ == "__main__":
    main()
