"""Time the device SIFT descriptor stage (sift_describe_kernel, gims_amd/csrc/sift.hip) next to detection: HIP events around whole
calls, median of --iters calls after --warmup, on boat1 (850 x 680, 15 383 keypoints) alone and on a batch of 16 images (boat1 and
shifted copies of it).  ``describe`` is hip.sift_describe alone, on the pyramid and the keypoints a detection left on the device (no
host read); ``detect`` is hip.sift_detect with its one host read of the counts; ``detect_and_compute`` is the front end's
sift_detect_and_compute_device.  Prints one JSON line, milliseconds.

Usage: python tools/sift_desc_bench.py [--iters 20] [--warmup 3] [--batch 16]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gims_amd import frontend, hip  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(float(np.median(ms)), 3), round(float(np.min(ms)), 3)


def measure(images, iters, warmup):
    B, H, W = images.shape[:3]
    dets, pyr = hip.sift_detect(images, return_pyramid=True)
    parts = [frontend.keypoint_arrays(d) for d in dets]
    kp4 = torch.cat([p[0] for p in parts]).contiguous()
    octv = torch.cat([p[1] for p in parts]).contiguous()
    image = torch.cat([torch.full((len(p[0]),), b, dtype=torch.int32, device=kp4.device) for b, p in enumerate(parts)]) if B > 1 else None
    det = timed(lambda: hip.sift_detect(images), iters, warmup)
    desc = timed(lambda: hip.sift_describe(pyr, H, W, B, kp4, octv, image), iters, warmup)
    both = timed(lambda: frontend.sift_detect_and_compute_device(images), iters, warmup)
    return {"images": B, "keypoints": int(kp4.shape[0]), "detect_ms": det[0], "detect_ms_min": det[1], "describe_ms": desc[0],
            "describe_ms_min": desc[1], "detect_and_compute_ms": both[0], "detect_and_compute_ms_min": both[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
    img = np.load(os.path.join(root, "sift_boat1.npz"))["img"]
    one = torch.from_numpy(img)[None].cuda()
    batch = torch.from_numpy(np.stack([np.roll(img, (7 * b, 13 * b), (0, 1)) for b in range(a.batch)])).cuda()
    print(json.dumps({"boat1": measure(one, a.iters, a.warmup), "batch": measure(batch, a.iters, a.warmup), "iters": a.iters}))


if __name__ == "__main__":
    main()
