"""Time the device DIoU-NMS keypoint thinning (diou_nms_kernel, gims_amd/csrc/nms.hip): HIP events around the op through
gims_run_ops_timed, median of --iters runs after --warmup, on three inputs -- the detections of a batch of 16 images (boat1 and shifted
copies of it) in one call, 15 382 random keypoints over 850 x 680 (the published configuration's count), and a chain of 32 768 collinear
points 2 px apart with descending scores (the worst case: as many rounds as points).  Each is compared, rows and time, with the NumPy
restatement tests/nms_ref.py on this node's CPU (for the batch: its first image).  Prints one JSON line, milliseconds.

Usage: python tools/nms_bench.py [--iters 20] [--warmup 3] [--batch 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gims_amd import frontend, hip  # noqa: E402
from tests import nms_ref  # noqa: E402

DEV = "cuda"


def device_ms(kp4, order, offsets, radius, thr, h, w, iters, warmup):
    n, n_images = kp4.shape[0], offsets.numel() - 1
    keep = torch.empty(n, dtype=torch.int32, device=DEV)
    count = torch.empty(n_images + 1, dtype=torch.int32, device=DEV)
    work = torch.empty(hip.diou_nms_workspace_bytes(n, n_images), dtype=torch.uint8, device=DEV)
    ops = hip.make_ops([hip.op_diou_nms(kp4, order, offsets, keep, count, work, n_images, h, w, radius, thr)])
    pool = hip.EventPool(2)
    ms = []
    for it in range(warmup + iters):
        hip.run_ops_timed(ops, pool)
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(pool.elapsed_ms()[0])
    return round(float(np.median(ms)), 3), round(float(np.min(ms)), 3), keep.cpu().numpy(), count.cpu().numpy()


def measure(name, kp4_np, scores_np, bounds, radius, thr, h, w, iters, warmup):
    order = np.concatenate([nms_ref.make_order(scores_np[a:b]) + a for a, b in zip(bounds[:-1], bounds[1:])])
    assert len(order) == len(kp4_np)
    kp4 = torch.from_numpy(kp4_np).to(DEV)
    med, best, keep, count = device_ms(kp4, torch.from_numpy(order.astype(np.int32)).to(DEV), torch.from_numpy(np.asarray(bounds, np.int32)).to(DEV),
                                       radius, thr, h, w, iters, warmup)
    t = time.perf_counter()
    want_keep, want_count = nms_ref.run_op(kp4_np[:bounds[1]], order[:bounds[1]], bounds[:2], radius, thr)      # the first image on the CPU
    cpu_ms = (time.perf_counter() - t) * 1e3
    equal = bool(want_count[0] == count[0] and np.array_equal(want_keep[:want_count[0]], keep[:count[0]]))
    return {"input": name, "images": len(bounds) - 1, "keypoints": int(len(kp4_np)), "radius": radius, "kept": int(count[:-1].sum()), "device_ms": med,
            "device_ms_min": best, "numpy_first_image_ms": round(cpu_ms, 1), "first_image_keypoints": int(bounds[1]), "first_image_equal": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    out = []
    img = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "sift_boat1.npz"))["img"]
    batch = torch.from_numpy(np.stack([np.roll(img, (7 * b, 13 * b), (0, 1)) for b in range(a.batch)])).to(DEV)
    dets = hip.sift_detect(batch)
    kp4 = torch.cat([frontend.keypoint_arrays(d)[0] for d in dets]).cpu().numpy()
    resp = torch.cat([d["response"] for d in dets]).cpu().numpy()
    bounds = np.concatenate([[0], np.cumsum([len(d["pt"]) for d in dets])])
    for radius in (4, 0):
        out.append(measure("detector batch", kp4, resp, bounds, radius, 0.3, img.shape[0], img.shape[1], a.iters, a.warmup))
    rng = np.random.default_rng(3)
    n = 15382
    kp4 = np.stack([rng.random(n) * 850, rng.random(n) * 680, np.exp(rng.normal(1.2, 0.7, n)) + 1.5, np.zeros(n)], 1).astype(np.float32)
    scores = ((rng.permutation(n) + 1) / n).astype(np.float32)
    for radius in (4, 0):
        out.append(measure("random 850 x 680", kp4, scores, [0, n], radius, 0.3, 680, 850, a.iters, a.warmup))
    n = 32768
    kp4 = np.stack([10 + 2.0 * np.arange(n), np.full(n, 8.0), np.full(n, 3.0), np.zeros(n)], 1).astype(np.float32)
    out.append(measure("chain", kp4, (np.arange(n, 0, -1) / n).astype(np.float32), [0, n], 4, 0.3, 16, 2 * n + 20, max(a.iters // 4, 1), 1))
    print(json.dumps({"results": out, "iters": a.iters}))


if __name__ == "__main__":
    main()
