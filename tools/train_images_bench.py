#!/usr/bin/env python3
"""One training step from images on the device, split the way the reference's console reports it (train.py:100-140):
Dtime = training_pair + collate (random homography, warpPerspective, INTER_AREA resize to 640x480, upload of the decoded image),
Ptime = training_inputs (SIFT over the 2B images, keypoint filter / padding, patches, CAR-HyNet, labels),
Mtime = forward + backward + optimiser step.  B = 1 pair and 2048 keypoints, the reference's setting; medians over the steps, next to
tools/train_bench.py's synthetic-keypoint figure.

    python tools/train_images_bench.py [--steps 20] [--warmup 3] [--batch 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gims_amd import GMatcher, synth  # noqa: E402
from gims_amd import homography as HG  # noqa: E402
from gims_amd.carhynet import CARHyNet  # noqa: E402
from gims_amd.optim import Adam as FusedAdam  # noqa: E402

AUG = dict(patch_ratio=0.85, perspective_x=0.0, perspective_y=0.0, shear_ratio=0.04, shear_angle=10, rotation_angle=25, scale=0.6,
           translation=0.6)                     # configs/coco_config.yaml
PARAMS = dict(image_height=480, image_width=640, resize_aspect=False, augmentation_params=AUG)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--keypoints", type=int, default=2048)
    ap.add_argument("--no-synthetic", action="store_true", help="skip the train_bench.py comparison")
    a = ap.parse_args()
    np.random.seed(10)
    images = [synth.make_textured_image(427, 640, 900 + i) for i in range(4)]          # decoded COCO-size images (640x427)
    net = CARHyNet().eval()
    net.load_state_dict(synth.make_carhynet_state_dict(321))
    m = GMatcher({"sinkhorn_iterations": 100, "pos_loss_weight": 0.45, "neg_loss_weight": 1.0})
    m.load_state_dict(synth.make_state_dict(123))
    m = m.cuda().train()
    opt = FusedAdam(m.parameters(), lr=1e-4)
    dt, pt, mt, rows = [], [], [], []
    for i in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pairs = [HG.training_pair(images[(i + k) % len(images)], PARAMS) for k in range(a.batch)]
        batch, hs = HG.collate(pairs)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        data = HG.training_inputs(batch, hs, net, max_keypoints=a.keypoints)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        with torch.enable_grad():
            loss, _, _ = m(data, mode="train")
            loss.backward()
        opt.step()
        opt.zero_grad()
        float(loss.detach())
        t3 = time.perf_counter()
        if i >= a.warmup:
            dt.append(t1 - t0), pt.append(t2 - t1), mt.append(t3 - t2), rows.append(len(data["matches"]))
    med = lambda v: float(np.median(v)) * 1e3   # noqa: E731
    out = {"batch": a.batch, "keypoints": a.keypoints, "steps": a.steps, "dtime_ms": med(dt), "ptime_ms": med(pt), "mtime_ms": med(mt),
           "step_ms": med(np.add(np.add(dt, pt), mt)), "steps_per_s": 1e3 / med(np.add(np.add(dt, pt), mt)), "label_rows": int(np.median(rows))}
    print(('%10s' * 4) % ('Dtime', 'Ptime', 'Mtime', 'steps/s'))
    print(('%10.4g' * 4) % (out["dtime_ms"] / 1e3, out["ptime_ms"] / 1e3, out["mtime_ms"] / 1e3, out["steps_per_s"]))
    if not a.no_synthetic:
        from tools.train_bench import measure
        syn = measure(keypoints=a.keypoints, steps=10, warmup=2, with_cpu=False)
        out["synthetic_train_bench"] = {"steps_per_s": syn["value"], "ms_per_step": syn["ms_per_step"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
