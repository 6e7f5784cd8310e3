#!/usr/bin/env python3
"""One training step from images on the device, split the way the reference's console reports it (train.py:100-140):
Dtime = training_pair + collate (random homography, warpPerspective, INTER_AREA resize to 640x480, upload of the decoded image),
Ptime = training_inputs (SIFT over the 2B images, keypoint filter / padding, patches, CAR-HyNet, labels),
Mtime = forward + backward + optimiser step.  B = 1 pair and 2048 keypoints, the reference's setting; medians over the steps, next to
tools/train_bench.py's synthetic-keypoint figure.

    python tools/train_images_bench.py [--steps 20] [--warmup 3] [--batch 1] [--color-aug]

--color-aug passes a seeded ``ColorAug`` to training_pair (the reference's ``apply_color_aug: true``); --aug-launch times the
augmentation launch alone (HIP events, two 480x640x3 images that both carry a non-empty plan) and prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gims_amd import ColorAug, ColorAugPlan, GMatcher, synth  # noqa: E402
from gims_amd import homography as HG  # noqa: E402
from gims_amd.carhynet import CARHyNet  # noqa: E402
from gims_amd.optim import Adam as FusedAdam  # noqa: E402

AUG = dict(patch_ratio=0.85, perspective_x=0.0, perspective_y=0.0, shear_ratio=0.04, shear_angle=10, rotation_angle=25, scale=0.6,
           translation=0.6)                     # configs/coco_config.yaml
PARAMS = dict(image_height=480, image_width=640, resize_aspect=False, augmentation_params=AUG)


def aug_launch(launches=300, warmup=20):
    """The augmentation launch alone for a batch of two 480x640x3 images, per kind of plan: median microseconds over `launches` HIP-event
    timings after a warm-up (table upload + kernel, as hip.color_aug enqueues them; output and workspace allocated before), next to the
    bytes the launch has to move (every byte read once and written once)."""
    from gims_amd import hip
    imgs = torch.from_numpy(np.stack([synth.make_textured_image(480, 640, 900 + i) for i in range(2)])).cuda()
    lib = hip.load()
    need = int(lib.gims_color_aug_workspace_bytes(2))
    out, work = torch.empty_like(imgs), torch.empty(need, dtype=torch.uint8, device="cuda")
    kinds = {"lut": [ColorAugPlan(True, "brightness", beta=0.2), ColorAugPlan(True, "contrast", alpha=1.2)],
             "lut+noise": [ColorAugPlan(True, "brightness", beta=0.2, sigma=6.0, key=11), ColorAugPlan(True, "contrast", alpha=1.2, sigma=5.0, key=12)],
             "lut+blur7": [ColorAugPlan(True, "brightness", beta=0.2, ksize=7, line=((0, 0), (6, 6))),
                           ColorAugPlan(True, "contrast", alpha=1.2, ksize=7, line=((6, 1), (0, 4)))],
             "mixed": [ColorAugPlan(True, "contrast", alpha=0.8, ksize=5, line=((4, 0), (0, 3))), ColorAugPlan(True, sigma=6.0, key=13)]}
    res = {"bytes_moved": 2 * imgs.numel(), "launches": launches}
    for name, plans in kinds.items():
        arr = (hip.AugPlan * 2)(*[p.to_c() for p in plans])
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for i in range(warmup + launches):
            if i >= warmup:
                ev[i - warmup][0].record()
            hip._check(lib.gims_color_aug(imgs.data_ptr(), 2, 480, 640, 3, arr, out.data_ptr(), work.data_ptr(), need, hip._stream()), "gims_color_aug")
            if i >= warmup:
                ev[i - warmup][1].record()
        torch.cuda.synchronize()
        us = [a.elapsed_time(b) * 1e3 for a, b in ev]
        res[name + "_us"] = {"median": float(np.median(us)), "min": float(np.min(us)), "p90": float(np.percentile(us, 90))}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for i in range(warmup + launches):                                                     # the plain copy of the same bytes
        if i >= warmup:
            ev[i - warmup][0].record()
        out.copy_(imgs)
        if i >= warmup:
            ev[i - warmup][1].record()
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in ev]
    res["copy_us"] = {"median": float(np.median(us)), "min": float(np.min(us)), "p90": float(np.percentile(us, 90))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--keypoints", type=int, default=2048)
    ap.add_argument("--no-synthetic", action="store_true", help="skip the train_bench.py comparison")
    ap.add_argument("--color-aug", action="store_true", help="augment both images of every pair (a ColorAug seeded with 10)")
    ap.add_argument("--aug-launch", action="store_true", help="time the augmentation launch alone and exit")
    a = ap.parse_args()
    if a.aug_launch:
        print(json.dumps({"aug_launch": aug_launch()}))
        return
    color_aug = ColorAug(rng=np.random.RandomState(10)) if a.color_aug else None
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
        pairs = [HG.training_pair(images[(i + k) % len(images)], PARAMS, color_aug=color_aug) for k in range(a.batch)]
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
    out = {"color_aug": bool(a.color_aug), "batch": a.batch, "keypoints": a.keypoints, "steps": a.steps, "dtime_ms": med(dt), "ptime_ms": med(pt), "mtime_ms": med(mt),
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
