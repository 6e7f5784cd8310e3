"""Write the homography / label fixtures of DESIGN.md 4.9 under tests/golden/ from the UNMODIFIED reference (build box only).

  warp_homographies.npz  seeded get_perspective_mat (utils/preprocess_utils.py:36-72) with the config's augmentation_params, and a
                         strong-perspective variant, for several image sizes; scale_homography to 640x480; resize_aspect_ratio's
                         geometry (placement and np.random fill) per size.
  warp_labels.npz        torch_find_matches (preprocess_utils.py:98-132) and the match_indexes rows of train.py:118-125 for keypoint
                         sets with duplicates, exact 3.0 px distances and zero-match pairs, at n_iters 1 and 3.

OpenCV is not installed: inside this process only, the inert cv2 stub gets a perspectiveTransform (gims_amd.homography's double
restatement) and a resize that returns 255s of the requested size (resize_aspect_ratio's pixels are not what is recorded).

Usage: python tools/gen_golden_warp.py /path/to/reference
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(HERE, "_ref_stubs"))
sys.path.insert(0, ROOT)

import cv2  # noqa: E402  (the stub)
from gims_amd.homography import perspective_transform  # noqa: E402

AUG = dict(patch_ratio=0.85, perspective_x=0.0, perspective_y=0.0, shear_ratio=0.04, shear_angle=10, rotation_angle=25, scale=0.6,
           translation=0.6)                                   # configs/coco_config.yaml augmentation_params
STRONG = dict(AUG, perspective_x=0.0008, perspective_y=0.0008)
SIZES = [(640, 480), (640, 427), (427, 640), (481, 639), (53, 37), (1024, 768)]    # (w, h)


def _load(ref):
    cv2.perspectiveTransform = lambda pts, m: perspective_transform(pts, m)
    cv2.resize = lambda img, dsize, **kw: np.full((dsize[1], dsize[0]) + img.shape[2:], 255, np.uint8)
    spec = importlib.util.spec_from_file_location("ref_preprocess_utils", os.path.join(ref, "utils", "preprocess_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _mat(P, aug, w, h):
    return P.get_perspective_mat(aug['patch_ratio'], w // 2, h // 2, aug['perspective_x'], aug['perspective_y'], aug['shear_ratio'],
                                 aug['shear_angle'], aug['rotation_angle'], aug['scale'], aug['translation'])


def homographies(P):
    out = {"sizes": np.array(SIZES, np.int64)}
    hs, scaled, strong, seeds, geo = [], [], [], [], []
    for si, (w, h) in enumerate(SIZES):
        for k in range(4):
            seed = 1000 * si + k
            np.random.seed(seed)
            m = _mat(P, AUG, w, h)
            m2 = _mat(P, STRONG, w, h)
            hs.append(m), strong.append(m2), seeds.append(seed)
            scaled.append(P.scale_homography(m, h, w, 480, 640))
        np.random.seed(7000 + si)
        t = P.resize_aspect_ratio(np.zeros((h, w, 3), np.uint8), 480, 640)
        inner = np.argwhere(t[:, :, 0] == 255)
        (y0, x0), (y1, x1) = inner.min(0), inner.max(0) + 1
        fill = int(t[0, 0, 0]) if (y0, x0) != (0, 0) else int(t[-1, -1, 0])
        geo.append([y0, x0, y1 - y0, x1 - x0, fill, 7000 + si])
    out.update(seeds=np.array(seeds, np.int64), H=np.array(hs), H_strong=np.array(strong), H_scaled=np.array(scaled),
               aspect=np.array(geo, np.int64), aug=np.array([AUG[k] for k in sorted(AUG)], np.float64), aug_keys=np.array(sorted(AUG)))
    np.savez_compressed(os.path.join(OUT, "warp_homographies.npz"), **out)


def _cases():
    rng = np.random.default_rng(4242)
    cases = []
    # 1: random sets, near-identity homography (many matches), n_iters 1 and 3
    k0 = rng.uniform(0, 640, (300, 2)).astype(np.float32)
    H = np.array([[1.02, 0.01, 3.5], [-0.01, 0.99, -2.25], [1e-5, 0, 1]], np.float32)
    p = (np.c_[k0, np.ones(300)] @ H.astype(np.float64).T)
    k1 = (p[:, :2] / p[:, 2:]).astype(np.float32)[rng.permutation(300)] + rng.normal(0, 1.2, (300, 2)).astype(np.float32)
    k1 = np.concatenate([k1, rng.uniform(0, 640, (50, 2)).astype(np.float32)])
    for it in (1, 3):
        cases.append((k0, k1, H, it))
    # 2: duplicates in both sets and exact 3.0 px distances under the identity
    base = rng.integers(10, 600, (80, 2)).astype(np.float32)
    k0 = np.concatenate([base, base[:10], base[20:25]])
    k1 = np.concatenate([base[:40] + np.array([3.0, 0.0], np.float32), base[40:] + np.array([0.0, 2.0], np.float32), base[:5]])
    for it in (1, 3):
        cases.append((k0, k1, np.eye(3, dtype=np.float32), it))
    # 3: zero matches (the sets far apart)
    cases.append((rng.uniform(0, 100, (64, 2)).astype(np.float32), rng.uniform(300, 400, (70, 2)).astype(np.float32), np.eye(3, dtype=np.float32), 1))
    # 4: a training-size pair (2048 x 2048) through a drawn homography
    k0 = rng.uniform(0, 640, (2048, 2)).astype(np.float32)
    H = np.array([[0.9, -0.2, 60.0], [0.15, 1.1, -20.0], [2e-4, -1e-4, 1.0]], np.float32)
    p = (np.c_[k0, np.ones(2048)] @ H.astype(np.float64).T)
    k1 = (p[:, :2] / p[:, 2:]).astype(np.float32) + rng.normal(0, 2.0, (2048, 2)).astype(np.float32)
    cases.append((k0, k1[rng.permutation(2048)], H, 1))
    return cases


def labels(P):
    out = {}
    for ci, (k0, k1, H, it) in enumerate(_cases()):
        ma0, ma1, mi0, mi1 = P.torch_find_matches(torch.from_numpy(k0), torch.from_numpy(k1), torch.from_numpy(H), dist_thresh=3, n_iters=it)
        k = 0
        c0 = torch.cat([torch.full((len(ma0) + len(mi0) + len(mi1),), k, dtype=torch.long)])
        c1 = torch.cat([ma0, mi0, torch.full((len(mi1),), -1, dtype=torch.long)])
        c2 = torch.cat([ma1, torch.full((len(mi0),), -1, dtype=torch.long), mi1])
        rows = torch.stack([c0, c1, c2], -1).numpy()
        out.update({f"k0_{ci}": k0, f"k1_{ci}": k1, f"H_{ci}": H, f"iters_{ci}": np.int64(it), f"rows_{ci}": rows})
        print(f"case {ci}: n0 {len(k0)} n1 {len(k1)} iters {it}: {len(ma0)} matches, {len(rows)} rows")
    out["n_cases"] = np.int64(len(_cases()))
    np.savez_compressed(os.path.join(OUT, "warp_labels.npz"), **out)


if __name__ == "__main__":
    P = _load(sys.argv[1] if len(sys.argv) > 1 else "../reference")
    homographies(P)
    labels(P)
