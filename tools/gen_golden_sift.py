"""Write the SIFT detector fixtures under tests/golden/ from the reference checkout (build box only; needs PIL).

  sift_boat1.npz, sift_graf1.npz  the two PNG images of the reference's sweeps, decoded with PIL and reordered to BGR the way
                                  cv2.imread returns them: uint8 [H, W, 3] ``img`` (compressed), plus ``name``.  graf1 in BGR
                                  does not fit the 1 MiB limit for a committed file, so its ``img`` is the uint8 [H, W] result
                                  of BGR2GRAY (OpenCV's fixed point, the detector's own first step: same keypoints).
  sift_counts.npz                 per sweep directory under tools/files: the number of OpenCV SIFT keypoints on image 0.  The
                                  sweep records hold rows [r, t, m, correct, total, time] with total = len(matches0); with
                                  m <= 2 the graph build removes nothing, so total is the detector's count.  Also the image
                                  file names of the directory and their sizes (w, h).

Usage: python tools/gen_golden_sift.py /path/to/reference
"""
import ast
import collections
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")


def _bgr(path):
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)[:, :, ::-1])


def _gray(bgr):
    b, g, r = (bgr[:, :, i].astype(np.int32) for i in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def main(ref):
    files = os.path.join(ref, "tools", "files")
    for name, rel in (("boat1", "oxford_boat3/boat1.png"), ("graf1", "oxford_graf/graf1.png")):
        img = _bgr(os.path.join(files, rel))
        if name == "graf1":
            img = _gray(img)
        np.savez_compressed(os.path.join(OUT, f"sift_{name}.npz"), img=img, name=np.array(rel))
    dirs, counts, rows, images, sizes = [], [], [], [], []
    for d in sorted(os.listdir(files)):
        rec = os.path.join(files, d, "record.txt")
        if not os.path.exists(rec):
            continue
        c = collections.Counter()
        for line in open(rec):
            line = line.strip()
            if line.startswith("["):
                r = ast.literal_eval(line)
                if r[2] <= 2:
                    c[int(r[4])] += 1
        if not c:
            continue
        (total, n), = c.most_common(1)
        assert n == sum(c.values()), f"{d}: rows with m <= 2 disagree on the count: {c}"
        imgs = sorted(f for f in os.listdir(os.path.join(files, d)) if f.lower().endswith((".png", ".jpg", ".jpeg")))
        dirs.append(d); counts.append(total); rows.append(n)
        images.append(";".join(imgs))
        sizes.append(";".join("%dx%d" % Image.open(os.path.join(files, d, f)).size for f in imgs))
    np.savez_compressed(os.path.join(OUT, "sift_counts.npz"), dirs=np.array(dirs), counts=np.array(counts, np.int64),
                        rows=np.array(rows, np.int64), images=np.array(images), sizes=np.array(sizes))
    for r in zip(dirs, counts, rows, sizes):
        print(*r)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "../reference")
