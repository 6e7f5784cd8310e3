"""Colour augmentation of the training images on the device (csrc/augment.hip).

The reference's default training configuration (configs/coco_config.yaml: ``apply_color_aug: true``) passes the original and the warped
image, each with its own draw, through this albumentations pipeline (utils/dataset.py:23-29)::

    Compose([OneOf([RandomBrightness(limit=0.4, p=0.6), RandomContrast(limit=0.3, p=0.7)], p=0.6),
             OneOf([MotionBlur(p=0.5), GaussNoise(p=0.6)], p=0.5)], p=0.65)

``ColorAug`` is this library's OWN, fully specified restatement of what those transforms are documented to do: the draws are NumPy's
(host, a seeded ``RandomState`` reproduces them), the pixels are computed by one HIP launch per batch (``hip.color_aug``; the arithmetic
is specified in include/gims_hip.h and restated in tests/aug_ref.py, which the device equals bit for bit).  Parity with albumentations /
OpenCV themselves is NOT pinned: neither package is available to compare against, and their random streams (Python's ``random``) could
not be reproduced from outside anyway.

Draw order of ``ColorAug.draw()`` (every line is one call on the generator; a seeded generator gives the same plans again):

1. ``uniform()`` < p, else the empty plan (1 call in all).
2. ``uniform()`` < 0.6 for the first OneOf; then ``choice(2, p=[6/13, 7/13])`` (the weights 0.6 : 0.7 normalised):
   0 brightness, alpha = 1, beta = ``uniform(-brightness_limit, brightness_limit)``;
   1 contrast, alpha = 1 + ``uniform(-contrast_limit, contrast_limit)``, beta = 0.
3. ``uniform()`` < 0.5 for the second OneOf; then ``choice(2, p=[5/11, 6/11])`` (0.5 : 0.6 normalised):
   0 motion blur: ksize = ``choice`` of the odd sizes in blur_limit, xs = ``randint(0, ksize)``, xe = ``randint(0, ksize)``; if xs == xe,
     (ys, ye) = ``choice(ksize, 2, replace=False)`` (two distinct values, one call), else ys = ``randint(0, ksize)``, ye = ``randint(0, ksize)``;
     the kernel is the 8-connected Bresenham line from (xs, ys) to (xe, ye) (what ``cv2.line(kernel, (xs, ys), (xe, ye), 1, thickness=1)``
     draws), cast to float32 and divided by its float32 sum;
   1 noise: var = ``uniform(*var_limit)``, sigma = float32(sqrt(var)), key = 64 bits from ``randint(0, 2**32, size=2, dtype=uint64)``
     (high word first).
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip

_KSIZES = (3, 5, 7)


def brightness_contrast_lut(alpha=1.0, beta=0.0):
    """albumentations' _brightness_contrast_adjust_uint with beta_by_max=True as a table: arange(256) in float32, times float32(alpha) if
    alpha != 1, plus float32(beta * 255) if beta != 0, clipped to [0, 255] and truncated to uint8."""
    lut = np.arange(256, dtype=np.float32)
    if alpha != 1:
        lut *= np.float32(alpha)
    if beta != 0:
        lut += np.float32(beta * 255)
    return np.clip(lut, 0, 255).astype(np.uint8)


def line_kernel(ksize, xs, ys, xe, ye):
    """The motion blur kernel: the 8-connected Bresenham line from (xs, ys) to (xe, ye) in a ksize x ksize float32 array (x the column),
    divided by its float32 sum.  Where the line passes exactly between two cells it takes the one nearer the END point."""
    k = np.zeros((ksize, ksize), dtype=np.float32)
    dx, dy = abs(xe - xs), -abs(ye - ys)
    sx, sy = (1 if xs < xe else -1), (1 if ys < ye else -1)
    x, y, err = xs, ys, dx + dy
    while True:
        k[y, x] = 1
        if x == xe and y == ye:
            break
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x += sx
        if e2 <= dx:
            err += dx
            y += sy
    return k / k.sum(dtype=np.float32)


class ColorAugPlan:
    """What one image gets: an optional LUT (brightness / contrast), then motion blur OR noise, or nothing.  ``applied`` is step 1 of the
    draw (the Compose's own p); ``empty`` says that nothing changes the image (not applied, or both OneOfs passed)."""

    def __init__(self, applied=False, lut_kind=None, alpha=1.0, beta=0.0, ksize=0, line=None, sigma=0.0, key=0):
        self.applied, self.lut_kind, self.alpha, self.beta = bool(applied), lut_kind, float(alpha), float(beta)
        self.ksize, self.line, self.sigma, self.key = int(ksize), line, np.float32(sigma), int(key)

    @property
    def empty(self):
        return self.lut_kind is None and self.ksize == 0 and not self.sigma > 0

    @property
    def lut(self):
        return None if self.lut_kind is None else brightness_contrast_lut(self.alpha, self.beta)

    @property
    def kernel(self):
        return None if self.ksize == 0 else line_kernel(self.ksize, *self.line[0], *self.line[1])

    def to_c(self) -> hip.AugPlan:
        p = hip.AugPlan()
        lut, kernel = self.lut, self.kernel
        if lut is not None:
            p.use_lut = 1
            p.lut[:] = lut.tolist()
        if kernel is not None:
            p.ksize = self.ksize
            p.kernel[:self.ksize * self.ksize] = kernel.reshape(-1).tolist()
        p.sigma = float(self.sigma)
        p.key = self.key
        return p

    def __repr__(self):
        return (f"ColorAugPlan(applied={self.applied}, lut_kind={self.lut_kind!r}, alpha={self.alpha}, beta={self.beta}, ksize={self.ksize}, "
                f"line={self.line}, sigma={float(self.sigma)}, key={self.key:#x})")


class ColorAug:
    """The reference's colour augmentation with its default parameters; see the module docstring for the draw order.  rng: an
    ``np.random.RandomState``; None draws from the global ``np.random`` like the homography draws do."""

    def __init__(self, p=0.65, brightness_limit=0.4, contrast_limit=0.3, blur_limit=(3, 7), var_limit=(10.0, 50.0), rng=None):
        self.p, self.brightness_limit, self.contrast_limit = float(p), float(brightness_limit), float(contrast_limit)
        self.ksizes = [k for k in _KSIZES if blur_limit[0] <= k <= blur_limit[1]]
        if not self.ksizes:
            raise ValueError("blur_limit must include one of the kernel sizes 3, 5, 7")
        self.var_limit = (float(var_limit[0]), float(var_limit[1]))
        if not 0 <= self.var_limit[0] <= self.var_limit[1]:
            raise ValueError("var_limit must be an ascending pair of variances >= 0")
        self.rng = rng if rng is not None else np.random

    def draw(self) -> ColorAugPlan:
        r = self.rng
        if not r.uniform() < self.p:
            return ColorAugPlan()
        plan = ColorAugPlan(applied=True)
        if r.uniform() < 0.6:
            if r.choice(2, p=[6 / 13, 7 / 13]) == 0:
                plan.lut_kind, plan.beta = "brightness", float(r.uniform(-self.brightness_limit, self.brightness_limit))
            else:
                plan.lut_kind, plan.alpha = "contrast", 1.0 + float(r.uniform(-self.contrast_limit, self.contrast_limit))
        if r.uniform() < 0.5:
            if r.choice(2, p=[5 / 11, 6 / 11]) == 0:
                k = int(r.choice(self.ksizes))
                xs, xe = int(r.randint(0, k)), int(r.randint(0, k))
                if xs == xe:
                    ys, ye = (int(v) for v in r.choice(k, 2, replace=False))
                else:
                    ys, ye = int(r.randint(0, k)), int(r.randint(0, k))
                plan.ksize, plan.line = k, ((xs, ys), (xe, ye))
            else:
                plan.sigma = np.float32(np.sqrt(r.uniform(*self.var_limit)))
                hi, lo = (int(v) for v in r.randint(0, 2 ** 32, size=2, dtype=np.uint64))
                plan.key = (hi << 32) | lo
        return plan

    def apply(self, images, plans=None):
        """images: device uint8 [n, h, w] / [n, h, w, 3], or one image [h, w] / [h, w, 3] (a 3-D tensor whose last dimension is 3 is one
        colour image, as in homography).  plans: one ColorAugPlan per image (or one plan for a single image); None draws them in batch
        order.  Returns a new device tensor of the same shape, asynchronously on the current stream; a batch whose plans are all empty is
        copied and nothing is launched."""
        if not torch.is_tensor(images) or not images.is_cuda or images.dtype != torch.uint8 or images.dim() not in (2, 3, 4):
            raise ValueError("ColorAug.apply takes a device uint8 tensor [n, h, w(, 3)] or one image [h, w(, 3)]")
        single = images.dim() == 2 or (images.dim() == 3 and images.shape[2] == 3)
        batch = images.unsqueeze(0) if single else images
        if plans is None:
            plans = [self.draw() for _ in range(batch.shape[0])]
        elif isinstance(plans, ColorAugPlan):
            plans = [plans]
        if len(plans) != batch.shape[0]:
            raise ValueError(f"{len(plans)} plans for {batch.shape[0]} images")
        if all(p.empty for p in plans):
            return images.clone(memory_format=torch.contiguous_format)
        out = hip.color_aug(batch, [p.to_c() for p in plans])
        return out[0] if single else out
