"""NumPy restatement of the descriptor stage of gims_amd/csrc/sift.hip (``sift_describe_kernel``): OpenCV 4.x ``calcSIFTDescriptor``
(d = 4, n = 8) for keypoints over the detector's own Gaussian pyramid (``sift_ref.pyramid``), as include/gims_hip.h states it under
GIMS_AUX_SIFT_DESCRIBE.

Every operation is float32 in the kernel's order, without fused multiply-add; ``exp``, ``cos`` and ``sin`` are taken in double and
rounded; each of the 360 histogram entries is summed in ascending sample order (``np.add.at`` walks its index list front to back) and
the two 128-term norms are sequential (``np.cumsum``).  Rows and columns outside ``0 < r < rows - 1``, ``0 < c < cols - 1`` are cut
from the sample ranges instead of being tested per sample, which keeps the same samples in the same order.
"""
from __future__ import annotations

import math

import numpy as np

from tests import sift_ref as R

F = np.float32
EPS = np.finfo(np.float32).eps
D, N = 4, 8
OFFSETS = np.array([0, 1, 10, 11, 60, 61, 70, 71], np.int64)      # (row, column, orientation) = 000 001 010 011 100 101 110 111


# The discrimination fixture: a synthetic textured image and its warp by a mild known homography.  What the restatement reaches on it
# (detect, describe, RootSIFT, mutual nearest neighbours at 0.8, matches within 3 px of the ground truth), recorded by
# tests/test_sift_desc_cpu.py::test_descriptors_discriminate_on_a_warped_pair, which asserts that it still holds.
PAIR = dict(h=240, w=320, seed=7, hseed=21, strength=0.3)
PAIR_RECORD = dict(matches=246, correct=244)          # precision 0.9919


def warped_pair():
    """(img0, img1, H): uint8 [240, 320, 3] images with img1 = warpPerspective(img0, H) (tests/warp_ref.py)."""
    from gims_amd import synth
    from tests import warp_ref
    h, w = PAIR["h"], PAIR["w"]
    img0 = synth.make_textured_image(h, w, PAIR["seed"])
    H = synth.make_homography(PAIR["hseed"], (w, h), strength=PAIR["strength"])
    return img0, warp_ref.warp_perspective(img0, H, (w, h)), H


def root_sift(desc, eps=1e-7, l2norm=False):
    """The reference's rootSIFT / desc_l2norm (utils/common.py:687-708) in float32 NumPy."""
    d = np.asarray(desc, F)
    d = d / (d.sum(axis=1, keepdims=True) + F(eps))
    d = np.sqrt(d)
    if l2norm:
        d = d / np.sqrt((d * d).sum(axis=1, keepdims=True) + F(1e-10))
    return d


def count_correct(pt0, pt1, matches0, H, tol=3.0):
    """(matches, those whose image-1 keypoint lies within tol px of H applied to the image-0 keypoint)."""
    m = np.asarray(matches0).reshape(-1)
    idx = np.nonzero(m >= 0)[0]
    p = np.concatenate([np.asarray(pt0, np.float64)[idx], np.ones((len(idx), 1))], 1) @ np.asarray(H, np.float64).T
    err = np.linalg.norm(p[:, :2] / p[:, 2:] - np.asarray(pt1, np.float64)[m[idx]], axis=1)
    return len(idx), int((err <= tol).sum())


def unpack_octave(octave):
    """(o, layer, scale) of OpenCV's unpackOctave."""
    o = int(octave) & 255
    o = o if o < 128 else (-128 | o)
    layer = (int(octave) >> 8) & 255
    scale = F(1) / F(1 << o) if o >= 0 else F(1 << -o)
    return o, layer, scale


def cv_round(v):
    """cvRound (half to even); NaN and what does not fit an int go to +-1e9 first, like the kernel."""
    v = F(v)
    if np.isnan(v):
        return -1000000000
    return int(np.rint(min(max(v, F(-1e9)), F(1e9))))


def radius_of(size, scale, rows, cols):
    hist_width = F(3) * (F(size) * scale * F(0.5))
    radius = cv_round(hist_width * F(1.4142135623730951) * F(5) * F(0.5))
    return min(radius, int(math.sqrt(float(cols) * cols + float(rows) * rows)))


def describe_one(img, x, y, size, angle, scale, exp32=False, entry9=None):
    """One keypoint on its level ``img`` -> float32 [128].  entry9: a list that receives the largest value any cell's orientation entry 9
    holds before the fold (non-zero only when a sample had o0 = -1)."""
    rows, cols = img.shape
    ptx, pty = F(x) * scale, F(y) * scale
    scl = F(size) * scale * F(0.5)
    ori = F(360) - F(angle)
    if abs(ori - F(360)) < EPS:
        ori = F(0)
    px, py = cv_round(ptx), cv_round(pty)
    arg = ori * F(math.pi / 180)
    cos_t, sin_t = F(math.cos(float(arg))), F(math.sin(float(arg)))
    bins_per_rad = F(8) / F(360)
    exp_scale = F(-1) / F(D * D * 0.5)
    hist_width = F(3) * scl
    radius = radius_of(size, scale, rows, cols)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos_t, sin_t = F(cos_t / hist_width), F(sin_t / hist_width)
    hist = np.zeros((D + 2) * (D + 2) * (N + 2), F)
    i_lo, i_hi = max(-radius, 1 - py), min(radius, rows - 2 - py)
    j_lo, j_hi = max(-radius, 1 - px), min(radius, cols - 2 - px)
    if i_hi >= i_lo and j_hi >= j_lo:
        ii, jj = np.meshgrid(np.arange(i_lo, i_hi + 1), np.arange(j_lo, j_hi + 1), indexing="ij")
        ii, jj = ii.reshape(-1), jj.reshape(-1)
        fi, fj = ii.astype(F), jj.astype(F)
        with np.errstate(invalid="ignore"):
            c_rot = fj * cos_t - fi * sin_t
            r_rot = fj * sin_t + fi * cos_t
            rbin = r_rot + F(2) - F(0.5)
            cbin = c_rot + F(2) - F(0.5)
            keep = (rbin > -1) & (rbin < D) & (cbin > -1) & (cbin < D)
        ii, jj, c_rot, r_rot, rbin, cbin = (v[keep] for v in (ii, jj, c_rot, r_rot, rbin, cbin))
        r, c = py + ii, px + jj
        dx = img[r, c + 1] - img[r, c - 1]
        dy = img[r - 1, c] - img[r + 1, c]
        w = ((c_rot * c_rot + r_rot * r_rot) * exp_scale).astype(F)
        w = np.exp(w).astype(F) if exp32 else np.exp(w.astype(np.float64)).astype(F)
        mag = np.sqrt(dx * dx + dy * dy).astype(F) * w
        obin = ((R.fast_atan2(dy, dx) - ori) * bins_per_rad).astype(F)
        r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
        rbin, cbin, obin = (rbin - r0).astype(F), (cbin - c0).astype(F), (obin - o0).astype(F)
        r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
        o0 = np.where(o0 < 0, o0 + N, o0)
        o0 = np.where(o0 >= N, o0 - N, o0)
        # an angle in -1 .. 360 (cv::KeyPoint's range; -1 gives ori = 361) leaves o0 in -1 .. 7, and o0 = -1 votes at idx - 1: entry 9 of
        # the cell before in the flat histogram (folded into that cell's entry 1 below) and entry 0 of its own.  A sample of any other
        # angle whose o0 falls outside -1 .. 7 is dropped, where OpenCV would write outside its histogram.
        ok = (o0 >= -1) & (o0 <= N - 1)
        mag, rbin, cbin, obin, r0, c0, o0 = (v[ok] for v in (mag, rbin, cbin, obin, r0, c0, o0))
        v_r1 = mag * rbin
        v_r0 = mag - v_r1
        v_rc11 = v_r1 * cbin
        v_rc10 = v_r1 - v_rc11
        v_rc01 = v_r0 * cbin
        v_rc00 = v_r0 - v_rc01
        vals = []
        for v in (v_rc00, v_rc01, v_rc10, v_rc11):
            v1 = v * obin
            vals += [v - v1, v1]
        vals = np.stack(vals, 1).astype(F)
        idx = (((r0 + 1) * (D + 2) + c0 + 1) * (N + 2) + o0)[:, None] + OFFSETS[None, :]
        idx, vals = idx.reshape(-1), vals.reshape(-1)
        inside = idx >= 0                                      # corner cell 0 with o0 = -1: idx - 1 is before the histogram, dropped
        np.add.at(hist, idx[inside], vals[inside])
    if entry9 is not None:
        entry9.append(float(hist[N + 1::N + 2].max()))
    dst = np.empty(D * D * N, F)
    for i in range(D):
        for j in range(D):
            idx = ((i + 1) * (D + 2) + (j + 1)) * (N + 2)
            hist[idx] += hist[idx + N]
            hist[idx + 1] += hist[idx + N + 1]
            dst[(i * D + j) * N:(i * D + j + 1) * N] = hist[idx:idx + N]
    nrm2 = np.cumsum(dst * dst, dtype=F)[-1]
    thr = F(np.sqrt(nrm2)) * F(0.2)
    dst = np.minimum(dst, thr)
    nrm2 = np.cumsum(dst * dst, dtype=F)[-1]
    f = F(512) / max(F(np.sqrt(nrm2)), EPS)
    return np.clip(np.rint(dst * f), 0, 255).astype(F)


def describe(gp, kp4, octave, exp32=False, entry9=None):
    """gp: ``sift_ref.pyramid(img)[0]``; kp4 [n, 4] = x, y, size, angle; octave [n] packed -> (float32 [n, 128] with integer values
    0 .. 255, bad): keypoints whose octave or layer is outside the pyramid get zeros and are counted."""
    kp4 = np.asarray(kp4, F).reshape(-1, 4)
    out = np.zeros((len(kp4), D * D * N), F)
    bad = 0
    for k in range(len(kp4)):
        o, layer, scale = unpack_octave(octave[k])
        if o + 1 < 0 or o + 1 >= len(gp) or layer >= len(gp[0]):
            bad += 1
            if entry9 is not None:
                entry9.append(0.0)
            continue
        out[k] = describe_one(gp[o + 1][layer], kp4[k, 0], kp4[k, 1], kp4[k, 2], kp4[k, 3], scale, exp32, entry9)
    return out, bad
