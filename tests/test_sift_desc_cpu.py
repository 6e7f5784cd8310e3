"""CPU tests of the SIFT descriptor stage: the ABI constant and the argument checks of GIMS_AUX_SIFT_DESCRIBE (they run before any HIP
call), the pins a feature must leave alone, properties of the NumPy restatement (tests/sift_desc_ref.py), ``frontend.root_sift`` and
the discrimination fixture the GPU test compares against."""
import ctypes as C

import numpy as np
import torch

from gims_amd import frontend, hip, synth
from tests import nn_ref, sift_desc_ref as DR, sift_ref as R

F = np.float32
H, W = 96, 128


def _kp4(k):
    return np.concatenate([k["pt"], k["size"][:, None], k["angle"][:, None]], 1).astype(F)


_CACHE = {}


def _small():
    """(img, gp, detected keypoints) of the 96 x 128 synthetic image."""
    if "small" not in _CACHE:
        img = synth.make_textured_image(H, W, 9)
        gp, dp = R.pyramid(img)
        _CACHE["small"] = (img, gp, R.detect_from_pyramid(gp, dp))
    return _CACHE["small"]


def test_abi_constant_and_pins():
    assert hip.AUX_SIFT_DESCRIBE == 6 == hip.ABI.constants["GIMS_AUX_SIFT_DESCRIBE"]
    # the descriptor stage adds no export, no struct and no ABI version
    assert len(hip.EXPORTS) == 90 and len(hip.ABI.structs) == 28 and hip.ABI_VERSION == 5 == hip.load().gims_abi_version()
    assert not any("describe" in name for name in hip.EXPORTS)


def _run(ptrs, ints):
    lib = hip.load()
    ops = hip.make_ops([hip.op_aux(hip.AUX_SIFT_DESCRIBE, ptrs, ints)])
    return lib.gims_run_ops(ops, 1, None), lib.gims_last_error()


def test_argument_checks_come_before_any_hip_call():
    """Every GIMS_EINVAL case of the header, with a message; the pointers are never dereferenced (no device is needed)."""
    p = [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000]          # pyr, kp4, octave, image, out, bad
    good = [5, 1, H, W, 128, 0]                                   # n, n_images, h, w, ld, reserved

    def refused(ptrs, ints, word):
        rc, msg = _run(ptrs, ints)
        assert rc == hip.GIMS_EINVAL and b"sift_describe" in msg and word in msg, (rc, msg)

    for k in (0, 1, 2, 4, 5):                                     # a null pyr / kp4 / octave / out / bad while n > 0
        refused([None if j == k else v for j, v in enumerate(p)], good, b"NULL")
    refused(p, [-1] + good[1:], b"n = -1")
    refused(p, [5, 0, H, W, 128, 0], b"n_images")
    refused([p[0], p[1], p[2], None, p[4], p[5]], [5, 2, H, W, 128, 0], b"image index")
    refused(p, [5, 1, 0, W, 128, 0], b"image size")
    refused(p, [5, 1, H, 20000, 128, 0], b"image size")
    refused(p, [5, 1, H, W, 127, 0], b"ld = 127")
    refused(p, [5, 1, H, W, 128, 1], b"reserved")
    # n == 0 is fine and touches nothing, even with null pointers; its other arguments are still checked
    assert _run([None] * 6, [0, 1, H, W, 128, 0])[0] == hip.GIMS_OK
    refused([None] * 6, [0, 1, H, W, 64, 0], b"ld = 64")


def test_restatement_flat_image_gives_zeros():
    gp, _ = R.pyramid(np.full((64, 80), 77, np.uint8))
    d, bad = DR.describe(gp, [[40, 30, 6, 10], [3.5, 2.5, 20, 300]], [(1 << 8) | 255, 2 << 8])
    assert bad == 0 and d.shape == (2, 128) and not d.any()


def test_restatement_outputs_are_bytes_and_borders_stay_in_bounds():
    img, gp, k = _small()
    kp4, octv = _kp4(k), k["octave"]
    assert len(kp4) > 30
    extra = np.array([[0, 0, 8, 45], [W - 1, H - 1, 8, 200], [W - 0.6, 0.2, 30, 0], [-3, H + 2, 5, 90]], F)      # on and past the border
    d, bad = DR.describe(gp, np.concatenate([kp4, extra]), np.concatenate([octv, [1 << 8, (2 << 8) | 255, (3 << 8) | 1, 1 << 8]]))
    assert bad == 0 and d.dtype == np.float32
    assert (d == np.rint(d)).all() and d.min() >= 0 and d.max() <= 255
    assert (d[:len(kp4)].sum(1) > 0).all()                       # a textured image: no empty descriptor among the detections


def test_restatement_padded_keypoint_radius_and_bad_levels():
    img, gp, _ = _small()
    pk = frontend.PaddedKeyPoint(50.2, 40.7)                     # cv2.KeyPoint(x, y, 1): size 1, angle -1, octave 0
    kp4, octv, _ = frontend.keypoint_arrays([pk])
    o, layer, scale = DR.unpack_octave(octv[0])
    assert (o, layer, float(scale)) == (0, 0, 1.0)
    rows, cols = gp[1][0].shape
    assert (rows, cols) == (H, W) and DR.radius_of(pk.size, scale, rows, cols) == 5          # cvRound(1.5 * 1.4142135 * 2.5) = cvRound(5.30)
    d, bad = DR.describe(gp, kp4, octv)
    assert bad == 0 and d.any()
    # the top octave's levels are a few pixels: the diagonal clamp takes over
    top = len(gp) - 1
    th, tw = gp[top][0].shape
    assert DR.radius_of(400.0, F(1) / F(1 << (top - 1)), th, tw) == int(np.sqrt(th * th + tw * tw)) < 10
    # octave or layer outside the pyramid: zeros, counted
    n_oct = len(gp)
    d, bad = DR.describe(gp, np.tile(kp4, (4, 1)), [octv[0], n_oct - 1, 6 << 8, 254])            # fine, octave past the top, layer 6, octave -2
    assert bad == 3 and d[0].any() and not d[1:].any()


def test_restatement_angle_minus_one_votes_into_entry_nine():
    """PaddedKeyPoint has angle -1, so ori = 361 and a gradient direction below 1 degree gives o0 = -9 + 8 = -1: the sample votes at
    idx - 1, orientation entry 9 of the cell before, which the fold adds to that cell's entry 1.  Some of 400 seeded padded keypoints
    must do so (24 here), none of the same keypoints with angle 0 may, and descriptors stay bytes."""
    img, gp, _ = _small()
    rng = np.random.default_rng(17)
    kp4 = np.stack([rng.random(400) * W, rng.random(400) * H, np.ones(400), -np.ones(400)], 1).astype(F)
    e9, e9_zero = [], []
    d, bad = DR.describe(gp, kp4, np.zeros(400, np.int32), entry9=e9)
    kp4[:, 3] = 0
    DR.describe(gp, kp4, np.zeros(400, np.int32), entry9=e9_zero)
    print("padded keypoints with a share in entry 9:", int((np.array(e9) > 0).sum()))
    assert bad == 0 and (np.array(e9) > 0).sum() >= 10 and not np.array(e9_zero).any()
    assert (d == np.rint(d)).all() and d.min() >= 0 and d.max() <= 255


def test_root_sift_equals_the_reference_formula():
    rng = np.random.default_rng(5)
    d = np.rint(rng.random((50, 128)) * 255).astype(F)
    d[3] = 0                                                     # an empty descriptor: eps keeps it finite
    for l2 in (False, True):
        want = DR.root_sift(d, 1e-7, l2)
        got = frontend.root_sift(torch.from_numpy(d.copy()), 1e-7, l2).numpy()
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose((DR.root_sift(d)[[0, 1, 2, 4]] ** 2).sum(1), 1.0, rtol=1e-5)      # L1-normalised, then the root: unit L2 norm
    assert torch.equal(frontend.root_sift(torch.from_numpy(d))[3], torch.zeros(128))


def _pair_results():
    if "pair" not in _CACHE:
        img0, img1, Hm = DR.warped_pair()
        side = []
        for img in (img0, img1):
            gp, dp = R.pyramid(img)
            k = R.detect_from_pyramid(gp, dp)
            d, bad = DR.describe(gp, _kp4(k), k["octave"])
            assert bad == 0
            side.append((gp, k, d))
        _CACHE["pair"] = (side, Hm)
    return _CACHE["pair"]


def test_descriptors_discriminate_on_a_warped_pair():
    """The fixture of the GPU end-to-end test: make_textured_image(240, 320, 7) and its warp by make_homography(21, strength 0.3).
    Restatement detect + describe, RootSIFT, mutual nearest neighbours at 0.8: 246 matches, 244 of them within 3 px of the ground truth
    (precision 0.9919); the bar is 90 %."""
    (s0, s1), Hm = _pair_results()
    out = nn_ref.solve(DR.root_sift(s0[2]).T, DR.root_sift(s1[2]).T, 0.8, True)
    n, ok = DR.count_correct(s0[1]["pt"], s1[1]["pt"], out["matches0"], Hm)
    print("matches", n, "correct", ok, "precision", ok / n, "keypoints", len(s0[2]), len(s1[2]))
    assert ok >= 0.9 * n and n >= 100
    assert (n, ok) == (DR.PAIR_RECORD["matches"], DR.PAIR_RECORD["correct"])


def test_float32_exp_changes_almost_no_descriptor():
    """How much hangs on exp being taken in double: with a float32 exp instead, 0 of the pair's 681 descriptors change (measured here);
    the device-against-restatement cap is 1 %, and a transcendental that differs in its last bit must stay well under it."""
    (s0, s1), _ = _pair_results()
    changed = total = 0
    for gp, k, d in (s0, s1):
        e, _ = DR.describe(gp, _kp4(k), k["octave"], exp32=True)
        assert np.abs(e - d).max() <= 1
        changed += int((e != d).any(1).sum())
        total += len(d)
    print("descriptors changed by a float32 exp:", changed, "of", total)
    assert changed <= 0.002 * total
