"""CPU tests of the SIFT detector's host layout (gims_sift_layout) and of the NumPy restatement it is checked against
(tests/sift_ref.py): known answers, fastAtan2's error, the octave packing and the recorded OpenCV keypoint counts."""
import os

import numpy as np
import pytest

from gims_amd import hip
from tests import sift_ref as R
from tests.sift_cases import blob as _blob


@pytest.mark.parametrize("h,w", [(480, 640), (680, 850), (517, 333), (640, 800), (12, 16), (9, 9)])
def test_layout_equals_restatement(h, w):
    L = hip.sift_layout(h, w)
    ref = R.layout(h, w)
    assert L.n_octaves == ref["n_octaves"]
    assert [(L.oct_h[o], L.oct_w[o]) for o in range(L.n_octaves)] == ref["sizes"]
    assert list(L.ksize) == ref["ksizes"]
    np.testing.assert_array_equal(np.array(list(L.sigma)), np.array(ref["sigmas"]))
    for i in range(6):
        k = R.gaussian_kernel(ref["ksizes"][i], ref["sigmas"][i])
        r = len(k) // 2
        np.testing.assert_array_equal(np.array(list(L.kernel[i])[:r + 1], np.float32), k[r:])
    off = 0
    for o in range(L.n_octaves):
        hh, ww = ref["sizes"][o]
        assert L.gauss_offset[o] == off and L.dog_offset[o] == off + 6 * hh * ww
        off += 11 * hh * ww
    assert L.image_floats == off and L.scratch_floats == 4 * h * w


def test_layout_known_values():
    assert hip.sift_layout(480, 640).n_octaves == 9                 # cvRound(log2(960) - 2) + 1
    assert list(hip.sift_layout(480, 640).ksize) == [11, 11, 13, 17, 21, 27]
    tiny = hip.sift_layout(12, 16)
    assert tiny.n_octaves == 4 and (tiny.oct_h[0], tiny.oct_w[0]) == (24, 32)
    usable = [o for o in range(tiny.n_octaves) if tiny.oct_h[o] > 10 and tiny.oct_w[o] > 10]
    assert usable == [0, 1]
    one = hip.sift_layout(9, 9)                                      # 18 x 18: one octave with an interior
    assert [o for o in range(one.n_octaves) if one.oct_h[o] > 10 and one.oct_w[o] > 10] == [0]
    with pytest.raises(hip.GimsHipError):
        hip.sift_layout(0, 10)


def test_fast_atan2_within_its_error():
    r = np.random.default_rng(0)
    y, x = r.normal(size=200000).astype(np.float32), r.normal(size=200000).astype(np.float32)
    a = R.fast_atan2(y, x).astype(np.float64)
    ref = np.degrees(np.arctan2(y.astype(np.float64), x.astype(np.float64))) % 360
    d = np.abs(a - ref)
    d = np.minimum(d, 360 - d)
    assert d.max() < 0.01                       # the polynomial's error is about 0.006 degrees
    assert ((a >= 0) & (a < 360)).all()
    assert R.fast_atan2(np.float32(0), np.float32(1)) == 0 and abs(R.fast_atan2(np.float32(1), np.float32(0)) - 90) < 1e-4


def test_isotropic_blob_position_and_size():
    """The doubled image's INTER_LINEAR grid puts OpenCV's keypoints 0.25 px right of and below the true centre (the shift
    enable_precise_upscale removes); a blob of standard deviation s answers the scale-normalised DoG best at scale s, which
    the layer below it reports as s / 2^(1/6); size = 2 * scale."""
    for cx, cy, s in ((40.3, 37.6, 4.0), (41.7, 36.2, 3.0)):
        k = R.detect(_blob(80, 84, cx, cy, s))
        d = np.hypot(k["pt"][:, 0] - (cx + 0.25), k["pt"][:, 1] - (cy + 0.25))
        i = int(np.argmax(k["response"] * (d < 2)))
        assert d[i] < 0.05, d[i]
        assert abs(k["size"][i] / (2 * s * 2 ** (-1 / 6)) - 1) < 0.03, k["size"][i]


def test_packed_octave_round_trips_through_patch_unpacking():
    k = R.detect(_blob(80, 84, 40.3, 37.6, 4.0))
    for packed, size in zip(k["octave"], k["size"]):
        octave, layer = packed & 255, (packed >> 8) & 255
        octave = octave | -128 if octave >= 128 else octave          # patches.hip:keypoint_affine
        xi = ((packed >> 16) & 255) / 255.0 - 0.5
        assert 1 <= layer <= 3 and -1 <= octave
        # size = 1.6 * 2^((layer + xi) / 3) * 2^octave * 2 (with firstOctave = -1 already applied to both)
        assert abs(size / (1.6 * 2 ** ((layer + xi) / 3) * 2.0 ** octave * 2) - 1) < 3e-3


@pytest.mark.parametrize("name,expected", [("graf1", 7848), ("boat1", 15382)])
def test_restatement_count_near_opencv(golden_dir, name, expected):
    img = np.load(os.path.join(golden_dir, f"sift_{name}.npz"))["img"]
    n = len(R.detect(img)["size"])
    assert abs(n - expected) <= 0.01 * expected, n
