"""Colour augmentation, host side (no GPU): known answers written out by hand for the NumPy restatement tests/aug_ref.py AND for the
product's own host code (gims_amd/augment.py: table, line kernel), the statistics of ColorAug.draw() and of the noise generator, the
plan struct against the header, and the documented draw order."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from gims_amd import ColorAug, ColorAugPlan, augment, hip
from tests import aug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240611          # the statistics below hold for this seed (checked before it was committed); the bounds are 5 standard errors


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("make", [R.lut, augment.brightness_contrast_lut], ids=["ref", "product"])
def test_lut_known_answers(make):
    assert np.array_equal(make(1.0, 0.4), np.minimum(255, np.arange(256) + 102))             # float32(0.4 * 255) = 102
    assert np.array_equal(make(1.0, -0.4), np.maximum(0, np.arange(256) - 102))
    lo = make(0.7, 0.0)       # i * float32(0.7): 0.7, 1.4, 2.1 truncate; 10 * 0.7f rounds to 7.0 in float32; 178.5 truncates
    assert [int(lo[i]) for i in (0, 1, 2, 3, 10, 255)] == [0, 0, 1, 2, 7, 178]
    hi = make(1.3, 0.0)       # 196 * 1.3 = 254.8 truncates, 197 * 1.3 = 256.1 clips
    assert [int(hi[i]) for i in (0, 1, 196, 197, 255)] == [0, 1, 254, 255, 255]
    assert np.array_equal(make(1.0, 0.0), np.arange(256))


def _cells(k):
    return sorted((int(x), int(y)) for y, x in zip(*np.nonzero(k)))


@pytest.mark.parametrize("make", [R.line_kernel, augment.line_kernel], ids=["ref", "product"])
def test_line_kernel_known_answers(make):
    cases = [((7, 0, 3, 6, 3), [(x, 3) for x in range(7)]),                                   # horizontal
             ((7, 2, 6, 2, 0), [(2, y) for y in range(7)]),                                   # vertical, drawn upwards
             ((7, 0, 0, 6, 6), [(i, i) for i in range(7)]),                                   # diagonal
             ((7, 0, 6, 6, 0), [(i, 6 - i) for i in range(7)]),                               # anti-diagonal
             ((7, 0, 0, 6, 2), [(0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 2), (6, 2)]),     # y = x / 3 rounded: no ties
             ((7, 6, 2, 0, 0), [(0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 2), (6, 2)]),     # the same line from its other end
             ((3, 0, 0, 2, 1), [(0, 0), (1, 1), (2, 1)]),                                     # y = 0.5 at x = 1: towards the end point
             ((3, 2, 1, 0, 0), [(0, 0), (1, 0), (2, 1)]),
             ((3, 0, 0, 1, 0), [(0, 0), (1, 0)])]
    for args, cells in cases:
        k = make(*args)
        assert k.dtype == np.float32 and k.shape == (args[0], args[0])
        assert _cells(k) == sorted(cells), args
        assert (k[k != 0] == np.float32(1) / np.float32(len(cells))).all()


def test_line_kernels_agree_for_every_pair_of_end_points():
    for k in (3, 5, 7):
        pts = [(x, y) for x in range(k) for y in range(k)]
        for (xs, ys) in pts:
            for (xe, ye) in pts:
                if (xs, ys) != (xe, ye):
                    assert np.array_equal(augment.line_kernel(k, xs, ys, xe, ye), R.line_kernel(k, xs, ys, xe, ye)), (k, xs, ys, xe, ye)


def test_reflect101_known_answers():
    assert [R.reflect101(p, 1) for p in range(-3, 4)] == [0] * 7
    assert [R.reflect101(p, 2) for p in range(-3, 5)] == [1, 0, 1, 0, 1, 0, 1, 0]
    assert [R.reflect101(p, 3) for p in range(-3, 6)] == [1, 2, 1, 0, 1, 2, 1, 0, 1]


def test_blur_known_answers():
    img = np.array([[10, 13, 20, 40, 80]], dtype=np.uint8).reshape(1, 5, 1)
    two = R.line_kernel(3, 0, 1, 1, 1)                  # taps at x - 1 and x, 0.5 each: ties go to the even value
    assert R.blur(img, two).reshape(-1).tolist() == [12, 12, 16, 30, 60]      # (13 + 10) / 2 = 11.5 -> 12, 11.5 -> 12, 16.5 -> 16
    img = np.arange(35, dtype=np.uint8).reshape(5, 7, 1) * 7
    k = R.line_kernel(3, 0, 0, 2, 2)                    # the diagonal: mean of (y-1, x-1), (y, x), (y+1, x+1)
    out = R.blur(img, k)
    assert out[2, 3, 0] == img[2, 3, 0]                 # a linear ramp is its own mean
    assert out[0, 0, 0] == round((int(img[1, 1, 0]) * 2 + int(img[0, 0, 0])) / 3)      # (-1, -1) reflects to (1, 1)


def test_noise_z_known_answers():
    """S worked out with Python integers from the specification (splitmix64(0) = 0xE220A8397B1DCDAF is the generator's published first value)."""
    assert int(R.splitmix64(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF
    for key, e, s in [(0, 0, 439213), (0x0123456789ABCDEF, 1, 399878), (0xFFFFFFFFFFFFFFFF, 921599, 399551)]:
        z = R.noise_z(key, [e])
        assert z.dtype == np.float32 and float(z[0]) == (s - 393210) / 65536.0


# ------------------------------------------------------------------------------------------------ statistics
def _within(count, n, p, what):
    se = np.sqrt(p * (1 - p) / n)
    assert abs(count / n - p) <= 5 * se, (what, count / n, p, se)


def test_plan_statistics():
    aug = ColorAug(rng=np.random.RandomState(SEED))
    plans = [aug.draw() for _ in range(20000)]
    applied = [p for p in plans if p.applied]
    assert all(p.empty for p in plans if not p.applied)
    _within(len(applied), len(plans), 0.65, "applied")
    _within(sum(p.empty for p in plans), len(plans), 0.35 + 0.65 * 0.4 * 0.5, "empty")
    n = len(applied)
    _within(sum(p.lut_kind == "brightness" for p in applied), n, 0.6 * 6 / 13, "brightness")
    _within(sum(p.lut_kind == "contrast" for p in applied), n, 0.6 * 7 / 13, "contrast")
    _within(sum(p.lut_kind is None for p in applied), n, 0.4, "no lut")
    blurs = [p for p in applied if p.ksize]
    _within(len(blurs), n, 0.5 * 5 / 11, "blur")
    _within(sum(p.sigma > 0 for p in applied), n, 0.5 * 6 / 11, "noise")
    _within(sum(p.ksize == 0 and not p.sigma > 0 for p in applied), n, 0.5, "neither")
    assert not any(p.ksize and p.sigma > 0 for p in plans)
    for k in (3, 5, 7):
        _within(sum(p.ksize == k for p in blurs), len(blurs), 1 / 3, f"ksize {k}")
    # the ranges of the parameters
    assert all(-0.4 <= p.beta <= 0.4 and p.alpha == 1 for p in applied if p.lut_kind == "brightness")
    assert all(0.7 <= p.alpha <= 1.3 and p.beta == 0 for p in applied if p.lut_kind == "contrast")
    assert all(np.float32(np.sqrt(10)) <= p.sigma <= np.float32(np.sqrt(50)) and 0 <= p.key < 2 ** 64 for p in applied if p.sigma > 0)
    assert all(p.line[0] != p.line[1] and 0 <= min(min(p.line)) and max(max(p.line)) < p.ksize for p in blurs)
    assert len({p.key for p in applied if p.sigma > 0}) == sum(p.sigma > 0 for p in applied)


def test_noise_statistics_of_the_restatement():
    img = np.full((96, 96, 3), 128, dtype=np.uint8)
    sigma = np.float32(np.sqrt(50))
    out = R.noise(img, sigma, 0x5DEECE66D1234567)
    d = out.astype(np.float64) - 128          # floor(sigma z): no clipping at 6 sigma = 42
    assert out.min() > 0 and out.max() < 255
    n = d.size
    var = 50 + 1 / 12
    assert abs(d.mean() + 0.5) <= 5 * np.sqrt(var / n), d.mean()
    m2 = d.var()
    kurt = ((d - d.mean()) ** 4).mean() / m2 ** 2 - 3
    assert abs(m2 - var) <= 5 * var * np.sqrt((2 - 0.1) / n), m2        # var(s^2) = sigma^4 (kurtosis_excess + 2) / n
    assert -0.25 <= kurt <= 0.05, kurt
    # channels of one image, and images under different keys, all differ
    other = R.noise(img, sigma, 0x5DEECE66D1234568)
    planes = [out[:, :, c] for c in range(3)] + [other[:, :, c] for c in range(3)]
    for i in range(len(planes)):
        for j in range(i + 1, len(planes)):
            assert (planes[i] != planes[j]).mean() > 0.9, (i, j)
    assert np.array_equal(R.noise(img, sigma, 0x5DEECE66D1234567), out)


# ------------------------------------------------------------------------------------------------ struct, draw order
def test_plan_struct_layout_matches_header(tmp_path):
    fields = ["lut", "kernel", "use_lut", "ksize", "sigma", "key"]
    body = 'printf("size %zu\\n", sizeof(gims_aug_plan));\n' + "".join('printf("%s %%zu\\n", offsetof(gims_aug_plan, %s));\n' % (f, f) for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gims_hip.h"\nint main(void) {\n' + body + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(hip.AugPlan) == 472
    for f in fields:
        assert int(got[f]) == getattr(hip.AugPlan, f).offset, f
    assert {"gims_color_aug", "gims_color_aug_workspace_bytes"} <= set(hip.EXPORTS)
    assert hip.load().gims_color_aug_workspace_bytes(3) == 1424 and hip.load().gims_color_aug_workspace_bytes(0) == 0


class _Counting:
    """A RandomState that lists the calls made on it."""

    def __init__(self, seed):
        self._r, self.calls = np.random.RandomState(seed), []

    def __getattr__(self, name):
        fn = getattr(self._r, name)

        def call(*a, **k):
            self.calls.append(name)
            return fn(*a, **k)
        return call


def _documented_calls(p):
    if not p.applied:
        return ["uniform"]
    calls = ["uniform", "uniform"] + (["choice", "uniform"] if p.lut_kind else []) + ["uniform"]
    if p.ksize:
        calls += ["choice", "choice", "randint", "randint"] + (["choice"] if p.line[0][0] == p.line[1][0] else ["randint", "randint"])
    elif p.sigma > 0:
        calls += ["choice", "uniform", "randint"]
    return calls


def test_draw_is_reproducible_and_makes_the_documented_calls():
    a, b = ColorAug(rng=np.random.RandomState(7)), ColorAug(rng=np.random.RandomState(7))
    assert [repr(a.draw()) for _ in range(300)] == [repr(b.draw()) for _ in range(300)]
    rng = _Counting(7)
    aug = ColorAug(rng=rng)
    seen = set()
    for _ in range(2000):
        del rng.calls[:]
        p = aug.draw()
        assert rng.calls == _documented_calls(p), (p, rng.calls)
        seen.add((p.applied, p.lut_kind, p.ksize > 0, bool(p.sigma > 0), bool(p.ksize and p.line[0][0] == p.line[1][0])))
    assert len(seen) == 1 + 3 * 4        # not applied; {no lut, brightness, contrast} x {nothing, noise, blur, blur with xs == xe}
    # rng=None draws from the global generator, like the homography draws
    np.random.seed(7)
    g = ColorAug()
    assert [repr(g.draw()) for _ in range(50)] == [repr(p) for p in _replay(7, 50)]


def _replay(seed, n):
    aug = ColorAug(rng=np.random.RandomState(seed))
    return [aug.draw() for _ in range(n)]


def test_plan_to_c_carries_table_kernel_and_key():
    p = ColorAugPlan(applied=True, lut_kind="contrast", alpha=1.3, ksize=5, line=((0, 0), (4, 2)))
    c = p.to_c()
    assert c.use_lut == 1 and bytes(c.lut) == R.lut(1.3, 0).tobytes() and c.ksize == 5 and c.sigma == 0
    assert np.array_equal(np.array(c.kernel[:25], dtype=np.float32).reshape(5, 5), R.line_kernel(5, 0, 0, 4, 2)) and not any(c.kernel[25:])
    q = ColorAugPlan(applied=True, sigma=np.float32(np.sqrt(10)), key=0xFEDCBA9876543210).to_c()
    assert q.use_lut == 0 and q.ksize == 0 and q.key == 0xFEDCBA9876543210 and np.float32(q.sigma) == np.float32(np.sqrt(10))
    assert ColorAugPlan().empty and not p.empty
    with pytest.raises(ValueError):
        ColorAug(blur_limit=(8, 9))
