"""GPU tests of the SIFT detector (gims_amd/csrc/sift.hip) on tiny, thin, odd-sized, tied and empty images, alone and in batches, against
the NumPy restatement (tests/sift_ref.py).  tests/sift_cases.py builds the images; tests/test_sift_edges_cpu.py shows that they reach what
they are for and caps the restatement's fragile share, which is what bounds the unmatched keypoints here.

Bars (the project's own, as tests/test_sift_gpu.py has them): pyramid 4 * 2^-24 * 256 = 6.1e-5 per pixel; keypoints 1e-3 px, 1e-4 relative
size and response, 0.05 degrees, octave equal; a keypoint only one side has must be fragile on the restatement's side (margin < 1e-3), and
either side may have at most 8 % of the restatement's count unmatched, none when that count is below 25.

Measured on MI355X (2026-10-21).  Pyramid, worst |device - restatement| over every level of every octave against the 6.1e-5 bar: 0.0 in
all 29 cases, the pyramid is bit-identical (octaves, smallest level): 2x2 (1, 4x4), 2x300 (1, 4x600), 2x16384 (1, 4x32768), 3x200
(2, 3x200), 5x64 (2, 5x64), 6x200 (3, 3x100), 8x32 (3, 4x16), 9x33 (3, 4x16), 31x33 (5, 3x4), 32x32 (5, 4x4), 64x64 (6, 4x4), 33x65 (5, 4x8),
63x129 (6, 3x8), 65x127 (6, 4x7), 16x513 (4, 4x128), 12x16384 (4, 3x4096), 16384x12 (4, 4096x3), 128x257 (7, 4x8), 40x56 (5, 5x7); the
noise cases as the blocks cases of their size.
Keypoints, device / restatement / matched / unmatched on either side:
  blocks 2x2, 2x300, 2x16384, 3x200, 5x64, 8x32: 0 / 0 / 0 / 0      6x200: 2 / 2 / 2 / 0        9x33: 4 / 4 / 4 / 0
  31x33: 18 / 18 / 18 / 0          32x32: 22 / 22 / 22 / 0          64x64: 102 / 102 / 102 / 0  33x65: 52 / 52 / 52 / 0
  63x129: 227 / 227 / 227 / 0      65x127: 236 / 236 / 236 / 0      16x513: 120 / 120 / 120 / 0
  12x16384: 2079 / 2079 / 2079 / 0                                  16384x12: 2013 / 2013 / 2013 / 0
  128x257: 961 / 961 / 961 / 0     colour noise 33x65: 2 / 2 / 2 / 0, 65x127: 37 / 37 / 37 / 0, 128x257: 103 / 103 / 103 / 0
  gray noise 2x2, 2x300, 2x16384, 3x200, 5x64: 0 / 0 / 0 / 0        6x200: 4 / 4 / 4 / 0        constant, zero: 0 / 0 / 0 / 0
  blocks8: 40 / 40 / 40 / 0        checker8: 194 / 194 / 194 / 0
so the fragile keypoints the cap allows for (77 of 2079 at 12x16384) all came out on the restatement's side of their decisions here.
Blobs: 0.029 px and 0.016 px from (cx + 0.25, cy + 0.25), size ratios 0.996 and 0.992.  Mixed batch counts [50, 0, 39, 0] gray and
[60, 0, 62, 0] colour; the overflow batch [21, 214, 32].  The file takes 4 s, the slowest test 0.4 s.

Sensitivity (scratch builds of sift.hip, not committed).  refl101 folding once (and clamped, to stay in bounds) instead of taking
i % p: every test_pyramid_equals_restatement case with a varying level narrower than a blur radius fails (23 of 29; of the thin sizes the noise
images only, since a block of 4 is constant down 2 or 3 rows), and both test_pyramid_of_a_batch tests.  The octave-0 destination without
b * stride: both test_pyramid_of_a_batch tests, both test_mixed_batch tests and test_candidate_overflow_in_a_batch fail.  sift_keep_kernel
keeping every filled slot: test_keypoints_equal_restatement fails at the seven sizes whose candidates include duplicates.
"""
import numpy as np
import pytest
import torch

from gims_amd import frontend, hip
from tests import sift_cases as SC
from tests.test_sift_gpu import _match

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = torch.device("cuda")

PYR_BAR = 4 * 2.0 ** -24 * 256
MARGIN_BAR = 1e-3
CAP, SMALL = 0.08, 25
FIELDS = ("pt", "size", "angle", "response", "octave")

NAMES = [n for n, _ in SC.CASES]
IMG = dict(SC.CASES)


def _dev(img):
    """One image [H, W(, 3)] or a batch as a device tensor with a leading batch axis."""
    t = torch.from_numpy(np.ascontiguousarray(img))
    return (t[None] if t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3) else t).to(DEV)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in FIELDS)


def _check_empty(d):
    assert d["pt"].shape == (0, 2) and d["pt"].dtype == torch.float32 and d["pt"].is_cuda
    for k in ("size", "angle", "response"):
        assert d[k].shape == (0,) and d[k].dtype == torch.float32 and d[k].is_cuda, k
    assert d["octave"].shape == (0,) and d["octave"].dtype == torch.int32 and d["octave"].is_cuda


def _check_no_duplicates(d):
    key = np.column_stack([d["pt"], d["size"], d["angle"]])
    assert len(np.unique(key, axis=0)) == len(key)


def _check(d, ref, label):
    """Device keypoints d against the restatement's ref (NumPy dicts) at the bars above; either side may be empty."""
    n_dev, n_ref = len(d["size"]), len(ref["size"])
    assert d["pt"].shape == (n_dev, 2) and d["pt"].dtype == np.float32 and d["octave"].dtype == np.int32
    pairs, lone_dev, lone_ref = _match(d, ref)
    pairs, lone_dev, lone_ref = pairs.astype(np.int64), lone_dev.astype(np.int64), np.asarray(lone_ref, np.int64)
    print(label, "device", n_dev, "restatement", n_ref, "matched", len(pairs), "only device", len(lone_dev), "only restatement", len(lone_ref))
    if len(pairs):
        i, j = pairs[:, 0], pairs[:, 1]
        assert np.abs(d["pt"][i] - ref["pt"][j]).max() <= 1e-3
        assert (np.abs(d["size"][i] - ref["size"][j]) <= 1e-4 * ref["size"][j]).all()
        assert (np.abs(d["response"][i] - ref["response"][j]) <= 1e-4 * ref["response"][j]).all()
        np.testing.assert_array_equal(d["octave"][i], ref["octave"][j])
    assert len(pairs) + len(lone_dev) == n_dev and len(pairs) + len(lone_ref) == n_ref
    # a keypoint only one side has must be one whose deciding comparison sat within the restatement's tolerance margin
    assert (ref["margin"][lone_ref] < MARGIN_BAR).all(), ref["margin"][lone_ref]
    for k in lone_dev:               # its candidate on the restatement's side sits at the same place with a fragile decision
        near = np.abs(ref["pt"] - d["pt"][k]).max(1) < 1.0
        assert near.any() and (ref["margin"][near] < MARGIN_BAR).any(), (k, d["pt"][k])
    allowed = 0 if n_ref < SMALL else int(CAP * n_ref)
    assert len(lone_dev) <= allowed and len(lone_ref) <= allowed, (len(lone_dev), len(lone_ref), allowed)
    _check_no_duplicates(d)
    return len(pairs), len(lone_dev), len(lone_ref)


# ---- a. the pyramid at every case

@pytest.mark.parametrize("name", NAMES)
def test_pyramid_equals_restatement(name):
    """Every Gaussian and DoG level of every octave, those without an interior and the 3-to-5-pixel ones included."""
    img = IMG[name]
    gp, dp, _, _ = SC.reference(name, img)
    gauss, dog = hip.sift_pyramid(_dev(img))
    L = hip.sift_layout(*img.shape[:2])
    assert len(gauss) == len(dog) == 1 and len(gauss[0]) == len(dog[0]) == len(gp) == L.n_octaves
    worst = 0.0
    for o in range(len(gp)):
        assert len(gauss[0][o]) == 6 and len(dog[0][o]) == 5
        for lv, want in list(zip(gauss[0][o], gp[o])) + list(zip(dog[0][o], dp[o])):
            got = lv.cpu().numpy()
            assert got.shape == want.shape == (L.oct_h[o], L.oct_w[o])
            assert np.isfinite(got).all()
            worst = max(worst, float(np.abs(got - want).max()))
    print(name, "octaves", len(gp), "smallest", gp[-1][0].shape, "pyramid max |d|", worst)
    assert worst <= PYR_BAR


# ---- b. the pyramid of a batch

@pytest.mark.parametrize("kind", ["gray", "colour"])
def test_pyramid_of_a_batch_equals_the_single_images(kind):
    batch = SC.batch_gray() if kind == "gray" else SC.batch_colour()
    assert batch.shape[0] == 3 and batch.ndim == (3 if kind == "gray" else 4)
    assert not np.array_equal(batch[0], batch[1]) and not np.array_equal(batch[1], batch[2]) and not np.array_equal(batch[0], batch[2])
    t = _dev(batch)
    gauss, dog = hip.sift_pyramid(t)
    buf = hip.sift_pyramid_buffer(t)
    singles = []
    for b in range(3):
        g1, d1 = hip.sift_pyramid(t[b:b + 1])
        assert len(g1[0]) == len(gauss[b])
        for o in range(len(g1[0])):
            for i in range(6):
                assert torch.equal(gauss[b][o][i], g1[0][o][i]), (b, o, i)
            for i in range(5):
                assert torch.equal(dog[b][o][i], d1[0][o][i]), (b, o, i)
        singles.append(hip.sift_pyramid_buffer(t[b:b + 1]))
    L = hip.sift_layout(*batch.shape[1:3])
    assert buf.numel() == 3 * L.image_floats
    assert torch.equal(buf, torch.cat(singles))
    # and the batch is right, not only consistent: image 1 against the restatement
    gp, dp = SC.reference(f"batch_{kind}_1", batch[1])[:2]
    worst = max(float(np.abs(gauss[1][o][i].cpu().numpy() - gp[o][i]).max()) for o in range(len(gp)) for i in range(6))
    worst = max(worst, max(float(np.abs(dog[1][o][i].cpu().numpy() - dp[o][i]).max()) for o in range(len(dp)) for i in range(5)))
    assert worst <= PYR_BAR


# ---- c. keypoints at every case

@pytest.mark.parametrize("name", NAMES)
def test_keypoints_equal_restatement(name):
    img = IMG[name]
    ref = SC.reference(name, img)[2]
    out = hip.sift_detect(_dev(img))
    assert len(out) == 1
    assert all(out[0][k].is_cuda for k in FIELDS)
    d = _np(out[0])
    _check(d, ref, name)
    if name in SC.EMPTY:
        _check_empty(out[0])


# ---- d. a known answer, independent of the restatement

def test_isotropic_blob_position_and_size_on_the_device():
    """tests/test_sift_cpu.py::test_isotropic_blob_position_and_size through the device, its assertions unchanged: the keypoint sits 0.25 px
    right of and below the true centre, and its size is 2 s 2^(-1/6)."""
    for cx, cy, s in ((40.3, 37.6, 4.0), (41.7, 36.2, 3.0)):
        k = _np(hip.sift_detect(_dev(SC.blob(80, 84, cx, cy, s)))[0])
        d = np.hypot(k["pt"][:, 0] - (cx + 0.25), k["pt"][:, 1] - (cy + 0.25))
        i = int(np.argmax(k["response"] * (d < 2)))
        print("blob", (cx, cy, s), "distance", d[i], "size ratio", k["size"][i] / (2 * s * 2 ** (-1 / 6)))
        assert d[i] < 0.05, d[i]
        assert abs(k["size"][i] / (2 * s * 2 ** (-1 / 6)) - 1) < 0.03, k["size"][i]


# ---- e. a batch that mixes images with and without keypoints

@pytest.mark.parametrize("colour", [False, True], ids=["gray", "colour"])
def test_mixed_batch_equals_the_single_images(colour):
    batch = SC.mixed_batch(colour)
    t = _dev(batch)
    out = hip.sift_detect(t)
    singles = [hip.sift_detect(t[b:b + 1])[0] for b in range(4)]
    counts = [len(o["size"]) for o in out]
    print("mixed batch", "colour" if colour else "gray", "counts", counts)
    assert counts[0] > 0 and counts[2] > 0 and counts[1] == 0 and counts[3] == 0
    for b in range(4):
        assert _same(out[b], singles[b]), b
    _check_empty(out[1])
    _check_empty(out[3])
    # the front end's entry point takes the same batch
    fe = frontend.sift_detect_device(batch, DEV)
    assert all(_same(fe[b], out[b]) for b in range(4))
    # descriptors for the detected keypoints, empty sets included
    desc = frontend.sift_describe_device(batch, out, DEV)
    assert [tuple(x.shape) for x in desc] == [(counts[0], 128), (0, 128), (counts[2], 128), (0, 128)]
    for b in range(4):
        one = frontend.sift_describe_device(batch[b], singles[b], DEV)
        assert desc[b].dtype == one.dtype == torch.float32 and torch.equal(desc[b], one), b
    assert float(desc[0].sum()) > 0 and float(desc[2].sum()) > 0


@pytest.mark.parametrize("colour", [False, True], ids=["gray", "colour"])
def test_batch_of_constants_is_four_empty_results(colour):
    batch = np.stack([SC.constant(*SC.FLAT, v, 3 if colour else 1) for v in (0, 93, 255, 17)])
    out = hip.sift_detect(_dev(batch))
    assert len(out) == 4
    for d in out:
        _check_empty(d)
    out = hip.sift_detect(_dev(batch), cand_cap=1)
    assert len(out) == 4
    for d in out:
        _check_empty(d)


# ---- f. candidate overflow in a batch

def _caps_agree(t):
    """Detection of the batch t with candidate capacities 1, 7, 1000, the default and half the default: the same bytes in every field.
    1 and 7 cannot hold the candidates, so the buffers grow and the call repeats; 1000 may or may not; half the default shows that the
    result does not hang on the default capacity."""
    B, H, W = t.shape[:3]
    default = B * max(4096, H * W // 16)
    full = hip.sift_detect(t)
    for cap in (1, 7, 1000, default // 2):
        got = hip.sift_detect(t, cand_cap=cap)
        assert len(got) == len(full)
        for b in range(B):
            assert _same(got[b], full[b]), (cap, b)
    return full


def test_candidate_overflow_in_a_batch():
    t = _dev(SC.batch_colour())
    full = _caps_agree(t)
    counts = [len(o["size"]) for o in full]
    print("overflow batch counts", counts)
    assert min(counts) > 0 and sum(counts) > 7          # every image has keypoints, and 1 and 7 candidates cannot hold them
    for b in range(3):
        assert _same(full[b], hip.sift_detect(t[b:b + 1])[0]), b


# ---- g. exact ties and the order of the candidates

@pytest.mark.parametrize("name", ["blocks8", "checker8"])
def test_ties_and_candidate_order(name):
    img = dict(SC.tie_images())[name]
    t = _dev(img)
    a = _caps_agree(t)[0]
    b = hip.sift_detect(t)[0]
    assert _same(a, b)
    d = _np(a)
    _check_no_duplicates(d)
    n, _, _ = _check(d, SC.reference(name, img)[2], name)
    assert n >= SMALL
