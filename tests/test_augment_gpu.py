"""Colour augmentation on the device (csrc/augment.hip, gims_amd/augment.py) against the NumPy restatement tests/aug_ref.py, bit for bit:
every operation and every pair of operations at shapes that reach each path of the kernel (one pixel, images narrower than the kernel
radius, unaligned rows, tile borders with a one-byte tail, tiles staged by aligned dwords, the training size), clipping, rounding ties,
batches, the argument checks, and training_pair with and without the augmentation."""
import numpy as np
import pytest
import torch

from gims_amd import ColorAug, ColorAugPlan, hip, synth
from gims_amd import homography as HG
from tests import aug_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
AUG = dict(patch_ratio=0.85, perspective_x=0.0, perspective_y=0.0, shear_ratio=0.04, shear_angle=10, rotation_angle=25, scale=0.6,
           translation=0.6)
PARAMS = dict(image_height=480, image_width=640, resize_aspect=False, augmentation_params=AUG, apply_color_aug=True)
SIG = np.float32(np.sqrt(37.5))


def _plan(lut=None, value=0.0, line=None, ksize=0, sigma=0.0, key=0):
    kw = dict(beta=value) if lut == "brightness" else (dict(alpha=value) if lut == "contrast" else {})
    return ColorAugPlan(applied=True, lut_kind=lut, ksize=ksize, line=line, sigma=sigma, key=key, **kw)


BLURS = [(3, ((0, 0), (2, 1))), (3, ((0, 1), (1, 1))), (5, ((4, 0), (0, 3))), (5, ((2, 0), (2, 4))), (7, ((0, 0), (6, 6))), (7, ((6, 1), (0, 4))),
         (7, ((0, 3), (6, 3)))]
SINGLE = ([_plan("brightness", 0.27), _plan("contrast", 0.74), _plan("brightness", -0.31), _plan("contrast", 1.29)] +
          [_plan(ksize=k, line=l) for k, l in BLURS] + [_plan(sigma=SIG, key=0x9E3779B97F4A7C15), _plan(sigma=np.float32(np.sqrt(10)), key=1)])
DOUBLE = [_plan("brightness", 0.27, ksize=7, line=((6, 1), (0, 4))), _plan("contrast", 1.29, ksize=5, line=((4, 0), (0, 3))),
          _plan("contrast", 0.74, ksize=3, line=((0, 0), (2, 1))), _plan("brightness", -0.31, sigma=SIG, key=0xDEADBEEFCAFEF00D),
          _plan("contrast", 1.29, sigma=np.float32(np.sqrt(50)), key=2 ** 64 - 1)]
ALL = SINGLE + DOUBLE + [ColorAugPlan()]
# the training size adds only the tiles staged by aligned dwords at a row shift of 3 and the wide byte path at scale; the small shapes
# carry every operation, so a table with a blur, a table with noise and a plain blur are enough here
LARGE = [DOUBLE[0], DOUBLE[4], SINGLE[6]]

# (40, 135, 3) adds to the shapes of the issue the only small colour image with a tile that is staged by aligned dwords at an odd row pitch
SHAPES = [(1, 1, 1), (2, 3, 3), (5, 7, 3), (37, 53, 3), (64, 257, 1), (40, 135, 3), (480, 640, 3)]


def _images(n, h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, c), dtype=np.uint8)


def _run(images, plans):
    return ColorAug().apply(torch.from_numpy(images).to(DEV), plans).cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_operation_equals_the_restatement(shape):
    h, w, c = shape
    plans = LARGE if h * w > 100000 else ALL
    images = _images(len(plans), h, w, c, h * 1000 + w)
    got = _run(images, plans)
    assert got.shape == images.shape and got.dtype == np.uint8
    for i, p in enumerate(plans):
        want = R.apply_plan(images[i], p)
        assert np.array_equal(got[i], want), (shape, p, int((got[i] != want).sum()))
        if not p.empty and h * w > 1:
            assert not np.array_equal(got[i], images[i]), p


def test_clipping_truncation_and_rounding_ties():
    h, w = 33, 70
    noise = [_plan(sigma=np.float32(np.sqrt(50)), key=77), _plan(sigma=np.float32(np.sqrt(50)), key=78)]
    flat = np.stack([np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)])
    got = _run(flat, noise)
    for i in range(2):
        assert np.array_equal(got[i], R.apply_plan(flat[i], noise[i]))
    assert (got[0] == 0).mean() > 0.5 and got[0].max() > 20 and (got[1] == 255).mean() > 0.45 and got[1].min() < 235      # v in (-1, 0) truncates to 0 too
    yy, xx = np.mgrid[:h, :w]
    odd = ((yy + xx) & 1).astype(np.uint8)[:, :, None].repeat(3, 2)
    # 0 / 255 under the ksize-7 diagonal (seven equal taps of float32(1 / 7): the chain must land on 255 again), then two-tap and four-tap
    # lines over cells that differ by an odd number: every pixel is an exact x.5, rounded to even
    boards = np.stack([odd * 255, 10 + 3 * odd, 11 + 3 * odd, 200 + odd * 55, (yy * w + xx).astype(np.uint8)[:, :, None].repeat(3, 2)])
    plans = [_plan(ksize=7, line=((0, 0), (6, 6))), _plan(ksize=3, line=((0, 1), (1, 1))), _plan(ksize=3, line=((1, 0), (1, 1))),
             _plan(ksize=7, line=((0, 3), (1, 3))), _plan(ksize=7, line=((1, 1), (4, 1)))]
    got = _run(boards, plans)
    for i in range(len(plans)):
        assert np.array_equal(got[i], R.apply_plan(boards[i], plans[i])), plans[i]
    assert np.array_equal(got[0], boards[0])
    assert (got[1] == 12).all() and (got[2] == 12).all()            # 11.5 -> 12 and 12.5 -> 12


def test_batch_equals_one_image_at_a_time_and_runs_are_identical():
    plans = [ALL[0], ALL[5], ColorAugPlan(), ALL[11], DOUBLE[0], DOUBLE[3]]
    images = _images(6, 37, 53, 3, 5)
    dev = torch.from_numpy(images).to(DEV)
    aug = ColorAug()
    got = aug.apply(dev, plans)
    for i, p in enumerate(plans):
        assert torch.equal(aug.apply(dev[i], p), got[i]), p                                   # a single [h, w, 3] image
    assert torch.equal(got[2], dev[2]) and torch.equal(aug.apply(dev, plans), got)
    assert torch.equal(dev.cpu(), torch.from_numpy(images))
    # grey images without a channel axis: a batch [n, h, w] and one image [h, w]
    grey = dev[:, :, :, 0].contiguous()
    g = aug.apply(grey, plans)
    assert g.shape == grey.shape and torch.equal(g, aug.apply(grey.unsqueeze(-1), plans).squeeze(-1))
    assert np.array_equal(aug.apply(grey[4], plans[4]).cpu().numpy(), R.apply_plan(images[4, :, :, 0], plans[4]))
    # a different key is different noise
    other = ColorAugPlan(applied=True, lut_kind="brightness", beta=-0.31, sigma=SIG, key=0xDEADBEEFCAFEF00E)
    assert (aug.apply(dev[5], other) != got[5]).float().mean() > 0.5


def test_all_empty_batch_is_a_copy_and_drawn_plans_follow_the_generator():
    images = torch.from_numpy(_images(3, 20, 31, 3, 9)).to(DEV)
    out = ColorAug().apply(images, [ColorAugPlan()] * 3)
    assert torch.equal(out, images) and out.data_ptr() != images.data_ptr()
    out = hip.color_aug(images, [ColorAugPlan().to_c()] * 3)                                    # the library's own copy path
    assert torch.equal(out, images) and out.data_ptr() != images.data_ptr()
    assert hip.color_aug(images[:0], []).shape == (0, 20, 31, 3)
    replay = ColorAug(rng=np.random.RandomState(9))
    plans = [replay.draw() for _ in range(3)]
    assert [p.empty for p in plans] == [False, False, True] and plans[0].ksize == 3 and plans[1].sigma > 0
    got = ColorAug(rng=np.random.RandomState(9)).apply(images)
    for i in range(3):
        assert np.array_equal(got[i].cpu().numpy(), R.apply_plan(images[i].cpu().numpy(), plans[i]))


@pytest.mark.parametrize("so,do", [(0, 0), (5, 5), (3, 9)])
def test_misaligned_buffers(so, do):
    """Source and destination at any byte offset: aligned alike (wide accesses after a scalar head) or differently (byte by byte)."""
    images = _images(2, 37, 53, 3, 21)
    n = images.size
    src = torch.zeros(n + 32, dtype=torch.uint8, device=DEV)
    dst = torch.full((n + 32,), 0xAB, dtype=torch.uint8, device=DEV)
    s = src[so:so + n].view(images.shape)
    s.copy_(torch.from_numpy(images))
    plans = [DOUBLE[3], DOUBLE[0]]
    hip.color_aug(s, [p.to_c() for p in plans], out=dst[do:do + n].view(images.shape))
    got = dst.cpu().numpy()
    assert (got[:do] == 0xAB).all() and (got[do + n:] == 0xAB).all()
    for i in range(2):
        assert np.array_equal(got[do:do + n].reshape(images.shape)[i], R.apply_plan(images[i], plans[i]))


def test_argument_errors_leave_the_input_untouched():
    host = _images(1, 8, 9, 3, 2)
    images = torch.from_numpy(host).to(DEV)
    ok = _plan(ksize=3, line=((0, 0), (2, 2))).to_c()
    with pytest.raises(hip.GimsHipError, match="overlaps"):
        hip.color_aug(images, [ok], out=images)
    two = torch.from_numpy(_images(1, 8, 9, 2, 3)).to(DEV)
    keep = two.clone()
    with pytest.raises(hip.GimsHipError, match="channels"):
        hip.color_aug(two, [ok])
    bad = _plan(ksize=3, line=((0, 0), (2, 2))).to_c()
    bad.ksize = 4
    with pytest.raises(hip.GimsHipError, match="ksize"):
        hip.color_aug(images, [bad])
    both = _plan(ksize=3, line=((0, 0), (2, 2))).to_c()
    both.sigma = 3.0
    with pytest.raises(hip.GimsHipError, match="both"):
        hip.color_aug(images, [both])
    with pytest.raises(ValueError):
        hip.color_aug(images, [ok, ok])
    assert torch.equal(images.cpu(), torch.from_numpy(host)) and torch.equal(two, keep)
    assert np.array_equal(hip.color_aug(images, [ok]).cpu().numpy()[0], R.apply_plan(host[0], _plan(ksize=3, line=((0, 0), (2, 2)))))


def test_training_pair_with_and_without_the_augmentation():
    img = synth.make_textured_image(427, 640, 500)
    np.random.seed(31)
    i0, w0, h0 = HG.training_pair(img, PARAMS)
    after = np.random.uniform()
    np.random.seed(31)
    i1, w1, h1 = HG.training_pair(img, PARAMS, color_aug=None)
    assert torch.equal(i0, i1) and torch.equal(w0, w1) and np.array_equal(h0, h1) and np.random.uniform() == after
    replay = ColorAug(rng=np.random.RandomState(21))
    plans = [replay.draw(), replay.draw()]              # contrast + ksize-7 blur for the original, contrast + noise for the warped image
    assert plans[0].ksize == 7 and plans[0].lut_kind and plans[1].sigma > 0 and plans[1].lut_kind
    np.random.seed(31)
    i2, w2, h2 = HG.training_pair(img, PARAMS, color_aug=ColorAug(rng=np.random.RandomState(21)))
    assert np.array_equal(h2, h0) and np.random.uniform() == after
    assert i2.shape == i0.shape == (480, 640, 3) and i2.dtype == torch.uint8 and i2.is_cuda
    assert np.array_equal(i2.cpu().numpy(), R.apply_plan(i0.cpu().numpy(), plans[0]))
    assert np.array_equal(w2.cpu().numpy(), R.apply_plan(w0.cpu().numpy(), plans[1]))
    # the global generator: the colour draws come after the homography's, which therefore stays the same
    np.random.seed(31)
    i3, w3, h3 = HG.training_pair(img, PARAMS, color_aug=ColorAug())
    assert np.array_equal(h3, h0) and np.random.uniform() != after
    # what collate and the detector take
    batch, hs = HG.collate([(i2, w2, h2)])
    assert batch.shape == (2, 480, 640, 3) and batch.dtype == torch.uint8 and hs.shape == (1, 3, 3)
    dets = hip.sift_detect(batch)
    assert len(dets) == 2 and all(d["pt"].shape[0] > 100 and d["pt"].shape[1] == 2 for d in dets)
