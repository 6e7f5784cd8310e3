"""GPU tests of the SIFT detector (gims_amd/csrc/sift.hip) against the NumPy restatement (tests/sift_ref.py), the recorded
OpenCV counts (tests/golden/sift_counts.npz), and through the front end and ``Matching``."""
import os

import numpy as np
import pytest
import torch

from gims_amd import Matching, frontend, hip, synth
from tests import sift_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = torch.device("cuda")


def _img(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"sift_{name}.npz"))["img"]


_REF = {}


def _ref(key, img):
    if key not in _REF:
        _REF[key] = R.detect(img)
    return _REF[key]


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _match(dev, ref):
    """One-to-one matching of device and restatement keypoints at the issue's bars.  Returns (pairs, unmatched device indices,
    unmatched restatement indices)."""
    order = np.argsort(ref["pt"][:, 0], kind="stable")
    rx = ref["pt"][order, 0]
    used = np.zeros(len(rx), bool)
    pairs, lone = [], []
    for i, (x, y) in enumerate(dev["pt"]):
        lo, hi = np.searchsorted(rx, x - 1e-3), np.searchsorted(rx, x + 1e-3, side="right")
        hit = -1
        for q in range(lo, hi):
            j = order[q]
            if used[q] or abs(ref["pt"][j, 1] - y) > 1e-3 or abs(ref["size"][j] - dev["size"][i]) > 1e-4 * ref["size"][j]:
                continue
            da = abs(ref["angle"][j] - dev["angle"][i]) % 360
            if min(da, 360 - da) > 0.05:
                continue
            hit = q
            break
        if hit < 0:
            lone.append(i)
        else:
            used[hit] = True
            pairs.append((i, order[hit]))
    return np.array(pairs).reshape(-1, 2), np.array(lone, np.int64), order[~used]


def _check_against_restatement(d, ref, margin_bar=1e-3):
    pairs, lone_dev, lone_ref = _match(d, ref)
    i, j = pairs[:, 0], pairs[:, 1]
    assert np.abs(d["pt"][i] - ref["pt"][j]).max() <= 1e-3
    assert (np.abs(d["size"][i] - ref["size"][j]) <= 1e-4 * ref["size"][j]).all()
    assert (np.abs(d["response"][i] - ref["response"][j]) <= 1e-4 * ref["response"][j]).all()
    np.testing.assert_array_equal(d["octave"][i], ref["octave"][j])
    # a keypoint only one side has must be one whose deciding comparison sat within the restatement's tolerance margin
    assert (ref["margin"][lone_ref] < margin_bar).all(), ref["margin"][lone_ref]
    for k in lone_dev:               # its candidate on the restatement's side sits at the same place with a fragile decision
        near = np.abs(ref["pt"] - d["pt"][k]).max(1) < 1.0
        assert near.any() and (ref["margin"][near] < margin_bar).any(), (k, d["pt"][k])
    return len(pairs), len(lone_dev), len(lone_ref)


@pytest.mark.parametrize("name", ["boat1", "graf1"])
def test_pyramid_equals_restatement(golden_dir, name):
    """Every Gaussian and DoG level against the restatement.  Both run float32 in the same order without fused multiply-add, so
    the bar is a few float32 ulps of the pixel range: |d| <= 4 * 2^-24 * 256."""
    img = _img(golden_dir, name)
    gauss, dog = hip.sift_pyramid(torch.from_numpy(img)[None].to(DEV))
    gp, dp = R.pyramid(img)
    bar = 4 * 2.0 ** -24 * 256
    assert len(gauss[0]) == len(gp)
    worst = 0.0
    for o in range(len(gp)):
        for i in range(6):
            worst = max(worst, float(np.abs(gauss[0][o][i].cpu().numpy() - gp[o][i]).max()))
        for i in range(5):
            worst = max(worst, float(np.abs(dog[0][o][i].cpu().numpy() - dp[o][i]).max()))
    print(name, "pyramid max |d|", worst)
    assert worst <= bar


@pytest.mark.parametrize("name,expected", [("boat1", 15382), ("graf1", 7848)])
def test_keypoints_equal_restatement_and_opencv_counts(golden_dir, name, expected):
    img = _img(golden_dir, name)
    d = _np(frontend.sift_detect_device(img, DEV))
    ref = _ref(name, img)
    n, ld, lr = _check_against_restatement(d, ref)
    print(name, "device", len(d["size"]), "restatement", len(ref["size"]), "matched", n, "only device", ld, "only restatement", lr)
    assert abs(len(d["size"]) - expected) <= 0.01 * expected
    counts = np.load(os.path.join(golden_dir, "sift_counts.npz"))
    rec = dict(zip(counts["dirs"].tolist(), counts["counts"].tolist()))
    assert rec[{"boat1": "oxford_boat3", "graf1": "oxford_graf"}[name]] == expected


@pytest.mark.parametrize("h,w,seed,gray", [(240, 320, 7, False), (333, 517, 11, True)])
def test_keypoints_on_synthetic_images(h, w, seed, gray):
    img = synth.make_textured_image(h, w, seed, gray=gray)
    d = _np(frontend.sift_detect_device(img, DEV))
    ref = R.detect(img)
    n, _, _ = _check_against_restatement(d, ref)
    assert n > 50


def test_deterministic_and_batch_invariant(golden_dir):
    img = _img(golden_dir, "boat1")
    other = np.ascontiguousarray(img[::-1, ::-1])
    a = _np(frontend.sift_detect_device(img, DEV))
    b = _np(frontend.sift_detect_device(img, DEV))
    batch = frontend.sift_detect_device(np.stack([other, img]), DEV)
    c = _np(batch[1])
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(a[k], c[k])
    solo = _np(frontend.sift_detect_device(other, DEV))
    for k in solo:
        np.testing.assert_array_equal(solo[k], batch[0][k].cpu().numpy())


def test_candidate_overflow_grows_the_buffer(golden_dir):
    img = _img(golden_dir, "graf1")
    full = _np(hip.sift_detect(torch.from_numpy(img)[None].to(DEV))[0])
    small = _np(hip.sift_detect(torch.from_numpy(img)[None].to(DEV), cand_cap=1000)[0])
    for k in full:
        np.testing.assert_array_equal(full[k], small[k])


def _net():
    from gims_amd.carhynet import CARHyNet
    net = CARHyNet().eval()
    net.load_state_dict(synth.make_carhynet_state_dict(321))
    return net


def test_device_front_end_equals_explicit_keypoints():
    img = np.stack([synth.make_textured_image(240, 320, 5), synth.make_textured_image(240, 320, 6)])
    net = _net()
    got = frontend.device_front_end({"image": img, "carhynet": net, "max_keypoints": -1}, DEV)
    dets = [frontend.sift_detect_device(im, DEV) for im in img]
    q = list(dets)
    want = frontend.sift_forward_device({"image": img, "carhynet": net, "max_keypoints": -1}, DEV, detector=lambda im: q.pop(0))
    for s in range(2):
        assert len(got["keypoints"][s]) == len(dets[s]["pt"]) > 50
        for k in ("keypoints", "scores", "descriptors"):
            assert torch.equal(got[k][s], want[k][s]), k
    # max_keypoints: the strongest responses, in descending order (ties: detector order)
    cap = 100
    top = frontend.device_front_end({"image": img, "carhynet": net, "max_keypoints": cap}, DEV)
    r = dets[0]["response"].cpu().numpy()
    np.testing.assert_array_equal(top["scores"][0].cpu().numpy(), -np.sort(-r, kind="stable")[:cap])
    idx = torch.sort(dets[0]["response"], descending=True, stable=True)[1][:cap]
    assert torch.equal(top["keypoints"][0], dets[0]["pt"][idx])


def test_device_front_end_is_train_padding_follows_np_random():
    img = synth.make_textured_image(96, 128, 9)[None]
    net = _net()
    n = len(frontend.sift_detect_device(img[0], DEV)["pt"])
    want = n + 37
    np.random.seed(1234)
    got = frontend.device_front_end({"image": img, "carhynet": net, "max_keypoints": want, "is_train": True}, DEV)
    np.random.seed(1234)
    host = frontend.pad_training_keypoints([], 37, img[0].shape)
    assert got["keypoints"][0].shape == (want, 2)
    np.testing.assert_allclose(got["keypoints"][0][n:].cpu().numpy(), np.array([k.pt for k in host], np.float32), rtol=0, atol=0)
    assert (got["scores"][0][n:] == 0).all()


def _warp(img, seed):
    """A seeded mild homography of img (bilinear, inverse map, border 0)."""
    h, w = img.shape[:2]
    H = synth.make_homography(seed, (w, h), strength=0.3)
    Hi = np.linalg.inv(H)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    p = Hi @ np.stack([xx.ravel(), yy.ravel(), np.ones(h * w)])
    sx, sy = (p[0] / p[2]).reshape(h, w), (p[1] / p[2]).reshape(h, w)
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    fx, fy = sx - x0, sy - y0
    ok = (x0 >= 0) & (y0 >= 0) & (x0 < w - 1) & (y0 < h - 1)
    x0c, y0c = np.clip(x0, 0, w - 2), np.clip(y0, 0, h - 2)
    f = img.astype(np.float64)
    out = ((1 - fy) * (1 - fx))[..., None] * f[y0c, x0c] + ((1 - fy) * fx)[..., None] * f[y0c, x0c + 1] + \
        (fy * (1 - fx))[..., None] * f[y0c + 1, x0c] + (fy * fx)[..., None] * f[y0c + 1, x0c + 1]
    return np.where(ok[..., None], np.clip(np.rint(out), 0, 255), 0).astype(np.uint8)


def test_matching_runs_from_images(golden_dir, synth_sd):
    img0 = _img(golden_dir, "boat1")
    img1 = _warp(img0, 77)
    net = _net()
    m = Matching({"front_end": frontend.device_front_end, "max_keypoints": 2048}).eval()
    m.gmodel.load_state_dict(synth_sd)
    base = {"carhynet": net, "device": DEV, "radius": 15, "percentile": 2, "min_size": 7}
    out = m({"image0": img0[None], "image1": img1[None], **base})
    explicit = {}
    for s, img in (("0", img0), ("1", img1)):
        fe = frontend.device_front_end({"image": img[None], "carhynet": net, "max_keypoints": 2048}, DEV)
        det = frontend.filter_max_num(frontend.sift_detect_device(img, DEV), 2048)
        assert len(det["pt"]) == 2048 and torch.equal(fe["keypoints"][0], det["pt"]) and torch.equal(fe["scores"][0], det["response"])
        explicit.update({k + s: torch.stack(fe[k]) for k in ("keypoints", "scores", "descriptors")})      # as Matching stacks them
    ref = m.gmodel({"image0": img0[None], "image1": img1[None], **base, **explicit})
    assert torch.equal(out["keypoints0"], ref["keypoints0"]) and torch.equal(out["keypoints1"], ref["keypoints1"])
    assert torch.equal(out["matches0"], ref["matches0"]) and torch.equal(out["matches1"], ref["matches1"])
    # scores at the soak tests' bar: two forward calls need not pick the same attention kernels
    assert float((out["matching_scores0"] - ref["matching_scores0"]).abs().max()) <= 5e-5
    assert int((out["matches0"] >= 0).sum()) > 0
