"""GPU tests of the SIFT descriptor stage (sift_describe_kernel, gims_amd/csrc/sift.hip) against the NumPy restatement
(tests/sift_desc_ref.py), through ``hip.sift_describe``, the front end, the op table and the classical baseline end to end.

Every comparison feeds the device's own detected keypoints, copied to the host, to both sides.  The rule: every element within 1 of the
restatement, and at most 1 % of the descriptors different at all (a cap: a transcendental or a pyramid pixel may differ in its last bit
and move a value across a rounding boundary)."""
import os

import numpy as np
import pytest
import torch

from gims_amd import baselines, frontend, hip, synth, verify
from tests import sift_desc_ref as DR, sift_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = torch.device("cuda")
F = np.float32
IMAGES = {"colour": lambda: synth.make_textured_image(96, 128, 9), "gray": lambda: synth.make_textured_image(75, 101, 4, gray=True)}
_CACHE = {}


def _case(name):
    """(img, device keypoints, their host copy, the restatement's Gaussian pyramid) of one test image."""
    if name not in _CACHE:
        img = IMAGES[name]()
        det = frontend.sift_detect_device(img, DEV)
        _CACHE[name] = (img, det, {k: v.cpu().numpy() for k, v in det.items()}, R.pyramid(img)[0])
    return _CACHE[name]


def _kp4(k):
    return np.concatenate([k["pt"], k["size"][:, None], k["angle"][:, None]], 1).astype(F)


def _describe(img, kp4, octv):
    t = torch.from_numpy(np.ascontiguousarray(img))[None].to(DEV)
    d, bad = hip.sift_describe(hip.sift_pyramid_buffer(t), img.shape[0], img.shape[1], 1, torch.from_numpy(np.ascontiguousarray(kp4, F)).to(DEV),
                               torch.from_numpy(np.asarray(octv, np.int32)).to(DEV))
    return d.cpu().numpy(), int(bad.item())


def _check_rule(what, got, want):
    diff = np.abs(got - want)
    changed = int((diff != 0).any(1).sum())
    print(what, "descriptors", len(got), "different", changed, "max |d|", float(diff.max()) if diff.size else 0.0)
    assert diff.size and diff.max() <= 1
    assert changed <= 0.01 * len(got)


@pytest.mark.parametrize("name", ["colour", "gray"])
def test_device_equals_restatement_with_edge_cases(name):
    img, det, k, gp = _case(name)
    h, w = img.shape[:2]
    top = len(gp) - 1                                             # pyramid octave of the smallest level
    extra = np.array([[0.3, 0.4, 6, 30], [w - 1, h - 1, 8, 200], [w - 0.6, 0.2, 30, 0], [1.4, h - 1.2, 12, 271], [w / 2, 0, 5, 90],   # on the border
                      [w * 0.4 + 0.2, h * 0.6 + 0.7, 1, -1], [w * 0.7, h * 0.3, 1, -1], [2.5, 3.5, 1, -1], [w - 3, h - 2.2, 1, -1],  # PaddedKeyPoint: size 1, angle -1, octave 0
                      [w / 2, h / 2, 60, 77], [w * 0.1, h * 0.9, 45, 359.5], [w * 0.8, h * 0.2, 200, -1],   # radius far past the level (636 before the clamp for size 60 on the 2x level): every interior pixel is a candidate, well over 100 LDS chunks
                      [w / 2, h / 2, 400, 123], [w * 0.3, h * 0.6, 250, 10]], F)   # top octave: the diagonal clamp on radius applies
    extra_oct = np.array([1 << 8, (2 << 8) | 255, (3 << 8) | 1, 1 << 8, 2 << 8, 0, 0, 0, 0, (2 << 8) | 255, (1 << 8) | 255, (3 << 8) | 255,
                          (1 << 8) | (top - 1), (2 << 8) | (top - 1)], np.int32)
    th, tw = gp[top][0].shape
    assert DR.radius_of(400, F(1) / F(1 << (top - 1)), th, tw) == int(np.sqrt(th * th + tw * tw))
    assert DR.radius_of(1, F(1), h, w) == 5
    kp4, octv = np.concatenate([_kp4(k), extra]), np.concatenate([k["octave"], extra_oct])
    assert len(k["octave"]) > 30
    got, bad = _describe(img, kp4, octv)
    want, wbad = DR.describe(gp, kp4, octv)
    assert bad == wbad == 0
    assert (got == np.rint(got)).all() and got.min() >= 0 and got.max() <= 255
    assert got[-14:-2].any(1).all()                               # the hand-made ones that have samples are not empty
    _check_rule(name, got, want)
    # one keypoint with an out-of-range octave: zeros and bad == 1; an IndexError with the count through the front end
    kp4b, octb = np.concatenate([kp4[:3], kp4[:1]]), np.concatenate([octv[:3], [len(gp) - 1]]).astype(np.int32)
    gotb, bad = _describe(img, kp4b, octb)
    assert bad == 1 and not gotb[3].any() and np.array_equal(gotb[:3], got[:3])
    with pytest.raises(IndexError, match="1 keypoint"):
        frontend.sift_describe_device(img, {"pt": kp4b[:, :2], "size": kp4b[:, 2], "angle": kp4b[:, 3], "octave": octb}, DEV)


@pytest.mark.parametrize("name", ["colour", "gray"])
def test_padded_keypoints_whose_samples_wrap_below_orientation_zero(name):
    """angle -1 gives ori = 361: a sample whose gradient direction is below 1 degree has o0 = -1 and votes into orientation entry 9 of
    the cell before and entry 0 of its own.  400 seeded PaddedKeyPoints per image; the restatement reports which of them fill entry 9."""
    img, _, _, gp = _case(name)
    h, w = img.shape[:2]
    rng = np.random.default_rng(17)
    kp4 = np.stack([rng.random(400) * w, rng.random(400) * h, np.ones(400), -np.ones(400)], 1).astype(F)
    octv = np.zeros(400, np.int32)
    entry9 = []
    want, wbad = DR.describe(gp, kp4, octv, entry9=entry9)
    hit = np.array(entry9) > 0
    print(name, "padded keypoints with a share in entry 9:", int(hit.sum()))
    assert hit.sum() >= 10
    got, bad = _describe(img, kp4, octv)
    assert bad == wbad == 0
    _check_rule(name + " padded", got, want)
    _check_rule(name + " padded, entry 9 filled", got[hit], want[hit])


def test_boat1_against_restatement(golden_dir):
    """All keypoints of the 850 x 680 golden image are described on the device; every 31st is compared with the restatement."""
    img = np.load(os.path.join(golden_dir, "sift_boat1.npz"))["img"]
    det = frontend.sift_detect_device(img, DEV)
    got = frontend.sift_describe_device(img, det, DEV).cpu().numpy()
    assert got.shape == (len(det["pt"]), 128) and len(got) > 15000
    assert got.any(1).all() and got.max() <= 255 and (got == np.rint(got)).all()
    k = {n: v.cpu().numpy()[::31] for n, v in det.items()}
    want, bad = DR.describe(R.pyramid(img)[0], _kp4(k), k["octave"])
    assert bad == 0 and len(want) > 490
    _check_rule("boat1", got[::31], want)


def test_deterministic_batch_invariant_and_empty():
    img, det, _, _ = _case("colour")
    other = np.ascontiguousarray(img[::-1, ::-1])
    det_o = frontend.sift_detect_device(other, DEV)
    a = frontend.sift_describe_device(img, det, DEV)
    b = frontend.sift_describe_device(img, det, DEV)
    assert torch.equal(a, b) and a.shape[0] > 30
    batch = frontend.sift_describe_device(np.stack([other, img]), [det_o, det], DEV)
    assert torch.equal(batch[1], a) and torch.equal(batch[0], frontend.sift_describe_device(other, det_o, DEV))
    none = {k: v[:0] for k, v in det.items()}
    e = frontend.sift_describe_device(img, none, DEV)
    assert e.shape == (0, 128) and e.dtype == torch.float32
    two = frontend.sift_describe_device(np.stack([other, img]), [none, det], DEV)        # an image without keypoints inside a batch
    assert two[0].shape == (0, 128) and torch.equal(two[1], a)


def test_detect_and_compute_shares_the_pyramid():
    imgs = np.stack([IMAGES["colour"](), synth.make_textured_image(96, 128, 10)])
    dets, descs = frontend.sift_detect_and_compute_device(imgs, device=DEV)
    want_k = frontend.sift_detect_device(imgs, DEV)
    want_d = frontend.sift_describe_device(imgs, want_k, DEV)
    for s in range(2):
        assert all(torch.equal(dets[s][n], want_k[s][n]) for n in want_k[s]) and torch.equal(descs[s], want_d[s]) and len(descs[s]) > 30
    # one image, max_keypoints: filter_max_num sits between detection and description
    k1, d1 = frontend.sift_detect_and_compute_device(imgs[0], 20, DEV)
    top = frontend.filter_max_num(want_k[0], 20)
    assert d1.shape == (20, 128) and torch.equal(k1["pt"], top["pt"]) and torch.equal(d1, frontend.sift_describe_device(imgs[0], top, DEV))


def test_baseline_end_to_end_on_the_warped_pair():
    """sift_baseline_front_end(root=True) -> nn_match_pairs('mnn') -> verify_pairs on the fixture of
    tests/test_sift_desc_cpu.py::test_descriptors_discriminate_on_a_warped_pair, against what the restatement recorded there (246
    matches, 244 correct).  The device and the restatement may disagree on margin keypoints only: precision within 0.02, count within 5 %."""
    img0, img1, Hm = DR.warped_pair()
    fe = frontend.sift_baseline_front_end({"image": np.stack([img0, img1]), "max_keypoints": -1, "root": True}, DEV)
    assert fe["descriptors"][0].shape[0] == 128 and fe["descriptors"][0].shape[1] == fe["keypoints"][0].shape[0] == fe["scores"][0].shape[0]
    np.testing.assert_allclose((fe["descriptors"][0] ** 2).sum(0).cpu().numpy(), 1.0, rtol=1e-4)       # RootSIFT rows have unit L2 norm
    data = {"descriptors0": fe["descriptors"][0][None], "descriptors1": fe["descriptors"][1][None],
            "keypoints0": fe["keypoints"][0][None], "keypoints1": fe["keypoints"][1][None]}
    out = baselines.nn_match_pairs([data], "mnn", 0.8)[0]
    n, ok = DR.count_correct(fe["keypoints"][0].cpu().numpy(), fe["keypoints"][1].cpu().numpy(), out["matches0"].cpu().numpy(), Hm)
    rec = DR.PAIR_RECORD
    print("device matches", n, "correct", ok, "precision", ok / n, "recorded", rec)
    assert abs(ok / n - rec["correct"] / rec["matches"]) <= 0.02
    assert abs(n - rec["matches"]) <= 0.05 * rec["matches"]
    v = verify.verify_pairs([data], [out])
    r = dict(zip(verify.RECORD_FIELDS, v["records"][0].cpu().tolist()))
    print("verify", r)
    assert r["n_valid"] == n and r["n_inliers"] >= 0.9 * n
    # root=False hands the plain descriptors through
    plain = frontend.sift_baseline_front_end({"image": img0[None]}, DEV)
    assert torch.equal(frontend.root_sift(plain["descriptors"][0].t().contiguous()), fe["descriptors"][0].t())


def test_op_replays_in_a_table_and_in_a_graph():
    """GIMS_AUX_SIFT_DESCRIBE next to another op (the SPL32 split of its output) in one gims_run_ops table, and the same table as a HIP
    graph after one plain run: equal bits."""
    img, det, _, _ = _case("colour")
    t = torch.from_numpy(img)[None].to(DEV)
    kp4, octv, _ = frontend.keypoint_arrays(det)
    pyr = hip.sift_pyramid_buffer(t)
    want, _ = hip.sift_describe(pyr, img.shape[0], img.shape[1], 1, kp4, octv)
    want_split = hip.split_spl32(want)
    n = kp4.shape[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        desc = torch.full((n, 128), -1.0, device=DEV)
        bad = torch.full((1,), 7, dtype=torch.int32, device=DEV)
        split = torch.zeros((n, 256), dtype=torch.bfloat16, device=DEV)
        ops = hip.make_ops([hip.op_sift_describe(pyr, img.shape[0], img.shape[1], 1, kp4, octv, None, desc, bad),
                            hip.op_aux(hip.AUX_SPLIT_SPL32, (desc, split), (desc.stride(0), split.stride(0), n, 128))])
        hip.run_ops(ops)
        assert torch.equal(desc, want) and torch.equal(split, want_split) and int(bad.item()) == 0
        graph = hip.OpsGraph(ops)
        desc.fill_(-1.0)
        split.zero_()
        bad.fill_(7)
        graph.launch()
        side.synchronize()
        assert torch.equal(desc, want) and torch.equal(split, want_split) and int(bad.item()) == 0
    torch.cuda.current_stream().wait_stream(side)
