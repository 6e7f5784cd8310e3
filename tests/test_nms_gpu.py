"""GPU tests of the DIoU-NMS keypoint thinning (diou_nms_kernel, gims_amd/csrc/nms.hip) against the goldens the reference's own
process_diou_nms produced and the NumPy restatement (tests/nms_ref.py), through ``hip.diou_nms``, the front end, the op table and
``Matching``.  Every comparison is exact integer equality of row lists, order included."""
import os

import numpy as np
import pytest
import torch

from gims_amd import frontend, hip, synth
from gims_amd.matching import Matching
from tests import nms_ref as N, sift_desc_ref as DR

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = torch.device("cuda")
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = [n for n, _, _ in N.FIXTURES]
_CACHE = {}


def _fixture(name):
    if name not in _CACHE:
        recipe = next(r for n, r, _ in N.FIXTURES if n == name)
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        kp, scores = (g["kp"], g["scores"]) if "kp" in g.files else N.build_fixture(recipe)
        _CACHE[name] = (recipe, kp, scores, g["rows"].tolist())
    return _CACHE[name]


def _kp4(kp):
    return np.concatenate([np.asarray(kp, F)[:, :3], np.zeros((len(kp), 1), F)], 1)


def _op(kp4, order, offsets, radius, thr, h, w):
    """hip.diou_nms on host arrays -> (keep, count) as NumPy."""
    keep, count = hip.diou_nms(torch.from_numpy(np.ascontiguousarray(kp4, F)).to(DEV), torch.from_numpy(np.asarray(order, np.int32)).to(DEV),
                               torch.from_numpy(np.asarray(offsets, np.int32)).to(DEV), radius, thr, h, w)
    return keep.cpu().numpy(), count.cpu().numpy()


def _dict(kp, scores):
    kp = np.asarray(kp, F)
    n = len(kp)
    return {"pt": torch.from_numpy(kp[:, :2].copy()).to(DEV), "size": torch.from_numpy(kp[:, 2].copy()).to(DEV), "angle": torch.zeros(n, device=DEV),
            "response": torch.from_numpy(np.asarray(scores, F)).to(DEV), "octave": torch.zeros(n, dtype=torch.int32, device=DEV),
            "row": torch.arange(n, device=DEV)}


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_reference(name):
    recipe, kp, scores, rows = _fixture(name)
    n = len(kp)
    keep, count = _op(_kp4(kp), N.make_order(scores), [0, n], recipe["radius"], recipe["thr"], recipe["height"], recipe["width"])
    print(name, "kept", int(count[0]), "of", n)
    assert count.tolist() == [len(rows), 0]
    assert keep[:count[0]].tolist() == rows and (keep[count[0]:] == -1).all()
    if recipe["kind"] == "chain":
        assert rows == list(range(0, n, 2))
    # the front end: every field indexed by the result, the order made on the device
    out = frontend.diou_nms_device(_dict(kp, scores), recipe["radius"] or None, recipe["thr"], (recipe["height"], recipe["width"]))
    assert out["row"].cpu().tolist() == rows
    assert torch.equal(out["pt"].cpu(), torch.from_numpy(kp[rows][:, :2])) and out["octave"].shape == (len(rows),)
    again = frontend.diou_nms_device(_dict(kp, scores), recipe["radius"] or None, recipe["thr"])          # no extent given
    assert again["row"].cpu().tolist() == rows


def _dense(n, seed, side=60.0):
    rng = np.random.default_rng(seed)
    kp = np.stack([rng.random(n) * side * 1.3, rng.random(n) * side, np.exp(rng.normal(1.0, 0.6, n)) + 1.0], 1).astype(F)
    return kp, (rng.permutation(n) + 1).astype(F) / F(n)


@pytest.mark.parametrize("radius", [4, 0])
def test_segments_of_every_size_in_one_batch(radius):
    """Images of 0, 1, 2, 1023, 1024, 1025 and 2049 keypoints (around one and two strides of the 1024-thread workgroup) in one call:
    every image equals its single-image result and the restatement."""
    sizes = [0, 1, 2, 1023, 1024, 1025, 0, 2049]
    parts = [_dense(m, 100 + b, 40.0 + m / 20) for b, m in enumerate(sizes)]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    kp4 = _kp4(np.concatenate([p[0] for p in parts]))
    order = np.concatenate([N.make_order(p[1]) + offsets[b] for b, p in enumerate(parts)])
    keep, count = _op(kp4, order, offsets, radius, 0.3, 200, 260)
    want_keep, want_count = N.run_op(kp4, order, offsets, radius, 0.3)
    assert count.tolist() == want_count.tolist() and count[-1] == 0
    assert keep.tolist() == want_keep.tolist()
    assert count[1] == 1 and 0 < count[3] < 1023 and 0 < count[7] < 2049
    for b, (kp, scores) in enumerate(parts):
        if sizes[b]:
            k1, c1 = _op(_kp4(kp), N.make_order(scores), [0, sizes[b]], radius, 0.3, 200, 260)
            assert c1[0] == count[b] and (k1[:c1[0]] + offsets[b]).tolist() == keep[offsets[b]:offsets[b] + count[b]].tolist()
    # the front end on the same batch (a list of dicts), images without keypoints included
    outs = frontend.diou_nms_device([_dict(*p) for p in parts], radius or None, 0.3, (200, 260))
    for b, out in enumerate(outs):
        assert (out["row"].cpu().numpy() + offsets[b]).tolist() == keep[offsets[b]:offsets[b] + count[b]].tolist()


def test_duplicates_map_to_the_lower_row():
    """Equal scores are processed higher row first, so the KEPT one of two identical keypoints is the higher row: the result names the lower."""
    recipe, kp, scores, rows = _fixture("nms_duplicates")
    twin = np.nonzero((kp[1:] == kp[:-1]).all(1) & (scores[1:] == scores[:-1]))[0] + 1
    order = N.make_order(scores)
    assert all(order.tolist().index(t) < order.tolist().index(t - 1) for t in twin[:10])
    keep, count = _op(_kp4(kp), order, [0, len(kp)], 4, 0.3, 240, 320)
    got = keep[:count[0]].tolist()
    assert got == rows and not set(got) & set(twin.tolist()) and len(set(got) & set((twin - 1).tolist())) > 40


@pytest.mark.parametrize("radius", [4, 0])
def test_bad_keypoints_are_dropped_and_counted(radius):
    rng = np.random.default_rng(11)
    kp4 = np.concatenate([rng.random((40, 2)) * 50, rng.random((40, 1)) * 4 + 1, np.zeros((40, 1))], 1).astype(F)
    kp4[3, 0], kp4[7, 1], kp4[9, 2], kp4[25, 2] = np.nan, np.inf, -np.inf, -1.0
    order = np.concatenate([np.arange(20)[::-1], 20 + rng.permutation(20)])
    order[5], order[30] = 33, -1                                  # a row of the other image, and a row that does not exist
    keep, count = _op(kp4, order, [0, 20, 40], radius, 0.3, 50, 50)
    want_keep, want_count = N.run_op(kp4, order, [0, 20, 40], radius, 0.3)
    assert count.tolist() == want_count.tolist() and count[2] == (5 if radius else 6)
    assert keep.tolist() == want_keep.tolist()
    # offsets beyond the buffer are clamped on the device: the last image ends at n
    keep2, count2 = _op(kp4, order, [-5, 20, 4000], radius, 0.3, 50, 50)
    assert keep2.tolist() == keep.tolist() and count2.tolist() == count.tolist()
    # a non-finite score takes the keypoint out at the Python layer
    scores = (np.arange(40, 0, -1) / 40).astype(F)
    scores[[2, 11]] = np.nan, np.inf
    d = _dict(kp4[:, :3], scores)
    out = frontend.diou_nms_device(d, radius or None, 0.3, (50, 50))
    valid = N.make_order(scores)
    valid = valid[~N.bad_rows(kp4, radius)[valid]]
    box = N.boxes(kp4, radius)
    assert out["row"].cpu().tolist() == N.map_back(box, N.sequential(box, valid, 0.3), valid)
    assert not set(out["row"].cpu().tolist()) & {2, 11, 3, 7, 9}


def test_extent_hint_changes_nothing():
    """Keypoints far outside the stated extent, negative coordinates, a tiny and a huge extent: the same rows."""
    kp, scores = _dense(1500, 5, 50.0)
    kp[::7, 0] -= 40
    kp[::11, 1] += 300
    kp[::13, 0] += 5000
    order = N.make_order(scores)
    want_keep, want_count = N.run_op(_kp4(kp), order, [0, 1500], 0, 0.3)
    assert 0 < want_count[0] < 1500
    for h, w in ((50, 65), (1, 1), (7, 3), (400, 6000), (1 << 30, 1 << 30)):
        keep, count = _op(_kp4(kp), order, [0, 1500], 0, 0.3, h, w)
        assert count.tolist() == want_count.tolist() and keep.tolist() == want_keep.tolist(), (h, w)


def test_one_huge_box_among_small_ones():
    """Size mode with one box of side 500: the cells grow to hold it, the search covers everything, the result stays the restatement's."""
    kp, scores = _dense(1200, 8, 120.0)
    kp[600] = (70.0, 60.0, 500.0)
    for top in (True, False):                                     # the huge box processed first, and in the middle of the order
        scores[600] = 2.0 if top else 0.5
        order = N.make_order(scores)
        want_keep, want_count = N.run_op(_kp4(kp), order, [0, 1200], 0, 0.3)
        keep, count = _op(_kp4(kp), order, [0, 1200], 0, 0.3, 120, 156)
        assert count.tolist() == want_count.tolist() and keep.tolist() == want_keep.tolist()
        assert 600 in keep.tolist()


def test_op_replays_in_a_table_and_in_a_graph():
    """GIMS_AUX_DIOU_NMS next to GIMS_AUX_SPLIT_SPL32 in one gims_run_ops table, and the same table as a HIP graph launched twice."""
    recipe, kp, scores, rows = _fixture("nms_dense_r4")
    n = len(kp)
    kp4 = torch.from_numpy(_kp4(kp)).to(DEV)
    order = torch.from_numpy(N.make_order(scores).astype(np.int32)).to(DEV)
    offsets = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    x = torch.randn(64, 128, device=DEV)
    want_split = hip.split_spl32(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        keep = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        count = torch.full((2,), -7, dtype=torch.int32, device=DEV)
        work = torch.empty(hip.diou_nms_workspace_bytes(n, 1), dtype=torch.uint8, device=DEV)
        split = torch.zeros((64, 256), dtype=torch.bfloat16, device=DEV)
        ops = hip.make_ops([hip.op_diou_nms(kp4, order, offsets, keep, count, work, 1, recipe["height"], recipe["width"], 4, 0.3),
                            hip.op_aux(hip.AUX_SPLIT_SPL32, (x, split), (x.stride(0), split.stride(0), 64, 128))])
        hip.run_ops(ops)
        assert count.tolist() == [len(rows), 0] and keep[:len(rows)].tolist() == rows and torch.equal(split, want_split)
        graph = hip.OpsGraph(ops)
        for _ in range(2):
            keep.fill_(-7)
            count.fill_(-7)
            split.zero_()
            work.fill_(255)
            graph.launch()
            side.synchronize()
            assert count.tolist() == [len(rows), 0] and keep[:len(rows)].tolist() == rows and (keep[len(rows):] == -1).all()
            assert torch.equal(split, want_split)
    torch.cuda.current_stream().wait_stream(side)


def _net():
    from gims_amd.carhynet import CARHyNet
    net = CARHyNet().eval()
    net.load_state_dict(synth.make_carhynet_state_dict(321))
    return net


def test_device_front_end_thins_between_detection_and_filter():
    """device_front_end with diou_nms=True on the 240 x 320 fixture: fewer keypoints than without, and exactly the restatement applied to
    the device detector's own output copied to the host; then max_keypoints cuts the thinned list."""
    img = synth.make_textured_image(240, 320, 7)[None]
    net = _net()
    det = frontend.sift_detect_device(img[0], DEV)
    k = {name: v.cpu().numpy() for name, v in det.items()}
    rows = N.process(np.concatenate([k["pt"], k["size"][:, None]], 1), k["response"], 4, 0.3)
    plain = frontend.device_front_end({"image": img, "carhynet": net, "max_keypoints": -1}, DEV)
    thin = frontend.device_front_end({"image": img, "carhynet": net, "max_keypoints": -1, "diou_nms": True}, DEV)
    print("keypoints", len(k["pt"]), "->", len(rows))
    assert 0 < len(rows) < len(k["pt"]) == plain["keypoints"][0].shape[0]
    assert np.array_equal(thin["keypoints"][0].cpu().numpy(), k["pt"][rows]) and np.array_equal(thin["scores"][0].cpu().numpy(), k["response"][rows])
    assert thin["descriptors"][0].shape == (256, len(rows))
    capped = frontend.device_front_end({"image": img, "carhynet": net, "max_keypoints": 100, "diou_nms": {"radius": 4, "iou_thresh": 0.3}}, DEV)
    assert np.array_equal(capped["keypoints"][0].cpu().numpy(), k["pt"][rows[:100]])
    # host keypoint lists inside sift_forward_device go through process_diou_nms
    host = [frontend.PaddedKeyPoint(x, y) for x, y in k["pt"]]
    for o, s, r in zip(host, k["size"], k["response"]):
        o.size, o.response = float(s), float(r)
    assert frontend.process_diou_nms(host, 4, 0.3) == [host[i] for i in rows]
    size_rows = N.process(np.concatenate([k["pt"], k["size"][:, None]], 1), k["response"], None, 0.3)
    assert frontend.process_diou_nms(host) == [host[i] for i in size_rows]
    # the classical baseline's front end reads the same key
    base = frontend.sift_baseline_front_end({"image": img, "diou_nms": True}, DEV)
    assert np.array_equal(base["keypoints"][0].cpu().numpy(), k["pt"][rows]) and base["descriptors"][0].shape == (128, len(rows))


def test_matching_runs_with_the_thinned_front_end(synth_sd):
    img0, img1, _ = DR.warped_pair()
    net = _net()
    m = Matching({"front_end": frontend.with_diou_nms(frontend.device_front_end), "max_keypoints": 200}).eval()
    m.gmodel.load_state_dict(synth_sd)
    base = {"carhynet": net, "device": DEV, "radius": 15, "percentile": 2, "min_size": 7}
    out = m({"image0": img0[None], "image1": img1[None], **base})
    explicit = {}
    for side, img in (("0", img0), ("1", img1)):
        fe = frontend.device_front_end({"image": img[None], "carhynet": net, "max_keypoints": 200, "diou_nms": True}, DEV)
        det = frontend.diou_nms_device(frontend.sift_detect_device(img, DEV), 4, 0.3, img.shape[:2])
        assert len(det["pt"]) > 200 and torch.equal(fe["keypoints"][0], det["pt"][:200])      # the 200 strongest of the thinned detections
        explicit.update({k + side: torch.stack(fe[k]) for k in ("keypoints", "scores", "descriptors")})
    ref = m.gmodel({"image0": img0[None], "image1": img1[None], **base, **explicit})
    assert torch.equal(out["keypoints0"], ref["keypoints0"]) and torch.equal(out["keypoints1"], ref["keypoints1"])
    assert torch.equal(out["matches0"], ref["matches0"]) and out["matches0"].shape[0] == 1 and 0 < out["matches0"].shape[1] <= 200
