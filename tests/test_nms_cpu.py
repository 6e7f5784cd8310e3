"""CPU tests of the DIoU-NMS keypoint thinning: the ABI constant and the argument checks of GIMS_AUX_DIOU_NMS (they run before any HIP
call), the pins a feature must leave alone, the NumPy restatement (tests/nms_ref.py) against the goldens the reference's own function
produced (tools/gen_golden_nms.py), its two forms against each other, and the Python argument rules of gims_amd.frontend."""
import os
import re

import numpy as np
import pytest
import torch

from gims_amd import frontend, hip
from tests import nms_ref as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def _fixture(name):
    """(recipe, kp, scores, golden rows) of one recipe; built once."""
    if name not in _CACHE:
        recipe = next(r for n, r, _ in N.FIXTURES if n == name)
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        kp, scores = (g["kp"], g["scores"]) if "kp" in g.files else N.build_fixture(recipe)
        assert len(kp) == int(g["n"]) and all(np.array_equal(g["recipe/" + k], np.array(v)) for k, v in recipe.items())
        _CACHE[name] = (recipe, kp, scores, g["rows"].tolist())
    return _CACHE[name]


NAMES = [n for n, _, _ in N.FIXTURES]


def test_abi_constant_and_pins():
    assert hip.AUX_DIOU_NMS == 7 == hip.ABI.constants["GIMS_AUX_DIOU_NMS"]
    # the thinning adds no export, no struct and no ABI version
    assert len(hip.EXPORTS) == 90 and len(hip.ABI.structs) == 28 and hip.ABI_VERSION == 5 == hip.load().gims_abi_version()
    assert not any("nms" in name.lower() for name in hip.EXPORTS)


def _run(ptrs, ints, floats=(4.0, 0.3)):
    lib = hip.load()
    ops = hip.make_ops([hip.op_aux(hip.AUX_DIOU_NMS, ptrs, ints, floats)])
    return lib.gims_run_ops(ops, 1, None), lib.gims_last_error()


def test_argument_checks_come_before_any_hip_call():
    """Every GIMS_EINVAL case of the header, with a message naming diou_nms; the pointers are never dereferenced (no device is needed)."""
    p = [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000]          # kp4, order, offsets, keep, count, work
    wb = hip.diou_nms_workspace_bytes(5, 2)
    good = [5, 2, 240, 320, wb, 0]                                # n, n_images, height, width, work_bytes, reserved

    def refused(ptrs, ints, word, floats=(4.0, 0.3)):
        rc, msg = _run(ptrs, ints, floats)
        assert rc == hip.GIMS_EINVAL and b"diou_nms" in msg and word in msg, (rc, msg)

    for k in range(6):                                            # any NULL pointer while n > 0
        refused([None if j == k else v for j, v in enumerate(p)], good, b"NULL")
    refused(p, [-1] + good[1:], b"n = -1")
    refused(p, [5, 0, 240, 320, wb, 0], b"n_images")
    refused(p, [5, 2, 0, 320, wb, 0], b"extent")
    refused(p, [5, 2, 240, 0, wb, 0], b"extent")
    for radius in (-1.0, float("nan"), float("inf")):
        refused(p, good, b"radius", (radius, 0.3))
    for thr in (0.0, 1.0, -0.2, 1.5, float("nan"), float("inf")):
        refused(p, good, b"iou_thresh", (4.0, thr))
    refused(p, [5, 2, 240, 320, wb - 1, 0], b"workspace")
    refused(p, [5, 2, 240, 320, wb, 1], b"reserved")
    refused([0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6004], good, b"aligned")
    # n == 0 is fine and touches nothing, even with null pointers; its other arguments are still checked
    wb0 = hip.diou_nms_workspace_bytes(0, 3)
    assert _run([None] * 6, [0, 3, 240, 320, wb0, 0])[0] == hip.GIMS_OK
    assert _run([None] * 6, [0, 3, 240, 320, wb0, 0], (0.0, 0.5))[0] == hip.GIMS_OK       # radius 0: boxes from the size
    refused([None] * 6, [0, 3, 240, 320, wb0 - 1, 0], b"workspace")
    refused([None] * 6, [0, 3, 240, 320, wb0, 0], b"iou_thresh", (4.0, 1.0))


@pytest.mark.parametrize("n,n_images", [(0, 1), (1, 1), (5, 2), (1023, 3), (15382, 1), (100000, 16), (1 << 20, 7)])
def test_workspace_formula_is_the_library_s(n, n_images):
    """hip.diou_nms_workspace_bytes is the library's own figure (gims_aux_layout); the op states the same need when it refuses one byte less."""
    wb = hip.diou_nms_workspace_bytes(n, n_images)
    rc, msg = _run([0x1000] * 6, [n, n_images, 10, 10, wb - 1, 0])
    assert rc == hip.GIMS_EINVAL and int(re.search(rb"(\d+) needed", msg).group(1)) == wb, msg


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference(name):
    """The rows the reference's process_diou_nms returned, as a list in its order."""
    recipe, kp, scores, rows = _fixture(name)
    want = next(c for n, _, c in N.FIXTURES if n == name)
    assert len(rows) == want
    assert N.process(kp, scores, recipe["radius"], recipe["thr"]) == rows


@pytest.mark.parametrize("name", NAMES)
def test_round_form_equals_sequential_form(name):
    recipe, kp, scores, rows = _fixture(name)
    box, order = N.boxes(kp, recipe["radius"]), N.make_order(scores)
    kept, n_rounds = N.rounds(box, order, recipe["thr"])
    print(name, "rounds", n_rounds)
    assert N.map_back(box, kept, order) == rows and kept == N.sequential(box, order, recipe["thr"])
    if recipe["kind"] == "chain":                                 # every decision waits for the one before it
        assert n_rounds == len(kp) and rows == list(range(0, len(kp), 2))
    else:
        assert n_rounds <= 8


def test_duplicates_come_back_as_their_first_row():
    recipe, kp, scores, rows = _fixture("nms_duplicates")
    twin = np.nonzero((kp[1:] == kp[:-1]).all(1) & (scores[1:] == scores[:-1]))[0] + 1     # the second row of every pair
    assert len(twin) == 60 and not set(rows) & set(twin.tolist())
    assert len(set(rows) & set((twin - 1).tolist())) > 40                                   # most first rows of a pair are there


def test_run_op_counts_bad_keypoints_and_foreign_order_entries():
    rng = np.random.default_rng(11)
    kp4 = np.concatenate([rng.random((40, 2)) * 50, rng.random((40, 1)) * 4 + 1, np.zeros((40, 1))], 1).astype(np.float32)
    kp4[3, 0], kp4[7, 1], kp4[9, 2], kp4[25, 2] = np.nan, np.inf, -np.inf, -1.0
    order = np.concatenate([np.arange(20)[::-1], 20 + rng.permutation(20)])
    order[5], order[30] = 33, -1                                  # a row of the other image, and a row that does not exist
    keep_r, count_r = N.run_op(kp4, order, [0, 20, 40], 4, 0.3)
    keep_s, count_s = N.run_op(kp4, order, [0, 20, 40], 0, 0.3)
    assert count_r[2] == 5 and count_s[2] == 6                    # 3 non-finite + 2 foreign entries; size mode adds the negative size
    for keep, count in ((keep_r, count_r), (keep_s, count_s)):
        assert (keep[:count[0]] < 20).all() and (keep[count[0]:20] == -1).all() and (keep[20:20 + count[1]] >= 20).all()
        assert not set(keep.tolist()) & {3, 7, 9, 14} and 33 not in keep[:20].tolist()          # row 14 lost its place in the order to 33
    assert 25 not in keep_s.tolist()


def test_python_argument_rules():
    assert frontend._nms_args(4, 0.3) == (4.0, 0.3)
    assert frontend._nms_args(None, 0.3) == (0.0, 0.3)            # None: boxes from the keypoint size
    assert frontend._nms_args(4, None) == (4.0, 0.5) and frontend._nms_args(4, 0) == (4.0, 0.5)      # a falsy threshold means 0.5
    assert frontend._nms_args(0, 0.3) is None and frontend._nms_args(0.0, 7.0) is None               # radius 0: the input comes back
    kps = [object(), object()]
    assert frontend.process_diou_nms(kps, 0, 0.3) is kps
    d = {"pt": torch.zeros(2, 2)}
    assert frontend.diou_nms_device(d, 0, 0.3) is d and frontend.diou_nms_device([d], 0) == [d]
    assert frontend.process_diou_nms([], 4, 0.3) == []            # the reference raises on an empty input
    for radius, thr in ((-1, 0.3), (float("nan"), 0.3), (4, 1.0), (4, -0.5), (4, 2), (None, 1)):
        with pytest.raises(ValueError, match="diou_nms"):
            frontend.diou_nms_device(d, radius, thr)
        with pytest.raises(ValueError, match="diou_nms"):
            frontend.process_diou_nms(kps, radius, thr)
    assert frontend._nms_settings(None) is None and frontend._nms_settings(False) is None
    assert frontend._nms_settings(True) == (4, 0.3) == frontend.NMS_DEFAULT
    assert frontend._nms_settings({"radius": None, "iou_thresh": 0.2}) == (None, 0.2) and frontend._nms_settings({}) == (4, 0.3)
    with pytest.raises(TypeError):
        frontend._nms_settings(4)


def test_order_rule_of_the_python_layer():
    """Descending score, equal scores with the higher row first, non-finite scores out: the restatement's make_order is the rule
    frontend._nms_rows implements with torch sorts (checked on the device in tests/test_nms_gpu.py)."""
    s = np.array([0.5, 0.9, 0.5, np.nan, 0.1, 0.9, np.inf], np.float32)
    assert N.make_order(s).tolist() == [5, 1, 2, 0, 4]


def _fake_det(n):
    return {"pt": torch.zeros(n, 2), "size": torch.ones(n), "angle": torch.zeros(n), "response": torch.arange(n, dtype=torch.float32),
            "octave": torch.zeros(n, dtype=torch.int32)}


def test_front_ends_without_the_key_make_the_calls_they_made(monkeypatch):
    calls = []
    dets = [_fake_det(3), _fake_det(4)]
    monkeypatch.setattr(frontend, "sift_detect_device", lambda imgs, device=None: dets)
    monkeypatch.setattr(frontend, "diou_nms_device", lambda k, *a, **kw: calls.append(("nms", a)) or k)
    monkeypatch.setattr(frontend, "sift_forward_device", lambda data, device, detector=None: calls.append(("forward", data)) or [detector(None), detector(None)])
    images = np.zeros((2, 24, 32, 3), np.uint8)
    data = {"image": images, "max_keypoints": -1}
    out = frontend.device_front_end(data, "cpu")
    assert calls == [("forward", data)] and calls[0][1] is data and out[0] is dets[0] and out[1] is dets[1]
    for off in (None, False):
        calls.clear()
        frontend.device_front_end({**data, "diou_nms": off}, "cpu")
        assert [c[0] for c in calls] == ["forward"]
    # with the key: one batched call with the reference's settings and the image size, and the stage is not applied a second time
    calls.clear()
    frontend.device_front_end({**data, "diou_nms": True}, "cpu")
    assert [c[0] for c in calls] == ["nms", "forward"] and calls[0][1] == (4, 0.3, (24, 32), "cpu") and calls[1][1]["diou_nms"] is None
    calls.clear()
    frontend.with_diou_nms(frontend.device_front_end, None, 0.2)(data, device="cpu")
    assert calls[0] == ("nms", (None, 0.2, (24, 32), "cpu")) and "diou_nms" not in data


def test_detect_and_compute_without_the_key_makes_the_calls_it_made(monkeypatch):
    calls = []
    dets = [_fake_det(3), _fake_det(4)]
    monkeypatch.setattr(hip, "sift_detect", lambda t, return_pyramid=False: (dets, "pyr"))
    monkeypatch.setattr(frontend, "_describe", lambda pyr, h, w, kps, dev: [torch.zeros(len(k["pt"]), 128) for k in kps])
    monkeypatch.setattr(frontend, "diou_nms_device", lambda k, *a, **kw: calls.append(a) or k)
    images = np.zeros((2, 24, 32, 3), np.uint8)
    k, d = frontend.sift_detect_and_compute_device(images, -1, "cpu")
    assert not calls and k[0] is dets[0] and d[1].shape == (4, 128)
    fe = frontend.sift_baseline_front_end({"image": images}, "cpu")
    assert not calls and fe["keypoints"][1].shape == (4, 2)
    frontend.sift_baseline_front_end({"image": images, "diou_nms": {"radius": 8}}, "cpu")
    assert calls == [(8, 0.3, (24, 32), torch.device("cpu"))]
