"""CPU tests of the multi-view tracks: the ABI constant and the argument checks of GIMS_AUX_BUILD_TRACKS (they run before any HIP call), the pins
a feature must leave alone, the host-side table builder and workspace formula of hip.build_tracks, the ValueErrors of gims_amd.build_tracks, the
NumPy restatement (tests/tracks_ref.py) against a hand-worked case, and the conditions on the generated scenes that keep the GPU tests from
being vacuous."""
import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import tracks_ref as R

# the hand-worked case: 3 images of 4, 3 and 5 keypoints -> nodes 0-3, 4-6, 7-11
#   pair (0, 1): kp 1 -> kp 0                       edge 1 - 4
#   pair (1, 2): kp 0 -> kp 2, kp 1 -> 0, kp 2 -> 0  edges 4 - 9, 5 - 7, 6 - 7   (two keypoints of image 1 meet through image 2: a conflict)
#   pair (0, 2): kp 1 -> kp 2, kp 3 -> kp 4          edges 1 - 9 (closes the chain 1 - 4 - 9), 3 - 11
# components: {1, 4, 9}, {3, 11}, {5, 6, 7} (conflicting), and the singletons 0, 2, 8, 10
HAND = dict(counts=[4, 3, 5], pairs=[(0, 1), (1, 2), (0, 2)], matches=[[-1, 0, -1, -1], [2, 0, 0], [-1, 2, -1, 4]])
HAND_DROP = dict(track_of=[-1, 0, -1, 1, 0, -1, -1, -1, -1, 0, -1, 1], indptr=[0, 3, 5], obs_image=[0, 1, 2, 0, 2], obs_keypoint=[1, 0, 2, 3, 4],
                 conflict=[0, 0], stats=dict(n_tracks=2, n_obs=5, n_conflicting=1, n_edges=6, n_bad=0, status=0))
HAND_KEEP = dict(track_of=[-1, 0, -1, 1, 0, 2, 2, 2, -1, 0, -1, 1], indptr=[0, 3, 5, 8], obs_image=[0, 1, 2, 0, 2, 1, 1, 2],
                 obs_keypoint=[1, 0, 2, 3, 4, 1, 2, 0], conflict=[0, 0, 1], stats=dict(n_tracks=3, n_obs=8, n_conflicting=1, n_edges=6, n_bad=0, status=0))
HAND_DROP3 = dict(track_of=[-1, 0, -1, -1, 0, -1, -1, -1, -1, 0, -1, -1], indptr=[0, 3], obs_image=[0, 1, 2], obs_keypoint=[1, 0, 2], conflict=[0],
                  stats=dict(n_tracks=1, n_obs=3, n_conflicting=1, n_edges=6, n_bad=0, status=0))
SCENE_A = dict(seed=7, n_points=600, n_images=6, p_seen=0.6, q_kept=0.8, w_wrong=0.02)


def same(got, want):
    for k in ("track_of", "indptr", "obs_image", "obs_keypoint", "conflict"):
        np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(want[k]), err_msg=k)
    assert got["stats"] == want["stats"]


def test_abi_constant_and_pins():
    assert hip.AUX_BUILD_TRACKS == 9 == hip.ABI.constants["GIMS_AUX_BUILD_TRACKS"]
    # the feature adds no export, no struct and no ABI version
    assert len(hip.EXPORTS) == 90 and len(hip.ABI.structs) == 28 and hip.ABI_VERSION == 5 == hip.load().gims_abi_version()
    assert not any("track" in name.lower() for name in hip.EXPORTS)
    assert gims_amd.build_tracks is gims_amd.tracks.build_tracks and gims_amd.Tracks is gims_amd.tracks.Tracks
    assert "build_tracks" in gims_amd.__all__ and "Tracks" in gims_amd.__all__
    assert hip.TRACKS_SCAN_TILE == hip.ABI.constants["GIMS_TRACKS_SCAN_TILE"] >= 256
    assert hip.TRACKS_SHORT_SEGMENT == hip.ABI.constants["GIMS_TRACKS_SHORT_SEGMENT"] >= 2
    assert hip.TRACKS_TABLE_WORDS == 8 and hip.TRACKS_COUNTERS == R.COUNTERS


def _run(ptrs, ints, floats=(0.0,)):
    """Through hip.run_ops, on the null stream (no device is needed: a refused call makes no HIP call)."""
    with hip.on_stream(0):
        hip.run_ops(hip.make_ops([hip.op_aux(hip.AUX_BUILD_TRACKS, ptrs, ints, floats)]))


def test_argument_checks_come_before_any_hip_call():
    """Every GIMS_EINVAL case of the header, with a message naming build_tracks; the pointers are never dereferenced."""
    p = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000]      # table, start, track_of, out, counters, work
    n = 5000
    good = [3, 4, n, 2, hip.tracks_work_bytes(3, 4, n), 0]         # n_pairs, n_images, N, min_length | flags, work_bytes, reserved

    def refused(ptrs, ints, word, floats=(0.0,)):
        with pytest.raises(hip.GimsHipError, match="build_tracks") as e:
            _run(ptrs, ints, floats)
        assert word in str(e.value) and f"({hip.GIMS_EINVAL})" in str(e.value), str(e.value)

    def ints(**kw):
        names = ["n_pairs", "n_images", "n", "mode", "work_bytes", "form"]
        return [kw.get(k, v) for k, v in zip(names, good)]

    def ptrs(**kw):
        names = ["table", "start", "track_of", "out", "counters", "work"]
        return [kw.get(k, v) for k, v in zip(names, p)]

    refused(p, ints(n_pairs=-1), "n_pairs = -1")
    refused(p, ints(n_pairs=(1 << 24) + 1), "n_pairs")
    refused(p, ints(n_images=0), "n_images = 0")
    refused(p, ints(n_images=(1 << 24) + 1), "n_images")
    refused(p, ints(n=-1), "N = -1")
    refused(p, ints(n=(1 << 30) + 1), "N = ")
    for mode in (0, 1, -2, (1 << 24) + 1, 2 | (1 << 29), 2 | (1 << 31), hip.TRACKS_KEEP_CONFLICTING | 1):
        refused(p, ints(mode=mode), "min_length")
    refused(p, good, "min_score is NaN", floats=(float("nan"),))
    refused(ptrs(start=None), good, "NULL")
    refused(ptrs(out=None), good, "NULL")
    refused(ptrs(counters=None), good, "NULL")
    refused(ptrs(table=None), good, "pair table is NULL")
    refused(ptrs(track_of=None), good, "track_of or the workspace is NULL")
    refused(ptrs(work=None), good, "track_of or the workspace is NULL")
    refused(ptrs(table=p[0] + 4), good, "8-byte aligned")
    for name in ("start", "track_of", "out", "counters"):
        refused(ptrs(**{name: dict(zip(["start", "track_of", "out", "counters"], p[1:5]))[name] + 2}), good, "4-byte aligned")
    refused(ptrs(work=p[5] + 8), good, "16-byte aligned")
    refused(p, ints(work_bytes=good[4] - 1), "work_bytes")
    refused(p, ints(work_bytes=-1), "work_bytes")
    refused(p, ints(form=1), "reserved")
    # i[5] would select a later form of the function, so it is read first: whatever the other words hold, this version does not know the call
    refused([None] * 6, [9, 9, 9, 9, 9, 9], "unknown auxiliary function form")


def test_empty_calls_are_still_checked():
    """N == 0 or n_pairs == 0 is GIMS_OK after the same checks.  Such a call writes its counters and indptr[0], so the calls that succeed need
    a device and live in tests/test_tracks_gpu.py; here: an empty call with a bad argument is refused like any other, and an empty call may
    leave out exactly what the header lets it leave out (that one is refused for the NEXT thing it lacks)."""
    p = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000]
    for ints in ([0, 4, 5000, 2, 1 << 30, 0], [3, 4, 0, 2, 0, 0], [0, 1, 0, 2, 0, 0]):
        with pytest.raises(hip.GimsHipError, match="build_tracks: start, the output buffer or the counters are NULL"):
            _run(p[:4] + [None, p[5]], ints)
        with pytest.raises(hip.GimsHipError, match="build_tracks: i.3. = 1"):
            _run(p, ints[:3] + [1] + ints[4:])
    # N == 0: track_of, work (and its size) may be absent; n_pairs == 0: the table
    with pytest.raises(hip.GimsHipError, match="4-byte aligned"):
        _run([p[0], p[1], None, p[3], p[4] + 2, None], [3, 4, 0, 2, 0, 0])
    with pytest.raises(hip.GimsHipError, match="4-byte aligned"):
        _run([None, p[1], p[2], p[3], p[4] + 2, p[5]], [0, 4, 5000, 2, 1 << 30, 0])
    with pytest.raises(hip.GimsHipError, match="work_bytes = 0"):            # ... but N > 0 without pairs still needs its workspace
        _run(p, [0, 4, 5000, 2, 0, 0])


def test_work_bytes_mirror_the_header_formula():
    al = lambda x: (x + 255) & ~255                                           # noqa: E731
    for n_pairs, n_images, n in ((0, 1, 0), (3, 3, 12), (15, 6, 2049), (1225, 50, 204800), (4950, 100, 2000000)):
        huge = max(1024, n // 1024)
        want = 12 * al(4 * n) + al(4 * (n // 2048 + 2)) + al(4 * (n // (huge + 1) + 1) * (n // 2048 + 1)) + 256
        assert hip.tracks_huge(n) == huge
        assert hip.tracks_work_bytes(n_pairs, n_images, n) == want
        if n:                                                                 # one byte less is refused by the library
            with pytest.raises(hip.GimsHipError, match=f"work_bytes = {want - 1}"):
                _run([0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000], [n_pairs, n_images, n, 2, want - 1, 0])
    assert hip.TRACKS_SCAN_TILE == 2048 and hip.TRACKS_LONG_SEGMENT == 1024 == hip.ABI.constants["GIMS_TRACKS_LONG_SEGMENT"]
    assert hip.tracks_out_layout(12) == (0, 7, 19, 31, 33) and hip.tracks_out_layout(0) == (0, 1, 1, 1, 1) and hip.tracks_out_layout(5) == (0, 3, 8, 13, 14)


def test_table_builder():
    m01, m12 = torch.tensor([-1, 0, -1, -1]), torch.tensor([2, 0, 0])
    sc, mask = torch.zeros(4), torch.ones(3, dtype=torch.uint8)
    tab = hip.tracks_table([(0, 1, m01, sc, None), (1, 2, m12, None, mask), (2, 2, torch.arange(5), None, None)], [4, 3, 5], "cpu")
    assert tab.dtype == np.int64 and tab.shape == (4, 8)
    np.testing.assert_array_equal(tab, [[m01.data_ptr(), sc.data_ptr(), 0, 4, 3, 0, 4, 0], [m12.data_ptr(), 0, mask.data_ptr(), 3, 5, 4, 7, 4],
                                        [tab[2, 0], 0, 0, 5, 5, 7, 7, 7], [0, 0, 0, 0, 0, 0, 0, 12]])
    np.testing.assert_array_equal(hip.tracks_table([], [4, 0, 5], "cpu"), np.zeros((1, 8), dtype=np.int64))
    e = torch.zeros(0, dtype=torch.int64)
    assert hip.tracks_table([(1, 0, e, None, None)], [4, 0], "cpu").tolist() == [[e.data_ptr(), 0, 0, 0, 4, 4, 0, 0], [0] * 8]
    for bad, word in (((0, 3, m01, None, None), "out of range"), ((-1, 0, m01, None, None), "out of range"),
                      ((0, 1, m01.int(), None, None), "torch.int64"), ((0, 1, m01, sc.double(), None), "torch.float32"),
                      ((0, 1, m01, None, torch.ones(4, dtype=torch.bool)), "torch.uint8"), ((1, 0, m01, None, None), "3 keypoints"),
                      ((0, 1, m01, sc[:3], None), "4 keypoints"), ((0, 1, m01[None], None, None), "1-D"),
                      ((0, 1, torch.zeros(8, dtype=torch.int64)[::2], None, None), "1-D"), ((0, 1, [1, 2, 3, 4], None, None), "tensor")):
        with pytest.raises(ValueError, match=word):
            hip.tracks_table([bad], [4, 3, 5], "cpu")
    with pytest.raises(ValueError, match="is on"):
        hip.tracks_table([(0, 1, m01, None, None)], [4, 3, 5], "cuda:0")
    with pytest.raises(ValueError, match="negative"):
        hip.tracks_table([], [4, -3], "cpu")


def test_python_value_errors_come_before_the_device():
    outs = [{"matches0": torch.tensor([HAND["matches"][p]]), "matching_scores0": torch.zeros((1, len(HAND["matches"][p])))} for p in range(3)]
    args = (HAND["counts"], HAND["pairs"], outs)
    bt = gims_amd.build_tracks
    with pytest.raises(ValueError, match="one length"):
        bt(HAND["counts"], HAND["pairs"][:2], outs)
    with pytest.raises(ValueError, match="one length"):
        bt(*args, inlier=[torch.ones(4, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="one length"):
        bt(*args, inlier={"inlier": []})
    with pytest.raises(ValueError, match="out of range"):
        bt(HAND["counts"], [(0, 1), (1, 3), (0, 2)], outs)
    with pytest.raises(ValueError, match="out of range"):
        bt(HAND["counts"], [(0, 1), (-1, 2), (0, 2)], outs)
    with pytest.raises(ValueError, match="image 1 has 3 keypoints"):
        bt(HAND["counts"], [(1, 0), (1, 2), (0, 2)], outs)
    with pytest.raises(ValueError, match="inlier has shape"):
        bt(*args, inlier=[torch.ones(4, dtype=torch.uint8)] * 3)
    with pytest.raises(ValueError, match="is on"):
        bt(*args[:2], [outs[0], {"matches0": torch.empty((1, 3), dtype=torch.int64, device="meta")}, outs[2]])
    with pytest.raises(ValueError, match="torch.int64"):
        bt(*args[:2], [{"matches0": outs[0]["matches0"].int()}] + outs[1:])
    with pytest.raises(ValueError, match="torch.float32"):
        bt(*args[:2], [{"matches0": outs[0]["matches0"], "matching_scores0": torch.zeros((1, 4), dtype=torch.float64)}] + outs[1:], min_score=0.1)
    with pytest.raises(ValueError, match="torch.uint8"):
        bt(*args, inlier=[torch.ones(n, dtype=torch.bool) for n in (4, 3, 4)])
    with pytest.raises(ValueError, match="no matching_scores0"):
        bt(*args[:2], [{"matches0": o["matches0"]} for o in outs], min_score=0.1)
    for bad in (1, 0, -3, 2.5, True):
        with pytest.raises(ValueError, match="min_length"):
            bt(*args, min_length=bad)
    with pytest.raises(ValueError, match="conflicts"):
        bt(*args, conflicts="split")
    with pytest.raises(ValueError, match="NaN"):
        bt(*args, min_score=float("nan"))
    with pytest.raises(ValueError, match="non-empty"):
        bt([], [], [])
    with pytest.raises(ValueError, match="on the GPU"):                       # everything is in order, except that these tensors are on the host
        bt(*args)


def test_restatement_against_the_hand_worked_case():
    same(R.build(**HAND), HAND_DROP)
    same(R.build(**HAND, conflicts="keep"), HAND_KEEP)
    same(R.build(**HAND, min_length=3), HAND_DROP3)
    # the edge set alone decides: pairs in another order, one of them twice, one the other way round
    m12_back = [-1, -1, 0, -1, -1]                                           # (2, 1): kp 2 -> kp 0; the non-injective rows of (1, 2) have no inverse
    again = R.build([4, 3, 5], [(0, 2), (2, 1), (1, 2), (0, 1), (0, 1)], [HAND["matches"][2], m12_back, HAND["matches"][1], HAND["matches"][0], HAND["matches"][0]])
    want = dict(HAND_DROP, stats=dict(HAND_DROP["stats"], n_edges=8))
    same(again, want)
    # filters, bad indices and a self pair
    got = R.build([4, 3, 5], [(0, 1), (1, 2), (0, 2), (2, 2)], HAND["matches"][:2] + [[-1, 2, 5, 4], [0, 1, 2, 4, 3]],
                  scores=[np.array([0, 0.5, 0, 0], dtype=np.float32), np.array([0.5, 0.2, np.nan], dtype=np.float32), None, None],
                  masks=[None, None, np.array([1, 1, 1, 0], dtype=np.uint8), None], min_score=0.5, conflicts="keep")
    # accepted: 1 - 4; 4 - 9 (0.2 and NaN are below); 1 - 9 (5 is bad, the mask drops 3 - 11); the self pair: three no-ops and 10 - 11 twice
    same(got, dict(track_of=[-1, 0, -1, -1, 0, -1, -1, -1, -1, 0, 1, 1], indptr=[0, 3, 5], obs_image=[0, 1, 2, 2, 2], obs_keypoint=[1, 0, 2, 3, 4],
                   conflict=[0, 1], stats=dict(n_tracks=2, n_obs=5, n_conflicting=1, n_edges=8, n_bad=1, status=0)))


def test_generated_scene_is_not_vacuous():
    """Scene A of the GPU tests: the restatement must find enough long tracks and enough conflicts for the comparison to mean something."""
    counts, pairs, matches = R.scene(**SCENE_A)
    assert len(counts) == 6 and len(pairs) == 15 and all(len(m) == counts[a] for (a, b), m in zip(pairs, matches))
    for (a, b), m in zip(pairs, matches):                                     # injective, as mutual matching makes it
        hit = m[m >= 0]
        assert len(np.unique(hit)) == len(hit) and hit.max() < counts[b]
    drop = R.build(counts, pairs, matches)
    lengths = np.diff(drop["indptr"])
    assert int((lengths >= 3).sum()) >= 100, int((lengths >= 3).sum())
    assert drop["stats"]["n_conflicting"] >= 10 and not drop["conflict"].any()
    keep = R.build(counts, pairs, matches, conflicts="keep")
    assert keep["stats"]["n_conflicting"] == drop["stats"]["n_conflicting"] == int(keep["conflict"].sum())
    assert int(np.diff(keep["indptr"]).max()) > len(counts)                   # a track longer than its number of images
    assert keep["stats"]["n_tracks"] == drop["stats"]["n_tracks"] + drop["stats"]["n_conflicting"]
