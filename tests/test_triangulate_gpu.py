"""GPU tests of the track triangulation: GIMS_AUX_TRIANGULATE_TRACKS (gims_amd/csrc/triangulate.hip) against the NumPy
restatement (tests/triangulate_ref.py) on the fixtures of tests/test_triangulate_cpu.py, which asserts their margins: status, n_inliers,
obs_inlier and the counters compare exactly, the floats within the bars below.  The op is called through a table on a buffer filled with
0xA5; every output must be overwritten, and neither the padding between the regions nor the 256 bytes behind the buffer may change.

Bars.  xyz: TOL_X x the scene extent = 9.2e-9 (16 x the restatement's own spread between forward and reverse summation, measured and
asserted in tests/test_triangulate_cpu.py).  obs_error: float32 storage (2^-23 relative) + 2 |d e / d X| TOL_X, the sensitivity taken from the
restatement per observation; rms_error: the same with the largest sensitivity among the track's inliers; max_angle: float32 storage +
2 (180 / pi) (2 / d) TOL_X with d the distance of the nearest inlier centre (an angle at X between two centres moves by at most |dX| (1 / |a| +
1 / |b|)).  The factor 2 is for the second order.

Shapes.  Track lengths 2, 3, 4, 5 (GIMS_TRI_SHORT_TRACK = 4: a group of four lanes / a wave), 8, 9, 16, 17, 63, 64, 65 (one observation per
lane / slots of 64), 128, 1024 and 1025 (TOO_LONG); T = 0, 1, 7, 8, 9, 63, 64, 65, 257 (64 short tracks or 4 mid ones per workgroup: several
workgroups, ragged last ones); max_hyp 0, 1, 3, 36 (= E of the track of nine), 64, 65535; refine_iters 0 and 10.

End to end ('e2e': 8 images x 256 keypoints, 0.5 px noise, 3 % wrong matches).  The restatement's own worst error over the valid tracks whose
inliers all belong to one planted point is 1.26e-2 of the scene extent over 219 tracks (printed by test_end_to_end; the device gave the same
1.26e-2), so the bar for the device is 1.26e-1.  Two views of that scene through cameras_from_pose: worst error 3.0e-2 of the extent."""
import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import triangulate_ref as R
from tests.test_triangulate_cpu import E2E, EXTENT, MIN_ANGLE, SEAM_COMBOS, T_COUNTS, THRESH, TOL_X, _pick, prefix, reference, scene

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FILL, PAD = 0xA5, 256
EXACT = ("status", "n_inliers", "obs_inlier")
FLOATS = ("xyz", "max_angle", "rms_error", "obs_error")
SIZES = dict(xyz=lambda T, n: 24 * T, max_angle=lambda T, n: 4 * T, rms_error=lambda T, n: 4 * T, n_inliers=lambda T, n: 4 * T, obs_error=lambda T, n: 4 * n,
             status=lambda T, n: T, obs_inlier=lambda T, n: n, counters=lambda T, n: 32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _buffers(sc):
    B = {k: _dev(sc[k]) for k in ("indptr", "obs_image", "obs_keypoint", "kpts", "cams")}
    B["T"], B["n_obs"], B["n_images"], B["n"] = len(sc["indptr"]) - 1, len(sc["obs_image"]), len(sc["cams"]), len(sc["kpts"])
    B["layout"] = hip.triangulate_out_layout(B["T"], B["n_obs"])
    B["out"] = torch.full((B["layout"]["bytes"] + PAD,), FILL, dtype=torch.uint8, device="cuda")
    return B


def _op(B, combo, thresh=THRESH, min_angle=MIN_ANGLE):
    p = lambda t: t if t.numel() else None      # noqa: E731  (an empty tensor has no address: NULL is allowed when T == 0)
    return hip.op_triangulate_tracks(B["indptr"], p(B["obs_image"]), p(B["obs_keypoint"]), B["kpts"], B["cams"], B["out"], B["T"], B["n_obs"],
                                     B["n_images"], B["n"], thresh, min_angle, combo[0], combo[1])


def _read(B):
    """The outputs as the restatement returns them.  The padding between the regions and the bytes behind the buffer must be as they were."""
    torch.cuda.synchronize()
    raw, o, T, n = B["out"].cpu().numpy(), B["layout"], B["T"], B["n_obs"]
    assert (raw[o["bytes"]:] == FILL).all()
    got, padding = {}, np.ones(o["outputs"], dtype=bool)
    for name, size in SIZES.items():
        got[name] = raw[o[name]:o[name] + size(T, n)]
        padding[o[name]:o[name] + size(T, n)] = False
    assert (raw[:o["outputs"]][padding] == FILL).all(), "the padding between the output regions was written"
    out = dict(xyz=got["xyz"].view(np.float64).reshape(T, 3), max_angle=got["max_angle"].view(np.float32), rms_error=got["rms_error"].view(np.float32),
               n_inliers=got["n_inliers"].view(np.int32), obs_error=got["obs_error"].view(np.float32), status=got["status"], obs_inlier=got["obs_inlier"])
    counters = got["counters"].view(np.int32)
    assert counters[7] == 0
    out["stats"] = dict(zip(hip.TRI_COUNTERS, (int(v) for v in counters[:7])))
    return out


def run(sc, combo, **kw):
    B = _buffers(sc)
    hip.run_ops(hip.make_ops([_op(B, combo, **kw)]))
    return _read(B)


def same(got, want, sc):
    for k in EXACT:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["stats"] == want["stats"]
    assert all(np.isfinite(got[k]).all() for k in FLOATS)
    dx = np.abs(got["xyz"] - want["xyz"]).max() if len(want["xyz"]) else 0.0
    assert dx <= TOL_X * EXTENT, f"xyz differs by {dx:.3g}, the bar is {TOL_X * EXTENT:.3g}"
    store = 2.0 ** -23
    bar = store * np.abs(want["obs_error"]) + 2 * want["obs_sens"] * TOL_X * EXTENT
    d = np.abs(got["obs_error"].astype(np.float64) - want["obs_error"])
    assert (d <= bar).all(), f"obs_error: {d.max():.3g} at {int(np.argmax(d - bar))}, bar {bar[int(np.argmax(d - bar))]:.3g}"
    ptr = np.asarray(sc["indptr"], dtype=np.int64)
    for t in np.nonzero((want["status"] & ~np.uint8(R.LOW_ANGLE)) == 0)[0]:
        sens = (want["obs_sens"][ptr[t]:ptr[t + 1]] * want["obs_inlier"][ptr[t]:ptr[t + 1]]).max()
        assert abs(float(got["rms_error"][t]) - want["rms_error"][t]) <= store * want["rms_error"][t] + 2 * sens * TOL_X * EXTENT, ("rms_error", t)
        bar_a = store * want["max_angle"][t] + 2 * np.degrees(2 / want["min_dist"][t]) * TOL_X * EXTENT
        assert abs(float(got["max_angle"][t]) - want["max_angle"][t]) <= bar_a, ("max_angle", t, got["max_angle"][t], want["max_angle"][t])
    rest = (want["status"] & ~np.uint8(R.LOW_ANGLE)) != 0
    assert (got["rms_error"][rest] == 0).all() and (got["max_angle"][rest] == 0).all()


def identical(a, b):
    for k in EXACT + FLOATS:
        assert a[k].tobytes() == b[k].tobytes(), k


def subset(sc, order):
    """The tracks `order` of a scene, in that order, as a scene of their own over the same keypoints and cameras."""
    ptr = np.asarray(sc["indptr"], dtype=np.int64)
    idx = np.concatenate([np.arange(ptr[t], ptr[t + 1]) for t in order]) if len(order) else np.zeros(0, np.int64)
    indptr = np.concatenate([[0], np.cumsum([ptr[t + 1] - ptr[t] for t in order])]).astype(np.int32)
    return dict(_pick(sc), indptr=indptr, obs_image=sc["obs_image"][idx], obs_keypoint=sc["obs_keypoint"][idx]), idx


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("combo", SEAM_COMBOS)
def test_track_lengths_and_parameters(combo):
    sc = scene("seams")
    got = run(sc, combo)
    same(got, reference("seams", combo)[0], sc)
    if combo == (64, 10):
        assert got["stats"]["n_ok"] == len(sc["indptr"]) - 1


def test_long_tracks():
    sc = scene("long")
    got = run(sc, (64, 10))
    same(got, reference("long", (64, 10))[0], sc)
    assert got["status"].tolist() == [0, 0, R.TOO_LONG, 0] and got["n_inliers"][1] > 700


@pytest.mark.parametrize("T", T_COUNTS)
def test_track_counts(T):
    sub, want = prefix(reference("batch", (64, 10))[0], scene("batch"), T)
    got = run(sub, (64, 10))
    same(got, want, sub)
    assert got["stats"]["n_ok"] + got["stats"]["n_no_model"] + got["stats"]["n_low_angle"] == T


@pytest.mark.parametrize("name,combo", [("edge", (64, 10)), ("edge0", (0, 10))])
def test_edge_cases(name, combo):
    sc = scene(name)
    got = run(sc, combo)
    same(got, reference(name, combo)[0], sc)
    assert R.NO_MODEL in got["status"] and R.TOO_SHORT in got["status"] and got["stats"]["n_bad_obs"] == 2
    if combo[0] == 0:
        t = int(np.nonzero(got["status"] == R.LOW_ANGLE)[0][0])
        assert np.abs(got["xyz"][t]).max() > 10 and 0 < got["max_angle"][t] < MIN_ANGLE


def test_poisoned_inputs_are_counted_and_never_used():
    sc = scene("poison")
    got = run(sc, (64, 10))
    want = reference("poison", (64, 10))[0]
    same(got, want, sc)
    assert got["stats"]["n_bad_obs"] == 5 and got["status"][[0, 20, 21]].tolist() == [R.TOO_SHORT] * 3
    clean_sc, _ = prefix(reference("batch", (64, 10))[0], scene("batch"), 40)
    clean = run(clean_sc, (64, 10))
    ptr = np.asarray(clean_sc["indptr"], dtype=np.int64)
    for t in range(40):                                  # the neighbours of every poisoned track: bit for bit what they are without the poison
        if t in (0, 3, 5, 8, 13, 20, 21):
            continue
        for k in ("xyz", "status", "n_inliers", "max_angle", "rms_error"):
            assert got[k][t].tobytes() == clean[k][t].tobytes(), (k, t)
        for k in ("obs_error", "obs_inlier"):
            assert got[k][ptr[t]:ptr[t + 1]].tobytes() == clean[k][ptr[t]:ptr[t + 1]].tobytes(), (k, t)


# ------------------------------------------------------------------------------------------------ batch independence
@pytest.mark.parametrize("name,combo", [("seams", (64, 10)), ("edge", (64, 10)), ("edge0", (0, 10))])
def test_batch_independence(name, combo):
    """Every track alone, the batch, the batch in reversed track order and the batch run again: bit-identical per track."""
    sc = scene(name)
    T = len(sc["indptr"]) - 1
    ptr = np.asarray(sc["indptr"], dtype=np.int64)
    whole = run(sc, combo)
    identical(whole, run(sc, combo))
    rev_sc, idx = subset(sc, list(range(T))[::-1])
    rev = run(rev_sc, combo)
    for k in ("xyz", "status", "n_inliers", "max_angle", "rms_error"):
        assert rev[k][::-1].tobytes() == whole[k].tobytes(), k
    for k in ("obs_error", "obs_inlier"):
        back = np.empty_like(whole[k])
        back[idx] = rev[k]
        assert back.tobytes() == whole[k].tobytes(), k
    assert rev["stats"] == whole["stats"]
    for t in range(T):
        one_sc, _ = subset(sc, [t])
        one = run(one_sc, combo)
        for k in ("xyz", "status", "n_inliers", "max_angle", "rms_error"):
            assert one[k][0].tobytes() == whole[k][t].tobytes(), (k, t)
        for k in ("obs_error", "obs_inlier"):
            assert one[k].tobytes() == whole[k][ptr[t]:ptr[t + 1]].tobytes(), (k, t)


# ------------------------------------------------------------------------------------------------ in a table behind build_tracks
def test_op_replays_in_a_table_behind_build_tracks():
    """One table: GIMS_AUX_BUILD_TRACKS, then GIMS_AUX_TRIANGULATE_TRACKS reading the first op's output where it lies -- no host step between
    the two.  The same bits as the op alone on the same tracks, twice."""
    from tests.test_tracks_gpu import SENT, _buffers as trk_buffers, _op as trk_op
    sc, m = scene("e2e"), scene("e2e")["matches"]
    TB = trk_buffers(m["counts"], m["pairs"], m["matches"], None, None)
    T, n_obs, n = len(sc["indptr"]) - 1, len(sc["obs_image"]), TB["n"]
    o_ptr, o_img, o_kp, _, _ = hip.tracks_out_layout(n)
    B = _buffers(sc)
    B["indptr"], B["obs_image"], B["obs_keypoint"] = TB["out"][o_ptr:o_ptr + T + 1], TB["out"][o_img:o_img + n_obs], TB["out"][o_kp:o_kp + n_obs]
    alone = run(sc, (64, 10))
    ops = hip.make_ops([trk_op(TB, None, 2, "drop"), _op(B, (64, 10))])
    for _ in range(2):
        for k in ("track_of", "out", "counters", "work"):
            TB[k].fill_(SENT)
        B["out"].fill_(FILL)
        hip.run_ops(ops)
        got = _read(B)
        identical(got, alone)
        assert got["stats"] == alone["stats"]
        np.testing.assert_array_equal(B["indptr"].cpu().numpy(), sc["indptr"])
    same(alone, reference("e2e", (64, 10))[0], sc)


# ------------------------------------------------------------------------------------------------ end to end
def _count_syncs(monkeypatch):
    counts = {"device": 0, "stream": 0, "event": 0, "item": 0}
    for name, owner, attr in (("device", torch.cuda, "synchronize"), ("stream", torch.cuda.Stream, "synchronize"), ("event", torch.cuda.Event, "synchronize"),
                              ("item", torch.Tensor, "item"), ("item", torch.Tensor, "tolist"), ("item", torch.Tensor, "cpu")):
        orig = getattr(owner, attr)

        def counted(*a, _orig=orig, _name=name, **kw):
            counts[_name] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(owner, attr, counted)
    return counts


def _planted_error(out, sc, m):
    """The worst |xyz - planted| over the valid tracks whose inlier observations all belong to one planted point, and their number."""
    ptr, worst, n = np.asarray(sc["indptr"], dtype=np.int64), 0.0, 0
    for t in np.nonzero(out["status"] == 0)[0]:
        sl = slice(ptr[t], ptr[t + 1])
        inl = out["obs_inlier"][sl].astype(bool)
        ids = {int(m["point_of"][k][i]) for k, i in zip(sc["obs_image"][sl][inl], sc["obs_keypoint"][sl][inl])}
        if len(ids) == 1:
            worst, n = max(worst, float(np.abs(out["xyz"][t] - m["points"][ids.pop()]).max())), n + 1
    return worst, n


def test_end_to_end(monkeypatch):
    sc = scene("e2e")
    m = sc["matches"]
    want = reference("e2e", (64, 10))[0]
    kpts = [_dev(k) for k in m["kpts"]]
    outs = [{"matches0": _dev(x).reshape(1, -1)} for x in m["matches"]]
    tracks = gims_amd.build_tracks(m["counts"], m["pairs"], outs)
    np.testing.assert_array_equal(tracks.indptr.cpu().numpy(), sc["indptr"])
    np.testing.assert_array_equal(tracks.obs_keypoint.cpu().numpy(), sc["obs_keypoint"])
    torch.cuda.synchronize()
    counts = _count_syncs(monkeypatch)
    pts = gims_amd.triangulate_tracks(tracks, kpts, (m["K"], m["R"], m["t"]), thresh=THRESH, min_angle=MIN_ANGLE)
    mask = pts.filter(min_views=3, max_rms=2.0)
    assert counts == {"device": 0, "stream": 0, "event": 0, "item": 0}, counts          # no host synchronisation at all
    stats = pts.stats
    assert counts == {"device": 0, "stream": 0, "event": 1, "item": 1}, counts          # .stats: one event, then the pinned words
    assert pts.stats is stats and counts["event"] == 1
    monkeypatch.undo()
    got = {k: getattr(pts, k).cpu().numpy() for k in EXACT + FLOATS}
    got["stats"] = stats
    same(got, want, sc)
    assert isinstance(pts, gims_amd.Points3D) and len(pts) == tracks.n_tracks and pts.xyz.dtype == torch.float64 and pts.valid.dtype == torch.bool
    np.testing.assert_array_equal(pts.valid.cpu().numpy(), want["status"] == 0)
    np.testing.assert_array_equal(mask.cpu().numpy(), (want["status"] == 0) & (want["n_inliers"] >= 3) & (got["rms_error"] <= 2.0))
    assert stats["n_ok"] > 150 and stats["n_inlier_obs"] == int(want["n_inliers"].sum())
    ref_worst, n_ref = _planted_error(want, sc, m)
    dev_worst, n_dev = _planted_error(got, sc, m)
    print(f"'e2e': restatement worst error {ref_worst:.3g} over {n_ref} tracks, device {dev_worst:.3g}")
    assert n_dev == n_ref > 150 and ref_worst < 0.02 and dev_worst <= 10 * ref_worst

    # one verified pair through cameras_from_pose: the points come out in camera 0's frame, in units of the baseline
    R0, R1, t0, t1 = m["R"][0], m["R"][1], m["t"][0], m["t"][1]
    Rr = R1 @ R0.T
    tr = t1 - Rr @ t0
    scale = np.linalg.norm(tr)
    cams = gims_amd.cameras_from_pose(m["K"][0], m["K"][1], torch.from_numpy(Rr), tr / scale)
    pair = gims_amd.build_tracks(m["counts"][:2], [(0, 1)], outs[:1])
    p2 = gims_amd.triangulate_tracks(pair, kpts[:2], cams)
    xyz, ok, img, kp, ptr = (x.cpu().numpy() for x in (p2.xyz, p2.valid, pair.obs_image, pair.obs_keypoint, pair.indptr))
    assert ok.sum() > 50
    worst = 0.0
    for t in np.nonzero(ok)[0]:
        a, b = ptr[t], ptr[t] + 1
        ida, idb = m["point_of"][img[a]][kp[a]], m["point_of"][img[b]][kp[b]]
        if ida == idb:
            worst = max(worst, float(np.abs(xyz[t] * scale - (R0 @ m["points"][ida] + t0)).max()))
    print(f"two views through cameras_from_pose: worst error {worst:.3g} of the scene extent")
    assert worst < 0.1                                   # 0.5 px at z^2 / (f b) = 16 / (800 x 1.6) per px of disparity: 6e-3 per sigma in depth
