"""GPU tests of bundle adjustment: GIMS_AUX_BUNDLE_ADJUST (gims_amd/csrc/ba.hip) against the NumPy restatement
(tests/ba_ref.py) on the fixtures of tests/test_ba_cpu.py, which asserts their margins: taken, the counters, cam_obs, the lambda column of
the history and the pattern of inactive observations compare exactly, the floats within the bars below.  The op is called through a
table on a buffer filled with 0xA5; every output must be overwritten, neither the padding between the regions nor the 256 bytes behind the
buffer may change, and a second run must give the same bytes.

Bars.  xyz, R, t and the costs of the history: TOL_BA = 5.3e-13, each difference divided by max(1, |word|) (16 x the restatement's own
spread between forward and reverse summation, measured and asserted in tests/test_ba_cpu.py).  obs_error: float32 storage (2^-23
relative) + 2 |d e / d parameter| TOL_BA, the sensitivity taken from the restatement per observation (the sum of the magnitudes of its
Jacobian words times the largest parameter); the factor 2 is for the second order.

Shapes.  2 images both fixed (only points move), 3, 5 and 17 images, 128 free + 2 fixed images over 300 points (the cap: a 768 x 768
reduced system); track lengths 2, 3, 4, 5 and 63, 64, 65 (a thread serves a track: there is no lane grouping, the long ones walk round the
cameras and put several observations into one image); T = 0, 1, 63, 64, 65, 257 (the blocks of 256 tracks); iters 0, 1, 10; huber 0 and 1.5;
'poison': an absent camera of NaN words, a held camera with three observations, obs_image / obs_keypoint entries of -1, n_images, 2^30, a
keypoint past n_k, two bad indptr ranges, a NaN point, a NaN keypoint, obs_use and point_use zeros; 'badcam' and 'behind': the two status
bits, outputs equal inputs; 'atmin': five rounds not taken, then nothing; 'rejtake': rejected rounds followed by taken ones.

End to end ('e2e' of tests/test_triangulate_cpu.py: 8 images x 256 keypoints, 0.5 px noise, 3 % wrong matches): estimate_pose(0, 1) ->
triangulate_tracks -> resect_images(2 .. 7) -> triangulate_tracks(all) -> bundle_adjust with cameras 0 and 1 fixed.  The rms
reprojection error over the active observations must not go up; its value and the worst |R - planted|, |t - planted| (in the frame of
camera 0 and in units of the baseline, the gauge the two estimated cameras fix) are printed before and after and recorded in DESIGN.md
4.20.  No bound on the pose errors is asserted: they are dominated by the error of the estimated pair, which the adjustment keeps."""
import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import ba_ref as B
from tests.test_ba_cpu import CASES, TOL_BA, reference, relative_difference, scene
from tests.test_resect_gpu import _count_syncs
from tests.test_triangulate_cpu import E2E

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FILL, PAD = 0xA5, 256
SIZES = lambda T, n_obs, n_images, iters: dict(xyz=24 * T, cams=144 * n_images, obs_error=4 * n_obs, cam_obs=4 * n_images, history=16 * (iters + 1),      # noqa: E731
                                               taken=iters, counters=32)


def _dev(a, shape, dtype):
    """On the device; an empty array becomes one zero element (the op wants an address and reads nothing through it)."""
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:
        a = np.zeros(shape, dtype)
    return torch.from_numpy(a).cuda()


def _buffers(sc, iters):
    B_ = dict(indptr=_dev(sc["indptr"], (1,), np.int32), obs_image=_dev(sc["obs_image"], (1,), np.int32), obs_keypoint=_dev(sc["obs_keypoint"], (1,), np.int32),
              obs_use=_dev(sc["obs_use"], (1,), np.uint8), point_use=_dev(sc["point_use"], (1,), np.uint8), kpts=_dev(sc["kpts"], (1, 2), np.float32),
              xyz=_dev(sc["xyz"], (1, 3), np.float64), cams=_dev(sc["cams"], (1, 18), np.float64))
    B_["mode"] = np.ascontiguousarray(sc["mode"], dtype=np.int32)
    B_["table"] = hip.ba_table(*(B_[k] for k in ("indptr", "obs_image", "obs_keypoint", "obs_use", "point_use")))
    B_["dims"] = (len(sc["indptr"]) - 1, len(sc["obs_image"]), len(sc["mode"]), iters)
    B_["n"] = len(sc["kpts"])
    B_["layout"] = hip.ba_out_layout(*B_["dims"], int((sc["mode"] == 2).sum()))
    B_["out"] = torch.full((B_["layout"]["bytes"] + PAD,), FILL, dtype=torch.uint8, device="cuda")
    return B_


def _op(B_, huber, lambda0):
    T, n_obs, _, iters = B_["dims"]
    return hip.op_bundle_adjust(B_["table"], B_["kpts"], B_["xyz"], B_["cams"], B_["mode"], B_["out"], T, n_obs, B_["n"], iters, huber, lambda0)


def _read(B_):
    """The outputs as the restatement returns them, and their bytes.  The padding between the regions and the bytes behind the buffer must
    be as they were."""
    torch.cuda.synchronize()
    raw, o = B_["out"].cpu().numpy(), B_["layout"]
    T, n_obs, n_images, iters = B_["dims"]
    assert (raw[o["bytes"]:] == FILL).all(), "bytes behind the buffer were written"
    got, padding = {}, np.ones(o["outputs"], dtype=bool)
    for name, size in SIZES(*B_["dims"]).items():
        got[name] = raw[o[name]:o[name] + size].copy()
        padding[o[name]:o[name] + size] = False
    assert (raw[:o["outputs"]][padding] == FILL).all(), "the padding between the output regions was written"
    out = dict(xyz=got["xyz"].view(np.float64).reshape(T, 3), cams=got["cams"].view(np.float64).reshape(n_images, 18), obs_error=got["obs_error"].view(np.float32),
               cam_obs=got["cam_obs"].view(np.int32), history=got["history"].view(np.float64).reshape(iters + 1, 2), taken=got["taken"])
    out["stats"] = dict(zip(hip.BA_COUNTERS, (int(v) for v in got["counters"].view(np.int32))))
    out["bytes"] = b"".join(got[k].tobytes() for k in SIZES(*B_["dims"]))
    return out


def run(sc, iters, huber=0.0, lambda0=1e-4):
    B_ = _buffers(sc, iters)
    hip.run_ops(hip.make_ops([_op(B_, huber, lambda0)]))
    return _read(B_)


def same(got, want, sc):
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])
    np.testing.assert_array_equal(got["taken"], want["taken"])
    np.testing.assert_array_equal(got["cam_obs"], want["cam_obs"])
    np.testing.assert_array_equal(got["history"][:, 1], want["history"][:, 1])          # lambda: the same divisions and products by ten
    np.testing.assert_array_equal(got["obs_error"] == -1, want["obs_error"] == -1)
    assert np.isfinite(got["history"]).all() and np.isfinite(got["obs_error"]).all()
    assert np.array_equal(np.isnan(got["xyz"]), np.isnan(np.asarray(sc["xyz"], np.float64))) and np.array_equal(np.isnan(got["cams"]), np.isnan(sc["cams"]))
    d = relative_difference(got, want, sc)
    print(f"xyz, R, t and the costs differ by {d:.3g}, the bar is {TOL_BA:.3g}")
    assert d <= TOL_BA, f"xyz, R, t or a cost differs by {d:.3g}, the bar is {TOL_BA:.3g}"
    bar = 2.0 ** -23 * np.abs(want["obs_error"]) + 2 * want["obs_sens"] * TOL_BA
    de = np.abs(got["obs_error"].astype(np.float64) - want["obs_error"])
    assert (de <= bar).all(), f"obs_error: {de.max():.3g} at {int(np.argmax(de - bar))}, bar {bar[int(np.argmax(de - bar))]:.3g}"
    # what does not move is copied through bit for bit: inactive points, absent / fixed / held cameras, the eight other words of a free one
    active_pt = np.zeros(len(sc["xyz"]), bool)
    for t in range(len(sc["xyz"])):
        b, e = int(sc["indptr"][t]), int(sc["indptr"][t + 1])
        active_pt[t] = 0 <= b <= e <= len(want["obs_error"]) and bool((want["obs_error"][b:e] >= 0).any())
    start = np.asarray(sc["xyz"], np.float64)
    if want["stats"]["status"] == 0:
        assert got["xyz"][~active_pt].tobytes() == start[~active_pt].tobytes()
    else:
        assert got["xyz"].tobytes() == start.tobytes() and got["cams"].tobytes() == np.asarray(sc["cams"], np.float64).tobytes()
        assert (got["obs_error"] == -1).all() and got["taken"].sum() == 0 and (got["history"][:, 0] == 0).all()
    still = np.ones((len(sc["mode"]), 18), bool)
    free = np.flatnonzero((sc["mode"] == 2) & (want["cam_obs"] >= 4))
    still[free, 4:16] = False
    assert got["cams"][still].tobytes() == np.asarray(sc["cams"], np.float64)[still].tobytes()


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("name,iters,huber,lambda0", CASES)
def test_against_the_restatement(name, iters, huber, lambda0):
    sc = scene(name)
    got, want = run(sc, iters, huber, lambda0), reference(name, iters, huber, lambda0)
    print(name, got["stats"], got["taken"].tolist(), f"cost {got['history'][0, 0]:.6g} -> {got['history'][-1, 0]:.6g}")
    same(got, want, sc)
    assert run(sc, iters, huber, lambda0)["bytes"] == got["bytes"], "two runs on the same input differ"
    if name == "cap":
        assert got["stats"]["n_free"] == hip.BA_MAX_FREE_CAMERAS
    if name in ("badcam", "behind"):
        assert got["stats"]["status"] == (hip.BA_BAD_CAMERA if name == "badcam" else hip.BA_BAD_START)
    if name == "atmin":
        assert got["taken"].sum() == 0 and got["history"][5, 1] == got["history"][-1, 1]
    if name == "rejtake":
        assert any(a == 0 and b == 1 for a, b in zip(got["taken"], got["taken"][1:]))
    if name == "T0":
        assert got["stats"]["n_points"] == 0 and got["stats"]["n_held"] == 3


def test_refused_before_any_launch_leaves_the_buffer_alone():
    sc = scene("c5")
    B_ = _buffers(dict(sc, mode=np.array([1, 1, 2, 2, 3], np.int32)), 3)
    with pytest.raises(hip.GimsHipError, match="bundle_adjust: image 4: mode = 3"):
        hip.run_ops(hip.make_ops([_op(B_, 0.0, 1e-4)]))
    torch.cuda.synchronize()
    assert bool((B_["out"] == FILL).all())


# ------------------------------------------------------------------------------------------------ a captured graph
def test_the_op_replays_from_a_captured_graph():
    """The same bytes from the direct run, a second direct run on the same buffer and the captured graph: every decision lives on the device."""
    sc = scene("poison")
    alone = run(sc, 10, 1.5)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        B_ = _buffers(sc, 10)
        ops = hip.make_ops([_op(B_, 1.5, 1e-4)])
        hip.run_ops(ops)
        side.synchronize()
        assert _read(B_)["bytes"] == alone["bytes"]
        graph = hip.OpsGraph(ops)
        for _ in range(2):
            B_["out"].fill_(FILL)
            graph.launch()
            side.synchronize()
            assert _read(B_)["bytes"] == alone["bytes"]
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------------------------------------ end to end
def _planted_in_frame_of_camera_0(m):
    """The planted cameras in the gauge of cameras_from_pose: camera 0 is the world, the baseline of cameras 0 and 1 is the unit."""
    R0, t0 = m["R"][0], m["t"][0]
    Rs = np.stack([R @ R0.T for R in m["R"]])
    ts = np.stack([t - R @ t0 for R, t in zip(Rs, m["t"])])
    return Rs, ts / np.linalg.norm(ts[1])


def test_end_to_end(monkeypatch):
    m = B.TR.planted_matches(**E2E)
    n_cams = E2E["n_cams"]
    kpts = [torch.from_numpy(k).cuda() for k in m["kpts"]]
    outs = [{"matches0": torch.from_numpy(x).cuda().reshape(1, -1)} for x in m["matches"]]
    tracks = gims_amd.build_tracks(m["counts"], m["pairs"], outs)
    assert m["pairs"][0] == (0, 1)
    good = m["matches"][0] >= 0
    Rr, tr, _ = gims_amd.estimate_pose(m["kpts"][0][good], m["kpts"][1][m["matches"][0][good]], m["K"][0], m["K"][1])
    K2, R2, t2 = gims_amd.cameras_from_pose(m["K"][0], m["K"][1], Rr, tr)
    Rn, tn = np.full((n_cams, 3, 3), np.nan), np.full((n_cams, 3), np.nan)
    Rn[:2], tn[:2] = R2, t2
    first = gims_amd.triangulate_tracks(tracks, kpts, (m["K"], Rn, tn))
    poses = gims_amd.resect_images(first, tracks, kpts, m["K"], which=list(range(2, n_cams)), iters=256, seed=7)
    cams = poses.cameras(m["K"], Rn, tn)
    pts = gims_amd.triangulate_tracks(tracks, kpts, cams)
    torch.cuda.synchronize()
    counts = _count_syncs(monkeypatch)
    adj = gims_amd.bundle_adjust(pts, tracks, kpts, cams, iters=20)
    assert counts == {"device": 0, "stream": 0, "event": 0, "item": 0}, counts          # no host synchronisation at all
    stats = adj.stats
    assert counts == {"device": 0, "stream": 0, "event": 1, "item": 1}, counts          # .stats: one event, then the pinned words
    monkeypatch.undo()
    posed = np.isfinite(cams[1]).all(axis=(1, 2))
    assert posed.sum() >= n_cams - 1 and adj.mode == [1, 1] + [2 if p else 0 for p in posed[2:]] and stats["status"] == 0 and stats["n_fixed"] == 2
    assert adj.R.shape == (n_cams, 3, 3) and adj.t.shape == (n_cams, 3) and adj.R.data_ptr() == adj.records.data_ptr() + 32 and adj.xyz.shape == pts.xyz.shape
    assert stats["n_free"] + stats["n_held"] == int(posed.sum()) - 2 and stats["n_points"] == int(pts.valid.sum()) and stats["rounds_taken"] >= 1
    hist, err = adj.history.cpu().numpy(), adj.obs_error.cpu().numpy()
    rms0, rms1 = np.sqrt(hist[0, 0] / stats["n_active_obs"]), np.sqrt(hist[-1, 0] / stats["n_active_obs"])
    assert (err >= 0).sum() == stats["n_active_obs"] and abs(np.sqrt((err[err >= 0].astype(np.float64) ** 2).mean()) - rms1) < 1e-5 * rms1
    Rp, tp = _planted_in_frame_of_camera_0(m)
    before = (np.abs(cams[1] - Rp)[posed].max(), np.abs(cams[2] - tp)[posed].max())
    Ka, Ra, ta = adj.cameras()
    after = (np.abs(Ra - Rp)[posed].max(), np.abs(ta - tp)[posed].max())
    print(f"'e2e': {stats}; rms reprojection error {rms0:.4g} -> {rms1:.4g} px over {stats['n_active_obs']} observations; worst |dR| {before[0]:.3g} -> {after[0]:.3g}, "
          f"|dt| {before[1]:.3g} -> {after[1]:.3g} against the planted cameras")
    assert rms1 <= rms0 and (Ra[:2] == cams[1][:2]).all() and (ta[:2] == cams[2][:2]).all() and (Ka == m["K"]).all()
    # the records go straight into the next triangulation, where they lie: the same bytes as through the host triple
    again = gims_amd.triangulate_tracks(tracks, kpts, adj.records)
    host = gims_amd.triangulate_tracks(tracks, kpts, (Ka, Ra, ta))
    assert again.xyz.cpu().numpy().tobytes() == host.xyz.cpu().numpy().tobytes() and int(again.valid.sum()) >= int(pts.valid.sum()) - 5
    with pytest.raises(ValueError, match="device camera records"):
        gims_amd.triangulate_tracks(tracks, kpts, adj.records.float())
