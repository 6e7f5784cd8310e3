"""GPU tests of the conjugate-gradient form of bundle adjustment: GIMS_AUX_BUNDLE_ADJUST_PCG (gims_amd/csrc/ba.hip) against
the NumPy restatement (tests/ba_pcg_ref.py) on the fixtures of tests/test_ba_pcg_cpu.py, which asserts their margins: taken, cg_used, the
counters, cam_obs, the lambda column of the history and the pattern of inactive observations compare exactly, the floats within the bars
below.  The op is called through a table on a buffer filled with 0xA5; every output must be overwritten, neither the padding between
the regions nor the 256 bytes behind the buffer may change, and a second run and a captured graph must give the same bytes.

Bars (all measured and asserted in tests/test_ba_pcg_cpu.py).  xyz, R, t and the costs of the history: TOL_PCG = 1.0e-12, each difference
divided by max(1, |word|): 16 x the restatement's own spread between forward and reverse summation.  cg_res: TOL_CG_RES = 4.5e-11, 16 x the
same spread of cg_res.  obs_error: float32 storage + 2 |d e / d parameter| TOL_PCG, as in tests/test_ba_gpu.py.  The device's function 14
against the device's function 13, with the iteration run to the end (cg_tol = 1e-12, cg_iters = 128): TOL_PCG_VS_DENSE = 2.4e-13, 16 x the
difference of the two restatements.

Shapes.  1, 63, 64, 65, 128, 129 and 257 free cameras (none held) over 300 points of 8 observations: the wave of 64, the dense cap, and
the 256 threads that share out the slots of a dot product; cameras whose lists hold exactly 63, 64, 65 and 129 observations (the lanes of
the slot sums, the tiles of the list ordering); track lengths 2 .. 5 and 63, 64, 65 ('c17'); T = 0, 1, 257; iters 0, 1, 10; cg_iters 1 and
2 (the cap is hit every round), 24 with cg_tol = 0, and 128 (an early stop: the launches behind it do nothing); huber 0 and 1.5; 'poison'
(an absent camera of NaN words, a held camera, bad indptr ranges and indices); 'T0' and 'T1' (every free camera held); 'two' (no free
camera); 'badcam' and 'behind' (the status bits); 'atmin' (a scene at its minimum: five rounds not taken, then nothing); 'rejtake'.

Measured on an MI355X (2026-10-21): on every fixture of CASES xyz, R, t, the costs and cg_res equal the restatement's bit for bit (the
largest difference is 0); function 14 and function 13 differ by at most 1.5e-14 ('c17', huber 1.5); 'e2e' ends at 0.737811 px with both
solvers and, run to the end, its costs differ from the dense run's by 3.2e-14.

End to end: the chain of tests/test_ba_gpu.py with solver='pcg'.  The rms reprojection error must not go up, and with the iteration run
to the end the history agrees with the dense run's: `taken` equal, the costs within 2 x TOL_PCG_VS_DENSE of max(1, |cost|) -- the bar was
measured over 10 rounds and this run has 20."""
import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import ba_ref as B
from tests.test_ba_cpu import relative_difference
from tests.test_ba_gpu import FILL, PAD, _dev, _planted_in_frame_of_camera_0
from tests.test_ba_gpu import run as run_dense
from tests.test_ba_pcg_cpu import CASES, DENSE_CASES, TOL_CG_RES, TOL_PCG, TOL_PCG_VS_DENSE, reference, scene
from tests.test_resect_gpu import _count_syncs
from tests.test_triangulate_cpu import E2E

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SIZES = lambda T, n_obs, n_images, iters: dict(xyz=24 * T, cams=144 * n_images, obs_error=4 * n_obs, cam_obs=4 * n_images, history=16 * (iters + 1),      # noqa: E731
                                               taken=iters, counters=32, cg_used=4 * iters, cg_res=8 * iters)


def _buffers(sc, iters, cg_iters, cg_tol):
    B_ = dict(indptr=_dev(sc["indptr"], (1,), np.int32), obs_image=_dev(sc["obs_image"], (1,), np.int32), obs_keypoint=_dev(sc["obs_keypoint"], (1,), np.int32),
              obs_use=_dev(sc["obs_use"], (1,), np.uint8), point_use=_dev(sc["point_use"], (1,), np.uint8), kpts=_dev(sc["kpts"], (1, 2), np.float32),
              xyz=_dev(sc["xyz"], (1, 3), np.float64), cams=_dev(sc["cams"], (1, 18), np.float64))
    B_["mode"] = np.ascontiguousarray(sc["mode"], dtype=np.int32)
    B_["table"] = hip.ba_table(*(B_[k] for k in ("indptr", "obs_image", "obs_keypoint", "obs_use", "point_use")), cg_iters=cg_iters, cg_tol=cg_tol)
    B_["dims"] = (len(sc["indptr"]) - 1, len(sc["obs_image"]), len(sc["mode"]), iters)
    B_["n"] = len(sc["kpts"])
    B_["layout"] = hip.ba_pcg_out_layout(*B_["dims"], int((sc["mode"] == 2).sum()))
    B_["out"] = torch.full((B_["layout"]["bytes"] + PAD,), FILL, dtype=torch.uint8, device="cuda")
    return B_


def _op(B_, huber, lambda0):
    T, n_obs, _, iters = B_["dims"]
    return hip.op_bundle_adjust_pcg(B_["table"], B_["kpts"], B_["xyz"], B_["cams"], B_["mode"], B_["out"], T, n_obs, B_["n"], iters, huber, lambda0)


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
               cam_obs=got["cam_obs"].view(np.int32), history=got["history"].view(np.float64).reshape(iters + 1, 2), taken=got["taken"],
               cg_used=got["cg_used"].view(np.int32), cg_res=got["cg_res"].view(np.float64))
    out["stats"] = dict(zip(hip.BA_COUNTERS, (int(v) for v in got["counters"].view(np.int32))))
    out["bytes"] = b"".join(got[k].tobytes() for k in SIZES(*B_["dims"]))
    return out


def run(sc, iters, huber=0.0, lambda0=1e-4, cg_iters=64, cg_tol=1e-6):
    B_ = _buffers(sc, iters, cg_iters, cg_tol)
    hip.run_ops(hip.make_ops([_op(B_, huber, lambda0)]))
    return _read(B_)


def same(got, want, sc):
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])
    np.testing.assert_array_equal(got["taken"], want["taken"])
    np.testing.assert_array_equal(got["cg_used"], want["cg_used"])
    np.testing.assert_array_equal(got["cam_obs"], want["cam_obs"])
    np.testing.assert_array_equal(got["history"][:, 1], want["history"][:, 1])          # lambda: the same divisions and products by ten
    np.testing.assert_array_equal(got["obs_error"] == -1, want["obs_error"] == -1)
    np.testing.assert_array_equal(got["cg_res"] == 0, want["cg_res"] == 0)
    assert np.isfinite(got["history"]).all() and np.isfinite(got["obs_error"]).all() and np.isfinite(got["cg_res"]).all()
    assert np.array_equal(np.isnan(got["xyz"]), np.isnan(np.asarray(sc["xyz"], np.float64))) and np.array_equal(np.isnan(got["cams"]), np.isnan(sc["cams"]))
    d = relative_difference(got, want, sc)
    dr = float(np.abs(got["cg_res"] - want["cg_res"]).max()) if len(want["cg_res"]) else 0.0
    print(f"xyz, R, t and the costs differ by {d:.3g}, the bar is {TOL_PCG:.3g}; cg_res by {dr:.3g}, the bar is {TOL_CG_RES:.3g}")
    assert d <= TOL_PCG, f"xyz, R, t or a cost differs by {d:.3g}, the bar is {TOL_PCG:.3g}"
    assert dr <= TOL_CG_RES, f"cg_res differs by {dr:.3g}, the bar is {TOL_CG_RES:.3g}"
    bar = 2.0 ** -23 * np.abs(want["obs_error"]) + 2 * want["obs_sens"] * TOL_PCG
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
        assert (got["obs_error"] == -1).all() and got["taken"].sum() == 0 and (got["history"][:, 0] == 0).all() and (got["cg_used"] == 0).all()
    still = np.ones((len(sc["mode"]), 18), bool)
    free = np.flatnonzero((sc["mode"] == 2) & (want["cam_obs"] >= 4))
    still[free, 4:16] = False
    assert got["cams"][still].tobytes() == np.asarray(sc["cams"], np.float64)[still].tobytes()


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("name,iters,huber,lambda0,cg_iters,cg_tol", CASES)
def test_against_the_restatement(name, iters, huber, lambda0, cg_iters, cg_tol):
    sc = scene(name)
    got, want = run(sc, iters, huber, lambda0, cg_iters, cg_tol), reference(name, iters, huber, lambda0, cg_iters, cg_tol)
    print(name, got["stats"], got["taken"].tolist(), got["cg_used"].tolist(), f"cost {got['history'][0, 0]:.6g} -> {got['history'][-1, 0]:.6g}")
    same(got, want, sc)
    assert run(sc, iters, huber, lambda0, cg_iters, cg_tol)["bytes"] == got["bytes"], "two runs on the same input differ"
    if name.startswith("f"):
        assert got["stats"]["n_free"] == int(name[1:]) and got["stats"]["n_held"] == 0
    if name.startswith("L"):
        assert got["cam_obs"].tolist() == [int(name[1:])] * 4
    if name in ("badcam", "behind"):
        assert got["stats"]["status"] == (hip.BA_BAD_CAMERA if name == "badcam" else hip.BA_BAD_START)
    if name == "atmin":
        assert got["taken"].sum() == 0 and got["history"][5, 1] == got["history"][-1, 1] and (got["cg_used"][5:] == 0).all()
    if name in ("T0", "T1"):
        assert got["stats"]["n_free"] == 0 and got["stats"]["n_held"] == 3 and (got["cg_used"] == 0).all()
    if cg_iters <= 2 and iters:
        assert got["cg_used"][0] == cg_iters and got["cg_res"][0] > cg_tol                  # the cap is hit
    if cg_iters == 128 and iters:
        assert got["cg_used"].max() < 128                                                    # an early stop: the launches behind it do nothing


@pytest.mark.parametrize("name,iters,huber,lambda0,cg_iters,cg_tol", DENSE_CASES)
def test_the_two_forms_agree_on_the_device(name, iters, huber, lambda0, cg_iters, cg_tol):
    sc = scene(name)
    got, want = run(sc, iters, huber, lambda0, cg_iters, cg_tol), run_dense(sc, iters, huber, lambda0)
    assert got["stats"] == want["stats"] and (got["taken"] == want["taken"]).all() and (got["history"][:, 1] == want["history"][:, 1]).all()
    np.testing.assert_array_equal(got["cam_obs"], want["cam_obs"])
    d = relative_difference(got, want, sc)
    print(name, f"function 14 and function 13 differ by {d:.3g}, the bar is {TOL_PCG_VS_DENSE:.3g}; cg_used {got['cg_used'].tolist()}")
    assert d <= TOL_PCG_VS_DENSE


def test_refused_before_any_launch_leaves_the_buffer_alone():
    sc = scene("c5")
    for kw, word in ((dict(cg_iters=0), "cg_iters = 0"), (dict(cg_tol=1.0), "cg_tol"), (dict(mode=np.array([1, 1, 2, 2, 3], np.int32)), "image 4: mode = 3")):
        B_ = _buffers(dict(sc, mode=kw.get("mode", sc["mode"])), 3, kw.get("cg_iters", 64), kw.get("cg_tol", 1e-6))
        with pytest.raises(hip.GimsHipError, match="bundle_adjust: .*" + word):
            hip.run_ops(hip.make_ops([_op(B_, 0.0, 1e-4)]))
        torch.cuda.synchronize()
        assert bool((B_["out"] == FILL).all())


# ------------------------------------------------------------------------------------------------ a captured graph
@pytest.mark.parametrize("name,iters,huber,cg_iters,cg_tol", [("poison", 10, 1.5, 128, 1e-6), ("f129", 2, 0.0, 64, 1e-6)])
def test_the_op_replays_from_a_captured_graph(name, iters, huber, cg_iters, cg_tol):
    """The same bytes from the direct run, a second direct run on the same buffer and the captured graph: every decision lives on the device."""
    sc = scene(name)
    alone = run(sc, iters, huber, 1e-4, cg_iters, cg_tol)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        B_ = _buffers(sc, iters, cg_iters, cg_tol)
        ops = hip.make_ops([_op(B_, huber, 1e-4)])
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


# ------------------------------------------------------------------------------------------------ the Python layer
class _Points:
    def __init__(self, sc):
        self.xyz = torch.from_numpy(np.asarray(sc["xyz"], np.float64)).cuda()
        self.valid = torch.from_numpy(sc["point_use"].astype(bool)).cuda()
        self.obs_inlier = torch.from_numpy(sc["obs_use"].astype(np.uint8)).cuda()


def test_131_images_run_with_pcg_where_the_default_raises(monkeypatch):
    """'f129' through gims_amd.bundle_adjust: 131 posed images, the first and the last fixed.  The default solver refuses 129 free cameras;
    solver='pcg' runs, without a host synchronisation, and gives what the restatement gives."""
    sc = scene("f129")
    counts = [int(c) for c in sc["cams"][:, 17]]
    start = [0] + [int(v) for v in np.cumsum(counts)]
    assert [int(f) for f in sc["cams"][:, 16]] == start[:-1]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()      # noqa: E731
    T, n_obs = len(sc["xyz"]), len(sc["obs_image"])
    tracks = gims_amd.Tracks(torch.zeros(start[-1], dtype=torch.int32, device="cuda"), i32(sc["indptr"]), i32(sc["obs_image"]), i32(sc["obs_keypoint"]),
                             torch.zeros(T, dtype=torch.uint8, device="cuda"), dict(n_tracks=T, n_obs=n_obs, n_conflicting=0, n_edges=0, n_bad=0, status=0), start)
    images = [torch.from_numpy(sc["kpts"][a:b]).cuda() for a, b in zip(start, start[1:])]
    K = np.tile(np.eye(3), (131, 1, 1))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = sc["cams"][:, 0], sc["cams"][:, 1], sc["cams"][:, 2], sc["cams"][:, 3]
    cams = (K, sc["cams"][:, 4:13].reshape(-1, 3, 3).copy(), sc["cams"][:, 13:16].copy())
    pts = _Points(sc)
    with pytest.raises(ValueError, match="129 free cameras, at most 128"):
        gims_amd.bundle_adjust(pts, tracks, images, cams, fixed=[0, 130], iters=2)
    torch.cuda.synchronize()
    syncs = _count_syncs(monkeypatch)
    adj = gims_amd.bundle_adjust(pts, tracks, images, cams, fixed=[0, 130], iters=2, solver="pcg")
    assert syncs == {"device": 0, "stream": 0, "event": 0, "item": 0}, syncs            # no host synchronisation at all
    stats = adj.stats
    assert syncs == {"device": 0, "stream": 0, "event": 1, "item": 1}, syncs            # .stats: one event, then the pinned words
    monkeypatch.undo()
    want = reference("f129", 2, 0.0, 1e-4, 64, 1e-6)                                    # the defaults of the Python layer
    assert stats == want["stats"] and stats["n_free"] == 129
    got = dict(xyz=adj.xyz.cpu().numpy(), cams=adj.records.cpu().numpy(), history=adj.history.cpu().numpy())
    assert adj.taken.cpu().numpy().tolist() == want["taken"].tolist() and adj.cg_used.cpu().numpy().tolist() == want["cg_used"].tolist()
    assert adj.cg_used.dtype == torch.int32 and adj.cg_res.dtype == torch.float64 and adj.cg_res.shape == (2,) and adj.cg_used.is_cuda
    d = relative_difference(got, want, sc)
    print(f"'f129' through gims_amd.bundle_adjust(solver='pcg'): {stats}, cg_used {want['cg_used'].tolist()}, differs from the restatement by {d:.3g}")
    assert d <= TOL_PCG


def test_end_to_end(monkeypatch):
    m = B.TR.planted_matches(**E2E)
    n_cams = E2E["n_cams"]
    kpts = [torch.from_numpy(k).cuda() for k in m["kpts"]]
    outs = [{"matches0": torch.from_numpy(x).cuda().reshape(1, -1)} for x in m["matches"]]
    tracks = gims_amd.build_tracks(m["counts"], m["pairs"], outs)
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
    adj = gims_amd.bundle_adjust(pts, tracks, kpts, cams, iters=20, solver="pcg")
    assert counts == {"device": 0, "stream": 0, "event": 0, "item": 0}, counts          # no host synchronisation at all
    monkeypatch.undo()
    stats = adj.stats
    dense = gims_amd.bundle_adjust(pts, tracks, kpts, cams, iters=20)
    assert dense.cg_used is None and dense.cg_res is None and stats == dense.stats and stats["status"] == 0 and stats["rounds_taken"] >= 1
    hist, hist_dense, used = adj.history.cpu().numpy(), dense.history.cpu().numpy(), adj.cg_used.cpu().numpy()
    rms0, rms1, rms_dense = (np.sqrt(h / stats["n_active_obs"]) for h in (hist[0, 0], hist[-1, 0], hist_dense[-1, 0]))
    posed = np.isfinite(cams[1]).all(axis=(1, 2))
    Rp, tp = _planted_in_frame_of_camera_0(m)
    Ka, Ra, ta = adj.cameras()
    print(f"'e2e', solver='pcg' (cg_iters 64, cg_tol 1e-6): {stats}; rms reprojection error {rms0:.4g} -> {rms1:.6g} px (dense: {rms_dense:.6g}); cg_used {used.tolist()}; "
          f"worst |dR| {np.abs(Ra - Rp)[posed].max():.3g}, |dt| {np.abs(ta - tp)[posed].max():.3g} against the planted cameras")
    assert rms1 <= rms0 and (Ra[:2] == cams[1][:2]).all() and (ta[:2] == cams[2][:2]).all()
    assert (used[adj.taken.cpu().numpy() == 1] > 0).all() and used.max() <= 64
    # run to the end, the iteration gives the dense form's history
    full = gims_amd.bundle_adjust(pts, tracks, kpts, cams, iters=20, solver="pcg", cg_iters=128, cg_tol=1e-12)
    hist_full = full.history.cpu().numpy()
    d = float((np.abs(hist_full[:, 0] - hist_dense[:, 0]) / np.maximum(1.0, np.abs(hist_dense[:, 0]))).max())
    print(f"'e2e', cg_tol 1e-12: the costs of the history differ from the dense run's by {d:.3g}, the bar is {2 * TOL_PCG_VS_DENSE:.3g}; cg_used {full.cg_used.cpu().numpy().tolist()}")
    assert full.taken.cpu().numpy().tolist() == dense.taken.cpu().numpy().tolist() and (hist_full[:, 1] == hist_dense[:, 1]).all()
    assert d <= 2 * TOL_PCG_VS_DENSE
