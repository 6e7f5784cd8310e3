"""GPU tests of bundle adjustment with focal groups: GIMS_AUX_BUNDLE_ADJUST_FOCAL (gims_amd/csrc/ba.hip) against the NumPy
restatement (tests/ba_focal_ref.py) on the fixtures of tests/test_ba_focal_cpu.py, which asserts their margins: taken, cg_used, the
counters, cam_obs, group_obs, the lambda column of the history and the pattern of inactive observations compare exactly, the floats
within TOL_FOCAL (16 x the restatement's own spread between forward and reverse summation, measured and asserted in
tests/test_ba_focal_cpu.py), each difference divided by max(1, |word|); cg_res within TOL_CG_RES of tests/test_ba_pcg_cpu.py; obs_error:
float32 storage + 2 |d e / d parameter| TOL_FOCAL.  Equality to the bit is what is expected: every comparison prints its largest
difference.  The op is called through a table on a buffer filled with 0xA5; every output must be overwritten, neither the padding
between the regions nor the 256 bytes behind the buffer may change, and a second run and a captured graph must give the same bytes.

Shapes.  Groups: one shared, two, one per image with 3, 5 and 17 images, none (the shared regions must hold function 14's bytes, run in
the same test), the two fixed cameras only, a group of the absent image only and a group of fewer than four observations (both held),
n_free == 0 with a moving shared group.  63, 64, 65, 255, 256 and 257 images in one group over 300 tracks of 8 observations (the lanes
of a wave and the 256 threads of the group sum); 255, 256 and 257 groups over 259 images (the group sum of a dot product); fixed images
whose lists hold exactly 63, 64 and 65 observations; iters 0, 1, 10; cg_iters 1 and 2 (the cap is hit); huber 0 and 1.5; 'rejtake' (a
refused round, then a taken one); 'mirror' (candidates with 1 + ds <= 0: four refused rounds then a taken one, and five refusals then
idle); 'badcam' and 'behind' (the status bits).

Measured on an MI355X (2026-10-21): on every fixture of CASES xyz, R, t, fx, fy, focal_scale, the costs and cg_res equal the restatement's
bit for bit (the largest difference is 0), and so does the Python layer; with every id -1, and with a single held group, the nine shared
regions hold function 14's bytes.

End to end: the chain of tests/test_ba_gpu.py with K scaled by 1.05 before it runs.  refine_focal='shared' ends at 0.663102 px against
0.684958 px without (from 1.235 px), with focal_scale 0.950036 (x 1.05 = 0.9975)."""
import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import ba_ref as B
from tests.test_ba_focal_cpu import CASES, TOL_FOCAL, fixture, focal_difference, reference
from tests.test_ba_gpu import FILL, PAD, _dev
from tests.test_ba_pcg_cpu import TOL_CG_RES
from tests.test_ba_pcg_gpu import run as run_pcg
from tests.test_resect_gpu import _count_syncs
from tests.test_triangulate_cpu import E2E

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SHARED = ("xyz", "cams", "obs_error", "cam_obs", "history", "taken", "counters", "cg_used", "cg_res")      # the regions function 14 has too


def SIZES(T, n_obs, n_images, iters, n_groups):
    return dict(xyz=24 * T, cams=144 * n_images, obs_error=4 * n_obs, cam_obs=4 * n_images, history=16 * (iters + 1), taken=iters, counters=32, cg_used=4 * iters,
                cg_res=8 * iters, focal_scale=8 * n_groups, group_obs=4 * n_groups)


def _buffers(sc, group, iters, cg_iters, cg_tol):
    B_ = dict(indptr=_dev(sc["indptr"], (1,), np.int32), obs_image=_dev(sc["obs_image"], (1,), np.int32), obs_keypoint=_dev(sc["obs_keypoint"], (1,), np.int32),
              obs_use=_dev(sc["obs_use"], (1,), np.uint8), point_use=_dev(sc["point_use"], (1,), np.uint8), kpts=_dev(sc["kpts"], (1, 2), np.float32),
              xyz=_dev(sc["xyz"], (1, 3), np.float64), cams=_dev(sc["cams"], (1, 18), np.float64))
    B_["mode"], B_["group"] = np.ascontiguousarray(sc["mode"], dtype=np.int32), np.ascontiguousarray(group, dtype=np.int32)
    B_["table"] = hip.ba_table(*(B_[k] for k in ("indptr", "obs_image", "obs_keypoint", "obs_use", "point_use")), cg_iters=cg_iters, cg_tol=cg_tol, group=B_["group"])
    n_groups = hip.ba_focal_groups(B_["mode"], B_["group"])
    B_["dims"] = (len(sc["indptr"]) - 1, len(sc["obs_image"]), len(sc["mode"]), iters, n_groups)
    B_["n"] = len(sc["kpts"])
    B_["layout"] = hip.ba_focal_out_layout(*B_["dims"][:4], int((sc["mode"] == 2).sum()), n_groups)
    B_["out"] = torch.full((B_["layout"]["bytes"] + PAD,), FILL, dtype=torch.uint8, device="cuda")
    return B_


def _op(B_, huber, lambda0):
    T, n_obs, _, iters, _ = B_["dims"]
    return hip.op_bundle_adjust_focal(B_["table"], B_["kpts"], B_["xyz"], B_["cams"], B_["mode"], B_["out"], T, n_obs, B_["n"], iters, huber, lambda0)


def _read(B_):
    """The outputs as the restatement returns them, and their bytes.  The padding between the regions and the bytes behind the buffer must
    be as they were."""
    torch.cuda.synchronize()
    raw, o = B_["out"].cpu().numpy(), B_["layout"]
    T, n_obs, n_images, iters, n_groups = B_["dims"]
    assert (raw[o["bytes"]:] == FILL).all(), "bytes behind the buffer were written"
    got, padding = {}, np.ones(o["outputs"], dtype=bool)
    for name, size in SIZES(*B_["dims"]).items():
        got[name] = raw[o[name]:o[name] + size].copy()
        padding[o[name]:o[name] + size] = False
    assert (raw[:o["outputs"]][padding] == FILL).all(), "the padding between the output regions was written"
    out = dict(xyz=got["xyz"].view(np.float64).reshape(T, 3), cams=got["cams"].view(np.float64).reshape(n_images, 18), obs_error=got["obs_error"].view(np.float32),
               cam_obs=got["cam_obs"].view(np.int32), history=got["history"].view(np.float64).reshape(iters + 1, 2), taken=got["taken"],
               cg_used=got["cg_used"].view(np.int32), cg_res=got["cg_res"].view(np.float64), focal_scale=got["focal_scale"].view(np.float64),
               group_obs=got["group_obs"].view(np.int32))
    out["stats"] = dict(zip(hip.BA_COUNTERS, (int(v) for v in got["counters"].view(np.int32))))
    out["bytes"] = b"".join(got[k].tobytes() for k in SIZES(*B_["dims"]))
    out["shared_bytes"] = b"".join(got[k].tobytes() for k in SHARED)
    return out


def run(name, iters, huber=0.0, lambda0=1e-4, cg_iters=64, cg_tol=1e-6):
    sc, group = fixture(name)
    B_ = _buffers(sc, group, iters, cg_iters, cg_tol)
    hip.run_ops(hip.make_ops([_op(B_, huber, lambda0)]))
    return _read(B_)


def same(got, want, sc, group):
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])
    np.testing.assert_array_equal(got["taken"], want["taken"])
    np.testing.assert_array_equal(got["cg_used"], want["cg_used"])
    np.testing.assert_array_equal(got["cam_obs"], want["cam_obs"])
    np.testing.assert_array_equal(got["group_obs"], want["group_obs"])
    np.testing.assert_array_equal(got["history"][:, 1], want["history"][:, 1])          # lambda: the same divisions and products by ten
    np.testing.assert_array_equal(got["obs_error"] == -1, want["obs_error"] == -1)
    np.testing.assert_array_equal(got["cg_res"] == 0, want["cg_res"] == 0)
    assert np.isfinite(got["history"]).all() and np.isfinite(got["obs_error"]).all() and np.isfinite(got["cg_res"]).all() and np.isfinite(got["focal_scale"]).all()
    assert np.array_equal(np.isnan(got["xyz"]), np.isnan(np.asarray(sc["xyz"], np.float64))) and np.array_equal(np.isnan(got["cams"]), np.isnan(sc["cams"]))
    d = focal_difference(got, want, sc)
    dr = float(np.abs(got["cg_res"] - want["cg_res"]).max()) if len(want["cg_res"]) else 0.0
    print(f"xyz, R, t, fx, fy, focal_scale and the costs differ by {d:.3g}, the bar is {TOL_FOCAL:.3g}; cg_res by {dr:.3g}, the bar is {TOL_CG_RES:.3g}; "
          f"equal to the bit: {d == 0 and dr == 0}")
    assert d <= TOL_FOCAL, f"xyz, R, t, fx, fy, focal_scale or a cost differs by {d:.3g}, the bar is {TOL_FOCAL:.3g}"
    assert dr <= TOL_CG_RES, f"cg_res differs by {dr:.3g}, the bar is {TOL_CG_RES:.3g}"
    bar = 2.0 ** -23 * np.abs(want["obs_error"]) + 2 * want["obs_sens"] * TOL_FOCAL
    de = np.abs(got["obs_error"].astype(np.float64) - want["obs_error"])
    assert (de <= bar).all(), f"obs_error: {de.max():.3g} at {int(np.argmax(de - bar))}, bar {bar[int(np.argmax(de - bar))]:.3g}"
    # what does not move is copied through bit for bit: inactive points, the pose of absent / fixed / held cameras, fx and fy outside the
    # groups that move, cx, cy and the last two words of every camera
    start, cams0 = np.asarray(sc["xyz"], np.float64), np.asarray(sc["cams"], np.float64)
    if want["stats"]["status"] != 0:
        assert got["xyz"].tobytes() == start.tobytes() and got["cams"].tobytes() == cams0.tobytes() and (got["focal_scale"] == 1).all()
        assert (got["obs_error"] == -1).all() and got["taken"].sum() == 0 and (got["history"][:, 0] == 0).all() and (got["cg_used"] == 0).all()
    still = np.ones((len(sc["mode"]), 18), bool)
    still[np.flatnonzero((sc["mode"] == 2) & (want["cam_obs"] >= 4)), 4:16] = False
    g = np.where(sc["mode"] != 0, group, -1)
    moving = (g >= 0) & (want["group_obs"][np.maximum(g, 0)] >= 4) if len(want["group_obs"]) else np.zeros(len(g), bool)
    still[moving, 0:2] = False
    assert got["cams"][still].tobytes() == cams0[still].tobytes()
    assert (got["focal_scale"][want["group_obs"] < 4] == 1).all()


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("name,iters,huber,lambda0,cg_iters,cg_tol", CASES)
def test_against_the_restatement(name, iters, huber, lambda0, cg_iters, cg_tol):
    sc, group = fixture(name)
    got, want = run(name, iters, huber, lambda0, cg_iters, cg_tol), reference(name, iters, huber, lambda0, cg_iters, cg_tol)
    print(name, got["stats"], got["taken"].tolist(), got["cg_used"].tolist(), f"cost {got['history'][0, 0]:.6g} -> {got['history'][-1, 0]:.6g}", got["focal_scale"][:4])
    same(got, want, sc, group)
    assert run(name, iters, huber, lambda0, cg_iters, cg_tol)["bytes"] == got["bytes"], "two runs on the same input differ"
    if name[0] in "gd":
        n = int(name[1:])
        assert len(got["focal_scale"]) == (1 if name[0] == "g" else n) and got["stats"]["rounds_taken"] == 2 and (got["focal_scale"][got["group_obs"] >= 4] != 1).all()
    if name[0] == "L":
        assert got["cam_obs"].tolist() == [int(name[1:])] * 4 and got["stats"]["n_fixed"] == 2
    if name in ("badcam", "behind"):
        assert got["stats"]["status"] == (hip.BA_BAD_CAMERA if name == "badcam" else hip.BA_BAD_START)
    if name == "mirror":
        assert got["taken"][0] == 0 and got["cg_used"][0] > 0 and (got["taken"].sum() > 0) == (lambda0 == 1e-4)
    if name == "nfree0":
        assert got["stats"]["n_free"] == 0 and got["stats"]["rounds_taken"] >= 2 and got["focal_scale"][0] != 1
    if name in ("few", "absent"):
        assert got["focal_scale"][0] == 1 and got["group_obs"][0] == (3 if name == "few" else 0)
    if cg_iters <= 2 and iters:
        assert got["cg_used"][0] == cg_iters and got["cg_res"][0] > cg_tol                  # the cap is hit


def test_without_a_group_the_shared_regions_hold_function_14s_bytes():
    """All ids -1, and a single held group: function 14 on the same input, run here, gives the same bytes in the nine regions it has."""
    for name, iters, huber in (("none5", 10, 0.0), ("none5", 10, 1.5), ("few", 10, 0.0)):
        sc, _ = fixture(name)
        got, want = run(name, iters, huber, 1e-4, 128, 1e-6), run_pcg(sc, iters, huber, 1e-4, 128, 1e-6)
        assert got["shared_bytes"] == want["bytes"] and got["stats"]["rounds_taken"] >= 2, name
        assert len(got["focal_scale"]) == (0 if name == "none5" else 1)


def test_refused_before_any_launch_leaves_the_buffer_alone():
    sc, group = fixture("shared5")
    for kw, word in ((dict(group=np.array([0, 0, 5, 0, 0], np.int32)), "image 2: group = 5"), (dict(group=np.array([0, -2, 0, 0, 0], np.int32)), "image 1: group = -2"),
                     (dict(cg_iters=0), "cg_iters = 0"), (dict(mode=np.array([1, 1, 2, 2, 3], np.int32)), "image 4: mode = 3")):
        B_ = _buffers(dict(sc, mode=kw.get("mode", sc["mode"])), kw.get("group", group), 3, kw.get("cg_iters", 64), 1e-6)
        with pytest.raises(hip.GimsHipError, match="bundle_adjust: .*" + word):
            hip.run_ops(hip.make_ops([_op(B_, 0.0, 1e-4)]))
        torch.cuda.synchronize()
        assert bool((B_["out"] == FILL).all())


# ------------------------------------------------------------------------------------------------ a captured graph
@pytest.mark.parametrize("name,iters,huber,cg_iters,cg_tol", [("absent", 10, 1.5, 128, 1e-6), ("g65", 2, 0.0, 64, 1e-6), ("mirror", 10, 0.0, 128, 1e-6)])
def test_the_op_replays_from_a_captured_graph(name, iters, huber, cg_iters, cg_tol):
    """The same bytes from the direct run, a second direct run on the same buffer and the captured graph: every decision lives on the device."""
    sc, group = fixture(name)
    alone = run(name, iters, huber, 1e-4, cg_iters, cg_tol)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        B_ = _buffers(sc, group, iters, cg_iters, cg_tol)
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


def _python_inputs(sc):
    counts = [int(c) for c in sc["cams"][:, 17]]
    start = [0] + [int(v) for v in np.cumsum(counts)]
    assert [int(f) for f in sc["cams"][:, 16]] == start[:-1]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()      # noqa: E731
    T, n_obs, n = len(sc["xyz"]), len(sc["obs_image"]), len(sc["cams"])
    tracks = gims_amd.Tracks(torch.zeros(start[-1], dtype=torch.int32, device="cuda"), i32(sc["indptr"]), i32(sc["obs_image"]), i32(sc["obs_keypoint"]),
                             torch.zeros(T, dtype=torch.uint8, device="cuda"), dict(n_tracks=T, n_obs=n_obs, n_conflicting=0, n_edges=0, n_bad=0, status=0), start)
    images = [torch.from_numpy(sc["kpts"][a:b]).cuda() for a, b in zip(start, start[1:])]
    K = np.tile(np.eye(3), (n, 1, 1))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = sc["cams"][:, 0], sc["cams"][:, 1], sc["cams"][:, 2], sc["cams"][:, 3]
    return _Points(sc), tracks, images, (K, sc["cams"][:, 4:13].reshape(-1, 3, 3).copy(), sc["cams"][:, 13:16].copy())


@pytest.mark.parametrize("name,refine", [("g65", "shared"), ("per17", "per_image"), ("two5", [7, 7, 3, 3, 3])])
def test_refine_focal_through_the_python_layer(monkeypatch, name, refine):
    """gims_amd.bundle_adjust(solver='pcg', refine_focal=...): no host synchronisation, the restatement's result, the refined K."""
    sc, group = fixture(name)
    iters = 2 if name == "g65" else 10
    pts, tracks, images, cams = _python_inputs(sc)
    fixed = [int(k) for k in np.flatnonzero(sc["mode"] == 1)]
    with pytest.raises(ValueError, match="solver='pcg'"):
        gims_amd.bundle_adjust(pts, tracks, images, cams, fixed=fixed, iters=iters, refine_focal=refine)
    torch.cuda.synchronize()
    syncs = _count_syncs(monkeypatch)
    adj = gims_amd.bundle_adjust(pts, tracks, images, cams, fixed=fixed, iters=iters, solver="pcg", refine_focal=refine)
    assert syncs == {"device": 0, "stream": 0, "event": 0, "item": 0}, syncs            # no host synchronisation at all
    monkeypatch.undo()
    want = reference(name, iters, 0.0, 1e-4, 64, 1e-6)                                  # the defaults of the Python layer
    assert adj.stats == want["stats"] and adj.group == group.tolist()
    got = dict(xyz=adj.xyz.cpu().numpy(), cams=adj.records.cpu().numpy(), history=adj.history.cpu().numpy(), focal_scale=adj.focal_scale.cpu().numpy())
    assert adj.taken.cpu().numpy().tolist() == want["taken"].tolist() and adj.cg_used.cpu().numpy().tolist() == want["cg_used"].tolist()
    assert adj.group_obs.cpu().numpy().tolist() == want["group_obs"].tolist() and adj.group_obs.dtype == torch.int32 and adj.focal_scale.dtype == torch.float64
    d = focal_difference(got, want, sc)
    print(f"'{name}' through gims_amd.bundle_adjust(refine_focal={refine!r}): focal_scale {got['focal_scale'][:4]}, differs from the restatement by {d:.3g}")
    assert d <= TOL_FOCAL
    assert adj.K.shape == (len(sc["mode"]), 4) and adj.K.is_cuda and (adj.K.cpu().numpy() == got["cams"][:, :4]).all()
    Ka, Ra, ta = adj.cameras()
    assert (Ka[:, 0, 0] == got["cams"][:, 0]).all() and (Ka[:, 1, 1] == got["cams"][:, 1]).all() and (Ka[:, :2, 2] == cams[0][:, :2, 2]).all()
    assert (Ka[:, 0, 0] != cams[0][:, 0, 0]).all() and np.abs(Ka[:, 0, 0] / cams[0][:, 0, 0] - got["focal_scale"][group]).max() < 1e-12
    plain = gims_amd.bundle_adjust(pts, tracks, images, cams, fixed=fixed, iters=iters, solver="pcg")
    assert plain.focal_scale is None and plain.group_obs is None and plain.group is None and (plain.cameras()[0] == cams[0]).all()
    assert (plain.K.cpu().numpy() == sc["cams"][:, :4]).all()


def test_end_to_end(monkeypatch):
    """The chain with K scaled by 1.05 before it runs: refine_focal='shared' ends lower than the same call without, the returned K differs
    from the input K by the returned focal_scale, and triangulate_tracks takes the refined records where they lie."""
    m = B.TR.planted_matches(**E2E)
    n_cams = E2E["n_cams"]
    K = m["K"].copy()
    K[:, 0, 0], K[:, 1, 1] = 1.05 * K[:, 0, 0], 1.05 * K[:, 1, 1]
    kpts = [torch.from_numpy(k).cuda() for k in m["kpts"]]
    outs = [{"matches0": torch.from_numpy(x).cuda().reshape(1, -1)} for x in m["matches"]]
    tracks = gims_amd.build_tracks(m["counts"], m["pairs"], outs)
    good = m["matches"][0] >= 0
    Rr, tr, _ = gims_amd.estimate_pose(m["kpts"][0][good], m["kpts"][1][m["matches"][0][good]], K[0], K[1])
    K2, R2, t2 = gims_amd.cameras_from_pose(K[0], K[1], Rr, tr)
    Rn, tn = np.full((n_cams, 3, 3), np.nan), np.full((n_cams, 3), np.nan)
    Rn[:2], tn[:2] = R2, t2
    first = gims_amd.triangulate_tracks(tracks, kpts, (K, Rn, tn))
    poses = gims_amd.resect_images(first, tracks, kpts, K, which=list(range(2, n_cams)), iters=256, seed=7)
    cams = poses.cameras(K, Rn, tn)
    pts = gims_amd.triangulate_tracks(tracks, kpts, cams)
    torch.cuda.synchronize()
    counts = _count_syncs(monkeypatch)
    adj = gims_amd.bundle_adjust(pts, tracks, kpts, cams, iters=20, solver="pcg", refine_focal="shared")
    assert counts == {"device": 0, "stream": 0, "event": 0, "item": 0}, counts          # no host synchronisation at all
    monkeypatch.undo()
    plain = gims_amd.bundle_adjust(pts, tracks, kpts, cams, iters=20, solver="pcg")
    stats = adj.stats
    assert stats["status"] == 0 and stats["rounds_taken"] >= 1 and stats["n_active_obs"] == plain.stats["n_active_obs"]
    rms0, rms1, rms_plain = (float(np.sqrt(h / stats["n_active_obs"])) for h in (adj.history.cpu().numpy()[0, 0], adj.history.cpu().numpy()[-1, 0],
                                                                              plain.history.cpu().numpy()[-1, 0]))
    scale = adj.focal_scale.cpu().numpy()
    Ka, Ra, ta = adj.cameras()
    posed = np.isfinite(cams[1]).all(axis=(1, 2))
    print(f"'e2e' with K x 1.05: {stats}; rms {rms0:.4g} -> {rms1:.6g} px with refine_focal='shared' (focal_scale {scale[0]:.6f}, x 1.05 = {1.05 * scale[0]:.6f}), "
          f"{rms_plain:.6g} px without; cg_used {adj.cg_used.cpu().numpy().tolist()}")
    assert rms1 < rms_plain and rms1 <= rms0
    assert scale.shape == (1,) and scale[0] != 1 and int(adj.group_obs.cpu()[0]) == stats["n_active_obs"]
    assert (Ka[posed, 0, 0] != cams[0][posed, 0, 0]).all() and np.abs(Ka[posed, 0, 0] / cams[0][posed, 0, 0] - scale[0]).max() < 1e-12
    assert np.abs(Ka[posed, 1, 1] / cams[0][posed, 1, 1] - scale[0]).max() < 1e-12 and (Ka[:, :2, 2] == cams[0][:, :2, 2]).all() and (Ka[~posed] == cams[0][~posed]).all()
    again = gims_amd.triangulate_tracks(tracks, kpts, adj.records)                      # the refined focal lengths flow on where they lie
    torch.cuda.synchronize()
    assert int(again.valid.sum()) > 0
