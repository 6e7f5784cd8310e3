"""CPU tests of the track triangulation: the ABI constant and the pins a feature must leave alone, the argument checks of
GIMS_AUX_TRIANGULATE_TRACKS (they run before any HIP call), the layout of its one buffer, the ValueErrors of gims_amd.triangulate_tracks, the
NumPy restatement (tests/triangulate_ref.py) on planted scenes, and the conditions on the fixtures that tests/test_triangulate_gpu.py compares
exactly with the device: their margins, and the float bar TOL_X.

Worst error of the restatement against the planted points (scene extent 1, cameras at distance 4, focal length 800 px), as measured here:
  noise-free tracks of 2 .. 9 views       2.8e-07  (the keypoints are float32: 6e-5 px of rounding at 1024 px)
  'seams', 0.5 px noise, 20 % wrong       3.2e-03  over the valid tracks
  'e2e', 0.5 px noise, 3 % wrong matches  see tests/test_triangulate_gpu.py

TOL_X.  Every fixture is solved twice by the restatement, its sums over observations taken forward and in reverse; the largest difference
of a coordinate, relative to the scene extent 1, is the restatement's own sensitivity to summation order, SPREAD.  TOL_X = 16 x SPREAD covers
the fused multiply-adds and the reduction trees of the device.  Measured here: SPREAD = 5.75e-10 (on 'batch'; 4.1e-10 on 'e2e', 2.4e-10 on
'poison', 2.6e-11 on 'long', 4e-12 and below on the others: where the guarded Gauss-Newton loop stops is itself a comparison of two costs
that agree to rounding), TOL_X = 9.2e-9.  test_tol_x_is_the_measured_one asserts that the number recorded here is the measured one."""
import functools

import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import tracks_ref
from tests import triangulate_ref as R

TOL_X = 9.2e-9            # 16 x the measured SPREAD, rounded up to two digits; test_tol_x_is_the_measured_one keeps it honest
EXTENT = 1.0
THRESH, MIN_ANGLE = 4.0, 1.5

# (max_hyp, refine_iters) of every fixture the GPU test compares exactly.  36 = E of the track of 9 observations.
SEAM_LENGTHS = [2, 3, 4, 5, 8, 9, 16, 17, 63, 64, 65]
SEAM_COMBOS = [(0, 10), (1, 0), (3, 10), (36, 10), (64, 0), (64, 10), (65535, 10)]
CASES = [("seams", c) for c in SEAM_COMBOS] + [("long", (64, 10)), ("batch", (64, 10)), ("edge", (64, 10)), ("edge0", (0, 10)), ("poison", (64, 10)),
                                               ("e2e", (64, 10))]
T_COUNTS = [0, 1, 7, 8, 9, 63, 64, 65, 257]
E2E = dict(seed=5, n_cams=8, n_points=400, n_kp=256, noise=0.5, w_wrong=0.03)


def _pick(sc):
    return {k: sc[k] for k in ("indptr", "obs_image", "obs_keypoint", "kpts", "cams")}


def edge_scene(drop=()):
    """Six arc cameras, a seventh that looks away from the scene and an eighth whose fx is zero.  Tracks: 0 a good pair; 1 a pair with one
    wrong observation (NO_MODEL); 2 three observations from one centre (degenerate: NO_MODEL); 3 three good views and one in the camera that
    looks away (a point behind a camera: that observation is no inlier); 4 a distant point seen by two neighbours (too little parallax: NO_MODEL
    with hypotheses, LOW_ANGLE without, the point still written); 5 two observations of image 0 and two others; 6 two good views and one in
    the bad camera; 7 one good view and one in the bad camera (TOO_SHORT).  drop: tracks to leave out ('edge0', the scene for max_hyp = 0, has
    no track 2: without hypotheses its point is the shared centre itself, where every depth is a rounding error and no decision is fair)."""
    rng = np.random.default_rng(11)
    K, Rm, t = R.arc_cameras(8)
    cen = np.array([-Rm[k].T @ t[k] for k in range(8)])
    Rm[6], t[6] = R.look_at(cen[6], 2 * cen[6])
    X = rng.uniform(-0.4, 0.4, (8, 3))
    X[4] = -80.0 * (cen[0] + cen[1]) / np.linalg.norm(cen[0] + cen[1])
    px = lambda k, j, noise=0.3: R.project(K[k], Rm[k], t[k], X[j]) + noise * rng.standard_normal(2)      # noqa: E731
    tracks = [[(0, px(0, 0)), (3, px(3, 0))],
              [(1, px(1, 1)), (4, np.array([37.0, 700.0]))],
              [(2, px(2, 2)), (2, px(2, 2)), (2, px(2, 2))],
              [(0, px(0, 3)), (2, px(2, 3)), (5, px(5, 3)), (6, np.array([500.0, 400.0]))],
              [(0, px(0, 4, 0.0)), (1, px(1, 4, 0.0))],
              [(0, px(0, 5)), (0, px(0, 5)), (3, px(3, 5)), (5, px(5, 5))],
              [(1, px(1, 6)), (4, px(4, 6)), (7, np.array([512.0, 384.0]))],
              [(2, px(2, 7)), (7, np.array([100.0, 100.0]))]]
    per = [[] for _ in range(8)]
    obs_image, obs_keypoint, indptr = [], [], [0]
    for tr in (tr for j, tr in enumerate(tracks) if j not in drop):
        for k, p in tr:
            obs_image.append(k)
            obs_keypoint.append(len(per[k]))
            per[k].append(p)
        indptr.append(len(obs_image))
    counts = [len(p) for p in per]
    K[7, 0, 0] = 0.0
    return dict(indptr=np.array(indptr, np.int32), obs_image=np.array(obs_image, np.int32), obs_keypoint=np.array(obs_keypoint, np.int32),
                kpts=np.concatenate([np.array(p).reshape(-1, 2) for p in per]).astype(np.float32), cams=R.camera_records(K, Rm, t, counts), points=X)


def poison_scene():
    """The first 40 tracks of 'batch' with poisoned entries: an image index out of range (track 3), a keypoint index >= n_k (5), a negative
    keypoint and a negative image index (8), a NaN pixel (13); an indptr that starts below zero (track 0), leaves n_obs (track 20) and
    descends (track 21): indptr[21] = n_obs + 5.  No two good ranges overlap, so every slot has one writer."""
    sc = {k: np.array(v, copy=True) for k, v in _pick(scene("batch")).items()}
    sc["indptr"], n_obs = sc["indptr"][:41], int(sc["indptr"][40])
    sc["obs_image"], sc["obs_keypoint"] = sc["obs_image"][:n_obs], sc["obs_keypoint"][:n_obs]
    ptr = sc["indptr"]
    sc["obs_image"][ptr[3]] = len(sc["cams"])
    sc["obs_keypoint"][ptr[5] + 1] = int(sc["cams"][sc["obs_image"][ptr[5] + 1], 17])
    sc["obs_keypoint"][ptr[8]] = -1
    sc["obs_image"][ptr[8] + 1] = -3
    k, i = sc["obs_image"][ptr[13]], sc["obs_keypoint"][ptr[13]]
    sc["kpts"][int(sc["cams"][k, 16]) + i, 1] = np.nan
    ptr[21] = n_obs + 5
    ptr[0] = -1
    return sc


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "seams":
        return R.planted_tracks(1, SEAM_LENGTHS)
    if name == "long":
        return R.planted_tracks(2, [128, 1024, 1025, 5])
    if name == "batch":
        lengths = np.random.default_rng(4).choice([2, 2, 3, 3, 4, 5, 6, 7, 8, 9, 10, 12, 17, 33], 257).tolist()
        return R.planted_tracks(4, lengths)
    if name == "edge":
        return edge_scene()
    if name == "edge0":
        return edge_scene(drop=(2,))
    if name == "poison":
        return poison_scene()
    if name == "e2e":
        m = R.planted_matches(**E2E)
        tr = tracks_ref.build(m["counts"], m["pairs"], m["matches"])
        return dict(indptr=tr["indptr"].astype(np.int32), obs_image=tr["obs_image"].astype(np.int32), obs_keypoint=tr["obs_keypoint"].astype(np.int32),
                    kpts=np.concatenate(m["kpts"]), cams=R.camera_records(m["K"], m["R"], m["t"], m["counts"]), matches=m, tracks=tr)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, combo, order="forward"):
    """The restatement on a fixture, computed once and shared (do not write to it) -> (result, trace)."""
    trace = {}
    out = R.triangulate(**_pick(scene(name)), thresh=THRESH, min_angle=MIN_ANGLE, max_hyp=combo[0], refine_iters=combo[1], order=order, trace=trace)
    return out, trace


def prefix(ref, sc, T):
    """The first T tracks of a fixture and of its reference (tracks do not depend on one another) -> (scene, reference)."""
    n_obs = int(sc["indptr"][T])
    sub = dict(_pick(sc), indptr=sc["indptr"][:T + 1], obs_image=sc["obs_image"][:n_obs], obs_keypoint=sc["obs_keypoint"][:n_obs])
    out = {k: (v[:n_obs] if k.startswith("obs_") else v[:T]) for k, v in ref.items() if k != "stats"}
    st, bad = out["status"], int(out["track_bad"].sum())
    out["stats"] = dict(n_ok=int((st == 0).sum()), n_low_angle=int((st == R.LOW_ANGLE).sum()), n_no_model=int((st == R.NO_MODEL).sum()),
                        n_too_short=int((st == R.TOO_SHORT).sum()), n_too_long=int((st == R.TOO_LONG).sum()), n_bad_obs=bad,
                        n_inlier_obs=int(out["n_inliers"].sum()))
    return sub, out


# ------------------------------------------------------------------------------------------------ pins, argument checks, layout
def test_abi_constant_and_pins():
    assert hip.AUX_TRIANGULATE_TRACKS == 10 == hip.ABI.constants["GIMS_AUX_TRIANGULATE_TRACKS"]
    # the feature adds no export, no struct and no ABI version
    assert len(hip.EXPORTS) == 90 and len(hip.ABI.structs) == 28 and hip.ABI_VERSION == 5 == hip.load().gims_abi_version()
    assert not any("triang" in name.lower() for name in hip.EXPORTS)
    assert hip.TRI_CAMERA_WORDS == 18 == R.CAMERA_WORDS and hip.TRI_MAX_OBS == 1024 == R.MAX_OBS and hip.TRI_COUNTERS == R.COUNTERS
    assert 2 <= hip.TRI_SHORT_TRACK <= 64 and 64 % hip.TRI_SHORT_TRACK == 0
    assert (hip.TRI_TOO_SHORT, hip.TRI_NO_MODEL, hip.TRI_LOW_ANGLE, hip.TRI_TOO_LONG) == (R.TOO_SHORT, R.NO_MODEL, R.LOW_ANGLE, R.TOO_LONG) == (1, 2, 4, 8)
    for name in ("triangulate_tracks", "Points3D", "cameras_from_pose"):
        assert getattr(gims_amd, name) is getattr(gims_amd.triangulate, name) and name in gims_amd.__all__
    # the lengths and counts the GPU test runs cover both seams of the lane grouping
    for seam in (hip.TRI_SHORT_TRACK, 64):
        assert {seam - 1, seam, seam + 1} <= set(SEAM_LENGTHS)


def _run(ptrs, ints, floats=(THRESH, MIN_ANGLE)):
    """Through hip.run_ops, on the null stream (no device is needed: a refused call makes no HIP call)."""
    with hip.on_stream(0):
        hip.run_ops(hip.make_ops([hip.op_aux(hip.AUX_TRIANGULATE_TRACKS, ptrs, ints, floats)]))


def test_argument_checks_come_before_any_hip_call():
    """Every GIMS_EINVAL case of the header, with a message naming triangulate_tracks; the pointers are never dereferenced."""
    p = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000]      # indptr, obs_image, obs_keypoint, kpts, cams, out
    good = [100, 400, 6, 900, 64 | (10 << 16), 0]                    # T, n_obs, n_images, N, max_hyp | refine_iters << 16, reserved

    def refused(ptrs, ints, word, floats=(THRESH, MIN_ANGLE)):
        with pytest.raises(hip.GimsHipError, match="triangulate_tracks") as e:
            _run(ptrs, ints, floats)
        assert word in str(e.value) and f"({hip.GIMS_EINVAL})" in str(e.value), str(e.value)

    def ints(**kw):
        return [kw.get(k, v) for k, v in zip(["T", "n_obs", "n_images", "N", "mode", "form"], good)]

    for name, word in (("T", "T = "), ("n_obs", "n_obs = "), ("N", "N = ")):
        refused(p, ints(**{name: -1}), word + "-1")
        refused(p, ints(**{name: (1 << 30) + 1}), "2^30")
    refused(p, ints(n_images=-1), "n_images = -1")
    refused(p, ints(n_images=(1 << 24) + 1), "2^24")
    refused(p, ints(mode=-1), "max_hyp")                                        # max_hyp is the low 16 bits of i[4]: 0 .. 65535 by construction
    refused(p, ints(mode=64 | (256 << 16)), "refine_iters in 0 .. 255")
    refused(p, ints(mode=1 << 40), "refine_iters in 0 .. 255")
    with pytest.raises(ValueError, match="max_hyp"):                            # ... so the binding refuses what would spill into refine_iters
        hip.op_triangulate_tracks(*p, 1, 2, 2, 2, max_hyp=65536)
    with pytest.raises(ValueError, match="refine_iters"):
        hip.op_triangulate_tracks(*p, 1, 2, 2, 2, refine_iters=256)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(p, good, "thresh", floats=(bad, MIN_ANGLE))
    for bad in (-0.5, 180.0, float("nan"), float("inf")):
        refused(p, good, "min_angle", floats=(THRESH, bad))
    for k in range(5):
        refused(p[:k] + [None] + p[k + 1:], good, "NULL while T = 100")
    refused(p[:5] + [None], good, "output buffer is NULL")
    refused(p[:5] + [None], ints(T=0), "output buffer is NULL")                 # T == 0 is checked like any other call
    for k in (4, 5):
        refused(p[:k] + [p[k] + 4] + p[k + 1:], good, "8-byte aligned")
    for k in range(4):
        refused(p[:k] + [p[k] + 2] + p[k + 1:], good, "4-byte aligned")
    refused(p, ints(form=1), "reserved")
    # i[5] would select a later form of the function, so it is read first: whatever the other words hold, this version does not know the call
    refused([None] * 6, [10, 10, 10, 10, 10, 10], "unknown auxiliary function form")
    refused([None] * 6, [-5, -5, -5, -5, -5, 7], "unknown auxiliary function form", floats=(float("nan"), float("nan")))


def test_out_layout():
    al = lambda x: (x + 255) & ~255      # noqa: E731
    for T, n_obs in ((0, 0), (1, 2), (7, 31), (64, 256), (257, 1300), (100000, 345678)):
        o = hip.triangulate_out_layout(T, n_obs)
        order = ["xyz", "max_angle", "rms_error", "n_inliers", "obs_error", "status", "obs_inlier", "counters"]
        sizes = [24 * T, 4 * T, 4 * T, 4 * T, 4 * n_obs, T, n_obs, 32]
        assert o["xyz"] == 0 and all(o[k] % 256 == 0 for k in order) and o["bytes"] % 256 == 0
        for a, b, size in zip(order, order[1:] + ["outputs"], sizes):
            assert o[b] - o[a] == al(size), (a, b)                              # back to back: nothing overlaps, nothing is wasted
        assert o["scratch"] == o["outputs"] and o["bytes"] - o["scratch"] == 2 * al(4 * T) + 256
    assert hip.triangulate_out_layout(257, 1300) == dict(xyz=0, max_angle=6400, rms_error=7680, n_inliers=8960, obs_error=10240, status=15616,
                                                         obs_inlier=16128, counters=17664, outputs=17920, scratch=17920, bytes=20736)
    rec = hip.triangulate_cameras(np.tile(np.diag([500.0, 510.0, 1.0]), (3, 1, 1)), np.tile(np.eye(3), (3, 1, 1)), np.arange(9.0).reshape(3, 3), [4, 0, 7])
    assert rec.shape == (3, 18) and rec.dtype == np.float64 and rec[:, 16].tolist() == [0, 4, 4] and rec[:, 17].tolist() == [4, 0, 7]
    assert rec[2, :4].tolist() == [500, 510, 0, 0] and rec[2, 4:13].tolist() == np.eye(3).reshape(-1).tolist() and rec[2, 13:16].tolist() == [6, 7, 8]
    np.testing.assert_array_equal(rec, R.camera_records(np.tile(np.diag([500.0, 510.0, 1.0]), (3, 1, 1)), np.tile(np.eye(3), (3, 1, 1)),
                                                        np.arange(9.0).reshape(3, 3), [4, 0, 7]))


# ------------------------------------------------------------------------------------------------ the Python layer
def _host_tracks(counts=(3, 2)):
    start = np.concatenate([[0], np.cumsum(counts)]).tolist()
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    stats = dict(n_tracks=1, n_obs=2, n_conflicting=0, n_edges=1, n_bad=0, status=0)
    return gims_amd.Tracks(i32(0, -1, -1, 0, -1), i32(0, 2), i32(0, 1), i32(0, 0), torch.zeros(1, dtype=torch.uint8), stats, start)


def test_value_errors_before_the_device_is_touched():
    tr = _host_tracks()
    images = [torch.zeros(3, 2), torch.zeros(2, 2)]
    K, Rm, t = np.tile(np.diag([500.0, 500.0, 1.0]), (2, 1, 1)), np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3))
    cams = (K, Rm, t)

    def refused(word, tracks=tr, images=images, cameras=cams, **kw):
        with pytest.raises(ValueError, match="triangulate_tracks") as e:
            gims_amd.triangulate_tracks(tracks, images, cameras, **kw)
        assert word in str(e.value), str(e.value)

    refused("1 images are given", images=images[:1])
    refused("image 1: keypoints of shape", images=[images[0], torch.zeros(3, 2)])
    refused("image 0: keypoints of shape", images=[torch.zeros(2, 3), images[1]])
    refused("floating-point", images=[images[0], torch.zeros(2, 2, dtype=torch.int64)])
    refused("floating-point", images=[images[0], [[0.0, 0.0]] * 2])
    refused("cameras must be", cameras=(K, Rm))
    refused("K must be a real array", cameras=(K[:, :2], Rm, t))
    refused("t must be a real array", cameras=(K, Rm, np.zeros((2, 4))))
    refused("R must be a real array", cameras=(K, np.zeros((2, 3, 3), dtype=complex), t))
    refused("3 / 2 / 2 cameras", cameras=(np.tile(K[:1], (3, 1, 1)), Rm, t))
    skew = K.copy()
    skew[1, 0, 1] = 0.1
    refused("skew", cameras=(skew, Rm, t))
    row = K.copy()
    row[0, 2, 2] = 2.0
    refused("last row", cameras=(row, Rm, t))
    for kw in (dict(thresh=0), dict(thresh=float("nan")), dict(thresh="4"), dict(min_angle=-1), dict(min_angle=180.0), dict(max_hyp=-1), dict(max_hyp=65536),
               dict(max_hyp=1.5), dict(max_hyp=True), dict(refine_iters=256), dict(refine_iters=-1)):
        refused(next(iter(kw)), **kw)
    bad = _host_tracks()
    bad.obs_image = bad.obs_image.long()
    refused("tracks.obs_image must be an int32 tensor", tracks=bad)
    refused("no indptr", tracks=object())
    refused("on the GPU")                                                        # everything else is right: the tracks are host tensors
    K2, R2, t2 = gims_amd.cameras_from_pose(torch.eye(3), np.diag([2.0, 2.0, 1.0]), np.eye(3)[[1, 0, 2]], torch.tensor([1.0, 0.0, 0.0]))
    assert K2.shape == (2, 3, 3) and R2.shape == (2, 3, 3) and t2.shape == (2, 3) and K2.dtype == R2.dtype == t2.dtype == np.float64
    assert (R2[0] == np.eye(3)).all() and (t2[0] == 0).all() and (R2[1] == np.eye(3)[[1, 0, 2]]).all() and t2[1].tolist() == [1, 0, 0] and K2[1, 0, 0] == 2


# ------------------------------------------------------------------------------------------------ the restatement on planted scenes
def test_noise_free_tracks_recover_the_planted_points():
    sc = R.planted_tracks(3, [2, 3, 4, 5, 6, 7, 8, 9] * 5, noise=0.0, p_wrong=0.0)
    for max_hyp, refine in ((64, 10), (0, 0), (1, 3)):
        out = R.triangulate(**_pick(sc), max_hyp=max_hyp, refine_iters=refine)
        assert (out["status"] == 0).all() and (out["n_inliers"] == np.diff(sc["indptr"])).all() and out["obs_inlier"].all()
        worst = np.abs(out["xyz"] - sc["points"]).max()
        print(f"noise-free, max_hyp={max_hyp}, refine_iters={refine}: worst error {worst:.3g}")
        assert worst < 2e-6                                                      # float32 pixels: 6e-5 px at f / z = 800 / 3 px per unit, a few views
        assert out["rms_error"].max() < 2e-4 and out["stats"]["n_ok"] == 40 and out["stats"]["n_inlier_obs"] == len(sc["obs_image"])


def test_wrong_observations_are_found():
    out, _ = reference("seams", (64, 10))
    sc = scene("seams")
    assert (out["status"] == 0).all()
    worst = np.abs(out["xyz"] - sc["points"]).max()
    print(f"'seams', max_hyp=64, refine_iters=10: worst error {worst:.3g}")
    assert worst < 0.01                                                          # 0.5 px of noise at 800 / 3 px per unit: 2e-3 per view
    assert not out["obs_inlier"][sc["wrong"]].any() and out["obs_inlier"][~sc["wrong"]].mean() > 0.97
    long_, _ = reference("long", (64, 10))
    assert long_["status"].tolist() == [0, 0, R.TOO_LONG, 0] and long_["stats"]["n_too_long"] == 1
    i = scene("long")["indptr"]
    assert (long_["obs_error"][i[2]:i[3]] == -1).all() and not long_["obs_inlier"][i[2]:i[3]].any() and (long_["xyz"][2] == 0).all()


def test_edge_cases_of_the_restatement():
    hyp, _ = reference("edge", (64, 10))
    flat, _ = reference("edge0", (0, 10))
    sc = scene("edge")
    N, L, S = R.NO_MODEL, R.LOW_ANGLE, R.TOO_SHORT
    assert hyp["status"].tolist() == [0, N, N, 0, N, 0, 0, S] and flat["status"].tolist() == [0, N, N, L, 0, 0, S]
    ptr = sc["indptr"]
    assert hyp["obs_inlier"][ptr[3]:ptr[4]].tolist() == [1, 1, 1, 0] and hyp["obs_error"][ptr[4] - 1] == -1        # behind the camera that looks away
    assert flat["status"][3] == L and np.abs(flat["xyz"][3]).max() > 10 and 0 < flat["max_angle"][3] < MIN_ANGLE   # the point is still written
    assert hyp["n_inliers"][5] == 4 and hyp["obs_inlier"][ptr[6]:ptr[7]].tolist() == [1, 1, 0] and hyp["obs_error"][ptr[7] - 1] == -1
    assert hyp["stats"]["n_bad_obs"] == 2 == flat["stats"]["n_bad_obs"]
    for out, ptr in ((hyp, ptr), (flat, scene("edge0")["indptr"])):
        for t in np.nonzero(out["status"] & ~np.uint8(L))[0]:                                                       # no model: nothing is reported
            assert (out["xyz"][t] == 0).all() and out["n_inliers"][t] == 0 and out["rms_error"][t] == 0 and out["max_angle"][t] == 0
            assert (out["obs_error"][ptr[t]:ptr[t + 1]] == -1).all() and not out["obs_inlier"][ptr[t]:ptr[t + 1]].any()
        assert all(np.isfinite(out[k]).all() for k in ("xyz", "max_angle", "rms_error", "obs_error"))
    poisoned, _ = reference("poison", (64, 10))
    clean, _ = reference("batch", (64, 10))
    assert poisoned["stats"]["n_bad_obs"] == 5 and poisoned["status"][[0, 20, 21]].tolist() == [S, S, S]
    untouched = [t for t in range(40) if t not in (0, 3, 5, 8, 13, 20, 21)]
    np.testing.assert_array_equal(poisoned["xyz"][untouched], clean["xyz"][untouched])


# ------------------------------------------------------------------------------------------------ the fixtures' margins, and TOL_X
@pytest.mark.parametrize("name,combo", CASES)
def test_fixture_margins(name, combo):
    """What makes an exact comparison of status, n_inliers and obs_inlier with the device fair: no decision of the restatement is close."""
    _, tr = reference(name, combo)
    ratio, depth, angle, lead = (np.array(tr.get(k, []), dtype=np.float64) for k in ("e2_over_thresh2", "depths", "angles", "cost_lead"))
    ratio, depth = ratio[np.isfinite(ratio)], depth[np.isfinite(depth)]
    m = dict(thresh=np.abs(ratio - 1).min() if len(ratio) else np.inf, depth=np.abs(depth).min() if len(depth) else np.inf,
             angle=np.abs(angle - MIN_ANGLE).min() if len(angle) else np.inf, lead=lead.min() if len(lead) else np.inf)
    print(name, combo, {k: f"{v:.3g}" for k, v in m.items()})
    assert m["thresh"] > 1e-6 and m["depth"] > 1e-9 and m["angle"] > 1e-6 and m["lead"] > 1e-9, m


def test_tol_x_is_the_measured_one():
    spread = 0.0
    for name, combo in CASES:
        fwd, rev = reference(name, combo)[0], reference(name, combo, "reverse")[0]
        for k in ("status", "n_inliers", "obs_inlier"):
            np.testing.assert_array_equal(fwd[k], rev[k], err_msg=f"{name} {combo} {k}")
        s = float(np.abs(fwd["xyz"] - rev["xyz"]).max()) / EXTENT if len(fwd["xyz"]) else 0.0
        print(name, combo, f"spread {s:.3g}")
        spread = max(spread, s)
    print(f"SPREAD = {spread:.4g}, 16 x SPREAD = {16 * spread:.4g}, TOL_X = {TOL_X:.4g}")
    assert 0.8 * TOL_X <= 16 * spread <= TOL_X
