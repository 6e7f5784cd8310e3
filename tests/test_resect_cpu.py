"""CPU tests of the resection op: the ABI constant and the pins a feature must leave alone, the argument checks of
GIMS_AUX_RESECT_IMAGES (they run before any HIP call), the layout of its one buffer, the ValueErrors of gims_amd.resect_images, the NumPy
restatement (tests/resect_ref.py) on planted scenes, and the conditions on the fixtures that tests/test_resect_gpu.py compares exactly with
the device: their margins, and the float bar TOL_POSE.

Worst error of the restatement against the planted pose (arc cameras at distance 4 around a scene of extent 1, focal length 800 px, the
keypoints float32: 6e-5 px of rounding at 1024 px), largest |R - R_planted| / |t - t_planted| over the noise-free scenes, as measured here:
  general scenes of 4 .. 257 points   1.1e-06 / 1.1e-06       purely planar scenes   4.1e-06 / 1.4e-06
  'e2e' (0.5 px noise, 3 % wrong matches; images 2 .. 7 from the 82 valid tracks of images 0 and 1)   6.7e-03 / 3.1e-02
NOISE_FREE_R / NOISE_FREE_T record the larger of each; test_noise_free_scenes_recover_the_planted_pose asserts that they are the measured
ones, and the GPU test allows the device ten times as much.

Margins (test_fixture_margins).  Stage 1 is the same float64 operations in the same order on the device (csrc/resect.hip is compiled
without contraction into fused multiply-adds), so what separates the device from the restatement is the order of the sums of stage 2 and
the last bit of a library function.  INLIER = 1e-6 (relative, in e^2) and DEPTH = 1e-9 are the bounds of tests/test_triangulate_cpu.py;
ROOT = 2^-40 leaves a factor 64 over the 2^-46 by which a change of 64 units in the last place moves a polynomial's value relative to sum
|c_i| |e|^i; STAB = 1e-6 bounds the movement of any model near the best under that change (a word of a pose moving by 1e-6 moves a
reprojection by about 1e-3 px); LEAD = 1e-11: stage 2 compares two costs as float32, and a cost -- a sum of at most 1025 terms, 1e-13 of
rounding -- must be a hundred times that far from a number that rounds to another float32.

TOL_POSE.  Every fixture is solved twice by the restatement, its sums over correspondences taken forward and in reverse; the largest
difference of a word of a pose is the restatement's own sensitivity to summation order, SPREAD.  TOL_POSE = 16 x SPREAD.  Measured here:
SPREAD = 1.39e-16 (on 'K65' with one hypothesis; 1.1e-16 on 'batch', 3e-17 and below on the others: the fixtures take few rounds, and two
orders of the same sums end in the same pose to the last bit or the one before), TOL_POSE = 2.3e-15: a few units in the last place of a
translation word near 4.  test_tol_pose_is_the_measured_one asserts that the number recorded here is the measured one."""
import functools

import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import resect_ref as R
from tests import tracks_ref
from tests import triangulate_ref as TR
from tests.test_triangulate_cpu import E2E

TOL_POSE = 2.3e-15        # 16 x the measured SPREAD, rounded up to two digits; test_tol_pose_is_the_measured_one keeps it honest
NOISE_FREE_R, NOISE_FREE_T = 4.1e-6, 1.4e-6
E2E_R, E2E_T = 6.7e-3, 3.1e-2                        # the restatement's worst error on 'e2e'; test_end_to_end_on_the_host keeps them honest
INLIER, DEPTH, ROOT, STAB, LEAD = 1e-6, 1e-9, 2.0 ** -40, 1e-6, 1e-11
THRESH, MIN_INLIERS, SEED = 4.0, 12, 7
HB = 16
KS = [0, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025]
ITERS = [1, HB - 1, HB, HB + 1, 300]
LO_ITERS = [0, 8]
BATCHES = {1: [3], 2: [0, 3], 5: [0, 1, 2, 3, 0]}                  # m -> the images of 'batch' that are listed
# every fixture the GPU test compares exactly: (scene, which entries, iters, lo_iters)
CASES = ([(f"K{k}", None, 64, 8) for k in KS] + [("K65", None, it, 8) for it in ITERS if it != 64] + [("K257", None, 64, 0), ("K64", None, HB, 0)]
         + [("batch", m, 64, lo) for m in BATCHES for lo in LO_ITERS] + [("badcam", None, 64, 8)])
SCENE_SEED = {"K65": 2, "K256": 2}                                           # a fixture that failed a margin got another seed, not another margin


def k_scene(k, seed=1):
    """One image of k correspondences: 0.5 px of noise; from 16 points on, 20 % wrong matches."""
    sc = R.planted_set(1000 * seed + k, k, noise=0.5, wrong=0.2 if k >= 16 else 0.0)
    return {key: sc[key] for key in ("track_of", "xyz", "use", "kpts", "cams", "K", "R", "t")}


def batch_scene():
    """Four images over 300 points, each a track of its own.  Image 0 (arc camera 1): 120 keypoints; image 1: none; image 2 (camera 5): 90
    keypoints on the points 200 .. 299, which `use` masks; image 3 (camera 6): 100 keypoints, among them every poisoned input: track_of
    entries of -1, T and 2^30, a NaN in the xyz of one track and a NaN keypoint.  0.5 px of noise, 20 % wrong matches, one keypoint in ten
    without a track."""
    rng = np.random.default_rng(21)
    K, Rm, t = TR.arc_cameras(8)
    T = 300
    X = rng.uniform(-0.5, 0.5, (T, 3))
    use = np.ones(T, np.uint8)
    use[200:] = 0
    kpts, track_of, counts = [], [], []
    for cam, n_k, lo, hi in ((1, 120, 0, 200), (0, 0, 0, 200), (5, 90, 200, 300), (6, 100, 0, 200)):
        ids = rng.permutation(np.arange(lo, hi))[:n_k]
        uv = np.array([TR.project(K[cam], Rm[cam], t[cam], X[i]) for i in ids]).reshape(n_k, 2) + 0.5 * rng.standard_normal((n_k, 2))
        bad = rng.random(n_k) < 0.2
        uv[bad] = rng.uniform([0, 0], [1024, 768], (int(bad.sum()), 2))
        ids = np.where(rng.random(n_k) < 0.1, -1, ids)
        kpts.append(uv)
        track_of.append(ids)
        counts.append(n_k)
    kpts, track_of = np.concatenate(kpts).astype(np.float32), np.concatenate(track_of).astype(np.int32)
    first3 = counts[0] + counts[1] + counts[2]
    track_of[first3 + 5], track_of[first3 + 6], track_of[first3 + 7] = -1, T, 2 ** 30
    X[int(track_of[first3 + 8])] = (0.1, np.nan, 0.2)
    kpts[first3 + 9, 0] = np.nan
    cams = hip.resect_cameras(K[[1, 0, 5, 6]], counts)
    return dict(track_of=track_of, xyz=X, use=use, kpts=kpts, cams=cams, K=K[[1, 0, 5, 6]], R=Rm[[1, 0, 5, 6]], t=t[[1, 0, 5, 6]], counts=counts)


@functools.lru_cache(maxsize=None)
def scene(name):
    if name.startswith("K"):
        return k_scene(int(name[1:]), SCENE_SEED.get(name, 1))
    if name == "batch":
        return batch_scene()
    if name == "badcam":                                            # entry 0: a record whose fx is NaN; entry 1: image 3 of 'batch'
        sc = dict(batch_scene())
        rec = sc["cams"][[0, 3]].copy()
        rec[0, 0] = np.nan
        return dict(sc, cams=rec)
    raise KeyError(name)


def entries(name, m):
    sc = scene(name)
    return sc["cams"] if m is None else np.ascontiguousarray(sc["cams"][BATCHES[m]])


@functools.lru_cache(maxsize=None)
def reference(name, m, iters, lo_iters, order="forward"):
    """The restatement on a fixture, computed once and shared (do not write to it)."""
    sc = scene(name)
    return R.resect(sc["track_of"], sc["xyz"], sc["use"], sc["kpts"], entries(name, m), thresh=THRESH, iters=iters, lo_iters=lo_iters,
                    min_inliers=MIN_INLIERS, seed=SEED, order=order)


# ------------------------------------------------------------------------------------------------ pins, argument checks, layout
def test_abi_constant_and_pins():
    assert hip.AUX_RESECT_IMAGES == 11 == hip.ABI.constants["GIMS_AUX_RESECT_IMAGES"]
    # the feature adds no export, no struct and no ABI version
    assert len(hip.EXPORTS) == 90 and len(hip.ABI.structs) == 28 and hip.ABI_VERSION == 5 == hip.load().gims_abi_version()
    assert not any("resect" in name.lower() for name in hip.EXPORTS)
    assert hip.RESECT_CAMERA_WORDS == 6 == R.CAMERA_WORDS and hip.RESECT_HB == HB == R.HB and hip.RESECT_COUNTERS == R.COUNTERS
    for name in ("resect_images", "Poses", "absolute_pose"):
        assert getattr(gims_amd, name) is getattr(gims_amd.resect, name) and name in gims_amd.__all__
    assert {HB - 1, HB, HB + 1} <= set(ITERS) and {63, 64, 65, 255, 256, 257} <= set(KS)       # the seams of the kernels' tiles


def _run(ptrs, ints, floats=(THRESH, 0.0)):
    """Through hip.run_ops, on the null stream (no device is needed: a refused call makes no HIP call)."""
    with hip.on_stream(0):
        hip.run_ops(hip.make_ops([hip.op_aux(hip.AUX_RESECT_IMAGES, ptrs, ints, floats)]))


def test_argument_checks_come_before_any_hip_call():
    """Every GIMS_EINVAL case of the header, with a message naming resect_images; no device pointer is ever dereferenced (cams is a host
    array: it is read)."""
    cams = np.array([[800.0, 800.0, 512.0, 384.0, 0.0, 100.0], [800.0, 800.0, 512.0, 384.0, 100.0, 50.0]])
    p = [0x10000, 0x20000, 0x30000, 0x40000, cams.ctypes.data, 0x60000]      # track_of, xyz, use, kpts, cams (host), out
    good = [2, 900, 400, 64 | (8 << 16) | (12 << 24), 7, 0]                   # m, N, T, iters | lo_iters << 16 | min_inliers << 24, seed, reserved

    def refused(ptrs, ints, word, floats=(THRESH, 0.0)):
        with pytest.raises(hip.GimsHipError, match="resect_images") as e:
            _run(ptrs, ints, floats)
        assert word in str(e.value) and f"({hip.GIMS_EINVAL})" in str(e.value), str(e.value)

    def ints(**kw):
        return [kw.get(k, v) for k, v in zip(["m", "N", "T", "mode", "seed", "form"], good)]

    refused(p, ints(m=-1), "m = -1")
    refused(p, ints(m=(1 << 24) + 1), "2^24")
    for name in ("N", "T"):
        refused(p, ints(**{name: -1}), f"{name} = -1")
        refused(p, ints(**{name: (1 << 30) + 1}), "2^30")
    refused(p, ints(mode=-1), "iters | lo_iters << 16 | min_inliers << 24")
    refused(p, ints(mode=((1 << 30) + 1) << 24), "min_inliers in 0 .. 2^30")
    for kw in (dict(iters=65536), dict(lo_iters=256), dict(min_inliers=2 ** 30 + 1), dict(iters=-1)):   # the binding refuses what would spill into a neighbour
        with pytest.raises(ValueError, match=next(iter(kw))):
            hip.op_resect_images(*p[:4], cams, p[5], 900, 400, **kw)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(p, good, "thresh", floats=(bad, 0.0))
    refused(p, good, "f[1]", floats=(THRESH, 1.0))
    for k in range(5):
        refused(p[:k] + [None] + p[k + 1:], good, "NULL while m = 2")
    refused(p[:5] + [None], good, "output buffer is NULL")
    refused(p[:5] + [None], ints(m=0), "output buffer is NULL")                # m == 0 is checked like any other call
    refused(p[:5] + [p[5] + 8], good, "16-byte aligned")
    for k in (1, 4):
        refused(p[:k] + [p[k] + 4] + p[k + 1:], good, "8-byte aligned")
    for k in (0, 3):
        refused(p[:k] + [p[k] + 2] + p[k + 1:], good, "4-byte aligned")
    for bad in (-1.0, 0.5, float("nan"), float(2 ** 30 + 1)):
        wrong = cams.copy()
        wrong[1, 5] = bad
        refused(p[:4] + [wrong.ctypes.data, p[5]], good, "entry 1: n_k")
    big = np.tile(cams[:1], (3, 1))
    big[:, 5] = 2.0 ** 29
    refused(p[:4] + [big.ctypes.data, p[5]], ints(m=3), "more than 2^30 keypoints")
    refused(p, ints(form=1), "reserved")
    # i[5] would select a later form of the function, so it is read first: whatever the other words hold, this version does not know the call
    refused([None] * 6, [10, 10, 10, 10, 10, 10], "unknown auxiliary function form")
    refused([None] * 6, [-5, -5, -5, -5, -5, 7], "unknown auxiliary function form", floats=(float("nan"), float("nan")))
    with pytest.raises(hip.GimsHipError, match="unknown auxiliary function 12"):     # the table ends at 11
        with hip.on_stream(0):
            hip.run_ops(hip.make_ops([hip.op_aux(12, p, good, (THRESH, 0.0))]))


def test_out_layout():
    al = lambda x: (x + 255) & ~255      # noqa: E731
    order = ["pose", "n_corr", "ok", "n_inliers", "best_hyp", "best_hyp_inliers", "lo_rounds", "rms_error", "kp_inlier", "kp_error", "counters"]
    for counts, iters in (([], 0), ([0], 1), ([7], 64), ([100, 0, 50, 100], 300), ([4096] * 48, 1024)):
        cams = hip.resect_cameras(np.tile(np.diag([500.0, 510.0, 1.0]), (max(len(counts), 1), 1, 1))[:len(counts)], counts)
        m, S = len(counts), sum(counts)
        o = hip.resect_out_layout(cams, iters)
        sizes = [96 * m] + [4 * m] * 7 + [S, 4 * S, 32]
        assert o["pose"] == 0 and all(o[k] % 256 == 0 for k in order) and o["bytes"] % 256 == 0
        for a, b, size in zip(order, order[1:] + ["outputs"], sizes):
            assert o[b] - o[a] == al(size), (a, b)                              # back to back: nothing overlaps, nothing is wasted
        assert o["scratch"] == o["outputs"] and o["bytes"] - o["scratch"] == al(56 * m) + al(48 * S) + al(4 * m * iters)
        assert o["slots"] == np.concatenate([[0], np.cumsum(counts)]).astype(int).tolist()
    o = hip.resect_out_layout(hip.resect_cameras(np.tile(np.eye(3), (4, 1, 1)), [100, 0, 50, 100]), 300)
    assert {k: o[k] for k in ("pose", "n_corr", "rms_error", "kp_inlier", "kp_error", "counters", "outputs", "bytes")} == dict(
        pose=0, n_corr=512, rms_error=2048, kp_inlier=2304, kp_error=2560, counters=3584, outputs=3840, bytes=3840 + 256 + 12032 + 4864)
    rec = hip.resect_cameras(np.tile(np.array([[500.0, 0, 320], [0, 510.0, 240], [0, 0, 1]]), (3, 1, 1)), [4, 0, 7], which=[2, 0, 2])
    assert rec.shape == (3, 6) and rec.dtype == np.float64 and rec.tolist() == [[500, 510, 320, 240, 4, 7], [500, 510, 320, 240, 0, 4], [500, 510, 320, 240, 4, 7]]
    for bad in (-1.0, 0.5, np.nan):
        wrong = rec.copy()
        wrong[0, 5] = bad
        with pytest.raises(ValueError, match="n_k"):
            hip.resect_out_layout(wrong)


# ------------------------------------------------------------------------------------------------ the Python layer
class _Points:
    def __init__(self, T, device="cpu"):
        self.xyz, self.valid = torch.zeros(T, 3, dtype=torch.float64, device=device), torch.ones(T, dtype=torch.bool, device=device)


def _host_tracks(counts=(3, 2)):
    start = np.concatenate([[0], np.cumsum(counts)]).tolist()
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    stats = dict(n_tracks=1, n_obs=2, n_conflicting=0, n_edges=1, n_bad=0, status=0)
    return gims_amd.Tracks(i32(0, -1, -1, 0, -1), i32(0, 2), i32(0, 1), i32(0, 0), torch.zeros(1, dtype=torch.uint8), stats, start)


def test_value_errors_before_the_device_is_touched():
    tr, pts = _host_tracks(), _Points(1)
    images = [torch.zeros(3, 2), torch.zeros(2, 2)]
    K = np.tile(np.diag([500.0, 500.0, 1.0]), (2, 1, 1))

    def refused(word, points=pts, tracks=tr, images=images, intrinsics=K, which=None, **kw):
        with pytest.raises(ValueError, match="resect_images") as e:
            gims_amd.resect_images(points, tracks, images, intrinsics, which, **kw)
        assert word in str(e.value), str(e.value)

    refused("1 images are given", images=images[:1])
    refused("image 1: keypoints of shape", images=[images[0], torch.zeros(3, 2)])
    refused("image 0: keypoints of shape", images=[torch.zeros(2, 3), images[1]])
    refused("floating-point", images=[images[0], torch.zeros(2, 2, dtype=torch.int64)])
    refused("floating-point", images=[images[0], [[0.0, 0.0]] * 2])
    refused("intrinsics must be a real array", intrinsics=K[:, :2])
    refused("intrinsics must be a real array", intrinsics=np.tile(K[:1], (3, 1, 1)))
    refused("intrinsics must be a real array", intrinsics=K.astype(complex))
    skew = K.copy()
    skew[1, 0, 1] = 0.1
    refused("skew", intrinsics=skew)
    row = K[0].copy()
    row[2, 2] = 2.0
    refused("last row", intrinsics=row)
    for which in ([2], [-1], [0, 1.5], [True]):
        refused("which holds", which=which)
    for kw in (dict(thresh=0), dict(thresh=float("nan")), dict(thresh="4"), dict(iters=-1), dict(iters=65536), dict(iters=1.5), dict(iters=True),
               dict(lo_iters=256), dict(lo_iters=-1), dict(min_inliers=-1), dict(min_inliers=2 ** 30 + 1), dict(seed=-1), dict(seed=2 ** 64)):
        refused(next(iter(kw)), **kw)
    bad = _host_tracks()
    bad.track_of = bad.track_of.long()
    refused("tracks.track_of must be an int32 tensor", tracks=bad)
    refused("no track_of", tracks=object())
    refused("no xyz", points=object())
    wrong = _Points(1)
    wrong.xyz = wrong.xyz.float()
    refused("points.xyz must be a float64 tensor", points=wrong)
    refused("use must be a bool or uint8 tensor", use=torch.ones(2, dtype=torch.bool))
    refused("use must be a bool or uint8 tensor", use=torch.ones(1))
    refused("on the GPU")                                                        # everything else is right: the tracks are host tensors
    refused("on the GPU", intrinsics=K[0], which=[1, 1, 0])
    with pytest.raises(ValueError, match="absolute_pose.*points3d must be"):
        gims_amd.absolute_pose(np.zeros((4, 2)), np.zeros((4, 2)), K[0])
    with pytest.raises(ValueError, match="absolute_pose: thresh"):
        gims_amd.absolute_pose(np.zeros((4, 3)), np.zeros((4, 2)), K[0], thresh=-1.0)
    with pytest.raises(ValueError, match="absolute_pose: intrinsics"):
        gims_amd.absolute_pose(np.zeros((4, 3)), np.zeros((4, 2)), np.eye(4))


# ------------------------------------------------------------------------------------------------ the restatement on planted scenes
NOISE_FREE = [(planar, n) for planar in (False, True) for n in (4, 5, 64, 257)]


@functools.lru_cache(maxsize=None)
def noise_free(planar, n):
    return R.planted_set(1 + n, n, planar=planar)


def test_noise_free_scenes_recover_the_planted_pose():
    worst = {False: [0.0, 0.0], True: [0.0, 0.0]}
    for planar, n in NOISE_FREE:
        sc = noise_free(planar, n)
        for lo in LO_ITERS:
            out = R.resect(sc["track_of"], sc["xyz"], sc["use"], sc["kpts"], sc["cams"], thresh=THRESH, iters=64, lo_iters=lo, min_inliers=0, seed=3)
            assert out["ok"][0] == 1 and out["n_inliers"][0] == n and out["kp_inlier"].all() and out["rms_error"][0] < 1e-3
            er, et = R.pose_errors(out["pose"][0], sc["R"], sc["t"])
            print(f"noise-free, planar={planar}, n={n}, lo_iters={lo}: |dR| {er:.3g}, |dt| {et:.3g}")
            worst[planar] = [max(worst[planar][0], er), max(worst[planar][1], et)]
    print("worst:", worst)
    wr, wt = max(w[0] for w in worst.values()), max(w[1] for w in worst.values())
    assert 0.8 * NOISE_FREE_R <= wr <= NOISE_FREE_R and 0.8 * NOISE_FREE_T <= wt <= NOISE_FREE_T, (wr, wt)
    sc = noise_free(False, 64)                                                   # three points fit their own models: not a pose
    three = R.resect(sc["track_of"][:3], sc["xyz"][:3], sc["use"][:3], sc["kpts"][:3], np.array([[800.0, 800.0, 512.0, 384.0, 0.0, 3.0]]), iters=8, min_inliers=0)
    assert three["ok"][0] == 0 and three["best_hyp_inliers"][0] == 3 and (three["pose"] == 0).all() and (three["kp_error"] == -1).all()


def test_wrong_matches_are_found():
    sc = R.planted_set(9, 300, noise=0.5, wrong=0.3)
    out = R.resect(sc["track_of"], sc["xyz"], sc["use"], sc["kpts"], sc["cams"], thresh=THRESH, iters=300, lo_iters=8, seed=3)
    er, et = R.pose_errors(out["pose"][0], sc["R"], sc["t"])
    print(f"0.5 px noise, 30 % wrong: |dR| {er:.3g}, |dt| {et:.3g}, {out['n_inliers'][0]} inliers of {(~sc['wrong']).sum()} good matches")
    assert out["ok"][0] == 1 and er < 0.05 and et < 0.05                        # 0.5 px at 800 px of focal length and a depth of 4, three points
    assert out["kp_inlier"][sc["wrong"]].sum() <= 2 and out["kp_inlier"][~sc["wrong"]].mean() > 0.97
    assert out["stats"] == dict(n_ok=1, n_failed=0, n_corr_total=300, n_inlier_total=int(out["n_inliers"][0]))


def test_edge_cases_of_the_restatement():
    five = reference("batch", 5, 64, 8)
    sc = scene("batch")
    assert five["n_corr"][1] == 0 and five["n_corr"][2] == 0 and five["ok"].tolist() == [1, 0, 0, 1, 1]
    assert five["n_corr"][3] <= 100 - 5 and five["stats"]["n_failed"] == 2      # the poisoned keypoints are no correspondences
    for e in (1, 2):
        assert (five["pose"][e] == 0).all() and five["best_hyp"][e] == -1 and five["rms_error"][e] == 0
        assert (five["kp_error"][five["slots"][e]:five["slots"][e + 1]] == -1).all()
    assert (five["pose"][0] == five["pose"][4]).all() and five["slots"].tolist() == [0, 120, 120, 210, 310, 430]
    first3 = sum(sc["counts"][:3])
    lo = int(five["slots"][3])
    assert (five["kp_error"][lo + 5:lo + 10] == -1).all() and not five["kp_inlier"][lo + 5:lo + 10].any()
    for e in (0, 3):
        er, et = R.pose_errors(five["pose"][e], sc["R"][BATCHES[5][e]], sc["t"][BATCHES[5][e]])
        assert er < 0.05 and et < 0.05, (e, er, et)
    bad = reference("badcam", None, 64, 8)
    assert bad["ok"].tolist() == [0, 1] and bad["n_corr"][0] == 0 and (bad["pose"][1] == five["pose"][3]).all()
    assert all(np.isfinite(five[k]).all() for k in ("pose", "rms_error", "kp_error")) and first3 == 210
    for k in (0, 2, 3):
        small = reference(f"K{k}", None, 64, 8)
        assert small["ok"][0] == 0 and small["n_corr"][0] == k and small["best_hyp"][0] == (0 if k == 3 else -1)


# ------------------------------------------------------------------------------------------------ the fixtures' margins, and TOL_POSE
@pytest.mark.parametrize("name,m,iters,lo_iters", CASES)
def test_fixture_margins(name, m, iters, lo_iters):
    """What makes an exact comparison of the chosen hypothesis and root, the scores, kp_inlier, the counts and lo_rounds with the device
    fair: no decision of the restatement is close."""
    ref = reference(name, m, iters, lo_iters)
    for e, mg in enumerate(ref["margins"]):
        print(name, m, iters, lo_iters, e, {k: f"{v:.3g}" for k, v in mg.items()})
        assert mg["inlier"] > INLIER and mg["depth"] > DEPTH and mg["root"] > ROOT and mg["stab"] < STAB and mg["lead"] > LEAD, (e, mg)


def test_tol_pose_is_the_measured_one():
    spread = 0.0
    for name, m, iters, lo_iters in CASES:
        fwd, rev = reference(name, m, iters, lo_iters), reference(name, m, iters, lo_iters, "reverse")
        for k in ("ok", "n_corr", "n_inliers", "best_hyp", "best_hyp_inliers", "lo_rounds", "root", "kp_inlier"):
            np.testing.assert_array_equal(fwd[k], rev[k], err_msg=f"{name} {m} {iters} {lo_iters} {k}")
        s = float(np.abs(fwd["pose"] - rev["pose"]).max()) if len(fwd["pose"]) else 0.0
        print(name, m, iters, lo_iters, f"spread {s:.3g}")
        spread = max(spread, s)
    print(f"SPREAD = {spread:.4g}, 16 x SPREAD = {16 * spread:.4g}, TOL_POSE = {TOL_POSE:.4g}")
    assert 0.8 * TOL_POSE <= 16 * spread <= TOL_POSE


# ------------------------------------------------------------------------------------------------ end to end, on the host
@functools.lru_cache(maxsize=None)
def e2e_host():
    """The incremental loop on the 'e2e' scene of tests/test_triangulate_cpu.py by the restatements alone: images 0 and 1 are posed, the rest
    hold NaN; triangulate, resect 2 .. 7, triangulate again -> (matches, tracks, first points, poses, second points, cameras)."""
    m = TR.planted_matches(**E2E)
    tr = tracks_ref.build(m["counts"], m["pairs"], m["matches"])
    Rn, tn = m["R"].copy(), m["t"].copy()
    Rn[2:], tn[2:] = np.nan, np.nan
    pick = dict(indptr=tr["indptr"], obs_image=tr["obs_image"], obs_keypoint=tr["obs_keypoint"], kpts=np.concatenate(m["kpts"]))
    first = TR.triangulate(**pick, cams=TR.camera_records(m["K"], Rn, tn, m["counts"]))
    which = list(range(2, E2E["n_cams"]))
    poses = R.resect(tr["track_of"], first["xyz"], (first["status"] == 0).astype(np.uint8), pick["kpts"], hip.resect_cameras(m["K"], m["counts"], which),
                     thresh=THRESH, iters=256, lo_iters=8, min_inliers=MIN_INLIERS, seed=SEED)
    for e, k in enumerate(which):
        if poses["ok"][e]:
            Rn[k], tn[k] = poses["pose"][e, :9].reshape(3, 3), poses["pose"][e, 9:]
    second = TR.triangulate(**pick, cams=TR.camera_records(m["K"], Rn, tn, m["counts"]))
    return m, tr, first, poses, second, (Rn, tn)


def test_end_to_end_on_the_host():
    m, tr, first, poses, second, _ = e2e_host()
    worst_r = worst_t = 0.0
    for e, k in enumerate(range(2, E2E["n_cams"])):
        if poses["ok"][e]:
            er, et = R.pose_errors(poses["pose"][e], m["R"][k], m["t"][k])
            print(f"'e2e' image {k}: {poses['n_corr'][e]} correspondences, {poses['n_inliers'][e]} inliers, |dR| {er:.3g}, |dt| {et:.3g}")
            worst_r, worst_t = max(worst_r, er), max(worst_t, et)
    print(f"'e2e': {int(poses['ok'].sum())} of {len(poses['ok'])} images resected, worst |dR| {worst_r:.3g}, |dt| {worst_t:.3g}; valid tracks "
          f"{int((first['status'] == 0).sum())} -> {int((second['status'] == 0).sum())}")
    assert poses["ok"].all() and (second["status"] == 0).sum() > (first["status"] == 0).sum()
    assert 0.8 * E2E_R <= worst_r <= E2E_R and 0.8 * E2E_T <= worst_t <= E2E_T
