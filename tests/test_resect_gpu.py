"""GPU tests of the resection op: GIMS_AUX_RESECT_IMAGES (gims_amd/csrc/resect.hip) against the NumPy restatement
(tests/resect_ref.py) on the fixtures of tests/test_resect_cpu.py, which asserts their margins: ok, n_corr, n_inliers, best_hyp,
best_hyp_inliers, lo_rounds, kp_inlier and the counters compare exactly, the floats within the bars below.  (The root of the chosen
hypothesis is no output: two roots of a sample give poses that differ in the first digit, so the bar on the pose compares it.)  The op is
called through a table on a buffer filled with 0xA5; every output must be overwritten, and neither the padding between the regions nor the
256 bytes behind the buffer may change.

Bars.  R and t: TOL_POSE = 2.3e-15 absolute (16 x the restatement's own spread between forward and reverse summation, measured and asserted
in tests/test_resect_cpu.py).  kp_error: float32 storage (2^-23 relative) + 2 |d e / d pose| TOL_POSE, the sensitivity taken from the
restatement per correspondence; rms_error: the same with the largest sensitivity among the entry's correspondences.  The factor 2 is for
the second order.

Shapes.  K = 0, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025 (the waves and the tiles of 256 of the gather and scoring kernels); iters = 1, 15,
16, 17, 300 (GIMS_RESECT_HB = 16 hypotheses a workgroup; 300: more models than one scoring group) and 64; lo_iters 0 and 8; m = 1, 2, 5 with an
image of no keypoints, one whose points `use` masks and one listed twice; track_of entries of -1, T and 2^30, a NaN in xyz and in a keypoint,
a camera record with a NaN.

Noise-free scenes against the planted pose: the restatement's worst error is 4.1e-6 (R) / 1.4e-6 (t) (tests/test_resect_cpu.py), the device
gets ten times that.  End to end ('e2e' of tests/test_triangulate_cpu.py: 8 images x 256 keypoints, 0.5 px noise, 3 % wrong matches; images
0 and 1 posed, 2 .. 7 resected from 82 valid tracks): the restatement's worst error against the planted cameras is 6.7e-3 (R) / 3.1e-2 (t)
(E2E_R / E2E_T, asserted in tests/test_resect_cpu.py), the device gets ten times that; the second triangulation has 219 valid tracks."""
import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import resect_ref as R
from tests.test_resect_cpu import (BATCHES, CASES, E2E, E2E_R, E2E_T, MIN_INLIERS, NOISE_FREE, NOISE_FREE_R, NOISE_FREE_T, SEED, THRESH, TOL_POSE, e2e_host,
                                   entries, noise_free, reference, scene)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FILL, PAD = 0xA5, 256
INTS = ("n_corr", "ok", "n_inliers", "best_hyp", "best_hyp_inliers", "lo_rounds")
EXACT = INTS + ("kp_inlier",)
FLOATS = ("pose", "rms_error", "kp_error")


def _dev(a, shape=None, dtype=None):
    """On the device; an empty array becomes one zero element (the op wants an address and reads nothing through it)."""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(shape, dtype)
    return torch.from_numpy(a).cuda()


def _buffers(sc, cams, iters):
    B = dict(track_of=_dev(sc["track_of"].astype(np.int32), (1,), np.int32), xyz=_dev(sc["xyz"].astype(np.float64), (1, 3), np.float64),
             use=_dev(sc["use"].astype(np.uint8), (1,), np.uint8), kpts=_dev(sc["kpts"].astype(np.float32), (1, 2), np.float32))
    B["cams"] = np.ascontiguousarray(cams, dtype=np.float64)
    B["n"], B["T"], B["iters"] = len(sc["track_of"]), len(sc["use"]), iters
    B["layout"] = hip.resect_out_layout(B["cams"], iters)
    B["out"] = torch.full((B["layout"]["bytes"] + PAD,), FILL, dtype=torch.uint8, device="cuda")
    return B


def _op(B, lo_iters, thresh=THRESH, min_inliers=MIN_INLIERS, seed=SEED):
    return hip.op_resect_images(B["track_of"], B["xyz"], B["use"], B["kpts"], B["cams"], B["out"], B["n"], B["T"], thresh, B["iters"], lo_iters,
                                min_inliers, seed)


def _read(B):
    """The outputs as the restatement returns them.  The padding between the regions and the bytes behind the buffer must be as they were."""
    torch.cuda.synchronize()
    raw, o = B["out"].cpu().numpy(), B["layout"]
    m, S = len(o["slots"]) - 1, o["slots"][-1]
    sizes = dict(pose=96 * m, rms_error=4 * m, kp_inlier=S, kp_error=4 * S, counters=32, **{k: 4 * m for k in INTS})
    assert (raw[o["bytes"]:] == FILL).all()
    got, padding = {}, np.ones(o["outputs"], dtype=bool)
    for name, size in sizes.items():
        got[name] = raw[o[name]:o[name] + size]
        padding[o[name]:o[name] + size] = False
    assert (raw[:o["outputs"]][padding] == FILL).all(), "the padding between the output regions was written"
    out = {k: got[k].view(np.int32) for k in INTS}
    out.update(pose=got["pose"].view(np.float64).reshape(m, 12), rms_error=got["rms_error"].view(np.float32), kp_inlier=got["kp_inlier"],
               kp_error=got["kp_error"].view(np.float32), slots=np.array(o["slots"]))
    counters = got["counters"].view(np.int32)
    assert (counters[4:] == 0).all()
    out["stats"] = dict(zip(hip.RESECT_COUNTERS, (int(v) for v in counters[:4])))
    return out


def run(sc, cams, iters, lo_iters, **kw):
    B = _buffers(sc, cams, iters)
    hip.run_ops(hip.make_ops([_op(B, lo_iters, **kw)]))
    return _read(B)


def same(got, want):
    for k in EXACT:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["stats"] == want["stats"]
    assert all(np.isfinite(got[k]).all() for k in FLOATS)
    dp = np.abs(got["pose"] - want["pose"]).max() if len(want["pose"]) else 0.0
    print(f"pose differs by {dp:.3g}, the bar is {TOL_POSE:.3g}")
    assert dp <= TOL_POSE, f"pose differs by {dp:.3g}, the bar is {TOL_POSE:.3g}"
    store = 2.0 ** -23
    bar = store * np.abs(want["kp_error"]) + 2 * want["kp_sens"] * TOL_POSE
    d = np.abs(got["kp_error"].astype(np.float64) - want["kp_error"])
    assert (d <= bar).all(), f"kp_error: {d.max():.3g} at {int(np.argmax(d - bar))}, bar {bar[int(np.argmax(d - bar))]:.3g}"
    for e in range(len(want["ok"])):
        sens = want["kp_sens"][want["slots"][e]:want["slots"][e + 1]].max(initial=0.0)
        assert abs(float(got["rms_error"][e]) - want["rms_error"][e]) <= store * want["rms_error"][e] + 2 * sens * TOL_POSE, ("rms_error", e)
    no_pose = want["ok"] == 0
    assert (got["pose"][no_pose] == 0).all() and (got["rms_error"][no_pose] == 0).all() and (got["n_inliers"][no_pose] == 0).all()


def entry_bytes(out, e):
    lo, hi = out["slots"][e], out["slots"][e + 1]
    return b"".join([out[k][e].tobytes() for k in INTS + ("pose", "rms_error")] + [out[k][lo:hi].tobytes() for k in ("kp_inlier", "kp_error")])


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("name,m,iters,lo_iters", CASES)
def test_against_the_restatement(name, m, iters, lo_iters):
    got = run(scene(name), entries(name, m), iters, lo_iters)
    want = reference(name, m, iters, lo_iters)
    same(got, want)
    if name == "batch" and m == 5:
        assert got["ok"].tolist() == [1, 0, 0, 1, 1] and got["stats"]["n_failed"] == 2 and entry_bytes(got, 0) == entry_bytes(got, 4)
    if name == "badcam":
        assert got["ok"].tolist() == [0, 1] and got["n_corr"][0] == 0
    if name in ("K0", "K2", "K3"):
        assert got["ok"][0] == 0 and (got["kp_error"] == -1).all() and not got["kp_inlier"].any()


def test_no_entries_and_no_hypotheses():
    sc = scene("K64")
    none = run(sc, np.zeros((0, 6)), 64, 8)
    assert none["stats"] == dict(n_ok=0, n_failed=0, n_corr_total=0, n_inlier_total=0)
    got = run(sc, sc["cams"], 0, 8)                                             # iters == 0: the correspondences are counted, there is no model
    same(got, R.resect(sc["track_of"], sc["xyz"], sc["use"], sc["kpts"], sc["cams"], thresh=THRESH, iters=0, lo_iters=8, min_inliers=MIN_INLIERS, seed=SEED))
    assert got["n_corr"][0] == 64 and got["ok"][0] == 0 and got["best_hyp"][0] == -1


def test_min_inliers_and_threshold():
    sc = scene("K65")
    want = reference("K65", None, 64, 8)
    n = int(want["n_inliers"][0])
    assert run(sc, sc["cams"], 64, 8, min_inliers=n)["ok"][0] == 1
    refused = run(sc, sc["cams"], 64, 8, min_inliers=n + 1)
    assert refused["ok"][0] == 0 and (refused["pose"] == 0).all() and refused["best_hyp"][0] == want["best_hyp"][0] and (refused["kp_error"] == -1).all()


# ------------------------------------------------------------------------------------------------ batch independence
def test_an_entry_is_bit_identical_alone_and_in_a_batch():
    """Image 3 of 'batch' alone, as entry 3 of the batch of five, and the batch run again."""
    sc = scene("batch")
    alone, five = run(sc, entries("batch", 1), 64, 8), run(sc, entries("batch", 5), 64, 8)
    again = run(sc, entries("batch", 5), 64, 8)
    assert BATCHES[1] == [BATCHES[5][3]] and alone["ok"][0] == 1 and alone["lo_rounds"][0] >= 0
    assert entry_bytes(alone, 0) == entry_bytes(five, 3)
    for e in range(5):
        assert entry_bytes(five, e) == entry_bytes(again, e), e
    assert five["stats"] == again["stats"]


# ------------------------------------------------------------------------------------------------ in a table behind build_tracks and triangulate_tracks
def test_op_replays_in_a_table_behind_build_tracks_and_triangulate_tracks():
    """One table: GIMS_AUX_BUILD_TRACKS, GIMS_AUX_TRIANGULATE_TRACKS (images 2 .. 7 hold NaN poses), GIMS_AUX_RESECT_IMAGES reading track_of and
    xyz where the first two ops left them -- no host step between the three.  The same bits as the op alone on the restatements' tracks
    and points, twice, and as a captured graph."""
    from tests import triangulate_ref as TR
    from tests.test_tracks_gpu import SENT, _buffers as trk_buffers, _op as trk_op
    from tests.test_triangulate_gpu import _buffers as tri_buffers, _op as tri_op
    m, tr, first, _, _, _ = e2e_host()
    Rn, tn = m["R"].copy(), m["t"].copy()
    Rn[2:], tn[2:] = np.nan, np.nan
    tri_sc = dict(indptr=tr["indptr"].astype(np.int32), obs_image=tr["obs_image"].astype(np.int32), obs_keypoint=tr["obs_keypoint"].astype(np.int32),
                  kpts=np.concatenate(m["kpts"]), cams=TR.camera_records(m["K"], Rn, tn, m["counts"]))
    T, n_obs = len(tri_sc["indptr"]) - 1, len(tri_sc["obs_image"])
    cams = hip.resect_cameras(m["K"], m["counts"], list(range(2, E2E["n_cams"])))
    use = np.ones(T, np.uint8)                                                   # no host step: every track's point may serve (zeros where there is none)
    res_sc = dict(track_of=tr["track_of"], xyz=first["xyz"], use=use, kpts=tri_sc["kpts"])

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        TB = trk_buffers(m["counts"], m["pairs"], m["matches"], None, None)
        o_ptr, o_img, o_kp, _, _ = hip.tracks_out_layout(TB["n"])
        B = tri_buffers(tri_sc)
        B["indptr"], B["obs_image"], B["obs_keypoint"] = TB["out"][o_ptr:o_ptr + T + 1], TB["out"][o_img:o_img + n_obs], TB["out"][o_kp:o_kp + n_obs]
        RB = _buffers(res_sc, cams, 128)
        RB["track_of"] = TB["track_of"][:TB["n"]]
        RB["xyz"] = B["out"][B["layout"]["xyz"]:B["layout"]["xyz"] + 24 * T].view(torch.float64)
        ops = hip.make_ops([trk_op(TB, None, 2, "drop"), tri_op(B, (64, 10)), _op(RB, 8)])

        def reset():
            for k in ("track_of", "out", "counters", "work"):
                TB[k].fill_(SENT)
            B["out"].fill_(0xA5)
            RB["out"].fill_(FILL)

        reset()
        hip.run_ops(ops, 0, 2)                                                   # the first two ops alone: the resection of THEIR outputs is the expectation
        side.synchronize()
        np.testing.assert_array_equal(RB["track_of"].cpu().numpy(), tr["track_of"])
        alone = run(dict(res_sc, xyz=RB["xyz"].cpu().numpy().reshape(T, 3)), cams, 128, 8)
        assert alone["ok"].sum() >= 4 and np.abs(RB["xyz"].cpu().numpy().reshape(T, 3) - first["xyz"]).max() < 1e-6
        for _ in range(2):
            reset()
            hip.run_ops(ops)
            side.synchronize()
            got = _read(RB)
            for e in range(len(cams)):
                assert entry_bytes(got, e) == entry_bytes(alone, e), e
            assert got["stats"] == alone["stats"]
        graph = hip.OpsGraph(ops)
        reset()
        graph.launch()
        side.synchronize()
        got = _read(RB)
        for e in range(len(cams)):
            assert entry_bytes(got, e) == entry_bytes(alone, e), e
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------------------------------------ against the planted pose
@pytest.mark.parametrize("planar,n", NOISE_FREE)
def test_noise_free_scenes_recover_the_planted_pose(planar, n):
    sc = noise_free(planar, n)
    for lo in (0, 8):
        got = run(sc, sc["cams"], 64, lo, min_inliers=0, seed=3)
        assert got["ok"][0] == 1 and got["n_inliers"][0] == n and got["kp_inlier"].all()
        er, et = R.pose_errors(got["pose"][0], sc["R"], sc["t"])
        print(f"noise-free, planar={planar}, n={n}, lo_iters={lo}: |dR| {er:.3g}, |dt| {et:.3g}")
        assert er <= 10 * NOISE_FREE_R and et <= 10 * NOISE_FREE_T


def test_absolute_pose():
    sc = noise_free(False, 64)
    K = np.array([[sc["cams"][0, 0], 0, sc["cams"][0, 2]], [0, sc["cams"][0, 1], sc["cams"][0, 3]], [0, 0, 1.0]])
    assert gims_amd.absolute_pose(sc["xyz"][:2], sc["kpts"][:2], K) is None
    assert gims_amd.absolute_pose(sc["xyz"][:3], sc["kpts"][:3], K, iters=16) is None      # three points fit their own model: no pose
    Rm, t, mask = gims_amd.absolute_pose(torch.from_numpy(sc["xyz"]).cuda(), sc["kpts"], K, iters=64, seed=3)
    er, et = R.pose_errors(np.concatenate([Rm.cpu().numpy().reshape(9), t.cpu().numpy()]), sc["R"], sc["t"])
    assert Rm.shape == (3, 3) and t.shape == (3,) and mask.dtype == torch.bool and mask.shape == (64,) and bool(mask.all())
    assert er <= 10 * NOISE_FREE_R and et <= 10 * NOISE_FREE_T
    wrong = sc["kpts"].copy()
    wrong[:20] = np.random.default_rng(0).uniform(0, 700, (20, 2))
    Rm, t, mask = gims_amd.absolute_pose(sc["xyz"], wrong, K, iters=256, seed=3)
    assert not mask[:20].any() and mask[20:].all()


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


def test_end_to_end(monkeypatch):
    m, tr, first, want, second, _ = e2e_host()
    n_cams = E2E["n_cams"]
    kpts = [torch.from_numpy(k).cuda() for k in m["kpts"]]
    outs = [{"matches0": torch.from_numpy(x).cuda().reshape(1, -1)} for x in m["matches"]]
    tracks = gims_amd.build_tracks(m["counts"], m["pairs"], outs)
    Rn, tn = m["R"].copy(), m["t"].copy()
    Rn[2:], tn[2:] = np.nan, np.nan                                             # images 2 .. 7 have no pose yet
    pts = gims_amd.triangulate_tracks(tracks, kpts, (m["K"], Rn, tn))
    torch.cuda.synchronize()
    counts = _count_syncs(monkeypatch)
    poses = gims_amd.resect_images(pts, tracks, kpts, m["K"], which=list(range(2, n_cams)), thresh=THRESH, iters=256, lo_iters=8, min_inliers=MIN_INLIERS, seed=SEED)
    assert counts == {"device": 0, "stream": 0, "event": 0, "item": 0}, counts          # no host synchronisation at all
    stats = poses.stats
    assert counts == {"device": 0, "stream": 0, "event": 1, "item": 1}, counts          # .stats: one event, then the pinned words
    monkeypatch.undo()
    assert isinstance(poses, gims_amd.Poses) and len(poses) == n_cams - 2 and poses.image == list(range(2, n_cams)) and poses.R.dtype == torch.float64
    assert poses.R.shape == (n_cams - 2, 3, 3) and poses.t.shape == (n_cams - 2, 3) and poses.ok.dtype == torch.bool
    np.testing.assert_array_equal(poses.n_corr.cpu().numpy(), want["n_corr"])
    assert bool(poses.ok.all()) and stats["n_ok"] == n_cams - 2 and stats["n_corr_total"] == int(want["n_corr"].sum())
    inl, err = poses.of_entry(1)
    assert inl.shape == (m["counts"][3],) and err.shape == (m["counts"][3],) and int(inl.sum()) == int(poses.n_inliers[1])
    Rd, td = poses.R.cpu().numpy(), poses.t.cpu().numpy()
    for e, k in enumerate(poses.image):
        er, et = float(np.abs(Rd[e] - m["R"][k]).max()), float(np.abs(td[e] - m["t"][k]).max())
        print(f"'e2e' image {k}: |dR| {er:.3g}, |dt| {et:.3g} (the restatement's worst: {E2E_R:.3g}, {E2E_T:.3g})")
        assert er <= 10 * E2E_R and et <= 10 * E2E_T
    K2, R2, t2 = poses.cameras(m["K"], Rn, tn)
    assert np.isfinite(R2).all() and np.isfinite(t2).all() and (R2[:2] == m["R"][:2]).all() and np.isnan(Rn[2:]).all()
    again = gims_amd.triangulate_tracks(tracks, kpts, (K2, R2, t2))
    n_first, n_again = int(pts.valid.sum()), int(again.valid.sum())
    print(f"'e2e': valid tracks {n_first} -> {n_again} (the restatement: {int((first['status'] == 0).sum())} -> {int((second['status'] == 0).sum())})")
    assert n_first == int((first["status"] == 0).sum()) and n_again > n_first
