"""The calibrated relative-pose model of gims_verify_pairs (csrc/verify.hip, model 3) and its Python surface on the device, against the
NumPy restatement of tests/pose_ref.py.

The chosen hypothesis, its model index, the score, the mask, the inlier count, the accepted rounds and n_front are compared exactly:
tests/test_pose_cpu.py asserts for every fixture that no inlier decision of any scored model or stage-2 model lies within 1e-6 px^2 of
the threshold, that no vote lies within 1e-6 of a zero depth, that the best score and the best vote lead by two (K > 6), and that no
polynomial of a hypothesis within two of the best score is about to gain or lose a real root.

E, R and t are compared entry by entry within the float32 storage bound of tests/test_fundamental_gpu.py, TOL = 4 * 2^-24 = 2.4e-7 (every
entry is at most 1 in magnitude).

Noise-free scenes against the planted pose: the restatement's own errors on the four scenes, points rounded to float32 as the kernel
reads them, 64 points, seed 3, 20 hypotheses, thresh 1 px, over lo_iters in {0, 8} (measured by tests/test_pose_cpu.py, which asserts
them), in degrees:
    general    rotation 8.6e-06  translation 4.9e-05
    forward    rotation 1.4e-05  translation 1.2e-04
    sideways   rotation 3.2e-05  translation 5.1e-05
    plane7of8  rotation 2.9e-05  translation 3.5e-04
(the larger of the two lo_iters: that is lo_iters = 0, the model of one minimal sample; with lo_iters = 8 every figure is below 4.8e-05.)
The bar is ten times the largest, CLEAN_BAR = 3.5e-3 degrees: that covers the float32 storage of R and t and fused multiply-adds; a
wrong twisted pair or a wrong root is off by degrees."""
import numpy as np
import pytest
import torch

from gims_amd import GMatcher, estimate_pose, hip, pose_error, pose_summary, synth, verify_pairs
from gims_amd.verify import RECORD_FIELDS
from tests import fundamental_ref as RF
from tests import pose_ref as R
from tests import verify_ref as RH
from tests.helpers import pair_to_data

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = 4 * 2.0 ** -24
CLEAN_WORST = 3.5e-4                # degrees: the largest error of the restatement in the table above
CLEAN_BAR = 10 * CLEAN_WORST
GARBAGE = 0x5B
COL = {k: i for i, k in enumerate(RECORD_FIELDS)}
POSE, FUND, HOMO = "pose", "fundamental", "homography"


def _cams(intr):
    i = [float(v) for v in intr]
    return (np.array([[i[0], 0, i[2]], [0, i[1], i[3]], [0, 0, 1.0]]), np.array([[i[4], 0, i[6]], [0, i[5], i[7]], [0, 0, 1.0]]))


def _items(specs, models, identity=False):
    """specs: (kp0, kp1, matches0, intr or other) in NumPy; outputs pre-filled with garbage the call has to overwrite in full."""
    items = []
    for spec, model in zip(specs, models):
        kp0, kp1, m0 = spec[:3]
        pose = model in (POSE, 3)
        it = dict(kpts0=torch.from_numpy(np.ascontiguousarray(kp0)).cuda(), kpts1=torch.from_numpy(np.ascontiguousarray(kp1)).cuda(),
                  matches0=None if identity else torch.from_numpy(m0).cuda(), model=model,
                  inlier=torch.full((len(kp0),), GARBAGE, dtype=torch.uint8, device="cuda"),
                  record=torch.full((8,), float("nan"), device="cuda"), homography=torch.full((24 if pose else 9,), -7.5e8, device="cuda"))
        if pose:
            it["intrinsics"] = _cams(spec[3])
        items.append(it)
    return items


def _run(specs, models=None, identity=False, **kw):
    models = [POSE] * len(specs) if models is None else models
    items = _items(specs, models, identity)
    keep = hip.verify_pairs(items, **kw)
    torch.cuda.synchronize()
    del keep
    outs = [dict(inlier=it["inlier"].cpu().numpy(), record=it["record"].cpu().numpy(), out=it["homography"].cpu().numpy()) for it in items]
    for spec, model, out in zip(specs, models, outs):
        if model in (POSE, 3):
            _invariants(spec, out, identity)
    return outs


def _invariants(spec, out, identity=False):
    """What holds for every set with the pose model, whatever the input."""
    m0, rec, inl, o = spec[2], out["record"], out["inlier"], out["out"].astype(np.float64)
    E, Rm, t = o[:9].reshape(3, 3), o[9:18].reshape(3, 3), o[18:21]
    matched = np.ones(len(spec[0]), bool) if identity else (m0 > -1) & (m0 < len(spec[1]))
    assert set(np.unique(inl).tolist()) <= {0, 1}
    assert not inl[~matched].any()
    assert rec[COL["n_valid"]] == matched.sum() and rec[COL["n_inliers"]] == inl.sum() and rec[7] == 0
    assert rec[COL["ok"]] in (0.0, 1.0) and rec[COL["err_corner"]] == -1
    assert np.isfinite(o).all() and o[23] == 0
    if rec[COL["ok"]] == 0:
        assert not o.any() and not inl.any() and not rec[2:6].any()
        return
    # the sign rule is applied in float64: an entry as large as the largest one to float32 rounding is positive (the E of a pure
    # translation has its two largest entries equal and opposite)
    assert abs(np.linalg.norm(E) - 1) <= TOL and E.max() >= np.abs(E).max() * (1 - 2.0 ** -22)
    assert 0 <= o[22] < 10 and 0 <= o[21] <= inl.sum()
    if Rm.any():                                                       # a pose: a rotation, a unit translation, E = [t]x R up to sign and scale
        assert np.abs(Rm.T @ Rm - np.eye(3)).max() <= 4 * TOL and abs(np.linalg.det(Rm) - 1) <= 4 * TOL and abs(np.linalg.norm(t) - 1) <= 2 * TOL
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        Ep = tx @ Rm / np.sqrt(2.0)
        s = np.linalg.svd(E, compute_uv=False)
        if s[1] > 0.5 and s[2] < 1e-3:                                 # (a degenerate set may return an E far from the manifold)
            assert min(np.abs(Ep - E).max(), np.abs(Ep + E).max()) <= 1e-5
    else:
        assert not t.any() and o[21] == 0


def _compare(spec, out, v):
    """One set against pose_ref.verify."""
    rec, o = out["record"], out["out"].astype(np.float64)
    assert rec[COL["ok"]] == v["ok"] and rec[COL["n_valid"]] == v["n_valid"]
    if not v["ok"]:
        return
    for k in ("best_hyp", "best_hyp_inliers", "n_inliers", "lo_rounds"):
        assert rec[COL[k]] == v[k], (k, rec[COL[k]], v[k])
    assert o[22] == v["root"] and o[21] == v["n_front"], (o[21:23], v["root"], v["n_front"])
    np.testing.assert_array_equal(out["inlier"][spec[2] > -1].astype(bool), v["mask"])
    for got, want in ((o[:9], v["E"].reshape(9)), (o[9:18], v["R"].reshape(9)), (o[18:21], v["t"])):
        d = float(np.abs(got - want).max())
        assert d <= TOL, d


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("config", R.CONFIGS)
@pytest.mark.parametrize("iters", R.ITERS)
@pytest.mark.parametrize("K", R.KS)
def test_against_the_restatement(K, iters, config):
    """Planted calibrated two-view scenes with 0.5 px noise, 30 % outliers and unmatched rows; K crosses the wave, tile and chunk
    borders, iters the block of hypotheses; lo_iters = 0 is the projected best model, lo_iters = 8 the guarded local optimisation."""
    spec = R.planted_spec(K, config)
    for lo in R.LO_ITERS:
        (out,) = _run([spec], thresh=R.THRESH, iters=iters, lo_iters=lo, seed=R.seed_of(K, config))
        v = R.fixture_expected(K, config, iters, lo)
        assert v["ok"] == (1 if K >= 5 else 0)
        _compare(spec, out, v)


@pytest.mark.parametrize("config", R.CONFIGS)
def test_noise_free_scenes_recover_the_planted_pose(config):
    a, b, _ = R.clean_pairs(config, 64)
    spec = (a, b, np.arange(64, dtype=np.int64), R.intr8(*R.cameras(config)[:2]))
    for lo in R.LO_ITERS:
        (out,) = _run([spec], thresh=R.THRESH, iters=20, lo_iters=lo, seed=3)
        o = out["out"].astype(np.float64)
        assert out["record"][COL["ok"]] == 1 and out["record"][COL["n_inliers"]] == 64 and o[21] == 64
        err_r, err_t = R.pose_errors(R.T_0to1(config), o[9:18].reshape(3, 3), o[18:21])
        print(config, lo, "rotation", err_r, "translation", err_t)
        assert err_r <= CLEAN_BAR and err_t <= CLEAN_BAR, (config, lo, err_r, err_t)


# ------------------------------------------------------------------------------------------------ degenerate sets, ragged and mixed batches
def _degenerate():
    r = np.random.default_rng(9)
    n = 40
    ident = np.arange(n, dtype=np.int64)
    intr = R.intr8(*R.cameras("general")[:2])
    t = np.linspace(0, 1, n)[:, None]
    line0 = (np.array([[50.0, 60.0]]) + t * np.array([[600.0, 400.0]])).astype(np.float32)
    line1 = (np.array([[90.0, 30.0]]) + t * np.array([[500.0, 450.0]])).astype(np.float32)
    one = np.repeat(np.array([[123.0, 45.0]], dtype=np.float32), n, 0)
    pa, pb, _ = R.clean_pairs("planar", n)
    K0, K1 = R.cameras("general")[:2]
    pix = r.random((n, 2)) * [800, 600]
    d = np.concatenate([(pix - K0[:2, 2]) / [K0[0, 0], K0[1, 1]], np.ones((n, 1))], 1)
    q = (d @ R.cameras("general")[2].T) @ K1.T                          # a pure rotation: no translation, no E
    rot = (q[:, :2] / q[:, 2:3]).astype(np.float32)
    return {"four": (pa[:4].copy(), pb[:4].copy(), ident[:4], intr), "identical": (one, one.copy(), ident, intr),
            "collinear": (line0, line1, ident, intr), "rotation": (pix.astype(np.float32), rot, ident, intr),
            "planar": (pa, pb, ident, R.intr8(*R.cameras("planar")[:2])), "empty": (np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), ident[:0], intr)}


def test_degenerate_sets_alone_and_in_a_ragged_batch():
    """Fewer than five points, identical or collinear points, a pure rotation, a purely planar scene: finite outputs or ok = 0 (the
    invariants, asserted by _run on every output), and every set byte for byte what a call of its own gives."""
    deg = _degenerate()
    ordinary = [R.planted_spec(K, c) for K, c in ((65, "general"), (257, "sideways"), (1025, "plane7of8"))]
    specs, who = [], []
    for i, name in enumerate(deg):
        specs += [ordinary[i % 3], deg[name]]
        who += [None, name]
    kw = dict(thresh=1.0, iters=100, lo_iters=8, seed=5)
    outs = _run(specs, **kw)
    for spec, name, out in zip(specs, who, outs):
        (alone,) = _run([spec], **kw)
        for k in ("inlier", "record", "out"):
            assert out[k].tobytes() == alone[k].tobytes(), (name, k)
        if name in ("four", "empty"):
            assert out["record"][COL["ok"]] == 0, name
        if name is None:
            assert out["record"][COL["ok"]] == 1
        if name == "planar":                                            # the five-point model stays determined on a plane
            assert out["record"][COL["ok"]] == 1 and out["record"][COL["n_inliers"]] == 40
    for name in ("identical", "collinear", "rotation", "planar"):
        _run([deg[name]], thresh=1.0, iters=100, lo_iters=0, seed=5)


def test_mixed_batch_equals_single_model_calls():
    """Homography, fundamental and pose sets interleaved in one call: every homography set is byte for byte the same set in a
    homography-only call (which carries no `model` key at all), every fundamental set the same set in a fundamental-only call, every
    pose set its solo run."""
    specs = [RH.planted_spec(257), R.planted_spec(257, "general"), RF.planted_spec(65, "general"), R.planted_spec(1025, "forward"), R.planted_spec(4, "general"),
             RH.planted_spec(1025), RF.planted_spec(257, "xtrans"), R.planted_spec(64, "sideways"), RH.planted_spec(3)]
    models = [HOMO, POSE, FUND, 3, POSE, 0, 1, POSE, HOMO]
    for lo in (0, 8):
        kw = dict(thresh=3.0, iters=200, lo_iters=lo, seed=7)
        outs = _run(specs, models, **kw)
        for kinds in ((HOMO, 0), (FUND, 1)):
            own = [s for s, m in zip(specs, models) if m in kinds]
            items = _items(own, [kinds[0]] * len(own))
            if kinds[0] == HOMO:
                for it in items:
                    del it["model"]
            keep = hip.verify_pairs(items, **kw)
            torch.cuda.synchronize()
            del keep
            q = 0
            for spec, model, out in zip(specs, models, outs):
                if model in kinds:
                    it = items[q]
                    q += 1
                    assert out["inlier"].tobytes() == it["inlier"].cpu().numpy().tobytes() and out["record"].tobytes() == it["record"].cpu().numpy().tobytes()
                    assert out["out"].tobytes() == it["homography"].cpu().numpy().tobytes(), model
                    assert out["record"][COL["ok"]] == (1 if len(spec[0]) > 10 else 0)
        for spec, model, out in zip(specs, models, outs):
            if model in (POSE, 3):
                (ref,) = _run([spec], **kw)
                for k in ("inlier", "record", "out"):
                    assert out[k].tobytes() == ref[k].tobytes(), (model, k)
                assert out["record"][COL["ok"]] == (1 if len(spec[0]) > 10 else 0)


def test_identity_pairing_equals_explicit_matches():
    for K in (6, 257):
        p0, p1 = R.correspondences(R.planted_spec(K, "general"))
        spec = (p0, p1, np.arange(K, dtype=np.int64), R.planted_spec(K, "general")[3])
        kw = dict(thresh=1.0, iters=64, lo_iters=8, seed=3)
        (a,), (b,) = _run([spec], identity=True, **kw), _run([spec], **kw)
        for k in ("inlier", "record", "out"):
            assert a[k].tobytes() == b[k].tobytes(), (K, k)
        assert a["record"][COL["ok"]] == 1


# ------------------------------------------------------------------------------------------------ arguments
def test_bad_pose_arguments_are_refused_before_launch():
    spec = R.planted_spec(64, "general")
    K0, K1 = _cams(spec[3])

    def refused(match, exc=hip.GimsHipError, **change):
        items = _items([spec, spec], [HOMO, POSE])
        items[1].update(change)
        with pytest.raises(exc, match=match):
            hip.verify_pairs(items, iters=16)
        torch.cuda.synchronize()
        for it in items:                                               # nothing was enqueued: the garbage is still there
            assert (it["inlier"] == GARBAGE).all() and torch.isnan(it["record"]).all() and (it["homography"] == -7.5e8).all()

    for bad in (0.0, -600.0, float("nan"), float("inf")):
        for which, r in ((0, 0), (0, 1), (1, 0), (1, 1)):
            Kb = [K0.copy(), K1.copy()]
            Kb[which][r, r] = bad
            refused("pose", intrinsics=tuple(Kb))
    refused("pose", h_ref=np.eye(3), height=600, width=800)
    refused("pose", intrinsics=None)
    refused("24", homography=torch.full((9,), -7.5e8, device="cuda"))
    items = _items([spec], [HOMO])
    items[0]["intrinsics"] = (K0, K1)
    with pytest.raises(hip.GimsHipError, match="pose"):
        hip.verify_pairs(items, iters=16)
    for bad in ("essential", 2):                                       # 2 stays free: no model is derived from F (include/gims_hip.h)
        with pytest.raises(hip.GimsHipError, match="model"):
            hip.verify_pairs(_items([spec], [bad]), iters=16)
    # the library's own check, past the Python layer: a raw set with model 2, and a pose set with has_ref or h_ref[8]
    it = _items([spec], [POSE])[0]
    for model, has_ref, h8 in ((2, 0, 0.0), (3, 1, 0.0), (3, 0, 1.0)):
        h = list(map(float, spec[3])) + [h8]
        arr = (hip.VerifySet * 1)(hip.VerifySet(hip._p(it["kpts0"]), hip._p(it["kpts1"]), hip._p(it["matches0"]), len(spec[0]), len(spec[1]), 0, 0, has_ref,
                                                model, (hip.C.c_float * 9)(*h), hip._p(it["inlier"]), hip._p(it["record"]), hip._p(it["homography"])))
        lib = hip.load()
        work = torch.empty(int(lib.gims_verify_workspace_bytes(arr, 1, 16)), dtype=torch.uint8, device="cuda")
        assert lib.gims_verify_pairs(arr, 1, 1.0, 16, 8, 0, hip._p(work), work.numel(), hip._stream()) == hip._K["GIMS_EINVAL"]
    torch.cuda.synchronize()
    assert torch.isnan(it["record"]).all()


# ------------------------------------------------------------------------------------------------ the Python surface
def test_estimate_pose_pose_error_and_summary():
    K, config = 257, "general"
    spec = R.planted_spec(K, config)
    p0, p1 = R.correspondences(spec)
    K0, K1 = _cams(spec[3])
    assert estimate_pose(p0[:4], p1[:4], K0, K1) is None
    same = np.repeat(p0[:1], 8, 0)
    assert estimate_pose(same, same, K0, K1, iters=64) is None
    with pytest.raises(ValueError):
        estimate_pose(p0, p1[:-1], K0, K1)
    Rm, t, mask = estimate_pose(torch.from_numpy(p0).cuda(), p1, K0, K1, thresh=R.THRESH, iters=500, lo_iters=8, seed=R.seed_of(K, config))
    v = R.fixture_expected(K, config, 500, 8)
    assert Rm.is_cuda and Rm.shape == (3, 3) and t.shape == (3,) and mask.shape == (K,) and mask.dtype == torch.bool
    np.testing.assert_array_equal(mask.cpu().numpy(), v["mask"])
    assert np.abs(Rm.cpu().numpy().astype(np.float64) - v["R"]).max() <= TOL and np.abs(t.cpu().numpy().astype(np.float64) - v["t"]).max() <= TOL
    T = R.T_0to1(config)
    err_t, err_r = pose_error(T, Rm, t)
    want_r, want_t = R.pose_errors(T, Rm.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64))
    assert err_t.dtype == torch.float64 and abs(err_r.item() - want_r) <= 1e-9 and abs(err_t.item() - want_t) <= 1e-9
    assert err_r.item() < 1.0 and err_t.item() < 5.0                   # 0.5 px of noise, 30 % outliers: a pose, not a twisted pair
    # batched, and the summary: one pair posed, one without a pose
    et, er = pose_error(np.stack([T, T]), torch.stack([Rm, torch.zeros_like(Rm)]), torch.stack([t, torch.zeros_like(t)]))
    assert et.shape == (2,) and et[0].item() == err_t.item() and et[1].item() == 90.0
    s = pose_summary([(err_t.item(), err_r.item()), None], thresholds=(5, 10, 20))
    assert s["n_pairs"] == 2 and s["n_posed"] == 1 and all(40.0 < a <= 50.0 for a in s["auc"])


def test_verify_pairs_pose_and_a_mixed_list():
    specs = [R.planted_spec(257, "general"), RH.planted_spec(257), R.planted_spec(65, "forward")]
    datas = [dict(keypoints0=torch.from_numpy(s[0]).cuda()[None], keypoints1=torch.from_numpy(s[1]).cuda()[None]) for s in specs]
    outs = [dict(matches0=torch.from_numpy(s[2]).cuda()[None]) for s in specs]
    cams = [_cams(specs[0][3]), None, _cams(specs[2][3])]
    kw = dict(thresh=1.0, iters=500, lo_iters=8, seed=R.seed_of(257, "general"))
    mixed = verify_pairs(datas, outs, model=[POSE, HOMO, POSE], intrinsics=cams, **kw)
    solo = verify_pairs(datas[:1], outs[:1], model=POSE, intrinsics=cams[0], **kw)
    homo = verify_pairs(datas[1:2], outs[1:2], **kw)
    torch.cuda.synchronize()
    assert set(homo) == {"records", "homographies", "models", "inlier", "_keep"} and homo["homographies"].shape == (1, 3, 3)
    assert homo["homographies"].is_contiguous() and homo["homographies"].untyped_storage().nbytes() == 36
    assert mixed["models"].shape == (3, 3, 3) and mixed["R"].shape == (3, 3, 3) and mixed["t"].shape == (3, 3) and mixed["n_front"].shape == (3,)
    assert torch.equal(mixed["models"][0], solo["models"][0]) and torch.equal(mixed["R"][0], solo["R"][0]) and torch.equal(mixed["t"][0], solo["t"][0])
    assert torch.equal(mixed["models"][1], homo["homographies"][0]) and torch.equal(mixed["records"][1], homo["records"][0])
    assert not mixed["R"][1].any() and not mixed["t"][1].any() and mixed["n_front"][1] == 0
    v = R.fixture_expected(257, "general", 500, 8)
    assert solo["records"][0, COL["n_inliers"]].item() == v["n_inliers"] and solo["n_front"][0].item() == v["n_front"]
    assert np.abs(solo["models"][0].cpu().numpy().astype(np.float64) - v["E"]).max() <= TOL
    assert np.abs(solo["R"][0].cpu().numpy().astype(np.float64) - v["R"]).max() <= TOL
    with pytest.raises(ValueError, match="intrinsics"):
        verify_pairs(datas[:1], outs[:1], model=POSE, **kw)
    with pytest.raises(ValueError, match="intrinsics"):
        verify_pairs(datas[1:2], outs[1:2], intrinsics=cams[0], **kw)
    with pytest.raises(ValueError, match="model"):
        verify_pairs(datas[:1], outs[:1], model=POSE, intrinsics=cams[0], h_refs=[np.eye(3)], **kw)


def test_sweep_with_the_pose_model():
    m = GMatcher({"sinkhorn_iterations": 20, "match_threshold": 0.02}).eval()
    m.load_state_dict(synth.make_state_dict(123))
    m(pair_to_data(synth.make_pair(256, 1002), 15, 2, 7, device="cuda"))
    data = pair_to_data(synth.make_pair(256, 1002), 25, 7, 8, device="cuda")
    grid = [(15, 2, 7), (25, 7, 8), (10, 0, 300)]
    cams = _cams(R.intr8(*R.cameras("general")[:2]))
    vk = dict(thresh=1.0, iters=500, lo_iters=8, seed=11, model=POSE, intrinsics=cams)
    recs = m.sweep(data, grid, outputs="all", verify=vk)
    assert [r["error"] is None for r in recs] == [True, True, False]
    for r in recs:
        assert {"essential", "R", "t", "correct_matches", "inlier"} <= set(r) and "homography" not in r and "fundamental" not in r
    assert recs[2]["correct_matches"] == 0 and recs[2]["essential"] is None and recs[2]["R"] is None and recs[2]["t"] is None
    live = [r for r in recs if r["error"] is None]
    ref = verify_pairs([r["result"] for r in live], [r["result"] for r in live], **vk)
    torch.cuda.synchronize()
    for q, rec in enumerate(live):
        assert rec["correct_matches"].item() == ref["records"][q, COL["n_inliers"]].item() == rec["inlier"].sum().item()
        assert torch.equal(rec["essential"], ref["models"][q]) and torch.equal(rec["R"], ref["R"][q]) and torch.equal(rec["t"], ref["t"][q])
        assert rec["R"].shape == (3, 3) and rec["t"].shape == (3,)
    with pytest.raises(ValueError, match="intrinsics"):
        m.sweep(data, grid, verify=dict(model=POSE))
    with pytest.raises(ValueError, match="intrinsics"):
        m.sweep(data, grid, verify=dict(model=FUND, intrinsics=cams))
