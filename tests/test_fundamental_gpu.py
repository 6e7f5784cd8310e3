"""The fundamental-matrix model of gims_verify_pairs (csrc/verify.hip) and its Python surface on the device, against the NumPy restatement
of tests/fundamental_ref.py.

Index sets, counts, the chosen hypothesis and the number of accepted rounds are compared exactly: tests/test_fundamental_cpu.py asserts
for every fixture that no inlier decision of any scored hypothesis or stage-2 model lies within 1e-6 px^2 of the threshold.

The model is compared entry by entry after the unit-norm and sign rule, within TOL = max(10 * SPREAD, 4 * 2^-24).  SPREAD is the largest
entry difference of the restatement against itself with the inlier sums accumulated in reversed order (the device adds per-wave partial
sums, an order between the two), measured over K in {63, 257, 2049}, both scenes, 500 hypotheses, lo_iters = 8: 6.0e-14, quoted below
rounded up and asserted by tests/test_fundamental_cpu.py.  So the float32 storage of the nine entries (each at most 1 in magnitude: a
rounding of at most 2^-25, taken with a factor of 8) decides the bound: TOL = 2.4e-7.  |det F| of the returned float32 matrix is held to
the same bound: rounding the entries of a rank-2, unit-norm F moves its determinant by at most 2^-24 * ||F|| * ||cof F|| <= 2^-25."""
import numpy as np
import pytest
import torch

from gims_amd import GMatcher, find_fundamental, hip, synth, verify_pairs
from gims_amd.verify import RECORD_FIELDS
from tests import fundamental_ref as R
from tests import verify_ref as RH
from tests.helpers import pair_to_data

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SPREAD = 1e-13
TOL = max(10 * SPREAD, 4 * 2.0 ** -24)
GARBAGE = 0x5B
COL = {k: i for i, k in enumerate(RECORD_FIELDS)}
FUND, HOMO = "fundamental", "homography"


def _items(specs, models, identity=False):
    """specs: (kp0, kp1, matches0, ...) in NumPy; outputs pre-filled with garbage the call has to overwrite in full."""
    items = []
    for spec, model in zip(specs, models):
        kp0, kp1, m0 = spec[:3]
        items.append(dict(kpts0=torch.from_numpy(np.ascontiguousarray(kp0)).cuda(), kpts1=torch.from_numpy(np.ascontiguousarray(kp1)).cuda(),
                          matches0=None if identity else torch.from_numpy(m0).cuda(), model=model,
                          inlier=torch.full((len(kp0),), GARBAGE, dtype=torch.uint8, device="cuda"),
                          record=torch.full((8,), float("nan"), device="cuda"), homography=torch.full((9,), -7.5e8, device="cuda")))
    return items


def _run(specs, models=None, identity=False, **kw):
    models = [FUND] * len(specs) if models is None else models
    items = _items(specs, models, identity)
    keep = hip.verify_pairs(items, **kw)
    torch.cuda.synchronize()
    del keep
    outs = [dict(inlier=it["inlier"].cpu().numpy(), record=it["record"].cpu().numpy(), F=it["homography"].cpu().numpy().reshape(3, 3)) for it in items]
    for spec, model, out in zip(specs, models, outs):
        if model in (FUND, 1):
            _invariants(spec, out, identity)
    return outs


def _invariants(spec, out, identity=False):
    """What holds for every set with the fundamental model, whatever the input."""
    m0, rec, inl, F = spec[2], out["record"], out["inlier"], out["F"]
    matched = np.ones(len(spec[0]), bool) if identity else (m0 > -1) & (m0 < len(spec[1]))
    assert set(np.unique(inl).tolist()) <= {0, 1}
    assert not inl[~matched].any()                                   # the mask is a subset of the matched rows
    assert rec[COL["n_valid"]] == matched.sum() and rec[COL["n_inliers"]] == inl.sum() and rec[7] == 0
    assert rec[COL["ok"]] in (0.0, 1.0) and rec[COL["err_corner"]] == -1
    if rec[COL["ok"]] == 0:
        assert not F.any() and not inl.any() and not rec[2:6].any()
    else:
        assert np.isfinite(F).all() and abs(np.linalg.norm(F.astype(np.float64)) - 1) <= TOL
        assert abs(np.linalg.det(F.astype(np.float64))) <= TOL
        assert F.reshape(9)[np.argmax(np.abs(F.reshape(9)))] > 0       # the sign rule


def _compare(spec, out, v):
    """One set against fundamental_ref.verify."""
    rec = out["record"]
    assert rec[COL["ok"]] == v["ok"] and rec[COL["n_valid"]] == v["n_valid"]
    if not v["ok"]:
        return
    for k in ("best_hyp", "best_hyp_inliers", "n_inliers", "lo_rounds"):
        assert rec[COL[k]] == v[k], (k, rec[COL[k]], v[k])
    np.testing.assert_array_equal(out["inlier"][spec[2] > -1].astype(bool), v["mask"])
    d = float(np.abs(out["F"].astype(np.float64) - v["F"]).max())
    assert d <= TOL, d


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("config", R.CONFIGS)
@pytest.mark.parametrize("iters", R.ITERS)
@pytest.mark.parametrize("K", R.KS)
def test_against_the_restatement(K, iters, config):
    """Planted two-view scenes with 30 % outliers and unmatched rows; K crosses the wave, tile and chunk borders, iters the block of
    hypotheses; lo_iters = 0 is the best hypothesis made rank 2, lo_iters = 8 the guarded local optimisation."""
    spec = R.planted_spec(K, config)
    for lo in R.LO_ITERS:
        (out,) = _run([spec], thresh=R.THRESH, iters=iters, lo_iters=lo, seed=R.seed_of(K, config))
        v = R.fixture_expected(K, config, iters, lo)
        assert v["ok"] == (1 if K >= 8 else 0)
        _compare(spec, out, v)


# ------------------------------------------------------------------------------------------------ degenerate sets, ragged and mixed batches
def _degenerate():
    r = np.random.default_rng(9)
    n = 40
    ident = np.arange(n, dtype=np.int64)
    plane = (r.random((n, 2)) * [800, 600]).astype(np.float32)
    H = synth.make_homography(31, (800, 600)).astype(np.float64)
    w = np.concatenate([plane, np.ones((n, 1), np.float32)], 1).astype(np.float64) @ H.T
    t = np.linspace(0, 1, n)[:, None]
    line0 = (np.array([[50.0, 60.0]]) + t * np.array([[600.0, 400.0]])).astype(np.float32)
    line1 = (np.array([[90.0, 30.0]]) + t * np.array([[500.0, 450.0]])).astype(np.float32)
    one = np.repeat(np.array([[123.0, 45.0]], dtype=np.float32), n, 0)
    return {"coplanar": (plane, (w[:, :2] / w[:, 2:3]).astype(np.float32), ident), "identical": (one, one.copy(), ident),
            "collinear": (line0, line1, ident), "empty": (np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), ident[:0]),
            "seven": (plane[:7].copy(), plane[:7].copy(), ident[:7])}


def test_degenerate_sets_alone_and_in_a_ragged_batch():
    """All points coplanar, identical or collinear, no points, seven points: only the invariants (asserted by _run on every output), and
    every set -- degenerate or not -- byte for byte what a call of its own gives."""
    deg = _degenerate()
    ordinary = [R.planted_spec(K, c) for K, c in ((65, "general"), (257, "xtrans"), (1025, "general"))]
    specs, who = [], []
    for i, name in enumerate(deg):
        specs += [ordinary[i % 3], deg[name]]
        who += [None, name]
    kw = dict(thresh=3.0, iters=100, lo_iters=8, seed=5)
    outs = _run(specs, **kw)
    for spec, name, out in zip(specs, who, outs):
        (alone,) = _run([spec], **kw)
        for k in ("inlier", "record", "F"):
            assert out[k].tobytes() == alone[k].tobytes(), (name, k)
        if name in ("identical", "empty", "seven"):
            assert out["record"][COL["ok"]] == 0, name
        if name is None:
            assert out["record"][COL["ok"]] == 1
    for lo in (0,):
        for name in ("coplanar", "identical", "collinear"):
            _run([deg[name]], thresh=3.0, iters=100, lo_iters=lo, seed=5)


def test_mixed_batch_equals_single_model_calls():
    """Homography and fundamental sets interleaved in one call: every homography set is byte for byte the same set in a homography-only
    call (which carries no `model` key at all, as before the field had a meaning), every fundamental set is its solo run."""
    specs = [RH.planted_spec(257), R.planted_spec(257, "general"), RH.planted_spec(65), R.planted_spec(1025, "xtrans"), R.planted_spec(7, "general"),
             RH.planted_spec(1025), R.planted_spec(64, "xtrans"), RH.planted_spec(3)]
    models = [HOMO, FUND, 0, 1, FUND, HOMO, FUND, HOMO]
    for lo in (0, 8):
        kw = dict(thresh=3.0, iters=200, lo_iters=lo, seed=7)
        outs = _run(specs, models, **kw)
        homs = [s for s, m in zip(specs, models) if m in (HOMO, 0)]
        items = _items(homs, [HOMO] * len(homs))
        for it in items:
            del it["model"]
        keep = hip.verify_pairs(items, **kw)
        torch.cuda.synchronize()
        del keep
        q = 0
        for spec, model, out in zip(specs, models, outs):
            if model in (HOMO, 0):
                it = items[q]
                q += 1
                ref = dict(inlier=it["inlier"].cpu().numpy(), record=it["record"].cpu().numpy(), F=it["homography"].cpu().numpy().reshape(3, 3))
                assert ref["record"][COL["ok"]] == (1 if len(spec[0]) > 10 else 0)
            else:
                (ref,) = _run([spec], **kw)
            for k in ("inlier", "record", "F"):
                assert out[k].tobytes() == ref[k].tobytes(), (model, k)


def test_identity_pairing_equals_explicit_matches():
    """matches0 = NULL is the pairing i <-> i."""
    for K in (9, 257, 1025):
        p0, p1 = R.correspondences(R.planted_spec(K, "general"))
        spec = (p0, p1, np.arange(K, dtype=np.int64))
        kw = dict(thresh=3.0, iters=64, lo_iters=8, seed=3)
        (a,), (b,) = _run([spec], identity=True, **kw), _run([spec], **kw)
        for k in ("inlier", "record", "F"):
            assert a[k].tobytes() == b[k].tobytes(), (K, k)
        assert a["record"][COL["ok"]] == 1


# ------------------------------------------------------------------------------------------------ the Python surface
def test_a_reference_homography_with_the_fundamental_model_is_refused_before_launch():
    spec = R.planted_spec(64, "general")
    items = _items([spec, spec], [HOMO, FUND])
    items[1].update(h_ref=np.eye(3), height=600, width=800)
    with pytest.raises(hip.GimsHipError, match="fundamental"):
        hip.verify_pairs(items, iters=16)
    torch.cuda.synchronize()
    for it in items:                                                   # nothing was enqueued: the garbage is still there
        assert (it["inlier"] == GARBAGE).all() and torch.isnan(it["record"]).all() and (it["homography"] == -7.5e8).all()
    with pytest.raises(hip.GimsHipError, match="model"):
        hip.verify_pairs(_items([spec], ["essential"]), iters=16)
    datas = [dict(keypoints0=torch.from_numpy(spec[0]).cuda()[None], keypoints1=torch.from_numpy(spec[1]).cuda()[None],
                  image0=np.zeros((600, 800, 3), dtype=np.uint8))]
    outs = [dict(matches0=torch.from_numpy(spec[2]).cuda()[None])]
    with pytest.raises(ValueError, match="model"):
        verify_pairs(datas, outs, iters=16, h_refs=[np.eye(3)], model=FUND)
    with pytest.raises(ValueError, match="model"):
        verify_pairs(datas, outs, iters=16, model=[FUND, FUND])


def test_find_fundamental():
    p0, p1 = R.correspondences(R.planted_spec(7, "general"))
    assert find_fundamental(p0, p1) == (None, None)
    K, config = 257, "xtrans"
    p0, p1 = R.correspondences(R.planted_spec(K, config))
    F, mask = find_fundamental(torch.from_numpy(p0).cuda(), p1, thresh=3.0, iters=500, lo_iters=8, seed=R.seed_of(K, config))
    v = R.fixture_expected(K, config, 500, 8)
    assert F.is_cuda and F.shape == (3, 3) and F.dtype == torch.float32 and mask.is_cuda and mask.shape == (K, 1) and mask.dtype == torch.uint8
    np.testing.assert_array_equal(mask.cpu().numpy()[:, 0].astype(bool), v["mask"])
    assert np.abs(F.cpu().numpy().astype(np.float64) - v["F"]).max() <= TOL
    same = np.repeat(p0[:1], 8, 0)
    assert find_fundamental(same, same, iters=64) == (None, None)
    with pytest.raises(ValueError):
        find_fundamental(p0, p1[:-1])


def test_verify_pairs_models_and_a_mixed_list():
    specs = [R.planted_spec(257, "general"), RH.planted_spec(257)]
    datas = [dict(keypoints0=torch.from_numpy(s[0]).cuda()[None], keypoints1=torch.from_numpy(s[1]).cuda()[None]) for s in specs]
    outs = [dict(matches0=torch.from_numpy(s[2]).cuda()[None]) for s in specs]
    kw = dict(thresh=3.0, iters=500, lo_iters=8)
    mixed = verify_pairs(datas, outs, seed=R.seed_of(257, "general"), model=[FUND, HOMO], **kw)
    fund = verify_pairs(datas[:1], outs[:1], seed=R.seed_of(257, "general"), model=FUND, **kw)
    homo = verify_pairs(datas[1:], outs[1:], seed=R.seed_of(257, "general"), **kw)
    torch.cuda.synchronize()
    assert mixed["models"].shape == (2, 3, 3) and mixed["models"].data_ptr() == mixed["homographies"].data_ptr()
    assert torch.equal(mixed["models"][0], fund["models"][0]) and torch.equal(mixed["models"][1], homo["homographies"][0])
    assert torch.equal(mixed["records"][0], fund["records"][0]) and torch.equal(mixed["records"][1], homo["records"][0])
    assert torch.equal(mixed["inlier"][0], fund["inlier"][0]) and torch.equal(mixed["inlier"][1], homo["inlier"][0])
    v = R.fixture_expected(257, "general", 500, 8)
    assert fund["records"][0, COL["n_inliers"]].item() == v["n_inliers"]
    assert np.abs(fund["models"][0].cpu().numpy().astype(np.float64) - v["F"]).max() <= TOL


def _model():
    m = GMatcher({"sinkhorn_iterations": 20, "match_threshold": 0.02}).eval()
    m.load_state_dict(synth.make_state_dict(123))
    m(pair_to_data(synth.make_pair(256, 1002), 15, 2, 7, device="cuda"))      # settle attention_precision='auto' before calls are compared
    return m


SWEEP_GRID = [(15, 2, 7), (25, 7, 8), (10, 0, 300)]        # the last keeps nothing: no component of 256 keypoints has 300 members
VERIFY = dict(thresh=3.0, iters=500, lo_iters=8, seed=11, model=FUND)


def test_sweep_with_the_fundamental_model():
    m = _model()
    data = pair_to_data(synth.make_pair(256, 1002), 25, 7, 8, device="cuda")
    recs = m.sweep(data, SWEEP_GRID, outputs="all", verify=VERIFY)
    assert [r["error"] is None for r in recs] == [True, True, False]
    for r in recs:
        assert "fundamental" in r and "homography" not in r and {"correct_matches", "inlier"} <= set(r)
    assert recs[2]["correct_matches"] == 0 and recs[2]["fundamental"] is None and recs[2]["inlier"] is None
    live = [r for r in recs if r["error"] is None]
    ref = verify_pairs([r["result"] for r in live], [r["result"] for r in live], **VERIFY)
    torch.cuda.synchronize()
    for q, rec in enumerate(live):
        assert rec["correct_matches"].item() == ref["records"][q, COL["n_inliers"]].item() == rec["inlier"].sum().item()
        assert torch.equal(rec["fundamental"], ref["models"][q]) and torch.equal(rec["inlier"], ref["inlier"][q])
        assert rec["inlier"].shape == (rec["kept0"],) and rec["correct_matches"].item() <= rec["n_matches"].item()
    with pytest.raises(ValueError, match="model"):
        m.sweep(data, SWEEP_GRID, verify=dict(model="essential"))
    with pytest.raises(ValueError, match="model"):
        m.sweep(data, SWEEP_GRID, verify=dict(modle=FUND))
