"""gims_verify_pairs (csrc/verify.hip) and its Python surface on the device, against the NumPy restatement of tests/verify_ref.py.

Index sets, counts, the chosen hypothesis and the number of accepted rounds are compared exactly: tests/test_verify_cpu.py asserts for
every fixture that no decision lies within 1e-6 px^2 of the threshold and that no competing count is one flipped decision away.

Homographies are compared by TRANSFER: the largest ||H_gpu x - H_ref x|| over the four image corners and all correspondences, bound
1e-3 px.  Derived, not measured: the float32 rounding of the nine returned entries moves a point of an 800 x 600 image by about 2e-4 px
while |w - 1| <= 0.5, the float64 solve adds about 1e-9 px; that leaves a factor of 5."""
import numpy as np
import pytest
import torch

from gims_amd import GMatcher, evalh, find_homography, hip, synth, verify_pairs
from gims_amd.verify import RECORD_FIELDS
from oracle import eval_oracle as E
from tests import eval_cases as C
from tests import verify_ref as R
from tests.helpers import pair_to_data
from tests.test_verify_cpu import ANCHORS, anchor_spec

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TRANSFER = 1e-3          # px
GARBAGE = 0x5B
COL = {k: i for i, k in enumerate(RECORD_FIELDS)}


def _items(specs, identity=False):
    """specs: (kp0, kp1, matches0, ...) in NumPy; outputs pre-filled with garbage the call has to overwrite in full."""
    items = []
    for spec in specs:
        kp0, kp1, m0 = spec[:3]
        items.append(dict(kpts0=torch.from_numpy(np.ascontiguousarray(kp0)).cuda(), kpts1=torch.from_numpy(np.ascontiguousarray(kp1)).cuda(),
                          matches0=None if identity else torch.from_numpy(m0).cuda(),
                          inlier=torch.full((len(kp0),), GARBAGE, dtype=torch.uint8, device="cuda"),
                          record=torch.full((8,), float("nan"), device="cuda"), homography=torch.full((9,), -7.5e8, device="cuda")))
    return items


def _run(specs, identity=False, **kw):
    items = _items(specs, identity)
    keep = hip.verify_pairs(items, **kw)
    torch.cuda.synchronize()
    del keep
    outs = [dict(inlier=it["inlier"].cpu().numpy(), record=it["record"].cpu().numpy(), H=it["homography"].cpu().numpy().reshape(3, 3)) for it in items]
    for spec, out in zip(specs, outs):
        _invariants(spec, out, identity)
    return outs


def _invariants(spec, out, identity=False):
    """What holds for every set, whatever the input."""
    m0, rec, inl = spec[2], out["record"], out["inlier"]
    matched = np.ones(len(spec[0]), bool) if identity else (m0 > -1) & (m0 < len(spec[1]))
    assert set(np.unique(inl).tolist()) <= {0, 1}
    assert not inl[~matched].any()                                   # an unmatched row is never an inlier
    assert rec[COL["n_valid"]] == matched.sum() and rec[COL["n_inliers"]] == inl.sum() and rec[7] == 0
    assert rec[COL["ok"]] in (0.0, 1.0) and rec[COL["err_corner"]] == -1        # no h_ref in these calls
    if rec[COL["ok"]] == 0:
        assert not out["H"].any() and not inl.any() and not rec[2:6].any()
    else:
        assert np.isfinite(out["H"]).all() and out["H"][2, 2] == 1 and rec[COL["n_inliers"]] >= 4


def _compare(spec, out, v):
    """One set against verify_ref.verify."""
    rec = out["record"]
    assert rec[COL["ok"]] == v["ok"]
    if not v["ok"]:
        return
    for k in ("best_hyp", "best_hyp_inliers", "n_inliers", "lo_rounds"):
        assert rec[COL[k]] == v[k], (k, rec[COL[k]], v[k])
    np.testing.assert_array_equal(out["inlier"][spec[2] > -1].astype(bool), v["mask"])
    d = R.transfer_distance(out["H"], v["H"], R.transfer_points(spec))
    assert d <= TRANSFER, d


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("iters", R.ITERS)
@pytest.mark.parametrize("K", R.KS)
def test_against_the_restatement(K, iters):
    """Planted homography with 30 % outliers and unmatched rows; K crosses the wave, tile and chunk borders, iters the block of hypotheses."""
    spec = R.planted_spec(K)
    for lo in (1, 8):
        (out,) = _run([spec], thresh=R.THRESH, iters=iters, lo_iters=lo, seed=R.SEEDS.get(K, 1))
        v = R.fixture_expected(K, iters, lo)
        assert v["ok"] == (1 if K >= 4 else 0)
        _compare(spec, out, v)


def test_no_hypotheses_and_identical_points():
    spec = R.planted_spec(64)
    (out,) = _run([spec], iters=0, lo_iters=8, seed=1)
    assert out["record"][COL["ok"]] == 0
    kp0, kp1, m0, _ = spec
    same = (np.repeat(kp0[:1], 8, 0), np.repeat(kp1[:1], 8, 0), np.arange(8, dtype=np.int64))
    for lo in (0, 8):
        (out,) = _run([same], iters=64, lo_iters=lo, seed=1)
        assert out["record"][COL["ok"]] == 0


# ------------------------------------------------------------------------------------------------ anchor: lo_iters = 0 is gims_eval_pairs
def _eval_items(spec):
    kp0, kp1, m0, s0, H, h, w = spec
    n0 = len(kp0)
    return [dict(kpts0=torch.from_numpy(kp0).cuda(), kpts1=torch.from_numpy(kp1).cuda(), matches0=torch.from_numpy(m0).cuda(),
                 mscores0=torch.from_numpy(s0).cuda(), h_gt=H, height=h, width=w, gt0=torch.empty(n0, dtype=torch.int32, device="cuda"),
                 inlier=torch.empty(n0, dtype=torch.uint8, device="cuda"), record=torch.zeros(16, device="cuda"),
                 homographies=torch.zeros(18, device="cuda"))]


@pytest.mark.parametrize("kind,n0,iters", ANCHORS)
def test_lo_iters_0_equals_evaluate_pairs_and_the_oracle(kind, n0, iters):
    spec, seed = anchor_spec(kind, n0)
    (out,) = _run([spec], thresh=3.0, iters=iters, lo_iters=0, seed=seed)
    ev = _eval_items(spec)
    keep = hip.eval_pairs(ev, ransac_thresh=3.0, ransac_iters=iters, seed=seed)
    torch.cuda.synchronize()
    del keep
    e = C.compaction_expected(n0, "all", iters) if kind == "compaction" else C.two_model_expected(False)
    pts = np.concatenate([np.array([[0, 0], [0, spec[5]], [spec[6], spec[5]], [spec[6], 0]], dtype=np.float64), spec[0][spec[2] > -1].astype(np.float64)])
    np.testing.assert_array_equal(out["inlier"], ev[0]["inlier"].cpu().numpy())
    np.testing.assert_array_equal(out["inlier"].astype(bool), e["inlier"])
    assert out["record"][COL["n_inliers"]] == ev[0]["record"][6].item() == e["record"][6]
    assert out["record"][COL["lo_rounds"]] == 0 and out["record"][COL["ok"]] == 1
    assert R.transfer_distance(out["H"], ev[0]["homographies"][9:].cpu().numpy(), pts) <= TRANSFER
    assert R.transfer_distance(out["H"], e["Hr"], pts) <= TRANSFER


# ------------------------------------------------------------------------------------------------ ragged batch
def test_ragged_batch_with_degenerate_sets():
    """The degenerate sets of eval_cases between ordinary ones, in one call: ok = 0 where the oracle finds no model, and every set --
    ordinary or not -- bit-identical to a call of its own."""
    deg, _ = C.degenerate_batch()
    exp = C.degenerate_expected()
    ordinary = [R.planted_spec(K) for K in (65, 257, 1025)]
    names = list(deg)
    specs, who = [], []
    for i, name in enumerate(names):
        specs += [ordinary[i % 3], deg[name]]
        who += [None, name]
    specs.append(ordinary[0])
    who.append(None)
    kw = dict(thresh=3.0, iters=500, lo_iters=8, seed=C.RANSAC_SEED)
    outs = _run(specs, **kw)
    for spec, name, out in zip(specs, who, outs):
        if name is not None:
            assert out["record"][COL["ok"]] == exp[name]["record"][10], name
        (alone,) = _run([spec], **kw)
        for k in ("inlier", "record", "H"):
            assert out[k].tobytes() == alone[k].tobytes(), (name, k)


def test_identity_pairing_equals_explicit_matches():
    """matches0 = NULL is the pairing i <-> i."""
    for K in (5, 257, 1025):
        p0, p1 = R.correspondences(R.planted_spec(K))
        spec = (p0, p1, np.arange(K, dtype=np.int64))
        kw = dict(thresh=3.0, iters=64, lo_iters=8, seed=3)
        (a,), (b,) = _run([spec], identity=True, **kw), _run([spec], **kw)
        for k in ("inlier", "record", "H"):
            assert a[k].tobytes() == b[k].tobytes(), (K, k)
        assert a["record"][COL["ok"]] == 1


def test_unmatched_rows_and_partners_out_of_range_are_no_correspondences():
    kp0, kp1, m0, _ = R.planted_spec(257)
    m = m0.copy()
    rows = np.nonzero(m > -1)[0]
    m[rows[::9]] = len(kp1) + 5                          # beyond keypoints1: treated as unmatched, never read
    (out,) = _run([(kp0, kp1, m)], thresh=3.0, iters=64, lo_iters=8, seed=3)
    keep = np.where(m < len(kp1), m, -1)
    (ref,) = _run([(kp0, kp1, keep)], thresh=3.0, iters=64, lo_iters=8, seed=3)
    assert out["record"][COL["n_valid"]] == (keep > -1).sum()
    for k in ("inlier", "record", "H"):
        assert out[k].tobytes() == ref[k].tobytes(), k
    assert not out["inlier"][keep == -1].any() and out["inlier"].any()


# ------------------------------------------------------------------------------------------------ the Python surface
def test_find_homography():
    p0, p1 = R.correspondences(R.planted_spec(3))
    assert find_homography(p0, p1) == (None, None)
    K = 257
    p0, p1 = R.correspondences(R.planted_spec(K))
    H, mask = find_homography(torch.from_numpy(p0).cuda(), p1, thresh=3.0, iters=500, lo_iters=8, seed=R.SEEDS[K])
    v = R.fixture_expected(K, 500, 8)
    assert H.is_cuda and H.shape == (3, 3) and H.dtype == torch.float32 and mask.shape == (K, 1) and mask.dtype == torch.uint8
    np.testing.assert_array_equal(mask.cpu().numpy()[:, 0].astype(bool), v["mask"])
    assert R.transfer_distance(H.cpu().numpy(), v["H"], R.transfer_points(R.planted_spec(K))) <= TRANSFER
    same = np.repeat(p0[:1], 8, 0)
    assert find_homography(same, same, iters=64) == (None, None)
    with pytest.raises(ValueError):
        find_homography(p0, p1[:-1])


def _model():
    m = GMatcher({"sinkhorn_iterations": 20, "match_threshold": 0.02}).eval()
    m.load_state_dict(synth.make_state_dict(123))
    m(pair_to_data(synth.make_pair(256, 1002), 15, 2, 7, device="cuda"))      # settle attention_precision='auto' before calls are compared
    return m


SWEEP_GRID = [(15, 2, 7), (25, 7, 8), (10, 0, 300)]        # the last keeps nothing: no component of 256 keypoints has 300 members
VERIFY = dict(thresh=3.0, iters=500, lo_iters=8, seed=11)


@pytest.mark.parametrize("outputs", ["all", "matches"])
def test_sweep_with_verification(outputs):
    m = _model()
    data = pair_to_data(synth.make_pair(256, 1002), 25, 7, 8, device="cuda")
    plain = m.sweep(data, SWEEP_GRID, outputs=outputs)
    recs = m.sweep(data, SWEEP_GRID, outputs=outputs, verify=VERIFY)
    assert [r["error"] is None for r in recs] == [True, True, False]
    for a, b in zip(plain, recs):
        assert set(a) == {"radius", "percentile", "min_size", "delaunay", "kept0", "kept1", "n_matches", "error", "result"}
        assert set(b) == set(a) | {"correct_matches", "homography", "inlier"}
    assert recs[2]["correct_matches"] == 0 and recs[2]["homography"] is None and recs[2]["inlier"] is None
    live = [r for r in m.sweep(data, SWEEP_GRID, outputs="all") if r["error"] is None]
    assert all(torch.equal(a["result"]["matches0"], b["result"]["matches0"]) for a, b in zip(live, recs[:2]))
    ref = verify_pairs([r["result"] for r in live], [r["result"] for r in live], **VERIFY)
    torch.cuda.synchronize()
    for q, rec in enumerate(recs[:2]):
        assert rec["correct_matches"].dim() == 0 and rec["correct_matches"].is_cuda
        assert rec["correct_matches"].item() == ref["records"][q, COL["n_inliers"]].item() == rec["inlier"].sum().item()
        assert torch.equal(rec["homography"], ref["homographies"][q]) and torch.equal(rec["inlier"], ref["inlier"][q])
        assert rec["inlier"].shape == (rec["kept0"],)
        assert rec["correct_matches"].item() <= rec["n_matches"].item()


def _eval_inputs():
    kp0, kp1, m0, H = R.planted_spec(257)
    specs = [C.compaction_case(1025, "all")[0],
             (kp0, kp1, m0, np.full(len(kp0), 0.5, dtype=np.float32) + np.arange(len(kp0), dtype=np.float32) * 1e-4, H, 600, 800)]
    datas = [dict(keypoints0=torch.from_numpy(s[0]).cuda()[None], keypoints1=torch.from_numpy(s[1]).cuda()[None],
                  image0=np.zeros((s[5], s[6], 3), dtype=np.uint8)) for s in specs]
    outs = [dict(matches0=torch.from_numpy(s[2]).cuda()[None], matching_scores0=torch.from_numpy(s[3]).cuda()[None]) for s in specs]
    return specs, datas, outs, [s[4] for s in specs]


def test_evaluate_pairs_with_local_optimisation():
    specs, datas, outs, hs = _eval_inputs()
    kw = dict(ransac_thresh=3.0, ransac_iters=500, seed=R.SEEDS[257])
    base = evalh.evaluate_pairs(datas, outs, hs, **kw)
    zero = evalh.evaluate_pairs(datas, outs, hs, lo_iters=0, **kw)
    lo = evalh.evaluate_pairs(datas, outs, hs, lo_iters=8, **kw)
    ver = verify_pairs(datas, outs, thresh=3.0, iters=500, lo_iters=8, seed=R.SEEDS[257], h_refs=hs)
    torch.cuda.synchronize()
    # lo_iters = 0 is today's call, bit for bit
    for k in ("records", "homographies"):
        assert base[k].cpu().numpy().tobytes() == zero[k].cpu().numpy().tobytes(), k
    for k in ("gt0", "inlier"):
        assert all(torch.equal(a, b) for a, b in zip(base[k], zero[k])), k
    # lo_iters = 8: the replaced values are verify_pairs'; everything else stays
    ecol = {k: i for i, k in enumerate(evalh.RECORD_FIELDS)}
    replaced = [ecol[k] for k in ("n_inliers", "err_ransac", "ransac_ok")]
    others = [c for c in range(16) if c not in replaced]
    rl, rb, rv = lo["records"].cpu().numpy(), base["records"].cpu().numpy(), ver["records"].cpu().numpy()
    assert rl[:, others].tobytes() == rb[:, others].tobytes()
    assert rl[:, replaced].tobytes() == rv[:, [COL["n_inliers"], COL["err_corner"], COL["ok"]]].tobytes()
    assert torch.equal(lo["homographies"][:, 0], base["homographies"][:, 0]) and torch.equal(lo["homographies"][:, 1], ver["homographies"])
    assert all(torch.equal(a, b) for a, b in zip(lo["inlier"], ver["inlier"])) and all(torch.equal(a, b) for a, b in zip(lo["gt0"], base["gt0"]))
    # err_ransac against the restatement's corner error: the transfer bound plus float32 rounding at magnitude 800
    v = R.fixture_expected(257, 500, 8)
    assert rl[1, ecol["ransac_ok"]] == 1 and rl[1, ecol["n_inliers"]] == v["n_inliers"]
    assert abs(rl[1, ecol["err_ransac"]] - E.corner_error(v["H"], hs[1], 600, 800)) <= 2e-3
    assert (rl[:, ecol["n_inliers"]] >= rb[:, ecol["n_inliers"]]).all()
