"""gims_eval_pairs (csrc/eval.hip) where its rules decide: distance ties, the strict threshold, compaction over several 1024-chunks,
confidence ties, fewer than four or exactly degenerate matches, tied hypotheses across the 1024 stride of the finish kernel, ragged
batches, and a workspace it has to initialise itself.  Inputs and oracle results come from tests/eval_cases.py; that they are as
adversarial as claimed is asserted on the CPU in tests/test_eval_cases_cpu.py.

Tolerances (those of test_eval_gpu.py::test_records_vs_oracle_batched): index sets and counts exact, precision / recall abs 1e-6,
homographies rtol 1e-4 / atol 1e-5, corner errors rel 1e-3 / abs 1e-3.  Inlier masks are exact: no case has a match within a relative
1e-6 of the RANSAC threshold (CPU test)."""
import numpy as np
import pytest
import torch

from tests import eval_cases as C
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

GARBAGE = 0x5B


@pytest.fixture(scope="module")
def hipmod():
    from gims_amd import hip
    hip.load()
    return hip


def _items(specs, garbage=False):
    items = []
    for kp0, kp1, m0, s0, H, h, w in specs:
        n0 = len(kp0)
        rec = torch.zeros(16)
        rec[11:] = torch.from_numpy(C.SENTINEL)
        it = dict(kpts0=torch.from_numpy(kp0).cuda(), kpts1=torch.from_numpy(kp1).cuda(), matches0=torch.from_numpy(m0).cuda(),
                  mscores0=torch.from_numpy(s0).cuda(), h_gt=H, height=h, width=w,
                  gt0=torch.empty(n0, dtype=torch.int32, device="cuda"), inlier=torch.empty(n0, dtype=torch.uint8, device="cuda"),
                  record=rec.cuda(), homographies=torch.zeros(18, device="cuda"))
        if garbage:                                               # outputs the call has to overwrite in full
            it["gt0"].fill_(0x5B5B5B5B)
            it["inlier"].fill_(GARBAGE)
            it["record"][:11] = float("nan")
            it["homographies"].fill_(-7.5e8)
        items.append(it)
    return items


def _fetch(items):
    torch.cuda.synchronize()
    return [dict(gt0=it["gt0"].cpu().numpy(), inlier=it["inlier"].cpu().numpy(), record=it["record"].cpu().numpy(),
                 homographies=it["homographies"].cpu().numpy()) for it in items]


def _run(hip, specs, garbage=True, work=None, **kw):
    items = _items(specs, garbage)
    keep = hip.eval_pairs(items, work=work, **kw)
    outs = _fetch(items)
    for spec, out in zip(specs, outs):
        _invariants(spec, out)
    return outs, keep


def _invariants(spec, out):
    """What holds for every pair, whatever the input."""
    m0, rec, hom, inl, gt0 = spec[2], out["record"], out["homographies"].reshape(2, 9), out["inlier"], out["gt0"]
    assert set(np.unique(inl).tolist()) <= {0, 1}
    assert rec[6] == inl.sum()
    assert not inl[m0 == -1].any()
    for ok, err, h in ((rec[9], rec[7], hom[0]), (rec[10], rec[8], hom[1])):
        assert ok in (0.0, 1.0)
        if ok == 0:
            assert err == -1 and not h.any()
        else:
            assert np.isfinite(h).all() and np.isfinite(err) and err >= 0
    assert rec[0] == (m0 > -1).sum()
    assert rec[1] == (gt0 >= 0).sum()
    assert ((gt0 >= -1) & (gt0 < len(spec[1]))).all()
    assert rec[11:].tobytes() == C.SENTINEL.tobytes()             # the caller's columns are the caller's


def _compare(spec, out, e, models=True):
    """One pair against eval_cases.expected."""
    rec, ref = out["record"], e["record"]
    np.testing.assert_array_equal(out["gt0"], e["gt0"])
    np.testing.assert_array_equal(rec[:4], ref[:4])
    for c in (4, 5):
        assert np.isnan(rec[c]) == np.isnan(ref[c])
        assert np.isnan(ref[c]) or rec[c] == pytest.approx(ref[c], abs=1e-6)
    if not models:
        return
    hom = out["homographies"].reshape(2, 3, 3)
    assert rec[9] == ref[9] and rec[10] == ref[10]
    np.testing.assert_allclose(hom[0], e["homographies"][0], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(hom[1], e["homographies"][1], rtol=1e-4, atol=1e-5)
    assert rec[7] == pytest.approx(ref[7], rel=1e-3, abs=1e-3)
    assert rec[8] == pytest.approx(ref[8], rel=1e-3, abs=1e-3)
    np.testing.assert_array_equal(out["inlier"].astype(bool), e["inlier"])
    assert rec[6] == ref[6]


# ------------------------------------------------------------------------------------------------ 1. GT matching under distance ties
@pytest.mark.parametrize("case", sorted(C.LATTICE_CASES))
@pytest.mark.parametrize("shift", sorted(C.LATTICE_SHIFTS))
def test_gt_matching_under_distance_ties(hipmod, case, shift):
    """Every projected point of a lattice shifted by half its spacing has two or four nearest neighbours at exactly the same float32
    distance: the first minimum wins, in both directions, in every iteration, as in torch.argmin."""
    spec, _ = C.lattice_case(case, shift)
    golden = [load_golden(n) for n, cs in C.TIE_GOLDENS.items() if cs == (case, shift)]
    for it in C.TIE_ITERS:
        (out,), _ = _run(hipmod, [spec], dist_thresh=3, n_iters=it, ransac_iters=0)
        e = C.expected(spec, 3, it, ransac_iters=0)
        _compare(spec, out, e)
        np.testing.assert_array_equal(out["gt0"], C.first_min_gt_matches(spec[0], spec[1], spec[4], 3, it))
        for g in golden:
            np.testing.assert_array_equal(out["gt0"], C.golden_gt0(g, it, len(spec[0])))


# ------------------------------------------------------------------------------------------------ 2. strict threshold
def test_distance_threshold_is_strict(hipmod):
    spec, _ = C.threshold_case()
    (out,), _ = _run(hipmod, [spec], dist_thresh=3.0, n_iters=1, ransac_iters=0)
    assert out["record"][1] == 0 and (out["gt0"] == -1).all()
    (out,), _ = _run(hipmod, [spec], dist_thresh=C.THRESH_UP, n_iters=1, ransac_iters=0)
    assert out["record"][1] == 100
    _compare(spec, out, C.expected(spec, C.THRESH_UP, 1, ransac_iters=0))
    # 2.1 is no float32: the comparison sees it rounded (down), and a distance of exactly that float32 is not below it
    spec, _ = C.threshold21_case()
    for it in (1, 3):
        (out,), _ = _run(hipmod, [spec], dist_thresh=2.1, n_iters=it, ransac_iters=0)
        _compare(spec, out, C.expected(spec, 2.1, it, ransac_iters=0))


# ------------------------------------------------------------------------------------------------ 3. compaction across chunks
@pytest.mark.parametrize("n0,pattern,iters", C.COMPACTION)
def test_compaction_across_chunks(hipmod, n0, pattern, iters):
    """More than 1024 valid matches, none in the first chunk, or a sparse set that touches every chunk boundary: the ordered list of valid
    matches feeds the top-4 selection, the RANSAC sampler and the inlier mask, so every output depends on its order."""
    spec, _ = C.compaction_case(n0, pattern)
    (out,), _ = _run(hipmod, [spec], dist_thresh=3, n_iters=3, ransac_thresh=3.0, ransac_iters=iters, seed=C.RANSAC_SEED)
    _compare(spec, out, C.compaction_expected(n0, pattern, iters))


# ------------------------------------------------------------------------------------------------ 4. score ties
@pytest.mark.parametrize("n0,pattern,kind", C.SCORE_TIES)
def test_confidence_ties_take_the_earlier_match(hipmod, n0, pattern, kind):
    spec, _ = C.score_tie_case(n0, pattern, kind)
    (out,), _ = _run(hipmod, [spec], dist_thresh=3, n_iters=3, ransac_iters=0)
    _compare(spec, out, C.score_tie_expected(n0, pattern, kind))


# ------------------------------------------------------------------------------------------------ 5. few or degenerate matches
def test_few_and_degenerate_matches_in_one_batch(hipmod):
    from gims_amd import evalh
    specs, K = C.degenerate_batch()
    exp = C.degenerate_expected()
    names = list(specs)
    ordinary = C.ordinary_pairs()
    outs, _ = _run(hipmod, [specs[n] for n in names] + ordinary, dist_thresh=3, n_iters=3, ransac_iters=500, seed=C.RANSAC_SEED)
    for n, out in zip(names, outs):
        _compare(specs[n], out, exp[n])
        rec = out["record"]
        assert np.isnan(rec[4]) == (K[n] == 0), n
        assert np.isnan(rec[5]) == (rec[2] + rec[3] == 0), n
        if K[n] < 4 or n in ("dup8", "three3"):
            assert rec[9] == 0 and rec[10] == 0 and rec[6] == 0, n
    k4 = outs[names.index("k4")]["homographies"].reshape(2, 9)
    np.testing.assert_allclose(k4[1], k4[0], rtol=1e-4, atol=1e-5)             # every hypothesis is the same four points
    for s, out in zip(ordinary, outs[len(names):]):
        _compare(s, out, C.expected(s, ransac_iters=500, seed=C.RANSAC_SEED))
    summ = evalh.summarize(np.stack([o["record"] for o in outs]))
    assert summ["n_pairs"] == len(ordinary)
    flat = [summ["precision"], summ["recall"], summ["mean_inliers"], *summ["auc_dlt"], *summ["auc_ransac"]]
    assert np.isfinite(flat).all(), summ


# ------------------------------------------------------------------------------------------------ 6. first best hypothesis
def test_first_best_hypothesis_across_the_stride(hipmod):
    """Two exact translations with 15 inliers each: the earliest 15-inlier hypothesis h* >= 1024 belongs to one model, a later one of the
    other model sits at a lower position modulo 1024.  "First hypothesis with the most inliers" returns the model of h*."""
    spec, ex = C.two_model_case()
    (out,), _ = _run(hipmod, [spec], dist_thresh=3, n_iters=3, ransac_thresh=3.0, ransac_iters=C.TWO_MODEL_ITERS, seed=ex["seed"])
    model = C.MODEL_A if ex["star_is_a"] else C.MODEL_B
    np.testing.assert_allclose(out["homographies"].reshape(2, 3, 3)[1], C.TRANSLATE(*model), rtol=0, atol=1e-6)
    np.testing.assert_array_equal(np.nonzero(out["inlier"])[0], np.arange(15) + (0 if ex["star_is_a"] else 15))
    _compare(spec, out, C.two_model_expected(False))
    # the seed is 64 bits wide
    (out,), _ = _run(hipmod, [spec], dist_thresh=3, n_iters=3, ransac_thresh=3.0, ransac_iters=C.TWO_MODEL_ITERS, seed=ex["seed"] | (1 << 63))
    _compare(spec, out, C.two_model_expected(True))


# ------------------------------------------------------------------------------------------------ 7. ragged batch
def _bytes(outs):
    return [{k: v.tobytes() for k, v in o.items()} for o in outs]


RAGGED_KW = dict(dist_thresh=3, n_iters=3, ransac_thresh=3.0, ransac_iters=3000, seed=7)


def test_ragged_batch_equals_single_calls(hipmod):
    specs = C.ragged_batch()
    batch, _ = _run(hipmod, specs, **RAGGED_KW)
    for k, spec in enumerate(specs):
        single, _ = _run(hipmod, [spec], **RAGGED_KW)
        assert _bytes(single)[0] == _bytes(batch)[k], k


# ------------------------------------------------------------------------------------------------ 8. workspace hygiene
def test_workspace_is_initialised_and_respected(hipmod):
    specs = C.ragged_batch()
    ref, keep = _run(hipmod, specs, garbage=False, **RAGGED_KW)
    need = keep.numel()
    for fill in (0x00, 0xFF, 0x7F):
        work = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        work[:need] = fill
        outs, used = _run(hipmod, specs, garbage=True, work=work, **RAGGED_KW)
        assert used.data_ptr() == work.data_ptr()
        assert _bytes(outs) == _bytes(ref), hex(fill)
        assert (work[need:] == 0xA5).all().item(), hex(fill)
