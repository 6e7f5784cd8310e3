"""The adversarial evaluation inputs of tests/eval_cases.py ARE adversarial: every condition the GPU tests of csrc/eval.hip rely on
(tests/test_eval_edges_gpu.py, tests/test_labels_edges_gpu.py), asserted with the CPU oracle alone.  A case that drifts -- another seed, a
changed generator -- fails here and not silently on the device."""
import numpy as np
import pytest
import torch

from oracle import eval_oracle as E
from tests import eval_cases as C
from tests.helpers import load_golden

EPS64 = np.finfo(np.float64).eps


def _oracle_gt0(spec, thr, iters):
    kp0, kp1, _, _, H, _, _ = spec
    ma = E.find_gt_matches(torch.from_numpy(kp0), torch.from_numpy(kp1), torch.from_numpy(H), thr, iters)
    gt = np.full(len(kp0), -1, dtype=np.int64)
    gt[ma[0]] = ma[1]
    return gt, ma


def _system_cond(spec, positions):
    """Condition number of the 4-point system through the valid matches at `positions`."""
    kp0, kp1, m0 = spec[:3]
    idx = np.nonzero(m0 > -1)[0][positions]
    A = np.zeros((8, 8))
    for k, i in enumerate(idx):
        x, y, u, v = (float(t) for t in (*kp0[i], *kp1[m0[i]]))
        A[2 * k], A[2 * k + 1] = [x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]
    return np.linalg.cond(A)


def _h_through(spec, positions):
    kp0, kp1, m0 = spec[:3]
    idx = np.nonzero(m0 > -1)[0][positions]
    return E.homography_from_4(kp0[idx], kp1[m0[idx]])


# ------------------------------------------------------------------------------------------------ 1. distance ties
@pytest.mark.parametrize("case", sorted(C.LATTICE_CASES))
@pytest.mark.parametrize("shift", sorted(C.LATTICE_SHIFTS))
def test_lattice_oracle_equals_first_minimum(case, shift):
    spec, _ = C.lattice_case(case, shift)
    counts = []
    for it in C.TIE_ITERS:
        gt, _ = _oracle_gt0(spec, 3, it)
        np.testing.assert_array_equal(gt, C.first_min_gt_matches(spec[0], spec[1], spec[4], 3, it))
        counts.append(int((gt >= 0).sum()))
    if shift == "id":
        # no tie under the identity: every image-1 point has its own lattice point at distance 0, all found in one iteration
        assert counts == [min(len(spec[0]), len(spec[1]))] * 4
        return
    d = C.ref_distances(spec[0], spec[1], spec[4])
    tied = ((d == d.min(1, keepdims=True)).sum(1) >= 2).mean()
    assert tied >= 0.25, tied                                                       # [cond] exact float32 ties at the minimum
    assert counts[0] < counts[1] < counts[2] <= counts[3], counts                   # [cond] later iterations do real work


@pytest.mark.parametrize("name", sorted(C.TIE_GOLDENS))
def test_lattice_oracle_equals_reference_golden(name):
    """The reference's own torch_find_matches on the tie cases: index arrays after 6 iterations, prefixes for fewer."""
    g = load_golden(name)
    case, shift = C.TIE_GOLDENS[name]
    spec, args = C.lattice_case(case, shift)
    assert [args[k] for k in ("nx", "ny", "spacing", "n0", "n1", "seed")] == g["lattice"].tolist()
    assert list(C.LATTICE_SHIFTS[shift]) == g["shift"].tolist() and tuple(g["iters"]) == C.TIE_ITERS
    for it, n in zip(g["iters"], g["n_after"]):
        gt, (ma0, ma1, mi0, mi1) = _oracle_gt0(spec, 3, int(it))
        np.testing.assert_array_equal(ma0, g["ma0"][:n])
        np.testing.assert_array_equal(ma1, g["ma1"][:n])
        np.testing.assert_array_equal(gt, C.golden_gt0(g, int(it), len(spec[0])))
        np.testing.assert_array_equal(gt, C.first_min_gt_matches(spec[0], spec[1], spec[4], 3, int(it)))
        if it == g["iters"][-1]:
            np.testing.assert_array_equal(mi0, g["miss0"])
            np.testing.assert_array_equal(mi1, g["miss1"])


# ------------------------------------------------------------------------------------------------ 2. strict threshold
def test_threshold_cases():
    spec, _ = C.threshold_case()
    d = C.ref_distances(spec[0], spec[1], spec[4]).min(1)
    assert (d == np.float32(3)).all()                                               # [cond] every nearest distance is exactly 3.0
    assert C.expected(spec, 3.0, 1, ransac_iters=0)["record"][1] == 0
    assert C.expected(spec, C.THRESH_UP, 1, ransac_iters=0)["record"][1] == 100
    spec, _ = C.threshold21_case()
    d = C.ref_distances(spec[0], spec[1], spec[4]).min(1)
    below, at, above = int((d < C.T21).sum()), int((d == C.T21).sum()), int((d > C.T21).sum())
    assert below >= 10 and above >= 10 and at >= 1, (below, at, above)               # [cond] distances on both sides and on float32(2.1)
    assert (d == np.nextafter(C.T21, np.float32(0))).any() and (d == np.nextafter(C.T21, np.float32(3))).any()
    # 2.1 reaches the comparison rounded to float32: a distance of exactly float32(2.1) is no match
    assert C.expected(spec, 2.1, 1, ransac_iters=0)["record"][1] == below


# ------------------------------------------------------------------------------------------------ 3. compaction
def test_compaction_cases():
    big, spread = 0, 0
    assert {n for n, _, _ in C.COMPACTION} == {1023, 1025, 2049, 2500} and {p for _, p, _ in C.COMPACTION} == {"all", "tail", "seventh"}
    assert {it for _, _, it in C.COMPACTION} >= {3000, 1001}
    for n0, pattern, iters in C.COMPACTION:
        spec, ex = C.compaction_case(n0, pattern)
        e = C.compaction_expected(n0, pattern, iters)
        assert e["K"] == ex["K"] and e["Hd"] is not None and e["Hr"] is not None
        big += ex["K"] > 1024
        spread += len(set((ex["top4"] // 1024).tolist())) >= 2
        assert len(np.unique(spec[3][spec[2] > -1])) == ex["K"]                       # no two confidences equal
        assert C.threshold_margin(spec, e["Hr"]) > 1e-6                               # [cond] no match on the RANSAC threshold
        assert _system_cond(spec, ex["top4"]) * EPS64 < 1e-6                          # the 4-point solve is far more exact than rtol 1e-4
        assert e["record"][8] < 1.0                                                   # the planted homography is recovered
    assert big >= 2                                                                   # [cond] K > 1024 in at least two patterns
    assert spread >= 1                                                                # [cond] the top four sit in two chunks somewhere
    assert C.compaction_case(2500, "tail")[1]["K"] > 1024 and C.compaction_case(2500, "all")[1]["K"] > 1024


# ------------------------------------------------------------------------------------------------ 4. score ties
@pytest.mark.parametrize("n0,pattern,kind", C.SCORE_TIES)
def test_score_tie_cases(n0, pattern, kind):
    spec, ex = C.score_tie_case(n0, pattern, kind)
    e = C.score_tie_expected(n0, pattern, kind)
    tied = ex["tied"]
    assert len(tied) >= 5
    s = spec[3][ex["valid_idx"]]
    assert (s[tied] == 1.0).all() and (np.delete(s, tied) < 1.0).all()
    Hd = e["Hd"]
    np.testing.assert_allclose(Hd, _h_through(spec, tied[:4]), rtol=1e-9)              # the oracle takes the first four of the tied
    tol = 1e-5 + 1e-4 * np.abs(Hd)                                                    # the comparison tolerance of the GPU test
    for other in (tied[-4:], tied[1:5]):                                              # [cond] a wrong tie-break cannot pass
        assert (np.abs(_h_through(spec, other) - Hd) > 100 * tol).any()
    assert _system_cond(spec, tied[:4]) * EPS64 < 1e-6
    if kind == "classes":
        first = tied[:4]
        assert len(set(((first % 1024) // 64).tolist())) >= 3                         # different waves of the counts kernel
        if ex["K"] > 1030:                                                            # (1023 / 1025: all four in chunk 0, 1024 has to lose)
            assert len(set((first // 1024).tolist())) >= 2                            # ... and different 1024-chunks of its scan
            assert len(set((tied % 1024).tolist())) < len(tied)                       # two tied matches in ONE thread's strided list


# ------------------------------------------------------------------------------------------------ 5. few / degenerate
def test_degenerate_cases():
    specs, K = C.degenerate_batch()
    exp = C.degenerate_expected()
    assert [K[f"k{k}"] for k in (0, 1, 3, 4, 5)] == [0, 1, 3, 4, 5] and K["dup8"] == 8 and K["three3"] == 9
    assert (len(specs["n0_1"][0]), len(specs["n0_1"][1])) == (1, 700) and (len(specs["n1_1"][0]), len(specs["n1_1"][1])) == (700, 1)
    for name, e in exp.items():
        r = e["record"]
        assert np.isnan(r[4]) == (K[name] == 0) and np.isnan(r[5]) == (r[2] + r[3] == 0), name
        if K[name] < 4 or name in ("dup8", "three3"):
            assert r[9] == 0 and r[10] == 0 and r[7] == -1 and r[8] == -1 and r[6] == 0 and not e["homographies"].any(), name
        else:
            assert r[9] == 1 and r[10] == 1, name
            assert C.threshold_margin(specs[name], e["Hr"]) > 1e-6
    # the duplicates are exact, in both images, and the matches point at distinct indices
    for name in ("dup8", "three3"):
        kp0, kp1, m0 = specs[name][:3]
        i = np.nonzero(m0 > -1)[0]
        assert len(set(m0[i].tolist())) == len(i)
        assert len(np.unique(kp0[i], axis=0)) == len(np.unique(kp1[m0[i]], axis=0)) == (1 if name == "dup8" else 3)
    # K = 4: every hypothesis draws the same four points, and RANSAC returns the model through them
    assert sorted(E.ransac_sample(C.RANSAC_SEED, 17, 4).tolist()) == [0, 1, 2, 3]
    np.testing.assert_allclose(exp["k4"]["Hr"], exp["k4"]["Hd"], rtol=1e-6, atol=1e-8)
    assert exp["k4"]["record"][6] == 4
    for s in C.ordinary_pairs():
        e = C.expected(s, ransac_iters=500, seed=C.RANSAC_SEED)
        assert e["K"] >= 12 and e["record"][9] == 1 and e["record"][10] == 1 and C.threshold_margin(s, e["Hr"]) > 1e-6


# ------------------------------------------------------------------------------------------------ 6. tied hypotheses
def test_two_model_case():
    spec, ex = C.two_model_case()
    kp0, kp1, m0 = spec[:3]
    assert (kp0 == np.rint(kp0)).all() and (kp1 == np.rint(kp1)).all() and (m0 > -1).sum() == 100
    np.testing.assert_array_equal(kp1[m0[:15]] - kp0[:15], np.tile(np.float32(C.MODEL_A), (15, 1)))
    np.testing.assert_array_equal(kp1[m0[15:30]] - kp0[15:30], np.tile(np.float32(C.MODEL_B), (15, 1)))
    cond = C.two_model_conditions(ex["seed"])
    assert cond is not None                                                           # the pinned seed fits ...
    assert (cond["h_star"], cond["star_is_a"]) == (ex["h_star"], ex["star_is_a"])     # ... and the pinned h* is its h*
    a, b, h_star, h_other = cond["a"], cond["b"], cond["h_star"], cond["h_other"]
    cnt = C.hypothesis_counts(spec, ex["seed"], C.TWO_MODEL_ITERS)
    assert cnt.max() == 15                                                            # [cond] the best count is 15
    assert a and b and (cnt[a] == 15).all() and (cnt[b] == 15).all()                  # [cond] ... attained by both models
    assert set(np.nonzero(cnt == 15)[0].tolist()) == set(a) | set(b)                  # ... and by pure hypotheses only
    assert int(cnt.argmax()) == h_star >= 1024                                        # [cond] the earliest is past the first stride
    pure_star, pure_other = (a, b) if ex["star_is_a"] else (b, a)
    assert h_other in pure_other and h_other > h_star and h_other % 1024 < h_star % 1024          # [cond] the tie crosses the stride
    assert np.sort(cnt)[-len(a) - len(b) - 1] <= 12                                   # nothing else comes near: no count hangs on rounding
    # the kernel's three-level reduction over the ORACLE's counts returns h*; with "lower index" turned into "higher" in the lane reduction,
    # in the wave merge, or in both, it returns a hypothesis of the other model: no such mistake can pass the GPU test
    assert C.finish_reduction(cnt) == h_star
    for flips in ((True, False), (False, True), (True, True)):
        assert C.finish_reduction(cnt, *flips) in pure_other, flips
    assert any(h != h_star and (h % 1024) // 64 == (h_star % 1024) // 64 for h in pure_other)    # a tie inside h*'s own wave
    e = C.two_model_expected(False)
    model = C.MODEL_A if ex["star_is_a"] else C.MODEL_B
    np.testing.assert_allclose(e["Hr"], C.TRANSLATE(*model), rtol=0, atol=1e-9)
    group = np.arange(15) + (0 if ex["star_is_a"] else 15)
    np.testing.assert_array_equal(np.nonzero(e["inlier"])[0], group)
    for hb in (False, True):
        e = C.two_model_expected(hb)
        assert e["record"][6] == 15 and C.threshold_margin(spec, e["Hr"]) > 1e-6


# ------------------------------------------------------------------------------------------------ 7, labels
def test_ragged_and_label_batches():
    shapes = [(len(s[0]), len(s[1])) for s in C.ragged_batch()]
    assert shapes == [(5, 2500), (2500, 5), (1025, 700), (64, 65), (300, 300)]
    for s in C.ragged_batch():
        assert s[2].max() < len(s[1]) and s[2].min() >= -1                            # every match index is inside image 1
    k0, k1, hs, names = C.label_batch()
    shapes = {(len(a), len(b)) for a, b in zip(k0, k1)}
    assert shapes >= {(1, 700), (700, 1), (1023, 1025), (2049, 1024)} and len(k0) >= 6
    from tests.warp_ref import label_rows
    rows = label_rows(k0, k1, hs, 3, 3)
    per = {n: rows[rows[:, 0] == k] for k, n in enumerate(names)}
    assert (per["identity"][:, 1:] >= 0).all() and len(per["identity"]) == len(k0[names.index("identity")])
    assert not (per["far"][:, 1:] >= 0).all(1).any()
