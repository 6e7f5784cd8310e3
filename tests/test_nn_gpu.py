"""Descriptor baselines on the device (gims_nn_match, csrc/nn.hip, through gims_amd.baselines) against the float64 restatement
(tests/nn_ref.py: every row) and the reference's own outputs (tests/golden/nn_*.npz: the exclusion rule and 1 % cap of test_nn_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

from gims_amd import baselines, evalh, synth
from tests import nn_ref
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

NAMES = [name for name, _ in nn_ref.FIXTURES]
BITWISE = ("matches0", "matching_scores0", "ratios0", "nn0", "nn0_second", "dist0", "dist0_second", "match0")


@functools.lru_cache(maxsize=None)
def fixture(name):
    g = load_golden(name)
    recipe = nn_ref.recipe_from_npz(g)
    a, b = nn_ref.build_fixture(recipe)
    return recipe, a, b, g


@functools.lru_cache(maxsize=None)
def restated(name, mutual):
    recipe, a, b, _ = fixture(name)
    return nn_ref.solve(a, b, recipe["threshold"], mutual)


def data_of(a, b):
    return dict(descriptors0=torch.from_numpy(a)[None].cuda(), descriptors1=torch.from_numpy(b)[None].cuda())


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


@functools.lru_cache(maxsize=None)
def device_run(name, method, exhaustive=False):
    """One pair alone; the default flow carries the candidate pass's debug output."""
    recipe, a, b, _ = fixture(name)
    out = baselines.nn_match_pairs([data_of(a, b)], method, recipe["threshold"], exhaustive=exhaustive, debug=not exhaustive)[0]
    return host(out)


def assert_ulp(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    tol = np.spacing(np.maximum(np.abs(got[ok]), np.abs(want[ok])))
    worst = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)) - tol
    assert (worst <= 0).all(), f"{what}: {int((worst > 0).sum())} values differ by more than 1 ulp"


def assert_equals_restatement(o, ref, mutual, what):
    np.testing.assert_array_equal(o["nn0"][0], ref["nn1"], err_msg=what)
    np.testing.assert_array_equal(o["nn0_second"][0], ref["nn2"], err_msg=what)
    np.testing.assert_array_equal(o["match0"][0].astype(bool), ref["match"], err_msg=what)
    np.testing.assert_array_equal(o["matches0"][0], ref["matches0"], err_msg=what)
    assert_ulp(o["dist0"][0], ref["d1"], what + " d1")
    assert_ulp(o["dist0_second"][0], ref["d2"], what + " d2")
    assert_ulp(o["ratios0"][0], ref["ratio"], what + " ratio")
    m = ref["match"]
    np.testing.assert_array_equal(o["matching_scores0"][0][~m], 0.0)
    np.testing.assert_array_equal(o["matching_scores0"][0][m], (np.float32(1) - o["ratios0"][0])[m])
    if mutual:
        np.testing.assert_array_equal(o["nn1"][0], ref["cnn1"], err_msg=what)
        np.testing.assert_array_equal(o["matches1"][0], ref["matches1"], err_msg=what)


@pytest.mark.parametrize("method", ["nndr", "mnn"])
@pytest.mark.parametrize("name", NAMES)
def test_every_row_equals_the_restatement(name, method):
    """nn1, nn2, cnn1 and the match masks on EVERY row; d1, d2 and the ratio within 1 float32 ulp.  Plain fixtures certify every row."""
    o = device_run(name, method)
    assert_equals_restatement(o, restated(name, method == "mnn"), method == "mnn", f"{name} {method}")
    assert o["fallback_rows"].tolist() == [0, 0], o["fallback_rows"]


@pytest.mark.parametrize("method", ["nndr", "mnn"])
@pytest.mark.parametrize("name", NAMES)
def test_reference_golden(name, method):
    """The reference's returned triple: decisions and indices on every row the exclusion rule keeps (at most 1 % left out), ratios within 1e-4."""
    recipe, a, b, g = fixture(name)
    mutual = method == "mnn"
    o = device_run(name, method)
    excl = nn_ref.excluded_rows(restated(name, mutual), recipe["threshold"], mutual)
    n_ex, err = nn_ref.compare_with_golden(name, a.shape[1], o["nn0"][0].astype(np.int64), o["ratios0"][0], o["match0"][0].astype(bool), excl,
                                           g[f"{method}/match_indices"], g[f"{method}/good_matches"], g[f"{method}/ratios"], 1e-4)
    print(f"{name} {method}: {n_ex} rows excluded, largest ratio difference {err:.2e}")


@pytest.mark.parametrize("name", NAMES)
def test_default_and_exhaustive_flows_are_bit_identical(name):
    d, e = device_run(name, "mnn"), device_run(name, "mnn", True)
    for k in BITWISE + ("matches1", "nn1"):
        assert d[k].tobytes() == e[k].tobytes(), (name, k)
    n0, n1 = d["nn0"].shape[1], d["nn1"].shape[1]
    assert e["fallback_rows"].tolist() == [n0, n1]


@pytest.mark.parametrize("name", NAMES)
def test_error_bound_of_the_candidate_pass(name):
    """debug = {eps_i, max |s^ - s| over all candidates of the row (measured on the device), s^ of nn1, T}: the a-priori bound holds for every
    candidate, and -- recomputed here in float64 from the inputs alone -- for the nearest neighbour's approximate score; the bound is not vacuous."""
    _, a, b, _ = fixture(name)
    o = device_run(name, "nndr")
    eps, worst, s_nn1, T = o["debug"].T
    assert np.isfinite(eps).all() and (eps > 0).all() and eps.max() < 1e-4
    assert (worst <= eps).all(), float((worst - eps).max())
    a64, b64 = a.T.astype(np.float64), b.T.astype(np.float64)
    near = b64[o["nn0"][0]]
    s = (near * near).sum(1) - 2.0 * (a64 * near).sum(1)
    assert not np.isnan(s_nn1).any()
    err = np.abs(s_nn1.astype(np.float64) - s)
    assert (err <= eps).all(), float((err - eps).max())
    assert (T > s_nn1).all()
    print(f"{name}: eps <= {eps.max():.2e}, largest measured error {worst.max():.2e}")


def crowded_pair():
    """B carries 8 copies of 16 of its rows, perturbed by 1e-7 and stored next to each other: more near-equal columns than one list of 4 keeps,
    so the rows of A that are nearest to them cannot be certified from the lists."""
    a, b = nn_ref.build_fixture(dict(kind="pair", n=1024, seed=1000, noise=0.12, threshold=0.8, twins=0))
    rows = synth.permutation(1000, 79, b.shape[1])[:16]
    copies = np.repeat(b.T[rows].astype(np.float64), 8, axis=0) + 1e-7 * synth.normal(1000, 80, 16 * 8 * 256).reshape(128, 256)
    return a, np.ascontiguousarray(np.concatenate([b, copies.astype(np.float32).T], axis=1))


@pytest.mark.parametrize("method", ["nndr", "mnn"])
def test_exhausted_lists_fall_back_and_stay_exact(method):
    a, b = crowded_pair()
    ref = nn_ref.solve(a, b, 0.8, method == "mnn")
    o = host(baselines.nn_match_pairs([data_of(a, b)], method, 0.8)[0])
    e = host(baselines.nn_match_pairs([data_of(a, b)], method, 0.8, exhaustive=True)[0])
    assert_equals_restatement(o, ref, method == "mnn", "crowded " + method)
    assert 0 < o["fallback_rows"][0] < a.shape[1] // 4, o["fallback_rows"]
    for k in BITWISE:
        assert o[k].tobytes() == e[k].tobytes(), k


def test_exact_duplicates_resolve_to_the_lowest_index():
    """Known answers: identical rows in B tie for a row of A, identical rows in A tie for a row of B."""
    a, b = nn_ref.build_fixture(dict(kind="pair", n=300, seed=12, noise=0.1, threshold=0.8, twins=0))
    a, b = a.copy(), b.copy()
    b[:, 200], b[:, 41], b[:, 77] = b[:, 9], b[:, 9], b[:, 9]          # columns 9, 41, 77, 200 of B are one vector
    a[:, 5] = b[:, 9]                                                  # row 5 of A sits on it: d1 = d2 = 0, ratio 0 / 0 = NaN, no match
    a[:, 250], a[:, 17] = a[:, 100], a[:, 100]                         # rows 17, 100, 250 of A are one vector
    j = int(nn_ref.solve(a, b, 0.8, False)["nn1"][100])
    for exhaustive in (False, True):
        o = host(baselines.nn_match_pairs([data_of(a, b)], "mnn", 0.8, exhaustive=exhaustive)[0])
        assert (o["nn0"][0][5], o["nn0_second"][0][5]) == (9, 41) and o["dist0"][0][5] == 0 and np.isnan(o["ratios0"][0][5])
        assert o["match0"][0][5] == 0 and o["matches0"][0][5] == -1
        assert o["nn0"][0][17] == o["nn0"][0][100] == o["nn0"][0][250] == j and o["nn1"][0][j] not in (100, 250)
        assert o["matches0"][0][100] == -1 and o["matches0"][0][250] == -1          # only the lowest of the three is mutual
        assert_equals_restatement(o, nn_ref.solve(a, b, 0.8, True), True, "duplicates")


def test_other_shapes_against_the_restatement():
    """d = 128 (the fixtures' 128-d half), d = 96, one query row, two data-base rows: the limits of the header."""
    a, b = nn_ref.build_fixture(dict(kind="pair", n=1024, seed=1000, noise=0.16, threshold=0.8, twins=0))
    cases = [(a[:128, :700], b[:128, :450], "mnn"), (a[:96, :130], b[:96, :129], "mnn"), (a[:, :1], b[:, :2], "nndr"), (a[:, :2], b[:, :2], "mnn"),
             (a[:128, :333], b[:128], "nndr")]
    outs = [host(baselines.nn_match_pairs([data_of(np.ascontiguousarray(x), np.ascontiguousarray(y))], m, 0.9)[0]) for x, y, m in cases]
    for (x, y, m), o in zip(cases, outs):
        assert_equals_restatement(o, nn_ref.solve(x, y, 0.9, m == "mnn"), m == "mnn", f"{x.shape} {y.shape} {m}")


@pytest.mark.parametrize("method", ["nndr", "mnn"])
def test_one_batched_call_equals_the_single_calls_and_itself(method):
    datas, thr = [], []
    for name in NAMES:
        recipe, a, b, _ = fixture(name)
        if recipe["threshold"] == 0.8:
            datas.append(data_of(a, b))
            thr.append(name)
    runs = [[host(o) for o in baselines.nn_match_pairs(datas, method, 0.8)] for _ in range(2)]
    keys = BITWISE + (("matches1", "nn1") if method == "mnn" else ())
    for name, first, second in zip(thr, *runs):
        single = device_run(name, method)
        for k in keys + ("fallback_rows",):
            assert first[k].tobytes() == second[k].tobytes(), (name, k)
            assert first[k].tobytes() == single[k].tobytes(), (name, k)


@pytest.mark.parametrize("method", ["nndr", "mnn"])
@pytest.mark.parametrize("name", ["nn_n1024_s1002_d12_t60_k64", "nn_n1024_s1002_d08_t60_k64", "nn_n1500_900_c700_s4001_d16_t80"])
def test_reference_shaped_functions_return_the_reference_shapes(name, method):
    """One match (0-dim indices, ratios of shape (1,)), many, and none (threshold 0.0: shapes (0,)), dtypes and device as documented."""
    recipe, a, b, g = fixture(name)
    fn = baselines.nndr if method == "nndr" else baselines.mnn
    idx, good, ratios = fn(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), recipe["threshold"])
    assert idx.is_cuda and idx.dtype == torch.int64 and good.dtype == torch.int64 and ratios.dtype == torch.float32
    assert tuple(idx.shape) == g[f"{method}/match_indices"].shape and tuple(good.shape) == g[f"{method}/good_matches"].shape
    assert tuple(ratios.shape) == g[f"{method}/ratios"].shape
    ref = restated(name, method == "mnn")
    np.testing.assert_array_equal(np.atleast_1d(idx.cpu().numpy()), np.nonzero(ref["match"])[0])
    np.testing.assert_array_equal(np.atleast_1d(good.cpu().numpy()), ref["nn1"][ref["match"]])
    idx, good, ratios = fn(a, b, 0.0)                                  # NumPy arrays are moved to the current device
    assert idx.is_cuda and tuple(idx.shape) == (0,) and tuple(good.shape) == (0,) and tuple(ratios.shape) == (0,)


def test_end_to_end_into_the_evaluation():
    """nn_match_pairs -> evalh.evaluate_pairs, unchanged: the record's precision and recall equal those computed here from matches0 and the
    reference's stored ground-truth correspondences (eval_gt_n1024_s3001.npz)."""
    g = load_golden("eval_gt_n1024_s3001")
    pair, H = synth.make_homography_pair(1024, 3001, desc_noise=0.12)
    datas = [{k: torch.from_numpy(v).cuda() for k, v in pair.items() if k != "gt_perm"}]
    for method in ("nndr", "mnn"):
        outs = baselines.nn_match_pairs(datas, method, 0.8)
        ev = evalh.evaluate_pairs(datas, outs, [H], ransac_iters=500, seed=5)
        rec = ev["records"].cpu().numpy()[0]
        m0 = outs[0]["matches0"][0].cpu().numpy()
        gt = np.full(1024, -1, np.int64)
        gt[g["ma0"]] = g["ma1"]
        np.testing.assert_array_equal(ev["gt0"][0].cpu().numpy(), gt)
        valid, correct = m0 > -1, (m0[g["ma0"]] == g["ma1"]).sum()
        missed = ((m0 != gt) & (m0 == -1)).sum()
        assert valid.sum() > 500 and rec[0] == valid.sum() and rec[2] == correct
        assert rec[4] == pytest.approx(correct / valid.sum(), abs=1e-6) and rec[5] == pytest.approx(correct / (correct + missed), abs=1e-6)
        assert rec[4] > 0.9 and rec[8] < 1.0, rec                      # descriptors alone recover the planted homography here
