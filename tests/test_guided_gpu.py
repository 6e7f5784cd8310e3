"""Guided matching on the device (GIMS_AUX_GUIDED_MATCH, csrc/nn.hip, through hip.guided_match and gims_amd.guided_match_pairs) against the
float64 restatement (tests/guided_ref.py): indices, masks, added0, matches1, n_admissible and info[2:] exactly, d1 / d2 / ratio within the
1-ulp bar of the gims_nn_match tests.  No row is ever excluded; every fixture's margins are asserted next to the comparison."""
import functools

import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import baselines, hip, synth
from tests import fundamental_ref as FR
from tests import guided_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
PAD, FILL = 8, 0xA5
INT_OUT = ("nn1", "nn2", "n_admissible", "matches0", "added0")
OUT = tuple(n for n, _ in hip.GUIDED_OUTPUTS)


def assert_ulp(got, want, what):
    """The bar of the gims_nn_match tests for d1, d2 and the ratio: NaN where the restatement has NaN, else within 1 float32 ulp."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.array_equal(np.isinf(got[ok]), np.isinf(want[ok])), what
    fin = ok & np.isfinite(want)
    tol = np.spacing(np.maximum(np.abs(got[fin]), np.abs(want[fin])))
    worst = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)) - tol
    assert (worst <= 0).all(), f"{what}: {int((worst > 0).sum())} values differ by more than 1 ulp"


# ------------------------------------------------------------------------------------------------ scenes
def unit_F(config="general"):
    F = FR.planted_F(config)
    return (F / np.linalg.norm(F)).astype(F32).reshape(9)


@functools.lru_cache(maxsize=None)
def scene(n0, n1, d, kind, seed=0, noise=0.5, sigma=0.03, crowd=0):
    """n0 x n1 keypoints under a planted model: row i < min(n0, n1) has its partner at column perm[i] (position noise `noise` px, descriptor
    noise sigma), the other columns are random.  crowd: the first `crowd` partners are each followed by 16 near-copies (1e-7) of their
    descriptor at the same place, stored side by side: more equal admissible columns than a list keeps."""
    rng = np.random.default_rng(4000 + 7 * n0 + 13 * n1 + d + 1000 * kind + 100003 * seed)
    m = max(n0, n1)
    w, h = FR.CANVAS
    if kind == R.FUNDAMENTAL:
        a, b = FR.project_pair("general", m, rng)
        model = unit_F()
    else:
        model = np.asarray(synth.make_homography(11 + seed, FR.CANVAS), F32).reshape(9)
        a = rng.random((m, 2)) * [w, h]
        q = np.concatenate([a, np.ones((m, 1))], 1) @ model.astype(np.float64).reshape(3, 3).T
        b = q[:, :2] / q[:, 2:3]
    b = b + noise * rng.standard_normal((m, 2))
    k = min(n0, n1 - 16 * crowd)
    assert k >= crowd
    perm = rng.permutation(n1 - 16 * crowd)
    kp0 = a[:n0].astype(F32)
    kp1 = (rng.random((n1, 2)) * [w, h]).astype(F32)
    kp1[perm[:k]] = b[:k].astype(F32)
    A, B = R.unit_rows(rng, n0, d), R.unit_rows(rng, n1, d)
    B[perm[:k]] = R.noisy(rng, A[:k], sigma)
    for c in range(crowd):
        lo = n1 - 16 * (crowd - c)
        B[lo:lo + 16] = (B[perm[c]].astype(np.float64) + 1e-7 * rng.standard_normal((16, d))).astype(F32)
        kp1[lo:lo + 16] = kp1[perm[c]]
    gt = -np.ones(n0, np.int64)
    gt[:k] = perm[:k]
    return dict(A=A, B=B, kp0=kp0, kp1=kp1, model=model, kind=kind, gt=gt)


def case(sc, **kw):
    c = dict(sc, ok=None, prior=None, mask=None, scores=None, thresh=3.0, ratio=0.8, max_distance=None, mutual=True)
    c.update(kw)
    return c


def restate(c):
    return R.solve(c["A"], c["B"], c["kp0"], c["kp1"], c["model"], c["kind"], ok=c["ok"], prior=c["prior"], mask=c["mask"], scores=c["scores"],
                   thresh=c["thresh"], ratio=c["ratio"], max_distance=c["max_distance"], mutual=c["mutual"])


# ------------------------------------------------------------------------------------------------ the device side
def _filled(n, dtype):
    t = torch.empty(n + PAD, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(FILL)
    return t


def device_items(cases):
    """The op's items for a list of cases: every output in a buffer of its own, PAD elements longer than needed and pre-filled with 0xA5."""
    cu = lambda x, dt=None: None if x is None else torch.from_numpy(np.ascontiguousarray(x if dt is None else np.asarray(x, dt))).cuda()      # noqa: E731
    items = []
    for c in cases:
        n0, n1 = len(c["A"]), len(c["B"])
        it = dict(a=cu(c["A"]), b=cu(c["B"]), kpts0=cu(c["kp0"]), kpts1=cu(c["kp1"]), model=cu(c["model"], F32), kind=c["kind"],
                  ok=cu(np.array([c["ok"]], F32)) if c["ok"] is not None else None, prior=cu(c["prior"], np.int64), prior_mask=cu(c["mask"], np.uint8),
                  prior_scores=cu(c["scores"], F32), mutual=c["mutual"], thresh=c["thresh"], threshold=c["ratio"], max_distance=c["max_distance"],
                  info=_filled(8, torch.int32))
        for name, dt in hip.GUIDED_OUTPUTS:
            it[name] = _filled(n0, dt)
        if c["mutual"]:
            it["cnn1"], it["matches1"] = _filled(n1, torch.int32), _filled(n1, torch.int64)
        items.append(it)
    return items


def _names(it):
    return OUT + ("info",) + (("cnn1", "matches1") if it["mutual"] else ())


def read_back(items):
    """Host copies of the outputs, after checking that the padding behind every one of them still holds 0xA5."""
    torch.cuda.synchronize()
    outs = []
    for it in items:
        n0, n1 = it["a"].shape[0], it["b"].shape[0]
        o = {}
        for name in _names(it):
            n = 8 if name == "info" else (n1 if name in ("cnn1", "matches1") else n0)
            t = it[name]
            assert (t[n:].view(torch.uint8) == FILL).all(), f"{name}: the call wrote behind its {n} elements"
            o[name] = t[:n].cpu().numpy()
        outs.append(o)
    return outs


def run(cases, flags=0):
    items = device_items(cases)
    keep = hip.guided_match(items, flags)
    outs = read_back(items)
    del keep
    return outs


def compare(o, ref, c, what):
    mutual = c["mutual"]
    for k in INT_OUT + (("cnn1", "matches1") if mutual else ()):
        np.testing.assert_array_equal(o[k], ref[k], err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(o["info"][2:], ref["info"][2:], err_msg=f"{what}: info")
    for k in ("d1", "d2", "ratio"):
        assert_ulp(o[k], ref[k], f"{what} {k}")
    fixed, added = ref["fixed"], ref["added0"] != 0
    want = np.where(fixed, ref["scores0"], np.where(added, F32(1) - o["ratio"], F32(0))).astype(F32)
    np.testing.assert_array_equal(o["scores0"], want, err_msg=f"{what}: scores0")
    near, ulps = R.margins(ref, c["ratio"], c["max_distance"])
    assert near > 1e-6 and ulps > 1.0, f"{what}: the fixture sits on a decision's edge ({near}, {ulps}): reseed it"


def check(cases, what, fallback=None):
    """Default and exhaustive flows against the restatement and bit-identical to each other; -> (outputs, restatements)."""
    refs = [restate(c) for c in cases]
    d, e = run(cases), run(cases, hip.NN_EXHAUSTIVE)
    for p, (c, ref) in enumerate(zip(cases, refs)):
        compare(d[p], ref, c, f"{what} [{p}]")
        for k in d[p]:
            if k != "info":
                assert d[p][k].tobytes() == e[p][k].tobytes(), f"{what} [{p}]: {k} differs between the default and the exhaustive flow"
        assert d[p]["info"][2:].tolist() == e[p]["info"][2:].tolist()
        assert e[p]["info"][:2].tolist() == [len(c["A"]), len(c["B"]) if c["mutual"] else 0]
        assert 0 <= d[p]["info"][0] <= len(c["A"]) and 0 <= d[p]["info"][1] <= len(c["B"])
        if fallback is not None:
            assert (d[p]["info"][0] > 0) == fallback, d[p]["info"]
    return d, refs


# ------------------------------------------------------------------------------------------------ shapes, kinds, flows
SHAPES = [(1, 1, 32), (1, 2, 128), (2, 1, 32), (3, 300, 256), (127, 129, 128), (128, 128, 32), (129, 127, 256), (300, 3, 128), (300, 300, 128),
          (128, 1, 128), (300, 129, 32), (2, 2, 256)]


@pytest.mark.parametrize("mutual", [True, False])
@pytest.mark.parametrize("kind", [R.FUNDAMENTAL, R.HOMOGRAPHY])
@pytest.mark.parametrize("n0, n1, d", SHAPES)
def test_shapes_against_the_restatement(n0, n1, d, kind, mutual):
    thresh = 3.0 if kind == R.FUNDAMENTAL else 25.0                         # a band and a disc that both hold a handful of keypoints
    check([case(scene(n0, n1, d, kind), mutual=mutual, thresh=thresh)], f"{n0} x {n1} x {d} kind {kind} mutual {mutual}")


@pytest.mark.parametrize("kind, thresh", [(R.FUNDAMENTAL, 8.0), (R.HOMOGRAPHY, 60.0)])
def test_rows_with_none_one_two_and_many_admissible_columns(kind, thresh):
    c = case(scene(300, 129, 128, kind), thresh=thresh)                      # 171 rows without a partner: what they can reach is chance
    _, (ref,) = check([c], f"kind {kind}")
    hist = np.bincount(np.minimum(ref["n_admissible"], 5), minlength=6)
    assert (hist[[0, 1, 2, 5]] > 0).all(), hist                             # 0, 1, 2 and 5 or more: each occurs
    assert ref["info"][6] > 50


@pytest.mark.parametrize("kind", [R.FUNDAMENTAL, R.HOMOGRAPHY])
def test_short_lists_certify_without_the_inequality(kind):
    """Every row has at most one admissible column (exact partners, a gate of 0.002 px): every list is short, nothing goes to the fallback."""
    c = case(scene(300, 300, 128, kind, noise=0.0), thresh=0.002)
    (o,), (ref,) = check([c], f"kind {kind}")
    assert ref["n_admissible"].max() == 1 and (ref["n_admissible"] == 1).sum() > 250
    assert o["info"][:2].tolist() == [0, 0]
    assert (o["nn2"] == -1).all() and np.isinf(o["d2"]).all()
    assert (o["ratio"][ref["n_admissible"] == 1] == 0).all() and np.isnan(o["ratio"][ref["n_admissible"] == 0]).all()
    assert ref["info"][6] == (ref["n_admissible"] == 1).sum()               # ratio 0 passes every threshold: each of them is matched


@pytest.mark.parametrize("mutual", [True, False])
def test_near_copies_side_by_side_take_the_fallback(mutual):
    c = case(scene(300, 300, 128, R.FUNDAMENTAL, crowd=4), mutual=mutual)
    (o,), (ref,) = check([c], "crowded", fallback=True)
    assert (ref["n_admissible"][:4] >= 17).all() and not ref["added0"][:4].any()      # 17 equal partners: the ratio test refuses them


# ------------------------------------------------------------------------------------------------ priors
def _prior_cases():
    sc = scene(300, 129, 128, R.FUNDAMENTAL)
    n0, n1, gt = 300, 129, sc["gt"]
    rng = np.random.default_rng(5)
    scores = (rng.random(n0) * 0.5 + 0.25).astype(F32)
    every = -np.ones(n0, np.int64)
    every[:n1] = rng.permutation(n1)
    dup = gt.copy()
    dup[200:210] = gt[0:10]                                                # ten columns claimed twice: the lower row keeps each
    dup[250] = gt[3]                                                       # ... and one three times
    out = gt.copy()
    out[5], out[6], out[7], out[8] = n1, -7, 1 << 40, -(1 << 33)
    mask = (rng.random(n0) < 0.5).astype(np.uint8)
    return sc, [("all fixed (n0 = 129)", dict(A=sc["A"][:129], kp0=sc["kp0"][:129], prior=every[:129], scores=scores[:129])),
                ("every column taken", dict(prior=every)), ("none fixed", dict(prior=-np.ones(n0, np.int64))),
                ("the ground truth, with scores", dict(prior=gt, scores=scores)), ("duplicate claims", dict(prior=dup, scores=scores)),
                ("priors outside the image", dict(prior=out)), ("a mask that frees rows", dict(prior=dup, mask=mask)),
                ("a mask of zeros", dict(prior=gt, mask=np.zeros(n0, np.uint8))), ("a mask without a prior", dict(mask=mask))]


@pytest.mark.parametrize("k", range(9))
def test_priors(k):
    sc, cases = _prior_cases()
    name, kw = cases[k]
    c = case(sc, **kw)
    (o,), (ref,) = check([c], name)
    n_fixed, n_bad, n_dup = (int(v) for v in o["info"][2:5])
    want = {0: (129, 0, 0), 1: (129, 0, 0), 2: (0, 0, 0), 5: (125, 4, 0), 7: (0, 0, 0), 8: (0, 0, 0)}
    if k in want:
        assert (n_fixed, n_bad, n_dup) == want[k], (name, o["info"])
    if k == 0:
        assert o["info"][6] == 0 and (o["matches0"] == c["prior"]).all() and (o["scores0"] == c["scores"]).all() and not o["added0"].any()
    if k == 1:
        assert o["info"][6] == 0 and (o["n_admissible"] == 0).all() and (o["scores0"][c["prior"] >= 0] == 1).all()
    if k == 4:
        assert n_dup == 11 and (o["matches0"][:10] == c["prior"][:10]).all()
    m0 = o["matches0"]
    rows = np.nonzero(m0 >= 0)[0]
    assert len(np.unique(m0[rows])) == len(rows) and (o["matches1"][m0[rows]] == rows).all()      # one-to-one, fixed rows included


# ------------------------------------------------------------------------------------------------ models
def test_a_pair_without_a_model_keeps_its_fixed_rows_only():
    sc = scene(300, 129, 128, R.FUNDAMENTAL)
    nan_model = sc["model"].copy()
    nan_model[4] = np.nan
    inf_model = sc["model"].copy()
    inf_model[8] = np.inf
    mask = (np.arange(300) % 3 == 0).astype(np.uint8)
    cases = [case(sc, ok=0.0, prior=sc["gt"], mask=mask), case(sc, model=nan_model, prior=sc["gt"], mask=mask), case(sc, model=inf_model),
             case(sc, ok=1.0, prior=sc["gt"], mask=mask), case(sc, ok=-2.5), case(sc, ok=0.0, kind=R.HOMOGRAPHY, mutual=False)]
    outs, refs = check(cases, "no model")
    for p in (0, 1, 2, 5):
        o = outs[p]
        assert o["info"][5] == 1 and o["info"][6] == 0 and (o["n_admissible"] == 0).all() and not o["added0"].any()
        fixed = refs[p]["fixed"]
        assert (o["matches0"][fixed] == sc["gt"][fixed]).all() and (o["matches0"][~fixed] == -1).all() and o["info"][2] == fixed.sum()
    assert outs[0]["info"][2] == 43 and outs[2]["info"][2] == 0
    assert outs[3]["info"][5] == 0 == outs[4]["info"][5] and outs[3]["info"][6] > 0 and outs[4]["info"][6] > 0


def test_a_homography_with_rows_on_its_lines_at_infinity():
    """pw = 1 - u / 1024 is exactly 0 at u = 1024, and the cofactors' qw = 1 + u' / 1024 at u' = -1024: those rows are not valid."""
    sc = dict(scene(129, 128, 128, R.HOMOGRAPHY))
    H = np.array([1, 0, 5, 0, 1, -3, -2.0 ** -10, 0, 1], F32)
    kp0, kp1 = sc["kp0"].copy(), sc["kp1"].copy()
    Hm = H.astype(np.float64).reshape(3, 3)
    q = np.concatenate([kp0.astype(np.float64), np.ones((129, 1))], 1) @ Hm.T
    kp1[sc["gt"][sc["gt"] >= 0]] = (q[:, :2] / q[:, 2:3])[sc["gt"] >= 0].astype(F32)
    kp0[[7, 100]] = [[1024.0, 50.0], [1024.0, 300.0]]
    kp1[[3, 90]] = [[-1024.0, 10.0], [-1024.0, 580.0]]
    sc.update(kp0=kp0, kp1=kp1, model=H)
    (o,), (ref,) = check([case(sc, thresh=2.0)], "line at infinity")
    wa, wb = R.row_words(R.HOMOGRAPHY, H, kp0, kp1)
    assert np.isnan(wa[[7, 100]]).all() and np.isnan(wb[[3, 90]]).all() and np.isfinite(np.delete(wa, [7, 100], 0)).all()
    assert (o["n_admissible"][[7, 100]] == 0).all() and (o["cnn1"][[3, 90]] == -1).all() and o["info"][6] > 90


def test_a_fundamental_matrix_whose_epipole_is_a_keypoint():
    """F = [e]x / 512 with e = (400, 300, 1): exact in float32, F e = 0 = F^T e, so g = 0 for a keypoint of image 0 at e and h = 0 for one of
    image 1: neither has an epipolar line, neither is admissible for anybody."""
    sc = dict(scene(129, 128, 128, R.FUNDAMENTAL))
    F = (np.array([0, -1, 300, 1, 0, -400, -300, 400, 0], np.float64) / 512).astype(F32)
    e = np.array([400.0, 300.0])
    rng = np.random.default_rng(8)
    kp0 = sc["kp0"].copy()
    kp1 = (rng.random((128, 2)) * FR.CANVAS).astype(F32)
    has = sc["gt"] >= 0
    kp1[sc["gt"][has]] = (e + (kp0[has].astype(np.float64) - e) * (1.1 + 0.4 * rng.random((int(has.sum()), 1)))).astype(F32)      # along the ray through e
    kp0[11], kp1[17] = e, e
    sc.update(kp0=kp0, kp1=kp1, model=F)
    (o,), (ref,) = check([case(sc, thresh=1.0)], "epipole")
    wa, wb = R.row_words(R.FUNDAMENTAL, F, kp0, kp1)
    assert wa[11, 3] == 0 and wb[17, 3] == 0 and (np.delete(wa[:, 3], 11) > 0).all()
    assert o["n_admissible"][11] == 0 and o["nn1"][11] == -1 and o["cnn1"][17] == -1 and not (o["nn1"] == 17).any() and o["info"][6] > 80


# ------------------------------------------------------------------------------------------------ against the plain matcher, batches, replays
@pytest.mark.parametrize("mutual", [True, False])
def test_a_gate_that_admits_everything_is_nn_match_pairs_bit_for_bit(mutual):
    sc = scene(300, 129, 128, R.FUNDAMENTAL)
    c = case(sc, thresh=1e9, mutual=mutual)
    (o,) = run([c])
    assert (o["n_admissible"] == 129).all()
    data = dict(descriptors0=torch.from_numpy(np.ascontiguousarray(sc["A"].T))[None].cuda(), descriptors1=torch.from_numpy(np.ascontiguousarray(sc["B"].T))[None].cuda())
    nn = baselines.nn_match_pairs([data], "mnn" if mutual else "nndr", 0.8)[0]
    torch.cuda.synchronize()
    pairs = [("nn1", "nn0"), ("nn2", "nn0_second"), ("d1", "dist0"), ("d2", "dist0_second"), ("ratio", "ratios0"), ("matches0", "matches0"),
             ("scores0", "matching_scores0"), ("added0", "match0")] + ([("cnn1", "nn1"), ("matches1", "matches1")] if mutual else [])
    for mine, theirs in pairs:
        assert o[mine].tobytes() == nn[theirs][0].cpu().numpy().tobytes(), mine
    assert o["info"][2:].tolist() == [0, 0, 0, 0, int(o["added0"].sum()), 0] and o["added0"].sum() > 100


def test_three_pairs_in_one_call_equal_the_same_pairs_alone():
    cases = [case(scene(300, 129, 128, R.FUNDAMENTAL), prior=scene(300, 129, 128, R.FUNDAMENTAL)["gt"], mask=(np.arange(300) % 2).astype(np.uint8)),
             case(scene(3, 300, 256, R.HOMOGRAPHY), thresh=25.0, mutual=False, max_distance=0.6),
             case(scene(129, 127, 256, R.FUNDAMENTAL, crowd=2), ratio=0.9)]
    together, refs = check(cases, "three pairs")
    for p, c in enumerate(cases):
        (alone,) = run([c])
        for k in alone:
            if k != "info":
                assert alone[k].tobytes() == together[p][k].tobytes(), (p, k)
        assert alone["info"][2:].tolist() == together[p]["info"][2:].tolist()


def _bytes(items):
    torch.cuda.current_stream().synchronize()
    return {(p, k): it[k].cpu().numpy().tobytes() for p, it in enumerate(items) for k in _names(it)}


def test_two_runs_and_a_captured_graph_are_byte_identical():
    cases = [case(scene(300, 300, 128, R.FUNDAMENTAL, crowd=4), prior=scene(300, 300, 128, R.FUNDAMENTAL, crowd=4)["gt"],
                  mask=(np.arange(300) % 4 == 0).astype(np.uint8)), case(scene(127, 129, 128, R.HOMOGRAPHY), thresh=25.0, mutual=False)]
    refs = [restate(c) for c in cases]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        items = device_items(cases)
        rows = [dict(it, lda=128, ldb=128, n0=it["a"].shape[0], n1=it["b"].shape[0], d=128, reserved=0) for it in items]
        need = hip.guided_layout([(r["n0"], r["n1"], r["mutual"]) for r in rows])["bytes"]
        work = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
        work.fill_(FILL)
        tab = hip.guided_table(rows)
        ops = hip.make_ops([hip.op_guided_match(tab, work, need)])
        hip.run_ops(ops)
        first = _bytes(items)
        for p, o in enumerate(read_back(items)):
            compare(o, refs[p], cases[p], f"run 1 [{p}]")
        assert (work[need:] == FILL).all()                                  # the workspace formula covers what the call writes
        hip.run_ops(ops)
        assert _bytes(items) == first
        graph = hip.OpsGraph(ops)
        for _ in range(2):
            for it in items:
                for k in _names(it):
                    it[k].view(torch.uint8).fill_(FILL)
            work.fill_(FILL)
            graph.launch()
            assert _bytes(items) == first
            read_back(items)
    torch.cuda.current_stream().wait_stream(side)


def test_refused_calls_leave_the_buffers_alone():
    cases = [case(scene(127, 129, 128, R.FUNDAMENTAL))]
    items = device_items(cases)
    rows = [dict(it, lda=128, ldb=128, n0=127, n1=129, d=128, reserved=0) for it in items]
    need = hip.guided_layout([(127, 129, True)])["bytes"]
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    work.fill_(FILL)
    before = _bytes(items)
    for bad, word in ((dict(work_bytes=need - 1), "work_bytes"), (dict(thresh=float("nan")), "thresh"), (dict(kind=3), "unknown kind"),
                      (dict(reserved=1), "reserved"), (dict(n_admissible=None), "null pointer")):
        r = [dict(rows[0], **{k: v for k, v in bad.items() if k != "work_bytes"})]
        with pytest.raises(hip.GimsHipError, match=word):
            hip.run_ops(hip.make_ops([hip.op_guided_match(hip.guided_table(r), work, bad.get("work_bytes", need))]))
    torch.cuda.synchronize()
    assert _bytes(items) == before and (work == FILL).all()


# ------------------------------------------------------------------------------------------------ the Python layer
def _count_syncs(monkeypatch):
    counts = {"device": 0, "stream": 0, "event": 0}
    for name, owner, attr in (("device", torch.cuda, "synchronize"), ("stream", torch.cuda.Stream, "synchronize"), ("event", torch.cuda.Event, "synchronize")):
        orig = getattr(owner, attr)

        def counted(*a, _orig=orig, _name=name, **kw):
            counts[_name] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(owner, attr, counted)
    return counts


def _layer_inputs(scs, priors, oks, inliers):
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()        # noqa: E731
    datas = [dict(descriptors0=cu(s["A"].T)[None], descriptors1=cu(s["B"].T)[None], keypoints0=cu(s["kp0"])[None], keypoints1=cu(s["kp1"])[None])
             for s in scs]
    outs = [dict(matches0=cu(p)[None], matching_scores0=cu(np.full(len(p), 0.75, F32))[None]) for p in priors]
    records = torch.zeros(len(scs), 8, device="cuda")
    records[:, gims_amd.verify.RECORD_FIELDS.index("ok")] = torch.tensor(oks, device="cuda")
    verified = dict(models=cu(np.stack([s["model"].reshape(3, 3) for s in scs])), records=records, inlier=[cu(m) for m in inliers])
    return datas, outs, verified


def test_the_python_layer_equals_the_restatement_without_a_synchronisation(monkeypatch):
    scs = [scene(300, 129, 128, R.FUNDAMENTAL), scene(127, 129, 128, R.HOMOGRAPHY), scene(129, 127, 256, R.FUNDAMENTAL)]
    priors = [s["gt"].copy() for s in scs]
    priors[0][::5] = -1
    inliers = [(np.arange(len(p)) % 3 != 0).astype(np.uint8) for p in priors]
    datas, outs, verified = _layer_inputs(scs, priors, [1.0, 1.0, 0.0], inliers)
    models = ["fundamental", "homography", "fundamental"]
    torch.cuda.synchronize()
    counts = _count_syncs(monkeypatch)
    got = {keep: gims_amd.guided_match_pairs(datas, outs, verified, model=models, thresh=4.0, ratio=0.85, max_distance=0.7, keep=keep)
           for keep in ("inliers", "all", "none")}
    nopr = gims_amd.guided_match_pairs(datas, None, verified, model=models, thresh=4.0, ratio=0.85, max_distance=0.7, mutual=False, exhaustive=True)

    class Feat:
        def __init__(self, desc, kpts):
            self.descriptors, self.keypoints, self.n = desc, kpts, desc.shape[0]
    feats = [Feat(datas[0]["descriptors0"][0].t().contiguous(), datas[0]["keypoints0"][0]), Feat(datas[0]["descriptors1"][0].t().contiguous(), datas[0]["keypoints1"][0])]
    one = {k: (v[:1] if k != "inlier" else v[:1]) for k, v in verified.items()}
    byfeat = gims_amd.guided_match_features(feats, [(0, 1)], outs[:1], one, model="fundamental", thresh=4.0, ratio=0.85, max_distance=0.7)
    assert counts == {"device": 0, "stream": 0, "event": 0}, counts
    monkeypatch.undo()
    torch.cuda.synchronize()
    names = dict(matches0="matches0", added0="added0", nn0="nn1", nn0_second="nn2", n_admissible0="n_admissible", matches1="matches1")
    for keep, res in list(got.items()) + [("nopr", nopr)]:
        for p, s in enumerate(scs):
            kw = dict(ok=[1.0, 1.0, 0.0][p], thresh=4.0, ratio=0.85, max_distance=0.7, mutual=keep != "nopr")
            if keep in ("inliers", "all"):
                kw.update(prior=priors[p], scores=np.full(len(priors[p]), 0.75, F32), mask=inliers[p] if keep == "inliers" else None)
            ref = R.solve(s["A"], s["B"], s["kp0"], s["kp1"], s["model"], s["kind"], **kw)
            o = {k: v.cpu().numpy() for k, v in res[p].items() if not k.startswith("_")}
            for mine, theirs in names.items():
                if mine != "matches1" or keep != "nopr":
                    assert o[mine].shape[0] == 1
                    np.testing.assert_array_equal(o[mine][0], ref[theirs], err_msg=f"{keep} [{p}] {mine}")
            np.testing.assert_array_equal(o["info"][2:], ref["info"][2:])
            for mine, theirs in (("dist0", "d1"), ("dist0_second", "d2"), ("ratios0", "ratio")):
                assert_ulp(o[mine][0], ref[theirs], f"{keep} [{p}] {mine}")
            assert (o["matching_scores0"][0][ref["fixed"]] == 0.75).all() and o["model"].tobytes() == s["model"].tobytes()
            if p == 2:
                assert o["info"][5] == 1 and o["info"][6] == 0
    for k in ("matches0", "added0", "matches1", "nn0", "dist0", "ratios0", "n_admissible0", "matching_scores0"):
        assert byfeat[0][k].cpu().numpy().tobytes() == got["inliers"][0][k].cpu().numpy().tobytes(), k
    assert int(got["inliers"][0]["info"][6]) > 0 and int(got["none"][0]["info"][2]) == 0


def test_pose_goes_through_the_fundamental_matrix_formed_on_the_device():
    sc = scene(300, 129, 128, R.FUNDAMENTAL)
    Kmat, Rm, t = FR.cameras("general")
    K1 = Kmat.copy()
    K1[0, 0], K1[1, 1], K1[0, 2] = 650.0, 660.0, 390.0                      # the fixture's F in other clothes: E = K1^T F K0 for a second camera K1
    E = K1.T @ sc["model"].astype(np.float64).reshape(3, 3) @ Kmat
    scale = np.linalg.norm(E)
    Ef = (E / scale).astype(F32)
    datas, outs, verified = _layer_inputs([dict(sc, model=Ef.reshape(9))], [sc["gt"]], [1.0], [np.ones(300, np.uint8)])
    res = gims_amd.guided_match_pairs(datas, outs, verified, model="pose", intrinsics=(Kmat, K1), keep="none")[0]
    torch.cuda.synchronize()
    Fdev = res["model"].cpu().numpy()
    want = np.linalg.inv(K1).T @ Ef.astype(np.float64) @ np.linalg.inv(Kmat)
    np.testing.assert_allclose(Fdev.reshape(3, 3), want, rtol=0, atol=2e-7 * np.abs(want).max())
    np.testing.assert_allclose(Fdev * scale, sc["model"], rtol=0, atol=1e-5 * np.abs(sc["model"]).max())
    ref = R.solve(sc["A"], sc["B"], sc["kp0"], sc["kp1"], Fdev, R.FUNDAMENTAL, ok=1.0)
    for mine, theirs in (("matches0", "matches0"), ("nn0", "nn1"), ("nn0_second", "nn2"), ("n_admissible0", "n_admissible"), ("matches1", "matches1")):
        np.testing.assert_array_equal(res[mine][0].cpu().numpy(), ref[theirs], err_msg=mine)
    assert int(res["info"][6]) == ref["info"][6] > 50


def test_the_result_feeds_build_tracks_and_verify_pairs():
    sc = scene(300, 300, 128, R.FUNDAMENTAL)
    prior = sc["gt"].copy()
    prior[1::2] = -1                                                        # the matcher found every second pair
    datas, outs, _ = _layer_inputs([sc], [prior], [1.0], [np.ones(300, np.uint8)])
    verified = gims_amd.verify_pairs(datas, outs, model="fundamental", thresh=3.0)
    refill = gims_amd.guided_match_pairs(datas, outs, verified, model="fundamental")
    again = gims_amd.verify_pairs(datas, refill, model="fundamental", thresh=3.0)
    tracks = gims_amd.build_tracks([300, 300], [(0, 1)], refill, inlier=again)
    before = gims_amd.build_tracks([300, 300], [(0, 1)], outs, inlier=verified)
    torch.cuda.synchronize()
    ok = gims_amd.verify.RECORD_FIELDS.index("ok")
    n_in = gims_amd.verify.RECORD_FIELDS.index("n_inliers")
    assert float(verified["records"][0, ok]) == 1.0 == float(again["records"][0, ok])
    m0 = refill[0]["matches0"][0].cpu().numpy()
    kept = verified["inlier"][0].cpu().numpy() != 0
    assert (m0[kept] == prior[kept]).all() and int(refill[0]["info"][2]) == kept.sum() and int(refill[0]["info"][6]) > 50
    assert float(again["records"][0, n_in]) > float(verified["records"][0, n_in]) + 50
    assert tracks.n_tracks > before.n_tracks + 50 and tracks.n_obs == 2 * tracks.n_tracks
