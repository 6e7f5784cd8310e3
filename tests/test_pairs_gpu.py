"""GPU tests of the pair selection (GIMS_AUX_SELECT_PAIRS, gims_amd/csrc/pairs.hip) against tests/pairs_ref.py.  Every decision of the op is
an integer one, so the pass condition of every case is equality: votes, pairs, pair_votes and the counters are the restatement's, the
entries of the output buffer behind n_pairs and its padding keep what they held, and a second run and a captured graph give the same bytes.

The shapes walk the seams of the kernels: an image fills whole blocks of 32 pooled rows (m = 31, 32, 33), a query tile is four blocks (127,
128, 129; several small images in one tile; an image across two), the database loop of an image runs 8 steps and one more (255, 256, 257),
every instance of the vote kernel (D = 32 .. 1024, and a D between two powers of two), and more images than one pass of the scan takes."""
import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import pairs_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FILL, PAD = -0x5A5A5A5B, 64                                        # the bytes 0xA5 as an int32


def scene(ms, d, seed, noise=0.3):
    """Images of ms rows each, drawn from one world of unit descriptors with noise (of that length): neighbours exist, so votes do."""
    rng = np.random.default_rng(seed)
    world = rng.standard_normal((max(8, 2 * max(ms)), d))
    world /= np.linalg.norm(world, axis=1, keepdims=True)
    return [(world[rng.permutation(len(world))[:m]] + noise / np.sqrt(d) * rng.standard_normal((m, d))).astype(np.float32) for m in ms]


def _device(descs, rows):
    keep, images = [], []
    for i, x in enumerate(descs):
        t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        r = None if rows is None or rows[i] is None else torch.from_numpy(np.asarray(rows[i], np.int32)).cuda()
        keep += [t, r]
        images.append((t if len(x) else None, x.shape[1], len(x), r, None if r is None else len(rows[i])))
    return images, keep


def device_run(descs, rows=None, k=20, per_image=512, ratio=0.8, min_votes=1, scale=None):
    """hip.select_pairs into a buffer of 0xA5 with padding behind it -> (votes, the whole buffer, counters) on the host."""
    images, keep = _device(descs, rows)
    images = [(t, ld, n, r, min(n, per_image) if m is None else m) for t, ld, n, r, m in images]
    words = hip.pairs_out_layout(len(descs), k)[2]
    out = torch.full((words + PAD,), FILL, dtype=torch.int32, device="cuda")
    votes, out, counters, alive = hip.select_pairs(images, descs[0].shape[1], "cuda", k, per_image, hip.pairs_rq(ratio), min_votes, scale, out=out)
    torch.cuda.synchronize()
    return votes.cpu().numpy(), out.cpu().numpy(), counters.cpu().numpy()


def check(descs, rows=None, **kw):
    """One case: the device against the restatement, exactly.  -> the restatement's result."""
    want = R.run(descs, rows=rows, **kw)
    votes, out, counters = device_run(descs, rows=rows, **kw)
    np.testing.assert_array_equal(votes, want["votes"], err_msg="votes")
    assert dict(zip(R.COUNTERS, counters[:5].tolist())) == want["counters"] and not counters[5:].any(), (counters, want["counters"])
    n_pairs = len(want["pairs"])
    _, o_votes, words, cap = hip.pairs_out_layout(len(descs), kw.get("k", 20))
    assert n_pairs <= cap
    np.testing.assert_array_equal(out[:2 * n_pairs].reshape(-1, 2), want["pairs"], err_msg="pairs")
    np.testing.assert_array_equal(out[o_votes:o_votes + n_pairs], want["pair_votes"], err_msg="pair_votes")
    assert (out[2 * n_pairs:o_votes] == FILL).all() and (out[o_votes + n_pairs:] == FILL).all(), "an entry behind n_pairs or the padding was written"
    return want


def test_ring_fixture():
    descs = R.ring_scene()
    a = check(descs, k=2)
    assert a["counters"]["n_pairs"] == 12 and (a["pair_votes"] == 112).all()
    b = check(descs, k=4)
    assert b["counters"]["n_pairs"] == 24 and sorted(set(b["pair_votes"].tolist())) == [32, 112]


@pytest.mark.parametrize("ms, d", [([40, 50], 128), ([20, 33, 64], 128), ([0, 1, 2, 40, 1, 0, 2, 35], 64), ([31, 32, 33, 127, 128, 129], 64),
                                   ([255, 256, 257], 32), ([5, 9, 3, 7, 20, 11, 2, 30, 4], 32), ([96, 64, 10, 70], 32), ([2, 2], 32), ([0, 0, 0], 32),
                                   ([1, 0], 32)])
def test_row_counts(ms, d):
    want = check(scene(ms, d, seed=len(ms) + d), k=3, min_votes=1)
    assert want["counters"]["n_short_images"] == sum(m < 2 for m in ms)
    if min(ms) >= 20:
        assert want["votes"].sum() > 0                             # (not a vacuous case)


@pytest.mark.parametrize("d", [32, 64, 96, 128, 256, 544, 1024])
def test_channel_counts(d):
    want = check(scene([40, 33, 50], d, seed=d), k=2)
    assert want["votes"].sum() > 0


@pytest.mark.parametrize("d", [32, 128, 256])
def test_operand_map_with_asymmetric_integers(d):
    """Integer-valued data with scale = 1: Q is the data.  Every row and every channel differ in magnitude, so a swapped operand, a
    transposed tile or a misplaced accumulator row changes the votes."""
    rng = np.random.default_rng(d)
    base = rng.integers(-127, 128, size=(90, d)) // (1 + (np.arange(90) % 4)[:, None])
    base[:, ::3] //= 2
    descs = []
    for m in (70, 33, 64, 45):
        x = base[rng.permutation(90)[:m]] + rng.integers(-2, 3, size=(m, d))
        descs.append(np.clip(x, -127, 127).astype(np.float32))
    want = check(descs, k=2, scale=1.0, ratio=0.9)
    assert all((q == x).all() for q, x in zip(want["q"], descs)) and want["votes"].sum() > 0


def test_duplicates_and_identical_images():
    descs = scene([40, 40, 30], 64, seed=5)
    descs[0][7] = descs[0][3]                                      # a duplicate inside image 0: whoever matches it has d1 = d2
    descs[1] = descs[0].copy()                                     # two identical images: d1 = 0 for every row, and the duplicate rows do not vote
    want = check(descs, k=2)
    assert want["votes"][0, 1] == want["votes"][1, 0] == 38


def test_saturation_nonfinite_and_bad_rows():
    descs = scene([40, 35, 50], 64, seed=11)
    big = [x * np.float32(300.0) for x in descs]
    big[0][0, :4] = [127.0, -127.0, 127.49, -128.6]
    for scale in (1.0, 0.5, 20.0, 0.0):
        check(big, k=2, scale=scale)
    bad = [x.copy() for x in descs]
    bad[0][3, 5], bad[0][9, 0], bad[1][0, 63], bad[2][49, 1] = np.nan, np.inf, -np.inf, np.nan
    bad[1][4] = np.nan                                             # a whole row
    want = check(bad, k=2)
    assert want["counters"]["n_nonfinite"] == 4 + 64
    check(bad, k=2, scale=100.0)
    # a selected index out of range, an index list next to NULL, an empty list, a list with repeats
    rows = [np.array([5, 40, 3, -1, 39, 0, 7, 7]), None, np.array([49, 48, 1000000, 2, 2 ** 31 - 1, 10, 11, 12, 13])]
    want = check(descs, rows=rows, k=2)
    assert want["counters"]["n_bad_rows"] == 4 and want["counters"]["n_rows"] == 8 + 35 + 9
    check(descs, rows=[np.zeros(0, np.int32), None, np.array([1, 0])], k=2)
    check(descs, rows=[np.array([3, 50]), np.array([1, 2, 3, 4]), None], k=2)      # image 0 is left with one row that exists: no votes for it
    check([np.zeros((20, 32), np.float32)] * 3, k=2, min_votes=0)                    # maxabs = 0: s = 0


def test_ratio_k_and_min_votes():
    descs = scene([40, 33, 50, 45, 38, 41], 64, seed=13)
    assert check(descs, k=2, ratio=0.0)["votes"].sum() == 0
    one = check(descs, k=2, ratio=1.0)
    assert one["votes"].sum() > check(descs, k=2, ratio=0.8)["votes"].sum()
    for k in (1, 4, 5, 6, 50):
        for min_votes in (0, 1, 10):
            check(descs, k=k, min_votes=min_votes)
    assert check(descs, k=5, min_votes=0)["counters"]["n_pairs"] == 15
    assert check(descs, k=3, min_votes=10 ** 6)["counters"]["n_pairs"] == 0


def test_equal_votes_are_decided_by_the_index():
    descs = scene([40, 40, 30, 44], 64, seed=17)
    descs = [descs[0], descs[1], descs[2], descs[1].copy(), descs[3], descs[1].copy()]      # images 1, 3 and 5 are one image
    for k in (1, 2, 3):
        want = check(descs, k=k, min_votes=0)
        s = want["votes"] + want["votes"].T
        assert s[0, 1] == s[0, 3] == s[0, 5]


@pytest.mark.parametrize("n, m", [(300, 8), (1100, 2)])
def test_many_images(n, m):
    """More rows of the map than one wave's step, and more than the 1024 rows one pass of the scan takes."""
    rng = np.random.default_rng(n)
    world = rng.standard_normal((n + m, 32))
    descs = [(world[i:i + m] + 0.02 * rng.standard_normal((m, 32))).astype(np.float32) for i in range(n)]
    want = check(descs, k=3, ratio=0.9, min_votes=1)
    assert want["counters"]["n_pairs"] >= n - 1                    # every image with the next one at the least


def _buffers(descs, k, per_image=512):
    images, keep = _device(descs, None)
    images = [(t, ld, n, r, min(n, per_image)) for t, ld, n, r, _ in images]
    n, d = len(descs), descs[0].shape[1]
    work = torch.empty(hip.pairs_work_bytes([im[4] for im in images], d), dtype=torch.uint8, device="cuda")
    tab = hip.pairs_table(images, hip.pairs_rq(0.8), work.numel())
    B = dict(votes=torch.full((n, n), FILL, dtype=torch.int32, device="cuda"), counters=torch.full((8,), FILL, dtype=torch.int32, device="cuda"),
             out=torch.full((hip.pairs_out_layout(n, k)[2] + PAD,), FILL, dtype=torch.int32, device="cuda"), work=work, tab=tab, keep=keep)
    B["op"] = hip.op_select_pairs(tab, B["votes"], B["out"], B["counters"], work, n, d, per_image, k, 1)
    return B


def _bytes(B):
    return b"".join(B[key].cpu().numpy().tobytes() for key in ("votes", "out", "counters"))


def test_two_runs_a_captured_graph_and_a_table():
    descs = R.ring_scene(n=8, d=64, n_world=320, per=70)
    want = R.run(descs, k=2)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        B = _buffers(descs, 2)
        ops = hip.make_ops([B["op"]])
        hip.run_ops(ops)
        side.synchronize()
        first = _bytes(B)
        np.testing.assert_array_equal(B["votes"].cpu().numpy(), want["votes"])
        assert int(B["counters"][0]) == len(want["pairs"]) > 0
        hip.run_ops(ops)
        side.synchronize()
        assert _bytes(B) == first
        graph = hip.OpsGraph(ops)
        for _ in range(2):
            for key in ("votes", "out", "counters", "work"):
                B[key].fill_(FILL if key != "work" else 0xA5)
            graph.launch()
            side.synchronize()
            assert _bytes(B) == first
        # in a table next to another op, and twice in one table
        x = torch.randn(5, 32, device="cuda")
        spl = torch.zeros(5, 64, dtype=torch.bfloat16, device="cuda")
        C_ = _buffers(descs, 2)
        table = hip.make_ops([hip.op_aux(hip.AUX_SPLIT_SPL32, [x, spl], [x.stride(0), spl.stride(0), 5, 32]), C_["op"], B["op"]])
        for key in ("votes", "out", "counters"):
            B[key].fill_(FILL)
        hip.run_ops(table)
        side.synchronize()
        assert _bytes(B) == first == _bytes(C_) and torch.equal(spl, hip.split_spl32(x))
    torch.cuda.current_stream().wait_stream(side)


def test_a_refused_call_leaves_the_buffers_alone():
    descs = scene([40, 33], 64, seed=19)
    B = _buffers(descs, 1)
    before = _bytes(B)
    B["tab"][2, 0] = 65537                                         # rq
    with pytest.raises(hip.GimsHipError, match="select_pairs: rq = 65537"):
        hip.run_ops(hip.make_ops([B["op"]]))
    B["tab"][2, 0], B["tab"][2, 2] = hip.pairs_rq(0.8), B["work"].numel() - 1
    with pytest.raises(hip.GimsHipError, match="work_bytes"):
        hip.run_ops(hip.make_ops([B["op"]]))
    torch.cuda.synchronize()
    assert _bytes(B) == before


def _count_syncs(monkeypatch):
    counts = {"device": 0, "stream": 0, "event": 0}
    for name, owner, attr in (("device", torch.cuda, "synchronize"), ("stream", torch.cuda.Stream, "synchronize"), ("event", torch.cuda.Event, "synchronize")):
        orig = getattr(owner, attr)

        def counted(*a, _orig=orig, _name=name, **kw):
            counts[_name] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(owner, attr, counted)
    return counts


def test_select_pairs_orders_by_score_without_a_host_synchronisation(monkeypatch):
    descs = scene([60, 45, 70, 20, 52], 64, seed=23)
    rng = np.random.default_rng(29)
    scores = [np.round(rng.random(len(x)) * 8).astype(np.float32) / 8 for x in descs]       # nine values: ties everywhere
    feats = [(torch.from_numpy(x).cuda(), torch.from_numpy(s).cuda()) for x, s in zip(descs, scores)]
    feats[3] = (feats[3][0], None)                                                          # no scores: the first rows
    wide = torch.zeros(70, 100, device="cuda")
    wide[:, :64] = feats[2][0]
    feats[2] = (wide[:, :64], feats[2][1])                                                  # a row stride above D
    torch.cuda.synchronize()
    counts = _count_syncs(monkeypatch)
    sel = gims_amd.select_pairs(feats, k=2, per_image=32, ratio=0.85, min_votes=1)
    first = gims_amd.select_pairs(feats, k=2, per_image=32, ratio=0.85, order="first", scale=90.0)
    assert counts == {"device": 0, "stream": 0, "event": 0}, counts
    monkeypatch.undo()
    rows = [None if s is None else R.order_rows(s, 32) for s in scores[:3] + [None] + scores[4:]]
    for got, want in ((sel, R.run(descs, rows=rows, k=2, per_image=32, ratio=0.85)), (first, R.run(descs, k=2, per_image=32, ratio=0.85, scale=90.0))):
        np.testing.assert_array_equal(got.votes.cpu().numpy(), want["votes"])
        assert got.stats == want["counters"] and int(got.n_rows) == want["counters"]["n_rows"] == 32 * 4 + 20
        assert got.tolist() == [tuple(p) for p in want["pairs"].tolist()] and len(got) == len(want["pairs"]) > 0
        assert got.pair_votes[:len(got)].tolist() == want["pair_votes"].tolist()
        assert got.pairs.shape == (10, 2) and got.pair_votes.shape == (10,) and got.votes.shape == (5, 5) and got.counters.shape == (8,)
        for i in range(5):
            assert got.partners(i) == sorted([b for a, b in got.tolist() if a == i] + [a for a, b in got.tolist() if b == i])
    assert any((scores[i][rows[i]][:-1] == scores[i][rows[i]][1:]).any() for i in (0, 1, 2, 4))      # tied scores were ordered
    with pytest.raises(AttributeError, match="immutable"):
        sel.votes = None


def test_end_to_end(synth_sd):
    """select_pairs on the image set of test_tracks_gpu.py::test_end_to_end, then match_features on its list: the same results as on the
    same list written by hand."""
    from tests.test_features_gpu import OUT_KEYS, _images, _model, _same
    m = _model(synth_sd, attention_precision="bf16x3")
    images, each = _images()
    feats = m.encode_images(images, each=each)
    sel = gims_amd.select_pairs(feats, k=2, per_image=256, min_votes=0)
    want = R.run([f.descriptors.cpu().numpy() for f in feats], k=2, per_image=256, min_votes=0,
                 rows=[R.order_rows(f.scores.cpu().numpy(), 256) for f in feats])
    np.testing.assert_array_equal(sel.votes.cpu().numpy(), want["votes"])
    pairs = sel.tolist()
    assert pairs == [tuple(p) for p in want["pairs"].tolist()] and 6 <= len(pairs) <= 12 and sel.stats == want["counters"]
    assert all(0 <= a < b < 6 for a, b in pairs) and pairs == sorted(set(pairs))
    outs = m.match_features(feats, pairs)
    by_hand = m.match_features(feats, [(int(a), int(b)) for a, b in want["pairs"]])
    assert len(outs) == len(pairs)
    _same(list(outs), list(by_hand), OUT_KEYS)
