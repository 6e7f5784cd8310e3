"""GPU tests of the multi-view tracks: GIMS_AUX_BUILD_TRACKS (gims_amd/csrc/tracks.hip) against the NumPy restatement
(tests/tracks_ref.py), all five outputs and the counters for exact equality, with 64 sentinel words behind every output and work buffer;
then gims_amd.build_tracks behind encode_images / match_features / verify_pairs.

Shapes.  The hand-worked case of tests/test_tracks_cpu.py; scene A (about 2 160 nodes in 6 images, 15 + 3 pairs: more than one scan tile, a
few hundred tracks, a few dozen conflicts); N = T - 1, T, T + 1 and 2 T + 1 for the scan tile T; components of exactly the short-segment limit
(one lane / a wave) and of the long-segment limit (a wave / the prefix count over the nodes) and one more each; three huge components that fill
the huge table, glued or not; chains and a star over 200 images; one conflicting component of 600 and one of 3000 over two tiles; empty
images, empty pairs, N = 0; poisoned indices; score and mask filters; permuted pair lists."""
import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip, verify_pairs
from tests import tracks_ref as R
from tests.test_tracks_cpu import HAND, HAND_DROP, HAND_DROP3, HAND_KEEP, SCENE_A, same

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENT, PAD = -0x5A5A5A5B, 64
KEYS = ("track_of", "indptr", "obs_image", "obs_keypoint", "conflict")


def _padded(words):
    return torch.full((words + PAD,), SENT, dtype=torch.int32, device="cuda")


def _buffers(counts, pairs, matches, scores, masks):
    """The device side of one call: table, start and the sentinel-filled outputs and workspace (what hip.build_tracks allocates, padded)."""
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()      # noqa: E731
    n = int(sum(counts))
    entries = [(a, b, dev(matches[p], np.int64), dev(None if scores is None else scores[p], np.float32),
                dev(None if masks is None else masks[p], np.uint8)) for p, (a, b) in enumerate(pairs)]
    B = dict(n=n, entries=entries, n_pairs=len(pairs), n_images=len(counts))
    B["table"] = hip.upload_large(hip.tracks_table(entries, counts, "cuda"), "cuda")
    B["start"] = hip.upload(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), "cuda")
    B["out_words"] = hip.tracks_out_layout(n)[-1]
    B["work_bytes"] = hip.tracks_work_bytes(len(pairs), len(counts), n)
    B["track_of"], B["out"], B["counters"], B["work"] = _padded(n), _padded(B["out_words"]), _padded(8), _padded(B["work_bytes"] // 4)
    return B


def _op(B, min_score, min_length, conflicts):
    return hip.op_build_tracks(B["table"], B["start"], B["track_of"], B["out"], B["counters"], B["work"][:B["work_bytes"] // 4], B["n_pairs"],
                               B["n_images"], B["n"], min_length, conflicts == "keep", 0.0 if min_score is None else min_score)


def _read(B):
    """The outputs as the restatement returns them; the sentinels behind every buffer, and behind what the call was to write, must be intact."""
    torch.cuda.synchronize()
    n = B["n"]
    counters = B["counters"].cpu().numpy()
    stats = dict(zip(hip.TRACKS_COUNTERS, (int(v) for v in counters[:6])))
    assert (counters[6:8] == 0).all() and (counters[8:] == SENT).all()
    track_of, out, work = B["track_of"].cpu().numpy(), B["out"].cpu().numpy(), B["work"].cpu().numpy()
    assert (track_of[n:] == SENT).all() and (out[B["out_words"]:] == SENT).all() and (work[B["work_bytes"] // 4:] == SENT).all()
    T, n_obs = stats["n_tracks"], stats["n_obs"]
    o_ptr, o_img, o_kp, o_conf, _ = hip.tracks_out_layout(n)
    conflict = out[o_conf:B["out_words"]].view(np.uint8)
    # nothing behind what the header says is written: indptr[T + 1 ..], obs[n_obs ..], conflict[T ..] keep the sentinel
    assert (out[o_ptr + T + 1:o_img] == SENT).all() and (out[o_img + n_obs:o_kp] == SENT).all() and (out[o_kp + n_obs:o_conf] == SENT).all()
    assert (conflict[T:] == np.array([SENT], dtype=np.int32).view(np.uint8)[0]).all()
    if n == 0 or B["n_pairs"] == 0:                   # (the empty call leaves track_of alone: the Python layer owns its -1)
        assert (track_of[:n] == SENT).all()
        track_of = np.full(n, -1, dtype=np.int32)
    return dict(track_of=track_of[:n], indptr=out[o_ptr:o_ptr + T + 1], obs_image=out[o_img:o_img + n_obs], obs_keypoint=out[o_kp:o_kp + n_obs],
                conflict=conflict[:T], stats=stats)


def run(counts, pairs, matches, scores=None, masks=None, min_score=None, min_length=2, conflicts="drop"):
    B = _buffers(counts, pairs, matches, scores, masks)
    hip.run_ops(hip.make_ops([_op(B, min_score, min_length, conflicts)]))
    return _read(B)


def check(counts, pairs, matches, scores=None, masks=None, min_score=None, min_length=2, conflicts="drop"):
    got = run(counts, pairs, matches, scores, masks, min_score, min_length, conflicts)
    want = R.build(counts, pairs, matches, scores, masks, min_score, min_length, conflicts)
    same(got, want)
    return got


def identical(a, b):
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.fixture(scope="module")
def scene_a():
    """Scene A and its three extra pairs: (0, 1) again, (3, 1) as the inverse of (1, 3), and a self pair (2, 2) with two rows swapped."""
    counts, pairs, matches = R.scene(**SCENE_A)
    pairs, matches = list(pairs), list(matches)
    pairs.append((0, 1))
    matches.append(matches[pairs.index((0, 1))].copy())
    pairs.append((3, 1))
    matches.append(R.inverse(matches[pairs.index((1, 3))], counts[3]))
    me = np.arange(counts[2], dtype=np.int64)
    me[[5, 9]] = me[[9, 5]]
    pairs.append((2, 2))
    matches.append(me)
    return counts, pairs, matches


def test_hand_worked_case():
    same(run(**HAND), HAND_DROP)
    same(run(**HAND, conflicts="keep"), HAND_KEEP)
    same(run(**HAND, min_length=3), HAND_DROP3)


@pytest.mark.parametrize("conflicts", ["drop", "keep"])
@pytest.mark.parametrize("min_length", [2, 3])
def test_scene_a(scene_a, conflicts, min_length):
    counts, pairs, matches = scene_a
    got = check(counts, pairs, matches, min_length=min_length, conflicts=conflicts)
    assert got["stats"]["n_tracks"] >= 100 and got["stats"]["n_conflicting"] >= 10 and sum(counts) > hip.TRACKS_SCAN_TILE
    assert (got["conflict"].sum() > 0) == (conflicts == "keep")


@pytest.mark.parametrize("n", [hip.TRACKS_SCAN_TILE - 1, hip.TRACKS_SCAN_TILE, hip.TRACKS_SCAN_TILE + 1, 2 * hip.TRACKS_SCAN_TILE + 1])
def test_scan_tile_seams(n):
    """Images of unequal counts and a sparse chain of matches; the last node of the set and the nodes on both sides of every tile seam are matched."""
    counts = [n // 2, n // 3, n - n // 2 - n // 3]
    pairs = [(0, 1), (1, 2), (0, 2)]
    matches = []
    for a, b in pairs:
        m = np.full(counts[a], -1, dtype=np.int64)
        rows = np.arange(0, counts[a], 37)
        m[rows] = (rows * 7 + 3) % counts[b]
        matches.append(m)
    matches[2][0] = counts[2] - 1                                            # node 0 - node n - 1
    start = np.concatenate([[0], np.cumsum(counts)])
    for seam in range(hip.TRACKS_SCAN_TILE, n, hip.TRACKS_SCAN_TILE):        # nodes seam - 1 and seam, from image 0 when they lie in another image
        for g in (seam - 1, seam):
            k = int(np.searchsorted(start, g, side="right") - 1)
            if k > 0:
                matches[k - 1 if k == 1 else 2][g - seam + 40] = g - start[k]
    got = check(counts, pairs, matches, conflicts="keep")
    assert got["stats"]["n_tracks"] > 20 and got["track_of"][n - 1] >= 0


@pytest.mark.parametrize("limit", ["short", "long"])
def test_components_at_a_segment_limit(limit):
    """S + 1 images of two keypoints: keypoint 0 chains through all of them (one more than the limit), keypoint 1 through the first S (the limit).
    short: one lane / a wave ranks the component by counting; long: a wave / the prefix count over the nodes (N = 2050: two scan tiles)."""
    S = hip.TRACKS_SHORT_SEGMENT if limit == "short" else hip.tracks_huge(2 * (hip.TRACKS_LONG_SEGMENT + 1))
    assert S == (32 if limit == "short" else 1024)
    counts = [2] * (S + 1)
    pairs = [(k, k + 1) for k in range(S)]
    matches = [np.array([0, 1 if k + 1 < S else -1], dtype=np.int64) for k in range(S)]
    got = check(counts, pairs, matches)
    assert np.diff(got["indptr"]).tolist() == [S + 1, S]


@pytest.mark.parametrize("order", ["descending", "random", "star"])
def test_deep_chains(order):
    n = 200
    counts = [1] * n
    if order == "star":
        pairs = [(k, 0) for k in range(1, n)]
    else:
        pairs = [(k, k + 1) for k in range(n - 1)][::-1]
        if order == "random":
            pairs = [pairs[i] for i in np.random.default_rng(3).permutation(n - 1)]
    got = check(counts, pairs, [np.zeros(1, dtype=np.int64)] * (n - 1))
    assert got["stats"]["n_tracks"] == 1 and got["indptr"].tolist() == [0, n] and got["obs_image"].tolist() == list(range(n))


def test_one_giant_conflicting_component():
    i = np.arange(300, dtype=np.int64)
    args = ([300, 300], [(0, 1), (0, 1)], [i, (i + 1) % 300])
    drop = check(*args)
    assert drop["stats"]["n_tracks"] == 0 and drop["stats"]["n_conflicting"] == 1 and all(len(drop[k]) == 0 for k in KEYS[2:]) and (drop["track_of"] == -1).all()
    keep = check(*args, conflicts="keep")
    assert keep["indptr"].tolist() == [0, 600] and keep["conflict"].tolist() == [1]
    assert keep["obs_image"].tolist() == [0] * 300 + [1] * 300 and keep["obs_keypoint"].tolist() == list(range(300)) * 2


@pytest.mark.parametrize("glue", [False, True])
def test_huge_components(glue):
    """1100 images of three keypoints, each keypoint chained through all images: three components of 1100 > 1024 nodes, as many as N = 3300 can
    hold (every row of the huge table is taken), interleaved node by node over two scan tiles.  glue: a self pair of image 7 joins the chains of
    keypoints 0 and 2 into one conflicting component of 2200."""
    n = 1100
    assert 3 * n // (hip.tracks_huge(3 * n) + 1) == 3
    counts = [3] * n
    pairs = [(k, k + 1) for k in range(n - 1)]
    matches = [np.arange(3, dtype=np.int64)] * (n - 1)
    if glue:
        pairs.append((7, 7))
        matches = matches + [np.array([2, 1, 2], dtype=np.int64)]
    for conflicts in ("drop", "keep"):
        got = check(counts, pairs, matches, conflicts=conflicts)
        want = ([2 * n, n] if conflicts == "keep" else [n]) if glue else [n, n, n]
        assert np.diff(got["indptr"]).tolist() == want and got["stats"]["n_conflicting"] == int(glue)
    if glue:
        assert got["conflict"].tolist() == [1, 0] and got["obs_keypoint"][:6].tolist() == [0, 2, 0, 2, 0, 2]


def test_one_huge_conflicting_component_over_two_tiles():
    i = np.arange(1500, dtype=np.int64)
    args = ([1500, 1500], [(0, 1), (0, 1)], [i, (i + 1) % 1500])
    assert check(*args)["stats"] == dict(n_tracks=0, n_obs=0, n_conflicting=1, n_edges=3000, n_bad=0, status=0)
    keep = check(*args, conflicts="keep")
    assert keep["indptr"].tolist() == [0, 3000] and keep["conflict"].tolist() == [1] and keep["obs_keypoint"].tolist() == list(range(1500)) * 2


def test_empty_inputs():
    none5, none0 = np.full(5, -1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    got = check([5, 0, 4], [(0, 1), (1, 2), (0, 2), (1, 1)], [none5, none0, np.array([3, -1, 0, -1, -1]), none0])     # an image of no keypoints inside a set
    assert got["stats"]["n_tracks"] == 2
    got = check([5, 0, 4], [(0, 2), (2, 0)], [none5, none5[:4]])                                                        # every pair empty
    assert got["stats"] == dict(n_tracks=0, n_obs=0, n_conflicting=0, n_edges=0, n_bad=0, status=0) and got["indptr"].tolist() == [0]
    for counts, pairs, matches in (([0, 0], [(0, 1)], [none0]), ([0], [], []), ([5, 4], [], [])):                       # N = 0; no pairs at all
        got = check(counts, pairs, matches)
        assert got["stats"]["n_tracks"] == 0 and got["indptr"].tolist() == [0]


def test_poisoned_indices_are_counted_and_never_used():
    counts, pairs, matches = R.scene(11, 120, 4, 0.6, 0.8, 0.05)
    clean = check(counts, pairs, matches, conflicts="keep")
    poisoned = [m.copy() for m in matches]
    poison = [-2, None, 2 ** 31, 2 ** 40, -2 ** 40]
    for k, v in enumerate(poison):
        p = k % len(pairs)
        row = np.nonzero(poisoned[p] == -1)[0][k]
        poisoned[p][row] = counts[pairs[p][1]] if v is None else v            # (None: n_b itself, the first index past the image)
    got = check(counts, pairs, poisoned, conflicts="keep")
    assert got["stats"]["n_bad"] == 5 and clean["stats"]["n_bad"] == 0
    identical(got, clean)
    assert got["stats"] == dict(clean["stats"], n_bad=5)


def test_filters():
    counts, pairs, matches = R.scene(12, 150, 4, 0.6, 0.8, 0.05)
    rng = np.random.default_rng(13)
    thr = np.float32(0.3)
    edge = np.array([np.nextafter(thr, np.float32(0)), thr, np.nextafter(thr, np.float32(1)), np.nan], dtype=np.float32)
    scores = [edge[rng.integers(0, 4, size=len(m))] for m in matches]
    masks = [(rng.random(len(m)) < 0.7).astype(np.uint8) * rng.integers(1, 256, size=len(m)).astype(np.uint8) for m in matches]
    plain = check(counts, pairs, matches)
    by_score = check(counts, pairs, matches, scores=scores, min_score=float(thr))
    by_mask = check(counts, pairs, matches, masks=masks)
    both = check(counts, pairs, matches, scores=scores, masks=masks, min_score=float(thr), conflicts="keep")
    some = check(counts, pairs, matches, scores=[scores[0]] + [None] * (len(pairs) - 1), masks=[None] * (len(pairs) - 1) + [masks[-1]], min_score=float(thr))
    assert plain["stats"]["n_edges"] > by_score["stats"]["n_edges"] > both["stats"]["n_edges"] > 0 and plain["stats"]["n_edges"] > by_mask["stats"]["n_edges"]
    assert plain["stats"]["n_edges"] > some["stats"]["n_edges"] > by_score["stats"]["n_edges"]
    want = sum(int(((m >= 0) & (s >= thr)).sum()) for m, s in zip(matches, scores))
    assert by_score["stats"]["n_edges"] == want


def test_order_independence(scene_a):
    counts, pairs, matches = scene_a
    first = run(counts, pairs, matches, conflicts="keep")
    identical(first, run(counts, pairs, matches, conflicts="keep"))         # the same call twice
    for seed in range(5):
        perm = np.random.default_rng(seed).permutation(len(pairs))
        again = run(counts, [pairs[i] for i in perm], [matches[i] for i in perm], conflicts="keep")
        identical(first, again)
        assert again["stats"] == first["stats"]


def test_op_replays_in_a_table_next_to_another_op(scene_a):
    counts, pairs, matches = scene_a
    want = R.build(counts, pairs, matches, conflicts="keep")
    B = _buffers(counts, pairs, matches, None, None)
    x = torch.randn(64, 128, device="cuda")
    want_split = hip.split_spl32(x)
    split = torch.zeros_like(want_split)
    ops = hip.make_ops([_op(B, None, 2, "keep"), hip.op_aux(hip.AUX_SPLIT_SPL32, (x, split), (x.stride(0), split.stride(0), 64, 128))])
    for _ in range(2):
        for k in ("track_of", "out", "counters", "work"):
            B[k].fill_(SENT)
        split.zero_()
        hip.run_ops(ops)
        same(_read(B), want)
        assert torch.equal(split, want_split)


def test_binding_allocates_and_fills_track_of(scene_a):
    """hip.build_tracks: its own buffers; -1 in track_of also when the op has nothing to join."""
    counts, pairs, matches = scene_a
    entries = [(a, b, torch.from_numpy(m).cuda(), None, None) for (a, b), m in zip(pairs, matches)]
    track_of, out, counters, start, keep = hip.build_tracks(entries, counts, "cuda", keep_conflicting=True)
    torch.cuda.synchronize()
    want = R.build(counts, pairs, matches, conflicts="keep")
    np.testing.assert_array_equal(track_of.cpu().numpy(), want["track_of"])
    assert counters.tolist()[:6] == [want["stats"][k] for k in R.COUNTERS] and start.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    track_of, out, counters, start, keep = hip.build_tracks([], [3, 4], "cuda")
    torch.cuda.synchronize()
    assert track_of.tolist() == [-1] * 7 and counters.tolist() == [0] * 8 and out[0].item() == 0


# ------------------------------------------------------------------------------------------------ end to end
def _count_syncs(monkeypatch):
    counts = {"device": 0, "stream": 0, "event": 0}
    for name, owner, attr in (("device", torch.cuda, "synchronize"), ("stream", torch.cuda.Stream, "synchronize"), ("event", torch.cuda.Event, "synchronize")):
        orig = getattr(owner, attr)

        def counted(*a, _orig=orig, _name=name, **kw):
            counts[_name] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(owner, attr, counted)
    return counts


def _against_restatement(tracks, feats, pairs, outs, **kw):
    counts = [f.n for f in feats]
    host = lambda key: [o[key].reshape(-1).cpu().numpy() for o in outs]      # noqa: E731
    want = R.build(counts, pairs, host("matches0"), scores=host("matching_scores0") if kw.get("min_score") is not None else None,
                   masks=[m.cpu().numpy() for m in kw["inlier"]] if kw.get("inlier") is not None else None, min_score=kw.get("min_score"),
                   min_length=kw.get("min_length", 2), conflicts=kw.get("conflicts", "drop"))
    got = {k: getattr(tracks, k).cpu().numpy() for k in KEYS}
    got["stats"] = tracks.stats
    same(got, want)
    assert tracks.n_tracks == want["stats"]["n_tracks"] == len(tracks) and tracks.n_obs == want["stats"]["n_obs"]
    assert tracks.image_start == np.concatenate([[0], np.cumsum(counts)]).tolist()
    return want


def test_end_to_end(synth_sd, monkeypatch):
    from tests.test_features_gpu import _images, _model
    m = _model(synth_sd, attention_precision="bf16x3")
    images, each = _images()
    feats = m.encode_images(images, each=each)
    pairs = [(0, 1), (2, 3), (4, 5), (0, 4), (1, 5), (4, 0), (2, 5), (1, 4)]
    outs = m.match_features(feats, pairs)
    inl = verify_pairs(outs.datas, outs)
    torch.cuda.synchronize()
    counts = _count_syncs(monkeypatch)
    tracks = gims_amd.build_tracks(feats, pairs, outs)
    assert counts == {"device": 0, "stream": 0, "event": 1}, counts          # the one read-back of the counters
    monkeypatch.undo()
    _against_restatement(tracks, feats, pairs, outs)
    _against_restatement(gims_amd.build_tracks(feats, pairs, outs, conflicts="keep", min_length=3), feats, pairs, outs, conflicts="keep", min_length=3)
    verified = gims_amd.build_tracks(feats, pairs, outs, inlier=inl)
    _against_restatement(verified, feats, pairs, outs, inlier=inl["inlier"])
    _against_restatement(gims_amd.build_tracks(feats, pairs, outs, inlier=inl["inlier"], min_score=0.5), feats, pairs, outs, inlier=inl["inlier"], min_score=0.5)
    scored = gims_amd.build_tracks([f.n for f in feats], pairs, list(outs), min_score=0.5, conflicts="keep")         # plain counts, a plain list
    want = _against_restatement(scored, feats, pairs, outs, min_score=0.5, conflicts="keep")
    # the accessors
    for t in (tracks, scored):
        start = t.image_start
        for k in range(len(feats)):
            assert torch.equal(t.of_image(k), t.track_of[start[k]:start[k + 1]]) and t.of_image(k).shape == (feats[k].n,)
        assert torch.equal(t.lengths(), (t.indptr[1:] - t.indptr[:-1])) and t.lengths().dtype == torch.int32
        pts = t.points(feats)
        assert pts.shape == (t.n_obs, 2) and pts.dtype == torch.float32
        host = t.to_host()
        assert len(host) == t.n_tracks and sum(len(tr) for tr in host) == t.n_obs
        flat = [ob for tr in host for ob in tr]
        assert flat == list(zip(t.obs_image.tolist(), t.obs_keypoint.tolist()))
        if flat:
            exp = torch.stack([feats[i].keypoints[j] for i, j in flat]).float()
            assert torch.equal(pts, exp)
    assert [len(tr) for tr in scored.to_host()] == np.diff(want["indptr"]).tolist()
    with pytest.raises(ValueError, match="out of range"):
        tracks.of_image(6)
