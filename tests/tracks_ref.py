"""NumPy restatement of GIMS_AUX_BUILD_TRACKS (include/gims_hip.h; gims_amd/csrc/tracks.hip), written from that specification -- TEST
REFERENCE ONLY -- and the synthetic scene generator of the track tests and of tools/track_bench.py.

Keypoint i of image k is node start[k] + i.  Row i of pair (a, b) with j = matches0[i] is an edge iff 0 <= j < n_b, its score (when given)
is >= min_score and its mask (when given) is non-zero; -1 is "no match", any other j outside the image is counted in n_bad.  Tracks are the
connected components with at least min_length nodes, numbered by their smallest node, their observations in ascending node order; a
component with two nodes of one image conflicts, and is dropped whole unless conflicts == 'keep'."""
import numpy as np

COUNTERS = ("n_tracks", "n_obs", "n_conflicting", "n_edges", "n_bad", "status")


def edges(counts, pairs, matches, scores=None, masks=None, min_score=None):
    """The accepted rows of all pairs as node pairs int64 [n_edges, 2] (duplicates and self loops included), and n_bad."""
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out, n_bad = [], 0
    for p, (a, b) in enumerate(pairs):
        m = np.asarray(matches[p]).reshape(-1).astype(np.int64)
        assert m.shape[0] == counts[a], (p, m.shape, counts[a])
        i = np.arange(counts[a], dtype=np.int64)
        inside = (m >= 0) & (m < counts[b])
        n_bad += int(((m != -1) & ~inside).sum())
        ok = inside.copy()
        if min_score is not None and scores is not None and scores[p] is not None:
            with np.errstate(invalid="ignore"):
                ok &= np.asarray(scores[p]).reshape(-1) >= np.float32(min_score)          # (a NaN compares false)
        if masks is not None and masks[p] is not None:
            ok &= np.asarray(masks[p]).reshape(-1) != 0
        out.append(np.stack([start[a] + i[ok], start[b] + m[ok]], axis=1))
    return (np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)), n_bad


def build(counts, pairs, matches, scores=None, masks=None, min_score=None, min_length=2, conflicts="drop"):
    """-> dict: track_of int32 [N], indptr int32 [T + 1], obs_image, obs_keypoint int32 [n_obs], conflict uint8 [T], stats (COUNTERS)."""
    assert min_length >= 2 and conflicts in ("drop", "keep")
    counts = [int(c) for c in counts]
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(start[-1])
    image_of = np.repeat(np.arange(len(counts)), counts)
    e, n_bad = edges(counts, pairs, matches, scores, masks, min_score)

    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in e.tolist():
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)

    components = {}                                   # root -> members; nodes are visited in ascending order, so the members ascend and the
    for g in range(n):                                # components appear in ascending order of their smallest member
        components.setdefault(find(g), []).append(g)

    track_of = np.full(n, -1, dtype=np.int32)
    indptr, obs, conflict, n_conflicting = [0], [], [], 0
    for members in components.values():
        imgs = image_of[members]
        c = len(set(imgs.tolist())) < len(members)
        n_conflicting += int(c)
        if len(members) < min_length or (c and conflicts == "drop"):
            continue
        track_of[members] = len(conflict)
        obs.extend(members)
        indptr.append(len(obs))
        conflict.append(int(c))
    obs = np.asarray(obs, dtype=np.int64)
    obs_image = image_of[obs].astype(np.int32) if len(obs) else np.zeros(0, dtype=np.int32)
    obs_keypoint = (obs - start[obs_image]).astype(np.int32) if len(obs) else np.zeros(0, dtype=np.int32)
    stats = dict(n_tracks=len(conflict), n_obs=len(obs), n_conflicting=n_conflicting, n_edges=len(e), n_bad=n_bad, status=0)
    return dict(track_of=track_of, indptr=np.asarray(indptr, dtype=np.int32), obs_image=obs_image, obs_keypoint=obs_keypoint,
                conflict=np.asarray(conflict, dtype=np.uint8), stats=stats)


def all_pairs(n_images):
    return [(a, b) for a in range(n_images) for b in range(a + 1, n_images)]


def scene(seed, n_points, n_images, p_seen, q_kept, w_wrong, pairs=None, n_seen=None):
    """A synthetic image set: n_points scene points; each image sees a point with probability p_seen (n_seen given: exactly n_seen random
    points instead), in a random keypoint order.  A pair's true matches are the commonly seen points, each kept with probability q_kept; a
    fraction w_wrong of the unmatched rows get a random FREE partner, so that matches0 stays injective, as mutual matching makes it.
    -> (counts, pairs, matches: int64 [n_a] per pair, -1 = no match)."""
    rng = np.random.default_rng(seed)
    pairs = all_pairs(n_images) if pairs is None else list(pairs)
    if n_seen is None:
        seen = [rng.permutation(np.nonzero(rng.random(n_points) < p_seen)[0]) for _ in range(n_images)]   # seen[k][i]: the point of keypoint i
    else:
        seen = [rng.permutation(n_points)[:n_seen] for _ in range(n_images)]
    counts = [len(s) for s in seen]
    where = []                                                                                            # where[k][point]: its keypoint, or -1
    for s in seen:
        inv = np.full(n_points, -1, dtype=np.int64)
        inv[s] = np.arange(len(s))
        where.append(inv)
    matches = []
    for a, b in pairs:
        m = where[b][seen[a]].copy()
        m[(m >= 0) & (rng.random(len(m)) >= q_kept)] = -1
        if a == b:
            m = np.arange(counts[a], dtype=np.int64)
        free = np.setdiff1d(np.arange(counts[b]), m[m >= 0])
        rows = np.nonzero(m < 0)[0]
        rows = rows[rng.random(len(rows)) < w_wrong][:len(free)]
        m[rows] = rng.permutation(free)[:len(rows)]
        matches.append(m.astype(np.int64))
    return counts, pairs, matches


def inverse(m, n_b):
    """matches1 of an injective matches0: the pair listed the other way round."""
    inv = np.full(n_b, -1, dtype=np.int64)
    ok = m >= 0
    inv[m[ok]] = np.nonzero(ok)[0]
    return inv
