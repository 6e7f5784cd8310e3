"""NumPy restatement of GIMS_AUX_SELECT_PAIRS (include/gims_hip.h): the scale, the int8 quantisation, the two smallest squared
distances of every row against every other image, the vote, the top-k selection and the compaction -- every decision in integers, so the
device must agree with it exactly.  ``votes_brute`` is a second, slower implementation of steps 3 and 4 for the CPU test."""
import numpy as np

COUNTERS = ("n_pairs", "n_rows", "n_short_images", "n_bad_rows", "n_nonfinite")
I32_MAX = 2 ** 31 - 1


def rq_of(ratio) -> int:
    r = float(np.float32(ratio))
    return int(np.rint(r * r * 65536.0))


def order_rows(scores, per_image):
    """order='score': the stable descending sort of the scores, cut to per_image."""
    return np.argsort(-np.asarray(scores, dtype=np.float64), kind="stable")[:per_image].astype(np.int32)


def select_rows(descs, rows, per_image):
    """-> per image (the selected float32 rows [m, D], exists [m]): rows=None takes the first min(n, per_image) rows; an index outside the
    image gives a row of zeros that does not exist."""
    out = []
    for i, x in enumerate(descs):
        x = np.asarray(x, dtype=np.float32)
        idx = np.arange(min(len(x), per_image)) if rows is None or rows[i] is None else np.asarray(rows[i], dtype=np.int64)
        ok = (idx >= 0) & (idx < len(x))
        sel = np.zeros((len(idx), x.shape[1]), np.float32)
        sel[ok] = x[idx[ok]]
        out.append((sel, ok))
    return out


def quantise(selected, scale=None):
    """Steps 1 and 2 -> (q int8 [m, D] per image, s float32, n_nonfinite)."""
    n_nonfinite = sum(int((~np.isfinite(x[ok])).sum()) for x, ok in selected)
    if scale is None:
        maxabs = np.float32(0)
        for x, ok in selected:
            v = np.abs(x[ok])
            v = v[np.isfinite(v)]
            if v.size:
                maxabs = max(maxabs, np.float32(v.max()))
        with np.errstate(over="ignore"):
            s = np.float32(127.0) / np.float32(maxabs) if maxabs > 0 else np.float32(0)
    else:
        s = np.float32(scale)
    qs = []
    for x, ok in selected:
        x = np.where(np.isfinite(x), x, np.float32(0)).astype(np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            p = np.rint(x * s)
        p = np.where(np.isnan(p), np.float32(0), p)
        q = np.clip(p, -127, 127).astype(np.int8)
        q[~ok] = 0
        qs.append(q)
    return qs, np.float32(s), min(n_nonfinite, I32_MAX)


def votes_of(qs, exists, rq):
    """Steps 3 and 4 -> votes int32 [N, N]."""
    n, d = len(qs), qs[0].shape[1]
    far = 1 << 40                                                  # the distance to a row that does not exist: beyond every real one
    width = max(2, max(len(q) for q in qs))
    base = np.zeros((n, width, d), np.int64)                       # every image on `width` rows, the rows behind its own not existing
    there = np.zeros((n, width), bool)
    for j, q in enumerate(qs):
        base[j, :len(q)] = q
        there[j, :len(q)] = exists[j]
    norms = (base * base).sum(2)
    flat = base.reshape(n * width, d).astype(np.float64)
    votes = np.zeros((n, n), np.int32)
    for i in range(n):
        if not exists[i].any():
            continue
        q = base[i, :len(qs[i])]
        dots = np.rint(q.astype(np.float64) @ flat.T).astype(np.int64).reshape(len(q), n, width)       # (exact: far below 2^53)
        dist = norms[i, :len(q), None, None] + norms[None, :, :] - 2 * dots                             # at most 4 * 127^2 * 1024
        dist = np.where(there[None], dist, far)
        two = np.partition(dist, 1, axis=2)[:, :, :2]
        vote = (two[:, :, 0] * 65536 < rq * two[:, :, 1]) & (two[:, :, 1] < far) & exists[i][:, None]
        votes[i] = vote.sum(0)
        votes[i, i] = 0
    return votes


def votes_brute(qs, exists, rq):
    """The same votes by a full sort of every block and Python integers."""
    n = len(qs)
    votes = np.zeros((n, n), np.int32)
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            cols = [[int(v) for v in qs[j][c]] for c in range(len(qs[j])) if exists[j][c]]
            if len(cols) < 2:
                continue
            for r in range(len(qs[i])):
                if not exists[i][r]:
                    continue
                a = [int(v) for v in qs[i][r]]
                ds = sorted(sum((x - y) ** 2 for x, y in zip(a, b)) for b in cols)
                votes[i, j] += ds[0] * 65536 < rq * ds[1]
    return votes


def select(votes, k, min_votes):
    """Step 5 -> (pairs int32 [n_pairs, 2] ascending, pair_votes int32 [n_pairs])."""
    n = len(votes)
    s = votes.astype(np.int64) + votes.T
    chosen = set()
    for i in range(n):
        js = np.flatnonzero((s[i] >= min_votes) & (np.arange(n) != i))
        for j in js[np.lexsort((js, -s[i, js]))][:k]:              # by (-S, j)
            chosen.add((min(i, int(j)), max(i, int(j))))
    pairs = np.array(sorted(chosen), dtype=np.int32).reshape(-1, 2)
    return pairs, np.array([s[a, b] for a, b in pairs], dtype=np.int32)


def run(descs, rows=None, k=20, per_image=512, ratio=0.8, min_votes=1, scale=None):
    """The whole op -> dict(votes, pairs, pair_votes, counters (the first five words, as a dict), scale, q)."""
    selected = select_rows(descs, rows, per_image)
    exists = [ok for _, ok in selected]
    qs, s, n_nonfinite = quantise(selected, scale)
    votes = votes_of(qs, exists, rq_of(ratio))
    pairs, pair_votes = select(votes, k, min_votes)
    ms = [len(ok) for ok in exists]
    counters = dict(zip(COUNTERS, (len(pairs), sum(ms), sum(m < 2 for m in ms), sum(int((~ok).sum()) for ok in exists), n_nonfinite)))
    return dict(votes=votes, pairs=pairs, pair_votes=pair_votes, counters=counters, scale=s, q=qs)


def ring_scene(n=12, d=128, n_world=480, per=96, step=40, noise=0.03, seed=7):
    """N images around a ring of unit "world" descriptors: image i sees world rows (step i .. step i + per - 1) mod n_world with noise,
    renormalised and permuted.  Images at ring distance t share per - step t world rows."""
    rng = np.random.default_rng(seed)
    world = rng.standard_normal((n_world, d))
    world /= np.linalg.norm(world, axis=1, keepdims=True)
    out = []
    for i in range(n):
        x = world[(step * i + np.arange(per)) % n_world] + noise * rng.standard_normal((per, d))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        out.append(x[rng.permutation(per)].astype(np.float32))
    return out


def ring_distance(a, b, n):
    return min((a - b) % n, (b - a) % n)
