"""NumPy restatement of GIMS_AUX_DIOU_NMS (include/gims_hip.h; gims_amd/csrc/nms.hip), written from that specification -- TEST
INFRASTRUCTURE.  The reference's own ``process_diou_nms`` is run by tools/gen_golden_nms.py on the seeded recipes below; its returned rows
are the ``tests/golden/nms_*.npz`` this restatement and the device are compared with, as exact row lists.

Two forms of the greedy rule: ``sequential`` (walk the order, keep the first, drop what does not survive it) and ``rounds`` (the
status relaxation the kernel runs: suppressed once an earlier non-survivor partner is kept, kept once all of them are suppressed).
``run_op`` is the whole op for a batch: keep rows per segment then -1, counts, bad."""
import numpy as np

F = np.float32


def boxes(kp, radius):
    """kp [n, >= 3] = x, y, size -> float32 [n, 4] corners: half-widths and corners in double, rounded once.  radius None / 0: size mode."""
    kp = np.asarray(kp, F)
    x, y = kp[:, 0].astype(np.float64), kp[:, 1].astype(np.float64)
    half = kp[:, 2].astype(np.float64) / 2 if not radius else np.full(len(kp), float(radius) / 2)
    return np.stack([x - half, y - half, x + half, y + half], 1).astype(F)


def bad_rows(kp, radius):
    kp = np.asarray(kp, F)
    bad = ~np.isfinite(kp[:, :3]).all(1)
    if not radius:
        bad |= kp[:, 2] < 0
    return bad


def make_order(scores):
    """Descending score, equal scores with the higher row first; rows with a non-finite score are left out."""
    s = np.asarray(scores, F)
    o = np.argsort(s, kind="stable")[::-1]
    return o[np.isfinite(s[o])].astype(np.int64)


def _derived(box):
    x1, y1, x2, y2 = (box[:, k] for k in range(4))
    with np.errstate(all="ignore"):                        # bad rows carry NaN / inf; they are never looked at
        return (x2 - x1 + F(1)) * (y2 - y1 + F(1)), (x1 + x2) / F(2), (y1 + y2) / F(2)


def survives(box, area, cx, cy, i, o, thr):
    """o (an index array) against the kept keypoint i: True where o survives.  float32 throughout, one rounding per operation."""
    with np.errstate(all="ignore"):
        w = np.maximum(F(0), np.minimum(box[i, 2], box[o, 2]) - np.maximum(box[i, 0], box[o, 0]) + F(1))
        h = np.maximum(F(0), np.minimum(box[i, 3], box[o, 3]) - np.maximum(box[i, 1], box[o, 1]) + F(1))
        inter = w * h
        iou = inter / ((area[i] + area[o]) - inter)
        ex = np.maximum(box[i, 2], box[o, 2]) - np.minimum(box[i, 0], box[o, 0])
        ey = np.maximum(box[i, 3], box[o, 3]) - np.minimum(box[i, 1], box[o, 1])
        diag = ex * ex + ey * ey
        dx, dy = cx[i] - cx[o], cy[i] - cy[o]
        cd = dx * dx + dy * dy
        diou = iou - cd / (diag + F(1e-10))
        assert diou.dtype == F
        return diou <= F(thr)


def sequential(box, order, thr):
    """The greedy rule over the rows of ``order`` (all valid): the kept rows, in processing order."""
    area, cx, cy = _derived(box)
    alive = np.asarray(order, np.int64)
    kept = []
    while alive.size:
        i, rest = alive[0], alive[1:]
        kept.append(int(i))
        alive = rest[survives(box, area, cx, cy, i, rest, thr)]
    return kept


def rounds(box, order, thr):
    """The parallel form: (kept rows in processing order, number of rounds).  Every round reads the statuses of the round before."""
    area, cx, cy = _derived(box)
    order = np.asarray(order, np.int64)
    m = len(order)
    J, Q = [], []                                          # position j does not survive the earlier position q
    for j in range(1, m):
        q = np.nonzero(~survives(box, area, cx, cy, order[j], order[:j], thr))[0]
        J.append(np.full(len(q), j))
        Q.append(q)
    J = np.concatenate(J) if J else np.zeros(0, np.int64)
    Q = np.concatenate(Q) if Q else np.zeros(0, np.int64)
    status = np.zeros(m, np.int8)                          # 0 undecided, 1 kept, 2 suppressed
    n_rounds = 0
    while (status == 0).any():
        has_kept = np.bincount(J[status[Q] == 1], minlength=m) > 0
        has_open = np.bincount(J[status[Q] == 0], minlength=m) > 0
        und = status == 0
        new = status.copy()
        new[und & has_kept] = 2
        new[und & ~has_kept & ~has_open] = 1
        status = new
        n_rounds += 1
    return [int(r) for r in order[status == 1]], n_rounds


def map_back(box, rows, among):
    """Each row replaced by the lowest row of ``among`` with the same four corners."""
    among = np.sort(np.asarray(among, np.int64))
    out = []
    for r in rows:
        same = (box[among] == box[r]).all(1)
        out.append(int(among[same][0]))
    return out


def process(kp, scores, radius, thr, form=sequential):
    """One image: the rows process_diou_nms returns, in its order."""
    box = boxes(kp, radius)
    bad = bad_rows(kp, radius)
    order = make_order(scores)
    order = order[~bad[order]]
    kept = form(box, order, thr)
    kept = kept[0] if isinstance(kept, tuple) else kept
    return map_back(box, kept, order)


def run_op(kp4, order, offsets, radius, thr):
    """The op on a batch: (keep int32 [n], count int32 [n_images + 1]) as include/gims_hip.h describes them."""
    kp4, order, offsets = np.asarray(kp4, F).reshape(-1, 4), np.asarray(order, np.int64), np.asarray(offsets, np.int64)
    n = len(kp4)
    box, bad = boxes(kp4, radius), bad_rows(kp4, radius)
    keep = np.full(n, -1, np.int32)
    count = np.zeros(len(offsets), np.int32)
    off = np.clip(offsets, 0, n)
    for b in range(len(offsets) - 1):
        o0, o1 = off[b], max(off[b], off[b + 1])
        seg = order[o0:o1]
        inside = (seg >= o0) & (seg < o1)
        valid = inside.copy()
        valid[inside] &= ~bad[seg[inside]]
        count[-1] += int((~valid).sum())
        rows = map_back(box, sequential(box, seg[valid], thr), seg[valid])
        keep[o0:o0 + len(rows)] = rows
        count[b] = len(rows)
    return keep, count


# ------------------------------------------------------------------------------------------------------------------------ fixtures
# name, recipe, the count the reference's function returned when the goldens were generated
FIXTURES = [
    ("nms_uniform_r4", {"kind": "uniform", "n": 3000, "width": 320, "height": 240, "seed": 3, "radius": 4, "thr": 0.3}, 2426),
    ("nms_uniform_size", {"kind": "uniform", "n": 3000, "width": 320, "height": 240, "seed": 3, "radius": 0, "thr": 0.3}, 2439),
    ("nms_uniform_r8", {"kind": "uniform", "n": 3000, "width": 320, "height": 240, "seed": 3, "radius": 8, "thr": 0.1}, 1060),
    ("nms_dense_r4", {"kind": "uniform", "n": 2000, "width": 100, "height": 80, "seed": 3, "radius": 4, "thr": 0.3}, 781),
    ("nms_chain", {"kind": "chain", "n": 2048, "width": 4200, "height": 16, "seed": 3, "radius": 4, "thr": 0.3}, 1024),
    ("nms_duplicates", {"kind": "duplicates", "n": 300, "width": 320, "height": 240, "seed": 3, "radius": 4, "thr": 0.3}, 291),
    ("nms_detector_r4", {"kind": "detector", "width": 320, "height": 240, "seed": 7, "radius": 4, "thr": 0.3}, 265),
    ("nms_detector_size", {"kind": "detector", "width": 320, "height": 240, "seed": 7, "radius": 0, "thr": 0.3}, 267),
    ("nms_detector_r8", {"kind": "detector", "width": 320, "height": 240, "seed": 7, "radius": 8, "thr": 0.3}, 265),
]


def build_fixture(recipe):
    """(kp float32 [n, 3] = x, y, size; scores float32 [n]).  Scores are distinct except where the recipe says otherwise."""
    kind = recipe["kind"]
    rng = np.random.default_rng(recipe["seed"])
    if kind == "detector":
        from gims_amd import synth
        from tests import sift_ref
        k = sift_ref.detect(synth.make_textured_image(recipe["height"], recipe["width"], recipe["seed"]))
        return np.concatenate([k["pt"], k["size"][:, None]], 1).astype(F), k["response"].astype(F)
    n = recipe["n"]
    if kind == "chain":                                    # collinear, 2 px apart, descending scores: every decision waits for the one before
        kp = np.stack([10 + 2.0 * np.arange(n), np.full(n, 8.0), np.full(n, 3.0)], 1).astype(F)
        return kp, (np.arange(n, 0, -1) / n).astype(F)
    x, y = rng.random(n) * recipe["width"], rng.random(n) * recipe["height"]
    size = np.exp(rng.normal(1.2, 0.7, n)) + 1.5
    kp = np.stack([x, y, size], 1).astype(F)
    scores = (rng.permutation(n) + 1).astype(F) / F(n)
    if kind == "duplicates":                               # every fifth row again, right after the original: same point, size and score
        rep = np.sort(np.concatenate([np.arange(n), np.arange(0, n, 5)]), kind="stable")
        kp, scores = kp[rep], scores[rep]
    return kp, scores
