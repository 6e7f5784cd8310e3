"""Seeded adversarial inputs for the evaluation kernels (csrc/eval.hip) and what the CPU oracle makes of them -- TEST INFRASTRUCTURE.

Every builder returns ``(spec, extra)``: ``spec = (kp0, kp1, matches0, mscores0, H, height, width)`` in NumPy, the order the
GPU tests upload, and ``extra`` a dict of whatever the case's conditions need.  ``expected`` turns a spec into the outputs of
``gims_eval_pairs`` through the public functions of oracle/eval_oracle.py alone.  tests/test_eval_cases_cpu.py asserts, without
a GPU, that every case is as adversarial as its docstring says; tests/test_eval_edges_gpu.py and test_labels_edges_gpu.py run
them on the device.  Builders and oracle results are cached: a test reads them and leaves them unchanged."""
import functools

import numpy as np
import torch

from gims_amd import synth
from oracle import eval_oracle as E

F32 = np.float32
TRANSLATE = lambda dx, dy: np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1]], dtype=F32)      # noqa: E731
THRESH_UP = float(np.nextafter(F32(3), F32(4)))
SENTINEL = np.array([11.5, -12.25, 13.0, 1e30, -0.0], dtype=F32)            # what the caller leaves in record columns 11-15


def _no_matches(n0):
    return np.full(n0, -1, dtype=np.int64), np.zeros(n0, dtype=F32)


# ------------------------------------------------------------------------------------------------ 1. distance ties
LATTICE_CASES = {"a": dict(nx=40, ny=30, spacing=2, n0=1200, n1=1100, seed=4101),       # the full lattice against 1100 of its points
                 "b": dict(nx=40, ny=30, spacing=2, n0=700, n1=1200, seed=4102)}        # n0 < n1, both permuted
LATTICE_SHIFTS = {"x": (1, 0), "xy": (1, 1), "id": (0, 0)}
TIE_GOLDENS = {"eval_tie_a_x": ("a", "x"), "eval_tie_b_xy": ("b", "xy")}               # tools/gen_golden_eval.py
TIE_ITERS = (1, 2, 3, 6)


def lattice_points(nx, ny, spacing, n0, n1, seed):
    """An nx x ny lattice of integer coordinates (offset 10 px): image 0 holds its first n0 points of one permutation (the whole lattice in
    order when n0 = nx * ny), image 1 n1 points of another permutation."""
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny))
    pts = (np.stack([gx.ravel(), gy.ravel()], 1) * spacing + 10).astype(F32)
    r = np.random.default_rng(seed)
    kp0 = pts if n0 == len(pts) else pts[r.permutation(len(pts))[:n0]]
    kp1 = pts[r.permutation(len(pts))[:n1]]
    return np.ascontiguousarray(kp0), np.ascontiguousarray(kp1)


@functools.lru_cache(maxsize=None)
def lattice_case(name, shift):
    """Under a shift of half the spacing every projected point is equidistant from two (x) or four (xy) lattice neighbours: only the
    first-minimum rule decides, and later iterations keep finding matches."""
    c = LATTICE_CASES[name]
    kp0, kp1 = lattice_points(**c)
    m0, s0 = _no_matches(len(kp0))
    h, w = 10 + c["ny"] * c["spacing"] + 10, 10 + c["nx"] * c["spacing"] + 10
    return (kp0, kp1, m0, s0, TRANSLATE(*LATTICE_SHIFTS[shift]), h, w), dict(c)


def golden_gt0(g, n_iters, n0):
    """gt0 after n_iters iterations from an eval_tie_* fixture (the reference appends iteration after iteration)."""
    n = int(g["n_after"][list(g["iters"]).index(n_iters)])
    gt = np.full(n0, -1, dtype=np.int64)
    gt[g["ma0"][:n]] = g["ma1"][:n]
    return gt


def ref_distances(kp0, kp1, H):
    """The reference's float32 distance matrix between warp(kp0) and kp1 (torch_cdist)."""
    proj = E.warp_keypoints(torch.from_numpy(kp0), torch.from_numpy(np.asarray(H, F32)))
    b = torch.from_numpy(kp1)
    return torch.sqrt(((proj[:, None, :] - b[None, :, :]) ** 2).sum(-1)).numpy()


def first_min_gt_matches(kp0, kp1, H, dist_thresh, n_iters):
    """torch_find_matches restated on the whole matrix with np.argmin (first minimum) and alive masks: gt0 [n0], -1 = none."""
    d = ref_distances(kp0, kp1, H)
    n0, n1 = d.shape
    alive0, alive1 = np.ones(n0, bool), np.ones(n1, bool)
    gt0 = np.full(n0, -1, dtype=np.int64)
    thr = F32(dist_thresh)
    for _ in range(n_iters):
        if not alive0.any() or not alive1.any():
            break
        m = np.where(alive0[:, None] & alive1[None, :], d, F32(np.inf))
        min1, min2 = np.argmin(m, 1), np.argmin(m, 0)
        for j in np.nonzero(alive1)[0]:
            i = min2[j]
            if alive0[i] and min1[i] == j and d[i, j] < thr:
                gt0[i] = j
        alive0[gt0 >= 0] = False
        alive1[gt0[gt0 >= 0]] = False
    return gt0


# ------------------------------------------------------------------------------------------------ 2. strict threshold
@functools.lru_cache(maxsize=None)
def threshold_case():
    """10 x 10 lattice of spacing 10 against itself (permuted) under translate(3, 0): every nearest distance is exactly 3.0."""
    gx, gy = np.meshgrid(np.arange(10), np.arange(10))
    kp0 = (np.stack([gx.ravel(), gy.ravel()], 1) * 10).astype(F32)
    perm = np.random.default_rng(4201).permutation(100)
    m0, s0 = _no_matches(100)
    return (kp0, np.ascontiguousarray(kp0[perm]), m0, s0, TRANSLATE(3, 0), 100, 100), dict(perm=perm)


T21 = F32(2.1)                                                                          # 2.1 rounded to float32 (below 2.1)
T21_OFFSETS = np.array([2.0, np.nextafter(T21, F32(0)), T21, np.nextafter(T21, F32(3)), 2.2, 1.0, 2.5, 2.0999, 2.1001, 0.0], dtype=F32)


@functools.lru_cache(maxsize=None)
def threshold21_case():
    """The same lattice under the identity, image-1 point i moved right by T21_OFFSETS[i % 10]: the column x = 0 has distances of exactly
    float32(2.1) and its two float32 neighbours, the other columns distances on both sides of it."""
    gx, gy = np.meshgrid(np.arange(10), np.arange(10))
    kp0 = (np.stack([gx.ravel(), gy.ravel()], 1) * 10).astype(F32)
    kp1 = kp0.copy()
    kp1[:, 0] = kp1[:, 0] + T21_OFFSETS[gy.ravel() % 10]
    perm = np.random.default_rng(4202).permutation(100)
    m0, s0 = _no_matches(100)
    return (kp0, np.ascontiguousarray(kp1[perm]), m0, s0, TRANSLATE(0, 0), 100, 100), dict(perm=perm)


# ------------------------------------------------------------------------------------------------ 3. compaction across chunks
COMPACTION = [(1023, "all", 500), (1025, "all", 1001), (2049, "all", 500), (2500, "all", 3000), (2500, "tail", 500),
              (1025, "seventh", 500), (2049, "seventh", 1001), (2500, "seventh", 500)]          # (n0, pattern, ransac_iters)
RANSAC_SEED = 99


def _planted(n0, seed):
    """A plausible matcher output on a planted homography: the planted partner for nine in ten keypoints, a wrong one for the rest;
    confidences above 0.5 for the right ones, below for the wrong ones, no two equal."""
    pair, H = synth.make_homography_pair(n0, seed, pos_noise=0.5, outlier_frac=0.0)
    kp0, kp1, gt = pair["keypoints0"][0], pair["keypoints1"][0], pair["gt_perm"]
    r = np.random.default_rng(seed)
    m0 = gt.astype(np.int64).copy()
    wrong = r.random(n0) < 0.1
    m0[wrong] = r.integers(0, n0, size=int(wrong.sum()))
    s0 = (0.5 + 0.5 * r.random(n0)).astype(F32)
    s0[wrong] *= F32(0.5)
    w, h = synth.canvas_for(n0)
    return kp0, kp1, m0, s0, H, h, w


def _valid_pattern(n0, pattern):
    i = np.arange(n0)
    if pattern == "all":
        return np.ones(n0, bool)
    if pattern == "tail":                                          # the first chunk contributes nothing: base stays 0 across it
        return i >= 1030
    if pattern == "seventh":                                       # sparse, plus both sides of every chunk boundary
        return (i % 7 == 0) | (i % 1024 == 1023) | ((i % 1024 == 0) & (i > 0))
    raise KeyError(pattern)


@functools.lru_cache(maxsize=None)
def compaction_case(n0, pattern):
    kp0, kp1, m0, s0, H, h, w = _planted(n0, 4300 + n0)
    valid = _valid_pattern(n0, pattern)
    m0 = np.where(valid, m0, -1)
    return (kp0, kp1, m0, s0, H, h, w), dict(K=int(valid.sum()), top4=np.argsort(-s0[valid].astype(np.float64), kind="stable")[:4],
                                             valid_idx=np.nonzero(valid)[0])


# ------------------------------------------------------------------------------------------------ 4. score ties
SCORE_TIES = [(1023, "all", "ones"), (1025, "seventh", "ones"), (2049, "all", "ones"), (2500, "seventh", "ones"),
              (1023, "all", "classes"), (1025, "all", "classes"), (2049, "all", "classes"), (2500, "all", "classes"), (2500, "tail", "classes")]
# positions in the list of valid matches that get the top score: the first four sit in different waves and, for 2049 and 2500, in two
# chunks of 1024 (for 1023 and 1025 all four are in chunk 0; 1024 only has to lose); 70 / 1094 / 2118 belong to the same thread of the
# counts kernel, the others to other lanes and waves
TOP_POSITIONS = {1023: [5, 64, 300, 700, 701, 900, 1000, 1022], 1025: [5, 300, 700, 1024, 64 + 7, 900],
                 2049: [70, 900, 1030, 1094, 1500, 2040, 2048, 130 + 1024], 2500: [70, 130, 900, 1030, 1094, 2118, 2200, 2499]}


@functools.lru_cache(maxsize=None)
def score_tie_case(n0, pattern, kind):
    """Confidences that tie: all 1.0 ("ones": the four most confident are the first four valid matches) or drawn from {0.25, 0.5, 1.0}
    ("classes": the first four of the 1.0 class, planted at TOP_POSITIONS)."""
    (kp0, kp1, m0, _, H, h, w), ex = compaction_case(n0, pattern)
    valid_idx = ex["valid_idx"]
    if kind == "ones":
        s0 = np.ones(n0, dtype=F32)
        tied = np.arange(len(valid_idx))
    else:
        s0 = np.random.default_rng(4400 + n0).choice(np.array([0.25, 0.5], dtype=F32), size=n0)
        tied = np.array(sorted(p for p in TOP_POSITIONS[n0] if p < len(valid_idx)))
        s0[valid_idx[tied]] = F32(1.0)
    return (kp0, kp1, m0, s0, H, h, w), dict(K=len(valid_idx), tied=tied, valid_idx=valid_idx)


# ------------------------------------------------------------------------------------------------ 5. few or degenerate matches
def _small_pair(n0, n1, seed):
    """Keypoints on a small canvas (coordinates below 64, so that even the normal equations of four points are well conditioned),
    image 1 = image 0 under a mild homography, permuted, with 0.05 px of noise; planted partner list."""
    r = np.random.default_rng(seed)
    w, h = 64, 48
    H = synth.make_homography(seed, (w, h))
    n = max(n0, n1)
    a = (r.random((n, 2)) * [w, h]).astype(F32)
    b = E.perspective_transform(a, H) + 0.05 * r.standard_normal((n, 2))
    perm = r.permutation(n)[:n1]                                   # image1[j] = warp(a[perm[j]])
    kp0, kp1 = np.ascontiguousarray(a[:n0]), np.ascontiguousarray(b[perm].astype(F32))
    part = np.full(n, -1, dtype=np.int64)
    part[perm] = np.arange(n1)
    return kp0, kp1, part[:n0], H, h, w


def _few(n0, n1, k, seed):
    kp0, kp1, part, H, h, w = _small_pair(n0, n1, seed)
    m0 = np.full(n0, -1, dtype=np.int64)
    have = np.nonzero(part >= 0)[0]
    sel = have[np.linspace(0, len(have) - 1, k).astype(int)] if k else have[:0]
    m0[sel] = part[sel]
    s0 = np.random.default_rng(seed + 1).random(n0).astype(F32)
    return (kp0, kp1, m0, s0, H, h, w)


@functools.lru_cache(maxsize=None)
def degenerate_batch():
    """K = 0, 1, 3, 4, 5 valid matches on n0 = 300; n0 = 1 against n1 = 700 and the reverse; eight copies of one keypoint pair; three
    distinct pairs three times each.  Returns ({name: spec}, {name: K}).

    The last two hold exactly singular samples only: every 8 x 8 system has two pairs of identical rows.  The elimination (LAPACK's in the
    oracle, solve8 in the kernel) reports that when the duplicate row cancels to an exact zero, which it does when pivot * (1 / pivot) rounds
    to 1 -- true for most values, not all (about four data seeds in ten leave a residue of one ulp and a meaningless model).  The seeds
    here are ones for which the oracle finds no model in any hypothesis; tests/test_eval_cases_cpu.py asserts that."""
    specs = {f"k{k}": _few(300, 300, k, 4500 + k) for k in (0, 1, 3, 4, 5)}
    specs["n0_1"] = _few(1, 700, 1, 4510)
    kp0, kp1, part, H, h, w = _small_pair(700, 1, 4511)
    m0 = np.full(700, -1, dtype=np.int64)
    m0[[int(np.nonzero(part >= 0)[0][0]), 699]] = 0               # the planted partner and a wrong keypoint both claim the one point
    specs["n1_1"] = (kp0, kp1, m0, np.random.default_rng(4512).random(700).astype(F32), H, h, w)
    # eight coincident keypoints in both images, i -> distinct but coincident j
    kp0, kp1, part, H, h, w = _small_pair(300, 300, 4513)
    i8, j8 = np.arange(10, 90, 10), np.arange(295, 215, -10)
    kp0, kp1 = kp0.copy(), kp1.copy()
    kp0[i8], kp1[j8] = kp0[10], kp1[part[10]]
    m0 = np.full(300, -1, dtype=np.int64)
    m0[i8] = j8
    specs["dup8"] = (kp0, kp1, m0, np.random.default_rng(4514).random(300).astype(F32), H, h, w)
    # three distinct pairs, each three times
    kp0, kp1, part, H, h, w = _small_pair(300, 300, 4517)
    kp0, kp1 = kp0.copy(), kp1.copy()
    i9, j9 = np.arange(20, 290, 30), np.arange(281, 11, -30)
    src0, src1 = kp0[i9[:3]].copy(), kp1[part[i9[:3]]].copy()
    for c in range(9):
        kp0[i9[c]], kp1[j9[c]] = src0[c % 3], src1[c % 3]
    m0 = np.full(300, -1, dtype=np.int64)
    m0[i9] = j9
    specs["three3"] = (kp0, kp1, m0, np.random.default_rng(4516).random(300).astype(F32), H, h, w)
    return specs, {k: int((v[2] > -1).sum()) for k, v in specs.items()}


@functools.lru_cache(maxsize=None)
def ordinary_pairs():
    """Two pairs the summary keeps: more than 12 matches and both models."""
    out = []
    for seed in (4520, 4521):
        kp0, kp1, m0, s0, H, h, w = _planted(300, seed)
        m0 = m0.copy()
        m0[::5] = -1
        out.append((kp0, kp1, m0, s0, H, h, w))
    return out


# ------------------------------------------------------------------------------------------------ 6. two models, tied hypotheses
TWO_MODEL_ITERS = 8192
MODEL_A, MODEL_B = (7, -3), (-20, 11)


def _general_position(r, n, size):
    """n distinct integer points in [0, size)^2, no three on a line (so that no four of them give a rank-deficient system)."""
    pts = []
    while len(pts) < n:
        p = r.integers(0, size, 2)
        ok = all((p != q).any() for q in pts)
        for a in range(len(pts)):
            for b in range(a + 1, len(pts)):
                u, v = pts[a] - p, pts[b] - p
                ok = ok and u[0] * v[1] - u[1] * v[0] != 0
        if ok:
            pts.append(p)
    return np.array(pts)


def two_model_data(seed):
    """100 matches (i -> perm[i]) on integer keypoints of a 64 px canvas: 0-14 follow translate(7, -3) exactly, 15-29 translate(-20, 11),
    the rest are outliers at more than 6 px from both models."""
    r = np.random.default_rng(seed)
    size = 64
    g = _general_position(r, 30, size)
    src = np.zeros((100, 2), dtype=np.int64)
    dst = np.zeros((100, 2), dtype=np.int64)
    src[:30] = g
    dst[:15], dst[15:30] = g[:15] + MODEL_A, g[15:] + MODEL_B
    k = 30
    while k < 100:
        p, q = r.integers(0, size, 2), r.integers(-20, size + 20, 2)
        if all(((p + np.array(t) - q) ** 2).sum() > 36 for t in (MODEL_A, MODEL_B)):
            src[k], dst[k] = p, q
            k += 1
    perm = r.permutation(100)
    kp1 = np.zeros((100, 2), dtype=F32)
    kp1[perm] = dst
    s0 = r.random(100).astype(F32)
    H = TRANSLATE(*MODEL_A)
    return (src.astype(F32), kp1, perm.astype(np.int64), s0, H, size, size)


def hypothesis_classes(seed, iters=TWO_MODEL_ITERS, k=100, g=15):
    """Hypotheses whose four samples all lie in matches [0, g) (a) or in [g, 2g) (b): E.ransac_sample alone."""
    a, b = [], []
    for h in range(iters):
        s = E.ransac_sample(seed, h, k)
        if (s < g).all():
            a.append(h)
        elif ((s >= g) & (s < 2 * g)).all():
            b.append(h)
    return a, b


def _tie_crosses_stride(a, b):
    if not a or not b:
        return None
    first = min(a[0], b[0])
    other = b if first == a[0] else a
    later = [h for h in other if h > first and h % 1024 < first % 1024]
    return (first, later[0]) if first >= 1024 and later else None


def finish_reduction(counts, flip_lane=False, flip_wave=False):
    """The three levels by which eval_ransac_finish_kernel picks the best hypothesis from the per-hypothesis inlier counts, restated: every
    one of 1024 threads keeps the first best of its strided list h = t, t + 1024, ...; the 64 lanes of a wave reduce with "more inliers, or as
    many and the lower hypothesis index"; thread 0 merges the 16 waves with the same rule.  `flip_lane` / `flip_wave` turn "lower" into
    "higher" at that level: what a wrong tie-break there would return."""
    bc, bh = np.full(1024, -1, dtype=np.int64), np.full(1024, 0x7fffffff, dtype=np.int64)
    for h, c in enumerate(counts):
        if c > bc[h % 1024]:
            bc[h % 1024], bh[h % 1024] = c, h

    def reduce(cs, hs, flip):                # the rule is a total order on distinct (count, index) pairs: any reduction tree gives the same
        c, h = cs[0], hs[0]
        for oc, oh in zip(cs[1:], hs[1:]):
            if oc > c or (oc == c and (oh > h if flip else oh < h)):
                c, h = oc, oh
        return c, h

    waves = [reduce(bc[w * 64:(w + 1) * 64], bh[w * 64:(w + 1) * 64], flip_lane) for w in range(16)]
    return int(reduce([w[0] for w in waves], [w[1] for w in waves], flip_wave)[1])


def two_model_conditions(seed):
    """For a RANSAC seed: the pure hypotheses of both models and, taking them as the tied best (15 inliers each, everything else fewer: the
    CPU test checks that with the oracle), what the kernel's reduction and its three wrong variants return.  None if the seed does not fit:
    h* >= 1024, a later pure hypothesis h' of the other model in a lower slot of the 1024 stride, and the OTHER model from the reduction with
    the tie-break flipped in the lanes, in the wave merge, or in both."""
    a, b = hypothesis_classes(seed)
    hit = _tie_crosses_stride(a, b)
    if not hit:
        return None
    counts = np.zeros(TWO_MODEL_ITERS, dtype=np.int64)
    counts[a + b] = 15
    star_is_a = hit[0] == a[0]
    wrong = [finish_reduction(counts, *f) for f in ((True, False), (False, True), (True, True))]
    if finish_reduction(counts) != hit[0] or any((h in a) == star_is_a for h in wrong):
        return None
    return dict(seed=seed, a=a, b=b, h_star=hit[0], h_other=hit[1], star_is_a=star_is_a, wrong=wrong)


def search_two_model_seed(first=1, last=200):
    """The lowest RANSAC seed that two_model_conditions accepts (how TWO_MODEL_SEED was found; about half a second per seed)."""
    for seed in range(first, last):
        if two_model_conditions(seed):
            return seed
    raise AssertionError("no RANSAC seed in range fits")


TWO_MODEL_SEED, TWO_MODEL_HSTAR, TWO_MODEL_STAR_IS_A = 4, 1970, False        # search_two_model_seed(); checked in tests/test_eval_cases_cpu.py


@functools.lru_cache(maxsize=None)
def two_model_case():
    """The two-model data with the pinned RANSAC seed: the first pure hypothesis h* >= 1024 belongs to one model; pure hypotheses of the other
    model sit (a) later but in a lower slot of the 1024-strided scan, (b) in h*'s own 64-lane group and in the other waves such that a
    flipped tie-break in the lane reduction, in the wave merge, or in both returns the other model."""
    return two_model_data(1), dict(seed=TWO_MODEL_SEED, h_star=TWO_MODEL_HSTAR, star_is_a=TWO_MODEL_STAR_IS_A)


def hypothesis_counts(spec, seed, iters, thresh=3.0):
    """The oracle's inlier count of every hypothesis (-1: no model), as ransac_homography scores them."""
    kp0, kp1, m0 = spec[0], spec[1], spec[2]
    valid = m0 > -1
    p0, p1 = kp0[valid], kp1[m0[valid]]
    out = np.full(iters, -1, dtype=np.int64)
    for h in range(iters):
        s = E.ransac_sample(seed, h, len(p0))
        try:
            Hh = E.homography_from_4(p0[s], p1[s])
        except np.linalg.LinAlgError:
            continue
        if np.isfinite(Hh).all():
            with np.errstate(all="ignore"):
                out[h] = int((E.reproj_error2(Hh, p0, p1) <= float(thresh) ** 2).sum())
    return out


# ------------------------------------------------------------------------------------------------ 7. ragged batch
@functools.lru_cache(maxsize=None)
def ragged_batch():
    """n0 / n1 = 5 / 2500, 2500 / 5, 1025 / 700, 64 / 65, 300 / 300: planted, lattice and degenerate inputs mixed."""
    kp0, kp1, m0, s0, H, h, w = compaction_case(2500, "all")[0]
    a = (np.ascontiguousarray(kp0[:5]), kp1, m0[:5].copy(), s0[:5].copy(), H, h, w)
    m = np.where(m0 < 5, m0, -1)
    m[np.nonzero(m < 0)[0][::3]] = 4                               # many keypoints claim the same few points of image 1
    b = (kp0, np.ascontiguousarray(kp1[:5]), m, s0, H, h, w)
    kp0, kp1, m0, s0, H, h, w = score_tie_case(1025, "all", "classes")[0]
    c = (kp0, np.ascontiguousarray(kp1[:700]), np.where(m0 < 700, m0, -1), s0, H, h, w)
    kp0, kp1, _, _, H, h, w = lattice_case("a", "x")[0]
    r = np.random.default_rng(4700)
    d = (np.ascontiguousarray(kp0[:64]), np.ascontiguousarray(kp0[:65] + F32(1)), r.integers(-1, 65, 64).astype(np.int64),
         np.ones(64, dtype=F32), H, h, w)
    e = degenerate_batch()[0]["three3"]
    return [a, b, c, d, e]


# ------------------------------------------------------------------------------------------------ labels
@functools.lru_cache(maxsize=None)
def label_batch():
    """(kp0 list, kp1 list, H list, names) for gims_train_labels: lattice ties, one-point images, sizes around the 1024-row chunk of the
    row compaction, an identity pair where everything matches and a far translation where nothing does."""
    k0, k1, hs, names = [], [], [], []

    def add(name, a, b, H):
        k0.append(np.ascontiguousarray(a, dtype=F32)), k1.append(np.ascontiguousarray(b, dtype=F32)), hs.append(np.asarray(H, F32)), names.append(name)

    for name, shift in (("a", "x"), ("b", "xy")):
        s = lattice_case(name, shift)[0]
        add(f"lattice_{name}_{shift}", s[0], s[1], s[4])
    for n0, n1 in ((1, 700), (700, 1), (1023, 1025), (2049, 1024)):
        n = max(n0, n1)
        pair, H = synth.make_homography_pair(n, 4800 + n0, pos_noise=0.7)
        add(f"n{n0}_{n1}", pair["keypoints0"][0][:n0], pair["keypoints1"][0][:n1], H)
    pair, _ = synth.make_homography_pair(1100, 4810, pos_noise=0.0)
    perm = np.random.default_rng(4811).permutation(1100)
    add("identity", pair["keypoints0"][0], pair["keypoints0"][0][perm], TRANSLATE(0, 0))
    add("far", pair["keypoints0"][0][:600], pair["keypoints0"][0][:500], TRANSLATE(10000, 0))
    return k0, k1, hs, names


# ------------------------------------------------------------------------------------------------ oracle -> expected outputs
def expected(spec, dist_thresh=3.0, n_iters=3, ransac_thresh=3.0, ransac_iters=3000, seed=0):
    """What gims_eval_pairs must return for one pair: gt0 [n0] int64, record [11] float64, homographies [2, 3, 3], inlier [n0] bool.
    "No model" (LinAlgError, non-finite entries, None, fewer than four matches, no hypotheses) is ok = 0, error -1, nine zeros."""
    kp0, kp1, m0, s0, H, h, w = spec
    n0 = len(kp0)
    H = np.asarray(H, F32)
    ma0, ma1, _, _ = E.find_gt_matches(torch.from_numpy(kp0), torch.from_numpy(kp1), torch.from_numpy(H), dist_thresh, n_iters)
    with np.errstate(all="ignore"):
        prec, rcl, gt = E.precision_recall(m0, ma0, ma1)
    valid = m0 > -1
    K = int(valid.sum())
    mk0, mk1, mc = kp0[valid], kp1[m0[valid]], s0[valid]
    rec = np.zeros(11)
    rec[0], rec[1] = K, len(ma0)
    rec[2] = int((m0[ma0] == ma1).sum())
    rec[3] = int(((m0 != gt) & (m0 == -1)).sum())
    rec[4], rec[5] = prec, rcl
    homs = np.zeros((2, 3, 3))
    inlier = np.zeros(n0, bool)
    Hd = None
    if K >= 4:
        try:
            Hd = E.dlt_top4(mk0, mk1, mc)
            Hd = Hd if np.isfinite(Hd).all() else None
        except np.linalg.LinAlgError:
            Hd = None
    rec[9], rec[7] = (1, E.corner_error(Hd, H, h, w)) if Hd is not None else (0, -1)
    if Hd is not None:
        homs[0] = Hd
    Hr, mask = (E.ransac_homography(mk0, mk1, seed=seed, iters=ransac_iters, thresh=ransac_thresh) if K >= 4 else (None, None))
    if Hr is not None:
        rec[10], rec[8], rec[6] = 1, E.corner_error(Hr, H, h, w), int(mask.sum())
        homs[1] = Hr
        inlier[np.nonzero(valid)[0][mask]] = True
    else:
        rec[10], rec[8], rec[6] = 0, -1, 0
    return dict(gt0=gt, record=rec, homographies=homs, inlier=inlier, K=K, Hd=Hd, Hr=Hr)


def threshold_margin(spec, Hr, ransac_thresh=3.0):
    """Smallest relative distance of a match's squared reprojection error under Hr from t^2 (the GPU tests assert inlier masks exactly)."""
    kp0, kp1, m0 = spec[0], spec[1], spec[2]
    valid = m0 > -1
    t2 = float(ransac_thresh) ** 2
    with np.errstate(all="ignore"):
        e = E.reproj_error2(Hr, kp0[valid], kp1[m0[valid]])
    return float(np.nanmin(np.abs(e - t2)) / t2)


@functools.lru_cache(maxsize=None)
def compaction_expected(n0, pattern, iters):
    return expected(compaction_case(n0, pattern)[0], ransac_iters=iters, seed=RANSAC_SEED)


@functools.lru_cache(maxsize=None)
def score_tie_expected(n0, pattern, kind):
    return expected(score_tie_case(n0, pattern, kind)[0], ransac_iters=0)


@functools.lru_cache(maxsize=None)
def degenerate_expected(iters=500):
    return {k: expected(v, ransac_iters=iters, seed=RANSAC_SEED) for k, v in degenerate_batch()[0].items()}


@functools.lru_cache(maxsize=None)
def two_model_expected(high_bit):
    spec, ex = two_model_case()
    return expected(spec, ransac_iters=TWO_MODEL_ITERS, seed=ex["seed"] | (1 << 63 if high_bit else 0))
