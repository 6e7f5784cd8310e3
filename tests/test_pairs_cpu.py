"""CPU tests of the pair selection: the ABI constant and the pins a feature must leave alone, the argument checks of GIMS_AUX_SELECT_PAIRS
(they run before any HIP call), the ValueErrors of gims_amd.select_pairs, the host-side layouts of hip.py against an independent
restatement, the NumPy restatement (tests/pairs_ref.py) against a brute-force second implementation, and the ring fixture that shows what
the feature is for."""
import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import pairs_ref as R


def test_abi_constant_and_pins():
    assert hip.AUX_SELECT_PAIRS == 17 == hip.ABI.constants["GIMS_AUX_SELECT_PAIRS"]
    # the feature adds no export, no struct and no ABI version
    assert len(hip.EXPORTS) == 90 and len(hip.ABI.structs) == 28 and hip.ABI_VERSION == 5 == hip.load().gims_abi_version()
    # (two exports from before this op carry "pairs" in their name; the op adds none, under that word or its own)
    assert sorted(name for name in hip.EXPORTS if "pairs" in name.lower()) == ["gims_eval_pairs", "gims_verify_pairs"]
    assert not any("select" in name.lower() for name in hip.EXPORTS)
    assert gims_amd.select_pairs is gims_amd.pairs.select_pairs and gims_amd.PairSelection is gims_amd.pairs.PairSelection
    assert "select_pairs" in gims_amd.__all__ and "PairSelection" in gims_amd.__all__
    assert (hip.PAIRS_MAX_IMAGES, hip.PAIRS_MAX_ROWS, hip.PAIRS_MAX_D, hip.PAIRS_TABLE_WORDS) == (8192, 4096, 1024, 8)
    assert hip.PAIRS_COUNTERS == R.COUNTERS
    p = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000, None]
    for fn in (12, 15, 99, -1):
        with pytest.raises(hip.GimsHipError, match=f"unknown auxiliary function {fn}"):
            with hip.on_stream(0):
                hip.run_ops(hip.make_ops([hip.op_aux(fn, p, [4, 128, 64, 2, 1, 0], (0.0,))]))


def test_argument_checks_come_before_any_hip_call():
    """Every GIMS_EINVAL case of the header, with a message naming select_pairs; the device pointers are never dereferenced (the table is
    HOST memory and is read)."""
    n, d, per = 4, 128, 64
    ms = [64, 10, 0, 33]
    need = hip.pairs_work_bytes(ms, d)
    p = [0x20000, 0x30000, 0x40000, 0x50000, None]                 # votes, out, counters, work, reserved
    good = [n, d, per, 2, 1, 0]

    def table(rq=hip.pairs_rq(0.8), flags=0, work_bytes=need, **kw):
        images = [[0x100000 * (i + 1), d, 500, 0x800000 * (i + 1), m] for i, m in enumerate(ms)]
        for i, row in kw.get("images", {}).items():
            images[i] = row
        tab = hip.pairs_table([tuple(r) for r in images], rq, work_bytes)
        tab[n, 1] = flags
        for (r, c), v in kw.get("words", {}).items():
            tab[r, c] = v
        return tab

    def refused(word, tab=None, ptrs=p, ints=good, scale=0.0, addr=None):
        tab = table() if tab is None else tab
        with pytest.raises(hip.GimsHipError, match="select_pairs") as e:
            with hip.on_stream(0):
                hip.run_ops(hip.make_ops([hip.op_aux(hip.AUX_SELECT_PAIRS, [tab.ctypes.data if addr is None else addr] + list(ptrs), ints, (scale,))]))
        assert word in str(e.value) and f"({hip.GIMS_EINVAL})" in str(e.value), str(e.value)

    def ints(**kw):
        return [kw.get(k, v) for k, v in zip(["n", "d", "per_image", "k", "min_votes", "form"], good)]

    for bad in (1, 0, -1, 8193):
        refused(f"N = {bad}", ints=ints(n=bad))
    for bad in (0, 16, 48, 100, 1056, 2048, -32):
        refused(f"D = {bad}", ints=ints(d=bad))
    refused("per_image = 4097", ints=ints(per_image=4097))
    refused("per_image = -1", ints=ints(per_image=-1))
    refused("image 0: m = 64", ints=ints(per_image=63))
    refused("image 3: m = -1", tab=table(images={3: [0x400000, d, 500, 0, -1]}))
    refused("k = 0", ints=ints(k=0))
    refused("min_votes = -1", ints=ints(min_votes=-1))
    refused("rq = -1", tab=table(rq=-1))
    refused("rq = 65537", tab=table(rq=65537))
    refused("NULL", addr=0)
    for i in range(4):
        refused("NULL", ptrs=p[:i] + [None] + p[i + 1:])
    refused("image 1: the descriptor pointer is NULL", tab=table(images={1: [0, d, 500, 0, 10]}))
    refused("8-byte aligned", addr=table().ctypes.data + 4)
    for i in range(3):
        refused("4-byte aligned", ptrs=p[:i] + [p[i] + 2] + p[i + 1:])
    refused("16-byte aligned", ptrs=p[:3] + [p[3] + 8, None])
    refused("image 0: the descriptors and the index list must be 4-byte aligned", tab=table(images={0: [0x100002, d, 500, 0, 64]}))
    refused("image 0: the descriptors and the index list must be 4-byte aligned", tab=table(images={0: [0x100000, d, 500, 0x800001, 64]}))
    refused("image 2: the row stride 127 is below D = 128", tab=table(images={2: [0x300000, 127, 500, 0, 0]}))
    refused("reserved", ints=ints(form=1))
    refused("p[5] is reserved", ptrs=p[:4] + [0x60000])
    for c in (5, 6, 7):
        refused("image 1: a reserved word", tab=table(words={(1, c): 1}))
    for c in (3, 7):
        refused("reserved word of the table's last entry", tab=table(words={(n, c): 1}))
    refused("reserved word of the table's last entry", tab=table(flags=2))
    for bad in (float("nan"), float("inf"), -1.0, -0.5):
        refused("scale must be finite and >= 0", tab=table(flags=hip.PAIRS_SCALE_GIVEN), scale=bad)
    refused("work_bytes", tab=table(work_bytes=need - 1))
    refused("work_bytes", tab=table(work_bytes=-1))
    refused("work_bytes", tab=table(flags=hip.PAIRS_SCALE_GIVEN, work_bytes=0), scale=1.0)      # a good scale passes its check
    # i[5] would select a later form of the function, so it is read first: whatever the other words hold, this version does not know the call
    with pytest.raises(hip.GimsHipError, match="unknown auxiliary function form"):
        with hip.on_stream(0):
            hip.run_ops(hip.make_ops([hip.op_aux(hip.AUX_SELECT_PAIRS, [None] * 6, [17] * 6, (float("nan"),))]))
    # the op builder
    tab = table()
    op = hip.op_select_pairs(tab, 0x20000, 0x30000, 0x40000, 0x50000, n, d, per, 2, 1, 0.5)
    a = op.u.aux
    assert op.kind == 2 and a.fn == 17 and a.p[0] == tab.ctypes.data and list(a.p)[1:] == [0x20000, 0x30000, 0x40000, 0x50000, None]
    assert list(a.i) == [n, d, per, 2, 1, 0] and a.f[0] == 0.5
    assert tab.shape == (n + 1, 8) and tab.dtype == np.int64 and tab[1].tolist() == [0x200000, d, 500, 0x1000000, 10, 0, 0, 0]
    assert tab[n].tolist() == [hip.pairs_rq(0.8), 0, need, 0, 0, 0, 0, 0]


def test_select_pairs_value_errors():
    x = lambda n=40, d=128: torch.zeros(n, d)                                  # noqa: E731
    feats = [(x(), None), (x(), None), (x(), torch.zeros(40))]
    with pytest.raises(ValueError, match="0 images"):
        gims_amd.select_pairs([])
    with pytest.raises(ValueError, match="1 images"):
        gims_amd.select_pairs(feats[:1])
    with pytest.raises(ValueError, match="D = 64, the images before it have D = 128"):
        gims_amd.select_pairs([feats[0], (x(d=64), None)])
    for d in (16, 48, 2048):
        with pytest.raises(ValueError, match=f"D = {d} is not served: the op takes a multiple of 32 in 32 .. 1024"):
            gims_amd.select_pairs([(x(d=d), None), (x(d=d), None)])
    for kw, word in ((dict(k=0), "k must"), (dict(k=1.5), "k must"), (dict(k=True), "k must"), (dict(per_image=0), "per_image"),
                     (dict(per_image=4097), "per_image"), (dict(ratio=-0.1), "ratio"), (dict(ratio=1.5), "ratio"), (dict(ratio=float("nan")), "ratio"),
                     (dict(min_votes=-1), "min_votes"), (dict(scale=float("inf")), "scale"), (dict(scale=float("nan")), "scale"),
                     (dict(scale=-1.0), "scale"), (dict(order="best"), "order must be one of")):
        with pytest.raises(ValueError, match="select_pairs: " + word):
            gims_amd.select_pairs(feats, **kw)
    with pytest.raises(ValueError, match="float32"):
        gims_amd.select_pairs([(x().double(), None), feats[0]])
    with pytest.raises(ValueError, match="scores must be"):
        gims_amd.select_pairs([(x(), torch.zeros(39)), feats[0]])
    with pytest.raises(ValueError, match="tensors before it on cpu"):
        gims_amd.select_pairs([feats[0], (torch.zeros(40, 128, device="meta"), None)])
    with pytest.raises(ValueError, match="on cpu: the pairs are selected on the GPU"):      # good arguments, CPU tensors: the device check is the last one
        gims_amd.select_pairs(feats)
    sel = gims_amd.PairSelection(torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), torch.zeros(3, 3, dtype=torch.int32),
                                 torch.tensor([2, 9, 0, 0, 0, 0, 0, 0], dtype=torch.int32), 3)
    with pytest.raises(AttributeError, match="immutable"):
        sel.pairs = None
    assert sel.tolist() == [(0, 0), (0, 0)] and sel.stats == dict(n_pairs=2, n_rows=9, n_short_images=0, n_bad_rows=0, n_nonfinite=0)
    assert int(sel.n_rows) == 9 and len(sel) == 2
    with pytest.raises(ValueError, match="out of range"):
        sel.partners(3)


# ------------------------------------------------------------------------------------------------ the layouts, restated
def _work_bytes(ms, d):
    """include/gims_hip.h, written out again: head, table, block images, Q, norms, map, two row arrays -- every region on 256 bytes."""
    def al(x):
        return -(-x // 256) * 256
    pool = sum(-(-m // 32) * 32 for m in ms)
    pool = -(-max(pool, 1) // 128) * 128
    dp = 1 << max(5, int(d - 1).bit_length())
    n = len(ms)
    return 256 + al(64 * n) + al(pool // 32 * 4) + al(pool * dp) + al(pool * 4) + al(n * n) + al(n * 4) + al(n * 4), pool


@pytest.mark.parametrize("ms, d", [([5, 7], 32), ([0, 0], 256), ([0] * 8192, 64), ([1] * 8192, 32), ([127], 128), ([100, 27], 128), ([128, 0], 128),
                                   ([127, 1], 128), ([129, 0], 128), ([64, 65], 96), ([4096, 4096, 1], 1024), ([31, 32, 33, 1], 544)])
def test_work_layout(ms, d):
    if len(ms) == 1:
        ms = ms + [0]                                              # R = 127 as one image of 127 rows and one of none
    want, pool = _work_bytes(ms, d)
    assert hip.pairs_work_bytes(ms, d) == want and hip.pairs_pool(ms) == pool and pool % 128 == 0 and pool >= 128


def test_work_layout_seams_of_the_total():
    # R = 127, 128, 129 rows in all, as whole blocks and as images that straddle them
    assert [hip.pairs_pool(ms) for ms in ([127, 0], [128, 0], [129, 0], [96, 31], [96, 32], [96, 33], [32] * 4, [32] * 4 + [1])] == \
        [128, 128, 256, 128, 128, 256, 128, 256]
    assert hip.pairs_pool([1, 1, 1, 1]) == 128 and hip.pairs_pool([1] * 5) == 256       # every image on a block of its own


@pytest.mark.parametrize("n, k, cap", [(2, 1, 1), (2, 5, 1), (3, 1, 3), (12, 2, 24), (12, 5, 60), (12, 6, 66), (12, 11, 66), (12, 100, 66),
                                       (8192, 1, 8192), (8192, 20, 163840), (8192, 8191, 8192 * 8191 // 2)])
def test_out_layout(n, k, cap):
    assert hip.pairs_out_layout(n, k) == (0, 2 * cap, 3 * cap, cap)
    assert cap == min(n * k, n * (n - 1) // 2)


# ------------------------------------------------------------------------------------------------ the restatement on its own
def test_rq():
    assert R.rq_of(0.0) == 0 == hip.pairs_rq(0.0) and R.rq_of(1.0) == 65536 == hip.pairs_rq(1.0)
    r = float(np.float32(0.8))                                     # 0.800000011920929
    assert R.rq_of(0.8) == hip.pairs_rq(0.8) == int(np.rint(r * r * 65536)) == 41943
    assert hip.pairs_rq(np.float32(0.8)) == 41943


def test_votes_against_brute_force():
    rng = np.random.default_rng(3)
    qs = [rng.integers(-127, 128, size=(m, 32)).astype(np.int8) for m in (9, 1, 0, 6, 2, 7)]
    qs[3][4] = qs[3][1]                                            # a duplicate: d1 = d2 = 0 for whoever matches it exactly
    qs[5][:3] = qs[0][:3]                                          # exact neighbours in another image: d1 = 0
    qs[5][3] = (qs[0][3].astype(np.int32) // 2).astype(np.int8)
    exists = [np.ones(len(q), bool) for q in qs]
    exists[0][8] = False
    exists[4][1] = False                                           # image 4 is left with one row: nobody votes for it
    for rq in (0, 20000, R.rq_of(0.8), 65536):
        got, want = R.votes_of(qs, exists, rq), R.votes_brute(qs, exists, rq)
        np.testing.assert_array_equal(got, want)
        assert (np.diag(got) == 0).all() and (got[:, [1, 2, 4]] == 0).all() and (got[2] == 0).all()
    assert R.votes_of(qs, exists, 0).sum() == 0 and R.votes_of(qs, exists, 65536).sum() > 0
    assert R.votes_of(qs, exists, R.rq_of(0.8))[0, 5] >= 3


def test_scale_and_quantisation():
    x = np.array([[0.5, -2.0, 0.25, 1.0], [1e-3, 2.0 - 1e-6, -0.75, 0.0]], np.float32)
    sel = R.select_rows([x, x[:1]], None, 8)
    qs, s, bad = R.quantise(sel)
    assert s == np.float32(127.0) / np.float32(2.0) and bad == 0 and qs[0].dtype == np.int8
    assert qs[0][0].tolist() == [32, -127, 16, 64] and qs[0][1, 1] == 127          # 31.75 -> 32 and 15.875 -> 16; the largest value to +-127
    # a tie rounds to even: 0.5 * 1 -> 0, 1.5 -> 2, 2.5 -> 2
    qs, s, _ = R.quantise(R.select_rows([np.array([[0.5, 1.5, 2.5, -2.5]], np.float32)], None, 8), scale=1.0)
    assert qs[0][0].tolist() == [0, 2, 2, -2] and s == 1
    # a scale that saturates is clamped
    qs, _, _ = R.quantise(R.select_rows([np.array([[1.0, -1.0, 0.3, 3e38]], np.float32)], None, 8), scale=1000.0)
    assert qs[0][0].tolist() == [127, -127, 127, 127]
    # NaN and +-inf count as 0, here and in the scale, and are counted
    y = np.array([[np.nan, np.inf, -np.inf, 4.0], [1.0, np.nan, 2.0, -3.0]], np.float32)
    qs, s, bad = R.quantise(R.select_rows([y], None, 8))
    assert bad == 4 and s == np.float32(127.0) / np.float32(4.0) and qs[0].tolist() == [[0, 0, 0, 127], [32, 0, 64, -95]]
    # nothing but zeros: s = 0
    qs, s, _ = R.quantise(R.select_rows([np.zeros((2, 4), np.float32)], None, 8))
    assert s == 0 and not qs[0].any()
    # an index outside the image: a row of zeros that does not exist, and is not read for the scale
    sel = R.select_rows([x], [np.array([1, 5, -1, 0])], 8)
    assert sel[0][1].tolist() == [True, False, False, True] and not sel[0][0][1:3].any()
    out = R.run([x, x, x], rows=[np.array([1, 5, -1, 0]), None, None], k=2, min_votes=0)
    assert out["counters"] == dict(n_pairs=3, n_rows=8, n_short_images=0, n_bad_rows=2, n_nonfinite=0)


def test_selection_rules():
    v = np.zeros((5, 5), np.int32)
    v[0, 1], v[1, 0], v[0, 2], v[3, 0], v[4, 0], v[2, 3] = 2, 1, 3, 3, 1, 7
    # S[0] = {1: 3, 2: 3, 3: 3, 4: 1}: equal S is decided by j
    pairs, pv = R.select(v, 1, 1)
    assert pairs.tolist() == [[0, 1], [0, 4], [2, 3]] and pv.tolist() == [3, 1, 7]
    pairs, _ = R.select(v, 2, 1)
    assert pairs.tolist() == [[0, 1], [0, 2], [0, 3], [0, 4], [2, 3]]
    assert R.select(v, 4, 4)[0].tolist() == [[2, 3]] and len(R.select(v, 4, 11)[0]) == 0
    assert len(R.select(v, 4, 0)[0]) == 10 and R.select(v, 99, 0)[1].sum() == (v + v.T)[np.triu_indices(5, 1)].sum()


def test_order_rows():
    assert R.order_rows([0.1, 0.9, 0.5, 0.9, 0.5], 4).tolist() == [1, 3, 2, 4]
    s = torch.tensor([0.1, 0.9, 0.5, 0.9, 0.5])
    assert torch.sort(s, descending=True, stable=True)[1][:4].tolist() == [1, 3, 2, 4]


# ------------------------------------------------------------------------------------------------ the ring: what the feature is for
def test_ring_fixture():
    """12 images around a ring of 480 world descriptors, 96 each, neighbours 40 apart: S is exactly twice the planted overlap -- 112 at ring
    distance 1 (56 shared rows vote both ways), 32 at distance 2 (16 shared), 0 everywhere else."""
    n = 12
    descs = R.ring_scene()
    assert len(descs) == n and all(x.shape == (96, 128) and x.dtype == np.float32 for x in descs)
    out = R.run(descs, k=2, ratio=0.8, min_votes=1)
    s = out["votes"] + out["votes"].T
    for a in range(n):
        for b in range(n):
            assert s[a, b] == {0: 0, 1: 112, 2: 32}.get(R.ring_distance(a, b, n), 0), (a, b, s[a, b])
    ring1 = sorted((min(a, (a + 1) % n), max(a, (a + 1) % n)) for a in range(n))
    assert [tuple(p) for p in out["pairs"]] == ring1 and (out["pair_votes"] == 112).all() and out["counters"]["n_pairs"] == 12
    out4 = R.run(descs, k=4, ratio=0.8, min_votes=1)
    ring2 = sorted(set(ring1) | {(min(a, (a + 2) % n), max(a, (a + 2) % n)) for a in range(n)})
    assert [tuple(p) for p in out4["pairs"]] == ring2 and len(ring2) == 24
    assert sorted(out4["pair_votes"].tolist()) == [32] * 12 + [112] * 12
    assert out["counters"] == dict(n_pairs=12, n_rows=12 * 96, n_short_images=0, n_bad_rows=0, n_nonfinite=0)
