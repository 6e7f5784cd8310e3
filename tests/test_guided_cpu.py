"""CPU tests of guided matching: the ABI constant and the pins a feature must leave alone, the argument checks of GIMS_AUX_GUIDED_MATCH (they
run before any HIP call), the ValueErrors of gims_amd.guided_match_pairs / guided_match_features, the workspace formula of hip.py against an
independent restatement, and the NumPy restatement (tests/guided_ref.py) on its own: the symmetry of the gate, its limit without a gate
(nn_ref.solve), and the fixtures that show what the feature is for."""
import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import guided_ref as R
from tests import nn_ref

W = hip.GUIDED_WORD


def test_abi_constant_and_pins():
    assert hip.AUX_GUIDED_MATCH == 18 == hip.ABI.constants["GIMS_AUX_GUIDED_MATCH"] and hip.GUIDED_TABLE_WORDS == 32 == len(W)
    # the feature adds no export, no struct and no ABI version
    assert len(hip.EXPORTS) == 90 and len(hip.ABI.structs) == 28 and hip.ABI_VERSION == 5 == hip.load().gims_abi_version()
    assert not any("guided" in name.lower() for name in hip.EXPORTS)
    assert gims_amd.guided_match_pairs is gims_amd.guided.guided_match_pairs and gims_amd.guided_match_features is gims_amd.guided.guided_match_features
    assert "guided_match_pairs" in gims_amd.__all__ and "guided_match_features" in gims_amd.__all__
    assert hip.GUIDED_INFO == R.INFO
    assert [W[k] for k in ("a", "n0", "kpts0", "model", "kind", "ok", "prior", "mutual", "nn1", "n_admissible", "info", "thresh", "reserved")] == \
        [0, 4, 7, 9, 10, 11, 12, 15, 16, 21, 27, 28, 31]
    p = [0x10000, 0x20000, None, None, None, None]
    for fn in (12, 15, 19, 99, -1):
        with pytest.raises(hip.GimsHipError, match=f"unknown auxiliary function {fn}"):
            with hip.on_stream(0):
                hip.run_ops(hip.make_ops([hip.op_aux(fn, p, [1, 0, 1 << 20, 0, 0, 0], (0.0,))]))


def _item(**kw):
    """One pair of stand-in addresses: nothing of it is ever dereferenced (every call below is refused)."""
    it = dict(a=0x100000, b=0x200000, lda=128, ldb=128, n0=300, n1=129, d=128, kpts0=0x300000, kpts1=0x310000, model=0x320000, kind=1, ok=0x330000,
              prior=0x340000, prior_mask=0x350000, prior_scores=0x360000, mutual=1, nn1=0x400000, nn2=0x410000, d1=0x420000, d2=0x430000,
              ratio=0x440000, n_admissible=0x450000, matches0=0x460000, scores0=0x470000, added0=0x480000, cnn1=0x490000, matches1=0x4a0000,
              info=0x4b0000, thresh=3.0, threshold=0.8, max_distance=None, reserved=0)
    it.update(kw)
    return it


def test_argument_checks_come_before_any_hip_call():
    """Every GIMS_EINVAL case of the header, with a message naming guided_match; the device pointers are never dereferenced (the table is
    HOST memory and is read).  No call of this test is a good one: each is refused."""
    need = hip.guided_layout([(300, 129, True)])["bytes"]
    work = 0x7000000

    def refused(word, items=None, ints=None, ptrs=None, floats=(0.0, 0.0), tab=None, addr=None, match="guided_match"):
        tab = hip.guided_table(items if items is not None else [_item()]) if tab is None else tab
        ints = [tab.shape[0], 0, need - 1, 0, 0, 0] if ints is None else ints
        ptrs = [tab.ctypes.data if addr is None else addr, work, None, None, None, None] if ptrs is None else [tab.ctypes.data] + ptrs
        with pytest.raises(hip.GimsHipError, match=match) as e:
            with hip.on_stream(0):
                hip.run_ops(hip.make_ops([hip.op_aux(hip.AUX_GUIDED_MATCH, ptrs, ints, floats)]))
        assert word in str(e.value) and f"({hip.GIMS_EINVAL})" in str(e.value), str(e.value)

    # the one difference between a good call and the first case: the workspace is one byte short
    refused(f"work_bytes = {need - 1} is below the {need} bytes")
    refused("work_bytes = -1", ints=[1, 0, -1, 0, 0, 0])
    refused("work_bytes", ints=[1, hip.NN_EXHAUSTIVE, hip.guided_layout([(300, 129, True)], hip.NN_EXHAUSTIVE)["bytes"] - 1, 0, 0, 0])
    # the size and alignment rules of gims_nn_match
    for d in (0, 16, 48, 544, 1024):
        refused("d must be a multiple of 32 in [32, 512]", [_item(d=d, lda=1024, ldb=1024)])
    refused("needs n0 >= 1 and n1 >= 1", [_item(n0=0)])
    refused("needs n0 >= 1 and n1 >= 1", [_item(n1=0)])
    refused("more than 32768 rows", [_item(n0=32769)])
    refused("more than 32768 rows", [_item(n1=40000)])
    refused("out of range", [_item(n0=-1)])
    refused("out of range", [_item(d=1 << 40)])
    refused("row pitch below d or not a multiple of 4", [_item(lda=127)])
    refused("row pitch below d or not a multiple of 4", [_item(ldb=130)])
    refused("a / b not 16-byte aligned", [_item(a=0x100008)])
    refused("a / b not 16-byte aligned", [_item(b=0x200004)])
    refused("pair 1 ", [_item(), _item(d=48)])
    # required pointers
    for name in ("a", "b", "nn1", "nn2", "d1", "d2", "ratio", "matches0", "scores0", "added0", "info"):
        refused("null pointer", [_item(**{name: None})])
    refused("null matches1 with mutual set", [_item(matches1=None)])
    for name in ("kpts0", "kpts1", "model", "n_admissible", "cnn1"):
        refused("null pointer (kpts0, kpts1, model, n_admissible, or cnn1 with mutual set)", [_item(**{name: None})])
    refused("the table or the workspace is NULL", addr=0)
    refused("the table or the workspace is NULL", ptrs=[None, None, None, None, None])
    # values
    for kind in (2, 3, -1, 99):
        refused(f"unknown kind {kind}", [_item(kind=kind)])
    for t in (0.0, -1.0, float("inf"), float("nan")):
        refused("thresh must be finite and > 0", [_item(thresh=t)])
    for m in (-0.5, float("nan"), float("-inf")):
        refused("max_distance must be >= 0", [_item(max_distance=m)])
    refused("unknown flag bits 0x2", ints=[1, 2, need, 0, 0, 0])
    refused("pairs in one call", ints=[0, 0, need, 0, 0, 0])
    refused("pairs in one call", ints=[-3, 0, need, 0, 0, 0])
    refused("pairs in one call", ints=[1 << 20, 0, need, 0, 0, 0])
    # reserved words
    refused("reserved word of the table", [_item(reserved=1)])
    for k in ("thresh", "threshold", "max_distance"):
        tab = hip.guided_table([_item()])
        tab[0, W[k]] |= 1 << 32
        refused("reserved word of the table", tab=tab)
    refused("reserved word of the call", ints=[1, 0, need, 1, 0, 0])
    refused("reserved word of the call", ints=[1, 0, need, 0, 1, 0])
    for k in range(4):
        refused("reserved word of the call", ptrs=[work] + [0x60000 if j == k else None for j in range(4)])
    refused("reserved word of the call", floats=(1.0, 0.0))
    refused("reserved word of the call", floats=(0.0, float("nan")))
    refused("8-byte aligned", addr=hip.guided_table([_item()]).ctypes.data + 4)
    refused("256-byte aligned", ptrs=[work + 128, None, None, None, None])
    # i[5] would select a later form of the function, so it is read first
    refused("i[5] = 1", ints=[1, 0, need, 0, 0, 1], match="unknown auxiliary function form")
    # the table and the op builder
    tab = hip.guided_table([_item(), _item(mutual=0, max_distance=1.25, n1=1)])
    assert tab.shape == (2, 32) and tab.dtype == np.int64
    assert tab[0, :8].tolist() == [0x100000, 0x200000, 128, 128, 300, 129, 128, 0x300000] and tab[0, 15] == 1 and tab[1, 15] == 0 and tab[1, 5] == 1
    assert tab[0, 28:].tolist() == [0x40400000, int(np.float32(0.8).view(np.uint32)), 0x7f800000, 0] and tab[1, 30] == 0x3fa00000
    op = hip.op_guided_match(tab, work, 12345, hip.NN_EXHAUSTIVE)
    a = op.u.aux
    assert op.kind == 2 and a.fn == 18 and list(a.p) == [tab.ctypes.data, work, None, None, None, None] and list(a.i) == [2, 1, 12345, 0, 0, 0]
    assert list(a.f) == [0.0, 0.0]


def test_value_errors_before_the_device_is_touched():
    n0, n1, d = 12, 9, 32
    data = dict(descriptors0=torch.zeros(1, d, n0), descriptors1=torch.zeros(1, d, n1), keypoints0=torch.zeros(1, n0, 2), keypoints1=torch.zeros(1, n1, 2))
    out = dict(matches0=torch.full((1, n0), -1, dtype=torch.int64))
    ver = dict(models=torch.zeros(1, 3, 3), records=torch.zeros(1, 8), inlier=[torch.zeros(n0, dtype=torch.uint8)])
    K = np.eye(3)
    g = gims_amd.guided_match_pairs
    with pytest.raises(ValueError, match="lists of one length"):
        g([data, data], [out], ver)
    with pytest.raises(ValueError, match="lists of one length"):
        g([], [], ver)
    with pytest.raises(ValueError, match="lists of unequal length"):
        g([data, data], [out, out], ver)
    with pytest.raises(ValueError, match="lists of unequal length"):
        g([data], None, dict(ver, inlier=[]))
    for keep in ("inlier", "", None, 1):
        with pytest.raises(ValueError, match="keep must be one of"):
            g([data], [out], ver, keep=keep)
    for model in ("affine", 1, ["fundamental", "pose"], []):
        with pytest.raises(ValueError, match="model must be one of"):
            g([data], [out], ver, model=model)
    with pytest.raises(ValueError, match="model='pose' needs intrinsics"):
        g([data], [out], ver, model="pose")
    with pytest.raises(ValueError, match="intrinsics must be one"):
        g([data], [out], ver, model="pose", intrinsics=(K, np.eye(2)))
    with pytest.raises(ValueError, match="intrinsics must be one"):
        g([data], [out], ver, model=["pose"], intrinsics=[None])
    for side, bad in (("0", torch.zeros(1, n0 + 1, 2)), ("1", torch.zeros(1, n1 - 1, 2))):
        with pytest.raises(ValueError, match=f"keypoints in image {side}: the counts differ"):
            g([dict(data, **{"keypoints" + side: bad})], [out], ver)

    class Feat:
        def __init__(self, n, nk=None):
            self.descriptors, self.keypoints, self.n = torch.zeros(n, 256), torch.zeros(n if nk is None else nk, 2), n

    f = gims_amd.guided_match_features
    feats = [Feat(n0), Feat(n1)]
    with pytest.raises(ValueError, match="lists of one length"):
        f(feats, [(0, 1), (1, 0)], [out], ver)
    with pytest.raises(ValueError, match="lists of unequal length"):
        f(feats, [(0, 1), (1, 0)], None, ver)
    with pytest.raises(ValueError, match="keep must be one of"):
        f(feats, [(0, 1)], [out], ver, keep="some")
    with pytest.raises(ValueError, match="model='pose' needs intrinsics"):
        f(feats, [(0, 1)], [out], ver, model="pose")
    with pytest.raises(ValueError, match="image 1: 9 descriptors and 8 keypoints"):
        f([Feat(n0), Feat(n1, 8)], [(0, 1)], [out], ver)
    with pytest.raises(ValueError, match="out of range"):
        f(feats, [(0, 2)], [out], ver)


# ------------------------------------------------------------------------------------------------ the layout, restated
def _work_bytes(sizes, exhaustive):
    """include/gims_hip.h, written out again."""
    def al(x):
        return -(-x // 256) * 256

    def up(a, b):
        return -(-a // b)
    probs = []
    for n0, n1, mutual in sizes:
        probs += [(n0, n1, False)] + ([(n1, n0, True)] if mutual else [])
    P, Q = len(sizes), len(probs)
    want = max(1, min(8, up(512, sum(up(nx, 128) for nx, _, _ in probs))))
    b = al(160 * Q) + al(200 * P) + al(16 * P) + al(48 * Q) + al(232 * P) + al(16 * P) + al(4 * sum(n1 for _, n1, _ in sizes))
    b += sum(al(8 * n0) + al(8 * n1) + al(4 * n0) + al(4 * n1) + al(32 * n0) + al(32 * n1) + al(n0) for n0, n1, _ in sizes)
    cs, items = [], 0
    for nx, ny, second in probs:
        tiles = up(ny, 128)
        c = up(tiles, up(tiles, min(want, tiles)))
        cs.append(c)
        items += up(nx, 128) * c
        b += al(4 * nx) * (4 if second else 1) + (0 if exhaustive else 2 * al(64 * nx * c) + al(16 * nx * c))
    return b, cs, items


@pytest.mark.parametrize("sizes", [[(1, 1, True)], [(1, 1, False)], [(127, 129, True)], [(128, 128, False)], [(300, 129, True)], [(4096, 4096, True)] * 8,
                                   [(15382, 14870, True)], [(32768, 32768, True)], [(3, 1, True), (300, 127, False), (129, 2, True)],
                                   [(2000, 700, True)], [(700, 2000, False)] * 3])
def test_work_layout(sizes):
    for flags in (0, hip.NN_EXHAUSTIVE):
        want, cs, items = _work_bytes(sizes, bool(flags))
        got = hip.guided_layout(sizes, flags)
        assert got == dict(bytes=want, csplit=cs, items=items) and want % 256 == 0
        assert all(1 <= c <= 8 for c in cs)


def test_work_layout_matches_the_matcher_where_both_serve():
    """The first part of the formula is gims_nn_workspace_bytes' own: for sizes the matcher serves, the guided workspace is larger by exactly
    the regions of the gate (a host call: no device is touched)."""
    lib = hip.load()
    for sizes in ([(300, 129, True)], [(1024, 1500, False), (64, 2, True)], [(4096, 4096, True)] * 2):
        arr = (hip.NnPair * len(sizes))()
        for i, (n0, n1, m) in enumerate(sizes):
            arr[i] = hip.NnPair(0x100000, 0x200000, 128, 128, n0, n1, 128, int(m), 0.8, 0, *[0x300000] * 8, 0x400000 if m else None,
                                0x500000 if m else None, 0x600000, None)
        for flags in (0, hip.NN_EXHAUSTIVE):
            nn = int(lib.gims_nn_workspace_bytes(arr, len(sizes), flags))
            assert nn > 0
            al = lambda x: -(-x // 256) * 256                                  # noqa: E731
            P, Q = len(sizes), sum(2 if m else 1 for _, _, m in sizes)
            gate = al(48 * Q) + al(232 * P) + al(16 * P) + al(4 * sum(n1 for _, n1, _ in sizes))
            gate += sum(al(32 * n0) + al(32 * n1) + al(n0) for n0, n1, _ in sizes)
            L = hip.guided_layout(sizes, flags)
            if not flags:
                k = 0
                for n0, n1, m in sizes:
                    gate += al(16 * n0 * L["csplit"][k])
                    k += 1
                    if m:
                        gate += al(16 * n1 * L["csplit"][k])
                        k += 1
            assert L["bytes"] == nn + gate


# ------------------------------------------------------------------------------------------------ the restatement on its own
def _gate_qc(kind, t2, q, c):
    """The gate as the kernels evaluate it: one expression of (query words, column words), whichever image the queries come from."""
    q, c = [q[:, k][:, None] for k in range(4)], [c[:, k][None, :] for k in range(4)]
    with np.errstate(all="ignore"):
        if kind == R.FUNDAMENTAL:
            n = (q[0] * c[0] + q[1] * c[1]) + q[2] * c[2]
            return (q[3] > 0) & (c[3] > 0) & (n * n <= t2 * q[3]) & (n * n <= t2 * c[3])
        dx, dy, ex, ey = q[0] - c[2], q[1] - c[3], c[0] - q[2], c[1] - q[3]
        return (dx * dx + dy * dy <= t2) & (ex * ex + ey * ey <= t2)


def test_the_gate_is_symmetric():
    A, B, kp0, kp1, m0, F, _ = R.planted_descriptors(255, "general")
    hA, hB, hk0, hk1, gt, H = R.homography_fixture()
    for kind, model, k0, k1 in ((R.FUNDAMENTAL, F, kp0, kp1), (R.HOMOGRAPHY, H, hk0, hk1)):
        for thresh in (0.5, 3.0, 40.0):
            wa, wb = R.row_words(kind, model, k0, k1)
            adm = R.admissible(kind, thresh, wa, wb)
            t2 = float(np.float32(thresh)) ** 2
            np.testing.assert_array_equal(_gate_qc(kind, t2, wa, wb), adm)
            np.testing.assert_array_equal(_gate_qc(kind, t2, wb, wa), adm.T)
            assert 0 < adm.sum() < adm.size
    # the words of the homography are the forward and the backward transfer: H and its cofactors agree up to the determinant
    wa, wb = R.row_words(R.HOMOGRAPHY, H, hk0, hk1)
    Hm = H.astype(np.float64).reshape(3, 3)
    back = np.linalg.inv(Hm) @ np.concatenate([hk1.astype(np.float64), np.ones((len(hk1), 1))], 1).T
    np.testing.assert_allclose(wb[:, :2], (back[:2] / back[2]).T, rtol=1e-9, atol=1e-9)
    # fundamental: n^2 / g and n^2 / h are the squared distances to the two epipolar lines
    wa, wb = R.row_words(R.FUNDAMENTAL, F, kp0, kp1)
    Fm = F.astype(np.float64).reshape(3, 3)
    x1 = np.concatenate([kp1.astype(np.float64), np.ones((len(kp1), 1))], 1)
    lines = x1 @ Fm                                                         # F^T x1: the line of every point of image 1 in image 0
    np.testing.assert_allclose(wb[:, 3], lines[:, 0] ** 2 + lines[:, 1] ** 2, rtol=1e-12)


def test_without_a_gate_it_is_the_plain_matcher():
    for K, config, mutual in ((64, "general", True), (255, "xtrans", True), (255, "general", False)):
        A, B, kp0, kp1, m0, F, _ = R.planted_descriptors(K, config)
        g = R.solve(A, B, kp0, kp1, F, R.FUNDAMENTAL, thresh=1e9, mutual=mutual)
        n = nn_ref.solve(np.ascontiguousarray(A.T), np.ascontiguousarray(B.T), 0.8, mutual)
        assert (g["n_admissible"] == len(B)).all() and g["info"].tolist() == [0, 0, 0, 0, 0, 0, int(n["match"].sum()), 0]
        for k in ("nn1", "nn2", "d1", "d2", "ratio", "matches0", "scores0") + (("matches1", "cnn1") if mutual else ()):
            np.testing.assert_array_equal(g[k], n[k].astype(g[k].dtype), err_msg=k)
        np.testing.assert_array_equal(g["added0"], n["match"].astype(np.uint8))


def test_fixed_rows_and_counters():
    prior = np.array([3, -1, 3, 7, 9, -5, 0, 2, 2, -1], np.int64)
    fixed, taken, bad, dup = R.fixed_rows(prior, None, 10, 8)
    assert fixed.tolist() == [1, 0, 0, 1, 0, 0, 1, 1, 0, 0] and np.nonzero(taken)[0].tolist() == [0, 2, 3, 7] and (bad, dup) == (2, 2)
    mask = np.array([0, 1, 1, 1, 0, 1, 1, 0, 1, 1], np.uint8)              # frees rows 0 and 7: rows 2 and 8 inherit their columns; row 4 is not read
    fixed, taken, bad, dup = R.fixed_rows(prior, mask, 10, 8)
    assert fixed.tolist() == [0, 0, 1, 1, 0, 0, 1, 0, 1, 0] and np.nonzero(taken)[0].tolist() == [0, 2, 3, 7] and (bad, dup) == (1, 0)
    assert R.fixed_rows(None, mask, 10, 8)[2:] == (0, 0) and not R.fixed_rows(None, None, 10, 8)[0].any()
    assert not R.has_model(np.zeros(9), 0.0) and R.has_model(np.zeros(9), 1.0) and R.has_model(np.zeros(9))
    assert not R.has_model(np.array([1, 0, 0, 0, np.nan, 0, 0, 0, 1.0])) and not R.has_model(np.array([1, 0, 0, 0, 3e38 * 10, 0, 0, 0, 1.0]))


# What the restatement gives on the probe's fixtures, from its own run here: conditions of the fixtures, not bars for the device.
# (n0, n1, true pairs = rows of the fixture's matches0 admissible under the planted F, rows the plain mutual ratio test keeps, of those
#  agreeing with a true pair, rows the gated test keeps, of those agreeing with a true pair).  "Agreeing" is counted against the true pairs:
# the fixture's matches0 also holds its planted geometric outliers, which the plain test keeps (their descriptors agree) and the gate drops.
PROBE = {(255, "general"): (321, 324, 172, 186, 103, 178, 172), (255, "xtrans"): (321, 324, 181, 187, 113, 187, 181),
         (1025, "general"): (1284, 1287, 693, 765, 432, 691, 691), (1025, "xtrans"): (1284, 1287, 720, 767, 462, 718, 718)}


@pytest.mark.parametrize("K, config", sorted(PROBE))
def test_probe_on_the_planted_two_view_fixture(K, config):
    A, B, kp0, kp1, m0, F, true = R.planted_descriptors(K, config)
    truth = np.full(len(m0), -2, np.int64)
    truth[true] = m0[true]
    plain = R.plain_mutual(A, B, 0.8)
    g = R.solve(A, B, kp0, kp1, F, R.FUNDAMENTAL, thresh=3.0, ratio=0.8, mutual=True)
    got = (len(A), len(B), len(true), int((plain >= 0).sum()), int((plain == truth).sum()), int((g["matches0"] >= 0).sum()),
           int((g["matches0"] == truth).sum()))
    assert got == PROBE[(K, config)], got
    assert got[6] > got[4]                                                  # the gate removes the twin that spoils the ratio ...
    assert got[5] - got[6] < got[3] - got[4]                                # ... and the match that contradicts the model
    # one-to-one, and a refill on top of the fixture's own matches keeps them and adds to them
    m1 = g["matches1"]
    rows = np.nonzero(g["matches0"] >= 0)[0]
    assert (m1[g["matches0"][rows]] == rows).all() and (m1 >= 0).sum() == len(rows)
    keep = np.zeros(len(m0), np.uint8)
    keep[true[1::2]] = 1                                                    # the matcher found every second true pair, verify_pairs kept them
    r = R.solve(A, B, kp0, kp1, F, R.FUNDAMENTAL, prior=m0, mask=keep)
    assert r["info"][2] == keep.sum() and (r["matches0"][keep != 0] == m0[keep != 0]).all() and r["info"][6] > 0
    assert int((r["matches0"] == truth).sum()) >= got[6] - 2
    # margins: no row of this fixture sits on a decision's edge
    near, _ = R.margins(g, 0.8)
    assert near > 1e-6, near
    near, ulps = R.margins(R.solve(A, B, kp0, kp1, F, R.FUNDAMENTAL, max_distance=0.45), 0.8, 0.45)
    assert near > 1e-6 and ulps > 1.0, (near, ulps)


def test_probe_on_the_homography_pair():
    A, B, kp0, kp1, gt, H = R.homography_fixture()
    plain = R.plain_mutual(A, B, 0.8)
    g = R.solve(A, B, kp0, kp1, H, R.HOMOGRAPHY, thresh=3.0, ratio=0.8)
    got = (int((plain >= 0).sum()), int(((plain == gt) & (gt >= 0)).sum()), int((g["matches0"] >= 0).sum()), int(((g["matches0"] == gt) & (gt >= 0)).sum()))
    assert got == (241, 241, 270, 270), got
    assert got[3] > got[1]
    assert R.margins(g, 0.8)[0] > 1e-6
