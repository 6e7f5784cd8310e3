"""CPU tests that go with tests/test_small_kernels_gpu.py.

* The argument checks of the small kernels' entry points (gims_amd/csrc/misc.hip, gims_amd/csrc/train.hip): each refusal comes before any HIP
  call, so dummy non-null addresses are enough and no device is needed; the error names the function.
* tests/small_ref.py against a second, loop formulation of every reference at tiny sizes -- and against deliberately wrong references
  (last neighbour, last row block, last column skipped), which the comparison the GPU tests use must refuse: that is the argument for
  the GPU tests' sensitivity, the kernels are never broken to show it."""
import numpy as np
import pytest
import torch

from gims_amd import hip
from tests import small_ref as R

P = [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000]      # never dereferenced: 16-byte aligned dummy addresses


def _refused(fn_name, *args, word=None):
    lib = hip.load()
    rc = getattr(lib, fn_name)(*args)
    msg = lib.gims_last_error()
    assert rc == hip.GIMS_EINVAL and fn_name.encode() in msg, (fn_name, args, rc, msg)
    if word is not None:
        assert word in msg, msg


# ------------------------------------------------------------------------------------------------ argument checks
def test_layernorm_act_arguments():
    f = "gims_layernorm_act"          # x, ldx, rows, c, a2, b2, eps, act, out, ldo, out_hi, out_lo, ld_split, stream

    def call(c=64, ldx=70, ldo=72, out=P[3], hi=None, lo=None, ld_split=0, word=None):
        _refused(f, P[0], ldx, 7, c, P[1], P[2], 1e-6, hip.ACT_RELU, out, ldo, hi, lo, ld_split, None, word=word)

    call(c=1)
    call(c=513)
    call(hi=P[4], lo=None, ld_split=128, word=b"come together")
    call(hi=None, lo=P[5], ld_split=128, word=b"come together")
    call(out=None)                                                 # no output at all
    # pitches below the row width: the last row would be read / written past its buffer
    call(ldx=63, word=b"pitch")
    call(ldo=63, word=b"pitch")
    call(c=65, ldx=65, ldo=65, hi=P[4], lo=P[5], ld_split=130, word=b"pitch")       # 65 channels fill three 32-blocks: 192 needed
    call(c=64, out=None, hi=P[4], lo=P[5], ld_split=127, word=b"pitch")


def test_layernorm_backward_arguments():
    for c in (1, 513):                # x, ldx, dy, ldd, rows, c, a2, b2, eps, relu, dx, ldo, g_bias, g_scale, stream
        _refused("gims_layernorm_backward", P[0], 600, P[1], 600, 7, c, P[2], P[3], 1e-6, 1, P[4], 600, P[5], P[6], None)
    _refused("gims_layernorm_backward", P[0], 63, P[1], 64, 7, 64, P[2], P[3], 1e-6, 1, P[4], 64, P[5], P[6], None)


def test_colsum_arguments():
    f = "gims_colsum"                 # x, ld, rows, c, beta, out, work, stream
    for c in (2, 6, 4100):
        _refused(f, P[0], 4104, 10, c, 0.0, P[1], P[2], None)
    _refused(f, P[0], 60, 10, 64, 0.0, P[1], P[2], None)           # ld < c
    _refused(f, P[0], 66, 10, 64, 0.0, P[1], P[2], None)           # pitch not a multiple of 4
    _refused(f, P[0] + 4, 64, 10, 64, 0.0, P[1], P[2], None)       # not 16-byte aligned
    _refused(f, P[0], 64, 0, 64, 0.0, P[1], P[2], None)            # no rows
    _refused(f, P[0], 64, 10, 64, 0.0, P[1], None, None)           # no workspace


def test_elementwise_arguments():
    f = "gims_elementwise"            # op, out, ldo, a, lda, b, ldb, rows, cols, alpha, stream
    for op in (-1, 5, 99):
        _refused(f, op, P[0], 8, P[1], 8, P[2], 8, 3, 8, 1.0, None, word=b"unknown operation")
    _refused(f, hip.EW_ADD, P[0], 8, P[1], 8, None, 0, 3, 8, 1.0, None, word=b"second operand")
    _refused(f, hip.EW_RELU_MASK, P[0], 8, P[1], 8, None, 0, 3, 8, 1.0, None, word=b"second operand")
    _refused(f, hip.EW_ADD, P[0], 8, P[1], 8, P[2], 7, 3, 8, 1.0, None, word=b"second operand")     # b's pitch below cols
    _refused(f, hip.EW_SCALE, P[0], 7, P[1], 8, None, 0, 3, 8, 1.0, None)
    _refused(f, hip.EW_SCALE, P[0], 8, P[1], 7, None, 0, 3, 8, 1.0, None)


def test_sage_mean_arguments():
    # h, ldh, indptr, indices, n, c, out, ldo, stream
    for f in ("gims_sage_mean", "gims_sage_mean_split", "gims_sage_mean_transposed"):
        _refused(f, P[0], 8, P[1], P[2], 5, 6, P[3], 64, None)                      # c = 6
        _refused(f, P[0], 10, P[1], P[2], 5, 8, P[3], 64, None)                     # input pitch not a multiple of 4
    # the split form: pitch >= 2 * roundup(c, 32), a multiple of 4, 8-byte aligned planes
    _refused("gims_sage_mean_split", P[0], 40, P[1], P[2], 5, 36, P[3], 124, None)  # 36 channels -> two blocks -> 128
    _refused("gims_sage_mean_split", P[0], 8, P[1], P[2], 5, 4, P[3], 60, None)
    _refused("gims_sage_mean_split", P[0], 8, P[1], P[2], 5, 4, P[3] + 4, 64, None)


def test_pack_softmax_gather_run_ops_arguments():
    # dev_images, n_images, max_kept, max_edges, d, feat, ldf, kpts_out, score_out, seg, indptr_out, indices_out, n_rows, n_edges, stream
    _refused("gims_pack_graphs", P[0], 2, 5, 5, 6, P[1], 8, P[2], None, P[3], P[4], P[5], 5, 5, None)          # d = 6
    _refused("gims_pack_graphs", P[0], 2, 5, 5, 4, P[1], 6, P[2], None, P[3], P[4], P[5], 5, 5, None)          # ldf = 6
    # s, ld, rows, cols, batch, stride, stream
    _refused("gims_softmax_rows", P[0], 7, 3, 8, 2, 24, None)                       # ld < cols
    _refused("gims_softmax_rows", P[0], 8, 3, 8, 65536, 24, None)                   # the batch is the grid's y dimension
    _refused("gims_softmax_rows_backward", P[0], P[1], 7, 3, 8, 2, 24, None)
    _refused("gims_softmax_rows_backward", P[0], P[1], 8, 3, 8, 65536, 24, None)
    # src, lds, idx, n, c, dst, ldd, stream: a pitch below the row width
    _refused("gims_gather_rows", P[0], 63, P[1], 5, 64, P[2], 64, None, word=b"pitch")
    _refused("gims_gather_rows", P[0], 64, P[1], 5, 64, P[2], 63, None, word=b"pitch")
    # dev_images, n_images, max_n, d, desc_out, ldo, kpts_out, score_out, stream: a batch of empty images is refused by the entry point
    # (hip.ingest_images does not make the call then, see the GPU test)
    _refused("gims_ingest_images", P[0], 3, 0, 4, P[1], 8, P[2], None, None)
    lib = hip.load()
    for fn in (8, 99, -1):
        rc = lib.gims_run_ops(hip.make_ops([hip.op_aux(fn, P[:6], [8, 8, 8, 8, 8, 8])]), 1, None)
        msg = lib.gims_last_error()
        assert rc == hip.GIMS_EINVAL and b"gims_run_ops" in msg and b"unknown auxiliary function" in msg, (rc, msg)


# ------------------------------------------------------------------------------------------------ the references, twice
def _tiny_graph():
    indptr = np.array([0, 3, 3, 4, 9], np.int32)                  # degrees 3, 0, 1, 5
    indices = np.array([1, 3, 3, 0, 2, 2, 0, 1, 3], np.int32)
    return indptr, indices


def test_sage_references_against_loops():
    indptr, indices = _tiny_graph()
    rng = np.random.default_rng(0)
    h = rng.integers(-8, 9, size=(4, 6))
    loop = np.zeros((4, 6), np.int64)
    short = np.zeros((4, 6), np.int64)                            # the wrong reference: skips every node's last neighbour
    for i in range(4):
        for e in range(indptr[i], indptr[i + 1]):
            loop[i] += h[indices[e]]
            if e < indptr[i + 1] - 1:
                short[i] += h[indices[e]]
    np.testing.assert_array_equal(R.sage_sum(h, indptr, indices), loop)
    exact = R.sage_mean_exact(h, indptr, indices)
    deg = np.diff(indptr)
    for i in range(4):
        want = np.zeros(6, np.float32) if deg[i] == 0 else loop[i].astype(np.float32) / np.float32(deg[i])
        np.testing.assert_array_equal(exact[i].view(np.int32), want.view(np.int32))
    np.testing.assert_allclose(R.sage_mean(h.astype(np.float32), indptr, indices), exact, rtol=1e-7)
    with pytest.raises(AssertionError):
        np.testing.assert_array_equal(R.sage_sum(h, indptr, indices), short)
    # transposed form on a symmetric multigraph
    ip, ix = np.array([0, 2, 5, 6, 6], np.int32), np.array([1, 1, 0, 0, 2, 1], np.int32)
    g = rng.normal(size=(4, 3))
    out, mag = R.sage_mean_transposed(g, ip, ix)
    d = np.diff(ip)
    for j in range(4):
        acc, am = np.zeros(3), np.zeros(3)
        for e in range(ip[j], ip[j + 1]):
            acc += g[ix[e]] / d[ix[e]]
            am += np.abs(g[ix[e]]) / d[ix[e]]
        np.testing.assert_allclose(out[j], acc, rtol=1e-14, atol=0)
        np.testing.assert_allclose(mag[j], am, rtol=1e-14, atol=0)
    # the adjoint identity the GPU test asserts holds for the references
    hh = rng.normal(size=(4, 3))
    assert abs((R.sage_mean(hh, ip, ix) * g).sum() - (hh * out).sum()) < 1e-13


def test_test_graphs_have_the_degrees_the_branches_need():
    indptr, indices = R.sage_graph()
    deg = np.diff(indptr)
    assert len(deg) == R.SAGE_N and R.SAGE_N % 4 != 0 and set(R.SAGE_DEGREES) <= set(deg.tolist())
    assert deg[0] == 200 and deg[-1] == 131 and indices.min() >= 0 and indices.max() < R.SAGE_N
    ip, ix = R.sym_graph()
    d = np.diff(ip)
    assert d[0] == 131 and d[40] == 0 and d[41] == 1 and ix[ip[41]] == 0
    a = np.zeros((R.SAGE_N, R.SAGE_N), np.int64)
    np.add.at(a, (np.repeat(np.arange(R.SAGE_N), d), ix), 1)
    assert (a == a.T).all() and np.trace(a) == 0                  # every undirected edge in both rows, no self loop


def test_copy_references_against_loops():
    rng = np.random.default_rng(1)
    src = np.arange(5 * 7, dtype=np.float32).reshape(5, 7)
    idx = np.array([4, 0, 4, 2])
    np.testing.assert_array_equal(R.gather_rows(src, idx), np.stack([src[i] for i in idx]))
    # ingest: channel-major -> point-major at the row offsets
    imgs = []
    for n, off, has in ((3, 1, True), (0, 5, True), (2, 6, False)):
        imgs.append((rng.normal(size=(n, 2)).astype(np.float32), rng.normal(size=(4, n + 3)).astype(np.float32),
                     rng.normal(size=n).astype(np.float32) if has else None, off))
    de, kp, sc, wr = R.ingest(imgs, 4, 9)
    assert wr.tolist() == [False, True, True, True, False, False, True, True, False]
    for kpts, desc, score, off in imgs:
        for k in range(kpts.shape[0]):
            for ch in range(4):
                assert de[off + k, ch] == desc[ch, k]
            assert (kp[off + k] == kpts[k]).all() and sc[off + k] == (0 if score is None else score[k])
    # pack
    images = []
    for N, k, e, has in ((6, 3, 4, True), (2, 0, 0, False), (5, 2, 0, False), (4, 4, 5, True)):
        ip = np.sort(np.r_[0, rng.integers(0, e + 1, size=max(k - 1, 0)), e]).astype(np.int32) if k else np.zeros(1, np.int32)
        images.append(dict(kpts=rng.normal(size=(N, 2)).astype(np.float32), desc=rng.normal(size=(N, 4)).astype(np.float32),
                           score=rng.normal(size=N).astype(np.float32) if has else None, kept=rng.permutation(N)[:k].astype(np.int32),
                           indptr=ip, indices=rng.integers(0, max(k, 1), size=e).astype(np.int32)))
    out = R.pack(images, 4)
    row = edge = 0
    for i, im in enumerate(images):
        for r, src_row in enumerate(im["kept"]):
            assert (out["feat"][row] == im["desc"][src_row]).all() and (out["kpts"][row] == im["kpts"][src_row]).all()
            assert out["seg"][row] == i and out["indptr"][row] == im["indptr"][r] + edge
            assert out["has_score"][row] == (im["score"] is not None) and (im["score"] is None or out["score"][row] == im["score"][src_row])
            row += 1
        base = row - len(im["kept"])
        for e, v in enumerate(im["indices"]):
            assert out["indices"][edge + e] == v + base
        edge += len(im["indices"])
    assert out["indptr"][row] == edge == 9 and row == 9
    # permute3: both sides strided, plain and accumulating
    shape, ds, ss = (2, 3, 4), (1, 30, 7), (40, 2, 11)
    s = rng.integers(-8, 9, size=80).astype(np.float64)
    d0 = rng.integers(-8, 9, size=90).astype(np.float64)
    for acc in (False, True):
        want = d0.copy()
        for i0 in range(2):
            for i1 in range(3):
                for i2 in range(4):
                    o, v = i0 * ds[0] + i1 * ds[1] + i2 * ds[2], s[i0 * ss[0] + i1 * ss[1] + i2 * ss[2]]
                    want[o] = want[o] + v if acc else v
        np.testing.assert_array_equal(R.permute3(d0, s, shape, ds, ss, acc), want)


def test_norm_references_against_loops():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(3, 5))
    x[1] = 1.5                                                     # constant row: std 0, eps decides
    a2, b2 = rng.normal(size=5), rng.normal(size=5)
    for eps in (1e-6, 1e-3):
        y = R.layernorm_act(x, a2, b2, eps, relu=False)
        for r in range(3):
            m = sum(x[r]) / 5
            sd = (sum((v - m) ** 2 for v in x[r]) / 4) ** 0.5
            for ch in range(5):
                assert abs(y[r, ch] - (a2[ch] * (x[r, ch] - m) / (sd + eps) + b2[ch])) < 1e-12
        np.testing.assert_array_equal(y[1], b2)
        np.testing.assert_array_equal(R.layernorm_act(x, a2, b2, eps, relu=True), np.maximum(y, 0))
    # the wrong reference that forgets the last column must fail the GPU test's comparison (1e-5 * max(1, |y|))
    y = R.layernorm_act(x, a2, b2, 1e-6, False)
    wrong = np.concatenate([R.layernorm_act(x[:, :4], a2[:4], b2[:4], 1e-6, False), y[:, 4:]], axis=1)
    assert (np.abs(wrong - y) > 1e-5 * np.maximum(1, np.abs(y))).any()
    kp = rng.random(size=(6, 2)).astype(np.float32) * 300
    norm3 = np.array([[160, 120, 224], [320, 240, 448], [50, 70, 91]], np.float32)
    seg = np.array([0, 0, 2, 2, 2, 0])
    kn = R.normalize_keypoints_f32(kp, norm3, seg)
    w1, b1 = rng.normal(size=(3, 2)), rng.normal(size=3)
    lin = R.kenc_first(kp, norm3, seg, w1, b1, relu=False)
    for i in range(6):
        c = norm3[seg[i]]
        assert kn[i, 0] == np.float32(np.float32(kp[i, 0] - c[0]) / c[2]) and kn[i, 1] == np.float32(np.float32(kp[i, 1] - c[1]) / c[2])
        for ch in range(3):
            want = w1[ch, 0] * (float(kp[i, 0]) - c[0]) / c[2] + w1[ch, 1] * (float(kp[i, 1]) - c[1]) / c[2] + b1[ch]
            assert abs(lin[i, ch] - want) < 1e-12
    assert (lin < 0).any()
    np.testing.assert_array_equal(R.kenc_first(kp, norm3, seg, w1, b1, relu=True), np.maximum(lin, 0))


def test_split_plane_helpers():
    assert R.spl_col(np.array([0, 31, 32, 63, 64, 259])).tolist() == [0, 31, 64, 95, 128, 515]
    x = np.array([1.0, 1.00390625, 1.01171875, -3.1415927, 65504.0, 1e-30, 0.0], np.float32)   # 1 + 2^-8: a tie, rounds to even (down);
    bits = R.bf16_bits(x)                                                                      # 1 + 3 * 2^-8: a tie, rounds to even (up)
    assert bits[0] == 0x3F80 and bits[1] == 0x3F80 and bits[2] == 0x3F82 and bits[6] == 0
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(bits, want)
    np.testing.assert_array_equal(R.bf16_value(bits), torch.from_numpy(x).to(torch.bfloat16).float().numpy())


def test_training_helper_references_against_loops():
    rng = np.random.default_rng(3)
    x = rng.integers(-8, 9, size=(300, 8))
    prev = 2 * rng.integers(-4, 5, size=8)
    loop = [sum(int(x[r, ch]) for r in range(300)) for ch in range(8)]
    assert R.colsum(x).tolist() == loop
    np.testing.assert_array_equal(R.colsum(x, prev, -0.5), np.array(loop) - 0.5 * prev)
    # wrong references: the last row block (rows 256 ..) or the last column group dropped
    with pytest.raises(AssertionError):
        np.testing.assert_array_equal(R.colsum(x), R.colsum(x[:256]))
    with pytest.raises(AssertionError):
        np.testing.assert_array_equal(R.colsum(x), np.r_[R.colsum(x)[:4], np.zeros(4, np.int64)])
    z = rng.normal(size=(4, 7)) * 30
    p = R.softmax(z)
    for r in range(4):
        e = [np.exp(v - max(z[r])) for v in z[r]]
        np.testing.assert_allclose(p[r], np.array(e) / sum(e), rtol=1e-14)
    assert np.abs(p.sum(-1) - 1).max() < 1e-15
    assert np.abs(R.softmax(z[:, :6]) - p[:, :6]).max() > 2e-5        # a reference without the last column fails the GPU test's bar
    dp = rng.normal(size=(4, 7))
    ds = R.softmax_backward(p, dp)
    for r in range(4):
        dot = sum(p[r, j] * dp[r, j] for j in range(7))
        np.testing.assert_allclose(ds[r], [p[r, j] * (dp[r, j] - dot) for j in range(7)], rtol=1e-13, atol=1e-16)
    # finite-difference check of the reverse formula against the forward reference
    eps = 1e-6
    num = np.array([[(((R.softmax(z[r] + eps * np.eye(7)[j]) - R.softmax(z[r] - eps * np.eye(7)[j])) / (2 * eps)) * dp[r]).sum() for j in range(7)]
                    for r in range(4)])
    np.testing.assert_allclose(ds, num, atol=1e-8)
    a = np.array([[-0.0, 0.0, np.nan, 2.0, -3.0]])
    b = np.array([[1.0, -0.0, 5.0, np.nan, 1.0]])
    assert R.elementwise("relu", a).tolist() == [[0.0, 0.0, 0.0, 2.0, 0.0]]
    rm = R.elementwise("relu_mask", a, b)
    assert rm[0, [0, 1, 3, 4]].tolist() == [0.0, 0.0, 0.0, -3.0] and np.isnan(rm[0, 2])
    av, bv, ov = np.array([[1.0, -2.0]]), np.array([[3.0, 5.0]]), np.array([[10.0, 20.0]])
    assert R.elementwise("scale", av, alpha=-2).tolist() == [[-2.0, 4.0]]
    assert R.elementwise("add", av, bv, alpha=0.5).tolist() == [[2.5, 0.5]]
    assert R.elementwise("acc", av, alpha=-2, out_prev=ov).tolist() == [[8.0, 24.0]]
