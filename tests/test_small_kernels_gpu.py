"""The small kernels of gims_amd/csrc/misc.hip and gims_amd/csrc/train.hip alone, at the smallest shapes that reach each branch, against the
plain references of tests/small_ref.py (checked on the CPU in tests/test_small_kernels_cpu.py).

Two devices everywhere:
  * EXACT INPUTS for copies and sums: small integers stored as f32 (distinct per position where a copy is tested), so every f32 partial sum
    is exact in any association and the result must equal the int64 reference bit for bit -- a dropped, doubled or misplaced element cannot
    hide inside a tolerance.
  * GUARD BANDS: every output has a pitch above its width where the entry point takes a pitch, G guard rows before and after, and a
    sentinel prefill (f32: the quiet NaN 0x7FC00000, bf16 planes: 0x7FFF, int32: -7); after the call everything outside the promised
    region still holds the sentinel, compared as raw bits.  Inputs have pitches above their widths with NaN in the padding: a read past
    the width poisons the result.

Case -> branch:
  sage_mean / sage_mean_split (sage_mean_kernel), graph small_ref.sage_graph: 79 nodes (the last workgroup has an idle wave: `node >= n`)
    degree 0: no pass, no division, zero out        degree 1, 3: remainder loop only            degree 4: one unrolled step, no remainder
    degree 5: one step + remainder 1                degree 63: 15 steps + remainder 3            degree 64: one full pass, no second
    degree 65 / 67: second `e0` pass of 1 / 3 (remainder only, after a full pass)                degree 128: two full passes
    degree 131 (last node): third pass with a remainder of 3                                     degree 200 (node 0): fourth pass, count 8
    c = 4: 63 inactive lanes (they read quad 0 and discard)    c = 128: 32 inactive lanes       c = 256: every lane, one `q0` iteration
    c = 260: second `q0` iteration with one active lane        c = 512: two full `q0` iterations
    ldh = c + 4, ldo = c + 8 (split: 2 * roundup(c, 32) + 8); c = 4, 260: the split planes of a partly filled 32-channel block
  sage_mean_transposed (sage_mean_t_kernel), graph small_ref.sym_graph: hub of degree 131 whose neighbour 41 has degree 1, node 40 without
    edges (zero out), c = 4 / 128 / 260 (one lane; 32 lanes; second `q` iteration), float64 reference of its own + the adjoint identity
  ingest (ingest_kernel): n = 1, 63, 64, 65, 130 in one batch (one ragged tile; tile - 1; exactly one tile; one tile + 1; three tiles with the
    early return of the images that end before `max_n`), d = 4, 64, 100, 128 (`d0 + r < d` ragged; one tile; ragged second tile; two tiles),
    ldd = n + 3, ldo = d + 3, a null per-image score (zeros), score_out = None, row offsets with gaps, an n = 0 image in the middle, a batch
    of empty images (no launch)
  pack (pack_graphs_kernel): n_kept = 5, 0, 4100, 1 (4100 > 1024 x 4: the row loop's second trip), n_edges = 12, 0, 262 200, 0 (> 1024 x 256:
    the edge loop's second trip), null scores, the closing indptr entry, row_off / edge_off renumbering
  layernorm_act: c = 2 (c - 1 = 1), 63 / 64 / 65 (one register per lane, ragged / full / second register on lane 0), 100, 256, 511, 512 (all
    eight registers); ACT_NONE and ACT_RELU; f32 only, split only, both; ldx = c + 3, ldo = c + 5; eps decides the constant row
  kenc_first<true> / <false>: n = 1, 1000; c1 = 1, 32, 100 (row = idx / c1 with c1 no power of two, a last block that ends inside a row); an
    empty middle segment
  gather_rows: c = 1, 63, 64, 65, 256 (lane loop: one lane, ragged, one trip, second trip, four trips), n = 1, 5, 123 (idle waves), repeats
  colsum (colsum_kernel): rows = 1, 127, 128, 129 (one row block, ragged / full / a second block of one row), 4096 (32 blocks: exactly one
    step of the final fold), 4097 (33 blocks: second step, `b0 + q < gridDim.y` false for 7 of 8), 4225 (34 blocks); c = 4 (one lane group),
    60 (partial group), 64, 68 (second channel block of 4), 512; beta = 0, 1, -0.5; counters zero on exit: shape A, shape B, shape A again
  softmax_rows_ and its reverse: cols = 1, 2, 63 (three waves contribute the identity), 64, 65, 255, 256 (one full trip), 257 (second trip
    of one thread), 600 (three trips); scale 1 and 30; an all-equal row; a row with one entry 80 above the rest; stride != rows * ld
  elementwise (ew_kernel): all five operations, 1x1, 3x255, 5x256, 2x257, three different pitches, alpha = 1, -2, 0.5, -0.0 / 0.0 / NaN inputs
  permute3: (3, 5, 7), both sides strided, plain and accumulating
  gims_run_ops: one op per auxiliary function in gmatcher.py's argument order, every integer argument distinct
"""
import itertools

import numpy as np
import pytest
import torch

from gims_amd import hip
from gims_amd.gmatcher import GMatcher, LN_EPS
from tests import small_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

G = 4                                                             # guard rows before and after every output
SENTINEL = {torch.float32: 0x7FC00000, torch.bfloat16: 0x7FFF, torch.int32: -7}
_RAW = {torch.float32: (torch.int32, np.int32), torch.bfloat16: (torch.int16, np.int16), torch.int32: (torch.int32, np.int32)}


def guarded(rows, width, ld, dtype=torch.float32):
    """(full, view): a sentinel-filled [rows + 2 G, ld] allocation and its [rows, width] window behind the first G rows."""
    full = torch.full((rows + 2 * G, ld), SENTINEL[dtype], dtype=_RAW[dtype][0], device="cuda").view(dtype)
    return full, full[G:G + rows, :width]


def bits(t):
    """raw bit patterns of a device tensor (int32 / int16 NumPy array)."""
    t = t.detach().contiguous().cpu()
    return t.view(_RAW[t.dtype][0]).numpy()


def check_guard(full, rows, width, written=None):
    """Everything of `full` outside the window's written elements (default: the whole [rows, width] window) still holds the sentinel."""
    b = bits(full)
    mask = np.ones(b.shape, bool)
    mask[G:G + rows, :width] = False if written is None else ~np.broadcast_to(written, (rows, width))
    np.testing.assert_array_equal(b[mask], SENTINEL[full.dtype])


def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def padded(a, ld):
    """[rows, w] values as a device view of a [rows, ld] f32 allocation whose padding columns hold NaN."""
    a = np.asarray(a, dtype=np.float32)
    full = np.full((a.shape[0], ld), np.nan, np.float32)
    full[:, :a.shape[1]] = a
    return torch.from_numpy(full).cuda()[:, :a.shape[1]]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", autouse=True)
def _library():
    hip.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"


@pytest.fixture(scope="module")
def sage_graph():
    indptr, indices = R.sage_graph()
    return indptr, indices, dev(indptr), dev(indices)


@pytest.fixture(scope="module")
def sym_graph():
    indptr, indices = R.sym_graph()
    return indptr, indices, dev(indptr), dev(indices)


# ------------------------------------------------------------------------------------------------ GraphSAGE mean
@pytest.mark.parametrize("c", [4, 128, 256, 260, 512])
def test_sage_mean_exact(sage_graph, c):
    """Integer-valued h in [-8, 8]: every sum is exact (|sum| <= 1600), so the output is the correctly rounded float32(sum) / float32(deg),
    bit for bit; the split form is hip.split_spl32 of that f32 result, bit for bit, and leaves the rest of its 32-channel blocks alone."""
    indptr, indices, ip, ix = sage_graph
    n = R.SAGE_N
    h = np.random.default_rng(c).integers(-8, 9, size=(n, c))
    hd = padded(h, c + 4)
    full, out = guarded(n, c, c + 8)
    hip.sage_mean(hd, ip, ix, out)
    want = R.sage_mean_exact(h, indptr, indices)
    np.testing.assert_array_equal(bits(out), f32_bits(want))
    check_guard(full, n, c)
    c32 = R.roundup(c, 32)
    fs, spl = guarded(n, 2 * c32, 2 * c32 + 8, torch.bfloat16)
    hip.sage_mean_split(hd, ip, ix, spl)
    dense = torch.zeros((n, c32), device="cuda")
    dense[:, :c] = out
    ref = bits(hip.split_spl32(dense))
    cols = R.spl_col(np.arange(c))
    written = np.zeros((n, 2 * c32), bool)
    written[:, cols] = written[:, cols + 32] = True
    got = bits(spl)
    np.testing.assert_array_equal(got[written], ref[written])
    np.testing.assert_array_equal(got[:, cols].view(np.uint16), R.bf16_bits(want))          # the hi plane without the library's help
    check_guard(fs, n, 2 * c32, written)


def test_sage_mean_normal(sage_graph):
    """N(0,1) rows at c = 256 against the float64 mean; atol = 1e-5 is the bar of test_hip_kernels.py::test_sage_mean_and_gather."""
    indptr, indices, ip, ix = sage_graph
    h = np.random.default_rng(1).normal(size=(R.SAGE_N, 256)).astype(np.float32)
    full, out = guarded(R.SAGE_N, 256, 264)
    hip.sage_mean(padded(h, 260), ip, ix, out)
    err = np.abs(out.cpu().numpy().astype(np.float64) - R.sage_mean(h, indptr, indices)).max()
    print(f"sage_mean N(0,1) c=256: max abs error {err:.3e} (bar 1e-5)")
    assert err <= 1e-5
    check_guard(full, R.SAGE_N, 256)


@pytest.mark.parametrize("c", [4, 128, 260])
def test_sage_mean_transposed(sym_graph, c):
    """out_j = sum_{i in N(j)} g_i / deg_i against float64.  Bar per element, derived: every quotient is rounded once (2^-24 relative) and
    the sum adds deg_j terms in f32 (at most deg_j - 1 roundings of partial sums bounded by the sum of magnitudes):
    (deg_j + 2) * 2^-24 * sum_i |g_i| / deg_i.  A node without edges has bar 0: its row is exactly zero."""
    indptr, indices, ip, ix = sym_graph
    n = R.SAGE_N
    rng = np.random.default_rng(10 + c)
    g = rng.normal(size=(n, c)).astype(np.float32)
    gd = padded(g, c + 4)
    full, out = guarded(n, c, c + 8)
    hip.sage_mean_transposed(gd, ip, ix, out)
    got = out.cpu().numpy().astype(np.float64)
    ref, mag = R.sage_mean_transposed(g, indptr, indices)
    deg = np.diff(indptr)[:, None]
    bar = (deg + 2) * 2.0 ** -24 * mag
    worst = (np.abs(got - ref) / np.maximum(bar, 1e-300)).max()
    print(f"sage_mean_transposed c={c}: worst error / bar = {worst:.3f}")
    assert (np.abs(got - ref) <= bar).all()
    assert not got[40].any()
    check_guard(full, n, c)
    # the adjoint identity <mean(h), g> == <h, mean^T(g)>.  Bar, derived the same way from both sides' element bars:
    # sum |g| * (deg + 1) 2^-24 mean(|h|)  +  sum |h| * (deg + 2) 2^-24 mag
    h = rng.normal(size=(n, c)).astype(np.float32)
    fm, mean = guarded(n, c, c + 8)
    hip.sage_mean(padded(h, c + 4), ip, ix, mean)
    lhs = (mean.cpu().numpy().astype(np.float64) * g).sum()
    rhs = (h.astype(np.float64) * got).sum()
    bar = 2.0 ** -24 * ((np.abs(g) * (deg + 1) * R.sage_mean(np.abs(h), indptr, indices)).sum() + (np.abs(h) * (deg + 2) * mag).sum())
    print(f"adjoint identity c={c}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bar {bar:.3e}")
    assert abs(lhs - rhs) <= bar


# ------------------------------------------------------------------------------------------------ ingest
INGEST_NS = [1, 63, 64, 65, 130]


def _ingest_batch(d, ns):
    """host images (kpts, desc [d, n + 3] with NaN padding, score or None, row_off) with a value per position, and the total row count."""
    images, off = [], 2
    for i, n in enumerate(ns):
        kp = (i * 1000 + np.arange(2 * n)).reshape(n, 2).astype(np.float32)
        desc = np.full((d, n + 3), np.nan, np.float32)
        desc[:, :n] = (i << 18) + np.arange(d)[:, None] * 1024 + np.arange(n)[None, :]
        score = None if i == 1 else (i * 256 + np.arange(n) + 0.5).astype(np.float32)
        images.append((kp, desc, score, off))
        off += n + 2 + i                                           # gaps between the images
    return images, off


def _run_ingest(images, d, total, with_score=True):
    keep, items = [], []
    for kp, desc, score, off in images:
        t = (dev(kp), dev(desc), None if score is None else dev(score))
        keep.append(t)
        n = kp.shape[0]
        items.append(hip.IngestImage(t[0].data_ptr() if n else None, t[1].data_ptr() if n else None, desc.shape[1],
                                     None if score is None or not n else t[2].data_ptr(), n, off))
    fd, de = guarded(total, d, d + 3)
    fk, kp_out = guarded(total, 2, 2)
    fs, sc = guarded(total, 1, 1)
    ret = hip.ingest_images(items, d, de, kp_out, sc[:, 0] if with_score else None)
    torch.cuda.synchronize()
    return ret, (fd, de), (fk, kp_out), (fs, sc)


def _check_ingest(images, d, total, outs, with_score=True):
    (fd, de), (fk, kp_out), (fs, sc) = outs
    want_d, want_k, want_s, wr = R.ingest([(k, x[:, :k.shape[0]], s, o) for k, x, s, o in images], d, total)
    np.testing.assert_array_equal(bits(de)[wr], f32_bits(want_d)[wr])
    np.testing.assert_array_equal(bits(kp_out)[wr], f32_bits(want_k)[wr])
    check_guard(fd, total, d, wr[:, None])
    check_guard(fk, total, 2, wr[:, None])
    if with_score:
        np.testing.assert_array_equal(bits(sc)[wr, 0], f32_bits(want_s)[wr])
        check_guard(fs, total, 1, wr[:, None])
    else:
        check_guard(fs, total, 1, np.zeros((total, 1), bool))


@pytest.mark.parametrize("d", [4, 64, 100, 128])
def test_ingest(d):
    images, total = _ingest_batch(d, INGEST_NS)
    _check_ingest(images, d, total, _run_ingest(images, d, total)[1:])
    _check_ingest(images, d, total, _run_ingest(images, d, total, with_score=False)[1:], with_score=False)
    # an image without keypoints in the middle (null pointers, as an empty tensor has): max_n comes from the others
    images, total = _ingest_batch(d, INGEST_NS[:2] + [0] + INGEST_NS[2:])
    _check_ingest(images, d, total, _run_ingest(images, d, total)[1:])


def test_ingest_of_empty_images_makes_no_launch():
    """GMatcher._ingest runs before the graph build's own check of the keypoint counts, which raises the reference's ValueError for an image
    with fewer than two keypoints: the caller relies on ingest RETURNING CLEANLY, so a batch in which every image is empty returns None
    without a launch (the entry point itself refuses max_n = 0: tests/test_small_kernels_cpu.py) and writes nothing."""
    images, total = _ingest_batch(4, [0, 0, 0])
    ret, *outs = _run_ingest(images, 4, total)
    assert ret is None
    for full, _ in outs:
        check_guard(full, total, full.shape[1], np.zeros((total, full.shape[1]), bool))


def test_matcher_without_keypoints_raises_what_the_reference_raises():
    """What the early return above is for, end to end: forward() and sweep() of a pair in which one image, or both, have no keypoints raise
    the reference's ValueError from the graph build's check -- with both empty, the ingest's argument error used to come first."""
    from gims_amd import synth
    from tests.helpers import pair_to_data
    m = GMatcher({}).eval()
    m.load_state_dict(synth.make_state_dict(123))
    m.cuda()
    pair = synth.make_pair(256, 1002)

    def data(empty_sides):
        d = pair_to_data(pair, 15, 2, 7, device="cuda")
        for s in empty_sides:
            d["keypoints" + s], d["descriptors" + s], d["scores" + s] = d["keypoints" + s][:, :0], d["descriptors" + s][:, :, :0], d["scores" + s][:, :0]
        return d

    for sides in ("1", "01"):
        with pytest.raises(ValueError, match="need at least one array"):
            m(data(sides))
        with pytest.raises(ValueError, match="need at least one array"):
            m.sweep(data(sides), [(15, 2, 7)])


# ------------------------------------------------------------------------------------------------ pack
def test_pack_graphs():
    """d = 4, four images; every output exact against NumPy indexing."""
    rng = np.random.default_rng(7)
    d, ldd = 4, 8
    spec = [(9, 5, 12, True), (3, 0, 0, False), (5000, 4100, 262200, True), (2, 1, 0, False)]     # source rows, kept, edges, has score
    images = []
    for i, (N, k, e, has) in enumerate(spec):
        desc = np.full((N, ldd), np.nan, np.float32)
        desc[:, :d] = (i << 20) + np.arange(N)[:, None] * 4 + np.arange(d)[None, :]
        indptr = np.sort(np.r_[0, rng.integers(0, e + 1, size=max(k - 1, 0)), e]).astype(np.int32) if k else np.zeros(1, np.int32)
        images.append(dict(kpts=((i << 16) + np.arange(2 * N)).reshape(N, 2).astype(np.float32), desc=desc,
                           score=(i * 8192 + np.arange(N) + 0.25).astype(np.float32) if has else None,
                           kept=rng.permutation(N)[:k].astype(np.int32), indptr=indptr, indices=rng.integers(0, max(k, 1), size=e).astype(np.int32)))
    want = R.pack(images, d)
    n_rows, n_edges = len(want["seg"]), len(want["indices"])
    assert n_rows == 4106 and n_edges == 262212
    keep, recs = [], []
    for im, (N, k, e, has) in zip(images, spec):
        t = {name: dev(im[name]) for name in ("kpts", "desc", "kept", "indptr", "indices")}
        t["score"] = dev(im["score"]) if has else None
        keep.append(t)
        recs.append((t["kpts"].data_ptr(), t["desc"].data_ptr(), ldd, t["score"].data_ptr() if has else 0,
                     t["kept"].data_ptr() if k else 0, t["indptr"].data_ptr(), t["indices"].data_ptr() if e else 0))
    table = hip.pack_table(recs)
    table["n_kept"], table["n_edges"] = [s[1] for s in spec], [s[2] for s in spec]
    table["row_off"] = np.r_[0, np.cumsum(table["n_kept"])][:-1]
    table["edge_off"] = np.r_[0, np.cumsum(table["n_edges"])][:-1]
    ff, feat = guarded(n_rows, d, d + 4)
    fk, kpts = guarded(n_rows, 2, 2)
    fs, score = guarded(n_rows, 1, 1)
    fg, seg = guarded(n_rows, 1, 1, torch.int32)
    fp, indptr_out = guarded(n_rows + 1, 1, 1, torch.int32)
    fi, indices_out = guarded(n_edges, 1, 1, torch.int32)
    hip.pack_graphs_table(table, d, feat, kpts, score[:, 0], seg[:, 0], indptr_out[:, 0], indices_out[:, 0], n_rows, n_edges)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(feat), f32_bits(want["feat"]))
    np.testing.assert_array_equal(bits(kpts), f32_bits(want["kpts"]))
    hs = want["has_score"]
    np.testing.assert_array_equal(bits(score)[hs, 0], f32_bits(want["score"])[hs])
    np.testing.assert_array_equal(bits(seg)[:, 0], want["seg"])
    np.testing.assert_array_equal(bits(indptr_out)[:, 0], want["indptr"])
    assert int(bits(indptr_out)[n_rows, 0]) == n_edges
    np.testing.assert_array_equal(bits(indices_out)[:, 0], want["indices"])
    check_guard(ff, n_rows, d)
    check_guard(fk, n_rows, 2)
    check_guard(fs, n_rows, 1, hs[:, None])                        # rows of an image without scores are left alone
    check_guard(fg, n_rows, 1)
    check_guard(fp, n_rows + 1, 1)
    check_guard(fi, n_edges, 1)


# ------------------------------------------------------------------------------------------------ LayerNorm + activation
@pytest.mark.parametrize("c", [2, 63, 64, 65, 100, 256, 511, 512])
def test_layernorm_act(c):
    """rows = 7 (the second workgroup has an idle wave); row 2 is constant (std 0: eps decides, y = b2 -- the constant 1.5 keeps the f32 mean
    exact, anything else would turn the mean's rounding error, amplified by 1 / eps, into the result); row 4 is scaled by 1e4.
    Bar: 1e-5 (test_train_kernels_gpu.py::test_layernorm_backward's bar on the forward) scaled by magnitude, 1e-5 * max(1, |y_ref|)."""
    rng = np.random.default_rng(100 + c)
    rows, c32 = 7, R.roundup(c, 32)
    x = (rng.normal(size=(rows, c)) * 1.5 + 0.2).astype(np.float32)
    x[2] = 1.5
    x[4] *= np.float32(1e4)
    a2 = (np.abs(rng.normal(size=c)) + 0.5).astype(np.float32)
    b2 = (rng.normal(size=c) * 0.1).astype(np.float32)
    xd, a2d, b2d = padded(x, c + 3), dev(a2), dev(b2)
    cols = R.spl_col(np.arange(c))
    written = np.zeros((rows, 2 * c32), bool)
    written[:, cols] = written[:, cols + 32] = True
    worst = 0.0
    for eps, act in itertools.product((1e-6, 1e-3), (hip.ACT_NONE, hip.ACT_RELU)):
        ref = R.layernorm_act(x, a2, b2, eps, act == hip.ACT_RELU)
        y_bits = None
        for mode in ("f32", "split", "both"):
            fo, out = guarded(rows, c, c + 5) if mode != "split" else (None, None)
            fs, spl = guarded(rows, 2 * c32, 2 * c32 + 8, torch.bfloat16) if mode != "f32" else (None, None)
            hip.layernorm_act(xd, a2d, b2d, out=out, out_split=spl, act=act, eps=eps)
            if out is not None:
                y = out.cpu().numpy()
                if y_bits is None:
                    y_bits = f32_bits(y)
                    ratio = (np.abs(y.astype(np.float64) - ref) / (1e-5 * np.maximum(1.0, np.abs(ref)))).max()
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (eps, act, ratio)
                    want2 = b2.astype(np.float64) if act == hip.ACT_NONE else np.maximum(b2.astype(np.float64), 0)
                    np.testing.assert_array_equal(y[2], want2.astype(np.float32))          # std 0: (x - mean) = 0 exactly, y = b2
                np.testing.assert_array_equal(f32_bits(y), y_bits)                          # the same bits whatever else is written
                check_guard(fo, rows, c)
            if spl is not None:
                yk = y_bits.view(np.float32)                                                # the kernel's own f32 output
                got = bits(spl).view(np.uint16)
                hi, lo = got[:, cols], got[:, cols + 32]
                np.testing.assert_array_equal(hi, R.bf16_bits(yk))
                # hi + lo within 2^-15 |y|: the bar of test_hip_kernels.py's test_linear_presplit for the split planes
                resid = np.abs(R.bf16_value(hi).astype(np.float64) + R.bf16_value(lo).astype(np.float64) - yk.astype(np.float64))
                assert (resid <= 2.0 ** -15 * np.abs(yk)).all()
                check_guard(fs, rows, 2 * c32, written)                                     # incl. the channels of the last block past c
    print(f"layernorm_act c={c}: worst error / (1e-5 max(1, |y|)) = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ keypoint encoder front end
NORM3 = np.array([[160.0, 120.0, 224.0], [9.0, 9.0, 9.0], [320.5, 240.25, 448.7]], np.float32)     # centre x, centre y, scale per segment


def _keypoints(n):
    kp = (np.random.default_rng(n).random(size=(n, 2)) * 600).astype(np.float32)
    seg = np.where(np.arange(n) < (2 * n) // 5, 0, 2).astype(np.int32)                             # segment 1 is empty
    return kp, seg


@pytest.mark.parametrize("c1", [1, 32, 100])
@pytest.mark.parametrize("n", [1, 1000])
def test_kenc_first(n, c1):
    """rtol = atol = 1e-5: the bar of test_hip_kernels.py::test_kenc_first.  The entry point has no pitch: out is [n, c1] dense, with guard rows."""
    kp, seg = _keypoints(n)
    rng = np.random.default_rng(c1)
    w1, b1 = rng.normal(size=(c1, 2)).astype(np.float32), rng.normal(size=c1).astype(np.float32)
    args = (dev(kp), dev(NORM3), dev(seg), dev(w1), dev(b1))
    for relu in (True, False):
        full, out = guarded(n, c1, c1)
        hip.kenc_first(*args, out, relu=relu)
        got = out.cpu().numpy()
        ref = R.kenc_first(kp, NORM3, seg, w1, b1, relu)
        err = np.abs(got - ref) / (1e-5 + 1e-5 * np.abs(ref))
        print(f"kenc_first n={n} c1={c1} relu={relu}: worst error / bar = {err.max():.3f}")
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)
        check_guard(full, n, c1)
        if relu:
            assert (got >= 0).all()
        elif n > 1:
            assert (got < 0).any()                                 # the linear form keeps its negative values
    if n == 1 and c1 == 100:                                       # one row: still some negative channel in the linear form
        assert (R.kenc_first(kp, NORM3, seg, w1, b1, False) < 0).any() and (got < 0).any()


@pytest.mark.parametrize("n", [1, 1000])
def test_normalize_keypoints(n):
    """(k - centre) / scale: one f32 subtraction and one correctly rounded f32 division -- bit for bit."""
    kp, seg = _keypoints(n)
    out = hip.normalize_keypoints(dev(kp), dev(NORM3), dev(seg))
    assert out.shape == (n, 2)
    np.testing.assert_array_equal(bits(out), f32_bits(R.normalize_keypoints_f32(kp, NORM3, seg)))


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("c", [1, 63, 64, 65, 256])
def test_gather_rows(c):
    src = (np.arange(200)[:, None] * 1024 + np.arange(c)[None, :]).astype(np.float32)              # a value per position, below 2^24
    sd = padded(src, c + 3)
    rng = np.random.default_rng(c)
    for n in (1, 5, 123):
        idx = rng.integers(0, 200, size=n).astype(np.int32)
        if n > 1:
            idx[n // 2] = idx[0]                                   # a repeated index
        full, out = guarded(n, c, c + 5)
        hip.gather_rows(sd, dev(idx), out)
        np.testing.assert_array_equal(bits(out), f32_bits(R.gather_rows(src, idx)))
        check_guard(full, n, c)


# ------------------------------------------------------------------------------------------------ column sums
def _colsum_case(rows, c, beta, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, size=(rows, c))
    prev = 2 * rng.integers(-4, 5, size=c)                         # even: -0.5 * prev stays an integer
    return x, prev, np.asarray(R.colsum(x, prev, beta), dtype=np.float64)


def _run_colsum(xd, prev, beta):
    c = xd.shape[1]
    full, out = guarded(c, 1, 1)
    out[:, 0] = dev(prev.astype(np.float32))
    hip.colsum(xd, out=out[:, 0], beta=beta)                       # the public path: the module's own workspace
    check_guard(full, c, 1)
    return bits(out)[:, 0]


@pytest.mark.parametrize("rows", [1, 127, 128, 129, 4096, 4097, 4225])
def test_colsum_exact(rows):
    """Integers in [-8, 8]: |sum| <= 33 800, every partial sum exact, beta * out an integer -- the int64 reference bit for bit."""
    for c in (4, 60, 64, 68, 512):
        for beta in (0.0, 1.0, -0.5):
            x, prev, want = _colsum_case(rows, c, beta, seed=rows * 1000 + c)
            xd = padded(x, c + 4)
            assert np.abs(want).max() < 2 ** 24
            np.testing.assert_array_equal(_run_colsum(xd, prev, beta), f32_bits(want), err_msg=f"rows {rows} c {c} beta {beta}")


def test_colsum_leaves_its_counters_and_workspace_ready():
    """Shape A, a different shape B, shape A again: the same bits (the counters are zero on exit, stale partials are never read)."""
    xa, pa, wa = _colsum_case(4225, 68, 1.0, seed=1)
    xb, pb, wb = _colsum_case(129, 512, -0.5, seed=2)
    xad, xbd = padded(xa, 72), padded(xb, 516)
    first = _run_colsum(xad, pa, 1.0)
    np.testing.assert_array_equal(first, f32_bits(wa))
    np.testing.assert_array_equal(_run_colsum(xbd, pb, -0.5), f32_bits(wb))
    np.testing.assert_array_equal(_run_colsum(xad, pa, 1.0), first)


def test_colsum_normal():
    """2031 rows of N(0,1) against float64; 2e-4 is the bar of test_train_kernels_gpu.py::test_colsum_elementwise_permute."""
    x = np.random.default_rng(3).normal(size=(2031, 512)).astype(np.float32)
    full, out = guarded(512, 1, 1)
    hip.colsum(padded(x, 516), out=out[:, 0])
    err = np.abs(out[:, 0].cpu().numpy().astype(np.float64) - x.astype(np.float64).sum(0)).max()
    print(f"colsum N(0,1) 2031 x 512: max abs error {err:.3e} (bar 2e-4)")
    assert err <= 2e-4
    check_guard(full, 512, 1)


# ------------------------------------------------------------------------------------------------ softmax rows
def _in_window(full, cols):
    """bool mask of a [batch, 3 + 2 G, ld] allocation: True outside the [batch, 3, cols] window."""
    m = np.ones(tuple(full.shape), bool)
    m[:, G:G + 3, :cols] = False
    return m


@pytest.mark.parametrize("cols", [1, 2, 63, 64, 65, 255, 256, 257, 600])
def test_softmax_rows_and_backward(cols):
    batch, rows, ld = 2, 3, R.roundup(cols + 5, 4)
    for scale in (1.0, 30.0):
        rng = np.random.default_rng(cols * 10 + int(scale))
        z = (rng.normal(size=(batch, rows, cols)) * scale).astype(np.float32)
        z[0, 1, :] = 0.75                                          # all entries equal
        z[1, 2, cols // 2] = (np.delete(z[1, 2], cols // 2).max() if cols > 1 else 0.0) + 80.0     # one entry 80 above the rest
        full = torch.full((batch, rows + 2 * G, ld), float("nan"), device="cuda")
        s = full[:, G:G + rows, :]                                 # stride(0) = (rows + 2 G) * ld != rows * ld
        s[:, :, :cols] = dev(z)
        before = bits(full)
        assert (before[_in_window(full, cols)] == SENTINEL[torch.float32]).all()
        hip.softmax_rows_(s, cols)
        p = s[:, :, :cols].cpu().numpy()
        ref = R.softmax(z)
        err = np.abs(p.astype(np.float64) - ref).max()
        sum_err = np.abs(p.astype(np.float64).sum(-1) - 1.0).max()
        print(f"softmax_rows cols={cols} scale={scale}: max abs error {err:.3e} (bar 2e-5), row sum off by {sum_err / 2.0 ** -23:.2f} x 2^-23 (bar {cols})")
        # 2e-5 absolute on probabilities: the bar of test_train_kernels_gpu.py::test_gemm_batched_strided_heads, which has logits within +-4.
        # It holds unwidened at a spread of +-100 too: __expf's worst case here was 1.9e-7 (cols = 257, scale 30).
        assert err <= 2e-5
        # the row sum: each probability rounded once, the f32 sum of the exponentials and its reciprocal likewise -- cols * 2^-23
        assert sum_err <= cols * 2.0 ** -23
        after = bits(full)
        m = _in_window(full, cols)
        np.testing.assert_array_equal(after[m], before[m])         # padding columns and guard rows untouched
        # reverse pass on the kernel's own probabilities: dS = P * (dP - sum_j dP_j P_j); 1e-6 * max |dP| is the current test's bar, scaled
        g = rng.normal(size=(batch, rows, cols)).astype(np.float32)
        dfull = torch.full((batch, rows + 2 * G, ld), float("nan"), device="cuda")
        dp = dfull[:, G:G + rows, :]
        dp[:, :, :cols] = dev(g)
        dbefore = bits(dfull)
        hip.softmax_rows_backward_(s, dp, cols)
        ds = dp[:, :, :cols].cpu().numpy().astype(np.float64)
        derr = np.abs(ds - R.softmax_backward(p, g)).max()
        print(f"softmax_rows_backward cols={cols} scale={scale}: max abs error {derr:.3e} (bar {1e-6 * np.abs(g).max():.3e})")
        assert derr <= 1e-6 * np.abs(g).max()
        np.testing.assert_array_equal(bits(dfull)[m], dbefore[m])
        np.testing.assert_array_equal(bits(full), after)           # the probabilities are read only


# ------------------------------------------------------------------------------------------------ element-wise
@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 255), (5, 256), (2, 257)])
def test_elementwise(rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    ldo, lda, ldb = cols + 3, cols + 1, cols + 2                   # three different pitches
    a = rng.integers(-8, 9, size=(rows, cols)).astype(np.float32)
    b = rng.integers(-8, 9, size=(rows, cols)).astype(np.float32)
    prev = rng.integers(-8, 9, size=(rows, cols)).astype(np.float32)
    ad, bd = padded(a, lda), padded(b, ldb)
    for alpha in (1.0, -2.0, 0.5):
        al = np.float32(alpha)
        for op, name, want in ((hip.EW_SCALE, "scale", al * a), (hip.EW_ADD, "add", a + al * b), (hip.EW_ACC, "acc", prev + al * a)):
            full, out = guarded(rows, cols, ldo)
            if name == "acc":
                out.copy_(dev(prev))
            hip.elementwise(op, out, ad, bd if name == "add" else None, alpha=alpha)
            # small integers times 1, -2 or 0.5: every product and sum is exact, fused or not; `want` is the same arithmetic in f32 NumPy
            # (it carries the sign of a zero product), the float64 reference states the value
            np.testing.assert_array_equal(bits(out), f32_bits(want), err_msg=f"{name} alpha {alpha}")
            np.testing.assert_array_equal(out.cpu().numpy().astype(np.float64), R.elementwise(name, a, b, alpha, prev))
            check_guard(full, rows, cols)
    # ReLU and its mask at -0.0, 0.0 and NaN.  The kernel writes fmaxf(a, 0) and b > 0 ? a : 0:
    #   fmaxf(NaN, 0) = 0 (the operand that is a number), fmaxf(0.0, 0) = 0.0, fmaxf(-0.0, 0) = a zero whose sign C leaves open;
    #   b = NaN, -0.0, 0.0 are not > 0: the result is 0.0 whatever a is; where b > 0 the bits of a pass through (a NaN, a -0.0 too).
    special = np.array([-0.0, 0.0, np.nan], np.float32)
    x = rng.normal(size=rows * cols).astype(np.float32)
    y = rng.normal(size=rows * cols).astype(np.float32)
    k = min(3, x.size)
    x[:k], y[-k:] = special[:k], special[:k]
    if x.size > 8:
        x[3:6] = special                                           # a = -0.0, 0.0, NaN under b > 0 and under b <= 0
        y[3:6], x[6:9], y[6:9] = 1.0, special, -1.0
    x, y = x.reshape(rows, cols), y.reshape(rows, cols)
    xd, yd = padded(x, lda), padded(y, ldb)
    full, out = guarded(rows, cols, ldo)
    hip.elementwise(hip.EW_RELU, out, xd)
    got = bits(out)
    want = f32_bits(np.where(x > 0, x, np.float32(0)))
    neg_zero = f32_bits(x) == np.int32(-2 ** 31)
    np.testing.assert_array_equal(got[~neg_zero], want[~neg_zero])
    assert ((got[neg_zero] & 0x7FFFFFFF) == 0).all()
    check_guard(full, rows, cols)
    full, out = guarded(rows, cols, ldo)
    hip.elementwise(hip.EW_RELU_MASK, out, xd, yd)
    np.testing.assert_array_equal(bits(out), f32_bits(np.where(y > 0, x, np.float32(0))))
    check_guard(full, rows, cols)


# ------------------------------------------------------------------------------------------------ permute3
def test_permute3_strided_and_accumulating():
    shape, ds, ss = (3, 5, 7), (2, 50, 7), (80, 2, 11)            # both maps one-to-one: 2 a + 7 b and 2 a + 11 b have no collisions here
    d_off, s_off = R.permute3_offsets(shape, ds).ravel(), R.permute3_offsets(shape, ss).ravel()
    assert len(set(d_off.tolist())) == 105 == len(set(s_off.tolist())) and d_off.max() < 250 and s_off.max() < 240
    rng = np.random.default_rng(9)
    src = np.full(240, np.nan, np.float32)
    src[s_off] = rng.permutation(105) - 50                         # a value per element
    written = np.zeros((250, 1), bool)
    written[d_off] = True
    for accumulate in (False, True):
        full, dst = guarded(250, 1, 1)
        prev = np.zeros(250, np.float32)
        if accumulate:
            prev[d_off] = rng.integers(-8, 9, size=105)
            dst[torch.from_numpy(d_off).cuda(), 0] = dev(prev[d_off])
        hip.permute3(dst[:, 0], dev(src), shape, ds, ss, accumulate=accumulate)
        want = R.permute3(prev.astype(np.float64), src.astype(np.float64), shape, ds, ss, accumulate)
        np.testing.assert_array_equal(bits(dst)[d_off, 0], f32_bits(want[d_off]))
        check_guard(full, 250, 1, written)


# ------------------------------------------------------------------------------------------------ auxiliary ops of gims_run_ops
def test_aux_ops_map_their_arguments_like_the_entry_points():
    """One op per auxiliary function, built with hip.op_aux in the argument order gmatcher.py uses (GMatcher._norm_args and the aux(...) calls
    of its sequence builder), replayed with hip.run_ops: the same bits as the direct wrapper call, guard bands included.  Every integer
    argument of an op has a value of its own, so two swapped slots cannot cancel."""
    rng = np.random.default_rng(12)

    def same(run_direct, run_op, make_out):
        outs = []
        for run in (run_direct, run_op):
            full, view = make_out()
            run(view)
            outs.append(bits(full))
        np.testing.assert_array_equal(outs[0], outs[1])
        assert (outs[0] != SENTINEL[full.dtype]).any()             # something was written

    def replay(*op):
        hip.run_ops(hip.make_ops([hip.op_aux(*op)]))

    # SPLIT_SPL32: p = {src, dst}, i = {lds, ldd, rows, k} = 36, 72, 5, 32
    x = padded(rng.normal(size=(5, 32)), 36)
    same(lambda o: hip.split_spl32(x, out=o), lambda o: replay(hip.AUX_SPLIT_SPL32, [x, o], [x.stride(0), o.stride(0), 5, 32]),
         lambda: guarded(5, 64, 72, torch.bfloat16))
    # SAGE_MEAN / SAGE_MEAN_SPLIT: p = {h, indptr, indices, out}, i = {ldh, n, c, ldo} = 12, 7, 8, 16 (split: 72)
    deg = np.array([3, 0, 1, 5, 2, 4, 2])
    ip, ix = dev(np.r_[0, np.cumsum(deg)].astype(np.int32)), dev(rng.integers(0, 7, size=int(deg.sum())).astype(np.int32))
    h = padded(rng.normal(size=(7, 8)), 12)
    same(lambda o: hip.sage_mean(h, ip, ix, o), lambda o: replay(hip.AUX_SAGE_MEAN, [h, ip, ix, o], [h.stride(0), 7, 8, o.stride(0)]),
         lambda: guarded(7, 8, 16))
    same(lambda o: hip.sage_mean_split(h, ip, ix, o), lambda o: replay(hip.AUX_SAGE_MEAN_SPLIT, [h, ip, ix, o], [h.stride(0), 7, 8, o.stride(0)]),
         lambda: guarded(7, 64, 72, torch.bfloat16))
    # KENC_FIRST / KENC_FIRST_LINEAR: p = {kpts, norm3, seg, w1, b1, out}, i = {c1, n} = 5, 9
    kp, seg = _keypoints(9)
    kd, nd, sd = dev(kp), dev(NORM3), dev(seg)
    w1, b1 = dev(rng.normal(size=(5, 2)).astype(np.float32)), dev(rng.normal(size=5).astype(np.float32))
    for fn, relu in ((hip.AUX_KENC_FIRST, True), (hip.AUX_KENC_FIRST_LINEAR, False)):
        same(lambda o: hip.kenc_first(kd, nd, sd, w1, b1, o, relu=relu), lambda o: replay(fn, [kd, nd, sd, w1, b1, o], [5, 9]),
             lambda: guarded(9, 5, 5))
    # LAYERNORM_ACT through GMatcher._norm_args: i = {ldx, rows, c, act, ldo, ld_split} = 44, 3, 40, 1, 48, 136
    xl = padded(rng.normal(size=(3, 40)), 44)
    a2, b2 = dev(rng.normal(size=40).astype(np.float32)), dev(rng.normal(size=40).astype(np.float32))
    fs_d, spl_d = guarded(3, 128, 136, torch.bfloat16)
    fs_o, spl_o = guarded(3, 128, 136, torch.bfloat16)
    same(lambda o: hip.layernorm_act(xl, a2, b2, out=o, out_split=spl_d, act=hip.ACT_RELU, eps=LN_EPS),
         lambda o: replay(*GMatcher._norm_args(xl, (a2, b2), 3, out=o, out_split=spl_o)), lambda: guarded(3, 40, 48))
    np.testing.assert_array_equal(bits(fs_d), bits(fs_o))
    assert (bits(spl_d).view(np.uint16) != 0x7FFF).any()
