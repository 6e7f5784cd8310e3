"""Nothing is written behind the size a workspace query reports.  Every batched entry point gets a buffer of need + 64 KiB filled with 0x5A,
is told work_bytes = need, and must leave the tail untouched (the pattern of test_hip_kernels.py::test_sinkhorn_workspace_is_not_overrun: an
overrun lands in memory the test owns).  The shapes sit on and around a 256-byte boundary of the int32 / float32 arrays (63, 64, 65 elements),
where a miscounted array shows, plus one ragged pair.  Each case also repeats the call on a fresh workspace of twice the size and asks for
bit-equal outputs (float outputs are compared as their bit patterns: NaN fields of the evaluation records compare equal to themselves)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PAIRS = [(63, 65), (64, 64), (65, 63), (257, 130)]
GUARD = 1 << 16


@pytest.fixture(scope="module")
def hip():
    from gims_amd import hip as H
    H.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return H


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _guarded(need, run):
    """run(work, work_bytes) launches on fresh, zeroed outputs and returns them; once on an exactly sized workspace with a guard band behind
    it, once on a fresh one of 2 x need."""
    assert need > 0
    buf = torch.full((need + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    out = run(buf, need)
    torch.cuda.synchronize()
    assert bool((buf[need:] == 0x5A).all()), "bytes behind the reported workspace size were written"
    big = torch.full((2 * need,), 0x5A, dtype=torch.uint8, device="cuda")
    ref = run(big, 2 * need)
    torch.cuda.synchronize()
    assert len(out) == len(ref)
    for k, (a, b) in enumerate(zip(out, ref)):
        assert torch.equal(_bits(a), _bits(b)), f"output {k} depends on the workspace size"


def _ok(hip, rc, what):
    assert rc == 0, f"{what}: {(hip.load().gims_last_error() or b'').decode()}"


def _keypoint_pairs(seed):
    """Per pair: kpts0 [n0, 2], kpts1 [n1, 2] (the first min(n0, n1) are the warped partners, a pixel of noise), the 3 x 3 homography."""
    r = np.random.default_rng(seed)
    out = []
    for n0, n1 in PAIRS:
        h = np.array([[1.02, 0.03, 4.0], [-0.02, 0.98, -3.0], [1e-5, -2e-5, 1.0]])
        k0 = r.uniform([20, 20], [620, 460], size=(n0, 2))
        p = np.concatenate([k0, np.ones((n0, 1))], 1) @ h.T
        w = p[:, :2] / p[:, 2:]
        k1 = r.uniform([20, 20], [620, 460], size=(n1, 2))
        c = min(n0, n1)
        k1[:c] = w[:c] + r.normal(size=(c, 2))
        out.append((k0.astype(np.float32), k1.astype(np.float32), h.astype(np.float32)))
    return out


@pytest.mark.parametrize("ransac_iters", [0, 1, 65])
def test_eval_pairs(hip, ransac_iters):
    lib = hip.load()
    data = [(_dev(k0), _dev(k1), h) for k0, k1, h in _keypoint_pairs(11)]
    m0 = []
    for (n0, n1), _ in zip(PAIRS, data):
        m = torch.arange(n0, dtype=torch.int64, device="cuda")
        m[m >= min(n0, n1)] = -1
        m[::7] = -1
        m0.append(m)

    def run(work, nbytes):
        outs, arr = [], (hip.EvalPair * len(PAIRS))()
        for i, ((n0, n1), (k0, k1, h)) in enumerate(zip(PAIRS, data)):
            o = [torch.zeros(n0, dtype=torch.int32, device="cuda"), torch.zeros(n0, dtype=torch.uint8, device="cuda"),
                 torch.zeros(16, device="cuda"), torch.zeros(18, device="cuda")]
            sc = torch.full((n0,), 0.5, device="cuda")
            arr[i] = hip.EvalPair(k0.data_ptr(), k1.data_ptr(), m0[i].data_ptr(), sc.data_ptr(), n0, n1, 480, 640, (C.c_float * 9)(*h.reshape(9).tolist()),
                                  *[t.data_ptr() for t in o])
            outs += o + [sc]
        _ok(hip, lib.gims_eval_pairs(arr, len(PAIRS), 3.0, 3, 3.0, ransac_iters, 7, work.data_ptr(), nbytes, hip._stream()), "gims_eval_pairs")
        return outs

    from tests.test_workspace_layout_cpu import fake_eval
    _guarded(int(lib.gims_eval_workspace_bytes(fake_eval(PAIRS), len(PAIRS), ransac_iters)), run)


def test_train_labels(hip):
    lib = hip.load()
    data = [(_dev(k0), _dev(k1), h) for k0, k1, h in _keypoint_pairs(12)]
    hs = _dev(np.stack([h.reshape(9) for _, _, h in data]))
    arr = (hip.LabelPair * len(PAIRS))(*[hip.LabelPair(k0.data_ptr(), k1.data_ptr(), n0, n1) for (n0, n1), (k0, k1, _) in zip(PAIRS, data)])

    def run(work, nbytes):
        rows = torch.zeros((sum(a + b for a, b in PAIRS), 3), dtype=torch.int64, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        _ok(hip, lib.gims_train_labels(arr, len(PAIRS), hs.data_ptr(), 3.0, 3, rows.data_ptr(), total.data_ptr(), work.data_ptr(), nbytes, hip._stream()),
            "gims_train_labels")
        return [rows, total]

    _guarded(int(lib.gims_train_labels_workspace_bytes(arr, len(PAIRS))), run)


def _ot_items(shapes, seed):
    r = np.random.default_rng(seed)
    items = []
    for n, m in shapes:
        zs = torch.zeros((n, (m + 3) // 4 * 4), dtype=torch.float32, device="cuda")
        zs[:, :m] = _dev((r.normal(size=(n, m)) * 3).astype(np.float32))
        items.append(dict(scores=zs, n=n, m=m))
    return items


def _ot_outputs(items):
    """Fresh outputs for every problem, in place in the item dicts; the flat list of them."""
    outs = []
    for it in items:
        n, m = it["n"], it["m"]
        it.update(matches0=torch.zeros(n, dtype=torch.int64, device="cuda"), matches1=torch.zeros(m, dtype=torch.int64, device="cuda"),
                  mscores0=torch.zeros(n, device="cuda"), mscores1=torch.zeros(m, device="cuda"), uv=torch.zeros(n + m + 3, device="cuda"))
        outs += [it[k] for k in ("matches0", "matches1", "mscores0", "mscores1", "uv")]
    return outs


@pytest.mark.parametrize("streamed", [False, True])
def test_sinkhorn_match(hip, streamed):
    """One call whose problems fall into several geometry classes of the on-chip kernel (r2_geom of sinkhorn2d.hip: (nx, nc) = (1, 1) for the
    small ones, (1, 2) for 257 x 130, (2, 16) for 2000 x 1990), so that the on-chip region is carved class after class; then the same list
    through the streamed kernels, which leave that region alone."""
    items = _ot_items(PAIRS + [(2000, 1990)], 13)
    flags = hip.OT_STREAMED if streamed else 0

    def run(work, nbytes):
        outs = _ot_outputs(items)
        probs = hip.make_ot_problems(items)
        assert (hip.sinkhorn_plan(probs, 20, flags) >= 3) == (not streamed)
        hip.sinkhorn_match(probs, 1.0, 20, 0.2, work[:nbytes], flags)
        return outs

    _ot_outputs(items)
    _guarded(hip.sinkhorn_workspace_bytes(hip.make_ot_problems(items)), run)


def test_sinkhorn_history(hip):
    lib = hip.load()
    items = _ot_items(PAIRS, 14)

    def run(work, nbytes):
        _ot_outputs(items)
        outs = [it["uv"] for it in items]
        hists = [torch.zeros(int(lib.gims_sinkhorn_history_floats(it["n"], it["m"], 3)), device="cuda") for it in items]
        hp = (C.c_void_p * len(items))(*[h.data_ptr() for h in hists])
        _ok(hip, lib.gims_sinkhorn_history(hip.make_ot_problems(items), len(items), 1.0, 3, hp, work.data_ptr(), nbytes, hip._stream()), "gims_sinkhorn_history")
        return outs + hists

    _ot_outputs(items)
    _guarded(hip.sinkhorn_workspace_bytes(hip.make_ot_problems(items)), run)


@pytest.mark.parametrize("iters", [3, 129])
def test_sinkhorn_backward(hip, iters):
    """129 iterations exceed the capacity of the low-rank sweep's buffers (128) and take the in-place sweep."""
    lib = hip.load()
    items = _ot_items(PAIRS, 15)
    _ot_outputs(items)
    hists = hip.sinkhorn_history(items, 1.0, iters)
    r = np.random.default_rng(16)
    grads = [_dev(r.normal(size=(it["n"] + 1, it["m"] + 1)).astype(np.float32)) for it in items]
    probs = hip.make_ot_problems(items)
    hp = (C.c_void_p * len(items))(*[h.data_ptr() for h in hists])

    def run(work, nbytes):
        dzs = [g.clone() for g in grads]                       # in place: the loss gradient on entry, d loss / d scores on exit
        dalpha = torch.zeros(len(items), device="cuda")
        dp = (C.c_void_p * len(items))(*[d.data_ptr() for d in dzs])
        _ok(hip, lib.gims_sinkhorn_backward(probs, len(items), 1.0, iters, hp, dp, dalpha.data_ptr(), work.data_ptr(), nbytes, hip._stream()),
            "gims_sinkhorn_backward")
        return dzs + [dalpha]

    _guarded(int(lib.gims_sinkhorn_backward_workspace_bytes(probs, len(items))), run)


def test_nn_match(hip):
    """One mutual and one plain pair in one call."""
    lib = hip.load()
    r = np.random.default_rng(17)
    shapes, mutual, d = [(63, 65), (257, 130)], [1, 0], 64
    ab = [(_dev(r.normal(size=(n0, d)).astype(np.float32)), _dev(r.normal(size=(n1, d)).astype(np.float32))) for n0, n1 in shapes]

    def run(work, nbytes):
        outs, arr = [], (hip.NnPair * len(shapes))()
        for i, ((n0, n1), mu, (a, b)) in enumerate(zip(shapes, mutual, ab)):
            o = [torch.zeros(n0, dtype=dt, device="cuda") for _, dt in hip.NN_OUTPUTS]
            m1, info = torch.zeros(n1, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
            arr[i] = hip.NnPair(a.data_ptr(), b.data_ptr(), d, d, n0, n1, d, mu, 0.8, 0, *[t.data_ptr() for t in o], None, m1.data_ptr() if mu else None,
                                info.data_ptr(), None)
            outs += o + [m1, info]
        _ok(hip, lib.gims_nn_match(arr, len(shapes), 0, work.data_ptr(), nbytes, hip._stream()), "gims_nn_match")
        return outs

    from tests.test_workspace_layout_cpu import fake_nn
    _guarded(int(lib.gims_nn_workspace_bytes(fake_nn(shapes, mutual, d), len(shapes), 0)), run)


def _graph_items(ns, seed, d):
    r = np.random.default_rng(seed)
    items = []
    for n in ns:
        kp = r.uniform(0, 200, size=(n, 2)).astype(np.float32)
        de = None
        if d:
            de = r.normal(size=(n, d)).astype(np.float32)
            de /= np.linalg.norm(de, axis=1, keepdims=True)
        items.append((kp, de, n))
    return items


def _graph_images(hip, data):
    """Fresh, zeroed outputs for every image -> (the output tensors, the descriptor array)."""
    items = [dict(kpts=_dev(kp), desc=None if de is None else _dev(de), kept=torch.zeros(n, dtype=torch.int32, device="cuda"),
                  indptr=torch.zeros(n + 1, dtype=torch.int32, device="cuda"), indices=torch.zeros(64 * n, dtype=torch.int32, device="cuda"),
                  info=torch.zeros(8, dtype=torch.int32, device="cuda")) for kp, de, n in data]
    return [it[k] for it in items for k in ("kept", "indptr", "indices", "info")], hip.make_agc_images(items)


@pytest.mark.parametrize("flags", [0, 1])
def test_agc_build_v(hip, flags):
    """The window flow and the robust flow (flag 1 = GIMS_AGC_ROBUST, which also holds the half similarity matrix), per-image parameters."""
    data = _graph_items([63, 64, 65, 257], 18, 128)
    params = [(15.0, 2.0, 3), (25.0, 5.0, 2), (15.0, 50.0, 1), (20.0, 2.0, 4)]

    def run(work, nbytes):
        outs, images = _graph_images(hip, data)
        hip.agc_build_each(images, params, work[:nbytes], flags)
        return outs

    _guarded(hip.agc_workspace_bytes(_graph_images(hip, data)[1], flags), run)


@pytest.mark.parametrize("n", [63, 64, 65])
def test_delaunay_build(hip, n):
    data = _graph_items([n, 257], 19 + n, 0)

    def run(work, nbytes):
        outs, images = _graph_images(hip, data)
        hip.delaunay_build(images, work[:nbytes])
        return outs

    _guarded(hip.delaunay_workspace_bytes(_graph_images(hip, data)[1]), run)


# ------------------------------------------------------------------------------------------------ the auxiliary functions of gims_run_ops
# Their buffers are laid out by the library's routines and sized through gims_aux_layout (hip.*_out_layout, hip.*_work_bytes,
# hip.diou_nms_workspace_bytes, hip.guided_layout).  Triangulation, resection and the three forms of bundle adjustment write their outputs
# into the buffer itself and take no byte count: `need` is the whole buffer and the outputs are its output regions, compared as bytes.
# The inputs are the smallest fixtures of the ops' own tests that reach every region.
def _region_bytes(views):
    return [v.clone().reshape(-1).view(torch.uint8) for v in views.values() if isinstance(v, torch.Tensor)]


def test_triangulate_tracks(hip):
    """Tracks of 2 .. 65 observations: the short ones, the list of the mid and the list of the long ones."""
    from tests import test_triangulate_gpu as G
    B = G._buffers(G.scene("seams"))

    def run(out, nbytes):
        hip.run_ops(hip.make_ops([G._op(dict(B, out=out), (64, 10))]))
        return _region_bytes(hip.triangulate_views(out, B["T"], B["n_obs"]))

    _guarded(B["layout"]["bytes"], run)


def test_resect_images(hip):
    """Two entries, one of them without keypoints; 17 hypotheses each (one more than a workgroup of the scoring kernel takes)."""
    from tests import test_resect_gpu as G
    B = G._buffers(G.scene("batch"), G.entries("batch", 2), 17)

    def run(out, nbytes):
        hip.run_ops(hip.make_ops([G._op(dict(B, out=out), 8)]))
        return _region_bytes(hip.resect_views(out, B["cams"], 17))

    _guarded(B["layout"]["bytes"], run)


def _two_free(sc):
    """Five images, the first two fixed: the third one fixed as well, which leaves two free cameras."""
    mode = np.array(sc["mode"], np.int32)
    mode[2] = 1
    assert (mode == 2).sum() == 2
    return dict(sc, mode=mode)


def test_bundle_adjust(hip):
    from tests import test_ba_gpu as G
    B = G._buffers(_two_free(G.scene("c5")), 2)

    def run(out, nbytes):
        hip.run_ops(hip.make_ops([G._op(dict(B, out=out), 0.0, 1e-4)]))
        return _region_bytes(hip.ba_views(out, *B["dims"], 2))

    _guarded(B["layout"]["bytes"], run)


def test_bundle_adjust_pcg(hip):
    from tests import test_ba_pcg_gpu as G
    B = G._buffers(_two_free(G.scene("c5")), 2, 8, 1e-6)

    def run(out, nbytes):
        hip.run_ops(hip.make_ops([G._op(dict(B, out=out), 0.0, 1e-4)]))
        return _region_bytes(hip.ba_pcg_views(out, *B["dims"], 2))

    _guarded(B["layout"]["bytes"], run)


def test_bundle_adjust_focal(hip):
    """One focal group over all five images."""
    from tests import test_ba_focal_gpu as G
    sc, group = G.fixture("shared5")
    B = G._buffers(_two_free(sc), group, 2, 8, 1e-6)
    assert B["dims"][4] == 1

    def run(out, nbytes):
        hip.run_ops(hip.make_ops([G._op(dict(B, out=out), 0.0, 1e-4)]))
        return _region_bytes(hip.ba_focal_views(out, *B["dims"][:4], 2, 1))

    _guarded(B["layout"]["bytes"], run)


def test_diou_nms(hip):
    """Three images of 0, 63 and 257 keypoints."""
    from tests import nms_ref
    from tests import test_nms_gpu as G
    sizes = [0, 63, 257]
    parts = [G._dense(m, 300 + b) for b, m in enumerate(sizes)]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    kp4, offs = _dev(G._kp4(np.concatenate([p[0] for p in parts]))), _dev(offsets.astype(np.int32))
    order = _dev(np.concatenate([nms_ref.make_order(p[1]) + offsets[b] for b, p in enumerate(parts)]).astype(np.int32))

    def run(work, nbytes):
        keep, count = torch.zeros(offsets[-1], dtype=torch.int32, device="cuda"), torch.zeros(len(sizes) + 1, dtype=torch.int32, device="cuda")
        hip.run_ops(hip.make_ops([hip.op_diou_nms(kp4, order, offs, keep, count, work[:nbytes], len(sizes), 200, 260, 4.0, 0.3)]))
        return [keep, count]

    _guarded(hip.diou_nms_workspace_bytes(int(offsets[-1]), len(sizes)), run)


def test_build_tracks(hip):
    """Scene A of the op's own tests: six images, more nodes than one scan tile."""
    from tests import test_tracks_gpu as G
    from tests import tracks_ref
    counts, pairs, matches = tracks_ref.scene(**G.SCENE_A)
    B = G._buffers(counts, pairs, matches, None, None)
    assert B["n"] > hip.TRACKS_SCAN_TILE

    def run(work, nbytes):
        outs = dict(track_of=torch.zeros_like(B["track_of"]), out=torch.zeros_like(B["out"]), counters=torch.zeros_like(B["counters"]))
        hip.run_ops(hip.make_ops([G._op(dict(B, work=work.view(torch.int32), work_bytes=nbytes, **outs), None, 2, "keep")]))
        return list(outs.values())

    _guarded(B["work_bytes"], run)


def test_select_pairs(hip):
    """Four images of 33, 64, 31 and 70 rows, 64 channels: blocks of 32 rows that are full, ragged and one more."""
    from tests import test_pairs_gpu as G
    descs = G.scene([33, 64, 31, 70], 64, 5)
    images, keep = G._device(descs, None)
    images = [(t, ld, n, r, n) for t, ld, n, r, _ in images]
    n, d, k = len(descs), 64, 2

    def run(work, nbytes):
        tab = hip.pairs_table(images, hip.pairs_rq(0.8), nbytes)
        outs = [torch.zeros((n, n), dtype=torch.int32, device="cuda"), torch.zeros(hip.pairs_out_layout(n, k)[2], dtype=torch.int32, device="cuda"),
                torch.zeros(8, dtype=torch.int32, device="cuda")]
        hip.run_ops(hip.make_ops([hip.op_select_pairs(tab, *outs, work, n, d, 512, k, 1)]))
        return outs

    _guarded(hip.pairs_work_bytes([im[4] for im in images], d), run)


@pytest.mark.parametrize("flags", [0, 1])
def test_guided_match(hip, flags):
    """One mutual pair under a fundamental matrix and one plain pair under a homography; flag 1 = GIMS_NN_EXHAUSTIVE (no candidate lists)."""
    from tests import test_guided_gpu as G
    cases = [G.case(G.scene(127, 129, 128, G.R.FUNDAMENTAL)), G.case(G.scene(64, 65, 32, G.R.HOMOGRAPHY), mutual=False)]

    def run(work, nbytes):
        items = G.device_items(cases)
        got, tab = hip.guided_match(items, flags, work=work[:nbytes])
        assert got.data_ptr() == work.data_ptr()
        outs = []
        for it in items:
            n0, n1 = it["a"].shape[0], it["b"].shape[0]
            outs += [it[name][:8 if name == "info" else n1 if name in ("cnn1", "matches1") else n0] for name in G._names(it)]
        torch.cuda.synchronize()                                # (the table is host memory the op reads while it is enqueued; the outputs are read after)
        return outs

    _guarded(hip.guided_layout([(127, 129, True), (64, 65, False)], flags)["bytes"], run)
