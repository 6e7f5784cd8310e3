"""GPU tests of image-set matching: the row-assembly kernel alone (GIMS_AUX_ASSEMBLE_ROWS, gims_amd/csrc/features.hip) against
the NumPy restatement (tests/features_ref.py) AND hip.split_spl32 of the gathered rows, bit for bit; then GMatcher.encode_images /
match_features against match_pairs on the same pairs, bit for bit.

Shapes.  The kernel: segments of 1, 7, 300 and 2 rows (a wave takes 4 consecutive rows, a workgroup 16: segments below a wave's rows, across
workgroups, and ends that fall inside a wave), k = 256 (one 16-byte step per lane) and k = 128 (half the lanes idle), 513 one-row segments
(a ten-level search), clipping, empty segments, gaps, either output alone.  End to end: the ragged batch of tests/test_kenc_early_gpu.py --
one build that keeps 284 / 294 of 300 keypoints, one that keeps a few dozen of 512, one that keeps all 256."""
import numpy as np
import pytest
import torch

from gims_amd import GMatcher, Matching, hip, synth, verify_pairs
from tests import features_ref as R
from tests.helpers import pair_to_data

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SPECIAL = np.array([1.0, -0.0, 1 + 2.0 ** -9, 3e38, 1e-40], dtype=np.float32)
SENT_F, SENT_S = -7.0, 0x1234


def _bits(t):
    return t.contiguous().cpu().view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def _store(rows, cols, seed, pitch=None, first=0):
    """A store of encoded rows: standard normal with the special values sprinkled in; pitch / first: a view into a larger allocation."""
    r = np.random.default_rng(seed)
    a = r.normal(size=(rows, cols)).astype(np.float32)
    flat = a.reshape(-1)
    flat[r.choice(flat.size, size=min(flat.size, 5 * max(1, rows // 4)), replace=False)] = np.resize(SPECIAL, min(flat.size, 5 * max(1, rows // 4)))
    if pitch is None:
        return torch.from_numpy(a).cuda()
    big = torch.full((rows + first + 3, pitch), 99.0, device="cuda")
    big[first:first + rows, :cols] = torch.from_numpy(a).cuda()
    return big[first:first + rows, :cols]


def _outputs(n_rows, ld_out, ld_split, which):
    out = torch.full((n_rows + 1, ld_out), SENT_F, device="cuda") if which != "split" else None
    spl = torch.full((n_rows + 1, ld_split), SENT_S, dtype=torch.int16, device="cuda").view(torch.bfloat16) if which != "out" else None
    return out, spl


def _check(segs, n_rows, k, out, spl, ld_out, ld_split):
    """out / spl (with their sentinel row) against the restatement on the sentinel-filled arrays, and the covered rows against
    hip.split_spl32 of the gathered rows."""
    torch.cuda.synchronize()
    host = [(s.cpu().numpy(), f) for s, f in segs]
    want_out = np.full((n_rows + 1, ld_out), SENT_F, dtype=np.float32) if out is not None else None
    want_spl = np.full((n_rows + 1, ld_split), SENT_S, dtype=np.uint16) if spl is not None else None
    R.assemble(sorted(host, key=lambda e: e[1]), k, None if out is None else want_out[:n_rows], None if spl is None else want_spl[:n_rows])
    if out is not None:
        np.testing.assert_array_equal(_bits(out), want_out.view(np.int32))
        assert (out[n_rows] == SENT_F).all()
    if spl is not None:
        np.testing.assert_array_equal(_bits(spl), want_spl.view(np.int16))
        assert (_bits(spl[n_rows]) == SENT_S).all()
    covered = [(f + j, s[j, :k]) for s, f in segs for j in range(s.shape[0]) if 0 <= f + j < n_rows]
    rows = torch.tensor([r for r, _ in covered], device="cuda")
    gathered = torch.stack([v for _, v in covered]).contiguous()
    if out is not None:
        np.testing.assert_array_equal(_bits(out[rows][:, :k]), _bits(gathered))
    if spl is not None:
        np.testing.assert_array_equal(_bits(spl[rows][:, :2 * k]), _bits(hip.split_spl32(gathered)))


def _four_segments(k):
    """1, 7, 300 and 2 rows from three stores: one used twice, one with a pitch of 320 floats whose first row is not row 0 of its allocation."""
    a, b, c = _store(7, k, 1), _store(300, k, 2, pitch=320, first=5), _store(2, k, 3)
    assert b.stride(0) == 320 and b.storage_offset() == 5 * 320
    return [(c[:1], 0), (a, 1), (b, 8), (c, 308)], 310


@pytest.mark.parametrize("k,ld_out,ld_split", [(256, 256, 512), (128, 192, 320)])
def test_segments_from_three_stores(k, ld_out, ld_split):
    """... and, at k = 128, outputs wider than the rows: the columns past k / 2 k keep the sentinel."""
    segs, n_rows = _four_segments(k)
    out, spl = _outputs(n_rows, ld_out, ld_split, "both")
    keep = hip.assemble_rows(segs[::-1], out[:n_rows], spl[:n_rows], k)              # (any order: the binding sorts by destination)
    assert keep.shape == (4, 4) and keep.dtype == torch.int64
    _check(segs, n_rows, k, out, spl, ld_out, ld_split)


def test_513_segments_of_one_row():
    store = _store(64, 256, 4)
    pick = np.random.default_rng(5).integers(0, 64, size=513)
    segs = [(store[int(p):int(p) + 1], r) for r, p in enumerate(pick)]
    out, spl = _outputs(513, 256, 512, "both")
    hip.assemble_rows(segs, out[:513], spl[:513], 256)
    _check(segs, 513, 256, out, spl, 256, 512)


def _raw(table, n_rows, k, out, spl):
    """A hand-made table through the op (what the binding's host checks would refuse or never build)."""
    tab = hip.upload(np.asarray(table, dtype=np.int64), "cuda")
    hip.run_ops(hip.make_ops([hip.op_assemble_rows(tab, len(table), n_rows, k, None if out is None else out[:n_rows], None if spl is None else spl[:n_rows])]))


def test_last_segment_overruns_and_is_clipped():
    a, b = _store(5, 256, 6), _store(40, 256, 7)
    n_rows = 21                                                                     # b would reach row 44
    out, spl = _outputs(n_rows, 256, 512, "both")
    _raw([[a.data_ptr(), 256, 5, 0], [b.data_ptr(), 256, 40, 5]], n_rows, 256, out, spl)
    _check([(a, 0), (b, 5)], n_rows, 256, out, spl, 256, 512)


@pytest.mark.parametrize("empty_first", [True, False])
def test_zero_row_segments_are_skipped(empty_first):
    """An empty segment (rows 0, and rows < 0) holds nothing, wherever equal first rows put it next to the segment that does hold the row."""
    a, b = _store(6, 256, 8), _store(9, 256, 9)
    ea, eb = [b.data_ptr(), 256, 0, 6], [a.data_ptr(), 256, -3, 6]
    real = [b.data_ptr(), 256, 9, 6]
    table = [[a.data_ptr(), 256, 6, 0]] + ([ea, eb, real] if empty_first else [real, ea, eb]) + [[a.data_ptr(), 256, 0, 15]]
    out, spl = _outputs(15, 256, 512, "both")
    _raw(table, 15, 256, out, spl)
    _check([(a, 0), (b, 6)], 15, 256, out, spl, 256, 512)


def test_a_gap_in_the_destination_keeps_what_was_there():
    a, b = _store(7, 256, 10), _store(18, 256, 11)
    segs = [(a, 2), (b, 14)]                                                        # rows 0 - 1 and 9 - 13 belong to nobody
    out, spl = _outputs(32, 256, 512, "both")
    hip.assemble_rows(segs, out[:32], spl[:32], 256)
    _check(segs, 32, 256, out, spl, 256, 512)
    assert (out[9:14] == SENT_F).all() and (out[:2] == SENT_F).all() and (_bits(spl[9:14]) == SENT_S).all()


@pytest.mark.parametrize("which", ["out", "split"])
def test_one_output_alone(which):
    segs, n_rows = _four_segments(256)
    out, spl = _outputs(n_rows, 256, 512, which)
    hip.assemble_rows(segs, None if out is None else out[:n_rows], None if spl is None else spl[:n_rows], 256)
    _check(segs, n_rows, 256, out, spl, 256, 512)


def test_binding_refuses_what_the_device_cannot_check():
    a = _store(7, 256, 12)
    out, spl = _outputs(10, 256, 512, "both")
    with pytest.raises(ValueError, match="overlap"):
        hip.assemble_rows([(a, 0), (a[:2], 6)], out[:10], spl[:10], 256)
    with pytest.raises(ValueError, match="outside"):
        hip.assemble_rows([(a, 4)], out[:10], spl[:10], 256)
    with pytest.raises(ValueError, match="is on"):
        hip.assemble_rows([(a.cpu(), 0)], out[:10], spl[:10], 256)
    with pytest.raises(ValueError, match="both None"):
        hip.assemble_rows([(a, 0)], None, None, 256)
    torch.cuda.synchronize()
    assert (out == SENT_F).all()


def test_op_replays_in_a_table_and_in_a_graph():
    """GIMS_AUX_ASSEMBLE_ROWS next to GIMS_AUX_SPLIT_SPL32 in one gims_run_ops table, and the same table as a HIP graph launched twice."""
    segs, n_rows = _four_segments(256)
    x = torch.randn(64, 128, device="cuda")
    want_split = hip.split_spl32(x)
    tab = hip.upload(hip.assemble_table(segs, n_rows, 256, "cuda"), "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out, spl = _outputs(n_rows, 256, 512, "both")
        split = torch.zeros_like(want_split)
        ops = hip.make_ops([hip.op_assemble_rows(tab, len(segs), n_rows, 256, out[:n_rows], spl[:n_rows]),
                            hip.op_aux(hip.AUX_SPLIT_SPL32, (x, split), (x.stride(0), split.stride(0), 64, 128))])
        hip.run_ops(ops)
        _check(segs, n_rows, 256, out, spl, 256, 512)
        assert torch.equal(split, want_split)
        graph = hip.OpsGraph(ops)
        for _ in range(2):
            out.fill_(SENT_F)
            spl.view(torch.int16).fill_(SENT_S)
            split.zero_()
            graph.launch()
            side.synchronize()
            _check(segs, n_rows, 256, out, spl, 256, 512)
            assert torch.equal(split, want_split)
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------------------------------------ end to end
# (pair, graph setting): "most" keeps 284 and 294 of 300 (294 is no multiple of 4), "few" a few dozen of 512, "full" all 256
PAIRS = [(dict(n=300, seed=2003, canvas=(200, 150)), (15, 50, 5)), (dict(n=512, seed=2000, canvas=(800, 600)), (15, 2, 7)), (dict(n=256, seed=1003), (25, 7, 8))]
OUT_KEYS = ("matches0", "matches1", "matching_scores0", "matching_scores1", "mdesc0", "mdesc1", "keypoints0", "keypoints1", "descriptors0", "descriptors1")


def _pair(spec):
    return synth.make_pair(spec["n"], spec["seed"], **({"canvas": spec["canvas"]} if "canvas" in spec else {}))


def _datas(delaunay=False):
    return [dict(pair_to_data(_pair(spec), *graph, device="cuda"), delaunay=delaunay) for spec, graph in PAIRS]


def _images(delaunay=False):
    """The six images of PAIRS as encode_images takes them, and one graph setting each."""
    images, each = [], []
    for spec, graph in PAIRS:
        pair = _pair(spec)
        for s in "01":
            images.append({"keypoints": torch.from_numpy(pair["keypoints" + s]).cuda(), "descriptors": torch.from_numpy(pair["descriptors" + s]).cuda(),
                           "scores": torch.from_numpy(pair["scores" + s]).cuda(), "image": pair["image" + s]})
            each.append(graph + (delaunay,))
    return images, each


def _model(sd, **cfg):
    m = GMatcher(cfg).eval()
    m.load_state_dict(sd)
    return m


def _same(outs, want, keys=OUT_KEYS):
    assert len(outs) == len(want)
    for p, (a, b) in enumerate(zip(outs, want)):
        for k in keys:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (p, k, a[k].shape, b[k].shape)
            np.testing.assert_array_equal(_bits(a[k]) if a[k].dtype != torch.int64 else a[k].cpu().numpy(),
                                          _bits(b[k]) if b[k].dtype != torch.int64 else b[k].cpu().numpy(), err_msg=f"pair {p}: {k}")


@pytest.mark.parametrize("attention", ["bf16x3", "bf16"])
def test_match_features_equals_match_pairs(synth_sd, attention):
    a, b = _model(synth_sd, attention_precision=attention), _model(synth_sd, attention_precision=attention)
    images, each = _images()
    feats = a.encode_images(images, each=each)
    outs = a.match_features(feats, [(0, 1), (2, 3), (4, 5)])
    cap = {}
    orig = b._encoder

    def spy(P, G):
        sage, desc = orig(P, G)
        cap["desc"] = desc.clone()
        return sage, desc
    b._encoder = spy
    datas = _datas()
    want = b.match_pairs(datas, per_pair_graph=True)
    torch.cuda.synchronize()
    kept = [f.n for f in feats]
    assert kept[:2] == [284, 294] and 0 < kept[2] < 200 and 0 < kept[3] < 200 and kept[4:] == [256, 256], kept
    np.testing.assert_array_equal(_bits(torch.cat([f.encoded for f in feats])), _bits(cap["desc"]))
    for p, d in enumerate(datas):
        for s in (0, 1):
            f = feats[2 * p + s]
            assert torch.equal(f.kept, d["kept_kpts%d_indices" % s][0]) and f.kept.dtype == torch.int32
            np.testing.assert_array_equal(_bits(f.keypoints), _bits(d["keypoints%d" % s][0]))
            np.testing.assert_array_equal(_bits(f.descriptors), _bits(d["descriptors%d" % s][0].t()))
            np.testing.assert_array_equal(_bits(f.scores), _bits(d["scores%d" % s][0]))
            assert f.n_edges == d["graph%d" % s][0].num_edges() == f.graph.num_edges() and f.setting == PAIRS[p][1] + (False,)
            assert f.encoded.shape == (f.n, 256) and f.shape == tuple(_pair(PAIRS[p][0])["image%d" % s].shape)
    _same(outs, want)
    assert outs.flat[0]["n0"] == want.flat[0]["n0"] and torch.equal(outs.flat[0]["matches0"], want.flat[0]["matches0"])
    assert [sorted(d) for d in outs.datas] == [sorted(k for k in d if k not in ("device", "radius", "percentile", "min_size", "delaunay")) for d in datas]
    with pytest.raises(AttributeError):
        feats[0].n = 3


def test_auto_attention_sees_the_same_batches(synth_sd):
    """attention_precision='auto': the first batch calibrates, the second runs on the tiers the first one's statistic chose."""
    a, b = _model(synth_sd), _model(synth_sd)
    images, each = _images()
    feats = a.encode_images(images, each=each)
    for _ in range(2):
        outs = a.match_features(feats, [(0, 1), (2, 3), (4, 5)])
        want = b.match_pairs(_datas(), per_pair_graph=True)
        torch.cuda.synchronize()
        _same(outs, want)
    ra, rb = a.attention_report(), b.attention_report()
    assert ra is not None and ra.keys() == rb.keys()
    for k in ra:
        np.testing.assert_array_equal(np.asarray(ra[k]), np.asarray(rb[k]), err_msg=k)


@pytest.mark.parametrize("delaunay", [False, True])
def test_one_to_many(synth_sd, delaunay):
    """Image 0 of the 256 pair against its own partner and the two images of the 300 pair, all at 25 / 7 / 8 (or all Delaunay) -- match_pairs on
    three dicts that repeat the anchor -- and a pair (i, i), which matches every kept keypoint to itself."""
    a, b = _model(synth_sd, attention_precision="bf16x3"), _model(synth_sd, attention_precision="bf16x3")
    images, _ = _images()
    feats = a.encode_images(images, radius=25, percentile=7, min_size=8, delaunay=delaunay)
    outs = a.match_features(feats, [(4, 5), (4, 0), (4, 1), (4, 4)])
    datas = []
    for j in (5, 0, 1):
        d = {"device": torch.device("cuda"), "radius": 25, "percentile": 7, "min_size": 8, "delaunay": delaunay}
        for s, im in (("0", images[4]), ("1", images[j])):
            d.update({"keypoints" + s: im["keypoints"], "descriptors" + s: im["descriptors"], "scores" + s: im["scores"], "image" + s: im["image"]})
        datas.append(d)
    want = b.match_pairs(datas)
    torch.cuda.synchronize()
    _same(outs[:3], want)
    if delaunay:
        assert [f.n for f in feats] == [300, 300, 512, 512, 256, 256]
    me = outs[3]
    assert torch.equal(me["matches0"][0], torch.arange(feats[4].n, device="cuda")) and torch.equal(me["matches1"], me["matches0"])


@pytest.mark.parametrize("variant", ["f32", "layernorm"])
def test_other_configurations(synth_sd, variant):
    """linear_precision='f32' has no SPL32 copy of the residual stream (the launch writes `out` alone); use_layernorm=True runs other tables."""
    cfg = dict(linear_precision="f32", attention_precision="bf16") if variant == "f32" else dict(use_layernorm=True)
    sd = synth.make_state_dict(123, use_layernorm=True) if variant == "layernorm" else synth_sd
    a, b = _model(sd, **cfg), _model(sd, **cfg)
    images, _ = _images()
    feats = a.encode_images(images[4:], radius=25, percentile=7, min_size=8)
    outs = a.match_features(feats, [(0, 1)])
    want = b.match_pairs([_datas()[2]])
    torch.cuda.synchronize()
    _same(outs, want)


def _count_syncs(monkeypatch):
    counts = {"device": 0, "stream": 0, "event": 0}
    for name, owner, attr in (("device", torch.cuda, "synchronize"), ("stream", torch.cuda.Stream, "synchronize"), ("event", torch.cuda.Event, "synchronize")):
        orig = getattr(owner, attr)

        def counted(*a, _orig=orig, _name=name, **kw):
            counts[_name] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(owner, attr, counted)
    return counts


@pytest.mark.parametrize("attention", ["auto", "bf16x3"])
def test_match_features_builds_nothing_and_does_not_synchronise(synth_sd, monkeypatch, attention):
    """No graph build, no gather, no host synchronisation during match_features.  With a fixed attention precision that holds for every call;
    with 'auto' for the first call, and a later call waits ONCE, on the event behind the previous batch's statistic read-back (every 'auto'
    batch folds the previous batch's measurement in before it picks its kernels: that is what keeps its choices independent of timing)."""
    m = _model(synth_sd, attention_precision=attention)
    images, each = _images()
    feats = m.encode_images(images, each=each)
    torch.cuda.synchronize()

    def boom(*a, **kw):
        raise AssertionError("match_features reached a graph build or a gather")
    for name in ("_run_build", "_gather", "_encoder"):
        monkeypatch.setattr(m, name, boom)
    for name in ("agc_build", "agc_build_each", "delaunay_build"):
        monkeypatch.setattr(hip, name, boom)
    counts = _count_syncs(monkeypatch)
    first = m.match_features(feats, [(0, 1), (2, 3), (4, 5)])
    assert counts == {"device": 0, "stream": 0, "event": 0}, counts
    second = m.match_features(feats, [(0, 1), (2, 3), (4, 5)])
    assert counts == {"device": 0, "stream": 0, "event": 1 if attention == "auto" else 0}, counts
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(int((o["matches0"] > -1).sum()) > 0 for o in first) and len(second) == 3


def test_stale_and_wrong_arguments_raise(synth_sd):
    m = _model(synth_sd, attention_precision="bf16x3")
    images, _ = _images()
    feats = m.encode_images(images[4:])
    with pytest.raises(ValueError, match="empty"):
        m.match_features(feats, [])
    for bad in [(0, 2), (-1, 0), (2, 2)]:
        with pytest.raises(ValueError, match="out of range"):
            m.match_features(feats, [(0, 1), bad])
    other = _model(synth_sd, attention_precision="bf16x3")
    with pytest.raises(ValueError, match="another matcher"):
        other.match_features(feats, [(0, 1)])
    with pytest.raises(ValueError, match="empty"):
        m.encode_images([])
    with pytest.raises(ValueError, match="need at least one array to concatenate"):      # an image that keeps nothing: what the reference raises
        m.encode_images(images[:2], radius=15, percentile=50, min_size=100000)
    assert len(m.match_features(feats, [(0, 1)])) == 1
    m.load_state_dict(synth.make_state_dict(124))
    with pytest.raises(ValueError, match="weight generation"):
        m.match_features(feats, [(0, 1)])
    feats = m.encode_images(images[4:])                                                    # encoded again, they serve
    assert len(m.match_features(feats, [(1, 0)])) == 1
    torch.cuda.synchronize()


def test_matching_extract_and_match_features(synth_sd):
    """The front end runs once for the image list.  attention_precision='bf16x3' is the configuration whose results do not depend on what shares
    a batch with a pair (tests/test_sweep_gpu.py), so a pair of the set is compared with Matching.forward on that pair alone, bit for bit; the
    verification records are compared with those of the match_pairs run of the same pairs."""
    pairs = [_pair(PAIRS[2][0]), synth.make_pair(256, 1002)]
    flat = [(p, s) for p in pairs for s in "01"]
    calls = []

    def front_end(d, device):
        calls.append(d["image"])
        assert d["max_keypoints"] == -1 and d["carhynet"] == "the-net"
        one = lambda key: [torch.from_numpy(p[key + s][0]).to(device) for p, s in flat]      # noqa: E731
        return {"keypoints": one("keypoints"), "scores": one("scores"), "descriptors": one("descriptors")}

    m = Matching({"front_end": front_end, "attention_precision": "bf16x3"}).eval()
    m.gmodel.load_state_dict(synth_sd)
    dev = torch.device("cuda")
    setting = {"radius": 15, "percentile": 2, "min_size": 7}
    feats = m.extract({"image": [p["image" + s] for p, s in flat], "carhynet": "the-net", "device": dev, **setting})
    assert len(calls) == 1 and len(feats) == 4
    outs = m.match_features(feats, [(0, 1), (2, 3)])
    for p, pair in enumerate(pairs):
        ref = m(pair_to_data(pair, 15, 2, 7, device="cuda"))
        assert torch.equal(outs[p]["matches0"], ref["matches0"]) and torch.equal(outs[p]["matches1"], ref["matches1"])
        np.testing.assert_array_equal(_bits(outs[p]["matching_scores0"]), _bits(ref["matching_scores0"]))
        np.testing.assert_array_equal(_bits(outs[p]["matching_scores1"]), _bits(ref["matching_scores1"]))
    assert len(calls) == 1
    # keypoints given: no front end at all
    given = m.extract({"image": [p["image" + s] for p, s in flat], "device": dev, **setting,
                       **{k: [torch.from_numpy(p[k + s][0]).cuda() for p, s in flat] for k in ("keypoints", "descriptors", "scores")}})
    assert len(calls) == 1 and [f.n for f in given] == [f.n for f in feats]
    datas = [pair_to_data(pair, 15, 2, 7, device="cuda") for pair in pairs]
    want = m.gmodel.match_pairs(datas)
    got_v, want_v = verify_pairs(outs.datas, outs, seed=3), verify_pairs(datas, want, seed=3)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(got_v["records"]), _bits(want_v["records"]))
    np.testing.assert_array_equal(_bits(got_v["homographies"]), _bits(want_v["homographies"]))
    assert float(got_v["records"][:, 2].min()) > 0            # (n_inliers: the synthetic pairs do verify)
