"""Per-image graph parameters on the GPU: gims_agc_build with n_params == n_images against the reference's graphs with every image's own triple, the scalar entry
points against it bit for bit, match_pairs(per_pair_graph=True) on a batch of mixed settings and graph kinds, and GMatcher.sweep over the
stored grids of tests/golden/sweep_* (tools/gen_golden_sweep.py), against forward() per setting, and across sub-batch sizes."""
import math
import traceback

import numpy as np
import pytest
import torch

from gims_amd import GMatcher, hip, synth
from tests import dgims_helpers as H
from tests.helpers import compare_with_golden, load_golden, pair_to_data
from tests.test_sweep_cpu import CONFIG, STORED, sweep_fixture

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

AGC_FIXTURES = ("agc_n1024_s2001_r15p2m7", "agc_n1024_s2002_r25p7m8", "agc_n300_s2003_r15p50m5", "agc_n512_s2000_r15p2m7")


def _agc_images():
    """The eight images of the four graph fixtures: (fixture name, side, fixture, kp [n, 2], de [n, d], the fixture's own triple)."""
    out = []
    for name in AGC_FIXTURES:
        g = load_golden(name)
        n, seed, rad, pct, ms, cw, ch = (int(x) for x in g["meta"])
        pair = synth.make_pair(n, seed, canvas=(cw, ch))
        for s in ("0", "1"):
            out.append((name, s, g, pair["keypoints" + s][0], np.ascontiguousarray(pair["descriptors" + s][0].T), (rad, pct, ms)))
    return out


def _build(imgs, call):
    """One batched graph build over imgs [(kp, de)]; call(arr, work) enqueues it.  Per image (kept, indptr, indices, info) as NumPy arrays."""
    items = []
    for kp, de in imgs:
        n = de.shape[0]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()      # noqa: E731
        items.append(dict(kpts=dev(kp), desc=dev(de), kept=torch.full((n,), -3, dtype=torch.int32, device="cuda"),
                          indptr=torch.full((n + 1,), -3, dtype=torch.int32, device="cuda"),
                          indices=torch.full((n * 64,), -3, dtype=torch.int32, device="cuda"),
                          info=torch.full((8,), -3, dtype=torch.int32, device="cuda")))
    arr = hip.make_agc_images(items)
    work = torch.empty(hip.agc_workspace_bytes(arr), dtype=torch.uint8, device="cuda")
    call(arr, work)
    torch.cuda.synchronize()
    out = []
    for it in items:
        inf = it["info"].cpu().numpy()
        nk, ne = int(inf[0]), int(inf[1])
        out.append((it["kept"][:nk].cpu().numpy(), it["indptr"][:nk + 1].cpu().numpy(), it["indices"][:ne].cpu().numpy(), inf))
    return out


def _csr_edges(indptr, indices):
    dst = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    e = np.stack([indices.astype(np.int64), dst], 1)
    e = e[e[:, 0] < e[:, 1]]
    return e[np.lexsort((e[:, 1], e[:, 0]))]


@pytest.mark.parametrize("flags", [0, hip.AGC_ROBUST], ids=["window", "robust"])
def test_one_build_with_each_images_own_parameters(flags):
    """ONE agc_build_each call over the images of four fixtures made with three different triples: kept ids and the final edge list of
    every image equal its fixture (the reference's graph)."""
    ims = _agc_images()
    assert len({im[5] for im in ims}) == 3
    res = _build([(kp, de) for _, _, _, kp, de, _ in ims], lambda arr, work: hip.agc_build_each(arr, [im[5] for im in ims], work, flags=flags))
    for (name, s, g, kp, _, _), (kept, indptr, indices, inf) in zip(ims, res):
        assert int(inf[7]) == 0, (name, s, inf)
        assert int(inf[2]) == len(g[f"agc{s}/coarse"]), (name, s)
        np.testing.assert_array_equal(kept, g[f"agc{s}/kept"], err_msg=f"{name} {s}")
        relabel = -np.ones(len(kp), dtype=np.int64)
        relabel[g[f"agc{s}/kept"]] = np.arange(len(kept))
        ref_e = relabel[g[f"agc{s}/final"]]
        np.testing.assert_array_equal(_csr_edges(indptr, indices), ref_e[np.lexsort((ref_e[:, 1], ref_e[:, 0]))], err_msg=f"{name} {s}")


@pytest.mark.parametrize("flags", [0, hip.AGC_ROBUST], ids=["window", "robust"])
def test_scalar_entry_equals_a_uniform_per_image_call(flags):
    """hip.agc_build (one triple for the batch) and agc_build_each with that triple for every image: bit-identical kept / indptr / indices / info."""
    imgs = [(kp, de) for _, _, _, kp, de, _ in _agc_images()]
    for triple in ((15, 2, 7), (25, 7, 8)):
        a = _build(imgs, lambda arr, work: hip.agc_build(arr, *triple, work, flags=flags))
        b = _build(imgs, lambda arr, work: hip.agc_build_each(arr, [triple] * len(imgs), work, flags=flags))
        for i, (x, y) in enumerate(zip(a, b)):
            for u, v in zip(x, y):
                np.testing.assert_array_equal(u, v, err_msg=f"image {i} {triple}")


def _model(config=None, settle=True):
    m = GMatcher(dict(config or {})).eval()
    m.load_state_dict(synth.make_state_dict(123))
    if settle:
        # attention_precision='auto': the first call after the weights change measures every layer and decides; tests that
        # compare calls with each other, or count host synchronisations, start from the settled state
        m(pair_to_data(synth.make_pair(256, 1002), 15, 2, 7, device="cuda"))
    return m


def _multiset(src, dst):
    e = np.stack([np.asarray(src), np.asarray(dst)], axis=1).astype(np.int64)
    return e[np.lexsort((e[:, 1], e[:, 0]))]


MIXED = ("e2e_n256_s1002_r15p2m7_i100", "e2e_n256_s1003_r25p7m8_i100", "dgims_e2e_n256_s5000_w123_i100")


def _mixed_datas(gs):
    """Fresh input dicts of the three fixtures (match_pairs mutates them), each with its fixture's own graph setting."""
    datas = []
    for nm, g in zip(MIXED, gs):
        if nm.startswith("dgims"):
            assert int(g["meta"][1]) == 123 and int(g["meta"][2]) == 100          # weight seed, iterations
            d = pair_to_data(H.e2e_pair(g["meta"]), 15, 2, 7, device="cuda")
            d["delaunay"] = True
        else:
            n, seed, rad, pct, ms, iters = (int(x) for x in g["meta"])
            assert iters == 100
            d = pair_to_data(synth.make_pair(n, seed), rad, pct, ms, device="cuda")
        datas.append(d)
    return datas


def _check_mixed(nm, g, d, o):
    compare_with_golden(o, d, g, float(g["match_threshold"]))
    if nm.startswith("dgims"):
        for s in ("0", "1"):
            src, dst = d["graph" + s][0].edges()
            np.testing.assert_array_equal(_multiset(src.cpu().numpy(), dst.cpu().numpy()), _multiset(g["out/dgl_src" + s], g["out/dgl_dst" + s]))


def test_match_pairs_with_per_pair_graphs():
    """One batch, three pairs, three graph settings (15/2/7, 25/7/8, Delaunay): every pair passes its own fixture's comparison."""
    gs = [load_golden(nm) for nm in MIXED]
    m = _model(settle=False)
    with pytest.raises(ValueError):
        m.match_pairs(_mixed_datas(gs))                          # still refused unless asked for by name
    datas = _mixed_datas(gs)
    outs = m.match_pairs(datas, per_pair_graph=True)
    assert len(outs) == 3
    for nm, g, d, o in zip(MIXED, gs, datas, outs):
        _check_mixed(nm, g, d, o)


def test_match_pairs_with_per_pair_graphs_on_two_stream_lanes():
    """streams=2: the batch twice over (a lane takes two pairs at least), every pair still its own fixture's."""
    gs = [load_golden(nm) for nm in MIXED]
    m = _model({"streams": 2}, settle=False)
    datas = _mixed_datas(gs) + _mixed_datas(gs)
    outs = m.match_pairs(datas, per_pair_graph=True)
    assert m.n_lanes_last == 2
    for i, (d, o) in enumerate(zip(datas, outs)):
        _check_mixed(MIXED[i % 3], gs[i % 3], d, o)


class _SyncCounter:
    """Counts what makes the host wait for the device: stream / device synchronisations, reads of a device tensor, and waits for an event
    that has not completed yet (the read-back of the attention statistics is consumed behind the build's synchronisation of the NEXT
    batch of its lane, through an event that has completed by then: no wait)."""

    def __init__(self, monkeypatch):
        self.n, self.where = 0, []
        for owner, name in ((torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize")):
            self._wrap(monkeypatch, owner, name, always=True)
        self._wrap(monkeypatch, torch.cuda.Event, "synchronize", always=False)
        for name in ("cpu", "item", "tolist", "numpy"):
            self._wrap(monkeypatch, torch.Tensor, name, always=False)

    def _wrap(self, monkeypatch, owner, name, always):
        orig = getattr(owner, name)

        def counted(*a, **k):
            if always or (a and torch.is_tensor(a[0]) and a[0].is_cuda) or (a and isinstance(a[0], torch.cuda.Event) and not a[0].query()):
                self.n += 1
                self.where.append(" < ".join(f"{f.name}:{f.lineno}" for f in reversed(traceback.extract_stack(limit=5)[:-1])))
            return orig(*a, **k)
        monkeypatch.setattr(owner, name, counted)


def _check_records(recs, settings, per, thr):
    assert len(recs) == len(settings)
    n_err = 0
    for rec, s in zip(recs, settings):
        assert (rec["radius"], rec["percentile"], rec["min_size"], rec["delaunay"]) == s + (False,)
        g = per[s]
        if "error_type" in g:
            assert rec["error"] == f"{g['error_type']}: {g['error_text']}", (s, rec["error"])
            assert rec["kept0"] == 0 and rec["kept1"] == 0 and rec["result"] is None and int(rec["n_matches"]) == 0
            n_err += 1
            continue
        assert rec["error"] is None, (s, rec["error"])
        res = rec["result"]
        compare_with_golden(res, res, g, thr)
        assert rec["kept0"] == len(g["out/kept0"]) and rec["kept1"] == len(g["out/kept1"])
        assert int(rec["n_matches"]) == int((g["out/matches0"] > -1).sum())
        assert res["keypoints0"].shape == (1, rec["kept0"], 2) and res["descriptors1"].shape[2] == rec["kept1"]
    return n_err


@pytest.mark.parametrize("prefix", list(STORED))
def test_sweep_over_the_stored_grid(prefix, monkeypatch):
    """Every stored setting passes compare_with_golden (1e-4); the settings the reference raised for come back as error records and leave
    the others alone; data is not mutated; one _ingest; one host synchronisation per sub-batch when no build had to be repeated."""
    pair, settings, per, _ = sweep_fixture(prefix)
    assert len(settings) == STORED[prefix]
    m = _model(CONFIG)
    data = pair_to_data(pair, 99, 99, 99, device="cuda")          # the dict's own triple plays no role in a sweep
    before = dict(data)
    copies = {k: v.clone() for k, v in data.items() if torch.is_tensor(v)}
    ingests, orig_ingest = [], m._ingest
    monkeypatch.setattr(m, "_ingest", lambda raw: (ingests.append(len(raw)), orig_ingest(raw))[1])
    n_rows = pair["keypoints0"].shape[1] + pair["keypoints1"].shape[1]
    rows = 16 * n_rows                                            # 16 settings per sub-batch: 2 sub-batches of 30, 3 of 48
    torch.cuda.synchronize()
    with monkeypatch.context() as mp:
        counter = _SyncCounter(mp)
        recs = m.sweep(data, settings, rows=rows)
        n_sync, where = counter.n, counter.where
    torch.cuda.synchronize()
    assert ingests == [2]
    st = m.sweep_stats_last
    assert st["ingests"] == 1 and st["sub_batches"] == math.ceil(len(settings) / 16)
    print(f"{prefix}: {len(settings)} settings, {st['sub_batches']} sub-batches, {n_sync} host synchronisations, {st['build_repeats']} repeated builds")
    if st["build_repeats"] == 0:
        assert n_sync == st["sub_batches"], where
    n_err = _check_records(recs, settings, per, CONFIG["match_threshold"])
    assert n_err == (4 if prefix.startswith("sweep_n1024sparse") else 0)
    assert set(data) == set(before) and all(data[k] is before[k] for k in data)
    for k, v in copies.items():
        assert torch.equal(data[k], v), k
    # dicts in the grid, the default sub-batch budget (one sub-batch here): the same records
    again = m.sweep(data, [dict(radius=r, percentile=t, min_size=ms) for r, t, ms in settings])
    assert m.sweep_stats_last["sub_batches"] == 1
    _check_records(again, settings, per, CONFIG["match_threshold"])


KEYS = ("matches0", "matches1", "matching_scores0", "matching_scores1")


def _one_and_many(prefix, config):
    """The stored grid of one pair through a single sub-batch and through at least three."""
    pair, settings, _, _ = sweep_fixture(prefix)
    m = _model(config)
    data = pair_to_data(pair, 25, 7, 8, device="cuda")
    n_rows = pair["keypoints0"].shape[1] + pair["keypoints1"].shape[1]
    one = m.sweep(data, settings, rows=len(settings) * n_rows)
    assert m.sweep_stats_last["sub_batches"] == 1
    many = m.sweep(data, settings, rows=(len(settings) // 3) * n_rows)
    assert m.sweep_stats_last["sub_batches"] >= 3
    for s, a, b in zip(settings, one, many):
        assert a["error"] == b["error"] and (a["kept0"], a["kept1"]) == (b["kept0"], b["kept1"]), s
    return [(s, a, b) for s, a, b in zip(settings, one, many) if a["error"] is None]


@pytest.mark.parametrize("prefix", list(STORED))
def test_sub_batch_size_does_not_change_the_results(prefix):
    """A budget that forces at least three sub-batches returns the same tensors as a single sub-batch, bit for bit -- with a FIXED attention
    precision, as in test_delaunay_gpu.py::test_alternating_modes_match_fresh_models: the graph build, the encoders, the split-bf16 attention,
    the GEMMs and both Sinkhorn plans (on-chip in one launch or in four, which the two runs differ in on the sparse pair) give the same bits
    whatever shares a launch with an entry."""
    for s, a, b in _one_and_many(prefix, dict(CONFIG, attention_precision="bf16x3")):
        assert int(a["n_matches"]) == int(b["n_matches"])
        for k in KEYS + ("keypoints0", "keypoints1", "descriptors0", "descriptors1", "mdesc0", "mdesc1"):
            assert torch.equal(a["result"][k], b["result"][k]), (s, k)
        for k in ("kept_kpts0_indices", "kept_kpts1_indices"):
            assert torch.equal(a["result"][k][0], b["result"][k][0]), (s, k)


@pytest.mark.parametrize("prefix", list(STORED))
def test_sub_batch_size_with_the_default_attention_precision(prefix):
    """With the default attention_precision='auto' (and with 'bf16' / 'f16') the SHAPE of a launch selects among the 16-bit attention kernel
    families (one sub-batch of 30 / 48 entries: the eight-wave kernel; ten or sixteen entries: the four-wave and split-key kernels), whose
    results differ in the last bits like a single pair's do from a batch's -- the case test_delaunay_gpu.py:201 and test_soak_gpu.py hold to
    5e-5.  So here: kept ids and every match index equal, scores within that 5e-5.  Measured on MI355X: every index equal, largest score
    difference 2.1e-5 (sparse pair) and 1.4e-5 (dense pair); the graph outputs (keypoints, descriptors, kept ids) are bit-identical."""
    worst = 0.0
    for s, a, b in _one_and_many(prefix, CONFIG):
        assert int(a["n_matches"]) == int(b["n_matches"])
        for k in KEYS[:2] + ("keypoints0", "keypoints1", "descriptors0", "descriptors1"):
            assert torch.equal(a["result"][k], b["result"][k]), (s, k)
        for k in ("kept_kpts0_indices", "kept_kpts1_indices"):
            assert torch.equal(a["result"][k][0], b["result"][k][0]), (s, k)
        for k in KEYS[2:]:
            worst = max(worst, (a["result"][k] - b["result"][k]).abs().max().item())
    print(f"{prefix}: largest score difference between one and three sub-batches {worst:.2e}")
    assert worst < 5e-5


@pytest.mark.parametrize("prefix", list(STORED))
def test_sweep_equals_forward_per_setting(prefix):
    """The same model, settled: indices equal, scores within 5e-5 (the bar the ragged tests hold a batch against a single pair to: a single
    pair is served by other attention kernels than a batch); where forward() raises, the sweep's record carries that exception."""
    pair, settings, _, _ = sweep_fixture(prefix)
    m = _model(CONFIG)
    recs = m.sweep(pair_to_data(pair, 25, 7, 8, device="cuda"), settings)
    for (r, t, ms), rec in zip(settings, recs):
        data = pair_to_data(pair, r, t, ms, device="cuda")
        try:
            ref = m(data)
        except ValueError as e:
            assert rec["error"] == f"ValueError: {e}", (r, t, ms)
            continue
        assert rec["error"] is None
        for s in ("0", "1"):
            assert rec["result"][f"kept_kpts{s}_indices"][0].tolist() == data[f"kept_kpts{s}_indices"][0], (r, t, ms)
        for k in KEYS[:2]:
            assert torch.equal(rec["result"][k], ref[k]), ((r, t, ms), k)
        for k in KEYS[2:]:
            assert (rec["result"][k] - ref[k]).abs().max().item() < 5e-5, ((r, t, ms), k)


def test_sweep_with_a_delaunay_entry_and_matches_only_outputs():
    """A grid may mix in delaunay=True; outputs='matches' leaves out keypoints / descriptors / mdesc and changes nothing else."""
    pair = synth.make_pair(512, 7001)
    m = _model(CONFIG)
    grid = [(15, 2, 7), dict(delaunay=True), (30, 10, 0)]
    full = m.sweep(pair_to_data(pair, 25, 7, 8, device="cuda"), grid)
    lean = m.sweep(pair_to_data(pair, 25, 7, 8, device="cuda"), grid, outputs="matches")
    assert [r["delaunay"] for r in full] == [False, True, False] and full[1]["kept0"] == full[1]["kept1"] == 512
    for a, b in zip(full, lean):
        assert set(b["result"]) == set(KEYS) | {"kept_kpts0_indices", "kept_kpts1_indices"}
        for k in KEYS:
            assert torch.equal(a["result"][k], b["result"][k]), k
    d = pair_to_data(pair, 25, 7, 8, device="cuda")
    d["delaunay"] = True
    ref = m(d)
    assert torch.equal(full[1]["result"]["matches0"], ref["matches0"])
    assert (full[1]["result"]["matching_scores0"] - ref["matching_scores0"]).abs().max().item() < 5e-5
