"""D-GIMS (delaunay=True) on the GPU: gims_delaunay_build against the reference's triangulations (tests/golden/dgims_tri*), the
matcher end to end against the reference network on the Delaunay graphs (dgims_e2e_*), match_pairs, degenerate inputs checked for
validity in exact arithmetic, ignored parameters, and isolation from the default (adaptive graph) path."""
import numpy as np
import pytest
import torch

from gims_amd import GMatcher, Matching, hip, synth
from tests import dgims_helpers as H
from tests.helpers import compare_with_golden, golden_names, load_golden, pair_to_data

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def dt_build(xys, cap_per_node=16):
    """gims_delaunay_build on a batch of point sets -> per image (indptr, indices, info, kept) as NumPy arrays."""
    dev = torch.device("cuda")
    info = torch.zeros((len(xys), 8), dtype=torch.int32, device=dev)
    items = []
    for i, xy in enumerate(xys):
        n = len(xy)
        items.append(dict(kpts=torch.from_numpy(np.ascontiguousarray(xy, dtype=np.float32)).to(dev), desc=None,
                          kept=torch.empty(n, dtype=torch.int32, device=dev), indptr=torch.empty(n + 1, dtype=torch.int32, device=dev),
                          indices=torch.full((cap_per_node * n + 1,), -7, dtype=torch.int32, device=dev), info=info[i]))
    arr = hip.make_agc_images(items)
    work = torch.empty(hip.delaunay_workspace_bytes(arr), dtype=torch.uint8, device=dev)
    hip.delaunay_build(arr, work)
    torch.cuda.synchronize()
    out = []
    for it in items:
        inf = it["info"].cpu().numpy()
        ip = it["indptr"].cpu().numpy()
        out.append(dict(indptr=ip, indices=it["indices"].cpu().numpy()[:ip[-1]], info=inf, kept=it["kept"].cpu().numpy()))
    return out


def edges_and_checks(xy, r):
    """Undirected edges of one build, after the structural checks every build must pass (symmetric, sorted, no flags)."""
    n = len(xy)
    assert r["info"][7] == 0, f"flags {r['info'][7]}"
    np.testing.assert_array_equal(r["kept"], np.arange(n))
    assert r["info"][0] == n and r["info"][1] == r["indptr"][-1] and r["info"][2] * 2 == r["info"][1]
    src, dst = H.csr_edges(r["indptr"], r["indices"])
    d = set(zip(src.tolist(), dst.tolist()))
    assert all((v, u) in d for u, v in d), "adjacency not symmetric"
    for u in range(n):
        seg = r["indices"][r["indptr"][u]:r["indptr"][u + 1]]
        assert (np.diff(seg) > 0).all()
    return H.canon_edges(np.stack([src, dst], axis=1))


def check_valid(xy, r):
    """Validity in exact arithmetic + the edge-count formula + duplicates isolated; returns the edges."""
    e = edges_and_checks(xy, r)
    st = H.check_delaunay(xy, e)
    assert r["info"][1] == 2 * (3 * st["n_distinct"] - 3 - st["hull"])
    assert r["info"][3] == len(xy) - st["n_distinct"]
    rep = H.lowest_id_map(xy)
    deg = np.diff(r["indptr"])
    assert (deg[rep != np.arange(len(xy))] == 0).all(), "a non-lowest duplicate has neighbours"
    return e


def tri_inputs():
    out = []
    for name in golden_names("dgims_tri_"):
        g = load_golden(name)
        n, seed = (int(v) for v in g["meta"])
        out.append((name, H.fixture_points(str(g["kind"]), n, seed), g["edges"].astype(np.int64)))
    g = load_golden("dgims_tripair_n15382_14870_s4003")
    n0, n1, c, seed = (int(v) for v in g["meta"])
    pair = synth.make_pair_unbalanced(n0, n1, c, seed)
    for s in ("0", "1"):
        out.append((f"readme{s}", pair["keypoints" + s][0], g["edges" + s].astype(np.int64)))
    return out


def test_triangulation_parity_with_the_reference():
    """Every triangulation fixture: the device edge set equals the reference's (Qhull's), duplicate endpoints mapped to the lowest id of
    their group; symmetric CSR; n_dir_edges = 2 (3 n' - 3 - h); the whole batch in one call equals image-by-image calls; a repeat is
    bit-identical."""
    ins = tri_inputs()
    batch = dt_build([xy for _, xy, _ in ins])
    again = dt_build([xy for _, xy, _ in ins])
    for (name, xy, ref), r, r2 in zip(ins, batch, again):
        rep = H.lowest_id_map(xy)
        e = check_valid(xy, r)
        np.testing.assert_array_equal(e, H.canon_edges(rep[ref]), err_msg=name)
        for k in ("indptr", "indices", "info"):
            np.testing.assert_array_equal(r[k], r2[k])
        print(f"{name}: n={len(xy)} edges={r['info'][2]} duplicates={r['info'][3]} hull={r['info'][4]} exact_fallbacks={r['info'][5]}")
    for (name, xy, _), r in zip(ins[:3], batch[:3]):
        single = dt_build([xy])[0]
        for k in ("indptr", "indices", "info"):
            np.testing.assert_array_equal(single[k], r[k])


def _wheel(m=2000):
    t = np.arange(m) * (2 * np.pi / m)
    rim = np.stack([300 + 200 * np.cos(t), 300 + 200 * np.sin(t)], axis=1).astype(np.float32)
    return np.concatenate([np.asarray([[300, 300]], dtype=np.float32), rim])


def degenerate_cases():
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16)), axis=-1).reshape(-1, 2).astype(np.float32)
    rng = np.random.default_rng(3)
    hull_line = np.concatenate([np.stack([np.arange(20), np.zeros(20)], axis=1), np.stack([np.zeros(10), np.arange(1, 11)], axis=1),
                                rng.uniform(0.5, 6, (40, 2))]).astype(np.float32)
    dups = np.concatenate([np.tile([[5.0, 5.0]], (30, 1)), [[1.0, 2.0], [9.0, 1.5]], np.tile([[1.0, 2.0]], (5, 1))]).astype(np.float32)
    return {"grid16": g, "wheel2000": _wheel(), "collinear_hull": hull_line, "all_duplicates_but_three": dups,
            "grid16_shuffled": g[rng.permutation(len(g))]}


@pytest.mark.parametrize("case", list(degenerate_cases()))
def test_degenerate_inputs_are_valid_and_deterministic(case):
    xy = degenerate_cases()[case]
    r = dt_build([xy])[0]
    check_valid(xy, r)
    r2 = dt_build([xy])[0]
    for k in ("indptr", "indices", "info"):
        np.testing.assert_array_equal(r[k], r2[k])
    if case == "wheel2000":
        assert r["indptr"][1] - r["indptr"][0] == len(xy) - 1          # the centre is adjacent to every rim point
    print(f"{case}: exact_fallbacks={r['info'][5]}")


@pytest.mark.parametrize("xy", [np.asarray([[0, 0], [1, 1], [2, 2], [5, 5]], np.float32), np.asarray([[1, 1], [1, 1], [3, 2]], np.float32),
                                np.asarray([[4, 4], [4, 4]], np.float32)], ids=["collinear", "two_distinct", "one_distinct"])
def test_degenerate_build_is_flagged(xy):
    r = dt_build([xy, H.uniform_points(64, 1)])
    assert r[0]["info"][7] & hip.DT_INFO_DEGENERATE
    assert r[1]["info"][7] == 0                     # the other image of the batch is unaffected


def _dgims_model(wseed, iters, settle=False, **cfg):
    cfg.update({} if iters == 100 else {"sinkhorn_iterations": 20, "match_threshold": 0.02})
    m = GMatcher(cfg).eval()
    m.load_state_dict(synth.make_state_dict(wseed))
    if settle:
        # attention_precision='auto': the first call after the weights change measures every layer and decides; tests that
        # compare calls with each other start from the settled state
        m(pair_to_data(synth.make_pair(256, 1002), 15, 2, 7, device="cuda"))
    return m


def _data(pair, radius=15, percentile=2, min_size=7):
    d = pair_to_data(pair, radius, percentile, min_size, device="cuda")
    d["delaunay"] = True
    return d


def _graph_multiset(g):
    src, dst = g.edges()
    e = np.stack([src.cpu().numpy(), dst.cpu().numpy()], axis=1).astype(np.int64)
    return e[np.lexsort((e[:, 1], e[:, 0]))]


def _golden_multiset(g, s):
    e = np.stack([g["out/dgl_src" + s], g["out/dgl_dst" + s]], axis=1).astype(np.int64)
    return e[np.lexsort((e[:, 1], e[:, 0]))]


@pytest.mark.parametrize("name", golden_names("dgims_e2e_"))
def test_end_to_end_parity(name):
    """GMatcher.forward with delaunay=True against the reference network on the reference's Delaunay graphs: kept ids, every match index,
    scores within 1e-4, the graph0 / graph1 edge multisets.  The Matching shell forwards data['delaunay'] unchanged: same bits."""
    g = load_golden(name)
    seed, wseed, iters = (int(v) for v in g["meta"][:3])
    pair = H.e2e_pair(g["meta"])
    m = _dgims_model(wseed, iters)
    data = _data(pair)
    out = m(data)
    compare_with_golden(out, data, g, float(g["match_threshold"]))
    for s in ("0", "1"):
        np.testing.assert_array_equal(data["kept_kpts%s_indices" % s][0], np.arange(len(pair["keypoints" + s][0])))
        np.testing.assert_array_equal(_graph_multiset(data["graph" + s][0]), _golden_multiset(g, s))
    mm = Matching({} if iters == 100 else {"sinkhorn_iterations": 20, "match_threshold": 0.02}).eval()
    mm.gmodel.load_state_dict(synth.make_state_dict(wseed))
    shell = mm(_data(pair))
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
        assert torch.equal(shell[k], out[k]), k


def test_match_pairs_ragged_equals_fixtures_and_forward():
    names = golden_names("dgims_e2e_")
    gs = {nm: load_golden(nm) for nm in names}
    sel = [nm for nm in names if int(gs[nm]["meta"][1]) == 123 and int(gs[nm]["meta"][2]) == 100]
    assert len(sel) >= 2
    m = _dgims_model(123, 100)
    datas = [_data(H.e2e_pair(gs[nm]["meta"])) for nm in sel]
    outs = m.match_pairs(datas)
    for nm, d, o in zip(sel, datas, outs):
        compare_with_golden(o, d, gs[nm], float(gs[nm]["match_threshold"]))
        # the same pair alone through forward(): the same matches; scores to 5e-5, the bar tests/test_soak_gpu.py holds the default path to
        # (a single pair is served by other attention kernels than a batch)
        ref = m(_data(H.e2e_pair(gs[nm]["meta"])))
        for k in ("matches0", "matches1"):
            assert torch.equal(o[k], ref[k]), (nm, k)
        for k in ("matching_scores0", "matching_scores1"):
            assert (o[k] - ref[k]).abs().max().item() < 5e-5, (nm, k)
    mixed = [_data(H.e2e_pair(gs[sel[0]]["meta"])), pair_to_data(H.e2e_pair(gs[sel[1]]["meta"]), 15, 2, 7, device="cuda")]
    with pytest.raises(ValueError, match="delaunay"):
        m.match_pairs(mixed)


def test_forward_raises_on_a_degenerate_image():
    pair = synth.make_pair(64, 11)
    pair["keypoints1"] = pair["keypoints1"].copy()
    pair["keypoints1"][0][:, 1] = pair["keypoints1"][0][:, 0] * 2          # all on one line
    m = _dgims_model(123, 100)
    with pytest.raises(ValueError, match="image 1"):
        m(_data(pair))


def test_ignored_parameters_give_identical_bits():
    pair = synth.make_pair(512, 77)
    m = _dgims_model(123, 100, settle=True)
    outs = [m(_data(pair, r, p, s)) for r, p, s in ((15, 2, 7), (25, 7, 8), (3, 90, 100))]
    for o in outs[1:]:
        for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "mdesc0"):
            assert torch.equal(o[k], outs[0][k]), k


def test_alternating_modes_match_fresh_models():
    """GIMS and D-GIMS calls alternating on one model give the bits of fresh single-mode models (edge capacity, encoder cache and attention
    launch tables are not disturbed by the other mode; a fixed attention precision, so that no measured statistic carries over by design);
    mode='train' with delaunay still raises."""
    pairs = [synth.make_pair(1024, 91), synth.make_pair(512, 92)]

    def run(m, pair, dl):
        d = pair_to_data(pair, 15, 2, 7, device="cuda")
        if dl:
            d["delaunay"] = True
        o = m(d)
        return {k: o[k].clone() for k in ("matches0", "matches1", "matching_scores0", "matching_scores1")}
    fresh = {}
    for dl in (False, True):
        m = _dgims_model(123, 100, settle=True, attention_precision="bf16x3")
        fresh[dl] = [run(m, p, dl) for p in pairs for _ in range(2)]
    m = _dgims_model(123, 100, settle=True, attention_precision="bf16x3")
    alt = {False: [], True: []}
    for p in pairs:
        for _ in range(2):
            for dl in (False, True):
                alt[dl].append(run(m, p, dl))
    for dl in (False, True):
        for a, b in zip(alt[dl], fresh[dl]):
            for k in a:
                assert torch.equal(a[k], b[k]), (dl, k)
    with pytest.raises(NotImplementedError, match="D-GIMS"):
        m(_data(pairs[1]), mode="train")
