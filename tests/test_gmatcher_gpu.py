"""End-to-end parity of the drop-in GMatcher (HIP path) against golden vectors produced by the reference
itself and against the CPU oracle.  Bars (BASELINE.json north_star): match indices bit-exact, f32 scores
within 1e-4.  Indices are compared wherever the reference's own decision is well-conditioned (top-1/top-2
gap of the OT row > 1e-3 and |score - threshold| > 1e-3, both recorded in the fixture); the number of
ill-conditioned rows is asserted to be small so the comparison cannot be vacuous."""
import numpy as np
import pytest
import torch

from gims_amd import GMatcher, Matching, synth
from oracle import gims_oracle as O
from tests.helpers import compare_with_golden as _compare, alpha_pair, check_score_gradients, fixture_state_dict, golden_names, make_rare_pair, load_golden, pair_to_data, safe_rows, train_data, train_pairs

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def models(synth_sd):
    out = {}
    for prec in ("bf16x3", "f32", "bf16x3-unfused"):
        for iters, thr in ((100, 0.2), (20, 0.02)):
            m = GMatcher({"sinkhorn_iterations": iters, "match_threshold": thr, "linear_precision": prec.split("-")[0],
                          "fuse_merge": not prec.endswith("unfused")}).eval()
            m.load_state_dict(synth_sd)
            _settle(m)
            out[(prec, iters)] = m
    return out


def _settle(m):
    """attention_precision='auto' (the default): the first call after the weights change measures every layer at bf16x3 and
    decides; tests that compare calls with each other start from the settled state."""
    m(pair_to_data(synth.make_pair(256, 1002), 15, 2, 7, device="cuda"))
    assert m.attention_report() is None or m.attention_report()["calibrated"]


@pytest.mark.parametrize("sinkhorn", ["streamed", "resident"])     # both Sinkhorn implementations against the reference
@pytest.mark.parametrize("prec", ["bf16x3", "f32", "bf16x3-unfused"])
@pytest.mark.parametrize("name", golden_names("e2e_"))
def test_e2e_vs_reference_golden(models, monkeypatch, name, prec, sinkhorn):
    monkeypatch.setenv("GIMS_OT_RESIDENT", "0" if sinkhorn == "streamed" else "2")
    g = load_golden(name)
    n, seed, rad, pct, ms, iters = [int(x) for x in g["meta"]]
    pair = synth.make_pair(n, seed)
    data = pair_to_data(pair, rad, pct, ms, device="cuda")
    out = models[(prec, iters)](data)
    stats = _compare(out, data, g, float(g["match_threshold"]))
    print(name, prec, sinkhorn, stats)
    # mutated dict, like the reference (gmatcher.py:244-252)
    nk0 = len(g["out/kept0"])
    assert data["keypoints0"].shape == (1, nk0, 2) and data["descriptors0"].shape == (1, 256, nk0)
    assert data["scores0"].shape == (1, nk0) and len(data["graph0"]) == 1
    np.testing.assert_array_equal(data["keypoints0"][0].cpu().numpy(), pair["keypoints0"][0][g["out/kept0"]])
    src, dst = data["graph1"][0].edges()
    a = np.stack([src.cpu().numpy(), dst.cpu().numpy()], 1)
    b = np.stack([g["out/dgl_src1"], g["out/dgl_dst1"]], 1)
    np.testing.assert_array_equal(a[np.lexsort((a[:, 1], a[:, 0]))], b[np.lexsort((b[:, 1], b[:, 0]))])


_ALPHA_MODELS = {}


def _alpha_model(g, prec="bf16x3"):
    """A settled GMatcher with the weights of a tools/gen_golden_alpha.py fixture (its weight seed and bin_score), one per setting."""
    rad, pct, ms, iters = [int(x) for x in g["meta"]]
    key = (int(g["weight_seed"]), float(g["bin_score"]), iters, float(g["match_threshold"]), prec)
    if key not in _ALPHA_MODELS:
        m = GMatcher({"sinkhorn_iterations": iters, "match_threshold": float(g["match_threshold"]), "linear_precision": prec}).eval()
        m.load_state_dict(fixture_state_dict(g))
        _settle(m)
        _ALPHA_MODELS[key] = m
    return _ALPHA_MODELS[key]


@pytest.mark.parametrize("sinkhorn", ["streamed", "resident"])
@pytest.mark.parametrize("name", golden_names("bine2e_") + golden_names("seede2e_"))
def test_e2e_alpha_and_weight_seeds_vs_reference_golden(monkeypatch, name, sinkhorn):
    """forward() against the reference at dustbin logits that compete with the scores (bine2e_*: -2, p10 / p50 / p90 of the pair's row
    maxima, above every score -- nothing matched) and with two more weight seeds at bin_score = 1 (seede2e_*), on both Sinkhorn paths, at
    compare_with_golden's bars.  Every other e2e fixture sits at bin_score = 1, far below the row maxima (~45-95)."""
    monkeypatch.setenv("GIMS_OT_RESIDENT", "0" if sinkhorn == "streamed" else "2")
    g = load_golden(name)
    rad, pct, ms, _ = [int(x) for x in g["meta"]]
    data = pair_to_data(alpha_pair(g), rad, pct, ms, device="cuda")
    # bin_score inside the row-max range (p10 / p50 / p90): a matched row's score exp(log P) = s is no longer saturated by a far dustbin, it
    # moves by s (1 - s) per unit of score error; the default precision's score matrix (bf16x3 linears) then gives 1.1e-4 ... 1.9e-4
    # (measured on both Sinkhorn paths, indices all exact), f32 linears stay within 1e-4 (next test).  Elsewhere: the 1e-4 bar.
    tol = 2.5e-4 if name.endswith(("_ap10", "_ap50", "_ap90")) else 1e-4
    out = _alpha_model(g)(data)
    print(name, float(g["bin_score"]), sinkhorn, _compare(out, data, g, float(g["match_threshold"]), score_tol=tol))


@pytest.mark.parametrize("sinkhorn", ["streamed", "resident"])
@pytest.mark.parametrize("name", [n for n in golden_names("bine2e_") if n.endswith(("_ap10", "_ap50", "_ap90"))])
def test_e2e_alpha_f32_linears_vs_reference_golden(monkeypatch, name, sinkhorn):
    """linear_precision='f32' at every bin_score inside the row-max range, at the 1e-4 bar."""
    monkeypatch.setenv("GIMS_OT_RESIDENT", "0" if sinkhorn == "streamed" else "2")
    g = load_golden(name)
    rad, pct, ms, _ = [int(x) for x in g["meta"]]
    data = pair_to_data(alpha_pair(g), rad, pct, ms, device="cuda")
    out = _alpha_model(g, "f32")(data)
    print(name, float(g["bin_score"]), sinkhorn, _compare(out, data, g, float(g["match_threshold"])))


def test_match_pairs_alpha_batch_vs_reference_golden():
    """match_pairs on one ragged batch of the bine2e_* fixtures that share bin_score = -2 and the (100, 0.2) setting (256 x 252 and
    1498 x 896 kept keypoints), each pair against its own fixture."""
    names = [n for n in golden_names("bine2e_") if n.endswith("_i100_am2")]
    assert len(names) == 2
    gs = [load_golden(n) for n in names]
    assert len({(float(g["bin_score"]), int(g["meta"][3])) for g in gs}) == 1
    datas = [pair_to_data(alpha_pair(g), *[int(x) for x in g["meta"][:3]], device="cuda") for g in gs]
    outs = _alpha_model(gs[0]).match_pairs(datas)
    for n, g, d, o in zip(names, gs, datas, outs):
        print(n, _compare(o, d, g, float(g["match_threshold"])))


def _unbalanced(name):
    g = load_golden(name)
    n0, n1, nc, seed, rad, pct, ms, iters = [int(x) for x in g["meta"]]
    return g, synth.make_pair_unbalanced(n0, n1, nc, seed), (rad, pct, ms), iters


@pytest.mark.parametrize("sinkhorn", ["streamed", "resident"])
@pytest.mark.parametrize("prec", ["bf16x3", "f32", "bf16x3-unfused"])
@pytest.mark.parametrize("name", [n for n in golden_names("ube2e_") if "n15382" not in n])
def test_e2e_unbalanced_vs_reference_golden(models, monkeypatch, name, prec, sinkhorn):
    """UNBALANCED pairs through forward() against the reference (every e2e_* fixture is an n = m permutation pair): n0 != n1, image 1 =
    partners of a subset of image 0's keypoints + fresh outliers, so rows AND columns end in the dustbin and the kept counts differ
    (1498 / 896 and 300 / 520).  Kept ids, DGL edges, indices exact; scores within 1e-4."""
    monkeypatch.setenv("GIMS_OT_RESIDENT", "0" if sinkhorn == "streamed" else "2")
    g, pair, (rad, pct, ms), iters = _unbalanced(name)
    data = pair_to_data(pair, rad, pct, ms, device="cuda")
    out = models[(prec, iters)](data)
    print(name, prec, sinkhorn, _compare(out, data, g, float(g["match_threshold"])))
    assert out["matches0"].shape[1] == len(g["out/kept0"]) != out["matches1"].shape[1] == len(g["out/kept1"])
    for s in ("0", "1"):
        src, dst = data["graph" + s][0].edges()
        a = np.stack([src.cpu().numpy(), dst.cpu().numpy()], 1)
        b = np.stack([g["out/dgl_src" + s], g["out/dgl_dst" + s]], 1)
        np.testing.assert_array_equal(a[np.lexsort((a[:, 1], a[:, 0]))], b[np.lexsort((b[:, 1], b[:, 0]))])


@pytest.mark.parametrize("name", [n for n in golden_names("ube2e_") if "n15382" in n])
def test_e2e_readme_configuration_vs_reference_golden(models, name):
    """The reference's one PUBLISHED hot-path configuration (README.md:143-163: 15 382 / 14 870 keypoints, N != M, eval setting: 20 Sinkhorn
    iterations, threshold 0.02), on a density-matched synthetic pair of exactly those sizes; the golden is the reference run on this pair
    (tools/gen_golden_large.py --only readme).  Default precision tiers, streamed Sinkhorn (the on-chip kernel holds up to 2 x 4096 x 4096)."""
    g, pair, (rad, pct, ms), iters = _unbalanced(name)
    data = pair_to_data(pair, rad, pct, ms, device="cuda")
    out = models[("bf16x3", iters)](data)
    print(name, _compare(out, data, g, float(g["match_threshold"])))
    for s in ("0", "1"):
        src, dst = data["graph" + s][0].edges()
        a = np.stack([src.cpu().numpy(), dst.cpu().numpy()], 1)
        b = np.stack([g["out/dgl_src" + s], g["out/dgl_dst" + s]], 1)
        np.testing.assert_array_equal(a[np.lexsort((a[:, 1], a[:, 0]))], b[np.lexsort((b[:, 1], b[:, 0]))])


def test_forward_above_16384_keypoints(models):
    """A pair above the former 16 384-keypoint cap through forward() (21 163 / 18 555: the two largest kept counts the reference publishes,
    tools/files/rgbd1/record.txt:635, scannet/record.txt:633; 16 000 keypoints in common).  Too large for a reference golden in the build
    container's memory budget for attention (4 x 21 163^2 floats per layer), so size-independent properties: the planted correspondences are
    recovered, matches0 / matches1 are mutually consistent, scores lie in (threshold, 1], the graph handles are consistent with the kept ids."""
    n0, n1, nc = 21163, 18555, 16000
    pair = synth.make_pair_unbalanced(n0, n1, nc, 3100)
    data = pair_to_data(pair, 15, 2, 7, device="cuda")
    out = models[("bf16x3", 20)](data)
    k0, k1 = np.asarray(data["kept_kpts0_indices"][0]), np.asarray(data["kept_kpts1_indices"][0])
    assert len(k0) > 0.95 * n0 and len(k1) > 0.9 * n1 and (np.diff(k0) > 0).all() and (np.diff(k1) > 0).all()
    m0, m1 = out["matches0"][0].cpu().numpy(), out["matches1"][0].cpu().numpy()
    s0 = out["matching_scores0"][0].cpu().numpy()
    assert m0.shape == (len(k0),) and m1.shape == (len(k1),)
    v = m0 >= 0
    assert (m1[m0[v]] == np.nonzero(v)[0]).all() and (m0[m1[m1 >= 0]] == np.nonzero(m1 >= 0)[0]).all()      # mutual
    assert (s0[v] > 0.02).all() and (s0[v] <= 1.0 + 1e-6).all() and (s0[~v] <= 0.02).all()      # (a mutual pair under the threshold keeps its score, gmatcher.py:290-292)
    gt = pair["gt_perm"]
    correct = int((k1[m0[v]] == gt[k0[v]]).sum())
    # (at the eval threshold 0.02 some of the 5 163 + 2 555 unpartnered keypoints pair up with each other at low scores: the planted ones are what counts)
    assert correct > 0.95 * nc and correct > 0.9 * v.sum(), (int(v.sum()), correct)
    for s, k in (("0", k0), ("1", k1)):
        g = data["graph" + s][0]
        assert g.num_nodes() == len(k) and g.num_edges() % 2 == 0


@pytest.mark.parametrize("sinkhorn", ["streamed", "resident"])
@pytest.mark.parametrize("tier", ["auto", "f16", "bf16x3"])
@pytest.mark.parametrize("name", golden_names("sharpe2e_") + golden_names("peakede2e_"))
def test_e2e_sharp_attention_vs_reference_golden(monkeypatch, name, sinkhorn, tier):
    """Trained-like, PEAKED attention (query / key projections of every layer scaled up: mean row maximum of the softmax
    0.21 for the 'sharp' fixtures and 0.76 for the 'peaked' ones, against 0.007 with the default synthetic weights).  The
    reference produced the goldens with the same weights; bars as everywhere: indices exact, scores within 1e-4.
    tier 'auto': the model is built WITHOUT naming an attention precision -- the default measures the peakedness itself (first
    call: every layer on the split-bf16 kernels) and routes the layers that need it to the IEEE-half kernels (plain bf16 attention
    is at 3.1e-4 on the 'peaked' fixtures); both the measuring first call and the settled second call are held to the bars.
    tiers 'f16' / 'bf16x3': every layer on that kernel family from the first call on."""
    monkeypatch.setenv("GIMS_OT_RESIDENT", "0" if sinkhorn == "streamed" else "2")
    g = load_golden(name)
    n, seed, rad, pct, ms, iters = [int(x) for x in g["meta"]]
    gq = float(g["gain_qk"])
    cfg = {"sinkhorn_iterations": iters, "match_threshold": float(g["match_threshold"])}
    if tier != "auto":
        cfg["attention_precision"] = tier
    m = GMatcher(cfg).eval()
    assert m.config["attention_precision"] == tier
    m.load_state_dict(synth.make_state_dict(123, gains={"attn.proj.0": gq, "attn.proj.1": gq}))
    for call in ("measuring", "settled"):
        data = pair_to_data(synth.make_pair(n, seed), rad, pct, ms, device="cuda")
        out = m(data)
        stats = _compare(out, data, g, float(g["match_threshold"]))
        rep = m.attention_report()
        if rep is not None:
            print(name, sinkhorn, call, stats, "modes:", {k: rep["modes"].count(k) for k in ("bf16", "f16", "bf16x3")}, "peak per layer:",
                  np.round(rep["peak"].max(1), 3), "range:", np.round(rep["range"].max(), 1))
        else:
            print(name, sinkhorn, tier, call, stats)
    if tier == "auto":
        assert rep["calibrated"]
        assert rep["modes"].count("bf16x3") == 0, rep["modes"]               # operands far inside half's range: nothing needs the 3-pass kernels
        if name.startswith("peaked"):
            assert rep["modes"].count("f16") >= 12, rep["modes"]             # mean row maximum 0.76: (nearly) every layer is over the threshold


@pytest.mark.parametrize("sinkhorn", ["streamed", "resident"])
@pytest.mark.parametrize("name", golden_names("mixede2e_") + golden_names("headsharpe2e_"))
def test_e2e_mixed_regimes_vs_reference_golden(monkeypatch, name, sinkhorn):
    """attention_precision='auto' holding a MIXED launch table against the reference (the state 'auto' exists for was
    only ever checked for self-consistency).  'mixed': the query / key gains differ per layer -- layers 0-5 diffuse (mean row maximum
    0.002), 6-11 sharp (0.1 - 0.46), 12-17 peaked (0.7 - 0.92); 'headsharp': ONE head (head 2) of layers 4-9 sharpened (layers 7-9:
    mean 0.63 - 0.88 in that head, 0.002 in the other three), everything else diffuse.  Goldens from the reference with the same
    weights (tools/gen_golden_large.py --only mixed).  Asserted: the decided modes really are mixed (bf16 and half layers in one
    pass), and the measuring and the settled call both hold the bars.  A second model with the half range limit placed between the
    measured operand ranges of the sharp and of the peaked layers holds all THREE families in one table."""
    monkeypatch.setenv("GIMS_OT_RESIDENT", "0" if sinkhorn == "streamed" else "2")
    g = load_golden(name)
    n, seed, rad, pct, ms, iters = [int(x) for x in g["meta"]]
    if name.startswith("mixed"):
        gains = {}
        for l, gl in enumerate([0.3] * 6 + [1.0] * 6 + [2.0] * 6):
            gains[f"layers.{l}.attn.proj.0"] = gl
            gains[f"layers.{l}.attn.proj.1"] = gl
        sd = synth.make_state_dict(123, gains=gains)
    else:
        sd = synth.make_state_dict(123, head_gains={**{(l, 2): 3.0 for l in range(4, 7)}, **{(l, 2): 6.0 for l in range(7, 10)}})
    cfg = {"sinkhorn_iterations": iters, "match_threshold": float(g["match_threshold"])}
    m = GMatcher(cfg).eval()
    m.load_state_dict(sd)
    for call in ("measuring", "settled", "settled again"):
        data = pair_to_data(synth.make_pair(n, seed), rad, pct, ms, device="cuda")
        out = m(data)
        stats = _compare(out, data, g, float(g["match_threshold"]))
        rep = m.attention_report()
        print(name, sinkhorn, call, stats, "modes:", rep["modes"], "peak:", np.round(rep["peak"].max(1), 3), "tail:", np.round(rep["tail"].max(1), 3),
              "range:", np.round(rep["range"].max(1), 1))
    modes = rep["modes"]
    assert rep["calibrated"] and "bf16x3" not in modes
    if name.startswith("mixed"):
        assert modes[:6] == ["bf16"] * 6 and modes[12:] == ["f16"] * 6 and modes[6:12].count("f16") >= 4, modes
    else:
        assert modes[:4] == ["bf16"] * 4 and modes[10:] == ["bf16"] * 8 and modes[7:10] == ["f16"] * 3, modes
        assert (rep["peak"][7:10, [0, 1, 3]] < 0.02).all() and (rep["peak"][7:10, 2] > 0.4).all()      # ONE head carries the decision
    if name.startswith("mixed"):
        # three families in one table: the range limit between the sharp layers' operands and the peaked layers'
        lo, hi = float(rep["range"][6:12].max()), float(rep["range"][12:].max())
        assert hi > 1.2 * lo, (lo, hi)
        m3 = GMatcher({**cfg, "attention_f16_range": float(np.sqrt(lo * hi))}).eval()
        m3.load_state_dict(sd)
        for call in ("measuring", "settled"):
            data = pair_to_data(synth.make_pair(n, seed), rad, pct, ms, device="cuda")
            _compare(m3(data), data, g, float(g["match_threshold"]))
        modes3 = m3.attention_report()["modes"]
        assert {"bf16", "f16", "bf16x3"} <= set(modes3) and modes3[:6] == ["bf16"] * 6, modes3


def test_auto_attention_settles_on_bf16_and_switches_when_a_layer_sharpens(synth_sd):
    """attention_precision='auto' with the default synthetic weights (mean row maximum 0.007): the first call measures at
    bf16x3, every later call runs the plain bf16 kernels and still agrees with the measuring call within the score bar; the bf16
    layers keep being measured -- lowering the threshold under their statistic moves them up to the half kernels on the next call."""
    m = GMatcher({"attention_monitor_period": 1}).eval()       # (measure every call, so that the test does not have to count them)
    m.load_state_dict(synth_sd)
    mk = lambda: pair_to_data(synth.make_pair(1024, 1003), 15, 2, 7, device="cuda")      # noqa: E731
    o1 = m(mk())
    rep = m.attention_report()
    assert rep["calibrated"] and rep["modes"] == ["bf16"] * 18, rep
    assert 0 < rep["peak"].max() < 0.05
    o2 = m(mk())
    np.testing.assert_array_equal(o1["matches0"].cpu().numpy(), o2["matches0"].cpu().numpy())
    assert np.abs(o1["matching_scores0"].cpu().numpy() - o2["matching_scores0"].cpu().numpy()).max() < 5e-5
    rep2 = m.attention_report()                    # the settled call reported too (split-key / sampled 8-wave kernels)
    assert (rep2["peak"] > 0).all() and np.abs(rep2["peak"] - rep["peak"]).max() < 0.2 * rep["peak"].max()
    m.config["attention_auto_threshold"] = 0.5 * float(rep2["peak"].max(1).min())
    m(mk())                                        # measured over the (new) threshold on this call ...
    rep3 = m.attention_report()
    assert rep3["modes"] == ["f16"] * 18 and sorted(rep3["switched"]) == list(range(18))
    o4 = m(mk())                                   # ... so this one runs on the half kernels
    np.testing.assert_array_equal(o1["matches0"].cpu().numpy(), o4["matches0"].cpu().numpy())
    np.testing.assert_allclose(o1["matching_scores0"].cpu().numpy(), o4["matching_scores0"].cpu().numpy(), atol=2e-5)
    # match_pairs (ragged batch, 8-wave kernels on sampled workgroups) settles the same way
    m2 = GMatcher({"attention_monitor_period": 1}).eval()
    m2.load_state_dict(synth_sd)
    batch = lambda: [pair_to_data(synth.make_pair(1024, 1000 + i), 15, 2, 7, device="cuda") for i in range(8)]      # noqa: E731
    m2.match_pairs(batch())
    r1 = m2.match_pairs(batch())
    torch.cuda.synchronize()
    repb = m2.attention_report()
    assert repb["calibrated"] and repb["modes"] == ["bf16"] * 18
    m2.match_pairs(batch())
    torch.cuda.synchronize()
    repc = m2.attention_report()
    # (the settled batch is measured by the sampling kernel: 32 queries per problem and head instead of all of them)
    assert (repc["peak"] > 0).all() and np.abs(repc["peak"] - repb["peak"]).max() < 0.5 * repb["peak"].max()
    m3 = GMatcher({"attention_precision": "bf16"}).eval()
    m3.load_state_dict(synth_sd)
    r3 = m3.match_pairs(batch())
    for a, b in zip(r1, r3):
        np.testing.assert_array_equal(a["matches0"].cpu().numpy(), b["matches0"].cpu().numpy())
        assert np.abs(a["matching_scores0"].cpu().numpy() - b["matching_scores0"].cpu().numpy()).max() < 5e-5


# fixtures of fewer than 512 keypoints per image: matched inside chip-filling batches by
# test_rare_peaked_rows_of_small_pairs_in_chip_filling_batches_vs_reference_golden (what they were generated for)
SMALL_RARE = [n for n in golden_names("raree2e_") if int(load_golden(n)["meta"][0]) < 512]


@pytest.mark.parametrize("api", ["forward", "match_pairs", "batch8_on_the_8wave_kernel"])
@pytest.mark.parametrize("name", [n for n in golden_names("raree2e_") if n not in SMALL_RARE])
def test_rare_peaked_rows_inside_diffuse_layers_vs_reference_golden(synth_sd, monkeypatch, name, api):
    """What the thresholds of attention_precision='auto' let through: one or two keypoints per image whose attention rows are
    sharply peaked (descriptors scaled by 6 / 10: the reference's own row maxima for them reach 0.8 - 1.0, stored in the fixture) inside layers
    whose mean row maximum stays near 0.01 and whose tail fraction is 1e-3 -- far under the 0.08 / 0.02 thresholds, and one row in a thousand is
    mostly outside the 32-query sample of the 8-wave kernel too.  Those rows run on plain bf16 operands.  The fixture is the unmodified reference on
    the same pair (tools/gen_golden_rare.py): EVERY match index equal, EVERY score within 1e-4 -- the hot keypoints' included, asserted separately.
    Round 6 answers these rows with the guard's LARGEST-ROW-MAXIMUM criterion (attention_auto_rowmax: the layer is redone on the device for this
    batch, not moved up): gain 6 holds the bar without it (5e-5), gain 8 and 10 need it (plain bf16: 6e-4 on neighbouring rows).
    The gain-10 fixture is also a RANGE stress: both partners' descriptors are ten times larger, the score matrix reaches |Z| = 2429 in their
    column, every row's maximum sits there, and the potentials end at |u| = 2308 -- one f32 ulp of which is 2.4e-4, so two correct f32 evaluations
    of that solve differ by more than the 1e-4 bar (our streamed log-domain solve, the arithmetic closest to the reference's, is 1.33e-4 from the
    golden).  It found a real defect: the on-chip Sinkhorn went on with column totals of e^-100 (denormal survivors of K) and was 4.4e-4 off without
    tripping a guard; it now gives up on totals below 1e-30 and the rescue re-solves.  Bar for that fixture: 2.5e-4, matched rows."""
    g = load_golden(name)
    n, seed, rad, pct, ms, iters = [int(x) for x in g["meta"]]
    thr = float(g["match_threshold"])
    pair, hot0, hot1 = make_rare_pair(n, seed, len(g["hot0"]), float(g["gain"]))
    np.testing.assert_array_equal(hot0, g["hot0"])
    assert g["hot_rowmax0"].max() > 0.75 and np.median(g["layer_mean_rowmax0"].max(axis=1)) < 0.03       # peaked rows, diffuse layers: what the fixture is for
    m = GMatcher({"sinkhorn_iterations": iters, "match_threshold": thr}).eval()
    m.load_state_dict(synth_sd)
    _settle(m)
    data = pair_to_data(pair, rad, pct, ms, device="cuda")
    if api == "forward":
        out = m(data)
    elif api == "match_pairs":               # (one pair alone: the running-maximum kernels, which report EVERY row to the statistic)
        out = m.match_pairs([data])[0]
    else:                                    # in a batch of eight on the 8-wave kernel: the statistic is the 32-query sample per (image, head)
        monkeypatch.setenv("GIMS_ATTN_QP", "8")
        hip_counts = __import__("gims_amd.hip", fromlist=["hip"])
        hip_counts.attention_launch_counts(reset=True)
        out = m.match_pairs([data] + [pair_to_data(synth.make_pair(n, 1000 + i), rad, pct, ms, device="cuda") for i in range(7)])[0]
        assert hip_counts.attention_launch_counts()["wave8"] >= 1
    torch.cuda.synchronize()
    tol = 2.5e-4 if float(g["gain"]) >= 10 else 1e-4
    stats = _compare(out, data, g, thr, score_tol=tol)
    k0 = data["kept_kpts0_indices"][0]
    k0 = k0.cpu().numpy() if torch.is_tensor(k0) else np.asarray(k0)
    pos = np.searchsorted(k0, hot0)
    matched = g["out/matches0"][pos] >= 0
    err_hot = np.abs(out["matching_scores0"][0].cpu().numpy()[pos] - g["out/matching_scores0"][pos])[matched].max() if matched.any() else 0.0
    rep = m.attention_report()
    print(name, api, stats, "hot rows' score error", float(err_hot), "tiers", rep["modes"], "redone", rep["redone"].tolist(), "rare", rep["rare"].tolist())
    assert err_hot < tol
    if float(g["gain"]) >= 8:
        assert rep["rare"].sum() > 0 and rep["modes"].count("bf16") >= 15          # answered per batch: the layers were not moved up for one outlier


def _hot_rows_error(out, data, g, hot0, b=0):
    k0 = data["kept_kpts0_indices"][b]
    k0 = k0.cpu().numpy() if torch.is_tensor(k0) else np.asarray(k0)
    pos = np.searchsorted(k0, hot0)
    matched = g["out/matches0"][pos] >= 0
    return float(np.abs(out["matching_scores0"][b].cpu().numpy()[pos] - g["out/matching_scores0"][pos])[matched].max()) if matched.any() else 0.0


def _stacked(pair, copies):
    both = {k: np.concatenate([pair[k]] * copies) for k in pair if k != "gt_perm"}
    both["gt_perm"] = None
    return both


@pytest.mark.parametrize("name,api", [(n, a) for n in SMALL_RARE for a in ("match_pairs_as_pair_0", "match_pairs_as_pair_17", "match_pairs_as_pair_31",
                                                                            "forward_32_copies")] + [(SMALL_RARE[0], "match_pairs_31_pairs")])
def test_rare_peaked_rows_of_small_pairs_in_chip_filling_batches_vs_reference_golden(synth_sd, name, api):
    """The everyday workload: 400-500 kept keypoints per image, 32 pairs per call.  64 images x 4 heads = 256 (problem, head) groups is exactly the
    launcher's threshold, so such a batch runs on the 8-wave kernel WITHOUT any environment switch -- with rows of fewer than 512 keys, where that
    kernel's half-tile bound is too coarse to be the reported figure and every wave whose bound reaches 1/2 measures its rows exactly instead.  The
    fixtures (tools/gen_golden_rare.py: the unmodified reference on a pair with one hot keypoint at gain 8 / two at gain 6, kept at a position
    outside the 32-query sample) are matched as pair 0, 17 and 31 of a batch whose other pairs are diffuse, and as 32 stacked copies through
    forward(): every match index equal, every score within 1e-4, the hot rows asserted separately, the outlier answered per batch
    (rep['rare'] > 0, at least 15 layers still on bf16), the 32 copies equal bit for bit.  With 31 pairs (248 groups) the launcher stays on the
    running-maximum kernels, which report every row: the threshold is pinned from both sides.
    Score error against the reference in the batch of 32, measured once with attention_auto_rowmax = 0 (plain bf16, no redo) and with the
    criterion on: n400 gain 8: 2.9e-5 off, 2.1e-5 on; n500 gain 6: 4.6e-5 (match_pairs) / 3.5e-5 (forward) off, 2.8e-5 / 2.7e-5 on.  Neither
    fixture exceeds the 1e-4 bar on plain bf16 at these sizes (at 1024 keypoints gain 8 cost 6e-4): they are parity coverage of the path, and
    tests/test_attention_rowmax_gpu.py carries the regression of the statistic itself.
    The n500 pair ALONE (or among 31 pairs) is not a case here: its two hot keypoints have no partner and tie for column 499 of the reference's
    assignment to the last bit (the fixture's gap1[499] is 0.0); the running-maximum kernels return 0.3341395 for row 497 against 0.3341293 for
    the reference's row 269 -- 1e-5 apart, the other side of the tie.  The 31-pair case therefore runs on the n400 fixture."""
    from gims_amd import hip
    g = load_golden(name)
    n, seed, rad, pct, ms, iters = [int(x) for x in g["meta"]]
    thr = float(g["match_threshold"])
    pair, hot0, hot1 = make_rare_pair(n, seed, len(g["hot0"]), float(g["gain"]))
    np.testing.assert_array_equal(hot0, g["hot0"])
    assert g["hot_rowmax0"].max() > 0.75 and np.median(g["layer_mean_rowmax0"].max(axis=1)) < 0.03       # peaked rows, diffuse layers
    m = GMatcher({"sinkhorn_iterations": iters, "match_threshold": thr}).eval()
    m.load_state_dict(synth_sd)
    _settle(m)
    hip.attention_launch_counts(reset=True)
    if api.startswith("match_pairs"):
        n_pairs = 31 if api == "match_pairs_31_pairs" else 32
        at = {"match_pairs_as_pair_0": 0, "match_pairs_as_pair_17": 17, "match_pairs_as_pair_31": 31, "match_pairs_31_pairs": 17}[api]
        batch = [pair_to_data(pair if i == at else synth.make_pair(n, 1000 + i), rad, pct, ms, device="cuda") for i in range(n_pairs)]
        out, data = m.match_pairs(batch)[at], batch[at]
    else:
        data = pair_to_data(_stacked(pair, 32), rad, pct, ms, device="cuda")
        out = m(data)
    torch.cuda.synchronize()
    counts = hip.attention_launch_counts()
    if api == "match_pairs_31_pairs":
        assert counts["wave8"] == 0 and counts["wave4"] >= 1, counts
    else:
        assert counts["wave8"] >= 1, counts
    stats = _compare(out, data, g, thr)
    err_hot = _hot_rows_error(out, data, g, hot0)
    rep = m.attention_report()
    print(name, api, stats, "hot rows' score error", err_hot, "tiers", rep["modes"], "redone", rep["redone"].tolist(), "rare", rep["rare"].tolist(), counts)
    assert err_hot < 1e-4
    assert rep["rare"].sum() > 0 and rep["modes"].count("bf16") >= 15
    if api == "forward_32_copies":
        for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
            assert (out[k] == out[k][0:1]).all(), k


@pytest.mark.parametrize("n", [400, 200])
def test_short_diffuse_rows_pay_no_redo_per_batch(synth_sd, n):
    """The other side of the guarantee: rows that are merely SHORT (32 pairs of 400 / 200 keypoints, synth.make_pair only: the 8-wave kernel,
    fewer than 512 keys per row) are no outliers.  The first call may still move layers (the model was settled on another size); from the second
    call on the device redoes nothing and forward() repeats nothing."""
    from gims_amd import hip
    m = GMatcher({}).eval()
    m.load_state_dict(synth_sd)
    _settle(m)
    batch = lambda: [pair_to_data(synth.make_pair(n, 1000 + i), 15, 2, 7, device="cuda") for i in range(32)]      # noqa: E731
    seen = []
    for _ in range(3):
        hip.attention_launch_counts(reset=True)
        m.match_pairs(batch())
        torch.cuda.synchronize()
        assert hip.attention_launch_counts()["wave8"] >= 1
        rep = m.attention_report()
        seen.append((int(rep["redone"].sum()), int(rep["rare"].sum()), rep["modes"].count("bf16")))
    print("match_pairs 32 x", n, "(redone, rare, bf16 layers) after each call:", seen)
    assert seen[1][0] == seen[0][0] and seen[2][0] == seen[0][0], seen        # the second and third call redo nothing
    m2 = GMatcher({}).eval()
    m2.load_state_dict(synth_sd)
    _settle(m2)
    reps = []
    for _ in range(3):
        hip.attention_launch_counts(reset=True)
        m2(pair_to_data(_stacked(synth.make_pair(n, 1000), 32), 15, 2, 7, device="cuda"))
        assert hip.attention_launch_counts()["wave8"] >= 1
        reps.append(getattr(m2, "_attn_forward_repeats", 0))
    print("forward 32 x", n, "repeats after each call:", reps)
    assert reps[1] == reps[0] and reps[2] == reps[0], reps


def test_forward_and_match_pairs_count_an_outlier_batch_alike(synth_sd):
    """attention_auto_rare_batches = 3 means three BATCHES for both entry points: forward() repeats an outlier batch with the device-side guards
    on, and the repeat's statistic -- the same rows again -- does not count a second time.  Three calls each on fresh settled models: the same
    rep['rare'] and the same tiers after every call, every returned batch within the reference golden."""
    name = "raree2e_n1024_s1052_h1g8_r15p2m7_i100"
    g = load_golden(name)
    n, seed, rad, pct, ms, iters = [int(x) for x in g["meta"]]
    pair, hot0, _ = make_rare_pair(n, seed, len(g["hot0"]), float(g["gain"]))
    seen = {}
    for api in ("forward", "match_pairs"):
        m = GMatcher({}).eval()
        m.load_state_dict(synth_sd)
        _settle(m)
        seen[api] = []
        for _ in range(3):
            data = pair_to_data(pair, rad, pct, ms, device="cuda")
            out = m(data) if api == "forward" else m.match_pairs([data])[0]
            torch.cuda.synchronize()
            _compare(out, data, g, 0.2)
            assert _hot_rows_error(out, data, g, hot0) < 1e-4
            rep = m.attention_report()
            seen[api].append((rep["rare"].tolist(), rep["modes"]))
        print(api, [(sum(r), md.count("f16")) for r, md in seen[api]], "forward repeats", getattr(m, "_attn_forward_repeats", 0))
    assert sum(seen["match_pairs"][0][0]) > 0
    for k in range(3):
        assert seen["forward"][k] == seen["match_pairs"][k], k
    assert seen["forward"][1][1].count("f16") == 0 and seen["forward"][2][1].count("f16") > 0      # moved up by the third batch, not the second


def test_an_outlier_batch_does_not_make_unmeasured_batches_repeat(synth_sd):
    """attention_monitor_period = 4: one measured batch with an outlier row is repeated once (and the repeat, being the same batch, is measured
    too: its device-side guards need the statistic); the six diffuse pairs after it -- mostly unmeasured -- inherit nothing from it."""
    rare_name, plain_name = "raree2e_n1024_s1052_h1g8_r15p2m7_i100", "e2e_n1024_s1000_r15p2m7_i100"
    g, gp = load_golden(rare_name), load_golden(plain_name)
    n, seed, rad, pct, ms, iters = [int(x) for x in g["meta"]]
    assert [int(x) for x in gp["meta"]][2:] == [rad, pct, ms, iters] and float(gp["match_threshold"]) == float(g["match_threshold"]) == 0.2
    pair, hot0, _ = make_rare_pair(n, seed, len(g["hot0"]), float(g["gain"]))
    plain = synth.make_pair(1024, 1000)
    m = GMatcher({"attention_monitor_period": 4}).eval()
    m.load_state_dict(synth_sd)
    _settle(m)                                                     # batch 0 (calibration)
    for _ in range(3):                                            # batches 1-3: not measured
        data = pair_to_data(plain, rad, pct, ms, device="cuda")
        _compare(m(data), data, gp, 0.2)
    r0 = getattr(m, "_attn_forward_repeats", 0)
    data = pair_to_data(pair, rad, pct, ms, device="cuda")      # batch 4: measured, one outlier row
    out = m(data)
    _compare(out, data, g, 0.2)
    assert _hot_rows_error(out, data, g, hot0) < 1e-4
    assert m.attention_report()["rare"].sum() > 0
    for _ in range(6):
        data = pair_to_data(plain, rad, pct, ms, device="cuda")
        _compare(m(data), data, gp, 0.2)
    r1 = getattr(m, "_attn_forward_repeats", 0)
    print("forward repeats before / after:", r0, r1)
    assert r1 - r0 <= 1


def test_repeated_rare_rows_move_the_layer_up(synth_sd):
    """attention_auto_rare_batches = 3: a layer whose rows reach the row-maximum criterion on three batches is no outlier -- a per-batch redo on
    the split-bf16 kernels (3 x the matrix work) costs more than the half tier (1.2 x) -- so it is moved to the half tier for good; the batches
    before and after that all meet the reference golden (raree2e_*_g8: the unmodified reference on the same pair)."""
    name = "raree2e_n1024_s1052_h1g8_r15p2m7_i100"
    g = load_golden(name)
    n, seed, rad, pct, ms, iters = [int(x) for x in g["meta"]]
    pair, hot0, _ = make_rare_pair(n, seed, len(g["hot0"]), float(g["gain"]))
    m = GMatcher({}).eval()
    m.load_state_dict(synth_sd)
    _settle(m)
    seen = []
    for k in range(5):
        data = pair_to_data(pair, rad, pct, ms, device="cuda")
        out = m.match_pairs([data])[0]
        torch.cuda.synchronize()
        _compare(out, data, g, 0.2)
        rep = m.attention_report()
        seen.append((rep["modes"].count("f16"), int(rep["redone"].sum())))
    print(seen)
    (f0, r0), (f1, r1), (f2, r2), (f3, r3), (f4, r4) = seen
    assert f0 == f1 == 0 and r0 > 0 and r1 > r0                     # batches 1-2: redone per batch, no layer moved
    assert f2 > 0 and f3 == f2 and f4 == f2                          # the third batch moved the repeat offenders up, once
    assert r4 - r3 < r1 - r0                                         # ... and what is left to redo per batch is less than before
    assert "bf16" in rep["modes"]                                    # layers without such rows stay on the fast tier


@pytest.mark.parametrize("api", ["forward", "match_pairs"])
@pytest.mark.parametrize("name", ["peakede2e_n1024_s1010_r15p2m7_i100", "peakede2e_n1024_s1011_r15p2m7_i20"])
def test_auto_attention_holds_the_bar_on_the_first_sharpened_batch(name, api):
    """'auto' as a GUARANTEE: ONE settled model -- all 18 layers on plain bf16 attention -- is handed a batch whose attention
    is PEAKED (the `peaked` weights swapped in under the settled tier table: a trained model meeting an input that sharpens its layers).  Plain
    bf16 is at 3.1e-4 on this fixture.  The verdict is drawn on the device inside the batch: the guarded launches behind every bf16 attention
    launch see the statistic that launch produced and redo the layer at split-bf16 before its message is consumed -- so THIS batch, not the one
    after it, already meets the reference golden (indices exact, scores < 1e-4), through forward() and through the asynchronous match_pairs().
    Afterwards the host has moved the layers up and nothing is redone any more."""
    g = load_golden(name)
    n, seed, rad, pct, ms, iters = [int(x) for x in g["meta"]]
    gq = float(g["gain_qk"])
    m = GMatcher({"sinkhorn_iterations": iters, "match_threshold": float(g["match_threshold"])}).eval()
    m.load_state_dict(synth.make_state_dict(123))
    mk = lambda: pair_to_data(synth.make_pair(n, seed), rad, pct, ms, device="cuda")      # noqa: E731
    m(mk()); m(mk())
    rep = m.attention_report()
    assert rep["calibrated"] and rep["modes"] == ["bf16"] * 18 and rep["redone"].sum() == 0, rep
    m.load_state_dict(synth.make_state_dict(123, gains={"attn.proj.0": gq, "attn.proj.1": gq}))
    m._keep_attention_tiers("cuda")

    def run():
        data = mk()
        if api == "forward":
            return m(data), data
        out = m.match_pairs([data])[0]
        torch.cuda.synchronize()
        data = dict(data, kept_kpts0_indices=[data["kept_kpts0_indices"][0].cpu().numpy()], kept_kpts1_indices=[data["kept_kpts1_indices"][0].cpu().numpy()])
        return out, data
    out, data = run()                                        # the FIRST sharpened batch: still the all-bf16 table, redone on the device
    stats = _compare(out, data, g, float(g["match_threshold"]))
    rep = m.attention_report()
    print(name, api, "first sharpened batch:", stats, "redone on the device:", rep["redone"], "forward repeats:", getattr(m, "_attn_forward_repeats", 0),
          "modes after:", rep["modes"])
    if api == "match_pairs":            # no host synchronisation inside the call: guarded launches redid the layers on the device
        assert (rep["redone"] > 0).sum() >= 12, rep["redone"]
    else:                               # forward() read the statistic at its final synchronisation and repeated the batch on the new table
        assert getattr(m, "_attn_forward_repeats", 0) >= 1 and rep["redone"].sum() == 0
    assert rep["modes"].count("f16") >= 12 and rep["modes"].count("bf16x3") == 0, rep["modes"]      # ... and the host moved them up for good
    before = rep["redone"].copy()
    out, data = run()                                        # settled on the half kernels: nothing left to redo on those layers
    print(name, api, "next batch:", _compare(out, data, g, float(g["match_threshold"])))
    rep = m.attention_report()
    moved = np.asarray([md != "bf16" for md in rep["modes"]])
    assert (rep["redone"][moved] == before[moved]).all()


def test_match_pairs_refuses_mixed_graph_parameters(synth_sd):
    """One graph-build launch serves a whole match_pairs batch; a caller mixing radius / percentile / min_size used to get pair 0's silently."""
    m = GMatcher({}).eval()
    m.load_state_dict(synth_sd)
    a = pair_to_data(synth.make_pair(256, 1002), 15, 2, 7, device="cuda")
    b = pair_to_data(synth.make_pair(256, 1003), 25, 7, 8, device="cuda")
    with pytest.raises(ValueError, match="share the adaptive-graph parameters"):
        m.match_pairs([a, b])


@pytest.mark.parametrize("name", golden_names("full_"))
def test_intermediates_vs_reference_golden(models, name):
    g = load_golden(name)
    n, seed, rad, pct, ms, iters = [int(x) for x in g["meta"]]
    pair = {k[3:]: g[k] for k in g if k.startswith("in/")}
    data = pair_to_data(pair, rad, pct, ms, device="cuda")
    m = models[("f32", iters)]
    out = m(data)
    last = m._last
    (o0, n0), (o1, n1) = last["pairs"][0]
    sage = last["sage"].cpu().numpy()  # noqa
    np.testing.assert_allclose(sage[o0:o0 + n0], g["out/sage0"], atol=5e-5, rtol=1e-5)
    np.testing.assert_allclose(sage[o1:o1 + n1], g["out/sage1"], atol=5e-5, rtol=1e-5)
    desc = last["desc"].cpu().numpy()
    np.testing.assert_allclose(desc[o0:o0 + n0].T, g["out/gnn0"], atol=2e-3, rtol=1e-3)   # bf16 attention inside
    np.testing.assert_allclose(out["mdesc0"].cpu().numpy(), g["out/mdesc0"], atol=5e-3, rtol=1e-3)
    it = last["items"][0]
    np.testing.assert_allclose(it["scores"][:, :n1].cpu().numpy(), g["out/scores"], atol=2e-2, rtol=1e-3)
    _compare(out, data, g, float(g["match_threshold"]))


def test_batch_of_two_pairs_equals_single(models):
    """B=2 (equal kept counts, as the reference requires for torch.stack) gives the same result per pair."""
    m = models[("bf16x3", 100)]
    pairs = [synth.make_pair(64, 1000), synth.make_pair(64, 1000)]
    singles = [m(pair_to_data(p, 15, 2, 7, device="cuda")) for p in pairs]
    both = {k: np.concatenate([p[k] for p in pairs]) for k in pairs[0] if k != "gt_perm"}
    both["gt_perm"] = None
    out = m(pair_to_data(both, 15, 2, 7, device="cuda"))
    for b in range(2):
        np.testing.assert_array_equal(out["matches0"][b].cpu().numpy(), singles[b]["matches0"][0].cpu().numpy())
        np.testing.assert_allclose(out["matching_scores0"][b].cpu().numpy(), singles[b]["matching_scores0"][0].cpu().numpy(), atol=1e-6)


def test_full_size_properties(models):
    """BASELINE config sizes (4096 keypoints): size-independent properties instead of an oracle run --
    matches are mutual, scores in (thr, 1], planted correspondences recovered, run-to-run bitwise equal."""
    m = models[("bf16x3", 100)]
    pair = synth.make_pair(4096, 1000)
    outs = []
    for _ in range(2):
        data = pair_to_data(pair, 15, 2, 7, device="cuda")
        outs.append((m(data), data))
    (o, data), (o2, _) = outs
    m0, m1 = o["matches0"][0].cpu().numpy(), o["matches1"][0].cpu().numpy()
    s0 = o["matching_scores0"][0].cpu().numpy()
    np.testing.assert_array_equal(m0, o2["matches0"][0].cpu().numpy())
    np.testing.assert_array_equal(s0, o2["matching_scores0"][0].cpu().numpy())       # deterministic kernels
    v = m0 >= 0
    assert (m1[m0[v]] == np.nonzero(v)[0]).all()
    assert (s0[v] > 0.2).all() and (s0 <= 1.0 + 1e-5).all()
    k0, k1 = np.asarray(data["kept_kpts0_indices"][0]), np.asarray(data["kept_kpts1_indices"][0])
    assert len(k0) > 4000 and len(k1) > 4000
    gt = pair["gt_perm"][k0[v]]
    correct = (k1[m0[v]] == gt).sum()
    assert correct > 0.95 * v.sum() and v.sum() > 3000, (correct, v.sum())


def test_match_pairs_ragged_equals_forward(models):
    """The ragged batch API returns, pair by pair, exactly what forward() returns for that pair alone."""
    m = models[("bf16x3", 100)]
    specs = [(256, 1002), (200, 1001), (512, 1004)]
    pairs = [synth.make_pair(n, s, canvas=synth.canvas_for(256) if n == 200 else None) for n, s in specs]
    singles = [m(pair_to_data(p, 15, 2, 7, device="cuda")) for p in pairs]
    datas = [pair_to_data(p, 15, 2, 7, device="cuda") for p in pairs]
    outs = m.match_pairs(datas)
    for o, s, d in zip(outs, singles, datas):
        np.testing.assert_array_equal(o["matches0"].cpu().numpy(), s["matches0"].cpu().numpy())
        np.testing.assert_array_equal(o["matches1"].cpu().numpy(), s["matches1"].cpu().numpy())
        np.testing.assert_allclose(o["matching_scores0"].cpu().numpy(), s["matching_scores0"].cpu().numpy(), atol=2e-6)
        assert d["keypoints0"].shape[1] == o["matches0"].shape[1]


def test_match_pairs_extreme_shapes_equal_forward(models):
    """One ragged batch holding very different problems -- 6000 / 300 and 300 / 6000 keypoints (tall and wide score matrices: the on-chip Sinkhorn
    geometry, the attention launch shapes and the score GEMM all see n0 >> n1 and n1 >> n0), a 64 / 64 pair, a 9000 / 8000 pair (streamed
    Sinkhorn) next to pairs that solve on chip -- against forward() on each pair alone: indices equal, scores within 5e-5 (the attention kernel a
    launch takes depends on the batch, so the bits need not be)."""
    m = models[("bf16x3", 20)]
    # (radius 25 / min_size 3: the 300-keypoint images lie on the 6000-keypoint canvas, a twentieth of the usual density)
    specs = [(6000, 300, 250, 3201), (300, 6000, 250, 3202), (64, 64, 50, 3203), (9000, 8000, 7000, 3204), (1500, 900, 700, 3001)]
    pairs = [synth.make_pair_unbalanced(a, b, c, sd, canvas=synth.canvas_for(max(a, b))) for a, b, c, sd in specs]
    singles = [m(pair_to_data(p, 25, 2, 3, device="cuda")) for p in pairs]
    outs = m.match_pairs([pair_to_data(p, 25, 2, 3, device="cuda") for p in pairs])
    torch.cuda.synchronize()
    assert (m.sinkhorn_status() == 0).all()
    for (a, b, c, sd), o, s1 in zip(specs, outs, singles):
        m0, r0 = o["matches0"].cpu().numpy(), s1["matches0"].cpu().numpy()
        sc, rs = o["matching_scores0"].cpu().numpy(), s1["matching_scores0"].cpu().numpy()
        assert m0.shape == r0.shape, (a, b)
        # rows whose decision is conditioned worse than the tolerance between two attention kernels may flip; there are next to none
        differ = m0 != r0
        assert differ.mean() < 2e-3, (a, b, int(differ.sum()))
        assert np.abs(sc - rs)[~differ].max() < 5e-5, (a, b)
        assert (m0 >= 0).sum() > 0.5 * c * (0.2 if min(a, b) < 1000 else 1.0), (a, b, int((m0 >= 0).sum()))


def test_errors_like_reference():
    m = GMatcher({}).eval()
    pair = synth.make_pair(64, 1000)
    data = pair_to_data(pair, 15, 2, 7, device="cpu")
    with pytest.raises(RuntimeError):
        m(data)            # no CPU fallback


def test_two_stream_lanes_equal_single_stream(synth_sd, monkeypatch):
    """match_pairs with two stream lanes returns exactly the single-stream results -- and plans the STREAMED Sinkhorn kernels
    (the on-chip kernels need the whole device; concurrent lanes would send every solve through the rescue), even where the
    environment forces the on-chip path for a single lane."""
    monkeypatch.setenv("GIMS_OT_RESIDENT", "2")
    pairs = [synth.make_pair(n, s, canvas=synth.canvas_for(256) if n == 200 else None)
             for n, s in ((256, 1002), (200, 1001), (512, 1004), (64, 1000), (256, 1003))]
    res = []
    for lanes in (1, 2):
        m = GMatcher({"streams": lanes}).eval()
        m.load_state_dict(synth_sd)
        outs = m.match_pairs([pair_to_data(p, 15, 2, 7, device="cuda") for p in pairs])
        torch.cuda.synchronize()
        assert (m.sinkhorn_plan_last > 0) == (lanes == 1), (lanes, m.sinkhorn_plan_last)
        assert (m.sinkhorn_status() == 0).all()
        res.append(outs)
    for a, b in zip(*res):
        np.testing.assert_array_equal(a["matches0"].cpu().numpy(), b["matches0"].cpu().numpy())
        np.testing.assert_allclose(a["matching_scores0"].cpu().numpy(), b["matching_scores0"].cpu().numpy(), atol=2e-5)   # on-chip vs streamed solve


def test_a_match_pairs_call_that_raises_leaves_no_mode_behind(synth_sd):
    """The mode of a call (stream lanes, device-side guards) travels with the call: a two-lane match_pairs that raises -- here in its argument
    check, before any launch -- leaves nothing on the model.  The next forward() plans the on-chip Sinkhorn and returns what a fresh
    single-stream model returns, bit for bit (a lane count that outlived the failed call made every later forward() plan the streamed kernels)."""
    m = GMatcher({"streams": 2}).eval()
    m.load_state_dict(synth_sd)
    datas = [pair_to_data(synth.make_pair(256, seed), 15, 2, 7, device="cuda") for seed in (1002, 1003, 1004, 1005)]
    datas[2] = {k: torch.cat([v, v]) if torch.is_tensor(v) else v for k, v in datas[2].items()}        # B == 2
    with pytest.raises(ValueError, match="match_pairs takes single-pair dicts"):
        m.match_pairs(datas)
    fresh = GMatcher({}).eval()
    fresh.load_state_dict(synth_sd)
    pair = synth.make_pair(256, 1002)
    out, ref = m(pair_to_data(pair, 15, 2, 7, device="cuda")), fresh(pair_to_data(pair, 15, 2, 7, device="cuda"))
    assert m.sinkhorn_plan_last == fresh.sinkhorn_plan_last and m._lane == 0, (m.sinkhorn_plan_last, fresh.sinkhorn_plan_last, m._lane)
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
        np.testing.assert_array_equal(out[k].cpu().numpy(), ref[k].cpu().numpy())


def test_replayed_layers_equal_stepwise(synth_sd):
    """The 18 GNN layers replayed through gims_run_ops (one ABI crossing, argument table cached across calls) give exactly
    what the launch-by-launch path gives (the one that runs when stage timers are on)."""
    pairs = [synth.make_pair(n, s) for n, s in ((256, 1002), (512, 1004), (256, 1003))]
    m = GMatcher({}).eval()
    m.load_state_dict(synth_sd)
    _settle(m)
    res = []
    for timed in (False, True, False):           # replay (cold cache), stepwise, replay (warm cache)
        m.enable_timing(timed, stepwise=timed)
        outs = m.match_pairs([pair_to_data(p, 15, 2, 7, device="cuda") for p in pairs])
        torch.cuda.synchronize()
        res.append([(o["matches0"].cpu().numpy(), o["matching_scores0"].cpu().numpy()) for o in outs])
    # (launch-by-launch issue fills the same caches: entry [2] counts the times a table went to the library in ONE call)
    assert any(e[2] for e in m.__dict__.get("_ops_cache", {}).values()), "the replay path did not run"
    assert any(e[2] for e in m.__dict__.get("_enc_cache", {}).values()), "the encoder stage (GraphSAGE + keypoint encoder) did not replay"
    for other in res[1:]:
        for (m0, s0), (m1, s1) in zip(res[0], other):
            np.testing.assert_array_equal(m0, m1)
            np.testing.assert_array_equal(s0, s1)
    # the cached encoder table is PATCHED per call (row count + the batch's pointers): batches of other sizes through the same table, then the
    # first batch again -- its bits must come back, and each must equal its stepwise evaluation
    m.enable_timing(False)
    others = [synth.make_pair(n, sd) for n, sd in ((200, 1001), (700, 1010))]
    n_tables = len(m._enc_cache)
    o_small = m.match_pairs([pair_to_data(p, 15, 2, 7, device="cuda") for p in others[:1]])
    s_small = o_small[0]["matching_scores0"].cpu().numpy()
    o_big = m.match_pairs([pair_to_data(p, 15, 2, 7, device="cuda") for p in others + pairs])
    s_big = [o["matching_scores0"].cpu().numpy() for o in o_big]
    again = m.match_pairs([pair_to_data(p, 15, 2, 7, device="cuda") for p in pairs])
    for (m0, s0), o in zip(res[0], again):
        np.testing.assert_array_equal(m0, o["matches0"].cpu().numpy())
        np.testing.assert_array_equal(s0, o["matching_scores0"].cpu().numpy())
    m.enable_timing(True, stepwise=True)
    ref_small = m.match_pairs([pair_to_data(p, 15, 2, 7, device="cuda") for p in others[:1]])[0]["matching_scores0"].cpu().numpy()
    ref_big = [o["matching_scores0"].cpu().numpy() for o in m.match_pairs([pair_to_data(p, 15, 2, 7, device="cuda") for p in others + pairs])]
    m.enable_timing(False)
    np.testing.assert_array_equal(s_small, ref_small)
    for a, b in zip(s_big, ref_big):
        np.testing.assert_array_equal(a, b)
    assert len(m._enc_cache) <= n_tables + 1          # (the arena may have grown once for the largest batch: a new table then, not one per size)


@pytest.mark.parametrize("variant", ["unfused", "f32", "layernorm"])
def test_one_call_issue_equals_stepwise_in_every_configuration(synth_sd, variant):
    """fuse_merge=False, linear_precision='f32' and use_layernorm=True run from the same cached tables as the default configuration: issued in
    one call and launch by launch they give the same bits -- also for a batch of another row count through the same patched encoder table, and
    for the first batch again after it (a stale row count or pointer in a cached table shows up there)."""
    cfg = {"unfused": {"fuse_merge": False}, "f32": {"linear_precision": "f32"}, "layernorm": {"use_layernorm": True}}[variant]
    m = GMatcher(cfg).eval()
    m.load_state_dict(synth.make_state_dict(123, use_layernorm=True) if variant == "layernorm" else synth_sd)
    _settle(m)
    batches = [[synth.make_pair(256, 1002), synth.make_pair(512, 1004)], [synth.make_pair(200, 1001)]]
    batches.append(batches[0])
    res = []
    for stepwise in (False, True):
        m.enable_timing(stepwise, stepwise=stepwise)
        res.append([])
        for batch in batches:
            outs = m.match_pairs([pair_to_data(p, 15, 2, 7, device="cuda") for p in batch])
            res[-1].append([(o["matches0"].cpu().numpy(), o["matching_scores0"].cpu().numpy()) for o in outs])
        if not stepwise:
            for cache in ("_ops_cache", "_enc_cache"):
                assert any(e[2] for e in m.__dict__.get(cache, {}).values()), cache + ": no table was issued in one call"
            uses = sum(e[2] for cache in ("_ops_cache", "_enc_cache") for e in m.__dict__[cache].values())
    m.enable_timing(False)
    assert uses == sum(e[2] for cache in ("_ops_cache", "_enc_cache") for e in m.__dict__[cache].values()), "the stepwise pass issued a table in one call"
    for a, b in list(zip(res[0], res[1])) + [(res[0][0], res[0][2])]:
        assert len(a) == len(b)
        for (m0, s0), (m1, s1) in zip(a, b):
            np.testing.assert_array_equal(m0, m1)
            np.testing.assert_array_equal(s0, s1)


def test_graph_replay_equals_plain_replay(synth_sd):
    """GIMS_OPS_GRAPH=1 on a non-default stream: the layer sequence captured into a HIP graph gives the same bits."""
    pairs = [synth.make_pair(n, s) for n, s in ((256, 1002), (512, 1004))]
    res = []
    side = torch.cuda.Stream()
    for graph in (False, True):
        m = GMatcher({}).eval()
        m.load_state_dict(synth_sd)
        m._use_graph = graph
        with torch.cuda.stream(side):
            for _ in range(3):                     # the graph is built on the second use of a cached table
                outs = m.match_pairs([pair_to_data(p, 15, 2, 7, device="cuda") for p in pairs])
            torch.cuda.synchronize()
        if graph:
            assert any(v[1] is not None for v in m.__dict__["_ops_cache"].values()), "no graph was instantiated"
        res.append([(o["matches0"].cpu().numpy(), o["matching_scores0"].cpu().numpy()) for o in outs])
    for (m0, s0), (m1, s1) in zip(*res):
        np.testing.assert_array_equal(m0, m1)
        np.testing.assert_array_equal(s0, s1)


def test_unequal_keypoint_counts_vs_oracle(models, synth_sd):
    """N0 != N1 (image 1 lost a third of its keypoints): HIP path vs the CPU oracle on the same inputs."""
    pair = synth.make_pair(384, 1010)
    keep = 250
    for k in ("keypoints1", "scores1"):
        pair[k] = np.ascontiguousarray(pair[k][:, :keep])
    pair["descriptors1"] = np.ascontiguousarray(pair["descriptors1"][:, :, :keep])
    m = models[("bf16x3", 100)]
    d_gpu = pair_to_data(pair, 15, 2, 7, device="cuda")
    out = m(d_gpu)
    d_cpu = pair_to_data(pair, 15, 2, 7, device="cpu")
    st = {}
    ref = O.gmatcher_forward(synth_sd, d_cpu, {}, stages=st)
    assert d_gpu["kept_kpts0_indices"] == d_cpu["kept_kpts0_indices"] and d_gpu["kept_kpts1_indices"] == d_cpu["kept_kpts1_indices"]
    assert out["matches0"].shape == ref["matches0"].shape and out["matches1"].shape == ref["matches1"].shape
    inner = st["ot"][0][:-1, :-1]
    t2 = inner.topk(2, dim=1).values
    rs0 = ref["matching_scores0"][0].numpy()
    safe = ((t2[:, 0] - t2[:, 1]).numpy() > 1e-3) & (np.abs(rs0 - 0.2) > 1e-3)
    m0, r0 = out["matches0"][0].cpu().numpy(), ref["matches0"][0].numpy()
    assert safe.mean() > 0.9 and (m0[safe] == r0[safe]).all()
    assert np.abs(out["matching_scores0"][0].cpu().numpy() - rs0)[m0 == r0].max() < 1e-4


def test_stress_8192_keypoints(models):
    """BASELINE config 5 size: one 2x8192 pair -- properties only (the oracle would take minutes)."""
    m = models[("bf16x3", 20)]
    pair = synth.make_pair(8192, 1000)
    data = pair_to_data(pair, 15, 2, 7, device="cuda")
    o = m(data)
    m0, m1 = o["matches0"][0].cpu().numpy(), o["matches1"][0].cpu().numpy()
    s0 = o["matching_scores0"][0].cpu().numpy()
    v = m0 >= 0
    assert (m1[m0[v]] == np.nonzero(v)[0]).all() and (s0[v] > 0.02).all() and np.isfinite(s0).all()
    k0, k1 = np.asarray(data["kept_kpts0_indices"][0]), np.asarray(data["kept_kpts1_indices"][0])
    assert len(k0) > 8000 and len(k1) > 8000
    correct = (k1[m0[v]] == pair["gt_perm"][k0[v]]).sum()
    assert v.sum() > 6000 and correct > 0.9 * v.sum(), (int(v.sum()), int(correct))


def test_sparse_graph_few_kept_vs_oracle(models, synth_sd):
    """Sparse keypoints: the adaptive graph drops most of them (512 on 800x600 keeps a few dozen); the
    rest of the path then runs on tiny, different-sized images."""
    pair = synth.make_pair(512, 2000, canvas=(800, 600))
    m = models[("bf16x3", 100)]
    d_gpu = pair_to_data(pair, 15, 2, 7, device="cuda")
    out = m(d_gpu)
    d_cpu = pair_to_data(pair, 15, 2, 7, device="cpu")
    st = {}
    ref = O.gmatcher_forward(synth_sd, d_cpu, {}, stages=st)
    assert d_gpu["kept_kpts0_indices"] == d_cpu["kept_kpts0_indices"] and d_gpu["kept_kpts1_indices"] == d_cpu["kept_kpts1_indices"]
    n0, n1 = len(d_cpu["kept_kpts0_indices"][0]), len(d_cpu["kept_kpts1_indices"][0])
    assert 0 < n0 < 200 and 0 < n1 < 200
    assert out["matches0"].shape == (1, n0) and out["matches1"].shape == (1, n1)
    np.testing.assert_allclose(out["matching_scores0"][0].cpu().numpy(), ref["matching_scores0"][0].numpy(), atol=1e-4)
    r0 = ref["matches0"][0].numpy()
    safe = safe_rows(st["ot"][0].numpy(), 0.2, r0, ref["matching_scores0"][0].numpy())
    assert safe.mean() > 0.8
    np.testing.assert_array_equal(out["matches0"][0].cpu().numpy()[safe], r0[safe])          # every well-conditioned row: exact


def test_everything_removed_raises_like_reference(models):
    """No radius edges at all -> every node is a size-1 component -> all removed -> the reference dies in np.vstack([])
    with ValueError (agc.py:701); same exception type here."""
    pair = synth.make_pair(64, 1000, canvas=(100000, 100000))
    with pytest.raises(ValueError):
        models[("bf16x3", 100)](pair_to_data(pair, 1, 2, 7, device="cuda"))


def test_tiny_pair(models, synth_sd):
    pair = synth.make_pair(24, 7, canvas=(40, 30))
    d_gpu = pair_to_data(pair, 15, 2, 3, device="cuda")
    out = models[("f32", 100)](d_gpu)
    d_cpu = pair_to_data(pair, 15, 2, 3, device="cpu")
    ref = O.gmatcher_forward(synth_sd, d_cpu, {})
    assert d_gpu["kept_kpts0_indices"] == d_cpu["kept_kpts0_indices"]
    np.testing.assert_allclose(out["matching_scores0"][0].cpu().numpy(), ref["matching_scores0"][0].numpy(), atol=1e-4)


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", golden_names("lne2e_"))
def test_e2e_layernorm_vs_reference_golden(name, prec):
    """use_layernorm=True (gmatcher.py:19-20, 74-85): conv -> LayerNorm (unbiased std, eps on the std) -> ReLU in every MLP."""
    g = load_golden(name)
    n, seed, rad, pct, ms, iters = [int(x) for x in g["meta"]]
    m = GMatcher({"use_layernorm": True, "sinkhorn_iterations": iters, "linear_precision": prec}).eval()
    m.load_state_dict(synth.make_state_dict(123, use_layernorm=True))
    pair = synth.make_pair(n, seed)
    data = pair_to_data(pair, rad, pct, ms, device="cuda")
    out = m(data)
    stats = _compare(out, data, g, float(g["match_threshold"]))
    print(name, prec, stats)


def test_layernorm_kernel(models):
    from gims_amd import hip
    r = np.random.default_rng(4)
    for rows, c in ((1000, 512), (77, 32), (300, 64), (513, 256)):
        x = (r.normal(size=(rows, c)) * 3 + 1).astype(np.float32)
        a2, b2 = r.normal(size=c).astype(np.float32), r.normal(size=c).astype(np.float32)
        xt = torch.from_numpy(x)
        ref = torch.from_numpy(a2) * ((xt - xt.mean(1, keepdim=True)) / (xt.std(1, keepdim=True) + 1e-6)) + torch.from_numpy(b2)
        ref = torch.relu(ref).numpy()
        xd = torch.from_numpy(x).cuda()
        osp = torch.zeros((rows, 2 * c), dtype=torch.bfloat16, device="cuda")
        out = hip.layernorm_act(xd, torch.from_numpy(a2).cuda(), torch.from_numpy(b2).cuda(), out=torch.empty_like(xd))
        hip.layernorm_act(xd, torch.from_numpy(a2).cuda(), torch.from_numpy(b2).cuda(), out_split=osp)
        np.testing.assert_allclose(out.cpu().numpy(), ref, atol=2e-5 * max(1.0, np.abs(ref).max()), rtol=0)
        hi, lo = hip.spl32_planes(osp)
        rec = hi.float().cpu().numpy().astype(np.float64) + lo.float().cpu().numpy()
        assert (np.abs(rec - out.cpu().numpy()) <= np.abs(out.cpu().numpy()) * 2.0 ** -15 + 1e-30).all()


def test_matching_without_keypoints_through_a_front_end(synth_sd):
    """The call eval_homography.py:177 makes -- image0 / image1 / carhynet / device and NO keypoints: Matching runs its front
    end per image (here a stand-in for utils.common.sift_forward that returns the synthetic pair's tensors as one-element
    lists, like sift_forward does) and returns {**front-end outputs, **GMatcher outputs} (models/matching.py:15-30):
    the same matches as the call with keypoints."""
    pair = synth.make_pair(256, 1002)
    order = []

    def front_end(d, device):
        s = str(len(order))
        order.append(d["image"].shape)
        assert d["max_keypoints"] == -1 and d["carhynet"] == "the-net"
        return {"keypoints": [torch.from_numpy(pair["keypoints" + s][0]).to(device)], "scores": [torch.from_numpy(pair["scores" + s][0]).to(device)],
                "descriptors": [torch.from_numpy(pair["descriptors" + s][0]).to(device)]}

    m = Matching({"front_end": front_end}).eval()
    m.gmodel.load_state_dict(synth_sd)
    _settle(m.gmodel)
    dev = torch.device("cuda")
    out = m({"image0": pair["image0"], "image1": pair["image1"], "carhynet": "the-net", "device": dev, "radius": 15, "percentile": 2, "min_size": 7})
    assert len(order) == 2
    ref = m(pair_to_data(pair, 15, 2, 7, device="cuda"))        # keypoints given: the front end is not called
    assert len(order) == 2
    for k in ("matches0", "matches1", "matching_scores0", "keypoints0", "descriptors1"):
        assert torch.equal(out[k], ref[k]), k
    assert isinstance(out["scores0"], list) and out["scores0"][0].shape == (256,)      # the front end's own entries are merged in
    assert "scores0" not in ref


@pytest.mark.parametrize("sinkhorn", ["streamed", "resident"])
@pytest.mark.parametrize("name", golden_names("trainloss_") + golden_names("binloss_"))
def test_train_loss_forward_vs_reference_golden(monkeypatch, name, sinkhorn):
    """mode='train' (train.py:136 -> gmatcher.py:254, 309-386), forward value: (loss, pos_loss, neg_loss) within 1e-4 of what the
    reference returned for the same pairs / ground-truth rows / weights (module in eval mode: running-statistics BatchNorm)."""
    monkeypatch.setenv("GIMS_OT_RESIDENT", "0" if sinkhorn == "streamed" else "2")
    g = load_golden(name)
    pairs = train_pairs(name, g)
    sd = fixture_state_dict(g)                       # binloss_*: the fixture's bin_score
    m = GMatcher({"sinkhorn_iterations": int(g["meta"][4]), "pos_loss_weight": float(g["pos_loss_weight"]),
                  "neg_loss_weight": float(g["neg_loss_weight"])}).eval()
    m.load_state_dict(sd)
    data = train_data(pairs, g, device="cuda")
    loss, pos, neg = m(data, mode="train")
    assert loss.dim() == 0 and loss.dtype == torch.float32
    for b in range(len(pairs)):
        np.testing.assert_array_equal(np.asarray(data["kept_kpts0_indices"][b]), g[f"kept0_{b}"])
    got = [float(loss), float(pos), float(neg)]
    print(name, sinkhorn, got, [float(g["loss"]), float(g["pos"]), float(g["neg"])])
    np.testing.assert_allclose(got, [g["loss"], g["pos"], g["neg"]], atol=1e-4, rtol=0)
    m2 = GMatcher({"sinkhorn_iterations": 5}).eval()
    m2.load_state_dict(sd)
    with pytest.raises(KeyError):                     # like the reference: the loss weights have no default (gmatcher.py:383)
        m2(train_data(pairs, g, device="cuda"), mode="train")


def test_missed_percentile_window_repeats_the_build(synth_sd, monkeypatch):
    """The graph build predicts where the percentile threshold lies from a sample of the similarities and verifies the prediction on the device;
    a build that reports a miss (forced here by GIMS_AGC_WINDOW_SHIFT) is repeated with the flow that histograms every similarity, inside the
    same forward() -- the outputs equal those of an undisturbed call."""
    pair = synth.make_pair(2048, 777)
    m = GMatcher({}).eval()
    m.load_state_dict(synth_sd)
    m(pair_to_data(pair, 15, 2, 7, device="cuda"))               # (the first call of a model measures its attention layers at another precision)
    d0 = pair_to_data(pair, 15, 2, 7, device="cuda")
    ref = m(d0)
    assert getattr(m, "_agc_window_misses", 0) == 0
    monkeypatch.setenv("GIMS_AGC_WINDOW_SHIFT", "0.1")
    d1 = pair_to_data(pair, 15, 2, 7, device="cuda")
    out = m(d1)
    assert m._agc_window_misses == 1
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
        assert torch.equal(ref[k], out[k]), k
    assert d0["kept_kpts0_indices"] == d1["kept_kpts0_indices"] and d0["kept_kpts1_indices"] == d1["kept_kpts1_indices"]


def test_dense_keypoints_grow_the_graph_capacity(synth_sd):
    """Densely packed keypoints at the GMatcher DEFAULT radius / percentile (25 / 7: what train.py runs with, gmatcher.py:220-222)
    give ~100 neighbours per node -- more than the 64 directed edges per node the buffers start with.  The reference has no
    such limit; here the overflow flag makes the build repeat with larger buffers (kept for later calls) and the result
    equals the oracle's."""
    pair = synth.make_pair(600, 4242, canvas=(120, 90))
    m = GMatcher({}).eval()
    m.load_state_dict(synth_sd)
    assert m._edge_cap == 64
    d_gpu = pair_to_data(pair, 25, 7, 8, device="cuda")
    out = m(d_gpu)
    assert m._edge_cap > 64
    g0 = d_gpu["graph0"][0]
    assert g0.num_edges() > 64 * g0.num_nodes()
    d_cpu = pair_to_data(pair, 25, 7, 8, device="cpu")
    st = {}
    ref = O.gmatcher_forward(synth_sd, d_cpu, {}, stages=st)
    assert d_gpu["kept_kpts0_indices"] == d_cpu["kept_kpts0_indices"] and d_gpu["kept_kpts1_indices"] == d_cpu["kept_kpts1_indices"]
    assert g0.num_edges() == len(d_cpu["graph0"][0]["indices"])
    r0 = ref["matches0"][0].numpy()
    safe = safe_rows(st["ot"][0].numpy(), 0.2, r0, ref["matching_scores0"][0].numpy())
    np.testing.assert_array_equal(out["matches0"][0].cpu().numpy()[safe], r0[safe])
    np.testing.assert_allclose(out["matching_scores0"][0].cpu().numpy(), ref["matching_scores0"][0].numpy(), atol=1e-4)
    # the next call starts with the grown capacity: no second build
    out2 = m(pair_to_data(pair, 25, 7, 8, device="cuda"))
    np.testing.assert_array_equal(out2["matches0"].cpu().numpy(), out["matches0"].cpu().numpy())


@pytest.mark.parametrize("name", golden_names("trainloss_") + golden_names("binloss_"))
def test_train_loss_score_gradients_vs_reference_golden(name):
    """First stage of the backward pass: d loss / d scores and d loss / d bin_score from gims_sinkhorn_backward
    (reverse mode through the unrolled Sinkhorn iterations) against the reference's own autograd."""
    g = load_golden(name)
    pairs = train_pairs(name, g)
    m = GMatcher({"sinkhorn_iterations": int(g["meta"][4]), "pos_loss_weight": float(g["pos_loss_weight"]),
                  "neg_loss_weight": float(g["neg_loss_weight"])}).eval()
    m.load_state_dict(fixture_state_dict(g))
    out = m.loss_and_score_gradients(train_data(pairs, g, device="cuda"))
    np.testing.assert_allclose(float(out["loss"]), float(g["loss"]), atol=1e-4, rtol=0)
    ds = [d.cpu().numpy() for d in out["dscores"]]
    errs = []
    for b in range(len(pairs)):
        ref = g[f"dscores_{b}"] if f"dscores_{b}" in g else None
        if ref is not None:
            errs.append(float(np.abs(ds[b] - ref).max() / g[f"dscores_absmax_{b}"]))
    print(name, "relative gradient errors", errs, "dbin", float(out["dbin_score"]), float(g["dbin_score"]))
    check_score_gradients(g, ds, out["dbin_score"].cpu(), len(pairs), rtol=2e-3)
