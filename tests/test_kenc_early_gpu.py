"""The keypoint encoder ahead of the graph build's read-back changes no arithmetic result, so every check here is bit equality -- against the
order it replaces, which stays reachable (GMatcher.kenc_early = False, GIMS_KENC_EARLY=0).

Shapes: GEMM rows 1, 31 and 257 (below a tile, an odd count, past a tile's edge) and 8320 / 49153 (the 128 x 128 and 256 x 256 tile instances) at
K = 256; batches in which the graph build drops keypoints -- 512 keypoints on 800 x 600 of which a few dozen are kept, and the 300-keypoint pair at
radius 15 / percentile 50 / min_size 5 that keeps most -- next to a pair that keeps all of its points; a repeated build; a pair that leaves the batch."""
import numpy as np
import pytest
import torch

from gims_amd import GMatcher, hip, synth
from tests.helpers import pair_to_data

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().cpu().view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def _operands(rows, k, n, seed):
    r = np.random.default_rng(seed)
    a = r.normal(size=(rows, k)).astype(np.float32)
    w = (r.normal(size=(n, k)) / np.sqrt(k)).astype(np.float32)
    b = r.normal(size=(n,)).astype(np.float32)
    return hip.split_spl32(_dev(a)), hip.split_spl32(_dev(w)), _dev(b)


# ------------------------------------------------------------------------------------------------ residual through a row index
@pytest.mark.parametrize("rows", [1, 31, 257, 8320, 49153])
def test_residual_rows_equals_gathered_residual(rows):
    """residual_rows: row r adds residual[residual_rows[r]] -- the bits of the launch on the gathered residual.  1, 31 and 257 rows take the
    64 x 64 tile, 8320 the 128 x 128 one, 49153 the 256 x 256 one (GraphSAGE's last layer at the headline size): each instance chunks the residual
    loads of its epilogue differently.  The residual has more rows than the launch, and the index is a random draw from them."""
    k, n, big = 256, 256, rows + 1500
    g = torch.Generator(device="cuda").manual_seed(rows)
    A = hip.split_spl32(torch.randn((rows, k), generator=g, device="cuda"))
    W = hip.split_spl32(torch.randn((n, k), generator=g, device="cuda") / 16)
    b = torch.randn((n,), generator=g, device="cuda")
    res = torch.randn((big, n), generator=g, device="cuda")
    idx = torch.randperm(big, generator=g, device="cuda")[:rows].to(torch.int32)
    kw = dict(bias=b, precision=hip.PREC_BF16X3, spl=True)
    got = hip.linear(A, W, residual=res, residual_rows=idx, out=torch.empty((rows, n), dtype=torch.float32, device="cuda"), **kw)
    want = hip.linear(A, W, residual=res[idx.long()].contiguous(), out=torch.empty((rows, n), dtype=torch.float32, device="cuda"), **kw)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(got), _bits(want))


def test_residual_rows_is_refused_where_it_would_be_ignored():
    """The one-launch MLP and the non-pre-split GEMMs take the same struct and do not read the index: they refuse it."""
    n = 256
    x = hip.split_spl32(torch.zeros((128, n), device="cuda"))
    w = hip.split_spl32(torch.zeros((3 * n, 2 * n), device="cuda"))
    out, spl = torch.empty((128, n), device="cuda"), torch.empty((128, 2 * n), dtype=torch.bfloat16, device="cuda")
    idx = torch.zeros(128, dtype=torch.int32, device="cuda")
    op = hip.op_mlp(x, x, w, torch.zeros(3 * n, device="cuda"), out, spl, residual=out)
    op.u.lin.residual_rows = idx.data_ptr()
    with pytest.raises(hip.GimsHipError, match="residual_rows"):
        hip.run_ops(hip.make_ops([op]))
    a = torch.zeros((4, 64), device="cuda")
    with pytest.raises(hip.GimsHipError, match="residual_rows"):
        hip.linear(a, torch.zeros((32, 64), device="cuda"), residual=torch.zeros((4, 32), device="cuda"), residual_rows=idx,
                   out=torch.empty((4, 32), device="cuda"))


def test_gemm_row_does_not_depend_on_the_rows_that_share_its_launch():
    """The early encoder runs its GEMMs over all input keypoints, the order behind the synchronisation over the kept ones: other row counts, so other
    tiles.  300 rows take the 64 x 64 tile, 8320 the 128 x 128 one, 49153 the 256 x 256 one (n = 256): the first 300 rows are the same bits."""
    g = torch.Generator(device="cuda").manual_seed(11)
    a = torch.randn((49153, 256), generator=g, device="cuda")
    w = torch.randn((256, 256), generator=g, device="cuda") / 16
    b = torch.randn((256,), generator=g, device="cuda")
    A, W = hip.split_spl32(a), hip.split_spl32(w)
    outs = [hip.linear(A[:m], W, bias=b, precision=hip.PREC_BF16X3, spl=True, act=hip.ACT_RELU)[:300] for m in (300, 8320, 49153)]
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(outs[0]), _bits(outs[1]))
    np.testing.assert_array_equal(_bits(outs[0]), _bits(outs[2]))


def test_kenc_first_over_whole_images_equals_per_row_index():
    """GIMS_AUX_KENC_FIRST with image starts (i[2] = n_img) against the per-row image index; images of 1, 7, 300 and 2 rows."""
    r = np.random.default_rng(3)
    ns = [1, 7, 300, 2]
    n, c1 = sum(ns), 32
    kpts = _dev((r.random((n, 2)) * 640).astype(np.float32))
    norm3 = _dev((r.random((len(ns), 3)) * 300 + 100).astype(np.float32))
    w1, b1 = _dev(r.normal(size=(c1, 2)).astype(np.float32)), _dev(r.normal(size=(c1,)).astype(np.float32))
    seg = _dev(np.repeat(np.arange(len(ns)), ns).astype(np.int32))
    starts = _dev(np.r_[0, np.cumsum(ns)][:-1].astype(np.int32))
    want = hip.kenc_first(kpts, norm3, seg, w1, b1, torch.empty((n, c1), dtype=torch.float32, device="cuda"))
    got = torch.full((n + 1, c1), -3.0, dtype=torch.float32, device="cuda")
    hip.run_ops(hip.make_ops([hip.op_aux(hip.AUX_KENC_FIRST, [kpts, norm3, starts, w1, b1, got], [c1, n, len(ns)])]))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(got[:n]), _bits(want))
    assert (got[n] == -3.0).all()


# ------------------------------------------------------------------------------------------------ encoder before the synchronisation
# "few": the input of test_sparse_graph_few_kept_vs_oracle -- 512 keypoints on 800 x 600 at 15 / 2 / 7, of which the build keeps a few dozen: the row index
# is far from the identity, most encoder rows go unread, the kept counts are below one tile.  "most": the input of the agc_n300_s2003_r15p50m5
# fixture (284 and 294 of 300 kept)
SPARSE = {"few": dict(n=512, seed=2000, canvas=(800, 600), graph=(15, 2, 7), below=200),
          "most": dict(n=300, seed=2003, canvas=(200, 150), graph=(15, 50, 5), below=300)}


def _batch(full_n=256, full_seed=1003, graph=(25, 7, 8), sparse="few"):      # (256, 1003) at 25 / 7 / 8: the e2e_n256_s1003_r25p7m8 input, which keeps all 256 + 256 points
    s = SPARSE[sparse]
    return [pair_to_data(synth.make_pair(s["n"], s["seed"], canvas=s["canvas"]), *s["graph"], device="cuda"),
            pair_to_data(synth.make_pair(full_n, full_seed), *graph, device="cuda")]


def _run(m, datas, early):
    """match_pairs with the encoder stage's outputs (desc, dpl) captured before the layers update them in place."""
    cap = {}
    orig = m._encoder

    def spy(P, G):
        sage, desc = orig(P, G)
        cap.update(desc=desc.clone(), dpl=m._act("dpl", G["n_tot"], 2 * m.config['descriptor_dim'], torch.bfloat16).clone(), early=G.get("early") is not None,
                   kept=[int(g["n_kept"]) for g in m._last_images])
        return sage, desc
    m._last_images = None
    gather = m._gather

    def spy_gather(ctx):
        G = gather(ctx)
        m._last_images = ctx["images"]
        return G
    m._encoder, m._gather, m.kenc_early = spy, spy_gather, early
    try:
        outs = m.match_pairs(datas, per_pair_graph=True)
        torch.cuda.synchronize()
    finally:
        del m._encoder, m._gather, m.kenc_early
    res = [(o["matches0"].cpu().numpy(), o["matching_scores0"].cpu().numpy(), o["mdesc0"].cpu().numpy()) for o in outs]
    return cap, res


@pytest.fixture(scope="module")
def settled(synth_sd):
    m = GMatcher({}).eval()
    m.load_state_dict(synth_sd)
    m(pair_to_data(synth.make_pair(256, 1002), 15, 2, 7, device="cuda"))       # 'auto' attention: the first call measures and decides
    return m


@pytest.mark.parametrize("sparse", list(SPARSE))
def test_encoder_before_the_synchronisation_is_bit_equal(settled, sparse):
    m = settled
    late, res_late = _run(m, _batch(sparse=sparse), early=False)
    early, res_early = _run(m, _batch(sparse=sparse), early=True)
    assert early["early"] and not late["early"]
    assert early["kept"] == late["kept"]
    below = SPARSE[sparse]["below"]
    assert 0 < early["kept"][0] < below and 0 < early["kept"][1] < below, ("the sparse pair was meant to drop points", early["kept"])
    assert early["kept"][2:] == [256, 256], "the other pair was meant to keep every point"
    np.testing.assert_array_equal(_bits(early["desc"]), _bits(late["desc"]))
    np.testing.assert_array_equal(_bits(early["dpl"]), _bits(late["dpl"]))
    for a, b in zip(res_early, res_late):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


def test_a_repeated_build_runs_the_early_encoder_again(settled, monkeypatch):
    """A build that reports a missed percentile window (forced by GIMS_AGC_WINDOW_SHIFT) is repeated: the early encoder of the first attempt is
    thrown away and enqueued again with the repeat -- the bits of the undisturbed call in the old order."""
    m = settled
    datas = lambda: [pair_to_data(synth.make_pair(700, 777), 15, 2, 7, device="cuda")]      # noqa: E731
    late, res_late = _run(m, datas(), early=False)
    misses = getattr(m, "_agc_window_misses", 0)
    monkeypatch.setenv("GIMS_AGC_WINDOW_SHIFT", "0.1")
    early, res_early = _run(m, datas(), early=True)
    assert m._agc_window_misses == misses + 1 and early["early"]
    np.testing.assert_array_equal(_bits(early["desc"]), _bits(late["desc"]))
    np.testing.assert_array_equal(_bits(early["dpl"]), _bits(late["dpl"]))
    for x, y in zip(res_early[0], res_late[0]):
        np.testing.assert_array_equal(x, y)


def test_a_pair_that_leaves_the_batch_behind_the_synchronisation(settled):
    """skip_empty (what a sweep's sub-batch runs with): pair 0 keeps nothing (no component reaches min_size) and leaves the batch after the early
    encoder ran over its keypoints too; pair 1's rows then start at 0 in the gathered arrays and at 2 x 300 in the encoder's."""
    m = settled
    runs = []
    for early in (False, True):
        pairs = [synth.make_pair(300, 2003, canvas=(200, 150)), synth.make_pair(256, 1003)]
        raw = [(_dev(p["keypoints" + s][0]), _dev(p["descriptors" + s][0]), _dev(p["scores" + s][0]), p["image" + s].shape) for p in pairs for s in "01"]
        m.kenc_early = early
        try:
            with hip.pinned_stream():
                ctx = m._run_build(m._ingest(raw), None, None, None, each=[(15, 50, 100000, False)] * 2 + [(25, 7, 8, False)] * 2)
                ctx.update(skip_empty=True, guards=True)
                out = m._run_rest(ctx)
            torch.cuda.synchronize()
        finally:
            del m.kenc_early
        assert out["dropped"] == [0] and len(out["items"]) == 1 and (out["sage"] is None) == early
        it = out["items"][0]
        runs.append([t.cpu().numpy() for t in (it["matches0"], it["mscores0"], it["matches1"], out["mdesc"])])
    for x, y in zip(*runs):
        np.testing.assert_array_equal(x, y)


def test_early_encoder_table_serves_two_batch_sizes(settled):
    """The table of the early encoder is patched per call like the one behind the synchronisation: another batch size through the same table, then
    the first batch again -- its bits come back, and each equals its launch-by-launch evaluation."""
    m = settled
    first, res_first = _run(m, _batch(), early=True)
    n_tables = len(m._kenc_cache)
    assert any(e[2] for e in m._kenc_cache.values()), "the early encoder did not replay its table"
    other, res_other = _run(m, _batch(200, 1001, (15, 2, 7), "most")[::-1], early=True)
    again, res_again = _run(m, _batch(), early=True)
    assert len(m._kenc_cache) <= n_tables + 1          # (the arena may have grown once: a new table then, not one per size)
    m.enable_timing(True, stepwise=True)
    try:
        step_first, _ = _run(m, _batch(), early=True)
        step_other, _ = _run(m, _batch(200, 1001, (15, 2, 7), "most")[::-1], early=True)
    finally:
        m.enable_timing(False)
    for got, want in ((again, first), (step_first, first), (step_other, other)):
        np.testing.assert_array_equal(_bits(got["desc"]), _bits(want["desc"]))
        np.testing.assert_array_equal(_bits(got["dpl"]), _bits(want["dpl"]))
    for a, b in zip(res_again, res_first):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


def test_a_gather_outside_run_rest_keeps_the_old_order(settled):
    """The training step gathers for an encoder of its own (gims_amd/trainstep.py): only _run_rest asks for the early encoder."""
    m = settled
    p = synth.make_pair(64, 1000)
    raw = [(_dev(p["keypoints" + s][0]), _dev(p["descriptors" + s][0]), _dev(p["scores" + s][0]), p["image" + s].shape) for s in "01"]
    G = m._gather(m._run_build(m._ingest(raw), 15, 2, 7))
    torch.cuda.synchronize()
    assert G is not None and G["early"] is None
