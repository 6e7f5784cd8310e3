"""The Sinkhorn kernels at dustbin logits (bin_score, alpha) that compete with the scores, against float64.

Every other test and fixture sits at alpha ~ 1, far below the row maxima of the score matrix: there the start potentials
u0 = -max(alpha, row max) never take the alpha branch, the dustbin factors of the on-chip kernel barely grow, and the dustbin terms
of the reverse pass are small.  Here alpha is chosen relative to Z's own row maxima -- -2, the 10th / 50th / 90th percentile, above
every score (nothing matched) and far below every score -- and the forward solve (both paths, every streamed-kernel template, both
start-potential forms, the rescue path) and the reverse solve (low-rank and in-place forms, a ragged batch) are compared with
oracle/gims_oracle.py evaluated in float64."""
import functools

import numpy as np
import pytest
import torch

from oracle import gims_oracle as O
from tests.helpers import safe_rows

pytestmark = pytest.mark.gpu

# -2; the 10th / 50th / 90th percentile of the row maxima; above every score; so far above every score that exp(alpha - row max)
# leaves the f32 range (start potentials without alpha overflow); far below every score
ALPHA_TAGS = ("m2", "p10", "p50", "p90", "top", "far", "below")
IN_RANGE = ("p10", "p50", "p90")


@pytest.fixture(scope="module")
def hip():
    from gims_amd import hip as H
    H.load()
    return H


def _alpha(z, tag):
    """alpha relative to the row maxima of z (float32, like the bin_score parameter)."""
    rmax = z.max(1).astype(np.float64)
    v = {"m2": -2.0, "p10": np.percentile(rmax, 10), "p50": np.percentile(rmax, 50), "p90": np.percentile(rmax, 90),
         "top": float(z.max()) + 10.0, "far": float(z.max()) + 100.0, "below": float(z.min()) - 30.0}[tag]
    return float(np.float32(v))


@functools.lru_cache(maxsize=None)
def _problem(n, m, scale, seed):
    """Random scores with planted matches (a permutation's worth of strong cells), row maxima spread over ~4 sigma."""
    r = np.random.default_rng(seed)
    z = (r.normal(size=(n, m)) * scale).astype(np.float32)
    k = min(n, m)
    z[np.arange(k), r.permutation(m)[:k]] += np.float32(4 * scale)
    return z


@functools.lru_cache(maxsize=None)
def _oracle(n, m, scale, seed, alpha, iters):
    """(float64 log-OT, float32 log-OT) of the oracle."""
    z = _problem(n, m, scale, seed)
    r64 = O.log_optimal_transport(torch.from_numpy(z).double()[None], torch.tensor(alpha, dtype=torch.float64), iters)[0].numpy()
    r32 = O.log_optimal_transport(torch.from_numpy(z)[None], torch.tensor(alpha, dtype=torch.float32), iters)[0].numpy()
    return r64, r32


def _item(z):
    n, m = z.shape
    zs = torch.zeros((n, (m + 3) // 4 * 4), dtype=torch.float32, device="cuda")
    zs[:, :m] = torch.from_numpy(z).cuda()
    return dict(scores=zs, n=n, m=m, matches0=torch.empty(n, dtype=torch.int64, device="cuda"),
                matches1=torch.empty(m, dtype=torch.int64, device="cuda"), mscores0=torch.empty(n, device="cuda"),
                mscores1=torch.empty(m, device="cuda"), uv=torch.empty(n + m + 3, device="cuda"))


def _check_forward(hip, it, z, scale, seed, alpha, iters, thr=0.2):
    n, m = z.shape
    r64, r32 = _oracle(n, m, scale, seed, alpha, iters)
    full = hip.ot_matrix(it["scores"], n, m, alpha, it["uv"]).cpu().numpy().astype(np.float64)
    assert float(it["uv"][-1]) == 0.0, "status word"
    assert np.isfinite(full).all()
    own = float(np.abs(r32 - r64).max())
    bar = max(2.0 * own, 2e-4 * max(1.0, scale))
    err = float(np.abs(full - r64).max())
    assert err <= bar, f"log-OT err {err:.3e} > bar {bar:.3e} (f32 oracle's own error {own:.3e})"
    ref32 = torch.from_numpy(r32)[None]
    i0, _, s0, _ = O.select_matches(ref32, thr)
    i0, s0 = i0[0].numpy(), s0[0].numpy()
    safe = safe_rows(r64, thr, i0, s0)
    assert safe.mean() > 0.9, safe.mean()
    m0 = it["matches0"].cpu().numpy()
    np.testing.assert_array_equal(m0[safe], i0[safe])
    # (rtol: after 0 iterations the "scores" are exp(Z - norm), up to ~1e9)
    np.testing.assert_allclose(it["mscores0"].cpu().numpy()[safe], s0[safe], atol=1e-4, rtol=1e-6)
    return err, bar, int((m0 >= 0).sum())


def _solve(hip, items, alpha, iters, thr=0.2):
    probs = hip.make_ot_problems(items)
    work = torch.empty(hip.sinkhorn_workspace_bytes(probs), dtype=torch.uint8, device="cuda")
    hip.sinkhorn_match(probs, alpha, iters, thr, work)
    return probs


# streamed kernels: ot_iter_kernel<1,8> (m <= 4096), <2,4> (<= 8192), <4,2> (<= 16384), <8,1> (> 16384); iteration counts 0, 1, 20, 100
STREAMED = [(37, 53, 20, 3.0), (300, 280, 100, 4.0), (64, 70, 0, 3.0), (64, 70, 1, 3.0), (60, 5000, 20, 4.0), (24, 12000, 20, 4.0),
            (12, 17000, 5, 4.0)]
# on-chip kernel: XCD-local, chip-wide (n, m > 2048), tall / narrow, 2 x 2
ONCHIP = [(300, 280, 100, 4.0), (2300, 2100, 20, 4.0), (900, 130, 100, 4.0), (1024, 5, 20, 4.0), (2, 2, 100, 1.0)]


@pytest.mark.parametrize("tag", ALPHA_TAGS)
@pytest.mark.parametrize("n,m,iters,scale", STREAMED)
def test_streamed_forward_vs_float64(hip, monkeypatch, n, m, iters, scale, tag):
    monkeypatch.setenv("GIMS_OT_RESIDENT", "0")
    seed = n * 7919 + m
    z = _problem(n, m, scale, seed)
    alpha = _alpha(z, tag)
    it = _item(z)
    probs = _solve(hip, [it], alpha, iters)
    assert hip.sinkhorn_plan(probs, iters) == 0
    print(n, m, iters, tag, alpha, _check_forward(hip, it, z, scale, seed, alpha, iters))


@pytest.mark.parametrize("init", ["0", "1"])        # start potentials: the separate ot_init_kernel sweep / formed inside the on-chip kernel
@pytest.mark.parametrize("tag", ALPHA_TAGS)
@pytest.mark.parametrize("n,m,iters,scale", ONCHIP)
def test_onchip_forward_vs_float64(hip, monkeypatch, n, m, iters, scale, tag, init):
    """The on-chip kernel re-derives K when a dustbin factor has grown past fixed bounds calibrated at alpha = 1; at every alpha inside the
    row-max range no solve may give up and be re-solved by the rescue path (outside it the count is printed; the results are checked
    either way)."""
    monkeypatch.setenv("GIMS_OT_RESIDENT", "2")
    monkeypatch.setenv("GIMS_OT_R2_INIT", init)
    seed = n * 7919 + m
    z = _problem(n, m, scale, seed)
    alpha = _alpha(z, tag)
    before = hip.sinkhorn_rescues()
    it = _item(z)
    probs = _solve(hip, [it], alpha, iters)
    assert hip.sinkhorn_plan(probs, iters) > 0
    print(n, m, iters, tag, alpha, _check_forward(hip, it, z, scale, seed, alpha, iters), "rescued", hip.sinkhorn_rescues() - before)
    if tag in IN_RANGE:
        assert hip.sinkhorn_rescues() == before, "an on-chip solve gave up and was re-solved by the rescue path"


@pytest.mark.parametrize("rescue", ["0", "1"])      # the one-workgroup ot_rescue_kernel / the streamed kernels
@pytest.mark.parametrize("tag", ["p50", "far"])
def test_rescue_forward_vs_float64(hip, monkeypatch, tag, rescue):
    """GIMS_OT_FORCE_FAIL=1 (a software flag: the on-chip result is marked as given up) hands every problem to the rescue path, whose start
    potentials take max(alpha, row max) on their own."""
    monkeypatch.setenv("GIMS_OT_RESIDENT", "2")
    monkeypatch.setenv("GIMS_OT_FORCE_FAIL", "1")
    monkeypatch.setenv("GIMS_OT_RESCUE", rescue)
    shapes = [(300, 280, 4.0), (700, 650, 4.0)]
    zs = [_problem(n, m, s, n * 7919 + m) for n, m, s in shapes]
    alpha = _alpha(np.concatenate([z.max(1) for z in zs])[:, None], tag)      # one alpha for the batch, from every row maximum
    items = [_item(z) for z in zs]
    before = hip.sinkhorn_rescues()
    probs = _solve(hip, items, alpha, 30)
    assert hip.sinkhorn_plan(probs, 30) > 0
    assert hip.sinkhorn_rescues() - before == len(items)
    for (n, m, s), z, it in zip(shapes, zs, items):
        print(n, m, tag, alpha, _check_forward(hip, it, z, s, n * 7919 + m, alpha, 30))


# ----------------------------------------------------------------------------------------------------------------- reverse pass
POS_W, NEG_W = 0.45, 1.0


def _gt_rows(n, m, drop0, drop1, b, rng, z, plant):
    """Ground-truth rows (b, i0, i1) in ORIGINAL ids for a problem whose kept ids are range(n + len(drop0)) minus drop0 (same for
    image 1): positives on planted cells, (b, -1, -1), one side -1, ids that were not kept, and positives on cells whose log-OT falls
    below the loss's -100 clamp (planted far below their row)."""
    kept0 = np.setdiff1d(np.arange(n + len(drop0)), drop0)
    kept1 = np.setdiff1d(np.arange(m + len(drop1)), drop1)
    rows = []
    for i, j in plant[: max(4, len(plant) // 2)]:
        rows.append((b, int(kept0[i]), int(kept1[j])))
    for i, j in ((n - 1, m - 1), (n // 2, 0)):               # cells planted ~200 below their row: log-OT < -100
        rows.append((b, int(kept0[i]), int(kept1[j])))
    rows += [(b, -1, -1)] * 3
    rows += [(b, int(kept0[k]), -1) for k in rng.choice(n, min(n, 5), replace=False)]
    rows += [(b, -1, int(kept1[k])) for k in rng.choice(m, min(m, 5), replace=False)]
    rows += [(b, int(drop0[0]), int(kept1[0])), (b, int(kept0[0]), int(drop1[0]))]       # not kept: remapped to (b, -1, -1)
    return kept0, kept1, rows


def _reverse_problem(n, m, seed, scale=4.0):
    r = np.random.default_rng(seed)
    z = (r.normal(size=(n, m)) * scale).astype(np.float32)
    k = min(n, m)
    cols = r.permutation(m)[:k]
    z[np.arange(k), cols] += np.float32(4 * scale)
    z[n - 1, m - 1] = np.float32(z[n - 1].max() - 200.0)
    z[n // 2, 0] = np.float32(z[n // 2].max() - 200.0)
    plant = [(i, int(c)) for i, c in zip(range(k), cols) if (i, int(c)) not in ((n - 1, m - 1), (n // 2, 0))]
    return z, plant, r


def _reverse(hip, shapes, tag, iters, seed0=5):
    probs_np, kept, rows = [], [], []
    for b, (n, m) in enumerate(shapes):
        z, plant, r = _reverse_problem(n, m, seed0 + 31 * b + n * 7 + m)
        k0, k1, rw = _gt_rows(n, m, np.array([3, n + 1]), np.array([m // 3]), b, r, z, plant)
        probs_np.append(z)
        kept.append((k0, k1))
        rows += rw
    alpha = _alpha(np.concatenate([z.max(1) for z in probs_np])[:, None], tag)      # one alpha for the batch, from every row maximum
    # --- HIP: recorded forward, loss, reverse sweep
    items = [_item(z) for z in probs_np]
    gt = torch.tensor(rows, dtype=torch.int64, device="cuda")
    k0d = [torch.from_numpy(k0.astype(np.int32)).cuda() for k0, _ in kept]
    k1d = [torch.from_numpy(k1.astype(np.int32)).cuda() for _, k1 in kept]
    hists = hip.sinkhorn_history(items, alpha, iters)
    out3, _ = hip.train_loss(items, k0d, k1d, gt, alpha, POS_W, NEG_W)
    dsc, dbin = hip.sinkhorn_score_gradients(items, alpha, iters, POS_W, NEG_W, hip.train_loss.last, hists)
    # --- float64 autograd through the oracle, one problem at a time (the loss is the mean over the batch of per-pair means)
    B = len(shapes)
    grads, clamped = {}, [0, 0]
    for dt in (torch.float64, torch.float32):       # float64: the reference; float32: the oracle's own rounding error, for the bars
        a_leaf = torch.tensor(alpha, dtype=dt, requires_grad=True)
        losses, leaves = [], []
        with torch.enable_grad():
            for b, z in enumerate(probs_np):
                s_leaf = torch.from_numpy(z).to(dt).requires_grad_(True)
                ot = O.log_optimal_transport(s_leaf[None], a_leaf, iters)
                mine = [[0, i0, i1] for bb, i0, i1 in rows if bb == b]
                loss_b, _, _ = O.train_loss(ot, torch.tensor(mine, dtype=torch.int64), [kept[b][0]], [kept[b][1]], 1, POS_W, NEG_W)
                losses.append(loss_b)
                leaves.append(s_leaf)
                if dt == torch.float64:             # the cells the loss reads, beyond the clamp at 0 / at -100
                    o = ot[0].detach().numpy()
                    r0 = {int(v): i for i, v in enumerate(kept[b][0])}
                    r1 = {int(v): i for i, v in enumerate(kept[b][1])}
                    for _, i0, i1 in mine:
                        i, j = (r0[i0], r1[i1]) if i0 in r0 and i1 in r1 else (-1, -1)
                        clamped[0] += int(o[i, j] > 0)
                        clamped[1] += int(o[i, j] < -100)
            loss = sum(losses) / B
            loss.backward()
        grads[dt] = ([lf.grad.double().numpy() for lf in leaves], float(a_leaf.grad), float(loss))
    (ref_d, ref_bin, loss), (f32_d, f32_bin, _) = grads[torch.float64], grads[torch.float32]
    assert abs(float(out3[0]) - loss) <= 1e-4 * max(1.0, abs(loss)), (float(out3[0]), loss)
    for b in range(B):
        ref = ref_d[b]
        d = dsc[b].cpu().numpy().astype(np.float64)
        scale = float(np.abs(ref).max())
        # check_score_gradients' bars; where every score cell is clamped out of the loss (alpha far above the scores) the gradient is
        # ~1e-45, below float32's normal range, and the bar is twice the float32 oracle's own error instead
        bar = max(2e-3 * scale, 2.0 * float(np.abs(f32_d[b] - ref).max()))
        assert bar > 0
        err = float(np.abs(d - ref).max())
        assert err <= bar, (b, err, bar, scale)
        np.testing.assert_allclose(d.sum(1), ref.sum(1), atol=8 * bar, rtol=0)
        np.testing.assert_allclose(d.sum(0), ref.sum(0), atol=8 * bar, rtol=0)
    # d loss / d bin_score sums the border cells of dZc, which cancel: 2e-3 relative with a floor of 1e-3, or twice the
    # float32 oracle's own error where that is larger
    bin_bar = max(2e-3 * max(abs(ref_bin), 1e-3), 2.0 * abs(f32_bin - ref_bin))
    assert abs(float(dbin) - ref_bin) <= bin_bar, (float(dbin), ref_bin, f32_bin)
    return alpha, loss, ref_bin, f32_bin, clamped


# (not "far": there every score cell is clamped out of the loss, d loss / d bin_score is ~1e-14, and its float32 evaluation by the border-cell
# sum is cancellation noise -- measured up to 1e-5 on the HIP path, 2e-6 by the float32 oracle)
REV_TAGS = ("m2", "p50", "p90", "top")
# m + 1 in each bucket of the low-rank form's column-per-thread instances: <= 512, <= 1536, <= 2560, <= 4608
REV_SHAPES = [(200, 300), (150, 1200), (96, 2400), (64, 4500)]


@pytest.mark.parametrize("form", ["lowrank", "inplace"])
@pytest.mark.parametrize("tag", REV_TAGS)
@pytest.mark.parametrize("n,m", REV_SHAPES)
def test_reverse_vs_float64_autograd(hip, monkeypatch, n, m, tag, form):
    """gims_sinkhorn_backward (with gims_train_loss / gims_train_loss_grad in front) against float64 autograd through the oracle's unrolled
    Sinkhorn and loss: d loss / d scores at check_score_gradients' bars, d loss / d bin_score within 2e-3 relative (floor 1e-3).  The
    in-place form is forced with GIMS_OT_BWD_INPLACE=1 at the same shapes."""
    monkeypatch.setenv("GIMS_OT_BWD_INPLACE", "1" if form == "inplace" else "0")
    print(n, m, tag, form, _reverse(hip, [(n, m)], tag, 20))


@pytest.mark.parametrize("tag", REV_TAGS)
def test_reverse_inplace_by_iteration_count(hip, monkeypatch, tag):
    """More than 128 iterations: the low-rank buffers are not used, the in-place form runs on its own."""
    monkeypatch.delenv("GIMS_OT_BWD_INPLACE", raising=False)
    print(tag, _reverse(hip, [(120, 100)], tag, 150))


@pytest.mark.parametrize("tag", REV_TAGS)
def test_reverse_inplace_by_width(hip, monkeypatch, tag):
    """m + 1 > 4608: the in-place form with the generic (non-register) row kernel."""
    monkeypatch.delenv("GIMS_OT_BWD_INPLACE", raising=False)
    print(tag, _reverse(hip, [(24, 5000)], tag, 10))


@pytest.mark.parametrize("tag", REV_TAGS)
def test_reverse_ragged_batch(hip, monkeypatch, tag):
    """Three problems of different shapes in one call, one alpha, per-pair loss means averaged over the batch."""
    monkeypatch.delenv("GIMS_OT_BWD_INPLACE", raising=False)
    print(tag, _reverse(hip, [(90, 130), (200, 60), (33, 700)], tag, 20))


def test_reverse_reaches_both_clamp_edges(hip, monkeypatch):
    """The reverse problems above are not vacuous at the loss clamps: with a competitive dustbin, dustbin cells read by rows with one side -1
    sit above 0 (the row marginals of a finite solve are not exact), and the planted cells sit below -100."""
    monkeypatch.delenv("GIMS_OT_BWD_INPLACE", raising=False)
    for tag in ("m2", "p90"):
        clamped = _reverse(hip, [(200, 300)], tag, 20)[-1]
        print(tag, "cells read above 0 / below -100:", clamped)
        assert clamped[0] > 0 and clamped[1] >= 2, (tag, clamped)
