"""The largest row maximum that a measured bf16 attention launch reports, on every kernel and launch shape the launcher can choose.

attention_precision='auto' redoes a layer at f32-class accuracy when a head's largest softmax row maximum reaches 1/2, so that figure has to be
COMPLETE (no row with a maximum >= 1/2 may go unreported, wherever it sits and however short its key row is) and QUIET (a row that is merely
short, or moderately peaked below 1/2, must not raise it).  Checker: the float64 softmax of the STORED (bf16-rounded) operands.

Inputs: qkv ~ N(0, 0.5^2), 4 heads of 64: the logits of an unplanted row are N(0, 0.25^2), so at the shortest row (33 keys) a probability of 0.2
is 7.5 standard deviations out.  A planted row is Q[row, head] = g * K[key, head]; with g = 12 its float64 maximum is >= 0.99 while every
unplanted (row, head) stays below 0.2 -- both asserted on the reference before the device is looked at.  A shape's planted positions
share one launch, one per head, each in a different problem; the unplanted launch of the same data carries "all heads stay diffuse".
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

H, DH = 4, 64
P_FILL = 64                 # problems of a chip-filling launch: 4 heads x 64 = 256 groups, the launcher's threshold for the 8-wave kernel
N_KV = [33, 64, 65, 200, 300, 400, 448, 511, 512, 513, 1000]
# (n_q, n_kv): self-shaped, cross-shaped with n_q = 37 (not a multiple of 32 or 64), n_q < 32, and n_q with a last, partial 512-query block
SHAPES = [(n, n) for n in N_KV] + [(37, n) for n in N_KV] + [(20, 33), (20, 300), (20, 511), (513, 200), (1000, 300), (513, 448), (1000, 511), (513, 1000)]
FORCED = {"4wave": ("1", None, "wave4"), "4wave2": ("2", None, "wave4"), "split": ("3", "2", "split"), "split4": ("3", "4", "split")}


@pytest.fixture(scope="module")
def hip():
    from gims_amd import hip as hp
    hp.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return hp


@functools.lru_cache(maxsize=2)
def _base(n_q, n_kv, n_prob):
    """The unplanted operands of a shape as f32 and the problem table.  n_q == n_kv: self-shaped as in the model (a problem's queries and keys are
    the same rows); otherwise cross-shaped (a problem's query rows, then its key rows)."""
    r = np.random.default_rng(1000 * n_q + n_kv)
    per, kofs = (n_q, 0) if n_q == n_kv else (n_q + n_kv, n_q)
    qkv = r.standard_normal(size=(n_prob * per, 3 * H * DH), dtype=np.float32) * np.float32(0.5)
    probs = [(i * per, n_q, i * per + kofs, n_kv) for i in range(n_prob)]
    return qkv, probs


def _sampled(n_q):
    n_s = min(32, n_q)
    return set(int(j * n_q // n_s) for j in range(n_s))


def _positions(n_q, n_kv, n_prob):
    """One planted (problem, query, key) per head: a query outside the 32-query sample, the last query, a query of the second 32-query plane of a
    wave, a query of the last (partial) 512-query block -- against the first key, the last key (inside a partial key tile) and the two keys at
    a half-tile boundary."""
    free = [q for q in range(n_q) if q not in _sampled(n_q)] or list(range(n_q))            # n_q <= 32: every query is sampled
    plane2 = [q for q in free if q % 64 >= 32] or [q for q in range(n_q) if q % 64 >= 32] or free
    last_block = [q for q in free if q >= 512 * ((n_q - 1) // 512)]
    return [(0, free[0], 0),
            (n_prob - 1, n_q - 1, n_kv - 1),
            (17 % n_prob, plane2[-1], 31),
            (40 % n_prob, last_block[len(last_block) // 2], 32)]


def _stored(x):
    """f32 -> the bf16 tensor the kernel reads."""
    return torch.from_numpy(x).to(torch.bfloat16)


def _row_pmax(fq, fk):
    """float64 softmax row: stored query [64] against stored keys [n_kv, 64] -> probabilities."""
    s = fk @ fq / 8.0
    p = np.exp(s - s.max())
    return p / p.sum()


def _f64(t):
    return t.float().numpy().astype(np.float64)


def _plant(qkv, scale, probs, plant, head, make_row, lo, hi, bisect):
    """Writes Q[row, head] = make_row(stored keys of the head, g) (times the softmax scale when Q is prescaled) and returns the float64 row
    maximum of the STORED row, asserted to lie in [lo, hi].  bisect: g is searched in [0, 16] for that; otherwise g = 12."""
    p, row, _ = plant
    qo, _, ko, nk = probs[p]
    fk = _f64(_stored(qkv[ko:ko + nk, 256 + head * DH:256 + (head + 1) * DH]))
    g_lo, g_hi = 0.0, 16.0
    for _ in range(40 if bisect else 1):
        g = 0.5 * (g_lo + g_hi) if bisect else 12.0
        qrow = (make_row(fk, g) * scale).astype(np.float32)
        pm = _row_pmax(_f64(_stored(qrow)) / scale, fk).max()
        if lo <= pm <= hi:
            break
        g_lo, g_hi = (g, g_hi) if pm < lo else (g_lo, g)
    assert lo <= pm <= hi, f"the construction failed: row maximum {pm} outside [{lo}, {hi}]"
    qkv[qo + row, head * DH:(head + 1) * DH] = qrow
    return pm


def _all_rows_reference(q16, probs, scale):
    """float64 softmax attention of the stored operands for every problem (equal sizes: one batch), on the device in torch.float64:
    the row maxima [P, H, n_q] and the output [P, n_q, 256]."""
    f = q16.cuda().double()
    qo, nq, ko, nk = probs[0]
    n_prob = len(probs)
    blk = f.view(n_prob, -1, 3 * H * DH)
    q = blk[:, :nq, 0:256].reshape(n_prob, nq, H, DH) / scale
    k = blk[:, ko - qo:, 256:512].reshape(n_prob, nk, H, DH)
    v = blk[:, ko - qo:, 512:768].reshape(n_prob, nk, H, DH)
    s = torch.einsum("pqhd,pkhd->phqk", q, k) / 8.0
    pr = torch.softmax(s, dim=-1)
    out = torch.einsum("phqk,pkhd->pqhd", pr, v).reshape(n_prob, nq, H * DH)
    return pr.amax(dim=-1).cpu().numpy(), out.cpu().numpy(), float(v.abs().max())


def _launch(hip, q16, probs, n_q, prescaled):
    pr = torch.tensor(probs, dtype=torch.int32, device="cuda")
    out = torch.full((q16.shape[0], H * DH), float("nan"), dtype=torch.float32, device="cuda")
    stat = torch.zeros((H + 1, 4), dtype=torch.int64, device="cuda")
    hip.attention_launch_counts(reset=True)
    hip.attention(q16.cuda(), pr, n_q, H, out, q_prescaled=prescaled, stat=stat)
    return stat, out.cpu().numpy(), hip.attention_launch_counts()


_GUARD_OPERANDS = {}


def _guard_fires(hip, stat, max_thr):
    """A projection behind a guard on `stat` (mean / tail thresholds of the model): did it run?"""
    if not _GUARD_OPERANDS:
        r = np.random.default_rng(5)
        _GUARD_OPERANDS["x"] = hip.split_spl32(torch.from_numpy(r.normal(size=(128, 256)).astype(np.float32)).cuda())
        _GUARD_OPERANDS["w"] = hip.split_spl32(torch.from_numpy((r.normal(size=(768, 256)) / 16.0).astype(np.float32)).cuda())
    g = hip.attn_guard(stat, hip.GUARD_PEAKED, H, mean_thr=0.08, tail_thr=0.02, max_thr=max_thr)
    qkv6 = torch.full((128, 1536), 0x7fc0, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    hip.linear(_GUARD_OPERANDS["x"], _GUARD_OPERANDS["w"], out_split=qkv6, precision=hip.PREC_BF16X3, spl=True, guard=g)
    return bool((qkv6.view(torch.int16) != 0x7fc0).any())


def _check_output(o, probs, ref_out, vmax, skip=()):
    """The attention output against float64 at the bf16 tolerance of test_attention; `skip`: (problem, query, head) whose reference is not in ref_out."""
    for p, (qo, nq, ko, nk) in enumerate(probs):
        got = o[qo:qo + nq].copy()
        want = ref_out[p].copy()
        for sp, row, head in skip:
            if sp == p:
                got[row, head * DH:(head + 1) * DH] = want[row, head * DH:(head + 1) * DH]
        assert np.isfinite(got).all()
        err = np.abs(got - want).max()
        assert err < 1.5e-2 * max(1.0, vmax / 4), f"attention err {err:.3e} (problem {p})"
        if ko != qo:
            assert np.isnan(o[ko:ko + nk]).all()                                    # rows that are not queries are untouched


def _run_case(hip, n_q, n_kv, n_prob, prescaled, want_kernel):
    scale = float(hip.ATTN_Q_SCALE) if prescaled else 1.0
    base, probs = _base(n_q, n_kv, n_prob)
    qkv = base.copy()
    if prescaled:
        qkv[:, :256] *= np.float32(scale)
    mx_scale = hip.ATTN_STAT_SCALE

    # ---- nothing planted: the reference is diffuse everywhere, every head stays below 1/2 and the guard is idle
    q16 = _stored(qkv)
    ref_pmax, ref_out, vmax = _all_rows_reference(q16, probs, scale)
    assert ref_pmax.max() < 0.2, ref_pmax.max()                                     # (about 0.1 at 33 keys, 0.02 from 200 keys up)
    stat, o, counts = _launch(hip, q16, probs, n_q, prescaled)
    assert counts[want_kernel] == 1 and sum(counts.values()) == 1, counts
    mx = stat.cpu().numpy()[:H, 2] / mx_scale
    print(f"[{want_kernel} n_q={n_q} n_kv={n_kv} prescaled={prescaled}] unplanted max {mx}")
    assert (mx < 0.5).all(), mx
    assert not _guard_fires(hip, stat, 0.5)
    _check_output(o, probs, ref_out, vmax)

    def planted_launch(lo, hi, make_row_for, bisect, check):
        """Plants one row per head, launches, and hands (reported maxima, float64 maxima, statistic) to `check`."""
        x = qkv.copy()
        plants = _positions(n_q, n_kv, n_prob)
        truth = np.array([_plant(x, scale, probs, plants[h], h, make_row_for(plants[h]), lo, hi, bisect) for h in range(H)])
        x16 = _stored(x)
        st, oo, cnt = _launch(hip, x16, probs, n_q, prescaled)
        assert cnt[want_kernel] == 1 and sum(cnt.values()) == 1, cnt
        got = st.cpu().numpy()[:H, 2] / mx_scale
        print(f"[{want_kernel} n_q={n_q} n_kv={n_kv} prescaled={prescaled}] target [{lo}, {hi}] at {plants}: truth {truth} reported {got}")
        check(got, truth, st)
        # the planted rows' own output against their own float64 row, every other row against the unplanted reference (only Q rows were changed)
        for h, (p, row, _) in enumerate(plants):
            qo, _, ko, nk = probs[p]
            f = _f64(x16[ko:ko + nk])
            pm = _row_pmax(_f64(x16[qo + row, h * DH:(h + 1) * DH]) / scale, f[:, 256 + h * DH:256 + (h + 1) * DH])
            want = pm @ f[:, 512 + h * DH:512 + (h + 1) * DH]
            err = np.abs(oo[qo + row, h * DH:(h + 1) * DH] - want).max()
            assert err < 1.5e-2 * max(1.0, vmax / 4), f"planted row {plants[h]}: output err {err:.3e}"
        _check_output(oo, probs, ref_out, vmax, skip=[(p, row, h) for h, (p, row, _) in enumerate(plants)])

    def one_key(plant):
        return lambda fk, g: g * fk[plant[2]]

    def two_keys(plant):
        """Logits (L, L - 0.25) with L = 20 on two keys of different half tiles -- the first and the last key, or the two sides of the boundary
        31 | 32 -- and next to nothing elsewhere: the pair shares the mass 56 : 44."""
        k1, k2 = (0, n_kv - 1) if plant[2] in (0, n_kv - 1) else (31, 32)

        def make_row(fk, g):
            a, b = fk[k1], fk[k2]
            return np.linalg.solve(np.array([[a @ a, a @ b], [a @ b, b @ b]]), 8.0 * np.array([20.0, 19.75])) @ np.stack([a, b])
        return make_row

    # ---- completeness: a one-hot row is reported from wherever it sits, and the guard fires on it (and only through max_thr)
    def complete(got, truth, st):
        assert (got >= 0.5).all() and (got >= truth - 1e-3).all(), (got, truth)
        assert _guard_fires(hip, st, 0.5) and not _guard_fires(hip, st, 0.0)
    planted_launch(0.99, 1.0, one_key, False, complete)

    # ---- a moderately peaked row, and a row whose mass sits on two keys of different half tiles: still reported
    def reported(got, truth, st):
        assert (got >= 0.5).all(), (got, truth)
    planted_launch(0.65, 0.85, one_key, True, reported)
    planted_launch(0.5, 0.6, two_keys, False, reported)

    # ---- no false alarm: rows with a maximum of 0.2 .. 0.3 leave every head below 1/2
    def quiet(got, truth, st):
        assert (got < 0.5).all(), (got, truth)
        assert not _guard_fires(hip, st, 0.5)
    planted_launch(0.2, 0.3, one_key, True, quiet)


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("n_q,n_kv", SHAPES)
def test_rowmax_is_complete_and_quiet_in_chip_filling_launches(hip, n_q, n_kv, prescaled):
    """64 problems x 4 heads: the launcher takes the 8-wave kernel by itself.  Its optimistic softmax tracks no maximum; every query contributes an
    upper bound of its row maximum (its largest half-tile mass), and where that is too coarse -- rows of fewer than 512 keys -- the exact figure."""
    _run_case(hip, n_q, n_kv, P_FILL, prescaled, "wave8")


@pytest.mark.parametrize("n_kv", [33, 300, 511, 513])
@pytest.mark.parametrize("kernel", sorted(FORCED))
def test_rowmax_is_complete_and_quiet_on_the_running_maximum_kernels(hip, monkeypatch, kernel, n_kv):
    """The other kernels the launcher can choose (forced as in test_attention) track a running maximum and report every row exactly."""
    qp, split, name = FORCED[kernel]
    monkeypatch.setenv("GIMS_ATTN_QP", qp)
    if split:
        monkeypatch.setenv("GIMS_ATTN_SPLIT", split)
    _run_case(hip, n_kv, n_kv, 8, True, name)
    _run_case(hip, 37, n_kv, 8, False, name)
