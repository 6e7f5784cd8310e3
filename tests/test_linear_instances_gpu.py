"""Every GEMM launch instance of gims_amd/csrc/linear.hip and linear6.hip at its tile seams, with canaries around every output window.

The launch census (hip.linear_launch_counts) says which kernel instance served a launch, so every case asserts that it reached the instance it
is meant to pin.  References and layouts are the plain restatements of tests/linear_ref.py (float64 products, the header's definitions of the
bf16 planes); every tolerance is one the project already asserts for the same kernel family and is cited where it is used.  Each test prints
its worst err / bar.

Compiled but not reached here: the instances that only GIMS_X3P_TILE, GIMS_X3P_QKV=0|2 or GIMS_X3P_SMALL select (the launcher reads these once
per process): x3p_256x128_w8_s2_hi and x3p_256x256_w8_s4_hi."""
import ctypes

import numpy as np
import pytest
import torch

from tests import linear_ref as R
from tests.helpers import compare_with_golden, golden_names, load_golden, pair_to_data

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

BAR_X3 = 4e-5            # test_linear / test_linear_presplit: three bf16 MFMAs per product, of the error scale
BAR_F32 = 2e-6           # test_linear (f32), test_linear_presplit_hi_only, test_linear_bf16x6: f32 roundoff class, of the error scale
BAR_ONE_PASS = 2.0 ** -7   # test_linear_presplit_hi_only: a hi-only launch against the UNROUNDED product


@pytest.fixture(scope="module")
def hip():
    from gims_amd import hip as H
    H.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return H


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _canary(shape, bits16=False):
    """A device buffer full of the canary: float32, or bfloat16 for the 16-bit outputs."""
    if bits16:
        return torch.full(shape, R.CANARY_16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return torch.full(shape, R.CANARY_F32, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    """Device tensor -> host array of its bit patterns (uint32 / uint16)."""
    if t.element_size() == 4:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _f32(bits):
    return bits.view(np.float32)


def _only(counts):
    return {k: v for k, v in counts.items() if v}


def _pitched_spl32(hip, x, pitch):
    """SPL32 image of x [rows, k] as a view into a wider buffer of row pitch `pitch` whose surplus columns hold the canary."""
    rows, k = x.shape
    buf = _canary((rows, pitch), bits16=True)
    view = buf[:, :2 * k]
    hip.split_spl32(_dev(x), out=view)
    return view


# ================================================================================================ 2. pre-split instances
def _presplit_case(m, n, k, k0, seed):
    r = np.random.default_rng(seed)
    a = r.normal(size=(m, k)).astype(np.float32)
    a[3, 5] = 321.5                                   # a transposed or shifted operand cannot hide
    w = (r.normal(size=(n, k)) / np.sqrt(k)).astype(np.float32)
    bias = r.normal(size=n).astype(np.float32)
    res = r.normal(size=(m, n)).astype(np.float32)
    return a, w, bias, res


@pytest.mark.parametrize("k,k0", [(32, 32), (160, 64)])      # one stage (fewer than any ring holds) / five stages, the longer segment second
@pytest.mark.parametrize("kind,m,n,hi_only", R.INSTANCE_TABLE, ids=[row[0] for row in R.INSTANCE_TABLE])
def test_presplit_instance(hip, kind, m, n, hi_only, k, k0):
    """One pre-split instance, reached by shape alone: census, values against float64, the 16-bit and split outputs bit for bit against the
    header's definitions applied to the launch's own f32 output, every pad row and pad column of every output, and a repeat."""
    a, w, bias, res = _presplit_case(m, n, k, k0, seed=m * 3 + n + k)
    # operands are views into wider buffers: pitches 2 k0 + 64, 2 (K - k0) + 128 and 2 K + 64
    A0 = _pitched_spl32(hip, a[:, :k0], 2 * k0 + 64)
    A1 = _pitched_spl32(hip, a[:, k0:], 2 * (k - k0) + 128) if k0 < k else None
    W = _pitched_spl32(hip, w, 2 * k + 64)
    Bias, Res = _dev(bias), _dev(res)
    flags = hip.LINEAR_HI_ONLY if hi_only else 0
    ld_split = 2 * R.ceil_to(n, 32) + 64
    PAD_ROWS = 3

    def launch(pitch16, f16=False):
        out = _canary((m + PAD_ROWS, n + 12))
        out[:m, :n] = Res                                            # the residual aliases the f32 output
        o16 = _canary((m + PAD_ROWS, pitch16), bits16=True)
        osp = _canary((m + PAD_ROWS, ld_split), bits16=True)
        hip.linear_launch_counts(reset=True)
        hip.linear(A0, W, a1=A1, spl=True, n=n, bias=Bias, residual=out[:m, :n], out=out[:m, :n], out_bf16=o16[:m, :n],
                   out_split=osp[:m, :2 * R.ceil_to(n, 32)], act=hip.ACT_RELU, precision=hip.PREC_BF16X3, scale=0.5,
                   flags=flags | (hip.LINEAR_OUT_F16 if f16 else 0))
        torch.cuda.synchronize()
        assert _only(hip.linear_launch_counts()) == {kind: 1}
        return _bits(out), _bits(o16), _bits(osp)

    def check_outputs(got, f16=False):
        ob, o16, osp = got
        what = f"{kind} {m}x{n}x{k}"
        R.assert_pad_intact(ob, m, n, what + " f32")
        R.assert_pad_intact(o16, m, n, what + " 16-bit")
        R.assert_pad_intact(osp, m, ld_split, what + " split", written_cols=R.spl32_written(n, ld_split))
        o = _f32(ob[:m, :n])
        np.testing.assert_array_equal(o16[:m, :n], R.f16_sat_bits(o) if f16 else R.bf16_bits(o))
        hi, lo = R.split2(o)
        cols = R.spl_col(np.arange(n))
        np.testing.assert_array_equal(osp[:m, cols], hi)
        np.testing.assert_array_equal(osp[:m, cols + 32], lo)
        return o

    first = launch(n + 4)                    # a multiple of 8 for these n: the 16-byte store of the 16-bit output
    assert (n + 4) % 8 == 0
    o = check_outputs(first)
    if hi_only:
        ah, wh = R.bf16_value(R.bf16_bits(a)), R.bf16_value(R.bf16_bits(w))
        ref, sc = R.linear_ref(ah, wh, bias, res, scale=0.5, relu=True)
        worst = float((np.abs(o - ref) / sc).max()) / BAR_F32
        full, _ = R.linear_ref(a, w, bias, res, scale=0.5, relu=True)
        one_pass = float((np.abs(o - full) / sc).max()) / BAR_ONE_PASS
        print(f"{kind} K={k}: worst err/bar {worst:.3f} (rounded operands), {one_pass:.3f} (unrounded, one-pass bar)")
        # ... and it IS one pass: rounding the planted 321.5 to bf16 (322) alone moves row 3 by about 1.5e-3 of its scale, far above what
        # the three-pass product leaves
        assert BAR_X3 / BAR_ONE_PASS < one_pass < 1.0
    else:
        ref, sc = R.linear_ref(a, w, bias, res, scale=0.5, relu=True)
        err = np.abs(o - ref) / sc
        worst = float(err.max()) / BAR_X3
        print(f"{kind} K={k}: worst err/bar {worst:.3f} at {np.unravel_index(err.argmax(), err.shape)}")
    assert np.isfinite(o).all() and worst < 1.0
    second = launch(n + 8)                   # not a multiple of 8: the 8-byte stores
    check_outputs(second)
    np.testing.assert_array_equal(second[0], first[0])
    np.testing.assert_array_equal(second[2], first[2])
    np.testing.assert_array_equal(second[1][:m, :n], first[1][:m, :n])
    again = launch(n + 4)                    # the first launch once more: the same bits
    for x, y in zip(again, first):
        np.testing.assert_array_equal(x, y)
    if n == 516:
        check_outputs(launch(n + 4, f16=True), f16=True)


def test_presplit_rows_are_the_same_bits_in_every_full_product_instance(hip):
    """'Same K order per output element: bit-identical': rows [:129] of the 3329-row (128 x 128 on eight waves), 6529-row (on four waves) and
    16129-row (256 x 256) launches equal the 129-row launch (64 x 64) bit for bit, at a ragged n = 516 and K = 160 in two segments."""
    n, k, k0 = 516, 160, 64
    a, w, bias, _ = _presplit_case(16129, n, k, k0, seed=77)
    A0, A1, W = _pitched_spl32(hip, a[:, :k0], 2 * k0 + 64), _pitched_spl32(hip, a[:, k0:], 2 * (k - k0) + 128), _pitched_spl32(hip, w, 2 * k + 64)
    Bias = _dev(bias)
    outs = {}
    for m in (129, 3329, 6529, 16129):
        out = _canary((m + 1, n + 12))
        hip.linear_launch_counts(reset=True)
        hip.linear(A0[:m], W, a1=A1[:m], spl=True, n=n, bias=Bias, out=out[:m, :n], act=hip.ACT_RELU, precision=hip.PREC_BF16X3, scale=0.5)
        torch.cuda.synchronize()
        assert _only(hip.linear_launch_counts()) == {R.x3p_instance(m, n)[0]: 1}
        bits = _bits(out)
        R.assert_pad_intact(bits, m, n, f"{m} rows")
        outs[m] = bits[:129, :n]
    for m in (3329, 6529, 16129):
        np.testing.assert_array_equal(outs[m], outs[129], err_msg=f"{m}-row launch")


# ================================================================================================ 3. register-staged kernels
def _staged_problems(hip, prec, seed):
    """The five problems of the batch-against-single test with fresh, canaried outputs: a list of dicts (a0, w, kw for hip.linear_args /
    hip.linear, the host operands, the padded output buffers)."""
    r = np.random.default_rng(seed)
    x3 = prec == hip.PREC_BF16X3
    shapes = [(300, 260, 128, 64, "relu_res_bf16"), (77, 100, 128, 128, "scaled"), (1, 513, 64, 64, "only16"), (129, 1, 64, 64, "split"),
              (260, 260, 64, 64, "upper")]
    out = []
    for (m, n, k, k0, epi) in shapes:
        a = r.normal(size=(m, k)).astype(np.float32)
        if m > 3:
            a[3, 5] = 321.5
        w = a.copy() if epi == "upper" else (r.normal(size=(n, k)) / np.sqrt(k)).astype(np.float32)
        A = _dev(a)
        a0, a1 = (A[:, :k0], A[:, k0:]) if k0 < k else (A, None)
        kw = dict(a1=a1, precision=prec, n=n)
        Wd = _dev(w)
        if x3:
            wh, wl = hip.split_bf16(Wd)
            Wop, kw["w_lo"] = wh, wl
        else:
            Wop = Wd
        p = dict(m=m, n=n, k=k, a=a, w=w, epi=epi, a0=a0, w_op=Wop, bias=None, res=None, scale=1.0, relu=False, keep=(A, Wd))
        o32 = _canary((m + 3, n + 12))
        if epi == "relu_res_bf16":
            p["bias"], p["res"], p["relu"] = r.normal(size=n).astype(np.float32), r.normal(size=(m, n)).astype(np.float32), True
            o32[:m, :n] = _dev(p["res"])
            p["o16"] = _canary((m + 3, n + 5), bits16=True)
            kw.update(bias=_dev(p["bias"]), residual=o32[:m, :n], out=o32[:m, :n], out_bf16=p["o16"][:m, :n], act=hip.ACT_RELU)
        elif epi == "scaled":
            p["scale"] = 0.5
            kw.update(out=o32[:m, :n], scale=0.5)
        elif epi == "only16":
            p["bias"] = r.normal(size=n).astype(np.float32)
            p["o16"] = _canary((m + 3, n + 5), bits16=True)
            kw.update(bias=_dev(p["bias"]), out_bf16=p["o16"][:m, :n])
            o32 = None
        elif epi == "split":
            p["bias"] = r.normal(size=n).astype(np.float32)
            p["osp"] = _canary((m + 3, 2 * R.ceil_to(n, 32) + 64), bits16=True)
            kw.update(bias=_dev(p["bias"]), out=o32[:m, :n], out_split=p["osp"][:m, :2 * R.ceil_to(n, 32)])
        else:
            p["scale"] = 0.5
            kw.update(out=o32[:m, :n], scale=0.5, flags=hip.LINEAR_UPPER)
        p["o32"], p["kw"] = o32, kw
        out.append(p)
    return out


def _staged_bits(p):
    return {key: _bits(p[key]) for key in ("o32", "o16", "osp") if p.get(key) is not None}


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_register_staged_batch_equals_single(hip, prec):
    """linear_f32_batch_kernel / linear_bf16x3_batch_kernel: five problems of different shapes, K and epilogues in ONE launch whose grid is
    sized for the largest.  Census; every problem against float64 at test_linear's bars; every problem bit-equal to the same arguments sent
    alone through hip.linear (one body function serves both kernels); every canary, so the surplus workgroups of the small problems stored
    nothing; GIMS_LINEAR_UPPER promises the strict upper triangle, the rest is within the bar or untouched."""
    P = hip.PREC_F32 if prec == "f32" else hip.PREC_BF16X3
    bar = BAR_F32 if prec == "f32" else BAR_X3
    batch = _staged_problems(hip, P, seed=31)
    dev_args = torch.empty(ctypes.sizeof(hip.LinearArgs) * len(batch), dtype=torch.uint8, device="cuda")
    hip.linear_launch_counts(reset=True)
    hip.linear_batch([hip.linear_args(p["a0"], p["w_op"], **p["kw"]) for p in batch], dev_args, P)
    torch.cuda.synchronize()
    assert _only(hip.linear_launch_counts()) == {prec + "_batch": 1}
    single = _staged_problems(hip, P, seed=31)
    hip.linear_launch_counts(reset=True)
    for p in single:
        hip.linear(p["a0"], p["w_op"], **p["kw"])
    torch.cuda.synchronize()
    assert _only(hip.linear_launch_counts()) == {prec: len(single)}
    worst = 0.0
    for pb, ps in zip(batch, single):
        m, n, what = pb["m"], pb["n"], f"{prec} {pb['epi']} {pb['m']}x{pb['n']}"
        got, alone = _staged_bits(pb), _staged_bits(ps)
        for key in got:
            np.testing.assert_array_equal(got[key], alone[key], err_msg=f"{what}: {key} differs between the batch and the single launch")
        ref, sc = R.linear_ref(pb["a"], pb["w"], pb["bias"], pb["res"], scale=pb["scale"], relu=pb["relu"])
        if "o32" in got:
            R.assert_pad_intact(got["o32"], m, n, what + " f32")
            o = _f32(got["o32"][:m, :n])
            ratio = np.abs(o - ref) / sc / bar
            if pb["epi"] == "upper":
                strict = np.triu(np.ones((m, n), dtype=bool), 1)
                untouched = R.is_canary(got["o32"][:m, :n])
                assert not untouched[strict].any() and (ratio[strict] < 1.0).all(), what
                assert (untouched | (ratio < 1.0))[~strict].all(), f"{what}: an element outside the strict upper triangle is neither right nor untouched"
                ratio = ratio[~untouched]
            assert np.isfinite(ratio).all() and ratio.max() < 1.0, f"{what}: {ratio.max():.3f} of the bar"
            worst = max(worst, float(ratio.max()))
        if "o16" in got:
            R.assert_pad_intact(got["o16"], m, n, what + " 16-bit")
            v = R.bf16_value(got["o16"][:m, :n]).astype(np.float64)
            if "o32" in got:                   # the side output is the rounded f32 output
                np.testing.assert_array_equal(got["o16"][:m, :n], R.bf16_bits(_f32(got["o32"][:m, :n])))
            else:                              # test_linear's bar for a 16-bit output: bf16 rounding (2^-8 relative) plus the f32 error
                excess = np.abs(v - ref) - (np.abs(ref) * 2.0 ** -8 + sc * bar)
                assert np.isfinite(v).all() and excess.max() <= 0, f"{what}: exceeds bf16 rounding + f32 error by {excess.max():.3e}"
        if "osp" in got:
            ld = got["osp"].shape[1]
            R.assert_pad_intact(got["osp"], m, ld, what + " split", written_cols=R.spl32_written(n, ld))
            hi, lo = R.split2(_f32(got["o32"][:m, :n]))
            cols = R.spl_col(np.arange(n))
            np.testing.assert_array_equal(got["osp"][:m, cols], hi)
            np.testing.assert_array_equal(got["osp"][:m, cols + 32], lo)
    print(f"register-staged {prec} batch: worst err/bar {worst:.3f}")


@pytest.mark.parametrize("name", golden_names("e2e_n256")[:1])      # one small fixture is enough to pin the kernel
def test_score_matrix_on_the_f32_batch_kernel(hip, monkeypatch, synth_sd, name):
    """GIMS_SCORE_PREC=f32: the score matrix of a forward() runs on linear_f32_batch_kernel instead of the six-pass kernel, and the fixture's
    own bars hold."""
    from gims_amd import GMatcher, synth
    g = load_golden(name)
    n, seed, rad, pct, ms, iters = [int(x) for x in g["meta"]]
    m = GMatcher({"sinkhorn_iterations": iters, "match_threshold": float(g["match_threshold"])}).eval()
    m.load_state_dict(synth_sd)
    m(pair_to_data(synth.make_pair(256, 1002), 15, 2, 7, device="cuda"))          # settle attention_precision='auto'
    monkeypatch.setenv("GIMS_SCORE_PREC", "f32")
    data = pair_to_data(synth.make_pair(n, seed), rad, pct, ms, device="cuda")
    hip.linear_launch_counts(reset=True)
    out = m(data)
    torch.cuda.synchronize()
    counts = hip.linear_launch_counts()
    assert counts["f32_batch"] == 1 and counts["x6_batch"] == 0, _only(counts)
    print(name, "GIMS_SCORE_PREC=f32", compare_with_golden(out, data, g, float(g["match_threshold"])))


# ================================================================================================ 4. the six-pass score GEMM
def _x6_launch(hip, problems, k, seed, expect_error=None):
    """One hip.linear_batch(PREC_BF16X6) launch over `problems` = [(m, n, upper)], scale 0.5.  Operands are row ranges of two SPL3 buffers, the
    outputs are carved back to back out of ONE canaried buffer (ld = ceil4(n) + 8, three pad rows each), so a store into the next
    problem's matrix shows as a torn canary or a wrong value.  Returns (worst err / bar, host data) after asserting every problem."""
    r = np.random.default_rng(seed)
    ma, mw = sum(p[0] for p in problems), sum(p[1] for p in problems if not p[2])
    a = r.normal(size=(ma, k)).astype(np.float32)
    a[min(3, ma - 1), 5] = 1234.5
    w = (r.normal(size=(max(mw, 1), k)) / np.sqrt(k)).astype(np.float32)
    A3, W3 = hip.split_spl3(_dev(a)), hip.split_spl3(_dev(w))
    lds = [R.ceil_to(n, 4) + 8 for (_, n, _) in problems]
    sizes = [(m + 3) * ld for (m, _, _), ld in zip(problems, lds)]
    flat = _canary((sum(sizes),))
    largs, views, ra, rw, off = [], [], 0, 0, 0
    for (m, n, upper), ld, size in zip(problems, lds, sizes):
        buf = flat[off:off + size].view(m + 3, ld)
        a_rows = (ra, ra + m)
        if upper:
            assert m == n
            w_op, w_rows = A3[ra:ra + m], None
        else:
            w_op, w_rows = W3[rw:rw + n], (rw, rw + n)
            rw += n
        la = hip.linear_args(A3[ra:ra + m], w_op, out=buf[:m, :n], precision=hip.PREC_BF16X6, scale=0.5, n=n)
        if upper:
            la.flags = hip.LINEAR_UPPER
        largs.append(la)
        views.append((a_rows, w_rows, off, size))
        ra, off = ra + m, off + size
    dev_args = torch.empty(ctypes.sizeof(hip.LinearArgs) * len(largs), dtype=torch.uint8, device="cuda")
    hip.linear_launch_counts(reset=True)
    if expect_error is not None:
        with pytest.raises(hip.GimsHipError, match=expect_error):
            hip.linear_batch(largs, dev_args, hip.PREC_BF16X6)
        torch.cuda.synchronize()
        assert _only(hip.linear_launch_counts()) == {}
        assert R.is_canary(_bits(flat)).all()
        return None
    hip.linear_batch(largs, dev_args, hip.PREC_BF16X6)
    torch.cuda.synchronize()
    assert _only(hip.linear_launch_counts()) == {"x6_batch": 1}
    bits = _bits(flat)
    worst = 0.0
    for i, ((m, n, upper), ld, (a_rows, w_rows, off, size)) in enumerate(zip(problems, lds, views)):
        what = f"problem {i} ({m}x{n}{', upper' if upper else ''})"
        b = bits[off:off + size].reshape(m + 3, ld)
        R.assert_pad_intact(b, m, n, what)
        ai = a[a_rows[0]:a_rows[1]]
        wi = ai if upper else w[w_rows[0]:w_rows[1]]
        ref, sc = R.linear_ref(ai, wi, scale=0.5)
        ratio = np.abs(_f32(b[:m, :n]) - ref) / sc / BAR_F32              # test_linear_bf16x6: 2e-6 of |a| |w| scale
        if upper:
            strict = np.triu(np.ones((m, n), dtype=bool), 1)
            untouched = R.is_canary(b[:m, :n])
            assert not untouched[strict].any() and (ratio[strict] < 1.0).all(), what
            assert (untouched | (ratio < 1.0))[~strict].all(), f"{what}: an element outside the strict upper triangle is neither right nor untouched"
            ratio = ratio[~untouched]
        assert np.isfinite(ratio).all() and ratio.max() < 1.0, f"{what}: {ratio.max():.3f} of the bar"
        worst = max(worst, float(ratio.max()))
    return worst


def _small_x6_problems(count):
    return [(1 + (7 * i) % 40, 1 + (11 * i) % 37, False) for i in range(count)]


def test_x6_tile_seams(hip):
    """m / n at 256 / 128 plus and minus one, single rows and columns, and a problem of 3 x 3 tiles, in one launch."""
    shapes = [(256, 128), (257, 129), (255, 127), (1, 1), (1, 300), (300, 1), (513, 260)]
    print(f"x6 seams: worst err/bar {_x6_launch(hip, [(m, n, False) for m, n in shapes], 64, seed=41):.3f}")


def test_x6_walks_1024_problems(hip):
    """The limit: 1024 one-tile problems.  256 workgroups walk four tiles each and skip 256 problems per stride, the table loop takes its
    second trip, and the descriptor upload spans many chunks."""
    problems = _small_x6_problems(R.X6_MAX_PROBLEMS)
    assert all(R.x6_tiles(m, n) == 1 for m, n, _ in problems)
    print(f"x6 1024 problems: worst err/bar {_x6_launch(hip, problems, 32, seed=42):.3f}")


def test_x6_leaves_a_large_problem_in_the_middle_of_its_walk(hip):
    problems = _small_x6_problems(300)
    problems[150] = (1300, 1300, False)
    assert R.x6_tiles(1300, 1300) > 1
    print(f"x6 mixed tile counts: worst err/bar {_x6_launch(hip, problems, 32, seed=43):.3f}")


def test_x6_refuses_1025_problems(hip):
    _x6_launch(hip, _small_x6_problems(R.X6_MAX_PROBLEMS + 1), 32, seed=44, expect_error="at most 1024 problems per launch")


def test_x6_upper_and_plain_in_one_launch(hip):
    print(f"x6 upper + plain: worst err/bar {_x6_launch(hip, [(700, 700, True), (300, 260, False), (1300, 1300, True)], 64, seed=45):.3f}")


# ================================================================================================ 5. split kernels
def _split_values(rows, k, seed):
    """normal * exp(4 normal) like test_split_spl3_exact, clipped below the largest finite bf16, with signed zeros, f32 subnormals and exact
    bf16 rounding ties (even and odd neighbours) in the first and the last row."""
    r = np.random.default_rng(seed)
    x = (r.normal(size=(rows, k)) * np.exp(r.normal(size=(rows, k)) * 4)).astype(np.float32)
    x = np.clip(x, -0.5 * R.BF16_MAX, 0.5 * R.BF16_MAX)
    ties = ((x[0, :16].view(np.uint32) & 0xFFFF0000) | 0x8000).view(np.float32)
    special = np.concatenate([np.array([0.0, -0.0, 1e-40, -3e-42, 1.4e-45, -1.4e-45, 1.1754942e-38, -8.8e-39], dtype=np.float32), ties])
    for row in {0, rows - 1}:
        x[row, :len(special)] = special
        x[row, k - len(special):] = special[::-1]
    return x


@pytest.mark.parametrize("rows", [4100, 1])       # 4100 x 544 = 2.2 M elements: above both grid caps (4096 and 8192 blocks of 256 threads)
def test_split_kernels_bit_for_bit(hip, rows):
    """gims_split_bf16 / gims_split_spl32 / gims_split_spl3 past the cap of their grids (second trip of the grid-stride loop), from a column
    window of a wider source into pitched destinations whose pads must not change; every plane bit-equal to the header's definition."""
    k = 544
    x = _split_values(rows, k, seed=rows)
    wide = _canary((rows, k + 40))
    src = wide[:, 8:8 + k]
    src.copy_(_dev(x))
    hi, lo = hip.split_bf16(src)                        # (flat: the wrapper makes the window contiguous)
    want_hi, want_lo = R.split2(x)
    np.testing.assert_array_equal(_bits(hi), want_hi)
    np.testing.assert_array_equal(_bits(lo), want_lo)
    d32 = _canary((rows + 2, 2 * k + 64), bits16=True)
    hip.split_spl32(src, out=d32[:rows, :2 * k])
    b32 = _bits(d32)
    R.assert_pad_intact(b32, rows, 2 * k, "SPL32")
    np.testing.assert_array_equal(b32[:rows, :2 * k], R.spl32(x))
    d3 = _canary((rows + 2, 3 * k + 8), bits16=True)
    hip.split_spl3(src, out=d3[:rows, :3 * k])
    b3 = _bits(d3)
    R.assert_pad_intact(b3, rows, 3 * k, "SPL3")
    np.testing.assert_array_equal(b3[:rows, :3 * k], R.spl3(x))
    planes = R.bf16_value(b3[:rows, :3 * k].reshape(rows, k // 32, 3, 32)).astype(np.float64)
    R.assert_spl3_sums_back(planes.sum(2).reshape(rows, k), x)      # a1 + a2 + a3 is the input, exactly (f32 subnormals: as far as bf16 reaches)
    assert R.is_canary(_bits(wide)[:, :8]).all() and R.is_canary(_bits(wide)[:, 8 + k:]).all()


def test_split_kernels_zero_rows(hip):
    """Zero rows: no launch, no error, nothing written (valid pointers: an empty torch tensor has none)."""
    k = 64
    src = _dev(np.ones((2, k), dtype=np.float32))
    dst = _canary((2, 3 * k), bits16=True)
    lib, stream = hip.load(), torch.cuda.current_stream().cuda_stream
    assert lib.gims_split_spl32(src.data_ptr(), k, dst.data_ptr(), 3 * k, 0, k, stream) == 0
    assert lib.gims_split_spl3(src.data_ptr(), k, dst.data_ptr(), 3 * k, 0, k, stream) == 0
    assert lib.gims_split_bf16(src.data_ptr(), dst.data_ptr(), dst[1].data_ptr(), 0, stream) == 0
    torch.cuda.synchronize()
    assert R.is_canary(_bits(dst)).all()


def test_split_kernels_non_finite_in_non_finite_out(hip):
    """inf and NaN: the hi plane is non-finite -- what test_linear_range_report_propagates_non_finite_values relies on, and no more."""
    x = np.ones((2, 32), dtype=np.float32)
    x[0, 3], x[0, 7], x[1, 30] = np.inf, -np.inf, np.nan
    bad = ~np.isfinite(x)
    hi, _ = hip.split_bf16(_dev(x))
    h32 = _bits(hip.split_spl32(_dev(x)))[:, :32]
    h3 = _bits(hip.split_spl3(_dev(x)))[:, :32]
    for planes in (_bits(hi), h32, h3):
        v = R.bf16_value(planes)
        assert (~np.isfinite(v[bad])).all() and np.isfinite(v[~bad]).all()


# ================================================================================================ 6. refusals
def test_refusals(hip):
    """Host-side checks, each on the library's own wording; every one returns before a launch (the census stays empty)."""
    x = torch.ones((8, 64), dtype=torch.float32, device="cuda")
    w = torch.ones((8, 64), dtype=torch.float32, device="cuda")
    out = _canary((8, 8))
    xs, ws = hip.split_spl32(x), hip.split_spl32(w)
    x3, w3 = hip.split_spl3(x), hip.split_spl3(w)
    wh, wl = hip.split_bf16(w)
    dev_args = torch.empty(ctypes.sizeof(hip.LinearArgs) * 2, dtype=torch.uint8, device="cuda")
    hip.linear_launch_counts(reset=True)
    E = hip.GimsHipError
    with pytest.raises(E, match="gims_linear_put_many: pre-split operands are not available in batches"):
        hip.linear_batch([hip.linear_args(xs, ws, spl=True, precision=hip.PREC_BF16X3, out=out)], dev_args, hip.PREC_BF16X3)
    with pytest.raises(E, match=r"gims_linear\(pre-split\): n, ldc and ldc_bf16 must be multiples of 4, ld_split of 8"):
        hip.linear(xs, ws, spl=True, precision=hip.PREC_BF16X3, out=out[:, :6], n=6)
    with pytest.raises(E, match=r"gims_linear\(pre-split\): K=16 k0=16 must be multiples of 32"):
        hip.linear(xs[:, :32], ws[:, :32], spl=True, precision=hip.PREC_BF16X3, out=out)
    with pytest.raises(E, match=r"gims_linear\(f32\): K=48 k0=48 must be multiples of 32"):
        hip.linear(x[:, :48], w[:, :48], precision=hip.PREC_F32, out=out)
    with pytest.raises(E, match=r"gims_linear\(f32\): K=64 k0=16 must be multiples of 32"):
        hip.linear(x[:, :16], w, a1=x[:, 16:], precision=hip.PREC_F32, out=out)
    with pytest.raises(E, match=r"gims_linear\(bf16x3\): K=32 k0=32 must be multiples of 64"):
        hip.linear(x[:, :32], wh[:, :32], w_lo=wl[:, :32], precision=hip.PREC_BF16X3, out=out)
    with pytest.raises(E, match=r"gims_linear\(bf16x6\): K=16 must be a multiple of 32, one A segment"):
        hip.linear_batch([hip.linear_args(x3[:, :48], w3[:, :48], precision=hip.PREC_BF16X6, out=out)], dev_args, hip.PREC_BF16X6)
    with pytest.raises(E, match="gims_linear: GIMS_PREC_BF16X6 runs through gims_linear_put_many \\+ gims_linear_batch"):
        hip.linear(x3, w3, precision=hip.PREC_BF16X6, out=out)
    with pytest.raises(E, match=r"gims_linear\(bf16x6\): plain scaled product only"):
        hip.linear_batch([hip.linear_args(x3, w3, precision=hip.PREC_BF16X6, out=out, bias=torch.ones(8, device="cuda"))], dev_args, hip.PREC_BF16X6)
    with pytest.raises(E, match="gims_linear_batch: unknown precision 7"):
        hip.linear_batch([hip.linear_args(x, w, precision=hip.PREC_F32, out=out)], dev_args, 7)
    torch.cuda.synchronize()
    assert _only(hip.linear_launch_counts()) == {}
    assert R.is_canary(_bits(out)).all()
