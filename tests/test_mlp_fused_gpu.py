"""One layer's MLP in one launch (GIMS_OP_MLP of gims_run_ops, gims_amd/csrc/linear_mlp.hip: `mlp_fused_x3_kernel`):

    out = residual + W1 relu(W0 [a0 | a1] + b0) + b1        (models/gmatcher.py:141-142, the merge conv folded into W0)

* the kernel, called through a one-op table (so not through GMatcher's size policy), against float64 and against the two gims_linear launches
  it replaces;
* the K-axis order of the W1 copy it reads (CPU);
* GMatcher with GIMS_MLP_FUSED=1 against =0 and against the reference's own outputs, through the replayed table and launch by launch;
* the compiler's resource report: no scratch (CPU).

Bars.  Against float64: scaled error < 4e-5, the bar of tests/test_hip_kernels.py::test_linear_presplit (2^-17 relative per split-bf16 product,
sqrt(K) accumulation), on the scale that propagates through both layers: |res| + |b1| + |W1| (|W0| |a| + |b0|).  Against the two launches:
< 2e-6 on the same scale -- the hidden values are equal bit for bit (same K order, same split arithmetic), so only the f32 summation order
of the second product differs (the kernel adds the two halves of its K range at the end).  The SPL32 copy reconstructs the f32 output to
2^-15 relative (hi + lo of a split f32 carries 16 mantissa bits)."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from gims_amd import hip

torch.set_grad_enabled(False)

D = 256
SENTINEL = 777.0


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _problem(m, d, seed, b0_shift=0.0):
    """Inputs built like test_linear_presplit's: normal activations with one 321.5 outlier, weights / sqrt(k), normal biases and residual; from
    31 rows on (and b0 not shifted), rows 8..15 are solved for pre-activations in (-3, -1) (hidden activation exactly zero) and rows 16..23 for (1, 3) (every hidden
    unit active)."""
    r = np.random.default_rng(seed)
    k = hid = 2 * d
    a = r.normal(size=(m, k)).astype(np.float32)
    w0 = (r.normal(size=(hid, k)) / np.sqrt(k)).astype(np.float32)
    w1 = (r.normal(size=(d, hid)) / np.sqrt(hid)).astype(np.float32)
    b0 = (r.normal(size=hid) + b0_shift).astype(np.float32)
    b1 = r.normal(size=d).astype(np.float32)
    res = r.normal(size=(m, d)).astype(np.float32)
    if m > 3:
        a[3, 5] = 321.5
    blocks = {}
    if m >= 31 and not b0_shift:
        for name, rows, sign in (("neg", slice(8, 16), -1.0), ("pos", slice(16, 24), 1.0)):
            t = sign * r.uniform(1.0, 3.0, size=(8, hid))
            a[rows] = np.linalg.solve(w0.astype(np.float64), (t - b0).T).T.astype(np.float32)
            blocks[name] = rows
    return a, w0, w1, b0, b1, res, blocks


def _reference(a, w0, w1, b0, b1, res):
    f = lambda x: x.astype(np.float64)          # noqa: E731
    pre = f(a) @ f(w0).T + f(b0)
    ref = f(res) + np.maximum(pre, 0) @ f(w1).T + f(b1)
    scale = np.abs(f(res)) + np.abs(f(b1)) + (np.abs(f(a)) @ np.abs(f(w0)).T + np.abs(f(b0))) @ np.abs(f(w1)).T
    return pre, ref, scale


def _run_fused(a, w0, w1, b0, b1, res, d, pad=64):
    """The op on buffers of m + pad rows whose tail carries a sentinel; residual aliases out.  Returns (out, SPL32 copy), all rows."""
    m = a.shape[0]
    A = hip.split_spl32(_dev(a))
    W = hip.split_spl32(_dev(np.concatenate([w0, hip.mlp_w1_permute(torch.from_numpy(w1)).numpy()], 0)))
    B = _dev(np.concatenate([b0, b1]))
    out = torch.full((m + pad, d), SENTINEL, dtype=torch.float32, device="cuda")
    out[:m] = _dev(res)
    osp = torch.full((m + pad, 2 * d), SENTINEL, dtype=torch.bfloat16, device="cuda")
    ops = hip.make_ops([hip.op_mlp(A[:, :2 * d], A[:, 2 * d:], W, B, out[:m], osp[:m], residual=out[:m])])
    hip.run_ops(ops)
    torch.cuda.synchronize()
    return out, osp


def _run_two_launches(a, w0, w1, b0, b1, res, d):
    A, W0, W1 = hip.split_spl32(_dev(a)), hip.split_spl32(_dev(w0)), hip.split_spl32(_dev(w1))
    hidden = torch.empty((a.shape[0], 4 * d), dtype=torch.bfloat16, device="cuda")
    hip.linear(A[:, :2 * d], W0, spl=True, a1=A[:, 2 * d:], bias=_dev(b0), act=hip.ACT_RELU, precision=hip.PREC_BF16X3, out_split=hidden)
    out = _dev(res)
    hip.linear(hidden, W1, spl=True, bias=_dev(b1), residual=out, out=out, precision=hip.PREC_BF16X3)
    return out.cpu().numpy()


def _check(m, b0_shift=0.0):
    a, w0, w1, b0, b1, res, blocks = _problem(m, D, 1000 + m, b0_shift)
    pre, ref, scale = _reference(a, w0, w1, b0, b1, res)
    if "neg" in blocks:
        assert (pre[blocks["neg"]] < -0.5).all() and (pre[blocks["pos"]] > 0.5).all()
    if b0_shift:
        assert (pre > 1.0).all()                 # every hidden unit of every row is active
    out, osp = _run_fused(a, w0, w1, b0, b1, res, D)
    o = out[:m].cpu().numpy()
    err = float((np.abs(o - ref) / scale).max())
    two = _run_two_launches(a, w0, w1, b0, b1, res, D)
    diff = float((np.abs(o - two) / scale).max())
    print(f"m={m} b0_shift={b0_shift}: scaled err vs float64 {err:.3e}, scaled diff vs two launches {diff:.3e}")
    assert err < 4e-5, f"max scaled err {err:.3e} at {np.unravel_index((np.abs(o - ref) / scale).argmax(), o.shape)}"
    assert diff < 2e-6, f"max scaled difference from the two launches {diff:.3e}"
    if "neg" in blocks:                          # hidden exactly zero: out = (0 + b1) + res, whatever the summation order
        np.testing.assert_array_equal(o[blocks["neg"]], (b1 + res[blocks["neg"]]).astype(np.float32))
    hi, lo = hip.spl32_planes(osp[:m])
    rec = hi.float().cpu().numpy().astype(np.float64) + lo.float().cpu().numpy()
    assert (np.abs(rec - o) <= np.abs(o) * 2.0 ** -15 + 1e-30).all()
    # rows beyond m: untouched
    assert (out[m:] == SENTINEL).all() and (osp[m:].float() == float(torch.tensor(SENTINEL).bfloat16())).all()


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 31, 128, 129, 300, 1000])      # a lone row, a partial MFMA block, a tile, tile + 1, ragged tiles, many tiles
def test_kernel_vs_float64_and_two_launches(m):
    _check(m)


@pytest.mark.gpu
def test_kernel_with_every_hidden_unit_active():
    _check(300, b0_shift=100.0)


@pytest.mark.gpu
def test_other_widths_are_refused():
    """The kernel serves D = 256 only: D = 128 is GIMS_EINVAL before anything is launched."""
    d, m = 128, 64
    a, w0, w1, b0, b1, res, _ = _problem(m, d, 5)
    out = _dev(res)
    with pytest.raises(hip.GimsHipError, match=r"\(-1\).*mlp_fused"):
        _run = hip.make_ops([hip.op_mlp(hip.split_spl32(_dev(a))[:, :2 * d], hip.split_spl32(_dev(a))[:, 2 * d:],
                                        hip.split_spl32(_dev(np.concatenate([w0, w1], 0))), _dev(np.concatenate([b0, b1])), out,
                                        torch.zeros((m, 2 * d), dtype=torch.bfloat16, device="cuda"), residual=out)])
        hip.run_ops(_run)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), res)


# --------------------------------------------------------------------------------------------- weights (CPU)
def _spl32_cpu(w):
    """SPL32 on the host: per 32-channel block 32 hi then 32 lo values (hi = bf16(x), lo = bf16(x - hi))."""
    n, k = w.shape
    hi = w.bfloat16()
    lo = (w - hi.float()).bfloat16()
    return torch.cat([hi.view(n, k // 32, 32), lo.view(n, k // 32, 32)], 2).reshape(n, 2 * k)


@pytest.mark.parametrize("d", [128, 256])
def test_w1_permutation_round_trip(d):
    """Un-permuting the packed, permuted W1 gives back the packed original; the order is the one a lane holds hid^T in."""
    order = list(hip.MLP_W1_ORDER)
    assert sorted(order) == list(range(32))
    for pos, c in enumerate(order):              # position 16 s + 8 (lane >> 5) + j  <-  channel (r & 3) + 8 (r >> 2) + 4 (lane >> 5), r = 8 s + j
        s, h, j = pos >> 4, (pos >> 3) & 1, pos & 7
        r = 8 * s + j
        assert c == (r & 3) + 8 * (r >> 2) + 4 * h
    w1 = torch.from_numpy(np.random.default_rng(d).normal(size=(d, 2 * d)).astype(np.float32))
    wp = hip.mlp_w1_permute(w1)
    assert wp.shape == w1.shape and not torch.equal(wp, w1)
    packed, packed_p = _spl32_cpu(w1).view(d, 2 * d // 32, 2, 32), _spl32_cpu(wp).view(d, 2 * d // 32, 2, 32)
    back = torch.empty_like(packed_p)
    back[:, :, :, order] = packed_p
    assert torch.equal(back.view(torch.int16), packed.view(torch.int16))


# --------------------------------------------------------------------------------------------- model level
GOLDEN = "e2e_n256_s1002_r15p2m7_i100"


def _model_outputs(synth_sd, g, fused, monkeypatch, no_replay):
    from gims_amd import GMatcher, synth
    from tests.helpers import compare_with_golden, pair_to_data
    monkeypatch.setenv("GIMS_MLP_FUSED", fused)
    if no_replay:
        monkeypatch.setenv("GIMS_NO_REPLAY", "1")
    else:
        monkeypatch.delenv("GIMS_NO_REPLAY", raising=False)
    thr = float(g["match_threshold"])
    m = GMatcher({"sinkhorn_iterations": 100, "match_threshold": thr}).eval()
    m.load_state_dict(synth_sd)
    datas = [pair_to_data(synth.make_pair(256, 1002 + i), 15, 2, 7, device="cuda") for i in range(2)]
    outs = m.match_pairs(datas)
    torch.cuda.synchronize()
    assert m.linear_launches_per_layer == (2 if fused == "1" else 3)          # the table that ran had / had not the one-launch MLP
    compare_with_golden(outs[0], datas[0], g, thr)
    res = []
    for o, d in zip(outs, datas):
        res.append({"kept0": d["kept_kpts0_indices"][0], "kept1": d["kept_kpts1_indices"][0], "m0": o["matches0"][0], "m1": o["matches1"][0],
                    "s0": o["matching_scores0"][0], "s1": o["matching_scores1"][0]})
    return [{k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in r.items()} for r in res]


@pytest.mark.gpu
@pytest.mark.parametrize("no_replay", [False, True], ids=["replayed", "launch_by_launch"])
def test_model_fused_vs_two_launches(synth_sd, monkeypatch, no_replay):
    """Two n = 256 pairs in one batch: GIMS_MLP_FUSED=1 and =0 keep the same keypoints and matches, scores within 1e-5 (f32 summation order
    against the 1e-4 bar), and both pass the reference's golden for pair 0."""
    from tests.helpers import load_golden
    g = load_golden(GOLDEN)
    assert [int(x) for x in g["meta"]] == [256, 1002, 15, 2, 7, 100]
    one = _model_outputs(synth_sd, g, "1", monkeypatch, no_replay)
    two = _model_outputs(synth_sd, g, "0", monkeypatch, no_replay)
    for a, b in zip(one, two):
        for k in ("kept0", "kept1", "m0", "m1"):
            np.testing.assert_array_equal(a[k], b[k])
        ds = max(float(np.abs(a["s0"] - b["s0"]).max()), float(np.abs(a["s1"] - b["s1"]).max()))
        print("max score difference fused vs two launches:", ds)
        assert ds < 1e-5


# --------------------------------------------------------------------------------------------- compiler report (CPU)
def test_kernel_is_scratch_free():
    from gims_amd import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = "linear_mlp.hip"
    assert src in B.SOURCES
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, *B.FLAGS, *B.EXTRA.get(src, []), "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, src), "-o", os.path.join(tmp, "x.o")]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    cur, seen = None, {}
    for line in out.splitlines():
        f = re.search(r"Function Name: (\S+)", line)
        if f:
            cur = f.group(1)
        for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "VGPRs"):
            f = re.search(r"\s" + re.escape(key) + r": (\d+)", line)
            if f and cur:
                seen.setdefault(cur, {})[key] = int(f.group(1))
    kern = [k for k in seen if "mlp_fused_x3_kernel" in k]
    assert len(kern) == 1, seen
    rep = seen[kern[0]]
    assert rep["ScratchSize [bytes/lane]"] == 0 and rep["VGPRs Spill"] == 0 and rep["VGPRs"] <= 256, rep
