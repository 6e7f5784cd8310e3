"""One training step on the HIP path (gims_amd/trainstep.py): model.train(); loss, pos, neg = model(data, mode='train');
loss.backward() -- against the reference's own training step (tests/golden/trainstep_*: train.py:100, 136-137 run on the
reference) and, on other seeds, against the oracle's autograd (oracle/gims_oracle.py: train_step, pinned to the same
goldens by tests/test_train_oracle_cpu.py)."""
import numpy as np
import pytest
import torch

from gims_amd import GMatcher, synth
from oracle import gims_oracle as O
from tests.helpers import check_step_gradients, fixture_state_dict, golden_names, load_golden, train_data, train_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _autograd_on():
    """Other test modules switch autograd off process-wide at import; a training step needs it."""
    with torch.enable_grad():
        yield

# Bars (relative to the largest entry of each gradient tensor, floor 1e-3 of the largest gradient entry anywhere).  The
# reference and the oracle -- two f32 evaluations of the same step -- differ by 6e-4 worst / 1.2e-4 p95 on these fixtures
# (4e-3 worst on the batch-of-two fixture, where one ReLU of a near-zero pre-activation falls the other way).  The default
# precision of the HIP step (split-bf16x6: 24 mantissa bits per operand) is held to the oracle's p95 bar (tests/test_train_oracle_cpu.py)
# and to 2e-2 on the worst of the 282 tensors: which ReLUs flip depends on the last bit of every product, and two builds of the same
# kernels (a different epilogue rounding order) moved the worst tensor of the 2x2048 fixture between 5.7e-3 and 1.1e-2; measured
# 1e-3 ... 1.1e-2 worst, 6e-5 ... 3.8e-4 p95.  'bf16x3' (16 bits per operand) is the
# faster, looser mode: ~100x more ReLU flips and cancellation noise in the bias-like gradients (measured 2.6e-2 ... 8.5e-2
# worst, 7e-4 ... 1e-2 p95).
BARS = {"bf16x6": (2e-2, 1e-3), "bf16x3": (1.5e-1, 2e-2)}
RTOL_WORST, RTOL_P95 = BARS["bf16x6"]
LOSS_ATOL = 1e-4


def _model(sd, g, precision="bf16x6", use_layernorm=False, **config):
    m = GMatcher({"sinkhorn_iterations": int(g["meta"][4]), "pos_loss_weight": float(g["pos_loss_weight"]),
                  "neg_loss_weight": float(g["neg_loss_weight"]), "train_precision": precision, "use_layernorm": use_layernorm, **config})
    m.load_state_dict(sd)
    return m.cuda().train()


@pytest.mark.parametrize("precision", ["bf16x6", "bf16x3"])
@pytest.mark.parametrize("name", golden_names("trainstep_") + golden_names("binstep_"))
def test_train_step_vs_reference_golden(name, precision):
    g = load_golden(name)
    ln = name.startswith("trainstep_ln_")          # use_layernorm=True: the reference's LayerNorm in every MLP
    # (binstep_*: bin_score at the median row maximum of the pair's score matrix, tools/gen_golden_alpha.py)
    sd = synth.make_state_dict(123, use_layernorm=ln) if "bin_score" not in g else fixture_state_dict(g)
    m = _model(sd, g, precision, ln)
    data = train_data(train_pairs(name, g), g, device="cuda")
    m.zero_grad()
    loss, pos, neg = m(data, mode="train")
    assert loss.requires_grad and loss.dim() == 0
    loss.backward()
    got = [float(loss.detach()), float(pos.detach()), float(neg.detach())]
    np.testing.assert_allclose(got, [g["loss"], g["pos"], g["neg"]], atol=LOSS_ATOL, rtol=0)
    for s in "01":
        for b in range(int(g["meta"][5])):
            assert data[f"kept_kpts{s}_indices"][b] == g[f"kept{s}_{b}"].tolist()
    grads = {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    # one ReLU of a near-zero pre-activation falling the other way moves a bias-like gradient by ~1 / (positions per call of the
    # module): with few kept keypoints (the sparse fixture keeps ~260 per image, the batch-of-two 2 x 64) the worst-tensor bar
    # scales with that; the p95 bar does not move
    positions = min(int(g["meta"][5]) * len(g[f"kept{s}_0"]) for s in "01")
    worst_bar = max(BARS[precision][0], 10.0 / positions)
    worst, where, p95 = check_step_gradients(g, grads, rtol=worst_bar, rtol_p95=BARS[precision][1])
    print(name, precision, "loss", got, "gradients: worst", worst, where, "p95", p95)
    bufs = dict(m.named_buffers())
    for k in g:
        if k.startswith("b:"):
            mine, ref = bufs[k[2:]].cpu().numpy(), g[k]
            if k.endswith("num_batches_tracked"):
                assert int(mine) == int(ref), k
            else:
                np.testing.assert_allclose(mine, ref, rtol=1e-4 if precision == "bf16x6" else 1e-3, atol=1e-5, err_msg=k)


@pytest.mark.parametrize("name", ["trainstep_n256_s1002_i100", "trainstep_n512_s1003_i20"])
def test_train_step_with_f32_reverse_pass_vs_reference_golden(name):
    """train_backward_precision='f32' (the documented setting for sharply peaked trained attention: the attention reverse on exact-f32 products,
    the reverse GEMMs in six bf16 passes) is held to the loss and gradient bars of the default step (BARS['bf16x6'])."""
    g = load_golden(name)
    m = _model(synth.make_state_dict(123), g, "bf16x6", train_backward_precision="f32")
    data = train_data(train_pairs(name, g), g, device="cuda")
    m.zero_grad()
    loss, pos, neg = m(data, mode="train")
    loss.backward()
    got = [float(loss.detach()), float(pos.detach()), float(neg.detach())]
    np.testing.assert_allclose(got, [g["loss"], g["pos"], g["neg"]], atol=LOSS_ATOL, rtol=0)
    grads = {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    positions = min(int(g["meta"][5]) * len(g[f"kept{s}_0"]) for s in "01")
    worst, where, p95 = check_step_gradients(g, grads, rtol=max(RTOL_WORST, 10.0 / positions), rtol_p95=RTOL_P95)
    print(name, "f32 reverse pass: loss", got, "gradients: worst", worst, where, "p95", p95)


@pytest.mark.parametrize("value", ["bf16x3", "bf16x6", "f32"])
def test_train_backward_precision_reaches_the_attention_reverse(monkeypatch, value):
    """What the reverse pass hands to hip.train_attention_backward: precision=PREC_F32 by name for 'f32', no precision argument for the other
    two values (the kernel then follows the GEMM precision of the reverse pass: bf16x3 -> three-pass kernel, bf16x6 -> exact f32), 18 calls."""
    from gims_amd import hip
    name = "trainstep_n256_s1002_i100"
    g = load_golden(name)
    m = _model(synth.make_state_dict(123), g, "bf16x6", train_backward_precision=value)
    seen = []
    real = hip.train_attention_backward

    def spy(*args, **kwargs):
        seen.append((len(args), dict(kwargs), getattr(hip._TLS, "gemm_prec", None)))
        return real(*args, **kwargs)
    monkeypatch.setattr(hip, "train_attention_backward", spy)
    data = train_data(train_pairs(name, g), g, device="cuda")
    m.zero_grad()
    loss, _, _ = m(data, mode="train")
    loss.backward()
    assert len(seen) == 18
    for n_args, kwargs, gemm_prec in seen:
        assert n_args == 6                                                     # (qkv, o, lse, d_o, problems, heads): precision is never positional
        assert kwargs == ({"precision": hip.PREC_F32} if value == "f32" else {})
        assert gemm_prec == (hip.PREC_BF16X3 if value == "bf16x3" else hip.PREC_BF16X6)
    np.testing.assert_allclose(float(loss.detach()), g["loss"], atol=LOSS_ATOL, rtol=0)


def test_train_step_vs_oracle_and_optimizer_step():
    """A seed without a fixture, compared with the oracle's autograd; then two optimizer steps lower the loss on the same batch
    (the gradients point downhill) and a second backward on released activations raises."""
    g = load_golden("trainstep_n256_s1002_i100")
    sd = synth.make_state_dict(7)
    pairs = [synth.make_pair(200, 77)]
    m = _model(sd, g)
    cfg = dict(sinkhorn_iterations=int(g["meta"][4]), pos_loss_weight=float(g["pos_loss_weight"]), neg_loss_weight=float(g["neg_loss_weight"]))
    (l_ref, p_ref, n_ref), g_ref, _ = O.train_step(sd, train_data(pairs, g), cfg)
    loss, pos, neg = m(train_data(pairs, g, device="cuda"), mode="train")
    (2.0 * loss + 0.5 * pos).backward()                   # upstream weights other than (1, 0, 0)
    assert abs(float(loss.detach()) - l_ref) < LOSS_ATOL and abs(float(pos.detach()) - p_ref) < LOSS_ATOL
    big = max(float(np.abs(v).max()) for v in g_ref.values())
    errs = []
    for k, p in m.named_parameters():
        ref = 2.5 * g_ref[k] if True else None            # d(2 loss + 0.5 pos) = 2.5 d pos + 2 d neg; neg has no gradient here (clamped corner cell)
        den = max(float(np.abs(ref).max()), 1e-3 * 2.5 * big)
        errs.append((float(np.abs(p.grad.cpu().numpy() - ref).max()) / den, k))
    errs.sort()
    # 200 keypoints per image: ONE ReLU whose pre-activation is within rounding of zero moves a BatchNorm bias gradient and
    # the matching row of the weight gradient by a few per cent (1 of ~200 addends) -- between two f32 evaluations as well;
    # such a flip in layer 4 (this seed has one) also shifts every gradient upstream of it by ~1e-3.  Bars for this small case:
    # median at the f32 level, p95 3e-3, worst tensor 1.5e-1 (structural errors are orders of magnitude above all three)
    assert errs[len(errs) // 2][0] < 2e-4 and errs[int(0.95 * (len(errs) - 1))][0] < 3e-3 and errs[-1][0] < 1.5e-1, errs[-5:]
    with pytest.raises(RuntimeError):
        loss.backward()
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    first = None
    for _ in range(3):
        opt.zero_grad()
        loss, _, _ = m(train_data(pairs, g, device="cuda"), mode="train")
        loss.backward()
        opt.step()
        first = float(loss) if first is None else first
    assert float(loss) < first, (first, float(loss))


def test_train_mode_under_no_grad_and_eval_mode_are_graph_free():
    g = load_golden("trainstep_n256_s1002_i100")
    m = _model(synth.make_state_dict(123), g)
    pairs = train_pairs("trainstep_n256_s1002_i100", g)
    with torch.no_grad():
        loss, _, _ = m(train_data(pairs, g, device="cuda"), mode="train")
    assert not loss.requires_grad
    loss2, _, _ = m.eval()(train_data(pairs, g, device="cuda"), mode="train")     # running statistics, forward value only
    assert not loss2.requires_grad


def test_train_step_edge_cases_vs_oracle():
    """Ground-truth tables the reference's loop can produce at the margins: only unmatched keypoints (every row reads the corner
    cell, gmatcher.py:368-372), and a single positive row -- loss and all gradients against the oracle's autograd."""
    g = load_golden("trainstep_n256_s1002_i100")
    sd = synth.make_state_dict(123)
    pairs = [synth.make_pair(96, 31)]
    cfg = dict(sinkhorn_iterations=int(g["meta"][4]), pos_loss_weight=float(g["pos_loss_weight"]), neg_loss_weight=float(g["neg_loss_weight"]))
    full = train_data(pairs, g)["matches"]
    neg_only = full[(full[:, 1] < 0) | (full[:, 2] < 0)]
    one_pos = full[(full[:, 1] >= 0) & (full[:, 2] >= 0)][:1]
    for table in (neg_only, one_pos):
        d_cpu, d_gpu = train_data(pairs, g), train_data(pairs, g, device="cuda")
        d_cpu["matches"], d_gpu["matches"] = table.clone(), table.clone().cuda()
        (l_ref, p_ref, n_ref), g_ref, _ = O.train_step(sd, d_cpu, cfg)
        m = _model(sd, g)
        loss, pos, neg = m(d_gpu, mode="train")
        loss.backward()
        assert abs(float(loss.detach()) - l_ref) < LOSS_ATOL and abs(float(neg.detach()) - n_ref) < LOSS_ATOL
        big = max(float(np.abs(v).max()) for v in g_ref.values())
        for k, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
            if big > 0:
                den = max(float(np.abs(g_ref[k]).max()), 1e-3 * big)
                assert float(np.abs(p.grad.cpu().numpy() - g_ref[k]).max()) / den < 1.5e-1, k
            else:
                assert float(p.grad.abs().max()) == 0.0, k
