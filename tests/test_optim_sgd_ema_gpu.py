"""gims_amd.optim.SGD and ModelEMA (csrc/optim.hip: gims_sgd_step, gims_ema_update) against torch.optim.SGD and the reference's
ModelEMA.update (utils/common.py:1005-1015) on the same tensors, at the shapes where a multi-tensor kernel can go wrong, and inside
the reference's training loop (train.py:136-141)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _autograd_on():
    """Other test modules switch autograd off process-wide at import; a training step needs it."""
    with torch.enable_grad():
        yield


# tests/test_optim_gpu.py's list, then: 3 elements, the 4096-element chunk border from both sides
SHAPES = [(256, 256, 1), (256,), (1,), (3, 5, 7), (4097,), (512, 512, 1), (0,), (33,), (768, 256, 1), (2, 2), (3,), (4096,)]
UNALIGNED = len(SHAPES)          # index of a parameter that starts one element into its storage: not 16-byte aligned, scalar path
N_TINY = 170                     # 1-9 elements each: with the rest, three launches of 80 tensors
NONCONTIG = 3                    # (3, 5, 7): its gradient arrives as a permuted view
NO_GRAD_34 = 4                   # no gradient on steps 3-4
LATE = 5                         # first gradient on step 3


def _tensors(seed, dev):
    """The float32 starting values, on the host (shared by every side) -- ~0.53 M elements."""
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(*s, generator=g) * 0.3 for s in SHAPES]
    vals.append(torch.randn(1001, generator=g) * 0.3)                       # UNALIGNED: elements 1.. of this are the parameter
    vals += [torch.randn(1 + i % 9, generator=g) * 0.3 for i in range(N_TINY)]
    return vals


def _params(vals, dev):
    ps = []
    for i, v in enumerate(vals):
        t = v.to(dev)
        ps.append(torch.nn.Parameter(t[1:] if i == UNALIGNED else t))
    assert ps[UNALIGNED].data_ptr() % 16 == 4 and ps[UNALIGNED].is_contiguous()
    return ps


def _grads(ps, seed, skip=()):
    """Host float32 gradients for one step (None: no gradient), one of them a non-contiguous view."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, p in enumerate(ps):
        shape = tuple(reversed(p.shape)) if i == NONCONTIG else tuple(p.shape)
        gr = torch.randn(*shape, generator=g) * (10.0 ** float(torch.randint(-4, 2, (1,), generator=g)))
        if i == NONCONTIG:
            gr = gr.permute(2, 1, 0)
            assert not gr.is_contiguous()
        out.append(None if i in skip else gr)
    return out


def _set(ps, grads):
    for i, (p, g) in enumerate(zip(ps, grads)):
        if g is None:
            p.grad = None
        elif i == NONCONTIG:
            p.grad = g.permute(2, 1, 0).contiguous().to(p.device).permute(2, 1, 0)       # non-contiguous on the device too
            assert not p.grad.is_contiguous()
        else:
            p.grad = g.to(p.device)


def _f64_step(p64, buf64, grads, group_of, groups):
    """torch's _single_tensor_sgd in float64 on the host, from the same float32 gradients."""
    for i, g in enumerate(grads):
        if g is None:
            continue
        h = groups[group_of[i]]
        g = g.double()
        if h['weight_decay'] != 0:
            g = g + h['weight_decay'] * p64[i]
        if h['momentum'] != 0:
            buf64[i] = g.clone() if buf64[i] is None else buf64[i] * h['momentum'] + (1 - h['dampening']) * g
            g = g + h['momentum'] * buf64[i] if h['nesterov'] else buf64[i]
        p64[i] = p64[i] - h['lr'] * g


def _ulp(x):
    return float(np.spacing(np.float32(x)))


def _within_rule(ours, theirs, ref64, what):
    """max|ours - f64| <= 2 * max|torch - f64| + one float32 ulp of max|f64|, for one tensor; returns max|ours - torch|.
    Margin 2: per operation the two may differ by one rounding (a fused multiply-add against a rounded product and sum), and the
    errors do not compound differently."""
    if ref64.numel() == 0:
        return 0.0
    o, t, r = ours.detach().double().cpu(), theirs.detach().double().cpu(), ref64.reshape(ours.shape)
    eo, et = float((o - r).abs().max()), float((t - r).abs().max())
    assert eo <= 2.0 * et + _ulp(float(r.abs().max())), (what, eo, et)
    return float((o - t).abs().max())


def _build(dev, hyper, ten_groups=False, seed=3):
    from gims_amd.optim import SGD
    vals = _tensors(seed, dev)
    pa, pb = _params(vals, dev), _params(vals, dev)
    n = len(pa)
    if ten_groups:               # two slices of 8 on our side
        bounds = [0, 2, 4, 6, 8, 10, 12, 13, 60, 120, n]
        extra = [dict(lr=1e-2 * (k + 1), weight_decay=(1e-4 * k if k % 2 else 0.0)) for k in range(10)]
    else:                        # train.py:55-57: pg0 with the defaults, pg1 with weight decay, pg2
        bounds = [0, 3, 7, n]
        extra = [dict(), dict(weight_decay=1e-4), dict()]
    opts = []
    for cls, ps in ((torch.optim.SGD, pa), (SGD, pb)):
        kw = dict(foreach=False) if cls is torch.optim.SGD else {}
        o = cls(ps[bounds[0]:bounds[1]], **{'lr': 1e-2, **hyper, **extra[0], **kw})
        for k in range(1, len(bounds) - 1):
            o.add_param_group({'params': ps[bounds[k]:bounds[k + 1]], **extra[k]})
        opts.append(o)
    group_of = [next(k for k in range(len(bounds) - 1) if bounds[k] <= i < bounds[k + 1]) for i in range(n)]
    p64 = [(v[1:] if i == UNALIGNED else v).double().clone() for i, v in enumerate(vals)]
    return pa, pb, opts[0], opts[1], group_of, p64


def _group_hyper(o):
    return [{k: g[k] for k in ('lr', 'momentum', 'dampening', 'weight_decay', 'nesterov')} for g in o.param_groups]


CONFIGS = {"nesterov": dict(momentum=0.9, nesterov=True), "dampening": dict(momentum=0.9, dampening=0.1), "plain": dict(momentum=0)}


@pytest.mark.parametrize("config, ten_groups", [("nesterov", False), ("dampening", False), ("plain", False), ("nesterov", True)])
def test_sgd_matches_torch_over_steps(config, ten_groups):
    dev = torch.device("cuda:0")
    pa, pb, oa, ob, group_of, p64 = _build(dev, CONFIGS[config], ten_groups)
    buf64 = [None] * len(pa)
    worst = 0.0
    for step in range(1, 8):
        skip = set()
        if step in (3, 4):
            skip.add(NO_GRAD_34)                              # a parameter without a gradient is skipped, its buffer kept
        if step < 3:
            skip.add(LATE)                                    # its buffer is first written on step 3, when every other one is read
        grads = _grads(pa, 100 + step, skip)
        _set(pa, grads)
        _set(pb, grads)
        if step == 5:                                         # train.py:21-26 change_lr
            for o in (oa, ob):
                for g in o.param_groups:
                    g['lr'] = g['lr'] * 0.3
        _f64_step(p64, buf64, grads, group_of, _group_hyper(ob))
        oa.step()
        ob.step()
        for i, (a, b) in enumerate(zip(pa, pb)):
            worst = max(worst, _within_rule(b, a, p64[i], (step, i, "param")))
            sa, sb = oa.state.get(a, {}), ob.state.get(b, {})
            assert set(sa.keys()) == set(sb.keys()), (step, i)
            if buf64[i] is not None:
                worst = max(worst, _within_rule(sb['momentum_buffer'], sa['momentum_buffer'], buf64[i], (step, i, "buffer")))
    if CONFIGS[config]['momentum'] == 0:                      # torch keeps no state without momentum; neither do we
        assert len(oa.state) == len(ob.state) == 0 and ob.state_dict()['state'] == oa.state_dict()['state'] == {}
    print(f"SGD {config}{' (10 groups)' if ten_groups else ''}: max|ours - torch.optim.SGD(foreach=False)| over 7 steps = {worst:.3e}")


@pytest.mark.parametrize("config", ["nesterov", "plain"])
def test_sgd_state_dict_round_trips_with_torch(config):
    dev = torch.device("cuda:0")
    pa, pb, oa, ob, group_of, _ = _build(dev, CONFIGS[config])
    for step in range(3):
        grads = _grads(pa, 50 + step)
        _set(pa, grads)
        _set(pb, grads)
        oa.step(); ob.step()
    sd_a, sd_b = oa.state_dict(), ob.state_dict()
    assert set(sd_a.keys()) == set(sd_b.keys())
    assert set(sd_a['state'].keys()) == set(sd_b['state'].keys())
    assert len(sd_a['state']) == (0 if config == "plain" else len(pa))
    for k in sd_a['state']:
        assert set(sd_a['state'][k].keys()) == set(sd_b['state'][k].keys()) == {'momentum_buffer'}
    for ga, gb in zip(sd_a['param_groups'], sd_b['param_groups']):
        assert set(ga.keys()) == set(gb.keys()) and all(ga[k] == gb[k] for k in ga if k != 'foreach')          # (torch's side was built with foreach=False)
    # cross-load: ours <- torch's checkpoint and torch's <- ours, then one more step on each side.  The float64 reference of a side
    # starts from the float32 state that side now holds (its own parameters, the other's buffers)
    ob.load_state_dict(sd_a)
    oa.load_state_dict(sd_b)
    grads = _grads(pa, 99)
    _set(pa, grads)
    _set(pb, grads)
    refs = []
    for o, ps in ((oa, pa), (ob, pb)):
        p64 = [p.detach().double().cpu() for p in ps]
        b64 = [o.state[p]['momentum_buffer'].double().cpu() if 'momentum_buffer' in o.state.get(p, {}) else None for p in ps]
        _f64_step(p64, b64, grads, group_of, _group_hyper(o))
        refs.append((p64, b64))
    oa.step(); ob.step()
    for i, (a, b) in enumerate(zip(pa, pb)):
        if a.numel() == 0:
            continue
        # each side against its own float64 step; the bound is torch's error on its side
        ea = float((a.detach().double().cpu() - refs[0][0][i]).abs().max())
        eb = float((b.detach().double().cpu() - refs[1][0][i]).abs().max())
        assert eb <= 2.0 * ea + _ulp(float(refs[1][0][i].abs().max())), (i, eb, ea)
        if refs[0][1][i] is not None:
            ea = float((oa.state[a]['momentum_buffer'].double().cpu() - refs[0][1][i]).abs().max())
            eb = float((ob.state[b]['momentum_buffer'].double().cpu() - refs[1][1][i]).abs().max())
            assert eb <= 2.0 * ea + _ulp(float(refs[1][1][i].abs().max())), (i, eb, ea)


def _reference_ema_update(ema_state, model_state, d):
    """utils/common.py:1012-1015, on a dict of tensors."""
    with torch.no_grad():
        for k, v in ema_state.items():
            if v.dtype.is_floating_point:
                v *= d
                v += (1. - d) * model_state[k].detach()


@pytest.mark.parametrize("decay", [0.9999 * (1 - np.exp(-1 / 4000)), 0.9, 0.9999, 0.0, 1.0])
def test_ema_update_kernel_is_bitwise_the_two_torch_statements(decay):
    """gims_ema_update on random tensors at the edge shapes (three launches of 80): the same three separately rounded float32 operations
    with the same once-rounded scalars as `v *= d; v += (1 - d) * m`, so equality is exact."""
    from gims_amd import hip
    dev = torch.device("cuda:0")
    ema, model = _params(_tensors(11, dev), dev), _params(_tensors(12, dev), dev)
    ema, model = [p.detach() for p in ema], [p.detach() for p in model]
    want = {i: t.clone() for i, t in enumerate(ema)}
    table = np.array([(a.data_ptr(), b.data_ptr(), a.numel()) for a, b in zip(ema, model)], dtype=hip.EMA_TENSOR_DTYPE)
    for _ in range(3):
        hip.ema_update(table, float(decay))
        _reference_ema_update(want, dict(enumerate(model)), float(decay))
    torch.cuda.synchronize()
    for i, t in enumerate(ema):
        assert torch.equal(t, want[i]), (i, tuple(t.shape))


def test_model_ema_is_bitwise_the_reference_update():
    from gims_amd import GMatcher, synth
    from gims_amd.optim import ModelEMA
    m = GMatcher({})
    m.load_state_dict(synth.make_state_dict(123))
    m.cuda().train()
    ema = ModelEMA(m)
    g = torch.Generator().manual_seed(5)
    want = {k: v.clone() for k, v in ema.ema.state_dict().items()}
    tracked0 = {k: v.clone() for k, v in want.items() if not v.dtype.is_floating_point}
    assert len(tracked0) == 22 and len(want) == 348
    for it in range(5):
        with torch.no_grad():                                 # the model moves between updates: weights, running statistics, counters
            for k, v in m.state_dict().items():
                if v.dtype.is_floating_point:
                    v.add_((torch.randn(v.shape, generator=g) * 0.05).to(v.device) * (v.abs() + 0.1))
                else:
                    v.add_(1)
        ema.update(m)
        _reference_ema_update(want, m.state_dict(), ema.decay(it + 1))
        if it == 2:                                           # the model's tensors are replaced: the cached pointer table must follow
            m.float().cpu().cuda()
    assert ema.updates == 5
    got = ema.ema.state_dict()
    for k, v in got.items():
        assert torch.equal(v, want[k]), k
        if not v.dtype.is_floating_point:
            assert torch.equal(v, tracked0[k]) and int(m.state_dict()[k]) == 5, k       # integral entries are left alone
    assert not ema.ema.training and all(not p.requires_grad for p in ema.ema.parameters())


def test_ema_update_reaches_the_forward():
    """After update() the EMA model's next forward() uses the new weights AND the new BatchNorm running statistics (GMatcher caches its
    packed weights, the statistics folded in, keyed on the parameters' version counters only)."""
    from gims_amd import GMatcher, synth
    from gims_amd.optim import ModelEMA
    from tests.helpers import pair_to_data
    cfg = {"sinkhorn_iterations": 100, "match_threshold": 0.2, "attention_precision": "bf16x3"}
    pair = synth.make_pair(256, 1002)

    def data():
        return pair_to_data(pair, 15, 2, 7, device="cuda")

    def fresh(state):
        f = GMatcher(cfg).eval()
        f.load_state_dict(state)
        return f.cuda()(data())

    def same(out, ref):          # the comparison of test_eval_forward_after_weight_updates_uses_the_new_weights between two instances
        for k in ("matches0", "matches1"):
            assert torch.equal(out[k], ref[k]), k
        for k in ("matching_scores0", "matching_scores1"):
            sel = (out[k.replace("matching_scores", "matches")] >= 0)
            assert sel.any() and float((out[k] - ref[k])[sel].abs().max()) < 1e-5, k

    m = GMatcher(cfg)
    m.load_state_dict(synth.make_state_dict(123, bin_score=62.1052))          # about the median row maximum of this pair's scores
    m.cuda().train()
    ema = ModelEMA(m, decay=0.1)                              # decay(1) = 2.5e-5: one update moves the EMA onto the model
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        before = ema.ema(data())                              # packs the EMA weights as they are
        for k, v in m.state_dict().items():                   # perturb weights and running statistics
            if k.endswith("running_var"):
                v.mul_(1.1)
            elif k.endswith("running_mean"):
                v.add_(0.02)
            elif v.dtype.is_floating_point and k != "bin_score":
                v.mul_(1.0 + 0.01 * torch.randn(v.shape, generator=g).to(v.device))
        ema.update(m)
        out = ema.ema(data())
        same(out, fresh(ema.ema.state_dict()))
        assert not torch.equal(out["matching_scores0"], before["matching_scores0"])
        for k, v in m.state_dict().items():                   # now the running statistics alone
            if k.endswith("running_var"):
                v.mul_(1.2)
            elif k.endswith("running_mean"):
                v.sub_(0.03)
        ema.update(m)
        out2 = ema.ema(data())
        same(out2, fresh(ema.ema.state_dict()))
        assert not torch.equal(out2["matching_scores0"], out["matching_scores0"])


def test_training_loop_with_fused_sgd_and_ema_tracks_torch():
    """The reference's loop (train.py:136-141: forward(mode='train'), backward, optimizer.step(), zero_grad, ema.update) once with
    gims_amd.optim.SGD + ModelEMA and once with torch.optim.SGD + the reference's per-entry EMA loop on a second GMatcher, on two copies
    of one model: the same losses step by step.  The EMA part is asserted on IDENTICAL model weights: next to the fused run's ModelEMA
    a shadow state is kept by the reference's loop from the same model, and the two are bitwise equal (the derivation of
    test_ema_update_kernel_is_bitwise_the_two_torch_statements).  A bound between the two RUNS' EMA states cannot be derived from the
    SGD rule: the runs' gradients differ by more than the roundings of the update (the reverse pass accumulates in an order that is not
    fixed), which is why the losses carry rtol 1e-4 and not an ulp bound.
    lr: the gradient-descent step is kept as small as the Adam loop test's (2e-4 per weight there), so that four steps on one pair
    descend and the two runs stay on one trajectory."""
    from gims_amd import synth
    from gims_amd.optim import SGD, ModelEMA, param_groups
    from tests.helpers import load_golden, train_data, train_pairs
    from tests.test_trainstep_gpu import _model
    name = "trainstep_n256_s1002_i100"
    g = load_golden(name)
    pairs = train_pairs(name, g)
    losses = []
    for fused in (False, True):
        m = _model(synth.make_state_dict(123), g)
        pg0, pg1, pg2 = param_groups(m)                       # train.py:42-57
        opt = SGD(pg0, lr=1e-4, momentum=0.9, nesterov=True) if fused else torch.optim.SGD(pg0, lr=1e-4, momentum=0.9, nesterov=True, foreach=False)
        opt.add_param_group({'params': pg1, 'weight_decay': 5e-4})
        opt.add_param_group({'params': pg2})
        ema = ModelEMA(m)
        start = {k: v.clone() for k, v in ema.ema.state_dict().items()}
        shadow = {k: v.clone() for k, v in start.items()}
        ls = []
        for it in range(4):
            loss, _, _ = m(train_data(pairs, g, device="cuda"), mode="train")
            loss.backward()
            opt.step()
            opt.zero_grad()
            if fused:
                ema.update(m)
                _reference_ema_update(shadow, m.state_dict(), ema.decay(it + 1))
            else:                                             # utils/common.py:1005-1015 as it stands
                ema.updates += 1
                _reference_ema_update(ema.ema.state_dict(), m.state_dict(), ema.decay(ema.updates))
            ls.append(float(loss.detach()))
        assert ema.updates == 4
        got = ema.ema.state_dict()
        if fused:
            for k, v in got.items():
                assert torch.equal(v, shadow[k]), k
        for k in ("gnn.layers.0.mlp.1.running_mean", "gnn.layers.17.mlp.3.weight"):          # the EMA followed the model
            assert not torch.equal(got[k], start[k]), (fused, k)
        losses.append(ls)
    print("losses (torch.optim.SGD, gims_amd.optim.SGD):", losses)
    assert losses[0][-1] < losses[0][0]
    assert np.allclose(losses[0], losses[1], rtol=1e-4, atol=1e-6), losses
