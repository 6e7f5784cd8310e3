"""gims_amd.optim.SGD / ModelEMA / param_groups and their entry points gims_sgd_step / gims_ema_update (csrc/optim.hip) as far as they
can be checked without a GPU: argument rejection before any HIP call, the parameter-group rule of train.py:42-51, the constructors, and
the checkpoint layout train.py:155-160 writes.  (The table layouts are checked in test_host_cpu.py, on the harness every struct of the header shares.)"""
import math

import pytest
import torch

from gims_amd import GMatcher, hip
from gims_amd.optim import SGD, ModelEMA, param_groups

EINVAL, OK = -1, 0


def _sgd(tensors, groups, count=None, n_groups=None):
    """gims_sgd_step on tables of (param, grad, buf, n, group, first) / (lr, momentum, dampening, weight_decay, nesterov); -> (rc, message)."""
    lib = hip.load()
    tt = (hip.SgdTensor * max(len(tensors), 1))(*[hip.SgdTensor(*t) for t in tensors])
    gt = (hip.SgdGroup * max(len(groups), 1))(*[hip.SgdGroup(*g) for g in groups])
    rc = lib.gims_sgd_step(tt, len(tensors) if count is None else count, gt, len(groups) if n_groups is None else n_groups, None)
    return rc, lib.gims_last_error()


def _ema(tensors, decay, count=None):
    lib = hip.load()
    tt = (hip.EmaTensor * max(len(tensors), 1))(*[hip.EmaTensor(*t) for t in tensors])
    rc = lib.gims_ema_update(tt, len(tensors) if count is None else count, decay, None)
    return rc, lib.gims_last_error()


P, G, B = 0x1000, 0x2000, 0x3000          # never dereferenced: every call below is refused before any HIP call
GOOD_T = (P, G, B, 16, 0, 0)
GOOD_G = (0.1, 0.9, 0.0, 1e-4, 1, 0)


def test_sgd_step_rejects_bad_arguments_without_a_device():
    lib = hip.load()
    assert _sgd([], [], count=0, n_groups=0)[0] == OK                      # count == 0: nothing to do, nothing is looked at
    assert lib.gims_sgd_step(None, 0, None, 0, None) == OK
    gt = (hip.SgdGroup * 1)(hip.SgdGroup(*GOOD_G))
    tt = (hip.SgdTensor * 1)(hip.SgdTensor(*GOOD_T))
    assert lib.gims_sgd_step(None, 1, gt, 1, None) == EINVAL and b"gims_sgd_step" in lib.gims_last_error()      # null tables
    assert lib.gims_sgd_step(tt, 1, None, 1, None) == EINVAL
    assert lib.gims_sgd_step(tt, -1, gt, 1, None) == EINVAL
    bad = {
        "no groups": ([GOOD_T], [GOOD_G], dict(n_groups=0)),
        "nine groups": ([GOOD_T], [GOOD_G] * 9, {}),
        "negative n": ([(P, G, B, -1, 0, 0)], [GOOD_G], {}),
        "n = 2^31": ([(P, G, B, 1 << 31, 0, 0)], [GOOD_G], {}),
        "null param": ([(0, G, B, 16, 0, 0)], [GOOD_G], {}),
        "null grad": ([(P, 0, B, 16, 0, 0)], [GOOD_G], {}),
        "null buffer with momentum": ([(P, G, 0, 16, 0, 0)], [GOOD_G], {}),
        "group too large": ([(P, G, B, 16, 1, 0)], [GOOD_G], {}),
        "group negative": ([(P, G, B, 16, -1, 0)], [GOOD_G], {}),
        "negative lr": ([GOOD_T], [(-0.1, 0.9, 0.0, 0.0, 0, 0)], {}),
        "negative momentum": ([GOOD_T], [(0.1, -0.9, 0.0, 0.0, 0, 0)], {}),
        "negative weight decay": ([GOOD_T], [(0.1, 0.9, 0.0, -1e-4, 0, 0)], {}),
        "nesterov without momentum": ([GOOD_T], [(0.1, 0.0, 0.0, 0.0, 1, 0)], {}),
        "nesterov with dampening": ([GOOD_T], [(0.1, 0.9, 0.1, 0.0, 1, 0)], {}),
        "second tensor bad": ([GOOD_T, (P, G, B, 16, 2, 0)], [GOOD_G, GOOD_G], {}),
    }
    for what, (tensors, groups, kw) in bad.items():
        rc, msg = _sgd(tensors, groups, **kw)
        assert rc == EINVAL and b"gims_sgd_step" in msg, (what, rc, msg)
    # what is allowed is refused by nothing above: an empty tensor may carry null pointers (it is skipped, so no launch follows here)
    assert _sgd([(0, 0, 0, 0, 0, 0)], [GOOD_G])[0] == OK
    assert _sgd([(0, 0, 0, 0, 0, 0)], [(0.1, 0.0, 0.0, 0.0, 0, 0)])[0] == OK


def test_ema_update_rejects_bad_arguments_without_a_device():
    lib = hip.load()
    assert lib.gims_ema_update(None, 0, 0.5, None) == OK
    assert lib.gims_ema_update(None, 1, 0.5, None) == EINVAL and b"gims_ema_update" in lib.gims_last_error()
    assert _ema([(P, G, 16)], 0.5, count=-1)[0] == EINVAL
    bad = {
        "negative n": ([(P, G, -1)], 0.5),
        "n = 2^31": ([(P, G, 1 << 31)], 0.5),
        "null ema": ([(0, G, 16)], 0.5),
        "null model": ([(P, 0, 16)], 0.5),
        "decay below 0": ([(P, G, 16)], -1e-9),
        "decay above 1": ([(P, G, 16)], 1.0 + 1e-9),
        "decay nan": ([(P, G, 16)], float("nan")),
        "ema is model": ([(P, G, 16), (P, P, 16)], 0.5),
    }
    for what, (tensors, decay) in bad.items():
        rc, msg = _ema(tensors, decay)
        assert rc == EINVAL and b"gims_ema_update" in msg, (what, rc, msg)
    assert _ema([(0, 0, 0)], 0.0)[0] == OK and _ema([(0, 0, 0)], 1.0)[0] == OK


@pytest.mark.parametrize("use_layernorm, counts", [(False, (23, 120, 139)), (True, (1, 120, 117))])
def test_param_groups_follow_the_rule_of_the_training_script(use_layernorm, counts):
    """train.py:42-51.  Default model: 22 BatchNorm weights + bin_score / 120 other weights / 139 biases = all 282 parameters.
    use_layernorm: the 22 norms are LayerNorms whose parameters are called a_2 / b_2, which the rule (it looks for .weight / .bias)
    puts nowhere: bin_score alone / the same 120 weights / 139 - 22 = 117 biases, 238 of 282."""
    m = GMatcher({"use_layernorm": use_layernorm})
    pg = param_groups(m)
    assert tuple(len(g) for g in pg) == counts
    ids = [id(p) for g in pg for p in g]
    assert len(set(ids)) == len(ids)                                       # disjoint
    named = dict(m.named_parameters())
    assert len(named) == 282
    in0, in1, in2 = ({id(p) for p in g} for g in pg)
    assert id(m.bin_score) in in0
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            assert id(mod.weight) in in0
    for name, p in named.items():
        if name.endswith(".bias"):
            assert id(p) in in2, name
        elif name.endswith(".weight"):
            assert id(p) in (in0 | in1), name
    left_out = [n for n, p in named.items() if id(p) not in (in0 | in1 | in2)]
    if use_layernorm:
        assert len(left_out) == 44 and all(n.endswith((".a_2", ".b_2")) for n in left_out)
    else:
        assert left_out == [] and sum(counts) == 282
    # the one-line replacements for train.py:53-57 work for both optimizers
    from gims_amd.optim import Adam
    for opt in (Adam(pg[0], lr=1e-4, betas=(0.9, 0.999)), SGD(pg[0], lr=1e-4, momentum=0.9, nesterov=True)):
        opt.add_param_group({'params': pg[1], 'weight_decay': 5e-4})
        opt.add_param_group({'params': pg[2]})
        assert [len(g['params']) for g in opt.param_groups] == list(counts) and opt.param_groups[1]['weight_decay'] == 5e-4


def test_sgd_constructor_and_cpu_refusal():
    p = [torch.nn.Parameter(torch.zeros(4))]
    for kw in (dict(lr=-1.0), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1.0), dict(lr=0.1, nesterov=True),
               dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError):
            SGD(p, **kw)
        with pytest.raises(ValueError):                                    # as in torch
            torch.optim.SGD(p, **kw)
    for kw in (dict(maximize=True), dict(differentiable=True)):
        with pytest.raises(NotImplementedError):
            SGD(p, lr=0.1, **kw)
    o, t = SGD(p, lr=0.1, momentum=0.9, nesterov=True), torch.optim.SGD(p, lr=0.1, momentum=0.9, nesterov=True)
    assert set(o.param_groups[0].keys()) == set(t.param_groups[0].keys())
    for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize"):
        assert o.param_groups[0][k] == t.param_groups[0][k], k
    assert SGD(p).defaults["lr"] == torch.optim.SGD(p).defaults["lr"] and SGD(p).defaults["momentum"] == 0
    o.add_param_group({'params': [torch.nn.Parameter(torch.zeros(2))], 'weight_decay': 0.5})       # train.py:56
    assert len(o.param_groups) == 2 and o.param_groups[1]['momentum'] == 0.9 and o.param_groups[1]['nesterov'] is True
    assert o.state_dict()['state'] == {}
    o.step()                                                               # no gradients: nothing to do, also without a GPU
    p[0].grad = torch.ones(4)
    with pytest.raises(RuntimeError):
        o.step()
    o.param_groups[0]['maximize'] = True
    with pytest.raises(NotImplementedError):
        o.step()


def test_model_ema_is_built_from_config_and_state(synth_sd):
    m = GMatcher({"sinkhorn_iterations": 20})
    m.load_state_dict(synth_sd)
    m.train()
    ema = ModelEMA(m, updates=7)
    assert isinstance(ema.ema, GMatcher) and ema.ema is not m and not ema.ema.training and m.training
    assert ema.updates == 7 and ema.ema.config["sinkhorn_iterations"] == 20 and ema.ema.config["weights_path"] is None
    assert all(not p.requires_grad for p in ema.ema.parameters()) and all(p.requires_grad for p in m.parameters())
    a, b = ema.ema.state_dict(), m.state_dict()
    assert list(a.keys()) == list(b.keys()) and len(a) == 348
    ptrs = {v.untyped_storage().data_ptr() for v in b.values()}
    for k in a:
        assert torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
        assert a[k].untyped_storage().data_ptr() not in ptrs, k
    for k, want in ((1, 0.9999 * (1 - math.exp(-1 / 4000))), (4000, 0.9999 * (1 - math.exp(-1.0))), (10 ** 6, 0.9999 * (1 - math.exp(-250.0)))):
        assert ema.decay(k) == want
    assert ModelEMA(m, decay=0.5).decay(4000) == 0.5 * (1 - math.exp(-1.0))
    with pytest.raises(RuntimeError):                                      # no CPU path
        ema.update(m)
    wrapped = torch.nn.DataParallel(m)                                     # train.py:62 hands over the bare model, :141 the wrapped one
    assert torch.equal(ModelEMA(wrapped).ema.bin_score, m.bin_score)
    m.some_attribute = 3
    ema.update_attr(m, include=("some_attribute",))
    assert ema.ema.some_attribute == 3


def test_checkpoint_of_the_training_loop_loads_the_ema_weights(tmp_path, synth_sd):
    """train.py:155-160 saves {'ema': ema.ema.state_dict(), 'ema_updates': ..., 'model': ...}; GMatcher prefers 'ema' (gmatcher.py:178-184)."""
    m = GMatcher({})
    m.load_state_dict(synth_sd)
    ema = ModelEMA(m)
    with torch.no_grad():
        ema.ema.bin_score.fill_(2.5)                                       # the two weight sets differ
        ema.ema.state_dict()["gnn.layers.3.mlp.1.running_var"].mul_(3.0)
    path = tmp_path / "lastiter.pt"
    torch.save({'epoch': 0, 'iter': 1, 'ema': ema.ema.state_dict(), 'ema_updates': ema.updates, 'model': m.state_dict(), 'optimizer': None}, path)
    loaded = GMatcher({"weights_path": str(path)})
    want, other = ema.ema.state_dict(), m.state_dict()
    for k, v in loaded.state_dict().items():
        assert torch.equal(v, want[k]), k
    assert float(loaded.bin_score.detach()) == 2.5 != float(other["bin_score"])
