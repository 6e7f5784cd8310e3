"""Optimizers and EMA weights of the reference's training loop on the HIP path.

train.py:52-57 builds ``optim.Adam(pg0, lr, betas=(0.9, 0.999))`` and adds two more parameter groups (weights with weight decay,
biases); train.py:138 calls ``optimizer.step()`` once per pair.  ``Adam`` below is that optimizer with the same constructor, the same
``param_groups`` / ``add_param_group`` / ``state_dict`` (state per parameter: ``step``, ``exp_avg``, ``exp_avg_sq`` -- a checkpoint
written by ``torch.optim.Adam`` loads and vice versa) and the same arithmetic, but ONE fused multi-tensor launch sequence per step
(``gims_adam_step``, csrc/optim.hip) instead of torch's per-operation list kernels: the 282 tensors of a GMatcher take 4 launches.

``SGD`` is the other optimizer train.py builds (``opt_type: sgd``, train.py:55: ``optim.SGD(pg0, lr, momentum=0.9, nesterov=True)``;
state per parameter: ``momentum_buffer``), ``ModelEMA`` the exponential moving average of the weights that train.py:60-62, 141 keeps
when ``use_ema`` is set (utils/common.py:990-1019) -- the weight set every checkpoint is loaded from --, and ``param_groups`` the
split of train.py:42-51.  Each is one fused multi-tensor launch sequence per call (``gims_sgd_step``, ``gims_ema_update``).

    from gims_amd.optim import Adam, SGD, ModelEMA, param_groups       # instead of train.py:17's ModelEMA and optim.Adam / optim.SGD
    pg0, pg1, pg2 = param_groups(gmodel)                               # train.py:42-51
    optimizer = Adam(pg0, lr=lr, betas=(0.9, 0.999)) if adam else SGD(pg0, lr=lr, momentum=0.9, nesterov=True)      # train.py:52-55

One process, one GPU: averaging gradients across ranks is not built.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

from . import hip

__all__ = ["Adam", "SGD", "ModelEMA", "param_groups"]


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's interface and update rule (L2 weight decay added to the gradient, bias-corrected moments); ``amsgrad``,
    ``maximize``, ``capturable``, ``differentiable`` and sparse gradients are not built and raise.  Parameters must be float32 tensors
    on the GPU: there is no CPU path."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None):
        if amsgrad or maximize or capturable or differentiable:
            raise NotImplementedError("gims_amd.optim.Adam: amsgrad / maximize / capturable / differentiable are not built")
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("gims_amd.optim.Adam: lr must be a Python number")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                                      capturable=False, differentiable=False, fused=None))

        self._plan = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plan = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._plan = None

    def _make_plan(self, active):
        """Everything about a step that does not change while the same parameters receive gradients: the pointer table (only its
        `grad` column is refreshed per step), the step tensors, and the (param group, step count) classes that share one set of
        bias corrections."""
        classes, cls_of, rows, counts = [], {}, [], []
        for gi, p in active:
            if not p.is_cuda or p.dtype != torch.float32:
                raise RuntimeError("gims_amd.optim.Adam needs float32 parameters on the GPU (no CPU path)")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)               # torch's layout: a CPU scalar tensor per parameter
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if not torch.is_tensor(st["step"]):
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
            if st["step"].is_cuda:
                raise NotImplementedError("gims_amd.optim.Adam: capturable state (step on the GPU) is not built")
            m, v = st["exp_avg"], st["exp_avg_sq"]
            if not (p.is_contiguous() and m.is_contiguous() and v.is_contiguous()) or m.dtype != torch.float32 or v.dtype != torch.float32 or not m.is_cuda:
                raise RuntimeError("gims_amd.optim.Adam needs contiguous float32 parameters and moments on the GPU")
            key = (gi, int(st["step"].item()))
            if key not in cls_of:
                cls_of[key] = len(classes)
                classes.append([gi, key[1]])
            counts.append(float(key[1]))
            rows.append((p.data_ptr(), 0, m.data_ptr(), v.data_ptr(), p.numel(), cls_of[key], 0))
        table = np.array(rows, dtype=hip.ADAM_TENSOR_DTYPE)
        # the per-parameter step counts (CPU scalars in torch's layout) become views into ONE vector, so that a step increments them
        # with one operation (282 separate scalars: 0.4 ms per step); distinct elements -- an in-place update through any one of
        # them, e.g. by torch.optim.Adam after loading this optimizer's state_dict, touches only its own.  A parameter that drops
        # out of the active set keeps its view into the vector of the plan it was last part of.
        steps = torch.tensor(counts, dtype=torch.float32)
        for i, (_, p) in enumerate(active):
            self.state[p]["step"] = steps[i]
        return dict(ids=[id(p) for _, p in active], ptrs=table["param"].tolist(), table=table, classes=classes, steps=steps)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        active, grads = [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    active.append((gi, p))
                    grads.append(g)
        if not active:
            return loss
        plan = self._plan
        # the plan holds raw pointers: it is rebuilt when the set of parameters with gradients or a parameter's storage changes
        # (load_state_dict / add_param_group drop it; replacing a moment tensor in .state by hand is not detected)
        if plan is None or plan["ids"] != [id(p) for _, p in active] or plan["ptrs"] != [p.data_ptr() for _, p in active]:
            plan = self._plan = self._make_plan(active)
        keep = []
        for i, g in enumerate(grads):
            if g.is_sparse:
                raise RuntimeError("Adam does not support sparse gradients")
            if not g.is_cuda or g.dtype != torch.float32:
                raise RuntimeError("gims_amd.optim.Adam needs float32 gradients on the GPU (no CPU path)")
            if not g.is_contiguous():
                grads[i] = g.contiguous()
                keep.append(grads[i])
        table = plan["table"]
        table["grad"] = [g.data_ptr() for g in grads]
        plan["steps"] += 1
        hyper = []
        for c in plan["classes"]:
            c[1] += 1
            group = self.param_groups[c[0]]
            if group.get("amsgrad") or group.get("maximize"):
                raise NotImplementedError("gims_amd.optim.Adam: amsgrad / maximize are not built")
            hyper.append(dict(lr=group["lr"], beta1=group["betas"][0], beta2=group["betas"][1], eps=group["eps"], weight_decay=group["weight_decay"], step=c[1]))
        if len(hyper) <= 8:
            hip.adam_step(table, hyper)
        else:
            for lo in range(0, len(hyper), 8):
                sel = table[(table["group"] >= lo) & (table["group"] < lo + 8)].copy()
                sel["group"] -= lo
                hip.adam_step(np.ascontiguousarray(sel), hyper[lo:lo + 8])
        # the kernel wrote the parameters through raw pointers: bump their version counters as an in-place torch op would, so that
        # caches keyed on them (GMatcher's packed weights, bin_score among them) see the update
        torch.autograd.graph.increment_version([p for _, p in active])
        return loss


class SGD(torch.optim.Optimizer):
    """torch.optim.SGD's interface and update rule (L2 weight decay added to the gradient, momentum with dampening, Nesterov);
    ``maximize``, ``differentiable`` and sparse gradients are not built and raise.  Parameters must be float32 tensors on the GPU: there
    is no CPU path.  A group with ``momentum == 0`` keeps no state, as in torch."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        if maximize or differentiable:
            raise NotImplementedError("gims_amd.optim.SGD: maximize / differentiable are not built")
        if isinstance(lr, torch.Tensor) or isinstance(weight_decay, torch.Tensor):
            raise NotImplementedError("gims_amd.optim.SGD: lr and weight_decay must be Python numbers")
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=False,
                                      foreach=None, differentiable=False, fused=None))
        self._plan = None
        self._unwritten = set()            # ids of parameters whose momentum buffer is allocated but not yet written by a step

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plan = None
        self._unwritten = set()

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._plan = None

    def _make_plan(self, active, with_momentum):
        """Everything about a step that does not change while the same parameters receive gradients: the pointer table (only its
        `grad` and `first` columns are refreshed per step) and the param groups that take part, in slices of 8."""
        classes, cls_of, rows = [], {}, []
        for gi, p in active:
            if not p.is_cuda or p.dtype != torch.float32:
                raise RuntimeError("gims_amd.optim.SGD needs float32 parameters on the GPU (no CPU path)")
            if not p.is_contiguous():
                raise RuntimeError("gims_amd.optim.SGD needs contiguous float32 parameters on the GPU")
            buf_ptr, first = 0, 0
            if with_momentum[gi]:
                st = self.state[p]
                buf = st.get("momentum_buffer")
                if buf is None:                    # torch: buf = grad.clone() on the first step; here the kernel writes it (first = 1)
                    buf = st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                    self._unwritten.add(id(p))
                elif not buf.is_contiguous():      # a checkpoint of torch's: the clone of a non-contiguous gradient
                    buf = st["momentum_buffer"] = buf.contiguous()
                if buf.dtype != torch.float32 or not buf.is_cuda or buf.shape != p.shape:
                    raise RuntimeError("gims_amd.optim.SGD needs float32 momentum buffers of the parameters' shapes on the GPU")
                buf_ptr, first = buf.data_ptr(), int(id(p) in self._unwritten)
            if gi not in cls_of:
                cls_of[gi] = len(classes)
                classes.append(gi)
            rows.append((p.data_ptr(), 0, buf_ptr, p.numel(), cls_of[gi], first))
        table = np.array(rows, dtype=hip.SGD_TENSOR_DTYPE)
        slices = None
        if len(classes) > 8:
            slices = [np.flatnonzero((table["group"] >= lo) & (table["group"] < lo + 8)) for lo in range(0, len(classes), 8)]
        return dict(ids=[id(p) for _, p in active], ptrs=table["param"].tolist(), table=table, classes=classes, slices=slices,
                    with_momentum=with_momentum, pending_first=bool(table["first"].any()))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        active, grads = [], []
        for gi, group in enumerate(self.param_groups):
            if group.get("maximize") or group.get("differentiable"):
                raise NotImplementedError("gims_amd.optim.SGD: maximize / differentiable are not built")
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    active.append((gi, p))
                    grads.append(g)
        if not active:
            return loss
        with_momentum = [group["momentum"] != 0 for group in self.param_groups]
        plan = self._plan
        # the plan holds raw pointers: it is rebuilt when the set of parameters with gradients, a parameter's storage or a group's use of
        # a momentum buffer changes (load_state_dict / add_param_group drop it; replacing a buffer in .state by hand is not detected)
        if (plan is None or plan["ids"] != [id(p) for _, p in active] or plan["ptrs"] != [p.data_ptr() for _, p in active]
                or plan["with_momentum"] != with_momentum):
            plan = self._plan = self._make_plan(active, with_momentum)
        keep = []
        for i, g in enumerate(grads):
            if g.is_sparse:
                raise RuntimeError("gims_amd.optim.SGD does not support sparse gradients")
            if not g.is_cuda or g.dtype != torch.float32:
                raise RuntimeError("gims_amd.optim.SGD needs float32 gradients on the GPU (no CPU path)")
            if not g.is_contiguous():
                grads[i] = g.contiguous()
                keep.append(grads[i])
        table = plan["table"]
        table["grad"] = [g.data_ptr() for g in grads]
        hyper = []
        for gi in plan["classes"]:
            group = self.param_groups[gi]                  # read every step: train.py:21-26, 102-105 rewrite lr
            hyper.append(dict(lr=group["lr"], momentum=group["momentum"], dampening=group["dampening"], weight_decay=group["weight_decay"],
                              nesterov=group["nesterov"]))
        if plan["slices"] is None:
            hip.sgd_step(table, hyper)
        else:
            for k, rows in enumerate(plan["slices"]):
                sel = table[rows]
                sel["group"] -= 8 * k
                hip.sgd_step(np.ascontiguousarray(sel), hyper[8 * k:8 * k + 8])
        if plan["pending_first"]:                          # every buffer of this plan now holds a value
            table["first"] = 0
            plan["pending_first"] = False
            self._unwritten.clear()
        # the kernel wrote the parameters through raw pointers: bump their version counters as an in-place torch op would, so that
        # caches keyed on them (GMatcher's packed weights, bin_score among them) see the update
        torch.autograd.graph.increment_version([p for _, p in active])
        return loss


def param_groups(model):
    """(pg0, pg1, pg2) by the rule of train.py:42-51: bin_score and BatchNorm weights / the other ``weight`` parameters (the group
    train.py:56 gives the weight decay) / every ``bias``.  With ``use_layernorm`` the norms' ``a_2`` / ``b_2`` are in none of the
    three, as in the reference."""
    nn = torch.nn
    pg0, pg1, pg2 = [], [], []
    for _, v in model.named_modules():
        if hasattr(v, 'bias') and isinstance(v.bias, nn.Parameter):
            pg2.append(v.bias)
        if hasattr(v, 'bin_score'):
            pg0.append(v.bin_score)
        if isinstance(v, (nn.BatchNorm2d, nn.BatchNorm1d, nn.SyncBatchNorm)):
            pg0.append(v.weight)
        elif hasattr(v, 'weight') and isinstance(v.weight, nn.Parameter):
            pg1.append(v.weight)
    return pg0, pg1, pg2


def _unwrap(model):
    return model.module if isinstance(model, (torch.nn.DataParallel, torch.nn.parallel.DistributedDataParallel)) else model


class ModelEMA:
    """The reference's ModelEMA (utils/common.py:990-1019): ``.ema`` is a second GMatcher holding the exponential moving average of
    every floating state-dict entry of the model (parameters and BatchNorm running statistics), ``update(model)`` after every
    optimizer step moves it by ``decay(updates) = decay * (1 - exp(-updates / 4000))``.  ``.ema`` is built from the model's config and
    state dict (no deep copy of the model's packed-weight caches), and ``update`` is one ``gims_ema_update`` over all entries -- five
    launches for a GMatcher instead of three torch operations per entry.  Tensors must be float32 on the GPU: there is no CPU path."""

    def __init__(self, model, decay=0.9999, updates=0):
        from .gmatcher import GMatcher
        model = _unwrap(model)
        cfg = copy.deepcopy({k: v for k, v in model.config.items() if k != 'weights_path'})
        ema = GMatcher(cfg)
        p = next(model.parameters(), None)
        if p is not None:
            ema.to(p.device)
        ema.load_state_dict(model.state_dict())          # copies values into the EMA model's own storage
        self.ema = ema.eval()
        self.updates = updates
        self.decay = lambda x: decay * (1 - math.exp(-x / 4000))      # exponential ramp (to help early epochs)
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self._plan = None

    def update(self, model):
        model = _unwrap(model)
        ours, theirs = self.ema._float_state(), model._float_state()
        plan = self._plan
        # the plan holds raw pointers: rebuilt when a tensor of either side is replaced or moves
        if plan is None or plan["ema"] is not ours or plan["model"] is not theirs or plan["ptrs"] != [t.data_ptr() for t in ours + theirs]:
            if len(ours) != len(theirs):
                raise RuntimeError("gims_amd.optim.ModelEMA: the model's state does not match the EMA model's")
            for a, b in zip(ours, theirs):
                if not (a.is_cuda and b.is_cuda) or a.dtype != torch.float32 or b.dtype != torch.float32:
                    raise RuntimeError("gims_amd.optim.ModelEMA needs float32 tensors on the GPU (no CPU path)")
                if a.shape != b.shape or a.device != b.device or not (a.is_contiguous() and b.is_contiguous()):
                    raise RuntimeError("gims_amd.optim.ModelEMA needs contiguous tensors of equal shapes on one device")
            table = np.array([(a.data_ptr(), b.data_ptr(), a.numel()) for a, b in zip(ours, theirs)], dtype=hip.EMA_TENSOR_DTYPE)
            plan = self._plan = dict(ema=ours, model=theirs, ptrs=[t.data_ptr() for t in ours + theirs], table=table)
        self.updates += 1
        hip.ema_update(plan["table"], self.decay(self.updates))
        # written through raw pointers: bump the version counters as the reference's in-place operations would.  GMatcher's packed
        # weights are keyed on the parameters' versions only, and the BatchNorm running statistics are folded into them: drop the pack
        torch.autograd.graph.increment_version(ours)
        self.ema._pack = None
        self.ema.__dict__.pop("_ops_cache", None)

    def update_attr(self, model, include=(), exclude=('process_group', 'reducer')):
        """Copy the model's public attributes to the EMA model (utils/common.py:982-988, copy_attr)."""
        for k, v in model.__dict__.items():
            if (len(include) and k not in include) or k.startswith('_') or k in exclude:
                continue
            setattr(self.ema, k, v)
