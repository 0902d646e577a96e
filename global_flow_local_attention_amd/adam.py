"""Adam / AdamW as one batched op per parameter group (csrc/adam.hip, include/gfla_adam.h).

torch.optim.Adam steps a group of tensors with a dozen launches, and under a GradScaler an unscale pass over every
gradient and a host-side decision come first.  FusedAdam steps a group with one kernel launch (and a one-wave launch that
advances the step counter): the gradients are unscaled inside the kernel, a step with inf / NaN gradients is skipped
inside the kernel, and nothing in step() waits for the device.

    FusedAdam     the optimizer: float32 parameters, or float16 / bfloat16 parameters behind float32 master copies

State: per group two flat float32 buffers (exp_avg, exp_avg_sq), a third for the master copies of 16-bit parameters, and
one device step counter; state[p]["exp_avg"], ["exp_avg_sq"] and ["master_param"] are views in the parameter's shape,
state[p]["step"] is the group's counter.  state_dict() / load_state_dict() interchange with torch.optim.Adam and AdamW.
"""
import ctypes
import operator

import torch

from . import _lib

_DEFAULT_KEYS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                     decoupled_weight_decay=False)
_ALIGN = 4            # every view into a flat buffer starts at a multiple of 4 floats: 16 bytes
_dtype, _grad = operator.attrgetter("dtype"), operator.attrgetter("grad")
_data_ptr, _contiguous, _get_device = torch.Tensor.data_ptr, torch.Tensor.is_contiguous, torch.Tensor.get_device


def _signature(params):
    """what a plan is built for: these parameter objects, their dtype, device and shapes"""
    return (tuple(map(id, params)), params[0].dtype, params[0].device, tuple(p.shape for p in params))


class _Plan(object):
    """What a group's step needs beside its hyper-parameters: the flat buffers, the step counter, the device table with
    the host numbers that go with it, and two pinned staging buffers for the table's uploads."""

    def __init__(self, params, device, masters):
        n = len(params)
        self.signature = _signature(params)
        self.device, self.dtype, self.n, self.masters = device, params[0].dtype, n, masters
        self.offsets, at = [], 0
        for p in params:
            self.offsets.append(at)
            at += -(-p.numel() // _ALIGN) * _ALIGN
        self.exp_avg = torch.zeros(at, dtype=torch.float32, device=device)
        self.exp_avg_sq = torch.zeros(at, dtype=torch.float32, device=device)
        self.master = torch.zeros(at, dtype=torch.float32, device=device) if masters else None
        self.step = torch.zeros((), dtype=torch.float32, device=device)
        self.numels = (ctypes.c_int64 * n)(*[p.numel() for p in params])
        self.param_ptrs = None                       # the parameter addresses the parameters were last examined at
        self.rows, self.table, self.uploaded = None, None, None
        self.staging, self.cells, self.events, self.turn = [None, None], [None, None], [None, None], 0

    def view(self, flat, i, p):
        return flat[self.offsets[i]:self.offsets[i] + p.numel()].view(p.shape)

    def build_table(self, params):
        """the constant columns, once per plan; needs the library"""
        first, totals = (ctypes.c_int64 * self.n)(), (ctypes.c_int64 * 1)()
        status = _lib.lib().gfla_adam_layout(ctypes.addressof(self.numels), self.n, ctypes.addressof(first),
                                             ctypes.addressof(totals))
        if status != 0:
            err = _lib.Unsupported if status == _lib._ERR_UNSUPPORTED else ValueError
            raise err("FusedAdam: %s" % _lib.lib().gfla_status_string(status).decode())
        self.table = torch.empty((self.n, 8), dtype=torch.int64, device=self.device)
        self.rows = torch.tensor([[0, 0, self.view(self.exp_avg, i, p).data_ptr(), self.view(self.exp_avg_sq, i, p).data_ptr(),
                                   self.view(self.master, i, p).data_ptr() if self.masters else 0, p.numel(), first[i], 0]
                                  for i, p in enumerate(params)], dtype=torch.int64)

    def upload(self, param_ptrs, grad_ptrs):
        """the table with this step's parameter and gradient addresses: two strided writes into a pinned buffer and one
        copy from it on the current stream.  Two buffers take turns, each behind the event of its last copy, so a buffer
        is never overwritten while a copy may still read it."""
        turn = self.turn
        self.turn = 1 - turn
        if self.staging[turn] is None:
            self.staging[turn] = torch.empty((self.n, 8), dtype=torch.int64, pin_memory=True)
            self.staging[turn].copy_(self.rows)
            self.cells[turn] = (ctypes.c_int64 * (8 * self.n)).from_address(self.staging[turn].data_ptr())
            self.events[turn] = torch.cuda.Event()
        elif not self.events[turn].query():
            self.events[turn].synchronize()
        self.cells[turn][0::8] = param_ptrs
        self.cells[turn][1::8] = grad_ptrs
        self.table.copy_(self.staging[turn], non_blocking=True)          # on the current stream of the table's device
        self.events[turn].record(torch.cuda.current_stream(self.device))
        self.uploaded = (param_ptrs, grad_ptrs)


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam's arithmetic (decoupled_weight_decay=True: AdamW's) on the library's kernel: one call per
    parameter group and step, whatever the number of tensors.

    Parameters of a group share one dtype -- float32, float16 or bfloat16 --, one device and one step counter; a parameter
    whose grad is None is left untouched by that step.  16-bit parameters are stepped on float32 master copies and stored
    as the master rounded to nearest even (master_weights=None, the default, or True); master_weights=False on 16-bit
    parameters is refused, and on float32 parameters masters are never kept.  amsgrad, maximize and sparse gradients are
    refused with ValueError; CPU parameters raise NotImplementedError at step() -- construction, state_dict() and
    load_state_dict() work on them.
    lr, betas, eps and weight_decay are read from param_groups at every step, so schedulers work.
    torch.amp.GradScaler: step() takes the scaler's grad_scale and found_inf as attributes (the contract of torch's fused
    optimizers), and the kernel unscales and skips: `scaler.step(opt); scaler.update()` works unchanged, the gradients in
    memory stay scaled, and nothing waits for the device."""

    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False,
                 decoupled_weight_decay=False, master_weights=None):
        if master_weights not in (None, True, False):
            raise ValueError("FusedAdam: master_weights is None, True or False (got %r)" % (master_weights,))
        self.master_weights = master_weights
        self._plans = {}
        defaults = dict(_DEFAULT_KEYS, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                        maximize=maximize, decoupled_weight_decay=decoupled_weight_decay)
        super(FusedAdam, self).__init__(params, defaults)

    # ---- groups ----------------------------------------------------------------------------------------------------------
    def _check_hyper(self, group):
        lr, (beta1, beta2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
        if isinstance(lr, torch.Tensor) or not float(lr) >= 0:
            raise ValueError("FusedAdam: lr is a number >= 0 (got %r)" % (lr,))
        if not (0 <= float(beta1) < 1 and 0 <= float(beta2) < 1):
            raise ValueError("FusedAdam: betas in [0, 1) (got %r)" % (group["betas"],))
        if not float(eps) > 0 or not float(wd) >= 0:
            raise ValueError("FusedAdam: eps > 0 and weight_decay >= 0 (got %r, %r)" % (eps, wd))
        if group.get("amsgrad") or group.get("maximize"):
            raise ValueError("FusedAdam: amsgrad and maximize are not offered")

    def _check_params(self, params):
        dtypes = set(map(_dtype, params))
        if len(dtypes) > 1:
            raise ValueError("FusedAdam: the parameters of a group share one dtype (got %s)"
                             % sorted(str(d) for d in dtypes))
        if dtypes and dtypes.pop() not in (torch.float32,) + _lib.HALF_TYPES:
            raise ValueError("FusedAdam: float32, float16 or bfloat16 parameters (got %s)" % params[0].dtype)
        if params and params[0].dtype in _lib.HALF_TYPES and self.master_weights is False:
            raise ValueError("FusedAdam: 16-bit parameters are stepped on float32 master copies; master_weights=False is "
                             "not offered")

    def _check_group(self, group):
        self._check_hyper(group)
        self._check_params(group["params"])

    def add_param_group(self, param_group):
        super(FusedAdam, self).add_param_group(param_group)
        self._check_group(self.param_groups[-1])

    def __setstate__(self, state):
        super(FusedAdam, self).__setstate__(state)
        self.__dict__.setdefault("master_weights", None)
        self.__dict__.setdefault("_plans", {})
        for group in self.param_groups:
            for key, value in _DEFAULT_KEYS.items():
                group.setdefault(key, value)

    # ---- state -----------------------------------------------------------------------------------------------------------
    def _plan(self, index, group, loaded=None):
        """The group's plan, built when the group is first stepped (or loaded), rebuilt -- from the state as it stands -- when
        its parameters, their dtype, device or shapes change.  `loaded`: {param: state} to start from instead."""
        params = group["params"]
        plan = self._plans.get(index)
        device = params[0].device
        if plan is not None and loaded is None and plan.signature == _signature(params):
            return plan
        for p in params:
            if p.device != device:
                raise ValueError("FusedAdam: the parameters of a group share one device (got %s and %s)" % (device, p.device))
            if not p.is_contiguous():
                raise ValueError("FusedAdam: contiguous parameters (got strides %s for shape %s)"
                                 % (p.stride(), tuple(p.shape)))
        old = {p: self.state[p] for p in params if len(self.state.get(p, {}))} if loaded is None else loaded
        steps = {float(s["step"]) for s in old.values() if "step" in s}
        if len(steps) > 1:
            raise ValueError("FusedAdam: the parameters of a group share one step counter (got steps %s)" % sorted(steps))
        plan = _Plan(params, device, masters=params[0].dtype in _lib.HALF_TYPES)
        plan.step.fill_(steps.pop() if steps else 0.0)
        for i, p in enumerate(params):
            s = old.get(p, {})
            for key, flat in (("exp_avg", plan.exp_avg), ("exp_avg_sq", plan.exp_avg_sq)):
                if key in s:
                    plan.view(flat, i, p).copy_(s[key])
            entry = {"step": plan.step, "exp_avg": plan.view(plan.exp_avg, i, p),
                     "exp_avg_sq": plan.view(plan.exp_avg_sq, i, p)}
            if plan.masters:
                entry["master_param"] = plan.view(plan.master, i, p)
                entry["master_param"].copy_(s["master_param"] if "master_param" in s else p.detach())
            self.state[p] = entry
        self._plans[index] = plan
        return plan

    def state_dict(self):
        """torch.optim.Adam's layout: per parameter `step` (a 0-d float32 tensor of its own), `exp_avg`, `exp_avg_sq`, and
        `master_param` where masters exist."""
        out = super(FusedAdam, self).state_dict()
        out["state"] = {k: dict(v, step=v["step"].clone()) if "step" in v else dict(v) for k, v in out["state"].items()}
        return out

    def load_state_dict(self, state_dict):
        """A state dict of this class, of torch.optim.Adam or of AdamW: `step` a number, a CPU or a device tensor.  Steps
        that differ within a group raise ValueError; parameters without state start from zero moments."""
        saved = [i for g in state_dict["param_groups"] for i in g["params"]]
        super(FusedAdam, self).load_state_dict(state_dict)
        own = [p for g in self.param_groups for p in g["params"]]
        # the tensors as saved: the base class casts state to the parameter's dtype, which would round the float32
        # moments and masters of 16-bit parameters
        loaded = {p: state_dict["state"][i] for i, p in zip(saved, own) if i in state_dict["state"]}
        self._plans = {}
        for index, group in enumerate(self.param_groups):
            self._check_group(group)
            mine = {p: loaded[p] for p in group["params"] if p in loaded}
            for p in group["params"]:
                self.state.pop(p, None)
            if mine:
                self._plan(index, group, loaded=mine)

    # ---- the step --------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        for index, group in enumerate(self.param_groups):
            params = group["params"]
            if not params:
                continue
            self._check_hyper(group)
            grads = list(map(_grad, params))
            present = [g for g in grads if g is not None]
            if not all(map(_contiguous, present)):               # which a sparse gradient is not either
                if any(g.is_sparse for g in present):
                    raise ValueError("FusedAdam: sparse gradients are not offered")
                grads = [g if g is None else g.contiguous() for g in grads]       # alive until the call is enqueued
                present = [g for g in grads if g is not None]
            # the parameters are examined when the group is first stepped and whenever an address among them has changed
            # (a new .data, a move to another device); the gradients, new tensors in most loops, at every step
            param_ptrs = list(map(_data_ptr, params))
            plan = self._plans.get(index)
            if plan is None or plan.param_ptrs != param_ptrs or plan.signature[0] != tuple(map(id, params)):
                self._check_params(params)
                _lib.require_gpu(*params)
                plan = self._plan(index, group)
                if plan.table is None:
                    plan.build_table(params)
                plan.param_ptrs = param_ptrs
            if present and (set(map(_dtype, present)) != {plan.dtype} or set(map(_get_device, present)) != {plan.device.index}):
                raise ValueError("FusedAdam: every gradient has its parameter's dtype and device (%s on %s)"
                                 % (plan.dtype, plan.device))
            grad_ptrs = [0 if g is None else g.data_ptr() for g in grads]
            if plan.uploaded != (param_ptrs, grad_ptrs):
                plan.upload(param_ptrs, grad_ptrs)
            scale, inf = (None if t is None else t.to(device=plan.device, dtype=torch.float32, non_blocking=True)
                          for t in (grad_scale, found_inf))
            beta1, beta2 = group["betas"]
            _lib.call("gfla_adam_step_" + _lib.suffix(params[0], "FusedAdam"), params[0], _lib.ptr(plan.table),
                      ctypes.c_void_p(ctypes.addressof(plan.numels)), plan.n, _lib.ptr(plan.step), _lib.ptr(scale),
                      _lib.ptr(inf), float(group["lr"]), float(beta1), float(beta2), float(group["eps"]),
                      float(group["weight_decay"]), 1 if group.get("decoupled_weight_decay") else 0)
        return loss
