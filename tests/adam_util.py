"""Shared by the CPU and GPU tests of FusedAdam (global_flow_local_attention_amd/adam.py): the inputs, the float64
references and the per-element bars.

References.  torch_reference: torch.optim.Adam / AdamW with foreach=False, fused=False on the CPU in float64, fed the same
float32-representable inputs.  restate: include/gfla_adam.h's formulas in float64, for what torch has no switch for -- a
gradient scale, a skipped step, master copies, and ONE step counter per group (torch counts per parameter, so a tensor that
missed a gradient falls behind its group there; per_tensor_step=True restates that, for the anchor against torch).
tests/test_adam_cpu.py anchors restate on torch_reference to 1e-14 relative wherever both apply.

Bars, per element, from the float64 run alone (T: the steps in which the tensor had a gradient):
  parameter / master   sum over those steps of 2 ulp32(max(|p_before|, |p_after|)) + 16 2^-24 max(|dp|, lr): a step rounds
                       p twice (decay, update) by half an ulp each, and this allows twice that; the second term covers a
                       six-operation update whose moment may cancel
  exp_avg              4 T 2^-24 G, G the largest |g'| the element saw (unscaled, with wd |p| under L2 decay): not relative
                       to the moment, which can cancel to zero
  exp_avg_sq           4 T 2^-24 G^2
"""
import functools
import math

import torch

LR, EPS, STEPS = 1e-4, 1e-8, 5
# (betas, weight_decay, decoupled)
CONFIGS = (((0.0, 0.999), 0.0, False), ((0.9, 0.999), 0.0, False), ((0.5, 0.9), 0.01, False), ((0.0, 0.999), 0.01, True),
           ((0.9, 0.999), 0.01, True))
HALF_CONFIGS = (CONFIGS[0], CONFIGS[4])        # the two configurations the 16-bit storage types run
NONE_TENSOR, NONE_STEP = 5, 1                  # this tensor has grad = None in the second step (index 1)
ZERO_TENSOR = 8                                # every seventh gradient element of this tensor is exactly 0
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def chunk():
    from global_flow_local_attention_amd import _lib
    return int(_lib.lib().gfla_adam_chunk_elems())


def shapes():
    c = chunk()
    return [(1,), (3,), (4,), (5,), (63,), (64,), (65,), (c - 1,), (c,), (c + 1,), (2 * c + 1,), (3, 5, 3, 3)]


def make_inputs(shape_list, dtype=torch.float32, seed=0, steps=STEPS, with_none=True):
    """(params, grads): params[k] = 0.1 randn, grads[s][k] = 10^(2 (k mod 5) - 6) randn, both rounded to `dtype` and held
    as float32 CPU tensors (exactly representable in the storage type)."""
    g = torch.Generator().manual_seed(seed)
    params = [(0.1 * torch.randn(s, generator=g)).to(dtype).float() for s in shape_list]
    grads = []
    for s in range(steps):
        row = []
        for k, shape in enumerate(shape_list):
            t = (10.0 ** (2 * (k % 5) - 6) * torch.randn(shape, generator=g)).to(dtype).float()
            if k == ZERO_TENSOR:
                t.view(-1)[::7] = 0.0
            row.append(None if with_none and (s, k) == (NONE_STEP, NONE_TENSOR) else t)
        grads.append(row)
    return params, grads


def ulp32(x):
    """spacing of float32 at |x| (float64 tensor in, float64 out)"""
    _, e = torch.frexp(x.abs().double())
    e = torch.where(x == 0, torch.full_like(e, -200), e)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), (e - 24).clamp(min=-149))


class Trace(object):
    """p, m, v: the float64 results per tensor; bar_p, bar_m, bar_v: the bars; step: the group's count"""


def restate(params, grads, config, lr=LR, eps=EPS, grad_scale=None, skip=(), per_tensor_step=False):
    (beta1, beta2), wd, decoupled = config
    n = len(params)
    p = [x.double().clone() for x in params]
    m, v = [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p]
    bar_p, big = [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p]
    had, group_t = [0] * n, 0
    for s, row in enumerate(grads):
        if s in skip:
            continue
        group_t += 1
        for k, g in enumerate(row):
            if g is None:
                continue
            had[k] += 1
            t = had[k] if per_tensor_step else group_t
            bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
            g = g.double()
            if grad_scale is not None:
                g = g * (1.0 / grad_scale)
            before = p[k].clone()
            if decoupled:
                p[k] = p[k] * (1 - lr * wd)
            elif wd != 0:
                g = g + wd * p[k]
            m[k] = m[k] + (g - m[k]) * (1 - beta1)
            v[k] = beta2 * v[k] + (1 - beta2) * g * g
            p[k] = p[k] - (lr / bc1) * m[k] / (v[k].sqrt() / math.sqrt(bc2) + eps)
            moved = (p[k] - before).abs().clamp(min=lr)
            bar_p[k] = bar_p[k] + 2 * ulp32(torch.maximum(before.abs(), p[k].abs())) + 16 * U * moved
            big[k] = torch.maximum(big[k], g.abs())
    out = Trace()
    out.p, out.m, out.v, out.step = p, m, v, group_t
    out.bar_p = bar_p
    out.bar_m = [4 * had[k] * U * big[k] for k in range(n)]
    out.bar_v = [4 * had[k] * U * big[k] ** 2 for k in range(n)]
    return out


def torch_reference(params, grads, config, lr=LR, eps=EPS, divide=None, skip=(), dtype=torch.float64):
    """(p, m, v) of torch's for-loop Adam / AdamW in `dtype` on the CPU; divide: every gradient is divided by it first"""
    (beta1, beta2), wd, decoupled = config
    ps = [torch.nn.Parameter(x.to(dtype).clone()) for x in params]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(ps, lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=wd, foreach=False, fused=False)
    for s, row in enumerate(grads):
        if s in skip:
            continue
        for q, g in zip(ps, row):
            q.grad = None if g is None else (g.to(dtype) if divide is None else g.to(dtype) / divide)
        opt.step()
    zero = [torch.zeros_like(q) for q in ps]
    return ([q.detach() for q in ps], [opt.state[q].get("exp_avg", z) for q, z in zip(ps, zero)],
            [opt.state[q].get("exp_avg_sq", z) for q, z in zip(ps, zero)])


def worst(got, want, bar, mask=None):
    """largest |got - want| / bar over the elements (mask: only where True); an element off a zero bar counts as inf"""
    err = (got.double().cpu() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    if mask is not None:
        ratio = ratio[mask]
    return float(ratio.max()) if ratio.numel() else 0.0


def check_within(trace, got_p, got_m, got_v, what, wants=None, masks=None):
    """every tensor's p (or master), m and v within the bars of `trace`; wants: (p, m, v) lists to compare against
    instead of the trace's own; masks[k]: the elements of tensor k to look at"""
    want_p, want_m, want_v = wants if wants is not None else (trace.p, trace.m, trace.v)
    for k in range(len(trace.p)):
        mask = None if masks is None else masks[k]
        for name, got, want, bar in (("p", got_p[k], want_p[k], trace.bar_p[k]), ("exp_avg", got_m[k], want_m[k], trace.bar_m[k]),
                                     ("exp_avg_sq", got_v[k], want_v[k], trace.bar_v[k])):
            w = worst(got, want, bar, mask)
            assert w <= 1.0, "%s: tensor %d %s is at %.3g of its bar" % (what, k, name, w)
