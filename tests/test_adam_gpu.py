"""FusedAdam on the GPU against the float64 references and per-element bars of tests/adam_util.py: parity in every
configuration and storage type, the gradient scale and the skipped step (by hand and through torch.amp.GradScaler),
non-finite gradients, every placement of parameter and gradient, reproducibility, no host synchronisation, and the trainer."""
import functools
import warnings

import pytest
import torch

import adam_util as au
import trainer_util as tu
from global_flow_local_attention_amd import FusedAdam, _lib
from global_flow_local_attention_amd.trainer import TrainerShell

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def inputs(name):
    return au.make_inputs(au.shapes(), DTYPES[name])


@functools.lru_cache(maxsize=None)
def reference(name, config):
    """(restatement with one counter per group, torch's float64 run): computed once, shared, never written"""
    params, grads = inputs(name)
    return au.restate(params, grads, config), au.torch_reference(params, grads, config)


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).clone()


def build(params, config, dtype, **kwargs):
    (beta1, beta2), wd, decoupled = config
    ps = [torch.nn.Parameter(x.to(device=DEV, dtype=dtype)) for x in params]
    return ps, FusedAdam(ps, lr=au.LR, betas=(beta1, beta2), eps=au.EPS, weight_decay=wd, decoupled_weight_decay=decoupled,
                         **kwargs)


def set_grads(ps, row, dtype, scale=None):
    for p, g in zip(ps, row):
        p.grad = None if g is None else (g if scale is None else g * scale).to(device=DEV, dtype=dtype)


def state_of(opt, ps):
    """(p or master, exp_avg, exp_avg_sq) per tensor"""
    value = [opt.state[p].get("master_param", p).detach() for p in ps]
    return value, [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps]


def run(name, config, upto=au.STEPS, only=None):
    params, grads = inputs(name)
    if only is not None:
        params, grads = [params[only]], [[row[only]] for row in grads]
    ps, opt = build(params, config, DTYPES[name])
    for row in grads[:upto]:
        set_grads(ps, row, DTYPES[name])
        opt.step()
    return ps, opt


# ---- 1. parity -------------------------------------------------------------------------------------------------------------
PARITY = [("f32", c) for c in au.CONFIGS] + [(n, c) for n in ("f16", "bf16") for c in au.HALF_CONFIGS]


@pytest.mark.parametrize("name, config", PARITY, ids=repr)
def test_parity(name, config):
    dtype = DTYPES[name]
    params, grads = inputs(name)
    trace, theirs = reference(name, config)
    ps, opt = build(params, config, dtype)
    k = au.NONE_TENSOR
    for s, row in enumerate(grads):
        set_grads(ps, row, dtype)
        before = [bits(t[k]) for t in state_of(opt, ps)] + [bits(ps[k])] if s == au.NONE_STEP else None
        opt.step()
        if before is not None:                           # grad is None: nothing of the tensor is touched
            after = [bits(t[k]) for t in state_of(opt, ps)] + [bits(ps[k])]
            assert all(torch.equal(a, b) for a, b in zip(before, after))
    got = state_of(opt, ps)
    au.check_within(trace, *got, what="restatement")
    # torch counts steps per parameter: the tensor that missed a gradient is behind its group there
    masks = [torch.full(p.shape, i != k, dtype=torch.bool) for i, p in enumerate(params)]
    au.check_within(trace, *got, what="torch float64", wants=theirs, masks=masks)
    assert all(opt.state[p]["step"] is opt.state[ps[0]]["step"] for p in ps)
    assert float(opt.state[ps[0]]["step"]) == au.STEPS
    assert all(float(e["step"]) == au.STEPS and e["step"].dim() == 0 for e in opt.state_dict()["state"].values())
    if dtype != torch.float32:                           # the stored parameter is the master rounded to nearest even
        for p in ps:
            master = opt.state[p]["master_param"]
            assert master.dtype == torch.float32 and torch.equal(bits(p), bits(master.to(dtype)))
    else:
        assert all("master_param" not in opt.state[p] for p in ps)


# ---- 2. scale and skip -----------------------------------------------------------------------------------------------------
def test_grad_scale_inside_the_kernel():
    config, scale = au.CONFIGS[2], 2.0 ** 16
    params, grads = inputs("f32")
    ps, opt = build(params, config, torch.float32)
    opt.grad_scale, opt.found_inf = torch.tensor(scale, device=DEV), torch.tensor(0.0, device=DEV)
    for row in grads:
        set_grads(ps, row, torch.float32)
        kept = [None if p.grad is None else bits(p.grad) for p in ps]
        opt.step()
        for p, b in zip(ps, kept):                       # the gradients in memory stay scaled
            assert b is None or torch.equal(bits(p.grad), b)
    trace = au.restate(params, grads, config, grad_scale=scale)
    au.check_within(trace, *state_of(opt, ps), what="restatement, scale 2^16")
    masks = [torch.full(p.shape, i != au.NONE_TENSOR, dtype=torch.bool) for i, p in enumerate(params)]
    au.check_within(trace, *state_of(opt, ps), what="torch float64 on gradients / 2^16",
                    wants=au.torch_reference(params, grads, config, divide=scale), masks=masks)


def test_found_inf_skips_the_step_and_nothing_else():
    config = au.CONFIGS[1]
    params, grads = inputs("f32")
    ps, opt = build(params, config, torch.float32)
    opt.grad_scale, opt.found_inf = None, torch.zeros((), device=DEV)
    for s, row in enumerate(grads):
        set_grads(ps, row, torch.float32)
        opt.found_inf.fill_(1.0 if s == 2 else 0.0)
        if s == 2:
            plan = opt._plans[0]
            before = [bits(t) for t in (plan.exp_avg, plan.exp_avg_sq, plan.step)] + [bits(p) for p in ps]
            kept = [bits(p.grad) for p in ps]
        opt.step()
        if s == 2:
            after = [bits(t) for t in (plan.exp_avg, plan.exp_avg_sq, plan.step)] + [bits(p) for p in ps]
            assert all(torch.equal(a, b) for a, b in zip(before, after))
            assert all(torch.equal(bits(p.grad), b) for p, b in zip(ps, kept))
    assert float(opt.state[ps[0]]["step"]) == au.STEPS - 1
    trace = au.restate(params, grads, config, skip=(2,))          # a reference that never saw the third step
    au.check_within(trace, *state_of(opt, ps), what="restatement without step 3")
    masks = [torch.full(p.shape, i != au.NONE_TENSOR, dtype=torch.bool) for i, p in enumerate(params)]
    au.check_within(trace, *state_of(opt, ps), what="torch float64 without step 3",
                    wants=au.torch_reference(params, grads, config, skip=(2,)), masks=masks)


def test_stock_grad_scaler_skips_and_halves():
    config = au.CONFIGS[0]
    params, grads = au.make_inputs(au.shapes(), with_none=False, steps=2)
    ps, opt = build(params, config, torch.float32)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    scaler.scale(torch.zeros(1, device=DEV))                     # creates the scale tensor, as a loss would
    with warnings.catch_warnings():
        warnings.simplefilter("error", FutureWarning)
        set_grads(ps, grads[0], torch.float32, scale=2.0 ** 16)
        ps[7].grad.view(-1)[11] = float("inf")
        before = [bits(p) for p in ps]
        scaler.step(opt)
        scaler.update()
        assert scaler.get_scale() == 2.0 ** 15
        assert all(torch.equal(bits(p), b) for p, b in zip(ps, before)) and not opt.state[ps[0]]["exp_avg_sq"].any()
        assert float(opt.state[ps[0]]["step"]) == 0
        set_grads(ps, grads[1], torch.float32, scale=2.0 ** 15)
        scaler.step(opt)
        scaler.update()
    assert scaler.get_scale() == 2.0 ** 15 and float(opt.state[ps[0]]["step"]) == 1
    assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
    trace = au.restate(params, [grads[1]], config)
    au.check_within(trace, *state_of(opt, ps), what="the step after the skipped one")


# ---- 3. non-finite gradients without found_inf ----------------------------------------------------------------------------
def test_non_finite_gradients_poison_their_own_elements():
    config = au.CONFIGS[1]
    params, grads = inputs("f32")
    k, c = 10, au.chunk()
    spots = {c - 1: float("nan"), c + 2: float("inf")}           # either side of a chunk boundary, in the second step
    grads = [list(row) for row in grads]
    grads[1][k] = grads[1][k].clone()
    for at, value in spots.items():
        grads[1][k].view(-1)[at] = value
    ps, opt = build(params, config, torch.float32)
    for row in grads:
        set_grads(ps, row, torch.float32)
        opt.step()
    got = state_of(opt, ps)
    masks = [torch.ones(p.shape, dtype=torch.bool) for p in params]
    for at in spots:
        masks[k].view(-1)[at] = False
        for t in got:
            assert not torch.isfinite(t[k].view(-1)[at])
    for t in got:
        assert all(int((~torch.isfinite(x)).sum()) == (2 if i == k else 0) for i, x in enumerate(t))
    au.check_within(au.restate(params, grads, config), *got, what="beside the poisoned elements", masks=masks)


# ---- 4. placement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "f16", "bf16"])
def test_every_phase_of_parameter_and_gradient(name):
    dtype = DTYPES[name]
    size = torch.empty((), dtype=dtype).element_size()
    phases = (0, 4, 8, 12) if size == 4 else (0, 2, 8, 14)
    config = au.CONFIGS[4]
    cases = [(n, pp, gp) for n in (1, 5, 67) for pp in phases for gp in phases]
    slot = 16 + ((67 * size + 15) // 16) * 16 + 32               # red zone, phase, the view, red zone
    arena = torch.full((2 * len(cases) * slot // size,), -3.0, dtype=dtype, device=DEV)
    assert arena.data_ptr() % 16 == 0
    inside = torch.zeros(arena.numel(), dtype=torch.bool)
    shape_list = [(n,) for n, _, _ in cases]
    params, grads = au.make_inputs(shape_list, dtype, seed=7, steps=2, with_none=False)
    ps, gviews = [], []
    for i, (n, pp, gp) in enumerate(cases):
        views = []
        for j, phase in enumerate((pp, gp)):
            at = ((2 * i + j) * slot + 16 + phase) // size
            views.append(arena[at:at + n])
            inside[at:at + n] = True
            assert views[-1].data_ptr() % 16 == phase
        views[0].copy_(params[i])
        ps.append(torch.nn.Parameter(views[0]))
        assert ps[-1].data_ptr() == views[0].data_ptr()
        gviews.append(views[1])
    (beta1, beta2), wd, decoupled = config
    opt = FusedAdam(ps, lr=au.LR, betas=(beta1, beta2), eps=au.EPS, weight_decay=wd, decoupled_weight_decay=decoupled)
    for row in grads:
        for p, view, g in zip(ps, gviews, row):
            view.copy_(g)
            p.grad = view
        opt.step()
    au.check_within(au.restate(params, grads, config), *state_of(opt, ps), what="placed")
    outside = ~inside.to(DEV)
    assert torch.equal(bits(arena)[outside], bits(torch.full_like(arena, -3.0))[outside])     # every red zone intact
    taken = set()
    for p, view, (n, pp, gp) in zip(ps, gviews, cases):
        st = opt.state[p]
        master = st["master_param"].data_ptr() if "master_param" in st else 0
        path = _lib.lib().gfla_adam_vector_path(p.data_ptr(), view.data_ptr(), st["exp_avg"].data_ptr(),
                                                st["exp_avg_sq"].data_ptr(), master, size)
        assert path == (1 if (pp, gp) == (0, 0) else 0)
        taken.add(path)
        if size == 2:
            assert torch.equal(bits(p), bits(st["master_param"].to(dtype)))
    assert taken == {0, 1}                                        # both paths have run


# ---- 5. reproducibility ----------------------------------------------------------------------------------------------------
def test_bits_repeat_and_do_not_depend_on_the_batch():
    config = au.CONFIGS[2]
    first, second = run("f32", config), run("f32", config)
    for a, b in zip(state_of(first[1], first[0]), state_of(second[1], second[0])):
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    for k in (4, 10, 11):                                          # 63, 2 c + 1 and (3,5,3,3) elements
        alone = run("f32", config, only=k)
        for a, b in zip(state_of(first[1], first[0]), state_of(alone[1], alone[0])):
            assert torch.equal(bits(a[k]), bits(b[0]))


# ---- 6. no host synchronisation --------------------------------------------------------------------------------------------
def test_step_never_waits_for_the_device():
    params, grads = au.make_inputs(au.shapes(), with_none=False, steps=4)
    ps, opt = build(params, au.CONFIGS[0], torch.float32)
    fresh = [[g.to(DEV) for g in row] for row in grads]
    scale, inf = torch.tensor(4.0, device=DEV), torch.tensor(0.0, device=DEV)
    for p, g in zip(ps, fresh[0]):
        p.grad = g
    opt.step()                                                   # the first step allocates the state
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()                                               # unchanged gradient addresses: no upload either
        for row in fresh[1:]:
            opt.zero_grad(set_to_none=True)
            for p, g in zip(ps, row):
                p.grad = g
            opt.step()
        opt.grad_scale, opt.found_inf = scale, inf               # as GradScaler.step hands them over
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert float(opt.state[ps[0]]["step"]) == 6


def test_sparse_gradients_are_refused_on_the_device():
    ps, opt = build([torch.zeros(4, 3)], au.CONFIGS[0], torch.float32)
    ps[0].grad = torch.zeros(4, 3, device=DEV).to_sparse()
    with pytest.raises(ValueError):
        opt.step()


# ---- 7. the trainer --------------------------------------------------------------------------------------------------------
def shells(amp=None):
    """TrainerShell(optimizer="kernels") and ("torch") on the stand-in generator's smallest network, equal parameters"""
    out = []
    base, net = tu.build_shell(DEV, ngf=16, lr=1e-3)
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    for optimizer in ("kernels", "torch"):
        base, net = tu.build_shell(DEV, ngf=16, lr=1e-3, state=state)
        out.append((TrainerShell(net, lr=1e-3, correctness=base.correctness, regularization=base.regularization,
                                 attn_layer=(2, 3), amp=amp, optimizer=optimizer), net))
    return out


def test_trainer_float32():
    (fused, fused_net), (plain, plain_net) = shells()
    assert type(fused.optimizer_G) is FusedAdam and type(plain.optimizer_G) is torch.optim.Adam
    batch = tu.make_batch(2, 64, 48)
    _, grads, before, after = tu.run_step(fused, fused_net, batch, DEV)
    tu.run_step(plain, plain_net, batch, DEV)
    names = [n for n, _ in fused_net.named_parameters() if n in grads]
    config = ((0.0, 0.999), 0.0, False)                          # TrainerShell's betas
    trace = au.restate([before[n].cpu() for n in names], [[grads[n].cpu() for n in names]], config, lr=1e-3)
    theirs = au.torch_reference([before[n].cpu() for n in names], [[grads[n].cpu() for n in names]], config, lr=1e-3)[0]
    for k, n in enumerate(names):
        assert au.worst(after[n], theirs[k], trace.bar_p[k]) <= 1.0, n
    second = tu.run_step(fused, fused_net, batch, DEV)[0], tu.run_step(plain, plain_net, batch, DEV)[0]
    assert set(second[0]) == set(second[1])
    for term in second[0]:
        assert abs(second[0][term] - second[1][term]) <= 1e-5 * abs(second[1][term]), term


def test_trainer_fp16_skips_what_torch_skips():
    (fused, fused_net), (plain, plain_net) = shells(amp="fp16")
    batch = tu.make_batch(2, 64, 48)
    for _ in range(2):
        tu.run_step(fused, fused_net, batch, DEV)
        tu.run_step(plain, plain_net, batch, DEV)
    assert fused.skipped_steps == plain.skipped_steps
    assert all(torch.isfinite(p).all() for p in fused_net.parameters())
