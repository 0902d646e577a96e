"""FusedAdam without a GPU: the C ABI's host side (symbols, layout, path decision, every argument refusal), the optimizer's
refusals, state-dict interchange with torch.optim.Adam / AdamW in both directions, TrainerShell's optimizer keyword, and the
self-checks of tests/adam_util.py's references and bars."""
import ctypes

import pytest
import torch

import adam_util as au
from global_flow_local_attention_amd import FusedAdam, _lib
from global_flow_local_attention_amd.trainer import TrainerShell

STEP_NAMES = ("gfla_adam_step_f32", "gfla_adam_step_f16", "gfla_adam_step_bf16")
ENTRY_POINTS = ("gfla_adam_chunk_elems", "gfla_adam_layout", "gfla_adam_vector_path") + STEP_NAMES


def i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def addr(array):
    return ctypes.addressof(array)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_extension_symbols_and_the_pinned_numbers_stay():
    assert set(ENTRY_POINTS) <= set(_lib.extension_symbols())
    assert not set(ENTRY_POINTS) & set(_lib.exported_symbols())
    assert len(_lib.exported_symbols()) == 154 and _lib.ABI_VERSION == 8 and _lib.PATH_COUNT == 22
    assert any(p.endswith("gfla_adam.h") for p in _lib.EXTENSION_HEADER_PATHS)


def test_chunk_and_layout_by_hand():
    lib = _lib.lib()
    c = lib.gfla_adam_chunk_elems()
    assert c == 4096
    numels = i64([1, c - 1, c, c + 1, 2 * c + 1, 3 * c])
    first, totals = i64([0] * 6), i64([0])
    assert lib.gfla_adam_layout(addr(numels), 6, addr(first), addr(totals)) == 0
    assert list(first) == [0, 1, 2, 3, 5, 8] and totals[0] == 11
    assert lib.gfla_adam_layout(None, 6, addr(first), addr(totals)) == -1
    assert lib.gfla_adam_layout(addr(numels), 6, None, addr(totals)) == -1
    assert lib.gfla_adam_layout(addr(numels), 6, addr(first), None) == -1
    assert lib.gfla_adam_layout(addr(numels), 0, addr(first), addr(totals)) == -2
    assert lib.gfla_adam_layout(addr(i64([4, 0])), 2, addr(first), addr(totals)) == -2
    assert lib.gfla_adam_layout(addr(i64([2 ** 31])), 1, addr(first), addr(totals)) == _lib._ERR_UNSUPPORTED
    assert lib.gfla_adam_layout(addr(i64([2 ** 31 - 1])), 1, addr(first), addr(totals)) == 0 and totals[0] == 2 ** 19


def test_vector_path_by_hand():
    path = _lib.lib().gfla_adam_vector_path
    assert path(4096, 8192, 256, 512, 0, 4) == 1            # all aligned, no master
    assert path(4096, 8192, 256, 512, 1024, 2) == 1
    for bad in range(5):                                    # any one address off a 16-byte boundary
        for off in (2, 4, 8, 12, 14):
            a = [4096, 8192, 256, 512, 1024]
            a[bad] += off
            assert path(*a, 2) == 0 and path(*a, 4) == 0, (bad, off)
    assert path(4096, 8192, 256, 512, 0, 8) == 0            # no such storage type


@pytest.mark.parametrize("name", STEP_NAMES)
def test_every_refusal_is_decided_without_a_device(name):
    fn = getattr(_lib.lib(), name)
    table, step = i64([0] * 16), (ctypes.c_float * 1)(0.0)           # never read: every call below is refused first
    numels = i64([5, 7])
    good = dict(table=addr(table), numels=addr(numels), n=2, step=addr(step), lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                wd=0.0, flags=0)

    def status(**change):
        a = dict(good, **change)
        return fn(a["table"], a["numels"], a["n"], a["step"], None, None, a["lr"], a["beta1"], a["beta2"], a["eps"], a["wd"],
                  a["flags"], None)
    for key in ("table", "numels", "step"):
        assert status(**{key: None}) == -1, key
    assert status(n=0) == -2 and status(n=-1) == -2
    assert status(numels=addr(i64([5, 0]))) == -2 and status(numels=addr(i64([-1, 7]))) == -2
    assert status(lr=-1e-3) == -2 and status(lr=float("nan")) == -2
    assert status(eps=0.0) == -2 and status(eps=-1e-8) == -2
    assert status(beta1=1.0) == -2 and status(beta1=-0.1) == -2 and status(beta2=1.0) == -2 and status(beta2=-0.5) == -2
    assert status(wd=-0.01) == -2
    assert status(flags=2) == -2 and status(flags=3) == -2 and status(flags=-1) == -2
    assert status(numels=addr(i64([5, 2 ** 31]))) == _lib._ERR_UNSUPPORTED
    many = i64([1] * 65536)
    assert status(numels=addr(many), n=65536) == _lib._ERR_UNSUPPORTED


# ---- the optimizer's refusals --------------------------------------------------------------------------------------------
def params_of(dtype=torch.float32, n=3):
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(4, 3, generator=g).to(dtype)) for _ in range(n)]


def test_refused_constructions():
    with pytest.raises(ValueError):
        FusedAdam(params_of(), amsgrad=True)
    with pytest.raises(ValueError):
        FusedAdam(params_of(), maximize=True)
    with pytest.raises(ValueError):
        FusedAdam(params_of() + params_of(torch.bfloat16))            # mixed dtypes within one group
    with pytest.raises(ValueError):
        FusedAdam(params_of(torch.bfloat16), master_weights=False)
    with pytest.raises(ValueError):
        FusedAdam(params_of(torch.float16), master_weights=False)
    for bad in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(eps=0.0), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            FusedAdam(params_of(), **bad)
    FusedAdam([dict(params=params_of()), dict(params=params_of(torch.bfloat16))])   # one dtype per GROUP is enough
    FusedAdam(params_of(), master_weights=False)                                    # float32: no masters either way
    assert FusedAdam._step_supports_amp_scaling is True


def test_step_on_cpu_parameters_is_not_implemented():
    ps = params_of()
    for p in ps:
        p.grad = torch.ones_like(p)
    opt = FusedAdam(ps)
    with pytest.raises(NotImplementedError):
        opt.step()


def test_sparse_gradients_are_refused():
    ps = params_of(n=1)
    ps[0].grad = torch.zeros(4, 3).to_sparse()
    with pytest.raises(ValueError):
        FusedAdam(ps).step()


# ---- state dicts ---------------------------------------------------------------------------------------------------------
def torch_steps(cls, ps, wd, steps, seed):
    opt = cls(ps, lr=1e-3, betas=(0.9, 0.999), weight_decay=wd, foreach=False)
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


@pytest.mark.parametrize("cls, wd", [(torch.optim.Adam, 0.0), (torch.optim.Adam, 0.01), (torch.optim.AdamW, 0.01)])
def test_state_dict_round_trip_with_torch(cls, wd):
    ps = params_of()
    theirs = torch_steps(cls, ps, wd, 3, seed=1)
    saved = theirs.state_dict()
    fused = FusedAdam(ps)
    fused.load_state_dict(saved)
    back = fused.state_dict()
    assert sorted(back["state"]) == sorted(saved["state"])
    for k, entry in saved["state"].items():
        mine = back["state"][k]
        assert mine["step"].dtype == torch.float32 and mine["step"].dim() == 0 and float(mine["step"]) == float(entry["step"]) == 3
        assert torch.equal(mine["exp_avg"], entry["exp_avg"]) and torch.equal(mine["exp_avg_sq"], entry["exp_avg_sq"])
        assert "master_param" not in mine
    group = fused.param_groups[0]
    assert group["weight_decay"] == wd and bool(group["decoupled_weight_decay"]) == (cls is torch.optim.AdamW)
    # views, each from a multiple of 4 elements of one flat buffer per moment
    views = [fused.state[p]["exp_avg"] for p in ps]
    assert len({v.untyped_storage().data_ptr() for v in views}) == 1 and all(v.storage_offset() % 4 == 0 for v in views)
    assert all(v.shape == p.shape for v, p in zip(views, ps))

    # the other way: torch continues from FusedAdam's state dict exactly as it continues by itself
    clones = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    other = cls(clones, lr=1e-3, betas=(0.9, 0.999), weight_decay=wd, foreach=False)
    other.load_state_dict(back)
    g = torch.Generator().manual_seed(9)
    for p, q in zip(ps, clones):
        p.grad = torch.randn(p.shape, generator=g)
        q.grad = p.grad.clone()
    theirs.step()
    other.step()
    for p, q in zip(ps, clones):
        assert torch.equal(p, q)
        assert torch.equal(theirs.state[p]["exp_avg_sq"], other.state[q]["exp_avg_sq"])
        assert float(other.state[q]["step"]) == 4


def test_fresh_and_partial_state_dicts():
    ps = params_of()
    fused = FusedAdam(ps, weight_decay=0.01)
    empty = fused.state_dict()
    assert empty["state"] == {} and len(empty["param_groups"]) == 1
    torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps]).load_state_dict(empty)   # torch accepts it
    # state for the first parameter only: the others start from zero moments at the same count
    theirs = torch_steps(torch.optim.Adam, ps[:1], 0.0, 2, seed=4)
    partial = theirs.state_dict()
    partial["param_groups"][0]["params"] = [0, 1, 2]
    fused.load_state_dict(partial)
    out = fused.state_dict()["state"]
    assert sorted(out) == [0, 1, 2] and all(float(out[k]["step"]) == 2 for k in out)
    assert torch.equal(out[0]["exp_avg"], partial["state"][0]["exp_avg"]) and not out[1]["exp_avg"].any()


@pytest.mark.parametrize("kind", ["number", "tensor"])
def test_step_kinds_and_unequal_steps(kind):
    ps = params_of()
    saved = torch_steps(torch.optim.Adam, ps, 0.0, 3, seed=2).state_dict()
    for entry in saved["state"].values():
        entry["step"] = 3 if kind == "number" else torch.tensor(3.0, dtype=torch.float64)
    fused = FusedAdam(ps)
    fused.load_state_dict(saved)
    assert all(float(e["step"]) == 3 and e["step"].dtype == torch.float32 for e in fused.state_dict()["state"].values())
    saved["state"][1]["step"] = 4 if kind == "number" else torch.tensor(4.0)
    with pytest.raises(ValueError):
        FusedAdam(ps).load_state_dict(saved)


def test_masters_survive_a_state_dict_in_float32():
    ps = params_of(torch.bfloat16)
    fused = FusedAdam(ps)
    state = {k: dict(step=torch.tensor(2.0), exp_avg=torch.full((4, 3), 1.0 + 2.0 ** -20), exp_avg_sq=torch.full((4, 3), 3.0),
                     master_param=ps[k].detach().float() + 2.0 ** -12) for k in range(3)}
    fused.load_state_dict(dict(state=state, param_groups=fused.state_dict()["param_groups"]))
    out = fused.state_dict()["state"]
    for k in range(3):                                    # not rounded to the parameter's 16 bits on the way
        assert out[k]["exp_avg"].dtype == torch.float32 and torch.equal(out[k]["exp_avg"], state[k]["exp_avg"])
        assert torch.equal(out[k]["master_param"], state[k]["master_param"])
    partial = dict(state={0: {key: state[0][key] for key in ("step", "exp_avg", "exp_avg_sq")}},
                   param_groups=fused.state_dict()["param_groups"])
    again = FusedAdam(ps)
    again.load_state_dict(partial)                        # no saved master: the parameter widened
    assert torch.equal(again.state[ps[1]]["master_param"], ps[1].detach().float())


# ---- TrainerShell ----------------------------------------------------------------------------------------------------------
def test_trainer_shell_optimizer_keyword():
    net = torch.nn.Conv2d(3, 4, 3)
    assert type(TrainerShell(net).optimizer_G) is torch.optim.Adam
    assert type(TrainerShell(net, optimizer="torch").optimizer_G) is torch.optim.Adam
    shell = TrainerShell(net, lr=3e-4, betas=(0.0, 0.99), optimizer="kernels")
    assert type(shell.optimizer_G) is FusedAdam
    group = shell.optimizer_G.param_groups[0]
    assert group["lr"] == 3e-4 and tuple(group["betas"]) == (0.0, 0.99) and len(group["params"]) == 2
    with pytest.raises(ValueError):
        TrainerShell(net, optimizer="bogus")


# ---- the references and the bars, checked before anything runs on a GPU ---------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    return au.make_inputs(au.shapes())


def rel(a, b):
    scale = b.abs().max().clamp(min=1e-300)
    return float((a - b).abs().max() / scale)


@pytest.mark.parametrize("config", au.CONFIGS, ids=repr)
def test_restatement_matches_torch_float64(inputs, config):
    params, grads = inputs
    trace = au.restate(params, grads, config, per_tensor_step=True)
    for got, want in zip((trace.p, trace.m, trace.v), au.torch_reference(params, grads, config)):
        for a, b in zip(got, want):
            assert rel(a, b) <= 1e-14
    # one counter per group: every tensor that never missed a gradient is torch's as well
    grouped = au.restate(params, grads, config)
    assert grouped.step == au.STEPS
    for k, (a, b) in enumerate(zip(grouped.p, au.torch_reference(params, grads, config)[0])):
        assert k == au.NONE_TENSOR or rel(a, b) <= 1e-14


def test_restatement_of_scale_and_skip_matches_torch(inputs):
    params, grads = inputs
    config = au.CONFIGS[2]
    for scale in (2.0 ** 16, 2.0 ** -3):                   # powers of two: the reciprocal is exact
        trace = au.restate(params, grads, config, grad_scale=scale, per_tensor_step=True)
        for got, want in zip((trace.p, trace.m, trace.v), au.torch_reference(params, grads, config, divide=scale)):
            for a, b in zip(got, want):
                assert rel(a, b) <= 1e-14
    trace = au.restate(params, grads, config, skip=(2,), per_tensor_step=True)
    assert trace.step == au.STEPS - 1
    for a, b in zip(trace.p, au.torch_reference(params, grads, config, skip=(2,))[0]):
        assert rel(a, b) <= 1e-14


@pytest.mark.parametrize("config", au.CONFIGS, ids=repr)
def test_torch_float32_is_well_inside_the_bars(inputs, config):
    """A bar the float32 reference implementation could not pass would be noticed here, not on the GPU: torch's own
    float32 for-loop Adam stays at <= 0.6 of every bar (measured: 0.50 / 0.19 / 0.12 at the worst)."""
    params, grads = inputs
    trace = au.restate(params, grads, config, per_tensor_step=True)
    p, m, v = au.torch_reference(params, grads, config, dtype=torch.float32)
    for k in range(len(params)):
        for got, want, bar in ((p[k], trace.p[k], trace.bar_p[k]), (m[k], trace.m[k], trace.bar_m[k]),
                               (v[k], trace.v[k], trace.bar_v[k])):
            assert au.worst(got, want, bar) <= 0.6, (k, au.worst(got, want, bar))


def test_ulp32():
    x = torch.tensor([1.0, 1.5, 2.0, 0.75, 2.0 ** -130, 0.0], dtype=torch.float64)
    assert au.ulp32(x).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 2.0 ** -149, 2.0 ** -149]
