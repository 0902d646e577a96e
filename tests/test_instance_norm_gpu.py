"""Fused InstanceNorm2d + LeakyReLU on the GPU (csrc/instance_norm.hip): goldens, a sweep over dtype x configuration x
shape through all three launch regimes, planes far from zero, bit identity, partial gradient requests, memory, the z == 0
tie, routing, and one training step of the stand-in generator fused against unfused.

The truth of every comparison is the float64 HOST evaluation of the torch composition (F.instance_norm, then F.leaky_relu /
F.relu) on the same, already rounded, inputs (instance_norm_util.truth).  Bars are not fixed numbers: the composition is
evaluated on the GPU in the same test (16-bit maps under torch.autocast, as they are used), its error against the truth
is the bar, and the kernel may not exceed it -- with a floor of 4 units in the last place of the compared tensor's type
at its largest entry, because the kernel and torch order their sums differently and neither is the truth.  float64: 1e-12
of the largest entry.

d/dz of the activation jumps at z = 0: every x here is nudged on the host until no |z| of the truth is within 1e-4 of
zero (instance_norm_util.clear_of_kinks), each case asserts that none is left, and no element is excluded."""
import os
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import instance_norm_util as iu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALF = (torch.float16, torch.bfloat16)
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
WHAT = ("forward", "d/d x", "d/d weight", "d/d bias")


def _run(fn, x, w, b, up, need=(True, True, True)):
    """(y, dx, dw, db) of fn(x, w, b) on the GPU for host tensors in their storage types"""
    xs = x.to(DEV).requires_grad_(need[0])
    ws = None if w is None else w.to(DEV).requires_grad_(need[1])
    bs = None if b is None else b.to(DEV).requires_grad_(need[2])
    y = fn(xs, ws, bs)
    if y.requires_grad:
        (y * up.to(DEV)).sum().backward()
    return y.detach(), xs.grad, None if ws is None else ws.grad, None if bs is None else bs.grad


def _kernel(gfla, slope):
    return lambda x, w, b: gfla.InstanceNormActFunction.apply(x, w, b, iu.EPS, slope)


def _composition(slope, dtype):
    def fn(x, w, b):
        with torch.autocast("cuda", dtype=dtype, enabled=dtype in HALF):
            return iu.composition(x, w, b, iu.EPS, slope)
    return fn


def check(gfla, x, w, b, up, slope, label, got=None):
    """x / w / b / up on the host in their storage types.  Prints every figure, then asserts."""
    if slope is not None:
        assert not iu.near_kink(x, w, b).any(), "a pre-activation is within %.0e of the kink" % iu.CLEAR
    want = iu.truth(x, w, b, up, iu.EPS, slope)
    got = _run(_kernel(gfla, slope), x, w, b, up) if got is None else got
    comp = _run(_composition(slope, x.dtype), x, w, b, up)
    assert got[0].dtype == x.dtype and got[1].dtype == x.dtype
    failures = []
    for what, g, c, t in zip(WHAT, got, comp, want):
        assert (g is None) == (t is None), what
        if t is None:
            continue
        assert g.dtype == (x.dtype if what in WHAT[:2] else w.dtype) and g.shape == t.shape
        scale = t.abs().max().item()
        err_k = (g.double().cpu() - t).abs().max().item()
        err_c = (c.double().cpu() - t).abs().max().item()
        if x.dtype == torch.float64:
            floor = bar = 1e-12 * scale
        else:
            floor = 4 * iu.ulp(g.dtype, scale)
            bar = max(err_c, floor)
        print("%s %s: kernel %.3e, composition %.3e, floor %.3e (scale %.3e)" % (label, what, err_k, err_c, floor, scale))
        assert torch.isfinite(g).all()
        if not err_k <= bar:
            failures.append((what, err_k, bar))
    assert not failures, failures
    return got


@pytest.mark.parametrize("config", sorted(iu.CONFIGS))
def test_goldens_float64(gfla, config):
    g = iu.golden(config)
    _, slope = iu.CONFIGS[config]
    got = _run(lambda x, w, b: gfla.instance_norm_act(x, w, b, iu.EPS, slope), g["x"], g["weight"], g["bias"], g["up"])
    for what, a, t in zip(WHAT, got, (g["y"], g["g_x"], g["g_weight"], g["g_bias"])):
        assert (a is None) == (t is None), what
        if t is not None:
            err = (a.cpu() - t).abs().max().item()
            print("golden %s %s: %.3e of %.3e" % (config, what, err, t.abs().max().item()))
            assert err <= 1e-12 * t.abs().max().item(), (what, err)


def _split_shape(dtype):
    shape = iu.smallest_split_shape(torch.empty((), dtype=dtype).element_size())
    return shape


# shape -> the regime the design puts it in ("split": found by query)
SWEEP = [((2, 3, 1, 2), 0),        # the smallest legal plane
         ((2, 5, 3, 7), 0),        # 21 values: less than a wave, odd
         ((3, 70, 8, 6), 0),       # 210 planes: not a multiple of the four planes of a workgroup
         ((2, 3, 33, 19), 0),      # 627 values, odd: every plane after the first starts off a 16-byte boundary
         ((1, 4, 64, 44), 1),      # the bench plane
         ((2, 130, 16, 11), 0),    # many channels through the dgamma / dbeta reduction
         ((1, 2, 256, 176), 2),    # the largest register-resident plane; two planes: split
         ("split", 2)]             # the smallest plane the library itself splits for two planes


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("config", sorted(iu.CONFIGS))
@pytest.mark.parametrize("shape,regime", SWEEP)
def test_sweep(gfla, shape, regime, config, dtype):
    if shape == "split":
        shape = _split_shape(dtype)
    esize = torch.empty((), dtype=dtype).element_size()
    assert iu.geometry(*shape, esize)["regime"] == regime
    x, w, b, up, slope = iu.make_case(shape, dtype, config, seed=iu.sweep_seed(shape))
    check(gfla, x, w, b, up, slope, "%s %s %s" % (shape, config, str(dtype)[6:]))


@pytest.mark.parametrize("shape", [(2, 3, 1030, 1), (1, 3, 37, 29)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_odd_planes_in_a_workgroup(gfla, shape, dtype):
    """regime 1 with an odd plane length: planes start off the 16-byte boundary, scalar head and tail"""
    assert iu.geometry(*shape, torch.empty((), dtype=dtype).element_size())["regime"] == 1
    x, w, b, up, slope = iu.make_case(shape, dtype, "affine_leaky", seed=17)
    check(gfla, x, w, b, up, slope, "%s %s" % (shape, str(dtype)[6:]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_full_register_plane(gfla, dtype):
    """256 planes of 256 x 176: the most vectors a thread holds, forward and backward, in regime 1"""
    shape = iu.FULL_PLANE_SHAPE
    g = iu.geometry(*shape, torch.empty((), dtype=dtype).element_size())
    assert g["regime"] == 1 and g["threads"] == 1024
    x, w, b, up, slope = iu.make_case(shape, dtype, "affine_leaky", seed=9)
    check(gfla, x, w, b, up, slope, "%s %s" % (shape, str(dtype)[6:]))


@pytest.mark.parametrize("dtype,offset", [(torch.float32, 1000.0), (torch.float16, 100.0)])
@pytest.mark.parametrize("shape", [(2, 4, 64, 44), "split"])
def test_planes_far_from_zero(gfla, shape, dtype, offset):
    """mean 1000 and spread 1: a one-pass variance, or a careless merge of the partials of a split plane, loses everything
    in float32.  The bar is still the composition's own error."""
    if shape == "split":
        shape = _split_shape(dtype)
    x, w, b, up, slope = iu.make_case(shape, dtype, "affine_leaky", seed=3, offset=offset)
    check(gfla, x, w, b, up, slope, "offset %g %s %s" % (offset, shape, str(dtype)[6:]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,regime", [((3, 70, 8, 6), 0), ((2, 6, 64, 44), 1), ("split", 2)])
def test_bit_identity_and_partial_requests(gfla, shape, regime, dtype):
    if shape == "split":
        shape = _split_shape(dtype)
    assert iu.geometry(*shape, torch.empty((), dtype=dtype).element_size())["regime"] == regime
    x, w, b, up, slope = iu.make_case(shape, dtype, "affine_leaky", seed=5)
    fn = _kernel(gfla, slope)
    first, again = _run(fn, x, w, b, up), _run(fn, x, w, b, up)
    assert all(torch.equal(a, c) for a, c in zip(first, again))
    # frozen parameters: d/d x alone, the same bits
    only_x = _run(fn, x, w, b, up, need=(True, False, False))
    assert torch.equal(only_x[1], first[1]) and only_x[2] is None and only_x[3] is None
    # the parameters alone
    only_p = _run(fn, x, w, b, up, need=(False, True, True))
    assert only_p[1] is None and torch.equal(only_p[2], first[2]) and torch.equal(only_p[3], first[3])
    only_w = _run(fn, x, w, b, up, need=(False, True, False))
    assert torch.equal(only_w[2], first[2]) and only_w[3] is None
    # nothing: no graph, nothing saved
    y = fn(x.to(DEV), w.to(DEV), b.to(DEV))
    assert torch.equal(y, first[0]) and y.grad_fn is None and not y.requires_grad
    xs = x.to(DEV).requires_grad_()
    y = gfla.InstanceNormActFunction.apply(xs.detach(), w.to(DEV), b.to(DEV), iu.EPS, slope)
    assert y.grad_fn is None
    with torch.no_grad():
        assert torch.equal(fn(xs, w.to(DEV), b.to(DEV)), first[0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_non_contiguous_input(gfla, dtype):
    x, w, b, up, slope = iu.make_case((2, 6, 33, 19), dtype, "affine_leaky", seed=8)
    big = torch.zeros(2, 9, 33, 19, dtype=dtype, device=DEV)
    big[:, 2:8] = x.to(DEV)
    view = big[:, 2:8]
    assert not view.is_contiguous()
    fn = _kernel(gfla, slope)
    want = _run(fn, x, w, b, up)
    vs = view.detach().requires_grad_()
    ws, bs = w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    y = fn(vs, ws, bs)
    (y * up.to(DEV)).sum().backward()
    assert torch.equal(y, want[0]) and torch.equal(vs.grad, want[1]) and torch.equal(ws.grad, want[2])
    # a contiguous view that starts off a 16-byte boundary
    flat = torch.zeros(x.numel() + 1, dtype=dtype, device=DEV)
    flat[1:] = x.to(DEV).reshape(-1)
    off = flat[1:].view(x.shape)
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    assert torch.equal(fn(off, w.to(DEV), b.to(DEV)), want[0])


@pytest.mark.parametrize("dtype", HALF)
def test_sixteen_bit_map_with_float32_parameters(gfla, dtype):
    x, w, b, up, slope = iu.make_case((2, 5, 33, 19), dtype, "affine_leaky", seed=12, param_dtype=torch.float32)
    assert w.dtype == torch.float32
    got = check(gfla, x, w, b, up, slope, "mixed %s" % str(dtype)[6:])
    assert got[0].dtype == dtype and got[1].dtype == dtype and got[2].dtype == torch.float32 and got[3].dtype == torch.float32


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_memory(gfla, dtype):
    """x itself is saved, and forward + backward peak below the composition and below 2.5 x the map (output + dx + the
    per-plane vectors; the composition also holds the normalised map)"""
    shape = (4, 64, 64, 44)
    x, w, b, up, slope = iu.make_case(shape, dtype, "affine_leaky", seed=13, param_dtype=torch.float32)
    xs = x.to(DEV).requires_grad_()
    ws, bs, ups = w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_(), up.to(DEV)
    peaks = {}
    for name, fn in (("kernel", _kernel(gfla, slope)), ("composition", _composition(slope, dtype))):
        for _ in range(2):      # the first pass warms the allocator and loads the code objects
            xs.grad = ws.grad = bs.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            y = fn(xs, ws, bs)
            if name == "kernel":
                saved = y.grad_fn.saved_tensors
                assert saved[0].data_ptr() == xs.data_ptr()
                assert len(saved) == 5 and sum(t.numel() == xs.numel() for t in saved) == 1   # no full-size tensor of its own
            y.backward(ups)
            del y
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - before
    map_bytes = x.numel() * x.element_size()
    print("peak bytes above the inputs, %s: kernel %d (%.2f maps), composition %d (%.2f maps)"
          % (str(dtype)[6:], peaks["kernel"], peaks["kernel"] / map_bytes, peaks["composition"], peaks["composition"] / map_bytes))
    assert peaks["kernel"] < peaks["composition"]
    assert peaks["kernel"] < 2.5 * map_bytes


def test_tie_at_zero_takes_the_slope(gfla):
    """gamma = beta = 0: every z is exactly zero, and d/dz is the slope, as in leaky_relu_backward.  dx equals the
    composition's exactly (both are zero: gamma scales it) and d/d bias = slope * sum dy.  d/d weight = sum dz xhat is a
    float32 sum that the kernel and torch take in different orders, so it cannot be required to have the same bits: it
    is held to the sweep's bar (the composition's error against the float64 truth, floor 4 ulp); the other side of the
    tie would be wrong by a factor of ten.  Whether the bits happen to agree is printed."""
    shape, slope = (2, 3, 16, 11), 0.1
    g = torch.Generator().manual_seed(14)
    x, up = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    w, b = torch.zeros(3), torch.zeros(3)
    got = _run(_kernel(gfla, slope), x, w, b, up)
    comp = _run(_composition(slope, torch.float32), x, w, b, up)
    assert not got[0].any() and not got[1].any() and torch.equal(got[1], comp[1])
    want = iu.truth(x, w, b, up, iu.EPS, slope)
    want_db = slope * up.double().sum(dim=(0, 2, 3))
    assert (want[3] - want_db).abs().max().item() <= 1e-12
    for what, i in (("d/d weight", 2), ("d/d bias", 3)):
        err_k = (got[i].double().cpu() - want[i]).abs().max().item()
        err_c = (comp[i].double().cpu() - want[i]).abs().max().item()
        floor = 4 * iu.ulp(torch.float32, want[i].abs().max().item())
        print("tie %s: kernel %.3e, composition %.3e, floor %.3e, same bits as the composition: %s"
              % (what, err_k, err_c, floor, torch.equal(got[i], comp[i])))
        assert err_k <= max(err_c, floor), what


def test_routing(gfla):
    x, w, b, up, slope = iu.make_case((2, 4, 16, 11), torch.float32, "affine_leaky", seed=15)
    mod = gfla.InstanceNormAct(4, affine=True, negative_slope=slope).to(DEV)
    with torch.no_grad():
        mod.weight.copy_(w)
        mod.bias.copy_(b)
    seq = nn.Sequential(nn.InstanceNorm2d(4, affine=True), nn.LeakyReLU(slope), nn.Conv2d(4, 2, 1)).to(DEV)
    with torch.no_grad():
        seq[0].weight.copy_(w)
        seq[0].bias.copy_(b)
    unfused = seq[1](seq[0](x.to(DEV))).detach()
    assert gfla.fuse_instance_norm_act(seq) == 1
    ours = gfla.InstanceNormActFunction._backward_cls
    y_mod, y_seq = mod(x.to(DEV)), seq[1](seq[0](x.to(DEV)))
    assert isinstance(y_mod.grad_fn, ours) and isinstance(y_seq.grad_fn, ours) and torch.equal(y_mod, y_seq)
    mod.impl = "torch"
    y_torch = mod(x.to(DEV))
    assert not isinstance(y_torch.grad_fn, ours) and torch.equal(y_torch.detach(), unfused)
    assert not isinstance(gfla.instance_norm_act(x.to(DEV), impl="torch").grad_fn, ours)
    want = iu.truth(x, w, b, up, iu.EPS, slope)[0]
    err_k, err_t = (y_mod.detach().double().cpu() - want).abs().max().item(), (y_torch.detach().double().cpu() - want).abs().max().item()
    print("routing: kernel %.3e, torch %.3e" % (err_k, err_t))
    assert err_k <= max(err_t, 4 * iu.ulp(torch.float32, want.abs().max().item()))
    with pytest.raises(TypeError):
        gfla.InstanceNormActFunction.apply(x.to(DEV).to(torch.int32), None, None, iu.EPS, slope)
    with pytest.raises(ValueError):
        gfla.InstanceNormActFunction.apply(x.to(DEV)[:, :, :1, :1], None, None, iu.EPS, slope)
    with pytest.raises(ValueError):
        gfla.InstanceNormActFunction.apply(x.to(DEV), w.to(DEV)[:3], b.to(DEV), iu.EPS, slope)


def test_one_fused_training_step(gfla):
    """the stand-in generator with fuse_instance_norm_act applied against the same network unfused, one optimiser step at
    the trainer tests' smallest shape, within the bars tests/test_trainer_gpu.py holds between the GPU and the host:
    every loss term 1e-4 relative, every gradient 1e-4 of its tensor's largest entry (gradients that are rounding noise
    of a cancelling sum on the reference side have to be noise here too)"""
    import trainer_util as tu
    batch = tu.make_batch(2, 64, 48)
    plain_shell, plain_net = tu.build_shell(DEV, ngf=16, lr=1e-3)
    state = {k: v.clone() for k, v in plain_net.state_dict().items()}
    fused_shell, fused_net = tu.build_shell(DEV, ngf=16, lr=1e-3, state=state)
    assert gfla.fuse_instance_norm_act(fused_net) == 13
    assert list(fused_net.state_dict().keys()) == list(state.keys())
    want_losses, want_grads, _, _ = tu.run_step(plain_shell, plain_net, batch, DEV)
    losses, grads, _, _ = tu.run_step(fused_shell, fused_net, batch, DEV)
    assert set(losses) == set(want_losses)
    for k in losses:
        print("fused step %s: %.9g / %.9g" % (k, losses[k], want_losses[k]))
        assert abs(losses[k] - want_losses[k]) <= 1e-4 * max(abs(want_losses[k]), 1e-3), (k, losses[k], want_losses[k])
    assert set(grads) == set(want_grads)
    gmax = max(w.abs().max().item() for w in want_grads.values())
    worst = ("", 0.0)
    for n in sorted(grads):
        g, w = grads[n].double(), want_grads[n].double()
        scale = w.abs().max().item()
        if scale <= 1e-5 * gmax:
            assert g.abs().max().item() <= 1e-5 * gmax, n
            continue
        err = (g - w).abs().max().item() / scale
        worst = max(worst, (n, err), key=lambda t: t[1])
        assert err <= 1e-4, "grad %s: %.3e of its max %.3e" % (n, err, scale)
    print("fused step, worst gradient: %s %.2e" % worst)
