"""Narrow 3x3 heads on the GPU (csrc/head_conv3x3.hip): a sweep over shape x dtype x padding x pre-activation, the goldens,
bit identity, partial gradient requests, the x == 0 tie, routing, the vendor fence, one training step of the stand-in
generator fused against unfused, and memory.

The truth of every comparison is the float64 HOST evaluation of the torch composition (head_conv_util.composition) on
the same inputs, already rounded to their storage type; the pre-activation acts on the stored x, so the kernel and the
truth pick the same slope everywhere and no element is excluded.  Per compared tensor an element may be off by the largest
of (a) the derived summation bound 2 (n + 2) 2^-24 S + u_T |t| (n terms: 9 Cin forward, 36 Cout for d x, B H W for d w and
d bias; S the same sum over absolute values in float64), (b) the largest error of the torch composition run on the GPU in
the same storage type in the same test, (c) 4 ulp of the result's type at its largest entry.  All figures are printed."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import head_conv_util as hu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
HALF = (torch.float16, torch.bfloat16)


def _run(fn, x, w, b, up, split, need=(True, True, True), use=(1, 1)):
    """([y..], dx, dw, db) of fn(x, w, b) on the GPU for host tensors"""
    xs = x.to(DEV).requires_grad_(need[0])
    ws = w.to(DEV).requires_grad_(need[1])
    bs = None if b is None else b.to(DEV).requires_grad_(need[2])
    ys = fn(xs, ws, bs)
    ys = ys if isinstance(ys, tuple) else (ys,)
    ups = up.to(DEV)
    parts = (ups,) if split is None else (ups[:, :split], ups[:, split:])
    if any(y.requires_grad for y in ys):
        sum((y * u).sum() for y, u, m in zip(ys, parts, use) if m).backward()
    return [y.detach() for y in ys], xs.grad, ws.grad, None if bs is None else bs.grad


def _kernel(gfla, padding, slope, post, split):
    return lambda x, w, b: gfla.HeadConv3x3Function.apply(x, w, b, padding, slope, hu.posts_of(post, w.size(0)), split)


def _composition(padding, slope, post, split, dtype):
    def fn(x, w, b):
        # the composition in the map's storage type: a parameter of another type is cast to it, as autocast would
        if w.dtype != dtype:
            w, b = w.to(dtype), None if b is None else b.to(dtype)
        return hu.composition(x, w, b, padding, slope, post, split)
    return fn


def check(gfla, case, dtype, padding, slope, label, seed=0, got=None, use=(1, 1), inputs=None, worst=None):
    shape, cout, post, split = case
    x, w, b, up = hu.make_case(shape, cout, dtype, seed) if inputs is None else inputs
    want = hu.truth(x, w, b, up, padding, slope, post, split, None if split is None else use)
    got = _run(_kernel(gfla, padding, slope, post, split), x, w, b, up, split, use=use) if got is None else got
    comp = _run(_composition(padding, slope, post, split, dtype), x, w, b, up, split, use=use)
    n = hu.term_counts(shape, cout)
    rows = [("y%d" % j, g, c, want["y"][j], want["S"]["y"][j], n["y"], dtype) for j, (g, c) in enumerate(zip(got[0], comp[0]))]
    rows += [("d x", got[1], comp[1], want["gx"], want["S"]["gx"], n["gx"], dtype),
             ("d w", got[2], comp[2], want["gw"], want["S"]["gw"], n["gw"], w.dtype)]
    if b is not None:
        rows.append(("d b", got[3], comp[3], want["gb"], want["S"]["gb"], n["gb"], b.dtype))
    failures = []
    for what, g, c, t, S, terms, rtype in rows:
        assert g is not None and g.dtype == rtype and tuple(g.shape) == tuple(t.shape), what
        assert torch.isfinite(g).all(), what
        err = (g.double().cpu() - t).abs()
        bound = hu.summation_bound(terms, S, t, rtype)
        err_c = (c.double().cpu() - t).abs().max().item()
        floor = 4 * hu.ulp(rtype, t.abs().max().item())
        bar = torch.clamp(bound, min=max(err_c, floor))
        ratio = (err / bar.clamp_min(1e-300)).max().item()
        print("%s %s: kernel %.3e, (a) bound %.3e, (b) composition %.3e, (c) floor %.3e, worst err/bar %.3f"
              % (label, what, err.max().item(), bound.max().item(), err_c, floor, ratio))
        if worst is not None:
            worst[0] = max(worst[0], ratio)
        if not bool((err <= bar).all()):
            failures.append((what, err.max().item(), ratio))
    assert not failures, failures
    return got


def _paddings(shape):
    return ("zeros", "reflect") if shape[2] >= 2 and shape[3] >= 2 else ("zeros",)


SWEEP_IDS = ["x".join(map(str, c[0])) + "-%d" % c[1] for c in hu.SWEEP]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("case", hu.SWEEP, ids=SWEEP_IDS)
def test_sweep(gfla, case, dtype):
    shape, cout = case[0], case[1]
    if shape == (1, 4, 70, 45):      # several tiles per plane, in both directions: asked of the library itself
        assert hu.geometry(*shape[:2], cout, *shape[2:])["tiles_per_plane"] > 1
        assert hu.geometry(*shape[:2], cout, *shape[2:], backward=True)["tiles_per_plane"] > 1
    if shape == (3, 16, 16, 11):
        assert hu.geometry(*shape[:2], cout, *shape[2:])["slabs"] > 3      # more than one slab per image
    worst = [0.0]
    for padding in _paddings(shape):
        for slope in (None, 0.1):
            check(gfla, case, dtype, padding, slope, "%s->%d %s %s slope %s" % (shape, cout, str(dtype)[6:], padding, slope),
                  seed=shape[1] * 100 + shape[3], worst=worst)
    print("sweep worst err/bar %s %s: %.3f" % (shape, str(dtype)[6:], worst[0]))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_one_output_plane(gfla, dtype):
    check(gfla, hu.OUTPUT_PLANE, dtype, "reflect", 0.1, "output plane %s" % str(dtype)[6:], seed=64)


@pytest.mark.parametrize("name", sorted(hu.GOLDENS))
def test_goldens(gfla, name):
    """the reference's own classes in float64, inputs rounded to float32, through the public functional form"""
    shape, cout, post, split, padding, slope = hu.GOLDENS[name]
    g = hu.golden(name)
    inputs = (g["x"].float(), g["weight"].float(), g["bias"].float(), g["up"].float())
    fn = lambda x, w, b: gfla.head_conv3x3(x, w, b, padding, slope, post, split)        # noqa: E731
    got = _run(fn, *inputs, split)
    check(gfla, (shape, cout, post, split), torch.float32, padding, slope, "golden " + name, got=got, inputs=inputs)
    # and against the recorded values themselves: the float32 rounding of the inputs moves them by at most 2^-24 S-ish
    for j, y in enumerate(got[0]):
        assert (y.double().cpu() - g["y%d" % j]).abs().max().item() <= 1e-5
    for a, k in zip(got[1:], ("g_x", "g_weight", "g_bias")):
        assert (a.double().cpu() - g[k]).abs().max().item() <= 1e-5 * max(1.0, g[k].abs().max().item()), k


@pytest.mark.parametrize("case,padding", [(((3, 16, 16, 11), 8, None, 5), "zeros"), (((1, 4, 70, 45), 3, "tanh", None), "reflect")])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda d: str(d)[6:])
def test_bit_identity_and_partial_requests(gfla, case, padding, dtype):
    shape, cout, post, split = case
    x, w, b, up = hu.make_case(shape, cout, dtype, seed=5)
    fn = _kernel(gfla, padding, 0.1, post, split)
    first, again = _run(fn, x, w, b, up, split), _run(fn, x, w, b, up, split)
    for a, c in zip(first[0] + list(first[1:]), again[0] + list(again[1:])):
        assert torch.equal(a, c)
    for need in ((True, False, False), (False, True, False), (False, False, True)):
        only = _run(fn, x, w, b, up, split, need=need)
        for i, wanted in enumerate(need):
            assert (only[1 + i] is not None) == wanted
            if wanted:
                assert torch.equal(only[1 + i], first[1 + i]), need
    # nothing asked: no graph
    y = fn(x.to(DEV), w.to(DEV), b.to(DEV))
    y = y if isinstance(y, tuple) else (y,)
    assert all(t.grad_fn is None for t in y) and all(torch.equal(a, c) for a, c in zip(y, first[0]))
    # no bias
    nb = _run(fn, x, w, None, up, split)
    assert nb[3] is None and (post is not None or torch.equal(nb[2], first[2]))      # (through tanh, y depends on the bias)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_unused_mask_output(gfla, dtype):
    """the mask is not part of the loss: its gradient enters the library as NULL"""
    case = ((2, 20, 9, 13), 6, (None,) * 4 + ("sigmoid",) * 2, 4)
    check(gfla, case, dtype, "zeros", None, "mask unused %s" % str(dtype)[6:], seed=7, use=(1, 0))
    check(gfla, case, dtype, "zeros", 0.1, "flow unused %s" % str(dtype)[6:], seed=8, use=(0, 1))


@pytest.mark.parametrize("dtype", HALF, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("case,padding", [(hu.SWEEP[2], "reflect"), (hu.SWEEP[4], "zeros")], ids=["tanh", "sigmoid"])
def test_sixteen_bit_map_with_float32_parameters(gfla, case, padding, dtype):
    """float32 parameters with a 16-bit map (autocast): the outputs and d x come back in the map's type and are held to
    the sweep's bar (the composition casts the parameters to the map's type, as autocast does); d w and d bias come back
    in float32.  Their derivative of the post-activation is taken from the SAVED
    16-bit output, which alone moves them by about u_16 of their size against the float64 truth -- the torch composition
    does the same, so comparing the two maxima would be a coin toss.  Instead the reduction itself is held to its derived
    bound in float32: the float64 truth is evaluated with g' = g post'(y) from the kernel's own saved outputs (as the VGG
    data-gradient test takes its mask from the kernel's own output), and the bar is the larger of
    2 (B H W + 2) 2^-24 S + 2^-24 |t| and 4 ulp of float32 at the largest entry.  An error in the saved y itself would not
    show in these two rows; y is held to the truth in the rows above."""
    shape, cout, post, split = case
    x, w, b, up = hu.make_case(shape, cout, dtype, seed=21, param_dtype=torch.float32)
    got = _run(_kernel(gfla, padding, 0.1, post, split), x, w, b, up, split)
    assert all(y.dtype == dtype for y in got[0]) and got[1].dtype == dtype
    assert got[2].dtype == torch.float32 and got[3].dtype == torch.float32
    want = hu.truth(x, w, b, up, padding, 0.1, post, split)
    comp = _run(_composition(padding, 0.1, post, split, dtype), x, w, b, up, split)
    n = hu.term_counts(shape, cout)
    rows = [("y%d" % j, y, c, want["y"][j], want["S"]["y"][j], n["y"]) for j, (y, c) in enumerate(zip(got[0], comp[0]))]
    rows.append(("d x", got[1], comp[1], want["gx"], want["S"]["gx"], n["gx"]))
    for what, g, c, t, S, terms in rows:        # the sweep's bar: max of (a), (b), (c)
        err = (g.double().cpu() - t).abs()
        err_c = (c.double().cpu() - t).abs().max().item()
        floor = 4 * hu.ulp(dtype, t.abs().max().item())
        bar = torch.clamp(hu.summation_bound(terms, S, t, dtype), min=max(err_c, floor))
        print("mixed %s %s %s: kernel %.3e, (b) composition %.3e, (c) floor %.3e, worst err/bar %.3f"
              % (str(dtype)[6:], padding, what, err.max().item(), err_c, floor, (err / bar).max().item()))
        assert bool((err <= bar).all()), what
    y_saved = torch.cat([y.double().cpu() for y in got[0]], 1)
    gate = torch.ones_like(y_saved)
    for c, p in enumerate(hu.posts_of(post, cout)):
        if p == "tanh":
            gate[:, c] = 1 - y_saved[:, c] ** 2
        elif p == "sigmoid":
            gate[:, c] = y_saved[:, c] * (1 - y_saved[:, c])
    gp = up.double() * gate
    a = F.leaky_relu(x.double(), 0.1)
    pad = F.pad(a, (1, 1, 1, 1), mode="reflect") if padding == "reflect" else F.pad(a, (1, 1, 1, 1))
    w0 = torch.zeros(w.shape, dtype=torch.float64, requires_grad=True)
    (F.conv2d(pad, w0) * gp).sum().backward()
    s0 = torch.zeros(w.shape, dtype=torch.float64, requires_grad=True)
    (F.conv2d(pad.abs(), s0) * gp.abs()).sum().backward()
    for what, g, t, S in (("d w", got[2], w0.grad, s0.grad), ("d b", got[3], gp.sum(dim=(0, 2, 3)), gp.abs().sum(dim=(0, 2, 3)))):
        err = (g.double().cpu() - t).abs()
        bound = hu.summation_bound(n["gw"], S, t, torch.float32)
        floor = 4 * hu.ulp(torch.float32, t.abs().max().item())
        err_truth = (g.double().cpu() - (want["gw"] if what == "d w" else want["gb"])).abs().max().item()
        print("mixed %s %s %s: kernel %.3e, (a) bound %.3e, (c) floor %.3e, worst err/bar %.3f; against the truth with exact y: %.3e"
              % (str(dtype)[6:], padding, what, err.max().item(), bound.max().item(), floor,
                 (err / torch.clamp(bound, min=floor)).max().item(), err_truth))
        assert bool((err <= torch.clamp(bound, min=floor)).all()), what


@pytest.mark.parametrize("padding", ["zeros", "reflect"])
def test_tie_at_zero_takes_the_slope(gfla, padding):
    """a quarter of x is exactly zero: d x there is the slope times the incoming gradient, as leaky_relu_backward"""
    case = ((2, 5, 9, 13), 3, "tanh", None)
    inputs = hu.make_case(case[0], case[1], torch.float32, seed=11, zeros_in_x=True)
    x = inputs[0]
    assert (x == 0).float().mean().item() > 0.15
    got = check(gfla, case, torch.float32, padding, 0.1, "tie " + padding, inputs=inputs)
    comp = _run(_composition(padding, 0.1, "tanh", None, torch.float32), *inputs, None)
    zero = (x == 0).to(DEV)
    # the other side of the tie would be ten times larger: compare with the composition where x == 0
    scale = comp[1].abs().max().item()
    assert (got[1][zero] - comp[1][zero]).abs().max().item() <= 1e-5 * scale
    flipped = comp[1][zero] * 10
    assert (got[1][zero] - flipped).abs().max().item() > 1e-2 * scale


def test_routing(gfla, monkeypatch):
    ours = gfla.HeadConv3x3Function._backward_cls
    x, w, b, up = hu.make_case((2, 6, 9, 13), 3, torch.float32, seed=15)
    xd, wd, bd = x.to(DEV).requires_grad_(), w.to(DEV), b.to(DEV)
    y = gfla.head_conv3x3(xd, wd, bd, "reflect", 0.1, "tanh")
    assert isinstance(y.grad_fn, ours)
    mod = gfla.HeadConv3x3(6, 3, padding="reflect", pre_slope=0.1, post="tanh").to(DEV)
    with torch.no_grad():
        mod.weight.copy_(wd)
        mod.bias.copy_(bd)
    assert torch.equal(mod(xd), y)
    want = hu.composition(xd, wd, bd, "reflect", 0.1, "tanh", None)[0]
    # Cout = 9, float64 and CPU inputs take the composition and agree with it
    w9 = torch.randn(9, 6, 3, 3, device=DEV) * 0.1
    y9 = gfla.head_conv3x3(xd, w9, None, "zeros", None, None)
    assert not isinstance(y9.grad_fn, ours) and torch.equal(y9, F.conv2d(xd, w9, None, padding=1))
    y64 = gfla.head_conv3x3(xd.double(), wd.double(), bd.double(), "reflect", 0.1, "tanh")
    assert not isinstance(y64.grad_fn, ours) and y64.dtype == torch.float64
    assert (y64 - want.double()).abs().max().item() <= 1e-5
    ycpu = gfla.head_conv3x3(x.requires_grad_(), w, b, "reflect", 0.1, "tanh")
    assert not isinstance(ycpu.grad_fn, ours) and (ycpu - want.cpu()).abs().max().item() <= 1e-5
    # impl="torch" never calls the library
    from global_flow_local_attention_amd import _lib

    def trap(*args, **kwargs):
        raise AssertionError("library call on the torch route")
    monkeypatch.setattr(_lib, "call", trap)
    yt = gfla.head_conv3x3(xd, wd, bd, "reflect", 0.1, "tanh", impl="torch")
    yt.sum().backward()
    assert not isinstance(yt.grad_fn, ours) and torch.equal(yt, want)
    mod.impl = "torch"
    assert torch.equal(mod(xd), want)
    with pytest.raises(AssertionError):
        gfla.head_conv3x3(xd, wd, bd, "reflect", 0.1, "tanh")
    monkeypatch.undo()
    with pytest.raises(TypeError):
        gfla.HeadConv3x3Function.apply(xd.double(), wd, bd, "zeros", None, None, None)
    with pytest.raises(ValueError):
        gfla.HeadConv3x3Function.apply(xd, w9, None, "zeros", None, None, None)


class _Output(nn.Module):
    def __init__(self, cin, cout, nonlinearity):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, kernel_size=3, padding=0, bias=True)
        self.model = nn.Sequential(nonlinearity, nn.ReflectionPad2d(1), self.conv1, nn.Tanh())

    def forward(self, x):
        return self.model(x)


def test_vendor_fence(gfla, monkeypatch):
    """No vendor convolution, pad or activation launch on the path: a fused Output-shaped head and flow_mask_heads run
    forward and backward with F.conv2d, torch.conv2d, F.pad, torch.tanh and torch.sigmoid booby-trapped."""
    torch.manual_seed(6)
    head = _Output(16, 3, nn.LeakyReLU(0.1)).to(DEV)
    flow = nn.Conv2d(16, 2, 3, 1, 1).to(DEV)
    mask = nn.Sequential(nn.Conv2d(16, 1, 3, 1, 1), nn.Sigmoid()).to(DEV)
    x = torch.randn(2, 16, 24, 20, device=DEV, dtype=torch.bfloat16).requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        want = head(x).float()
    assert gfla.fuse_output_heads(head) == 1

    def trap(*args, **kwargs):
        raise AssertionError("vendor library call on the head path")

    for mod, name in ((F, "conv2d"), (torch, "conv2d"), (F, "pad"), (torch, "tanh"), (torch, "sigmoid"), (F, "leaky_relu"),
                      (torch.Tensor, "tanh"), (torch.Tensor, "sigmoid")):
        monkeypatch.setattr(mod, name, trap)
    monkeypatch.setattr(nn.Conv2d, "forward", trap)
    y = head(x)
    f, m = gfla.flow_mask_heads(x, flow, mask)
    assert y.dtype == torch.bfloat16 and f.shape == (2, 2, 24, 20) and m.shape == (2, 1, 24, 20)
    assert f.is_contiguous() and m.is_contiguous()
    (y.float().sum() + f.float().square().sum() + m.float().sum()).backward()
    monkeypatch.undo()
    assert (y.float() - want).abs().max().item() <= 0.05
    for p in list(head.parameters()) + list(flow.parameters()) + list(mask.parameters()) + [x]:
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
    assert m.min() > 0 and m.max() < 1


def test_one_fused_training_step(gfla):
    """the stand-in generator with fuse_output_heads applied (its outconv is Conv2d(c1, 3, 3, 1, 1) -> Tanh) against the
    same network unfused, one optimiser step, within the bars tests/test_trainer_gpu.py holds: every loss term 1e-4
    relative, every gradient 1e-4 of its tensor's largest entry"""
    import trainer_util as tu
    batch = tu.make_batch(2, 64, 48)
    plain_shell, plain_net = tu.build_shell(DEV, ngf=16, lr=1e-3)
    state = {k: v.clone() for k, v in plain_net.state_dict().items()}
    fused_shell, fused_net = tu.build_shell(DEV, ngf=16, lr=1e-3, state=state)
    assert gfla.fuse_output_heads(fused_net) == 1
    assert type(fused_net.outconv[0]) is gfla.HeadConv3x3 and fused_net.outconv[0].post == ("tanh",) * 3
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


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda d: str(d)[6:])
def test_memory(gfla, dtype):
    """forward + backward peak above the inputs stays below the composition's: the composition keeps the activated and the
    padded map, the op keeps neither (x itself is saved, and nothing else of its size)"""
    shape, cout = (4, 64, 64, 44), 3
    x, w, b, up = hu.make_case(shape, cout, dtype, seed=13)
    xs = x.to(DEV).requires_grad_()
    ws, bs, ups = w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_(), up.to(DEV)
    peaks = {}
    for name, fn in (("kernel", _kernel(gfla, "reflect", 0.1, "tanh", None)),
                     ("composition", lambda x_, w_, b_: _composition("reflect", 0.1, "tanh", None, dtype)(x_, w_, b_)[0])):
        for _ in range(2):      # the first pass warms the allocator and loads the code objects
            xs.grad = ws.grad = bs.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            y = fn(xs, ws, bs)
            if name == "kernel":
                saved = y.grad_fn.saved_tensors
                assert saved[0].data_ptr() == xs.data_ptr()
                assert sum(t.numel() >= xs.numel() for t in saved) == 1        # no full-size tensor of its own
            y.backward(ups)
            del y
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - before
    map_bytes = x.numel() * x.element_size()
    print("peak bytes above the inputs, %s: kernel %d (%.2f maps), composition %d (%.2f maps)"
          % (str(dtype)[6:], peaks["kernel"], peaks["kernel"] / map_bytes, peaks["composition"], peaks["composition"] / map_bytes))
    assert peaks["kernel"] < peaks["composition"]
