"""The gradients of the generator convolutions on the GPU (gen_conv.GenConvFunction; csrc/gen_conv_bwd.hip,
csrc/gen_conv_wgrad.hip): every gradient of every geometry against float64 host gradients built from the very tensors
the kernels read, with the derived bars

    |grad_x - grad_x64| <= 2 (K + 2) 2^-24 S_x + u |grad_x64|,    K = 9 Cout (S1K3, T2K3), 4 Cout (S2K4)
    |grad_w - grad_w64| <= 2 (K + 2) 2^-24 S_w + u_w |grad_w64|,  K = B H W (S1K3, T2K3), B Hout Wout (S2K4)
    |grad_b - grad_b64| <= 2 (K + 2) 2^-24 sum |g| + u_w |grad_b64|

(S: the same gradient from |g|, |a|, |w|; u of x's dtype, u_w of the parameter's), then only-what-is-asked-for,
determinism, autocast, a training step of a whole generator-shaped network behind the vendor fence, and the parity of its
gradients with the unrewritten network.  The figures measured on an MI355X are in DESIGN.md, "Generator convolutions:
gradients"."""
import pytest
import torch
import torch.nn.functional as F

import gen_conv_train_util as tu
import gen_conv_util as gu
from gen_conv_util import DTYPES, bar, call, case_id as _id, conv_inputs

pytestmark = pytest.mark.gpu


def _call(gfla, geometry, x, w, b, reflect, slope, add):
    if geometry == gu.S1K3:
        return gfla.conv3x3(x, w, b, padding="reflect" if reflect else "zeros", pre_slope=slope, add=add, grad="kernels")
    if geometry == gu.S2K4:
        return gfla.conv4x4_down(x, w, b, pre_slope=slope, grad="kernels")
    return gfla.conv_transpose3x3_up(x, w, b, add=add, pre_slope=slope, grad="kernels")


def _leaves(tensors, needs):
    return [None if t is None else t.detach().clone().requires_grad_(need) for t, need in zip(tensors, needs)]


def _case(geometry, name, shape, opts):
    """the seeded inputs of a case on the GPU: x in its dtype, float32 parameters representable in it, addend, upstream"""
    dtype = DTYPES[name]
    x, w, b, add = conv_inputs(geometry, shape, dtype, seed=sum(shape) + geometry, with_add=bool(opts.get("add")))
    g = tu.upstream(geometry, shape, dtype, seed=sum(shape))
    return x, w, b, add, g


def check_gradients(gfla, geometry, name, shape, opts):
    dtype = DTYPES[name]
    B, Cin, Cout, H, W = shape
    reflect, slope = bool(opts.get("reflect")), opts.get("slope")
    x, w, b, add, g = _case(geometry, name, shape, opts)
    xg, wg, bg, ag = _leaves((x.cuda(), w.float().cuda(), b.float().cuda(), None if add is None else add.cuda()), (True,) * 4)
    y = _call(gfla, geometry, xg, wg, bg, reflect, slope, ag)
    assert y.dtype == dtype and type(y.grad_fn).__name__ == "GenConvFunctionBackward"
    with torch.no_grad():                             # the forward is the inference launch, bit for bit
        assert torch.equal(y, call(gfla, geometry, xg, wg, bg, reflect, slope, ag))
    y.backward(g.cuda())
    assert xg.grad.dtype == dtype and wg.grad.dtype == bg.grad.dtype == torch.float32
    assert ag is None or (ag.grad.dtype == dtype and torch.equal(ag.grad.cpu(), g))
    (gx64, gw64, gb64), (Sx, Sw, Sb) = tu.grads64(geometry, x, w, b, g, reflect, slope)
    worst = []
    for what, got, want, S, K, u in (
            ("grad_x", xg.grad, gx64, Sx, tu.data_reduction_length(geometry, Cout), dtype),
            ("grad_w", wg.grad, gw64, Sw, tu.weight_reduction_length(geometry, shape), torch.float32),
            ("grad_b", bg.grad, gb64, Sb, tu.weight_reduction_length(geometry, shape), torch.float32)):
        assert got.shape == want.shape and torch.isfinite(got).all(), what
        err = (got.cpu().double() - want).abs()
        limit = bar(S, want, K, u, False)
        worst.append((what, err.max().item(), (err / limit.clamp_min(1e-300)).max().item(), bool((err <= limit).all())))
    print("geometry %d %s %s %s: " % (geometry, name, shape, opts)
          + ", ".join("%s max err %.3e err/bar %.3f" % w3[:3] for w3 in worst))
    assert all(w3[3] for w3 in worst), worst
    return xg.grad, wg.grad, bg.grad


@pytest.mark.parametrize("name,shape,opts", tu.S1K3_CASES, ids=_id)
def test_s1k3_gradients(gfla, name, shape, opts):
    check_gradients(gfla, gu.S1K3, name, shape, opts)


@pytest.mark.parametrize("name,shape,opts", tu.S2K4_CASES, ids=_id)
def test_s2k4_gradients(gfla, name, shape, opts):
    check_gradients(gfla, gu.S2K4, name, shape, opts)


@pytest.mark.parametrize("name,shape,opts", tu.T2K3_CASES, ids=_id)
def test_t2k3_gradients(gfla, name, shape, opts):
    check_gradients(gfla, gu.T2K3, name, shape, opts)


@pytest.mark.parametrize("geometry,opts", [(gu.S1K3, {"reflect": True, "slope": 0.1}), (gu.S2K4, {"slope": 0.1}), (gu.T2K3, {})],
                         ids=["s1k3", "s2k4", "t2k3"])
def test_only_what_is_asked_for(gfla, geometry, opts):
    shape, name = (2, 20, 40, 17, 9), "f32"
    reflect, slope = bool(opts.get("reflect")), opts.get("slope")
    full = check_gradients(gfla, geometry, name, shape, opts)
    x, w, b, _, g = _case(geometry, name, shape, opts)
    x, w, b, g = x.cuda(), w.cuda(), b.cuda(), g.cuda()
    xg, wg, bg, _ = _leaves((x, w, b, None), (True, False, False, False))
    _call(gfla, geometry, xg, wg, bg, reflect, slope, None).backward(g)
    assert wg.grad is None and bg.grad is None and torch.equal(xg.grad, full[0])
    xg, wg, bg, _ = _leaves((x, w, b, None), (False, True, True, False))
    _call(gfla, geometry, xg, wg, bg, reflect, slope, None).backward(g)
    assert xg.grad is None and torch.equal(wg.grad, full[1]) and torch.equal(bg.grad, full[2])
    xg, wg, bg, _ = _leaves((x, w, b, None), (False, False, True, False))            # the bias alone
    _call(gfla, geometry, xg, wg, bg, reflect, slope, None).backward(g)
    assert xg.grad is None and wg.grad is None and torch.equal(bg.grad, full[2])
    # a non-contiguous upstream gradient
    strided = torch.empty(g.shape[:3] + (2 * g.shape[3],), dtype=g.dtype, device=g.device)[..., ::2]
    strided.copy_(g)
    assert not strided.is_contiguous()
    xg, wg, bg, _ = _leaves((x, w, b, None), (True, True, True, False))
    _call(gfla, geometry, xg, wg, bg, reflect, slope, None).backward(strided)
    assert all(torch.equal(a, b) for a, b in zip((xg.grad, wg.grad, bg.grad), full))


@pytest.mark.parametrize("geometry", [gu.S1K3, gu.S2K4, gu.T2K3])
def test_determinism(gfla, geometry):
    shape = (2, 40, 72, 19, 21)
    x, w, b, add = conv_inputs(geometry, shape, torch.float32, seed=3, with_add=geometry != gu.S2K4)
    g = tu.upstream(geometry, shape, torch.float32, seed=3).cuda()
    runs = []
    for _ in range(2):
        leaves = _leaves([t if t is None else t.cuda() for t in (x, w, b, add)], (True,) * 4)
        _call(gfla, geometry, *leaves[:3], geometry == gu.S1K3, 0.1, leaves[3]).backward(g)
        runs.append([t.grad for t in leaves if t is not None])
    assert all(a is not None and torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("geometry", [gu.S1K3, gu.S2K4, gu.T2K3])
def test_autocast(gfla, geometry):
    shape = (2, 12, 20, 10, 7)
    x, w, b, _ = conv_inputs(geometry, shape, torch.float32, seed=6, with_add=False)
    g = tu.upstream(geometry, shape, torch.bfloat16, seed=6).cuda()
    xa, wa, ba, _ = _leaves((x.cuda(), w.cuda(), b.cuda(), None), (True,) * 4)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ya = _call(gfla, geometry, xa, wa, ba, False, 0.1, None)
    assert ya.dtype == torch.bfloat16
    ya.backward(g)
    assert xa.grad.dtype == wa.grad.dtype == ba.grad.dtype == torch.float32
    xd, wd, bd, _ = _leaves((x.cuda().bfloat16(), w.cuda(), b.cuda(), None), (True,) * 4)
    yd = _call(gfla, geometry, xd, wd, bd, False, 0.1, None)
    yd.backward(g)
    assert torch.equal(ya, yd) and torch.equal(xa.grad, xd.grad.float())
    assert torch.equal(wa.grad, wd.grad) and torch.equal(ba.grad, bd.grad)


# ---- the whole network -------------------------------------------------------------------------------------------------
def test_training_step_behind_the_vendor_fence(gfla, monkeypatch):
    (net,), _, image = tu.conv_generators("cuda", copies=1)
    assert tu.rewrite(gfla, net) == (14, 3, 16) and net.training
    assert not any(type(m) in (torch.nn.Conv2d, torch.nn.ConvTranspose2d) for m in net.modules())

    def trap(*args, **kwargs):
        raise AssertionError("vendor library call in the generator's training step")

    for mod, name in ((F, "conv2d"), (torch, "conv2d"), (F, "conv_transpose2d"), (torch, "conv_transpose2d"), (torch, "bmm"),
                      (torch.nn.grad, "conv2d_input"), (torch.nn.grad, "conv2d_weight")):
        monkeypatch.setattr(mod, name, trap)
    net(image.cuda()).square().mean().backward()
    for key, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, key


def test_whole_network_gradient_parity(gfla):
    """The rule of test_whole_network_parity, on gradients: the bar is 4x the distance of the UNREWRITTEN float32 GPU
    network's gradients from a float64 host evaluation, the largest over the parameters of (largest error / scale of the
    parameter); every parameter of the rewritten network is within it of the unrewritten one, relative to the same scale.
    The scale of a parameter is its largest float64 gradient entry -- except where that gradient is zero in exact
    arithmetic: the bias of a convolution whose output goes straight into an InstanceNorm2d is cancelled by the norm's mean,
    its float64 gradient is rounding noise (1e-18 here) and no error can be measured relative to it.  Such a parameter
    (largest float64 entry below 1e-10 of the network's largest) is measured on the network's largest gradient entry
    instead, in `measured` and in its own check alike; none is left out."""
    (fused, plain), host, image = tu.conv_generators("cuda")
    tu.rewrite(gfla, fused)
    host(image.double()).square().mean().backward()
    plain(image.cuda()).square().mean().backward()
    fused(image.cuda()).square().mean().backward()
    want = {k: p.grad for k, p in host.named_parameters()}
    base = {k: p.grad.cpu().double() for k, p in plain.named_parameters()}
    got = {k: p.grad.cpu().double() for k, p in fused.named_parameters()}
    assert set(want) == set(base) == set(got) and all(p.grad.dtype == torch.float32 for p in fused.parameters())
    top = max(w.abs().max().item() for w in want.values())
    scale = {k: w.abs().max().item() if w.abs().max().item() >= 1e-10 * top else top for k, w in want.items()}
    cancelled = sorted(k for k in want if scale[k] == top and want[k].abs().max().item() < 1e-10 * top)
    assert all(k.endswith(".bias") for k in cancelled) and len(cancelled) < len(want) / 2, cancelled
    measured = max(((base[k] - want[k]).abs().max() / scale[k]).item() for k in want)
    own = max(((got[k] - want[k]).abs().max() / scale[k]).item() for k in want)
    print("conv generator gradients: unrewritten float32 network %.3e from float64, bar %.3e, rewritten network %.3e; "
          "%d of %d parameters (biases in front of a norm) on the network's scale"
          % (measured, 4 * measured, own, len(cancelled), len(want)))
    assert 0 < measured < 1e-4
    for k in want:
        assert ((got[k] - base[k]).abs().max() / scale[k]).item() <= 4 * measured, k
