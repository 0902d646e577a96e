"""VGG19Features on the GPU: csrc/conv3x3.hip and csrc/maxpool2x2.hip layer by layer against float64 host references
computed from the very tensors the kernels read, with derived (not measured) bars, then the whole network: golden values
of the reference's own class, the full-width network in bfloat16, the vendor fence, determinism and autocast.

Forward bar of a convolution (the kernel sums K = 9 Cin products and a bias in float32, in an order of its own):
    |y - y64| <= 2 (K + 2) 2^-24 S + u |y64|,   S = conv(|x|, |w|) + |b| in float64,
u = 0 (float32), 2^-11 (float16), 2^-8 (bfloat16): the one rounding of a 16-bit result.  The absolute term also covers a
sign flip at the ReLU.  The data gradient has the same bar with K = 9 Cout and S = conv_transpose(|g mask|, |w|), the mask
taken from the kernel's own saved output."""
import pytest
import torch
import torch.nn.functional as F

import vgg_util as vu
from vgg_util import conv_inputs

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
# (B, Cin, Cout, H, W): first layer with one padded chunk; nothing a multiple of anything, tiles straddle both edges; all
# halo (twice); several channel chunks and channel blocks; the longest reduction
CONV_SHAPES = [(1, 3, 64, 9, 7), (2, 20, 40, 33, 17), (1, 64, 64, 1, 1), (1, 16, 32, 1, 40), (3, 128, 96, 16, 11)]
CONV_CASES = [(n, s) for s in CONV_SHAPES for n in ("f32", "f16", "bf16")] + \
             [(n, (1, 512, 512, 4, 3)) for n in ("f32", "bf16")]


@pytest.mark.parametrize("name,shape", CONV_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_conv3x3_relu_forward_and_data_gradient(gfla, name, shape):
    dtype = DTYPES[name]
    B, Cin, Cout, H, W = shape
    x, w, b, gy = conv_inputs(shape, dtype, seed=sum(shape))
    xg = x.cuda().requires_grad_()
    # parameters held in float32 (values already representable in the compute type): the packing converts them
    y = gfla.conv3x3_relu(xg, w.float().cuda(), b.float().cuda())
    assert y.dtype == dtype and y.shape == (B, Cout, H, W) and y.grad_fn is not None
    y64, S = vu.conv_ref64(x, w, b)
    err = (y.detach().cpu().double() - y64).abs()
    bar = vu.conv_bar(S, y64, 9 * Cin, dtype)
    print("fwd %s %s: max err %.3e, max err/bar %.3f" % (name, shape, err.max(), (err / bar.clamp_min(1e-300)).max()))
    assert (err <= bar).all()
    assert (y.detach() >= 0).all()
    y.backward(gy.cuda())
    dx64, Sg = vu.dgrad_ref64(gy, y, w)
    assert xg.grad.dtype == dtype and xg.grad.shape == x.shape
    err = (xg.grad.cpu().double() - dx64).abs()
    bar = vu.conv_bar(Sg, dx64, 9 * Cout, dtype)
    print("bwd %s %s: max err %.3e, max err/bar %.3f" % (name, shape, err.max(), (err / bar.clamp_min(1e-300)).max()))
    assert (err <= bar).all()


@pytest.mark.parametrize("name", list(DTYPES))
def test_parameters_in_another_float_type_are_packed_into_the_activation_dtype(gfla, name):
    dtype = DTYPES[name]
    other = torch.bfloat16 if dtype != torch.bfloat16 else torch.float16
    x, w, b, _ = conv_inputs((1, 5, 7, 6, 9), other, seed=4)      # parameters representable in `other`
    x = x.float().to(dtype)
    y = gfla.conv3x3_relu(x.cuda(), w.cuda(), b.cuda())
    assert y.dtype == dtype
    wr, br = w.float().to(dtype), b.float().to(dtype)              # one rounding to the compute type
    y64, S = vu.conv_ref64(x, wr, br)
    assert ((y.cpu().double() - y64).abs() <= vu.conv_bar(S, y64, 45, dtype)).all()


def test_input_without_gradient_saves_nothing(gfla):
    x, w, b, _ = conv_inputs((1, 3, 8, 6, 5), torch.float32, seed=1)
    y = gfla.conv3x3_relu(x.cuda(), w.cuda(), b.cuda())
    assert y.grad_fn is None and not y.requires_grad
    p = gfla.maxpool2x2(y)
    assert p.grad_fn is None
    # a weight that requires a gradient takes the composition (the kernels have no weight gradient)
    wg = w.cuda().requires_grad_()
    y2 = gfla.conv3x3_relu(x.cuda(), wg, b.cuda())
    y2.sum().backward()
    assert wg.grad is not None and torch.allclose(y2, y, atol=1e-5)


def pool_input(kind, dtype):
    g = torch.Generator().manual_seed(11)
    if kind == "ties":
        return (torch.randn(2, 3, 9, 12, generator=g) * 2).round().div(2).clamp(-1, 1).to(dtype)   # multiples of 0.5
    if kind.startswith("nan"):
        # the odd map with a NaN in slot 0..3 (scan order) of one window, and in two slots of another: F.max_pool2d returns
        # NaN for a window with a NaN in it and routes the gradient to the last one
        x = torch.randn(2, 5, 7, 9, generator=g).to(dtype)
        slot = int(kind[3])
        x[0, 3, 4 + slot // 2, 6 + slot % 2] = float("nan")
        x[1, 0, 0, 0] = x[1, 0, 1, slot % 2] = float("nan")
        return x
    shape = {"odd": (2, 5, 7, 9), "empty": (1, 3, 1, 1), "even": (1, 64, 16, 10)}[kind]
    return torch.randn(shape, generator=g).to(dtype)


def equal_with_nans(a, b):
    """torch.equal that takes a NaN for equal to a NaN: equal NaN masks, equal values elsewhere"""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("kind", ["odd", "empty", "even", "ties", "nan0", "nan1", "nan2", "nan3"])
def test_maxpool2x2_is_bit_equal_to_torch(gfla, kind, name):
    dtype = DTYPES[name]
    x = pool_input(kind, dtype)
    if kind.startswith("nan"):
        xg = x.cuda().requires_grad_()
        y = gfla.maxpool2x2(xg)
        xr = x.float().requires_grad_()
        yr = F.max_pool2d(xr, kernel_size=2, stride=2)
        assert int(torch.isnan(yr).sum()) == 2
        assert y.dtype == dtype and equal_with_nans(y.detach().cpu().float(), yr.detach())
        g = torch.randn(yr.shape, generator=torch.Generator().manual_seed(5)).to(dtype)
        g = g + (g == 0).to(dtype)
        y.backward(g.cuda())
        yr.backward(g.float())
        assert torch.equal(xg.grad.cpu().float(), xr.grad)           # routed exactly: the gradient itself has no NaN
        assert not xg.grad[:, :, 6].any() and not xg.grad[:, :, :, 8].any()
        return
    xg = x.cuda().requires_grad_()
    y = gfla.maxpool2x2(xg)
    if kind == "empty":
        # H = W = 1: F.max_pool2d itself refuses an empty output; the kernels support it: an empty map, a zero gradient
        assert y.shape == (1, 3, 0, 0) and y.dtype == dtype and y.grad_fn is not None
        y.sum().backward()
        assert xg.grad.dtype == dtype and torch.equal(xg.grad.cpu(), torch.zeros_like(x))
        return
    # reference on the host, on the widened values (exact): F.max_pool2d and its gradient routing
    xr = x.float().requires_grad_()
    yr = F.max_pool2d(xr, kernel_size=2, stride=2)
    assert y.dtype == dtype and y.shape == yr.shape
    assert torch.equal(y.detach().cpu().float(), yr.detach())
    g = torch.randn(yr.shape, generator=torch.Generator().manual_seed(5)).to(dtype)
    g = g + (g == 0).to(dtype)                                       # no zero: an unwritten or misrouted entry shows
    y.backward(g.cuda())
    yr.backward(g.float())
    assert xg.grad.dtype == dtype
    # dropped last row / column and every loser are exactly zero: the whole of dX is written by the kernel
    assert torch.equal(xg.grad.cpu().float(), xr.grad)
    if kind == "odd":
        assert not xg.grad[:, :, 6].any() and not xg.grad[:, :, :, 8].any()
    if kind == "ties":
        win = F.max_pool2d(x.float(), 2, 2).repeat_interleave(2, 2).repeat_interleave(2, 3)
        assert ((x.float()[:, :, :8, :12] == win).sum() > 1.3 * yr.numel())     # ties are frequent in this input


def cuda_golden_module(gfla, gold, dtype=torch.float32, impl="auto"):
    m = gfla.VGG19Features(widths=vu.GOLDEN_WIDTHS, impl=impl)
    m.load_state_dict(vu.golden_state_dict(gold, torch.float32), strict=True)
    return m.cuda().to(dtype)


def relative_errors(out, grad, gold, tag):
    """largest |got - golden| / max |golden| per map, and the same for the image gradient"""
    errs = {}
    for layer in vu.LAYERS:
        want = gold["%s/out/%s" % (tag, layer)]
        errs[layer] = ((out[layer].detach().cpu().double() - want).abs().max() / want.abs().max()).item()
    want = gold[tag + "/grad_image"]
    errs["grad_image"] = ((grad.cpu().double() - want).abs().max() / want.abs().max()).item()
    return errs


def run_with_r(module, image, gold, tag):
    image = image.clone().requires_grad_()
    out = module(image)
    total = 0
    for layer in vu.LAYERS:
        total = total + (out[layer] * gold["%s/r/%s" % (tag, layer)].to(image)).sum()
    total.backward()
    return out, image.grad


@pytest.mark.parametrize("tag", vu.GOLDEN_IMAGES)
def test_golden_network_float32(gfla, tag):
    # The bar is measured in the test, not guessed: torch's own float32 composition on the HOST (F.conv2d / F.max_pool2d,
    # vu.TorchVGG: never the code under test) against the same float64 golden, largest relative error over the sixteen
    # maps and the image gradient; the kernels get 4x of it (another valid float32 summation order).  Measured on the
    # golden file of this commit: host composition 6.6e-7 (image a, relu5_4), 4.3e-7 (image b, relu3_2) -> bars 2.6e-6 / 1.7e-6.
    gold = vu.load_golden()
    host = vu.TorchVGG(vu.golden_state_dict(gold, torch.float32))
    out, grad = run_with_r(host, gold[tag + "/image"].float(), gold, tag)
    measured = max(relative_errors(out, grad, gold, tag).values())
    bar = 4 * measured
    m = cuda_golden_module(gfla, gold)
    out, grad = run_with_r(m, gold[tag + "/image"].float().cuda(), gold, tag)
    assert out["relu3_3"] is out["relu3_2"] and all(v.dtype == torch.float32 and v.is_cuda for v in out.values())
    errs = relative_errors(out, grad, gold, tag)
    print("golden %s: host float32 composition %.3e, bar %.3e, kernels %.3e (%s)"
          % (tag, measured, bar, max(errs.values()), max(errs, key=errs.get)))
    assert 0 < measured < 1e-5
    for key, e in errs.items():
        assert e <= bar, (key, e, bar)


def test_full_width_bfloat16_layer_by_layer(gfla):
    """VGG19Features() at full width, He-scaled random weights, bfloat16: every layer against the float64 evaluation of
    that layer on the kernel's own previous output, so compounding needs no number."""
    m = gfla.VGG19Features()
    m.load_torchvision_state_dict(vu.torchvision_features(m.widths, seed=7).state_dict())
    m = m.cuda().to(torch.bfloat16)
    image = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).cuda()
    whole = m(image)
    x = image
    for name in vu.LAYERS:
        for sub in getattr(m, name):
            y = sub(x)
            if isinstance(sub, torch.nn.Conv2d):
                y64, S = vu.conv_ref64(x, sub.weight, sub.bias)
                err = (y.cpu().double() - y64).abs()
                assert (err <= vu.conv_bar(S, y64, 9 * sub.in_channels, torch.bfloat16)).all(), name
                assert (y64 > 0).double().mean() > 0.05, name               # the layer is alive
            elif isinstance(sub, type(m.relu2_1[0])):
                assert torch.equal(y.cpu().float(), F.max_pool2d(x.cpu().float(), 2, 2)), name
            x = y
        assert torch.equal(x, whole[name]), name


def test_vendor_fence(gfla, monkeypatch):
    """No vendor convolution / GEMM on the path: VGGLoss and PerceptualCorrectness around VGG19Features run with
    F.conv2d, torch.conv2d, F.max_pool2d and torch.bmm booby-trapped."""
    vgg = gfla.VGG19Features(widths=(8, 8, 16, 16, 16))
    vgg.load_torchvision_state_dict(vu.torchvision_features(vgg.widths, seed=5).state_dict())
    vgg = vgg.cuda()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 32, 24, generator=g).to(torch.bfloat16).cuda().requires_grad_()
    y = torch.randn(2, 3, 32, 24, generator=g).to(torch.bfloat16).cuda()
    flow = torch.randn(2, 2, 8, 6, generator=g).cuda().requires_grad_()

    def trap(*args, **kwargs):
        raise AssertionError("vendor library call on the VGG19Features path")

    monkeypatch.setattr(F, "conv2d", trap)
    monkeypatch.setattr(torch, "conv2d", trap)
    monkeypatch.setattr(torch.nn.functional, "max_pool2d", trap)
    monkeypatch.setattr(torch, "bmm", trap)
    content, style = gfla.VGGLoss(vgg=vgg)(x, y)
    (content + style).backward()
    assert torch.isfinite(content) and torch.isfinite(style) and style > 0 and content > 0
    assert x.grad is not None and x.grad.dtype == torch.bfloat16 and x.grad.abs().max() > 0
    loss = gfla.PerceptualCorrectness(vgg=vgg)(y, x.detach(), [flow], [2])      # layer[2] = relu3_1
    loss.backward()
    assert torch.isfinite(loss) and flow.grad is not None and torch.isfinite(flow.grad).all()


def test_determinism(gfla):
    gold = vu.load_golden()
    m = cuda_golden_module(gfla, gold)
    image = gold["a/image"].float().cuda()
    first = run_with_r(m, image, gold, "a")
    second = run_with_r(m, image, gold, "a")
    for layer in vu.LAYERS:
        assert torch.equal(first[0][layer], second[0][layer]), layer
    assert torch.equal(first[1], second[1])


def test_autocast_runs_the_16_bit_kernels(gfla):
    gold = vu.load_golden()
    m = cuda_golden_module(gfla, gold)
    image = gold["b/image"].float().cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        auto = m(image)
    direct = m(image.bfloat16())
    for layer in vu.LAYERS:
        assert auto[layer].dtype == torch.bfloat16 and torch.equal(auto[layer], direct[layer]), layer
