"""Generator inference convolutions on the GPU (csrc/gen_conv.hip): each geometry against a float64 host reference built
from the very tensors the kernel reads, with the derived bar of gen_conv_util.bar

    |y - y64| <= 2 (K + 2 + a) 2^-24 S + u |y64|,   S = conv(|act(x)|, |w|) + |b| + |add|,

K = 9 Cin (S1K3), 16 Cin (S2K4), 4 Cin (T2K3: the deepest phase), a = 1 with an addend, u = 0 / 2^-11 / 2^-8; then dispatch,
determinism, autocast, and a whole generator-shaped network: the vendor fence and parity with the unrewritten network.

Whole-network figures measured on an MI355X (printed by test_whole_network_parity): see DESIGN.md, "Generator inference
convolutions"."""
import pytest
import torch
import torch.nn.functional as F

import gen_conv_util as gu
from gen_conv_util import (ALL, DTYPES, S1K3_CASES, S2K4_CASES, T2K3_CASES, call, call_in_place, case_id as _id,
                           conv_inputs)

pytestmark = pytest.mark.gpu


def check_forward(gfla, geometry, name, shape, opts):
    dtype = DTYPES[name]
    B, Cin, Cout, H, W = shape
    reflect, slope = bool(opts.get("reflect")), opts.get("slope")
    has_add = bool(opts.get("add") or opts.get("alias"))
    x, w, b, add = conv_inputs(geometry, shape, dtype, seed=sum(shape) + geometry, with_add=has_add)
    with torch.no_grad():
        # parameters held in float32 (values already representable in the compute type): the packing converts them
        if opts.get("alias"):
            y = call_in_place(x.cuda(), w.float().cuda(), b.float().cuda(), add.cuda())
        else:
            y = call(gfla, geometry, x.cuda(), w.float().cuda(), b.float().cuda(), reflect, slope,
                     None if add is None else add.cuda())
    assert y.dtype == dtype and y.shape == (B, Cout) + gu.out_size(geometry, H, W) and y.grad_fn is None
    y64, S = gu.ref64(geometry, x, w, b, reflect, slope, add)
    err = (y.cpu().double() - y64).abs()
    bar = gu.bar(S, y64, gu.reduction_length(geometry, Cin), dtype, has_add)
    print("geometry %d %s %s %s: max err %.3e, max err/bar %.3f"
          % (geometry, name, shape, opts, err.max(), (err / bar.clamp_min(1e-300)).max()))
    assert torch.isfinite(y).all() and (err <= bar).all()


@pytest.mark.parametrize("name,shape,opts", S1K3_CASES, ids=_id)
def test_s1k3_forward(gfla, name, shape, opts):
    check_forward(gfla, gu.S1K3, name, shape, opts)


@pytest.mark.parametrize("name,shape,opts", S2K4_CASES, ids=_id)
def test_s2k4_forward(gfla, name, shape, opts):
    check_forward(gfla, gu.S2K4, name, shape, opts)


@pytest.mark.parametrize("name,shape,opts", T2K3_CASES, ids=_id)
def test_t2k3_forward(gfla, name, shape, opts):
    check_forward(gfla, gu.T2K3, name, shape, opts)


@pytest.mark.parametrize("geometry", [gu.S1K3, gu.S2K4, gu.T2K3])
@pytest.mark.parametrize("name", ALL)
def test_parameters_in_another_float_type_are_packed_into_the_activation_dtype(gfla, geometry, name):
    dtype = DTYPES[name]
    other = torch.bfloat16 if dtype != torch.bfloat16 else torch.float16
    shape = (1, 5, 7, 6, 9)
    x, w, b, _ = conv_inputs(geometry, shape, other, seed=4, with_add=False)      # parameters representable in `other`
    x = x.float().to(dtype)
    with torch.no_grad():
        y = call(gfla, geometry, x.cuda(), w.cuda(), b.cuda())
    assert y.dtype == dtype
    wr, br = w.float().to(dtype), b.float().to(dtype)                              # one rounding to the compute type
    y64, S = gu.ref64(geometry, x, wr, br)
    assert ((y.cpu().double() - y64).abs() <= gu.bar(S, y64, gu.reduction_length(geometry, 5), dtype, False)).all()


@pytest.mark.parametrize("geometry", [gu.S1K3, gu.S2K4, gu.T2K3])
def test_dispatch_on_gradients(gfla, geometry):
    x, w, b, _ = conv_inputs(geometry, (2, 6, 9, 8, 6), torch.float32, seed=2, with_add=False)
    x, w, b = x.cuda(), w.cuda(), b.cuda()
    with torch.no_grad():
        y = call(gfla, geometry, x, w, b, slope=0.2)
    assert y.grad_fn is None and not y.requires_grad
    frozen = call(gfla, geometry, x, w, b, slope=0.2)                  # grad mode, but nothing requires a gradient: the kernel
    assert frozen.grad_fn is None and torch.equal(frozen, y)
    for which in ("x", "w"):
        xg = x.clone().requires_grad_(which == "x")
        wg = w.clone().requires_grad_(which == "w")
        yg = call(gfla, geometry, xg, wg, b, slope=0.2)                # the composition, with its gradients
        assert yg.grad_fn is not None and torch.allclose(yg, y, atol=1e-4, rtol=1e-4)
        yg.sum().backward()
        assert (xg.grad if which == "x" else wg.grad) is not None
        with torch.no_grad():
            again = call(gfla, geometry, xg, wg, b, slope=0.2)         # the same call under no_grad: the kernel
        assert again.grad_fn is None and torch.equal(again, y)
    # the module: Parameters require gradients, so grad mode decides
    conv = {gu.S1K3: torch.nn.Conv2d(6, 9, 3, 1, 1), gu.S2K4: torch.nn.Conv2d(6, 9, 4, 2, 1),
            gu.T2K3: torch.nn.ConvTranspose2d(6, 9, 3, 2, 1, output_padding=1)}[geometry].cuda()
    seq = torch.nn.Sequential(torch.nn.LeakyReLU(0.2), conv)
    want = seq(x)
    assert gfla.fuse_inference_convs(seq) == 1 and seq[1].pre_slope == 0.2
    assert seq(x).grad_fn is not None and torch.allclose(seq(x), want, atol=1e-6, rtol=1e-6)
    with torch.no_grad():
        got = seq(x)
    assert got.grad_fn is None and torch.allclose(got, want, atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("geometry", [gu.S1K3, gu.S2K4, gu.T2K3])
def test_determinism(gfla, geometry):
    x, w, b, add = conv_inputs(geometry, (2, 40, 72, 19, 21), torch.float32, seed=3, with_add=geometry != gu.S2K4)
    args = [t if t is None else t.cuda() for t in (x, w, b, add)]
    with torch.no_grad():
        first = call(gfla, geometry, *args[:3], slope=0.1, add=args[3])
        second = call(gfla, geometry, *args[:3], slope=0.1, add=args[3])
    assert torch.equal(first, second)


@pytest.mark.parametrize("geometry", [gu.S1K3, gu.S2K4, gu.T2K3])
def test_autocast_runs_the_16_bit_kernels(gfla, geometry):
    x, w, b, add = conv_inputs(geometry, (2, 12, 20, 10, 7), torch.float32, seed=6, with_add=geometry != gu.S2K4)
    x, w, b = x.cuda(), w.cuda(), b.cuda()
    add = None if add is None else add.cuda()
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            auto = call(gfla, geometry, x, w, b, slope=0.1, add=add)
        direct = call(gfla, geometry, x.bfloat16(), w, b, slope=0.1, add=None if add is None else add.bfloat16())
    assert auto.dtype == torch.bfloat16 and torch.equal(auto, direct)


# ---- the whole network -------------------------------------------------------------------------------------------------
def _standin(gfla, device):
    """(rewritten network or None, plain network, float64 host network, inputs): the same parameters in all three"""
    from oracle import cpu_modules
    torch.manual_seed(7)
    host = gu.StandInGenerator(cpu_modules.ExtractorAttnCPU)
    with torch.no_grad():                 # hidden FC activations clear of the LeakyReLU kink, both slopes in use (trainer_util)
        bias = host.attn.fully_connect_layer[0].bias
        bias.copy_(torch.where(torch.arange(bias.numel()) % 2 == 0, 8.0, -8.0) + 0.1 * bias)
    state = host.state_dict()
    nets = []
    for _ in range(2):
        net = gu.StandInGenerator(gfla.ExtractorAttn)
        net.load_state_dict(state)
        nets.append(net.to(device).eval())
    g = torch.Generator().manual_seed(8)
    inputs = (torch.rand(2, 3, 32, 24, generator=g) * 2 - 1, torch.rand(2, 6, 32, 24, generator=g),
              torch.randn(2, 2, 4, 3, generator=g))
    return nets[0], nets[1], host.double().eval(), inputs


def _rewrite(gfla, net):
    counts = (gfla.fuse_instance_norm_act(net), gfla.fuse_output_heads(net), gfla.fuse_inference_convs(net))
    # 6 encoder + 1 residual + 3 decoder blocks of two norm + activation pairs each; 6 x 2 + 2 + 3 x 3 + 1 = 24 convolutions
    # of the body, of which the three 3x3 with 8 output channels go to head_conv.py's kernel like the image head
    assert counts == (20, 4, 21), counts
    return net


def test_whole_network_behind_the_vendor_fence(gfla, monkeypatch):
    fused, _, _, inputs = _standin(gfla, "cuda")
    _rewrite(gfla, fused)
    assert not any(type(m) in (torch.nn.Conv2d, torch.nn.ConvTranspose2d) for n, m in fused.named_modules()
                   if "fully_connect_layer" not in n)

    def trap(*args, **kwargs):
        raise AssertionError("vendor library call on the generator's inference path")

    for mod, name in ((F, "conv2d"), (torch, "conv2d"), (F, "conv_transpose2d"), (torch, "conv_transpose2d"), (torch, "bmm")):
        monkeypatch.setattr(mod, name, trap)
    with torch.no_grad():
        image = fused(*(t.cuda() for t in inputs))
    assert image.shape == (2, 3, 32, 24) and torch.isfinite(image).all() and image.abs().max() > 0


def test_whole_network_parity(gfla):
    """The rule of test_golden_network_float32: the bar is 4x the distance of the UNREWRITTEN float32 GPU network from a
    float64 host evaluation of the same network, each measured as the largest error over the largest entry."""
    fused, plain, host, inputs = _standin(gfla, "cuda")
    _rewrite(gfla, fused)
    with torch.no_grad():
        want = host(*(t.double() for t in inputs))
        base = plain(*(t.cuda() for t in inputs))
        got = fused(*(t.cuda() for t in inputs))
    scale = want.abs().max()
    measured = ((base.cpu().double() - want).abs().max() / scale).item()
    own = ((got.cpu().double() - want).abs().max() / scale).item()
    print("stand-in generator: unrewritten float32 network %.3e from float64, bar %.3e, rewritten network %.3e"
          % (measured, 4 * measured, own))
    assert got.dtype == torch.float32 and 0 < measured < 1e-4
    assert ((got - base).abs().max() / base.abs().max()).item() <= 4 * measured
