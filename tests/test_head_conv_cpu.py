"""Narrow 3x3 heads without a GPU: argument validation, the torch route against hand-written nn.Sequential heads in
float64, fuse_output_heads on an `Output`-shaped module, install(fuse_heads=True) on the unmodified reference, the goldens,
and the C entry points' argument checks."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import head_conv_util as hu  # noqa: E402

HAVE_REF = os.path.isdir("/root/reference/model/networks")


def test_argument_validation(gfla):
    x = torch.randn(1, 4, 5, 6)
    w = torch.randn(3, 4, 3, 3)
    calls = [
        dict(x=torch.randn(1, 4, 1, 6), weight=w, padding="reflect"),             # reflect with H = 1
        dict(x=torch.randn(1, 4, 6, 1), weight=w, padding="reflect"),
        dict(x=x, weight=torch.randn(3, 5, 3, 3)),                                # Cin does not match
        dict(x=x, weight=torch.randn(3, 4, 1, 1)),                                # not 3 x 3
        dict(x=x, weight=torch.randn(3, 4, 3)),
        dict(x=x, weight=w, post=("tanh", None)),                                 # per-channel post of the wrong length
        dict(x=x, weight=w, post="relu"),
        dict(x=x, weight=w, split=0),
        dict(x=x, weight=w, split=3),
        dict(x=x, weight=w, bias=torch.zeros(2)),
        dict(x=x, weight=w, padding="replicate"),
        dict(x=x, weight=w, pre_slope=-0.5),
        dict(x=x[0], weight=w),
        dict(x=x, weight=w, impl="triton"),
    ]
    for kw in calls:
        with pytest.raises(ValueError):
            gfla.head_conv3x3(**kw)
    # the kernels take at most 8 output channels: the Function refuses more before it looks at anything else
    with pytest.raises(ValueError):
        gfla.HeadConv3x3Function.apply(x, torch.randn(9, 4, 3, 3), None, "zeros", None, None, None)
    with pytest.raises(NotImplementedError):      # and CPU tensors, as every op of the library
        gfla.HeadConv3x3Function.apply(x, w, None, "zeros", None, None, None)
    for bad in (dict(padding="same"), dict(post=("tanh",)), dict(split=5), dict(impl="x"), dict(pre_slope=-1.0)):
        with pytest.raises(ValueError):
            gfla.HeadConv3x3(4, 3, **bad)


def test_c_entry_points_check_their_arguments(gfla):
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n = None
    tail = (0, 0, 0.0, 0, 0, n)
    assert L.gfla_head_conv3x3_fwd_f32(n, p, p, p, n, 1, 1, 1, 1, 2, 2, *tail) == -1
    assert L.gfla_head_conv3x3_fwd_f32(p, p, p, p, n, 1, 1, 2, 1, 2, 2, *tail) == -1        # C0 < Cout without y1
    assert L.gfla_head_conv3x3_fwd_f32(p, p, p, p, n, 1, 1, 9, 9, 2, 2, *tail) == -2        # Cout > 8
    assert L.gfla_head_conv3x3_fwd_f16(p, p, p, p, n, 1, 1, 1, 1, 1, 2, 1, 0, 0.0, 0, 0, n) == -2   # reflect, H = 1
    assert L.gfla_head_conv3x3_fwd_bf16(p, p, p, p, n, 1, 1, 2, 2, 2, 2, 0, 0, 0.0, 1, 1, n) == -2  # overlapping masks
    assert L.gfla_head_conv3x3_fwd_f32(p, p, p, p, n, 1, 1, 2, 2, 2, 2, 0, 0, 0.0, 4, 0, n) == -2   # mask bit beyond Cout
    assert L.gfla_head_conv3x3_fwd_f32(p, p, p, p, n, 1, 1, 1, 1, 2, 2, 2, 0, 0.0, 0, 0, n) == -2   # pad_mode
    assert L.gfla_head_conv3x3_fwd_f32(p, p, p, p, n, 1, 1, 1, 1, 65536, 65536, *tail) == -3        # H W > 2^31 - 1
    assert L.gfla_head_conv3x3_bwd_f32(p, p, p, n, p, n, p, p, p, n, 1, 1, 1, 1, 2, 2, *tail) == -1  # grad_w, no workspace
    assert L.gfla_head_conv3x3_bwd_f32(p, p, p, n, p, n, n, n, n, n, 0, 1, 1, 1, 2, 2, *tail) == -2
    assert L.gfla_head_conv3x3_workspace_bytes(1, 4, 9, 8, 8, 4) == -2
    assert L.gfla_head_conv3x3_workspace_bytes(1, 4, 3, 8, 8, 8) == -2
    assert L.gfla_head_conv3x3_workspace_bytes(3, 16, 8, 16, 11, 4) == 3 * 4 * (8 * 9 * 16 + 8) * 4   # 12 slabs of 4 rows
    # the launch plans fit the hardware and cover the plane, over a sweep of shapes
    for B in (1, 3, 32):
        for (H, W) in ((1, 1), (2, 2), (9, 13), (70, 45), (64, 44), (32, 22), (256, 176), (5, 1000)):
            for cout in (1, 3, 6, 8):
                for bwd in (False, True):
                    g = hu.geometry(B, 20, cout, H, W, bwd)
                    px, py = ((4 if cout <= 4 else 2), 1) if bwd else (4, 2)
                    assert g["threads"] in (64, 128, 256) and g["tile_w"] in (8, 16, 32, 64)
                    assert g["tile_w"] // px * (g["tile_h"] // py) == g["threads"]
                    assert g["tiles_per_plane"] == -(-W // g["tile_w"]) * -(-H // g["tile_h"])
                    assert -(-(g["tile_h"] + 2) * (g["tile_w"] + 2) // g["threads"]) <= 11       # staged elements per thread
                    lds = (4 * (g["tile_h"] + 2) * (g["tile_w"] + 4) if not bwd else cout * (g["tile_h"] + 2) * (g["tile_w"] + 2)) * 4
                    assert lds <= 64 * 1024
                    assert g["slab_rows"] % 4 == 0 and g["slabs"] == B * -(-H // g["slab_rows"]) and g["slabs"] <= 2048


def _grads(ys, ups, params):
    loss = sum((y * u).sum() for y, u in zip(ys, ups))
    return torch.autograd.grad(loss, params)


def test_torch_route_equals_hand_written_heads(gfla):
    torch.manual_seed(3)
    # the Output pattern
    x = torch.randn(2, 5, 6, 7, dtype=torch.float64, requires_grad=True)
    conv = nn.Conv2d(5, 3, 3, padding=0).double()
    seq = nn.Sequential(nn.LeakyReLU(0.1), nn.ReflectionPad2d(1), conv, nn.Tanh())
    up = torch.randn(2, 3, 6, 7, dtype=torch.float64)
    params = (x, conv.weight, conv.bias)
    want_y = seq(x)
    want = _grads((want_y,), (up,), params)
    y = gfla.head_conv3x3(x, conv.weight, conv.bias, "reflect", 0.1, "tanh", impl="torch")
    assert torch.equal(y, gfla.torch_head_conv3x3(x, conv.weight, conv.bias, "reflect", 0.1, "tanh"))
    assert torch.equal(y, gfla.head_conv3x3(x, conv.weight, conv.bias, "reflect", 0.1, "tanh"))    # CPU: auto routes there
    assert (y - want_y).abs().max().item() <= 1e-14
    for a, b in zip(_grads((y,), (up,), params), want):
        assert (a - b).abs().max().item() <= 1e-13
    # a flow + mask pair
    flow = nn.Conv2d(5, 4, 3, 1, 1).double()
    mask = nn.Sequential(nn.Conv2d(5, 2, 3, 1, 1), nn.Sigmoid()).double()
    ups = (torch.randn(2, 4, 6, 7, dtype=torch.float64), torch.randn(2, 2, 6, 7, dtype=torch.float64))
    params = (x, flow.weight, flow.bias, mask[0].weight, mask[0].bias)
    want_ys = (flow(x), mask(x))
    want = _grads(want_ys, ups, params)
    ys = gfla.flow_mask_heads(x, flow, mask, impl="torch")
    assert ys[0].is_contiguous() and ys[1].is_contiguous() and ys[0].shape == (2, 4, 6, 7) and ys[1].shape == (2, 2, 6, 7)
    for a, b in zip(ys, want_ys):
        assert (a - b).abs().max().item() <= 1e-14
    for a, b in zip(_grads(ys, ups, params), want):
        assert (a - b).abs().max().item() <= 1e-13
    # ReLU is slope 0, and a module carries nn.Conv2d's names
    m = gfla.HeadConv3x3(5, 3, pre_slope=0.0, post=("tanh", None, "sigmoid"), impl="torch").double()
    assert list(m.state_dict().keys()) == ["weight", "bias"] and m.weight.shape == (3, 5, 3, 3)
    s = nn.functional.conv2d(torch.relu(x), m.weight, m.bias, padding=1)
    want_y = torch.stack((torch.tanh(s[:, 0]), s[:, 1], torch.sigmoid(s[:, 2])), 1)
    assert (m(x) - want_y).abs().max().item() <= 1e-14
    # a mask head of another form is simply called
    odd = nn.Sequential(nn.Conv2d(5, 2, 3, 1, 1), nn.Tanh()).double()
    f2, m2 = gfla.flow_mask_heads(x, flow, odd)
    assert torch.equal(f2, flow(x)) and torch.equal(m2, odd(x))


class _Output(nn.Module):
    """the shape of the reference's Output (base_function.py:650-670): the convolution is registered twice"""

    def __init__(self, cin, cout, nonlinearity):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, kernel_size=3, padding=0, bias=True)
        self.model = nn.Sequential(nonlinearity, nn.ReflectionPad2d(1), self.conv1, nn.Tanh())

    def forward(self, x):
        return self.model(x)


def test_fuse_output_heads(gfla):
    torch.manual_seed(4)
    shared = nn.LeakyReLU(0.1)
    net = nn.ModuleDict({
        "out": _Output(6, 3, shared),
        "other": nn.Sequential(nn.Conv2d(6, 6, 3, 1, 1), shared),                       # 6 channels, zero padding: a head too
        "mask": nn.Sequential(nn.Conv2d(6, 1, 3, 1, 1), nn.Sigmoid()),
        "wide": nn.Sequential(shared, nn.ReflectionPad2d(1), nn.Conv2d(6, 32, 3)),      # `Jump`: not narrow
        "strided": nn.Sequential(nn.Conv2d(6, 2, 3, 2, 1)),
        "padded0": nn.Sequential(nn.Conv2d(6, 2, 3, 1, 0)),                             # no padding at all: another map
        "spect": nn.Sequential(nn.utils.spectral_norm(nn.Conv2d(6, 2, 3, 1, 1))),
        "hooked": nn.Sequential(nn.Conv2d(6, 2, 3, 1, 1)),
    })
    seen = []
    net["hooked"][0].register_forward_hook(lambda m, i, o: seen.append(1))
    keys = list(net.state_dict().keys())
    params = {n: p for n, p in net.named_parameters()}
    x = torch.randn(2, 6, 5, 7)
    net.eval()
    want = {k: net[k](x) for k in ("out", "other", "mask", "wide")}
    assert gfla.fuse_output_heads(net, impl="torch") == 3
    assert list(net.state_dict().keys()) == keys                                        # conv1.* and model.2.* both survive
    assert all(params[n] is p for n, p in net.named_parameters()) and len(params) == len(dict(net.named_parameters()))
    model = net["out"].model
    assert type(model[2]) is gfla.HeadConv3x3 and model[2].weight is net["out"].conv1.weight
    assert (model[2].padding, model[2].pre_slope, model[2].post) == ("reflect", 0.1, ("tanh",) * 3)
    assert all(type(model[i]) is nn.Identity for i in (0, 1, 3))
    assert type(net["out"].conv1) is nn.Conv2d                                          # the second registration stays
    assert type(shared) is nn.LeakyReLU and net["other"][1] is shared and net["wide"][0] is shared   # untouched object
    assert type(net["other"][0]) is gfla.HeadConv3x3 and net["other"][0].pre_slope is None and net["other"][0].post == (None,) * 6
    assert type(net["mask"][0]) is gfla.HeadConv3x3 and net["mask"][0].post == ("sigmoid",) and type(net["mask"][1]) is nn.Identity
    assert type(net["wide"][2]) is nn.Conv2d and type(net["strided"][0]) is nn.Conv2d and type(net["padded0"][0]) is nn.Conv2d
    assert type(net["spect"][0]) is nn.Conv2d
    net["hooked"](x)
    assert type(net["hooked"][0]) is nn.Conv2d and seen == [1]                          # a hook keeps firing: left alone
    for k, v in want.items():
        assert (net[k](x) - v).abs().max().item() <= 1e-6, k
    assert gfla.fuse_output_heads(net, impl="torch") == 0                               # again: nothing more
    relu = nn.Sequential(nn.ReLU(), nn.Conv2d(6, 2, 3, 1, 1))                           # an nn.ReLU is folded in as slope 0
    want_relu = relu(x)
    assert gfla.fuse_output_heads(relu, impl="torch") == 1 and type(relu[0]) is nn.Identity and relu[1].pre_slope == 0.0
    assert torch.equal(relu(x), want_relu)
    # a fused mask head still pairs with its flow convolution
    flow = nn.Conv2d(6, 2, 3, 1, 1)
    f, m = gfla.flow_mask_heads(x, flow, net["mask"], impl="torch")
    assert (f - flow(x)).abs().max().item() <= 1e-6 and (m - want["mask"]).abs().max().item() <= 1e-6


_REF_CODE = r"""
import sys, types
sys.path.insert(0, %r)
import torch
from torch import nn
import global_flow_local_attention_amd as g
sys.modules.setdefault('torchvision', types.ModuleType('torchvision'))
bf = g.install('/root/reference')
import model.networks.generator as gen
plain_attn = {n: getattr(gen, n).attn_output for n in ('PoseFlowNet', 'FaceFlowNet', 'ShapeNetFlowNet')}
plain_init = bf.Output.__init__


def build():
    torch.manual_seed(1)
    pose = gen.PoseGenerator(image_nc=3, structure_nc=6, ngf=8, img_f=32, layers=3, num_blocks=2, use_spect=False,
                             attn_layer=[2, 3], norm='instance', activation='LeakyReLU', extractor_kz={'2': 5, '3': 3})
    face = gen.FaceGenerator(image_nc=3, structure_nc=4, ngf=8, img_f=32, layers=3, num_blocks=2, norm='instance',
                             activation='LeakyReLU', attn_layer=[2, 3], extractor_kz={'2': 5, '3': 3}, use_spect=False)
    return pose.eval(), face.eval()


pose0, face0 = build()
assert g.install('/root/reference') is bf and bf.Output.__init__ is plain_init            # the default changes nothing
assert all(getattr(gen, n).attn_output is f for n, f in plain_attn.items())
g.install('/root/reference', fuse_heads='torch')
assert bf.Output.__init__ is not plain_init and all(getattr(gen, n).attn_output is not f for n, f in plain_attn.items())
g.install('/root/reference', fuse_heads='torch')                                          # idempotent
pose1, face1 = build()
for a, b in ((pose0, pose1), (face0, face1)):
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    b.load_state_dict(a.state_dict())
    assert type(b.target.outconv.model[2]) is g.HeadConv3x3 and type(a.target.outconv.model[2]) is nn.Conv2d
    assert b.target.outconv.model[2].weight is b.target.outconv.conv1.weight
torch.manual_seed(2)
B, H, W = 2, 64, 64
with torch.no_grad():
    src, sb, tb = torch.randn(B, 3, H, W), torch.randn(B, 6, H, W), torch.randn(B, 6, H, W)
    want, got = pose0.flow_net(src, sb, tb), pose1.flow_net(src, sb, tb)
    n = 0
    for ws, gs in zip(want, got):
        for w_, g_ in zip(ws, gs):
            assert w_.shape == g_.shape and g_.is_contiguous() and (w_ - g_).abs().max().item() <= 1e-6
            n += 1
    assert n == 4
    bp = torch.randn(B, 4, H, W)
    args = (bp, torch.randn(B, 3, H, W), torch.randn(B, 4, H, W), torch.randn(B, 3, H, W), torch.randn(B, 4, H, W))
    want, got = face0.flow_net(*args), face1.flow_net(*args)
    n = 0
    for ws, gs in zip(want, got):
        for w_, g_ in zip(ws, gs):
            assert w_.shape == g_.shape and (w_ - g_).abs().max().item() <= 1e-6
            n += 1
    assert n == 8
    feat = torch.randn(B, 8, H, W)
    for a, b in ((pose0, pose1), (face0, face1)):
        assert (a.target.outconv(feat) - b.target.outconv(feat)).abs().max().item() <= 1e-6
print('ok')
"""


@pytest.mark.skipif(not HAVE_REF, reason="reference checkout not present")
def test_install_fuses_the_heads_of_the_unmodified_reference(gfla):
    out = subprocess.run([sys.executable, "-c", _REF_CODE % ROOT], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-3000:]


@pytest.mark.parametrize("name", sorted(hu.GOLDENS))
def test_goldens(gfla, name):
    """what the reference's own classes computed in float64 (tests/golden/make_head_conv_golden.py), reproduced by the
    torch route to 1e-12"""
    shape, cout, post, split, padding, slope = hu.GOLDENS[name]
    g = hu.golden(name)
    assert g["x"].dtype == torch.float64 and tuple(g["x"].shape) == shape and tuple(g["weight"].shape) == (cout, shape[1], 3, 3)
    x, w, b = (g[k].clone().requires_grad_() for k in ("x", "weight", "bias"))
    ys = gfla.head_conv3x3(x, w, b, padding, slope, post, split, impl="torch")
    ys = (ys,) if split is None else ys
    ups = (g["up"],) if split is None else (g["up"][:, :split], g["up"][:, split:])
    got = _grads(ys, ups, (x, w, b))
    for j, y in enumerate(ys):
        assert (y - g["y%d" % j]).abs().max().item() <= 1e-12
    for a, k in zip(got, ("g_x", "g_weight", "g_bias")):
        assert (a - g[k]).abs().max().item() <= 1e-12, k
