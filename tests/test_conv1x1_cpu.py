"""gen_conv.conv1x1 without a GPU: the validation in front of every launch, the torch composition that CPU tensors take
(bit-identical, values and gradients), the two rewrites that put 1x1 convolutions on it -- fuse_spectral_norm with
pointwise="kernels", which also folds the AvgPool2d(2) in front of a shortcut, and fuse_inference_convs with
pointwise=True --, install()'s argument check, and the host-side status codes of the C entry points."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils import spectral_norm as sn

import conv1x1_util as cu
import discriminator_util as du


def test_validation_before_anything_is_launched(gfla):
    x, w, b = torch.zeros(1, 4, 6, 6), torch.zeros(5, 4, 1, 1), torch.zeros(5)
    for bad_w in (torch.zeros(5, 4, 3, 3), torch.zeros(5, 3, 1, 1), torch.zeros(5, 4, 1), torch.zeros(0, 4, 1, 1)):
        with pytest.raises(ValueError, match="weight"):
            gfla.conv1x1(x, bad_w)
    with pytest.raises(ValueError, match="bias"):
        gfla.conv1x1(x, w, torch.zeros(4))
    for pool in (0, 3, None, "2"):
        with pytest.raises(ValueError, match="pool"):
            gfla.conv1x1(x, w, b, pool=pool)
    with pytest.raises(ValueError, match="pre-activation"):
        gfla.conv1x1(x, w, b, pre_slope=0.1, pool=2)
    with pytest.raises(ValueError, match="H, W >= 2"):
        gfla.conv1x1(torch.zeros(1, 4, 1, 6), w, b, pool=2)
    with pytest.raises(ValueError, match="H, W >= 2"):
        gfla.conv1x1(torch.zeros(1, 4, 6, 1), w, b, pool=2)
    with pytest.raises(ValueError, match="pre_slope"):
        gfla.conv1x1(x, w, b, pre_slope=-0.5)
    with pytest.raises(ValueError, match="grad"):
        gfla.conv1x1(x, w, b, grad="hip")
    with pytest.raises(ValueError, match="impl"):
        gfla.conv1x1(x, w, b, impl="hip")
    with pytest.raises(ValueError, match="map"):
        gfla.conv1x1(torch.zeros(4, 6, 6), w, b)
    assert gfla.conv1x1(torch.zeros(1, 4, 1, 6), w, b).shape == (1, 5, 1, 6)        # pool 1 takes a single row


@pytest.mark.parametrize("grad", ["torch", "kernels"])
@pytest.mark.parametrize("shape,opts", cu.ROWS[1:], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else
                         "-".join("%s%s" % kv for kv in sorted(v.items())))
def test_cpu_is_the_torch_composition(gfla, shape, opts, grad):
    """values and all gradients, bit for bit; grad="kernels" changes nothing on the CPU"""
    pool, slope = opts.get("pool", 1), opts.get("slope")
    (x, w, b), g = cu.leaves("f32", shape, cu.key(opts), "cpu")
    (x2, w2, b2), _ = cu.leaves("f32", shape, cu.key(opts), "cpu")
    y = gfla.conv1x1(x, w, b, pre_slope=slope, pool=pool, grad=grad)
    a = F.avg_pool2d(x2, 2, 2) if pool == 2 else F.leaky_relu(x2, slope)
    want = F.conv2d(a, w2, b2)
    assert y.shape == (shape[0], shape[2], shape[3] // pool, shape[4] // pool) and torch.equal(y, want)
    y.backward(g)
    want.backward(g)
    assert torch.equal(x.grad, x2.grad) and torch.equal(w.grad, w2.grad)
    assert b is None or torch.equal(b.grad, b2.grad)
    assert torch.equal(gfla.torch_conv1x1(x, w, b, slope, pool), want)
    x64, w64 = x.detach().double(), w.detach().double()                               # float64 takes it as well
    assert gfla.conv1x1(x64, w64, pre_slope=slope, pool=pool).dtype == torch.float64


def _cpu_discriminators():
    (fused, plain), _, images = du.discriminators("cpu")
    return fused, plain, images


def test_fuse_spectral_norm_defaults_are_todays(gfla):
    fused, plain, images = _cpu_discriminators()
    keys = list(fused.state_dict().keys())
    assert gfla.fuse_spectral_norm(fused) == 10
    for block in fused.blocks:
        assert type(block.shortcut[0]) is nn.AvgPool2d and type(block.shortcut[1]) is gfla.SpectralConv
        assert block.shortcut[1].pool == 1 and not block.shortcut[1].pointwise
    assert not fused.conv.pointwise and list(fused.state_dict().keys()) == keys
    assert torch.equal(fused(images[0]), plain(images[0]))


def test_fuse_spectral_norm_pointwise_folds_the_pool(gfla):
    fused, plain, images = _cpu_discriminators()
    keys = list(plain.state_dict().keys())
    assert gfla.fuse_spectral_norm(fused, pointwise="kernels") == 10 and not du.hooked_convs(fused)
    for block in fused.blocks:
        assert type(block.shortcut[0]) is nn.Identity and type(block.shortcut[1]) is gfla.SpectralConv
        assert block.shortcut[1].pool == 2 and block.shortcut[1].pointwise and block.shortcut[1].pre_slope is None
        assert "pool=2" in repr(block.shortcut[1])
    assert fused.conv.pointwise and fused.conv.pool == 1
    assert list(fused.state_dict().keys()) == keys                                   # keys and their order
    state = copy.deepcopy(plain.state_dict())
    fused.load_state_dict(state, strict=True)
    plain.load_state_dict(copy.deepcopy(fused.state_dict()), strict=True)
    # the rewritten network on the CPU is the unrewritten one, bit for bit: two training-mode forwards (u, v move), one eval
    for image in images:
        assert torch.equal(fused(image), plain(image))
    assert all(torch.equal(a, b) for a, b in zip(fused.state_dict().values(), plain.state_dict().values()))
    assert torch.equal(fused.eval()(images[0]), plain.eval()(images[0]))
    with pytest.raises(ValueError, match="pointwise"):
        gfla.fuse_spectral_norm(_cpu_discriminators()[0], pointwise="hip")


@pytest.mark.parametrize("pool", [nn.AvgPool2d(3, 2), nn.AvgPool2d(2, 2, ceil_mode=True), nn.AvgPool2d(2, 1),
                                  nn.AvgPool2d(2, 2, padding=1), nn.AvgPool2d(2, 2, divisor_override=3), nn.MaxPool2d(2, 2)],
                         ids=["kernel3", "ceil", "stride1", "padding", "divisor", "max"])
def test_a_pool_of_another_geometry_is_not_folded(gfla, pool):
    torch.manual_seed(3)
    net = nn.Sequential(pool, sn(nn.Conv2d(4, 6, 1)))
    ref = copy.deepcopy(net)
    assert gfla.fuse_spectral_norm(net, pointwise="kernels") == 1
    assert net[0] is pool and net[1].pool == 1 and net[1].pointwise
    x = torch.randn(2, 4, 9, 7)
    assert torch.equal(net(x), ref(x))


def test_spectral_conv_arguments(gfla):
    conv1, conv3 = sn(nn.Conv2d(4, 6, 1)), sn(nn.Conv2d(4, 6, 3, 1, 1))
    with pytest.raises(ValueError, match="pointwise"):
        gfla.SpectralConv(conv1, pointwise="hip")
    with pytest.raises(ValueError, match="pool"):
        gfla.SpectralConv(conv1, pool=2)                              # the default route has no pool
    with pytest.raises(ValueError, match="pool"):
        gfla.SpectralConv(conv3, pointwise="kernels", pool=2)         # no 1x1 convolution
    with pytest.raises(ValueError, match="pool"):
        gfla.SpectralConv(conv1, pre_slope=0.1, pointwise="kernels", pool=2)
    assert not gfla.SpectralConv(conv3, pointwise="kernels").pointwise
    assert not gfla.SpectralConv(sn(nn.Conv2d(4, 6, 1, 2)), pointwise="kernels").pointwise      # stride 2


def test_fuse_inference_convs_pointwise(gfla):
    (a, b, plain), x = cu.widening_blocks("cpu", copies=3)
    keys = list(plain.state_dict().keys())
    assert gfla.fuse_inference_convs(a) == 2 and type(a.shortcut[0]) is nn.Conv2d
    assert gfla.fuse_inference_convs(b, pointwise=True) == 3
    fused = b.shortcut[0]
    assert type(fused) is gfla.InferenceConv and fused.geometry == 3 and fused.pre_slope is None
    assert fused.weight is fused.original.weight and "conv1x1" in repr(fused)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys()) == keys
    assert torch.equal(a(x), plain(x)) and torch.equal(b(x), plain(x))
    with torch.no_grad():
        assert torch.equal(b(x), plain(x))
    # a LeakyReLU in front of a 1x1 convolution is folded like any other; inside an ExtractorAttn nothing is touched
    seq = nn.Sequential(nn.LeakyReLU(0.2), nn.Conv2d(12, 20, 1))
    ref = copy.deepcopy(seq)
    assert gfla.fuse_inference_convs(seq, pointwise=True) == 1 and type(seq[0]) is nn.Identity and seq[1].pre_slope == 0.2
    assert torch.equal(seq(x), ref(x))
    attn = gfla.ExtractorAttn(16, 3, nn.LeakyReLU(0.1), softmax=True)
    assert gfla.fuse_inference_convs(attn, pointwise=True) == 0
    with pytest.raises(ValueError, match="geometry"):
        gfla.InferenceConv(nn.Conv2d(4, 4, 1), 3, padding="reflect")


def test_install_pointwise_convs_needs_a_rewrite(gfla):
    with pytest.raises(ValueError, match="pointwise_convs"):
        gfla.install(pointwise_convs=True)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.isdir("/root/reference/model/networks"), reason="reference checkout not present")
def test_install_puts_the_reference_1x1_convolutions_on_the_op(gfla):
    """install(pointwise_convs=True) in a process of its own: every shortcut of a reference ResDiscriminator loses its
    pool to the convolution behind it, the final convolution takes the route, no nn.Conv2d and no nn.AvgPool2d is left,
    state-dict keys stay, and on the CPU a block is still the reference's own forward; a generator ResBlock with a
    learnable shortcut gets it as an InferenceConv"""
    import subprocess
    import sys
    code = r"""
import sys, types
sys.path.insert(0, %r)
import torch
from torch import nn
import global_flow_local_attention_amd as g
sys.modules.setdefault('torchvision', types.ModuleType('torchvision'))
bf = g.install('/root/reference', inference_convs=True, discriminator_convs=True, train_convs=True, pointwise_convs=True)
import model.networks.discriminator as d
torch.manual_seed(0)
net = d.ResDiscriminator(ndf=8, img_f=32, layers=3)
convs = [m for m in net.modules() if type(m) is g.SpectralConv]
assert len(convs) == 10 and all(c.grad == 'kernels' for c in convs)
assert not any(type(m) in (nn.Conv2d, nn.AvgPool2d) for m in net.modules())
assert [c.pool for c in convs if c.pointwise] == [2, 2, 2, 1] and net.conv.pointwise
for block in (net.block0, net.encoder0, net.encoder1):
    assert type(block.shortcut[0]) is nn.Identity and block.shortcut[1].pool == 2
assert 'block0.shortcut.1.weight_orig' in net.state_dict() and 'conv.weight_u' in net.state_dict()
plain = bf.ResBlockEncoder.forward.__wrapped__
x = torch.randn(1, 3, 33, 31)
net.eval()
with torch.no_grad():
    want = net.block0.model(x) + torch.nn.functional.conv2d(torch.nn.functional.avg_pool2d(x, 2, 2),
        net.block0.shortcut[1].weight_orig / torch.dot(net.block0.shortcut[1].weight_u, torch.mv(
            net.block0.shortcut[1].weight_orig.flatten(1), net.block0.shortcut[1].weight_v)), net.block0.shortcut[1].bias)
    assert torch.equal(net.block0(x), want) and torch.equal(plain(net.block0, x), want)
net.train()
net(x).sum().backward()
assert all(p.grad is not None for p in net.parameters())
res = bf.ResBlock(12, 20, 16, nn.InstanceNorm2d, nn.LeakyReLU(0.1))
assert res.learnable_shortcut and type(res.shortcut[0]) is g.InferenceConv and res.shortcut[0].geometry == 3
assert res.shortcut[0].grad == 'kernels' and res(torch.randn(1, 12, 9, 7)).shape == (1, 20, 9, 7)
print('ok')
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_entry_points_and_status_codes(gfla):
    import ctypes
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    names = {"gfla_conv1x1_%s_%s" % (what, sfx) for sfx in ("f32", "f16", "bf16")
             for what in ("pack_weights", "pack_grad_weights", "fwd", "bwd_data", "bwd_weight")}
    names |= {"gfla_conv1x1_packed_bytes", "gfla_conv1x1_grad_packed_bytes", "gfla_conv1x1_bwd_workspace_bytes"}
    assert names <= set(_lib.extension_symbols()) and _lib.ABI_VERSION == 8
    # [chunk][Cout padded to 32][32 bytes]; the gradient's packing is the transposed matrix
    assert L.gfla_conv1x1_packed_bytes(40, 20, 4) == 3 * 64 * 32 and L.gfla_conv1x1_packed_bytes(40, 20, 2) == 2 * 64 * 32
    assert L.gfla_conv1x1_grad_packed_bytes(40, 20, 4) == 5 * 32 * 32 and L.gfla_conv1x1_grad_packed_bytes(1, 33, 2) == 64 * 32
    assert L.gfla_conv1x1_packed_bytes(0, 20, 4) == -2 and L.gfla_conv1x1_packed_bytes(40, 20, 3) == -2
    assert L.gfla_conv1x1_packed_bytes(65537, 20, 4) == -3 and L.gfla_conv1x1_grad_packed_bytes(4, 65537, 2) == -3
    ws = L.gfla_conv1x1_bwd_workspace_bytes
    assert ws(2, 20, 40, 21, 19, 2, 4) >= 40 * 20 * 4 + 16 and ws(2, 20, 40, 21, 19, 1, 2) > ws(2, 20, 40, 21, 19, 2, 2)
    assert ws(2, 20, 40, 1, 19, 2, 4) == -2 and ws(2, 20, 40, 21, 19, 3, 4) == -2 and ws(2, 20, 40, 21, 19, 2, 8) == -2
    assert ws(65536, 20, 40, 4, 4, 1, 4) == -3 and ws(1, 20, 40, 1 << 16, 1 << 15, 1, 4) == -3       # B; 2^31 pixels
    assert ws(4, 20, 40, 1 << 15, 1 << 15, 1, 4) == -3                                              # B x pixels
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n = None
    assert L.gfla_conv1x1_fwd_f32(n, p, p, p, 1, 4, 4, 4, 4, 1, 0, 0.0, n) == -1
    assert L.gfla_conv1x1_fwd_f32(p, p, n, p, 1, 4, 4, 4, 4, 3, 0, 0.0, n) == -2                    # pool
    assert L.gfla_conv1x1_fwd_bf16(p, p, n, p, 1, 4, 4, 4, 4, 2, 1, 0.1, n) == -2                   # pool 2 with pre_act
    assert L.gfla_conv1x1_fwd_f16(p, p, n, p, 1, 4, 4, 1, 4, 2, 0, 0.0, n) == -2                    # pool 2 on H = 1
    assert L.gfla_conv1x1_fwd_f32(p, p, n, p, 1, 65537, 4, 4, 4, 1, 0, 0.0, n) == -3
    assert L.gfla_conv1x1_bwd_data_f32(p, n, p, p, 1, 4, 4, 4, 4, 1, 1, 0.1, n) == -1               # pre_act needs x
    assert L.gfla_conv1x1_bwd_data_f32(p, n, p, p, 70000, 4, 4, 4, 4, 2, 0, 0.0, n) == -3
    assert L.gfla_conv1x1_bwd_weight_f32(p, p, n, n, p, 1, 4, 4, 4, 4, 1, 0, 0.0, n) == -1          # nothing asked for
    assert L.gfla_conv1x1_bwd_weight_f32(p, p, p, n, n, 1, 4, 4, 4, 4, 1, 0, 0.0, n) == -1          # grad_w without workspace
    assert L.gfla_conv1x1_bwd_weight_f32(p, p, p, p, p, 1, 4, 4, 4, 4, 0, 0, 0.0, n) == -2
    assert L.gfla_conv1x1_pack_weights_f32(n, 0, p, 4, 4, n) == -1 and L.gfla_conv1x1_pack_weights_f32(p, 3, p, 4, 4, n) == -2
    # the existing entry points keep refusing anything but geometries 0 .. 2
    assert L.gfla_gen_conv_packed_bytes(8, 8, 3, 4) == -2 and L.gfla_gen_conv_bwd_workspace_bytes(1, 8, 8, 4, 4, 3, 0, 4) == -2
