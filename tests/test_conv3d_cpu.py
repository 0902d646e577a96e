"""The frames-major 3-D convolutions without a GPU (conv3d.py, spectral_norm.SpectralConv3d; include/gfla_conv3d.h): the
binding and every refusal of the entry points by its status code, the torch compositions against F.conv3d / F.avg_pool3d
bit for bit, the window rule emulated on the host against F.conv3d and its data gradient in float64, the rewrite of a
network (state dict, identity of Parameters and buffers, idempotence, what is left alone, the untouched default, bit
equality with the hooked network over two training steps) and install()."""
import copy
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import conv3d_util as c3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SFX = ("f32", "f16", "bf16")


def test_binding(gfla):
    from global_flow_local_attention_amd import _lib
    names = {"gfla_%s_%s" % (what, sfx) for sfx in SFX
             for what in ("conv3d_fwd", "conv3d_bwd_data", "conv3d_bwd_weight", "avg_pool_frames_fwd", "avg_pool_frames_bwd")}
    names |= {"gfla_conv3d_bwd_workspace_bytes", "gfla_conv3d_out_size"}
    assert names <= set(_lib.extension_symbols()) and not names & set(_lib.exported_symbols())
    assert len(_lib.exported_symbols()) == 154 and _lib.ABI_VERSION == 8 and _lib.PATH_COUNT == 22
    assert any(p.endswith("gfla_conv3d.h") for p in _lib.EXTENSION_HEADER_PATHS)
    handle = _lib.lib()
    assert handle.gfla_conv3d_bwd_workspace_bytes.restype is ctypes.c_int64
    for name in ("to_frames_major", "from_frames_major", "conv3d_frames", "avg_pool_frames", "Conv3dFramesFunction",
                 "AvgPoolFramesFunction", "torch_conv3d_frames", "torch_avg_pool_frames", "SpectralConv3d"):
        assert hasattr(gfla, name), name


def test_out_size_and_workspace_queries(gfla):
    from global_flow_local_attention_amd import _lib, conv3d
    L = _lib.lib()
    assert conv3d.out_size("k333", 4, 17, 9) == (4, 17, 9) and conv3d.out_size("k344", 6, 33, 17) == (4, 16, 8)
    assert conv3d.out_size("k344", 3, 2, 2) == (1, 1, 1)
    lo, ho, wo = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    ptrs = [ctypes.addressof(v) for v in (lo, ho, wo)]
    assert L.gfla_conv3d_out_size(0, 4, 5, 5, None, ptrs[1], ptrs[2]) == -1
    for bad in ((2, 4, 5, 5), (-1, 4, 5, 5), (0, 0, 5, 5), (0, 4, 0, 5), (1, 2, 5, 5), (1, 3, 1, 5), (1, 3, 5, 1)):
        assert L.gfla_conv3d_out_size(*bad, *ptrs) == -2, bad
    with pytest.raises(ValueError):
        conv3d.out_size("k344", 2, 8, 8)
    # the float32 partial sums of grad_w (Cout, 3 C, k, k), at least one split, 16 bytes to spare
    n = L.gfla_conv3d_bwd_workspace_bytes(2, 4, 20, 40, 17, 9, 0, 4)
    assert n >= 40 * 60 * 9 * 4 + 16 and (n - 16) % (40 * 60 * 9 * 4) == 0
    assert L.gfla_conv3d_bwd_workspace_bytes(2, 4, 20, 40, 17, 9, 0, 3) == -2
    assert L.gfla_conv3d_bwd_workspace_bytes(2, 2, 20, 40, 17, 9, 1, 4) == -2            # k344 with L < 3
    assert L.gfla_conv3d_bwd_workspace_bytes(1, 3, 20, 40, 1 << 16, 1 << 16, 0, 4) == _lib._ERR_UNSUPPORTED


def test_every_refusal_by_its_status_code(gfla):
    """nothing is launched on a refusal, so none of these needs a GPU: the pointers are host buffers nobody reads"""
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    U = _lib._ERR_UNSUPPORTED
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 1)
    good = (1, 3, 4, 8, 6, 6)                          # B, L, C, Cout, H, W
    for sfx in SFX:
        fwd, bwd_d, bwd_w = (getattr(L, "gfla_conv3d_%s_%s" % (w, sfx)) for w in ("fwd", "bwd_data", "bwd_weight"))
        pf, pb = (getattr(L, "gfla_avg_pool_frames_%s_%s" % (w, sfx)) for w in ("fwd", "bwd"))
        # NULL -> -1
        for args in ((None, p, None, None, p), (p, None, None, None, p), (p, p, None, None, None)):
            assert fwd(*args, *good, 0, 0, 0.0, None) == -1
        for args in ((None, p, p, p), (p, p, None, p), (p, p, p, None), (p, None, p, p)):
            assert bwd_d(*args, *good, 0, 1, 0.1, None) == -1                  # x is read with pre_act only
        for args in ((None, p, p, p, p), (p, p, None, None, p), (p, None, p, None, p), (p, p, p, None, None)):
            assert bwd_w(*args, *good, 0, 0, 0.0, None) == -1
        assert pf(None, p, 1, 3, 4, 6, 6, None) == -1 and pf(p, None, 1, 3, 4, 6, 6, None) == -1
        assert pb(None, p, 1, 3, 4, 6, 6, None) == -1 and pb(p, None, 1, 3, 4, 6, 6, None) == -1
        # non-positive sizes, an unknown geometry, k344 with L < 3 or H, W < 2 -> -2
        bad = [tuple(0 if j == i else v for j, v in enumerate(good)) + (0,) for i in range(6)]
        bad += [good + (2,), good + (-1,), (1, 2, 4, 8, 6, 6, 1), (1, 3, 4, 8, 1, 6, 1), (1, 3, 4, 8, 6, 1, 1)]
        for b in bad:
            assert fwd(p, p, None, None, p, *b, 0, 0.0, None) == -2, b
            assert bwd_d(p, p, p, p, *b, 0, 0.0, None) == -2, b
            assert bwd_w(p, p, p, p, p, *b, 0, 0.0, None) == -2, b
            assert L.gfla_conv3d_bwd_workspace_bytes(*b, 4) == -2, b
        for b in ((0, 3, 4, 6, 6), (1, 0, 4, 6, 6), (1, 3, 0, 6, 6), (1, 3, 4, 0, 6), (1, 3, 4, 6, 0), (1, 2, 4, 6, 6),
                  (1, 3, 4, 1, 6), (1, 3, 4, 6, 1)):
            assert pf(p, p, *b, None) == -2 and pb(p, p, *b, None) == -2, b
        # a plane beyond 2^31 - 1, B L or B Lout beyond 65535, more than 65536 windowed channels -> unsupported
        big = [(1, 3, 4, 8, 1 << 16, 1 << 15, 0), (1, 3, 4, 8, 1 << 16, 1 << 15, 1), (256, 256, 4, 8, 6, 6, 0),
               (256, 258, 4, 8, 6, 6, 1), (1, 65536, 4, 8, 6, 6, 0), (1, 3, 21846, 8, 6, 6, 0), (1, 3, 4, 21846, 6, 6, 1)]
        for b in big:
            assert fwd(p, p, None, None, p, *b, 0, 0.0, None) == U, b
            assert bwd_d(p, p, p, p, *b, 0, 0.0, None) == U, b
            assert bwd_w(p, p, p, p, p, *b, 0, 0.0, None) == U, b
            assert L.gfla_conv3d_bwd_workspace_bytes(*b, 4) == U, b
        for b in ((1, 3, 4, 1 << 16, 1 << 15), (256, 256, 4, 6, 6), (1, 3, 65537, 6, 6)):
            assert pf(p, p, *b, None) == U and pb(p, p, *b, None) == U, b
        # a reduction of the weight gradient beyond 2^31 - 1: B Lout Hout Wout
        deep = (1, 65535, 4, 8, 256, 256, 0)
        assert bwd_w(p, p, p, p, p, *deep, 0, 0.0, None) == U and L.gfla_conv3d_bwd_workspace_bytes(*deep, 4) == U
        # a pointer that is not aligned to its element
        assert fwd(odd, p, None, None, p, *good, 0, 0, 0.0, None) == U and pf(odd, p, 1, 3, 4, 6, 6, None) == U
        assert bwd_d(p, p, p, odd, *good, 0, 0, 0.0, None) == U and pb(p, odd, 1, 3, 4, 6, 6, None) == U


def test_python_argument_checks(gfla):
    x, w = torch.zeros(1, 3, 4, 6, 6), torch.zeros(8, 4, 3, 3, 3)
    for kwargs in ({"geometry": "k345"}, {"grad": "mine"}, {"impl": "fast"}, {"pre_slope": -1.0},
                   {"bias": torch.zeros(7)}, {"add": torch.zeros(1, 3, 8, 6, 5)}, {"geometry": "k344"}):
        with pytest.raises(ValueError):
            gfla.conv3d_frames(x, w, **kwargs)
    with pytest.raises(ValueError):
        gfla.conv3d_frames(x[0], w)
    with pytest.raises(ValueError):
        gfla.conv3d_frames(torch.zeros(1, 2, 4, 6, 6), torch.zeros(8, 4, 3, 4, 4), geometry="k344")
    with pytest.raises(ValueError):
        gfla.avg_pool_frames(torch.zeros(1, 2, 4, 6, 6))
    with pytest.raises(ValueError):
        gfla.to_frames_major(torch.zeros(1, 2, 3, 4))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("geometry,shape", [("k333", (2, 1, 5, 7, 9, 7)), ("k333", (1, 4, 6, 5, 6, 11)),
                                            ("k344", (2, 3, 5, 7, 9, 7)), ("k344", (1, 5, 6, 5, 6, 11))], ids=c3.case_id)
def test_compositions_equal_torch_bit_for_bit(gfla, geometry, shape, dtype):
    B, L, C, Cout, H, W = shape
    k = c3.K[geometry]
    gen = torch.Generator().manual_seed(sum(shape))
    xt = torch.randn(B, C, L, H, W, generator=gen, dtype=dtype)
    w, b = torch.randn(Cout, C, 3, k, k, generator=gen, dtype=dtype), torch.randn(Cout, generator=gen, dtype=dtype)
    xf = gfla.to_frames_major(xt)
    assert xf.shape == (B, L, C, H, W) and xf.is_contiguous() and torch.equal(gfla.from_frames_major(xf), xt)
    want = F.conv3d(F.leaky_relu(xt, 0.1), w, b, stride=c3.STRIDE[geometry], padding=c3.PADDING[geometry])
    add = torch.randn(want.shape, generator=gen, dtype=dtype)
    for fn in (gfla.torch_conv3d_frames, gfla.conv3d_frames):             # on the host the functional form is the composition
        got = fn(xf, w, b, geometry=geometry, pre_slope=0.1, add=gfla.to_frames_major(add))
        assert got.is_contiguous() and torch.equal(gfla.from_frames_major(got), want + add)
    assert torch.equal(gfla.from_frames_major(gfla.torch_conv3d_frames(xf, w, geometry=geometry)),
                       F.conv3d(xt, w, None, stride=c3.STRIDE[geometry], padding=c3.PADDING[geometry]))
    if L >= 3:
        want = F.avg_pool3d(xt, (3, 2, 2), (1, 2, 2))
        for fn in (gfla.torch_avg_pool_frames, gfla.avg_pool_frames):
            assert torch.equal(gfla.from_frames_major(fn(xf)), want)


@pytest.mark.parametrize("geometry,shape", [("k333", (1, 1, 3, 4, 5, 4)), ("k333", (2, 2, 5, 6, 7, 5)),
                                            ("k333", (2, 4, 5, 6, 7, 5)), ("k344", (1, 3, 3, 4, 6, 5)),
                                            ("k344", (2, 6, 5, 6, 9, 8)), ("k344", (1, 4, 2, 3, 2, 2))], ids=c3.case_id)
def test_window_rule_reproduces_conv3d_and_its_data_gradient(geometry, shape):
    """the host twin of what the kernels compute: the sample start, [clo, chi), the permuted weight, and for the gradient
    the reversed temporal taps -- F.conv2d on the windows against F.conv3d, float64"""
    B, L, C, Cout, H, W = shape
    k = c3.K[geometry]
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, L, C, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(Cout, C, 3, k, k, generator=gen, dtype=torch.float64)
    b = torch.randn(Cout, generator=gen, dtype=torch.float64)
    xt = c3.torch_layout(x).clone().requires_grad_()
    want = F.conv3d(xt, w, b, stride=c3.STRIDE[geometry], padding=c3.PADDING[geometry])
    got = c3.window_forward(x, w, b, geometry)
    assert got.shape == c3.torch_layout(want).shape
    assert (got - c3.torch_layout(want)).abs().max() <= 1e-12 * want.abs().max()
    g = torch.randn(got.shape, generator=gen, dtype=torch.float64)
    gx, = torch.autograd.grad(want, xt, c3.torch_layout(g))
    mine = c3.window_grad_x(g, w, geometry, L, H, W)
    assert mine.shape == x.shape and (mine - c3.torch_layout(gx)).abs().max() <= 1e-12 * gx.abs().max()


# ---- the rewrite -----------------------------------------------------------------------------------------------------------
def _net(seed=5):
    torch.manual_seed(seed)
    return c3.TemporalDiscriminator()


def test_rewrite_keeps_the_state_dict_and_the_objects(gfla):
    net = _net()
    before = [(k, id(v)) for k, v in net.state_dict(keep_vars=True).items()]
    params = [(k, id(p)) for k, p in net.named_parameters()]
    assert gfla.fuse_spectral_norm(net, temporal="kernels") == 10 and not c3.hooked_convs(net)
    assert [(k, id(v)) for k, v in net.state_dict(keep_vars=True).items()] == before
    assert [(k, id(p)) for k, p in net.named_parameters()] == params
    for block in (net.block0, net.block1):
        assert [type(m).__name__ for m in block.model] == ["Identity", "SpectralConv3d", "Identity", "SpectralConv3d"]
        assert [type(m).__name__ for m in block.shortcut] == ["AvgPoolFrames", "SpectralConv3d"]
        assert [m.geometry for m in block.modules() if type(m) is gfla.SpectralConv3d] == ["k333", "k344", "k111"]
        assert block.model[1].pre_slope == block.model[3].pre_slope == 0.1 and block.shortcut[1].pre_slope is None
    assert gfla.fuse_spectral_norm(net, temporal="kernels") == 0                         # idempotent
    assert [(k, id(v)) for k, v in net.state_dict(keep_vars=True).items()] == before
    fresh = _net(6)
    fresh.load_state_dict(net.state_dict(), strict=True)                                 # both ways
    net.load_state_dict(_net(7).state_dict(), strict=True)
    clone = copy.deepcopy(net)
    x = torch.randn(c3.VIDEO)
    assert torch.equal(clone.eval()(x), net.eval()(x))
    with pytest.raises(ValueError, match="temporal"):
        gfla.fuse_spectral_norm(_net(), temporal="yes")


def test_the_default_leaves_the_3d_blocks_alone(gfla):
    net = _net()
    assert gfla.fuse_spectral_norm(net) == 4                      # the 2-D encoder block and the final convolution, as before
    assert len([m for m in net.modules() if type(m) is nn.Conv3d]) == 6 and type(net.block0.shortcut[0]) is nn.AvgPool3d
    assert "forward" not in net.block0.__dict__
    assert gfla.fuse_spectral_norm(net, temporal="kernels") == 6  # and a later call picks them up


def test_blocks_that_are_left_alone(gfla):
    Block3D = c3.Block3D
    torch.manual_seed(3)
    with_norm = Block3D(3, 8, 8, norm=nn.InstanceNorm3d)
    other_pool = Block3D(3, 8, 8, pool=(1, 2, 2))
    foreign = Block3D(3, 8, 8)
    foreign.model[1].register_forward_hook(lambda m, i, o: None)
    plain_conv = Block3D(3, 8, 8)
    torch.nn.utils.remove_spectral_norm(plain_conv.shortcut[1])
    for block in (with_norm, other_pool, foreign, plain_conv):
        assert gfla.fuse_spectral_norm(block, temporal="kernels") == 0
        assert not any(type(m) is gfla.SpectralConv3d for m in block.modules()) and "forward" not in block.__dict__
    good = Block3D(3, 8, 8)
    assert gfla.fuse_spectral_norm(good, temporal="kernels") == 3


def test_rewritten_network_equals_the_hooked_one_on_the_host(gfla):
    """two steps of D(a), D(b), backward, SGD in float32 on the CPU: outputs, u / v buffers and gradients bit for bit"""
    hooked, fused = _net(), _net()
    fused.load_state_dict(hooked.state_dict())
    assert gfla.fuse_spectral_norm(fused, grad="kernels", pointwise="kernels", temporal="kernels") == 10
    gen = torch.Generator().manual_seed(9)
    videos = [torch.rand(c3.VIDEO, generator=gen) * 2 - 1 for _ in range(2)]
    opts = [torch.optim.SGD(n.parameters(), lr=0.05) for n in (hooked, fused)]
    for step in range(2):
        outs = []
        for net, opt in zip((hooked, fused), opts):
            opt.zero_grad(set_to_none=True)
            ya, yb = net(videos[0]), net(videos[1])
            (ya + yb).square().mean().backward()
            outs.append((ya.detach(), yb.detach()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), step
        for (k, a), (_, b) in zip(hooked.named_buffers(), fused.named_buffers()):
            assert torch.equal(a, b), (step, k)
        for (k, a), (_, b) in zip(hooked.named_parameters(), fused.named_parameters()):
            assert a.grad is not None and torch.equal(a.grad, b.grad), (step, k)
        for opt in opts:
            opt.step()
    # a rewritten block on its own takes and returns torch's layout
    x = torch.randn(1, 3, 5, 12, 10)
    hooked.eval(), fused.eval()
    with torch.no_grad():
        assert torch.equal(fused.block0(x), hooked.block0(x))
        xf = gfla.to_frames_major(x)
        assert torch.equal(gfla.from_frames_major(fused.block0(xf, frames_major=True)), hooked.block0(x))


def test_patched_classes_keep_the_network_frames_major(gfla):
    """patch_reference_discriminators on stand-in classes: the network's forward converts once, both blocks run
    frames-major, and the result is the unpatched network's, bit for bit on the host"""
    import types
    Block3D, Net = c3.standin_classes()
    torch.manual_seed(5)
    hooked = c3.TemporalDiscriminator()
    with pytest.raises(ValueError, match="temporal"):
        gfla.patch_reference_discriminators(types.SimpleNamespace(), temporal="on")
    wrapped = gfla.patch_reference_discriminators(types.SimpleNamespace(TemporalDiscriminator=Net),
                                                  types.SimpleNamespace(ResBlock3DEncoder=Block3D), temporal="kernels")
    assert wrapped == ["TemporalDiscriminator"]
    assert gfla.patch_reference_discriminators(types.SimpleNamespace(TemporalDiscriminator=Net),
                                               types.SimpleNamespace(ResBlock3DEncoder=Block3D), temporal="kernels") == wrapped
    net = Net()
    net.load_state_dict(hooked.state_dict())
    assert not c3.hooked_convs(net) and "forward" not in net.block0.__dict__     # the class-wide wrapper serves the blocks
    seen = []
    net.block1.model[1].register_forward_pre_hook(lambda m, i: seen.append(tuple(i[0].shape)))
    x = torch.randn(c3.VIDEO)
    assert torch.equal(net(x), hooked(x)) and seen == [(1, 4, 8, 16, 16)]        # (B, L, C, H, W) between the blocks
    assert torch.equal(net.block0(x), hooked.block0(x))
    unrewritten = Block3D(3, 8, 8, norm=nn.InstanceNorm3d)                        # the wrapper calls the original forward
    assert unrewritten(x).shape == (1, 8, 4, 16, 16)


def test_install_needs_discriminator_convs(gfla):
    import inspect
    assert list(inspect.signature(gfla.install).parameters)[-1] == "temporal_convs"
    assert inspect.signature(gfla.install).parameters["temporal_convs"].default is False
    with pytest.raises(ValueError, match="temporal_convs"):
        gfla.install(temporal_convs=True)


@pytest.mark.skipif(not os.path.isdir("/root/reference/model/networks"), reason="reference checkout not present")
def test_install_rewrites_the_reference_temporal_discriminator(gfla):
    """install(discriminator_convs=True, temporal_convs=True) in a process of its own: the reference's own
    TemporalDiscriminator comes out rewritten and matches the unpatched one on the host"""
    code = r"""
import sys, types
sys.path.insert(0, %r)
import torch
from torch import nn
import global_flow_local_attention_amd as g
sys.modules.setdefault('torchvision', types.ModuleType('torchvision'))
g.install('/root/reference')
import model.networks.discriminator as d
torch.manual_seed(0)
plain = d.TemporalDiscriminator(input_length=6, ndf=8, img_f=32, layers=3)
keys = list(plain.state_dict())
bf = g.install('/root/reference', discriminator_convs=True, train_convs=True, pointwise_convs=True, temporal_convs=True)
net = d.TemporalDiscriminator(input_length=6, ndf=8, img_f=32, layers=3)
assert list(net.state_dict()) == keys
net.load_state_dict(plain.state_dict(), strict=True)
convs = [m for m in net.modules() if type(m) is g.SpectralConv3d]
assert len(convs) == 6 and all(c.grad == 'kernels' for c in convs)
assert not any(type(m) in (nn.Conv3d, nn.AvgPool3d, nn.Conv2d) for m in net.modules())
assert type(net.block0.shortcut[0]) is g.AvgPoolFrames and 'forward' not in net.block0.__dict__
x = torch.rand(1, 3, 6, 32, 32) * 2 - 1
ya, yb = plain(x), net(x)
assert ya.shape == yb.shape and torch.equal(ya, yb)
ya.square().mean().backward()
yb.square().mean().backward()
for (k, a), (_, b) in zip(plain.named_parameters(), net.named_parameters()):
    assert a.grad is not None and torch.equal(a.grad, b.grad), k
for (k, a), (_, b) in zip(plain.named_buffers(), net.named_buffers()):
    assert torch.equal(a, b), k
assert torch.equal(net.block0(x), plain.block0(x))
print('ok')
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]
