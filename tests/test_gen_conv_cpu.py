"""Generator inference convolutions without a GPU: the packed index maps of csrc/gen_conv.hip (emulated in
gen_conv_util) reproduce torch's convolutions in float64, the host-only entry points answer and refuse as documented, and
fuse_inference_convs rewrites generator-shaped blocks without changing keys, Parameters, results or gradients."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import gen_conv_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REF = os.path.isdir("/root/reference/model/networks")


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# (B, Cin, Cout, H, W): channels that are no multiple of either chunk (8, 16) nor of 32; odd maps
@pytest.mark.parametrize("ck", [8, 16])
@pytest.mark.parametrize("reflect", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 7, 6, 9), (1, 20, 40, 2, 3)])
def test_s1k3_packing_reproduces_conv2d(shape, reflect, ck):
    B, Cin, Cout, H, W = shape
    x, w = _rand((B, Cin, H, W), 1), _rand((Cout, Cin, 3, 3), 2)
    packed = gu.pack_emulated(w, gu.S1K3, ck)
    assert packed.shape == (9,) + gu.packed_dims(Cout, Cin, ck) + (ck,)
    got = gu.conv_from_packed(x, packed, gu.S1K3, Cout, ck, reflect)
    want = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w) if reflect else F.conv2d(x, w, padding=1)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    assert not packed[:, :, Cout:].any() and packed.count_nonzero() == w.numel()       # zero-padded, nothing lost


@pytest.mark.parametrize("ck", [8, 16])
@pytest.mark.parametrize("shape", [(2, 5, 7, 6, 8), (1, 20, 40, 33, 17), (1, 3, 4, 2, 2), (1, 9, 33, 3, 7)])
def test_s2k4_packing_reproduces_strided_conv2d(shape, ck):
    B, Cin, Cout, H, W = shape
    x, w = _rand((B, Cin, H, W), 3), _rand((Cout, Cin, 4, 4), 4)
    packed = gu.pack_emulated(w, gu.S2K4, ck)
    assert packed.shape[0] == 16
    got = gu.conv_from_packed(x, packed, gu.S2K4, Cout, ck)
    want = F.conv2d(x, w, stride=2, padding=1)
    assert got.shape == want.shape == (B, Cout) + gu.out_size(gu.S2K4, H, W)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("ck", [8, 16])
@pytest.mark.parametrize("shape", [(2, 5, 7, 3, 4), (1, 20, 40, 1, 1), (1, 9, 33, 5, 2)])
def test_t2k3_packing_reproduces_conv_transpose2d_phase_by_phase(shape, ck):
    B, Cin, Cout, H, W = shape
    x, w = _rand((B, Cin, H, W), 5), _rand((Cin, Cout, 3, 3), 6)             # torch's transposed order
    packed = gu.pack_emulated(w, gu.T2K3, ck)
    got = gu.conv_from_packed(x, packed, gu.T2K3, Cout, ck)
    want = F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
    assert got.shape == want.shape == (B, Cout, 2 * H, 2 * W)
    for phase in range(4):
        dy, dx = divmod(phase, 2)
        assert torch.allclose(got[:, :, dy::2, dx::2], want[:, :, dy::2, dx::2], rtol=0, atol=1e-12), phase
    # 1 + 2 + 2 + 4 taps: nine per input pixel, and every tap of a phase reads another neighbour
    per_phase = [[gu.t2k3_tap(t)[1:] for t in range(9) if gu.t2k3_tap(t)[0] == p] for p in range(4)]
    assert [len(p) for p in per_phase] == [1, 2, 2, 4] and all(len(set(p)) == len(p) for p in per_phase)


def test_host_only_entry_points(gfla):
    from global_flow_local_attention_amd import _lib, gen_conv
    L = _lib.lib()
    UNSUPPORTED = -3
    # sizes
    assert gen_conv.out_size(0, 33, 17) == (33, 17) and gen_conv.out_size(1, 33, 17) == (16, 8)
    assert gen_conv.out_size(1, 2, 2) == (1, 1) and gen_conv.out_size(1, 3, 70) == (1, 35) and gen_conv.out_size(2, 1, 40) == (2, 80)
    ho, wo = ctypes.c_int64(), ctypes.c_int64()
    pho, pwo = ctypes.addressof(ho), ctypes.addressof(wo)
    assert L.gfla_gen_conv_out_size(0, 4, 4, None, pwo) == -1 and L.gfla_gen_conv_out_size(0, 4, 4, pho, None) == -1
    for args in ((3, 4, 4), (-1, 4, 4), (0, 0, 4), (2, 4, -1), (1, 1, 4), (1, 4, 1)):
        assert L.gfla_gen_conv_out_size(*args, pho, pwo) == -2, args
    # packed bytes: taps x chunks x padded Cout x 32 bytes
    for geometry, taps in ((0, 9), (1, 16), (2, 9)):
        for esize in (2, 4):
            ck = 32 // esize
            for cout, cin in ((1, 1), (40, 20), (64, 64), (96, 128)):
                want = taps * -(-cin // ck) * -(-cout // 32) * 32 * 32
                assert L.gfla_gen_conv_packed_bytes(cout, cin, geometry, esize) == want
    for args in ((0, 4, 0, 4), (4, -1, 0, 4), (4, 4, 3, 4), (4, 4, -1, 2), (4, 4, 0, 8), (4, 4, 0, 3)):
        assert L.gfla_gen_conv_packed_bytes(*args) == -2, args
    assert L.gfla_gen_conv_packed_bytes(65537, 4, 0, 4) == UNSUPPORTED and L.gfla_gen_conv_packed_bytes(4, 65537, 2, 2) == UNSUPPORTED
    assert L.gfla_gen_conv_packed_bytes(65536, 1, 0, 4) > 0
    # launch geometry: covers the tiled map and the channels, stages within its budget, fits the LDS twice per CU
    out = (ctypes.c_int64 * 8)()
    po = ctypes.cast(out, ctypes.c_void_p)
    items = {0: 11, 1: 21, 2: 6}
    for geometry in (0, 1, 2):
        for cout in (1, 7, 32, 40, 64, 65, 96, 256, 512):
            for (H, W) in ((128, 88), (64, 44), (32, 22), (33, 17), (2, 2), (3, 70), (9, 7), (2, 40), (16, 11)):
                for esize in (2, 4):
                    assert L.gfla_gen_conv_geometry(geometry, cout, H, W, esize, po) == 0
                    tw, th, wm, tx, ty, cblocks, halo, lds = list(out)
                    th_map, tw_map = gu.out_size(1, H, W) if geometry == 1 else (H, W)
                    assert tw in (8, 16, 32) and wm in (1, 2) and tw * th == (4 // wm) * (1 if geometry == 2 else 2) * 32
                    assert tx * tw >= tw_map > (tx - 1) * tw and ty * th >= th_map > (ty - 1) * th
                    assert cblocks * wm * 2 * 32 >= cout > (cblocks - 1) * wm * 2 * 32
                    assert halo == {0: (th + 2) * (tw + 2), 1: (2 * th + 2) * (2 * tw + 2), 2: (th + 1) * (tw + 1)}[geometry]
                    assert 8 * halo <= items[geometry] * 256 and lds == 2 * 32 * halo and 2 * lds <= 160 * 1024 and lds <= 64 * 1024
    assert L.gfla_gen_conv_geometry(0, 64, 8, 8, 4, None) == -1
    for args in ((3, 64, 8, 8, 4), (-1, 64, 8, 8, 4), (0, 0, 8, 8, 4), (0, 64, 0, 8, 4), (0, 64, 8, 8, 8), (1, 64, 1, 8, 4),
                 (1, 64, 8, 1, 2)):
        assert L.gfla_gen_conv_geometry(*args, po) == -2, args
    assert L.gfla_gen_conv_geometry(0, 65537, 8, 8, 4, po) == UNSUPPORTED
    assert L.gfla_gen_conv_geometry(0, 64, 1 << 16, 1 << 15, 4, po) == UNSUPPORTED        # plane of 2^31
    assert L.gfla_gen_conv_geometry(2, 64, 1 << 15, 1 << 14, 4, po) == UNSUPPORTED        # output plane of 2^31
    assert L.gfla_gen_conv_geometry(0, 64, 1 << 15, 1 << 15, 4, po) == 0

    # the launching entry points check before they launch: nothing below reaches a GPU
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n = None
    for sfx in ("f32", "f16", "bf16"):
        fwd, pack = getattr(L, "gfla_gen_conv_fwd_" + sfx), getattr(L, "gfla_gen_conv_pack_weights_" + sfx)
        ok = (1, 4, 4, 4, 4, 0, 0, 0, 0.0, n)                          # B, Cin, Cout, H, W, geometry, pad_mode, pre_act, slope
        assert fwd(n, p, p, n, p, *ok) == -1 and fwd(p, n, p, n, p, *ok) == -1 and fwd(p, p, n, n, n, *ok) == -1
        for bad in ((0, 4, 4, 4, 4, 0, 0), (1, 0, 4, 4, 4, 0, 0), (1, 4, -1, 4, 4, 0, 0), (1, 4, 4, 0, 4, 0, 0),
                    (1, 4, 4, 4, 0, 0, 0), (1, 4, 4, 4, 4, 3, 0), (1, 4, 4, 4, 4, -1, 0), (1, 4, 4, 4, 4, 0, 2),
                    (1, 4, 4, 4, 4, 0, -1), (1, 4, 4, 4, 4, 1, 1), (1, 4, 4, 4, 4, 2, 1), (1, 4, 4, 1, 4, 0, 1),
                    (1, 4, 4, 4, 1, 0, 1), (1, 4, 4, 1, 4, 1, 0), (1, 4, 4, 4, 1, 1, 0)):
            assert fwd(p, p, n, n, p, *bad, 0, 0.0, n) == -2, (sfx, bad)
        for big in ((65536, 4, 4, 4, 4, 0, 0), (1, 65537, 4, 4, 4, 0, 0), (1, 4, 65537, 4, 4, 2, 0), (1, 4, 4, 1 << 16, 1 << 15, 0, 0),
                    (1, 4, 4, 1 << 15, 1 << 14, 2, 0)):
            assert fwd(p, p, n, n, p, *big, 0, 0.0, n) == UNSUPPORTED, (sfx, big)
        assert pack(n, 0, p, 4, 4, 0, n) == -1 and pack(p, 0, n, 4, 4, 0, n) == -1
        for bad in ((3, 4, 4, 0), (-1, 4, 4, 0), (0, 0, 4, 0), (0, 4, 0, 0), (0, 4, 4, 3), (0, 4, 4, -1)):
            assert pack(p, bad[0], p, *bad[1:], n) == -2, (sfx, bad)
        assert pack(p, 0, p, 65537, 4, 1, n) == UNSUPPORTED
    assert set(_lib.extension_symbols()) >= {"gfla_gen_conv_fwd_bf16", "gfla_gen_conv_geometry"} and _lib.ABI_VERSION == 8


# ---- fuse_inference_convs on blocks written in gen_conv_util -----------------------------------------------------------
def _snapshot(net):
    return list(net.state_dict().keys()), {k: id(p) for k, p in net.named_parameters(remove_duplicate=False)}


def _check_rewrite(gfla, net, x, count, extra=()):
    keys, ids = _snapshot(net)
    net.eval()
    with torch.no_grad():
        before = net(x, *extra)
    assert gfla.fuse_inference_convs(net) == count
    assert _snapshot(net) == (keys, ids)
    with torch.no_grad():
        after = net(x, *extra)
    assert torch.equal(before, after)                         # the CPU takes the torch path
    assert gfla.fuse_inference_convs(net) == 0                # nothing left to take
    out = net(x, *extra)                                      # grad mode: the composition, gradients for every weight
    assert torch.equal(out, before)
    out.sum().backward()
    fused = [m for m in net.modules() if type(m) is gfla.InferenceConv]
    assert len({id(m) for m in fused}) == count and all(m.weight.grad is not None for m in fused)
    return fused


def test_fuse_encoder_block(gfla):
    torch.manual_seed(0)
    net = gu.EncoderBlock(5, 12, nn.LeakyReLU(0.1))
    act = net.model[1]
    fused = _check_rewrite(gfla, net, torch.randn(2, 5, 9, 8), 2)
    assert [(m.geometry, m.padding, m.pre_slope) for m in fused] == [(1, "zeros", 0.1), (0, "zeros", 0.1)]
    assert type(net.model[1]) is nn.Identity and type(net.model[4]) is nn.Identity and type(net.model[0]) is nn.InstanceNorm2d
    assert type(act) is nn.LeakyReLU                          # the shared activation object itself is untouched
    assert type(fused[0].original) is nn.Conv2d and fused[0].original.weight is fused[0].weight
    assert "original" not in dict(fused[0].named_children())


def test_fuse_jump_and_its_second_registration(gfla):
    torch.manual_seed(1)
    net = gu.Jump(12, nn.LeakyReLU(0.2))
    keys = list(net.state_dict().keys())
    assert keys == ["conv1.weight", "conv1.bias", "model.2.weight", "model.2.bias"]
    fused = _check_rewrite(gfla, net, torch.randn(1, 12, 5, 4), 1)
    assert (fused[0].geometry, fused[0].padding, fused[0].pre_slope) == (0, "reflect", 0.2)
    assert net.conv1 is net.model[2] is fused[0]
    assert type(net.model[0]) is nn.Identity and type(net.model[1]) is nn.Identity


def test_fuse_decoder_pair_and_residual(gfla):
    torch.manual_seed(2)
    net = gu.DecoderBlock(12, 9, nn.LeakyReLU(0.1))
    fused = _check_rewrite(gfla, net, torch.randn(2, 12, 3, 5), 3)
    assert {(m.geometry, m.pre_slope) for m in fused} == {(0, 0.1), (2, None), (2, 0.1)}
    assert type(net.shortcut[0]) is gfla.InferenceConv and type(net.model[5].original) is nn.ConvTranspose2d
    res = gu.ResBlock(10, nn.LeakyReLU(0.1))
    _check_rewrite(gfla, res, torch.randn(1, 10, 4, 4), 2)
    # the functional forms on the host are the composition, addend included
    x, w, b = torch.randn(1, 4, 3, 3), torch.randn(4, 9, 3, 3), torch.randn(9)
    add = torch.randn(1, 9, 6, 6)
    want = F.conv_transpose2d(F.leaky_relu(x, 0.3), w, b, stride=2, padding=1, output_padding=1) + add
    assert torch.equal(gfla.conv_transpose3x3_up(x, w, b, add=add, pre_slope=0.3), want)
    w4 = torch.randn(9, 4, 4, 4)
    assert torch.equal(gfla.conv4x4_down(x.double(), w4.double(), b.double()), F.conv2d(x.double(), w4.double(), b.double(), stride=2, padding=1))
    w3 = torch.randn(9, 4, 3, 3)
    assert torch.equal(gfla.conv3x3(x, w3, None, padding="reflect", impl="torch"), F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w3))
    with pytest.raises(ValueError):
        gfla.conv3x3(x[:, :, :1], w3, padding="reflect")
    with pytest.raises(ValueError):
        gfla.conv4x4_down(x[:, :, :1], w4)
    with pytest.raises(ValueError):
        gfla.conv3x3(x, w3, add=add)


class _Coord(nn.Module):
    """a coordinate convolution: the convolution is an attribute, not a slot of a Sequential"""

    def __init__(self, c):
        super(_Coord, self).__init__()
        self.conv = nn.Conv2d(c + 2, c, 3, 1, 1)

    def forward(self, x):
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, x.size(2)), torch.linspace(-1, 1, x.size(3)), indexing="ij")
        grid = torch.stack((xx, yy)).expand(x.size(0), 2, -1, -1).to(x)
        return self.conv(torch.cat((x, grid), 1))


def test_what_is_left_alone(gfla):
    c = 12
    hooked = nn.Conv2d(c, c, 3, 1, 1)
    hooked.register_forward_hook(lambda m, i, o: None)

    class _Attn(nn.Module):
        def __init__(self):
            super(_Attn, self).__init__()
            self.fully_connect_layer = nn.Sequential(nn.Conv2d(c, c, 3, 1, 1), nn.LeakyReLU(0.1), nn.Conv2d(c, 9, 1))

    left = nn.Sequential(
        torch.nn.utils.spectral_norm(nn.Conv2d(c, c, 3, 1, 1)),              # spectral norm: a forward pre-hook
        torch.nn.utils.spectral_norm(nn.ConvTranspose2d(c, c, 3, 2, 1, output_padding=1)),
        hooked,
        _Coord(c),
        nn.Conv2d(c, c, 3, 1, 1, groups=2),
        nn.Conv2d(c, c, 3, 1, 2, dilation=2),
        nn.Conv2d(c, c, 3, 1, 1, padding_mode="reflect"),
        nn.Conv2d(c, c, 4, 2, 1, padding_mode="replicate"),
        nn.Conv2d(c, c, 1),                                                  # 1x1 shortcut
        nn.Conv2d(c, c, 3, 1, 0),                                            # no pad in front of it: another map
        nn.Conv2d(c, c, 3, 2, 1),
        nn.Conv2d(c, c, 4, 2, 0),
        nn.ConvTranspose2d(c, c, 3, 2, 1),                                   # no output padding
        nn.ConvTranspose2d(c, c, 4, 2, 1),
        _Attn(),
        gfla.HeadConv3x3(c, 3, padding="reflect", pre_slope=0.1, post="tanh"),
        nn.Conv2d(c, 2, 3, 1, 1),                                            # a flow head: head_conv.py's
        nn.ReLU(), nn.Conv2d(c, c, 3, 1, 1),                                 # taken, but a ReLU is not folded in
    )
    types = [type(m) for m in left]
    assert gfla.fuse_inference_convs(left) == 1
    assert [type(m) for m in left][:-1] == types[:-1] and type(left[-1]) is gfla.InferenceConv and left[-1].pre_slope is None
    assert type(left[-2]) is nn.ReLU
    assert all(type(m) is not gfla.InferenceConv for m in left[14].modules())
    with pytest.raises(ValueError):
        gfla.fuse_inference_convs(left, impl="triton")


_REFERENCE_CODE = r"""
import sys, types
sys.path.insert(0, %r)
import torch
from torch import nn
import global_flow_local_attention_amd as g
sys.modules.setdefault('torchvision', types.ModuleType('torchvision'))
kw = dict(image_nc=3, structure_nc=18, ngf=64, img_f=512, layers=3, num_blocks=2, use_spect=False, attn_layer=[2, 3],
          norm='instance', activation='LeakyReLU', extractor_kz={'2': 5, '3': 3})
bf = g.install('/root/reference')
import model.networks.generator as gen
for name in ('EncoderBlock', 'ResBlock', 'ResBlockDecoder', 'Jump'):         # install() without the argument patches nothing
    cls = getattr(bf, name)
    assert not hasattr(cls.__init__, '_gfla_fuses_inference_convs') and not hasattr(cls.forward, '_gfla_residual_in_epilogue')
torch.manual_seed(0)
plain = gen.PoseGenerator(**kw)
assert not any(type(m) is g.InferenceConv for m in plain.modules())
g.install('/root/reference', inference_convs=True, fuse_instance_norm=True, fuse_heads=True)
g.install('/root/reference', inference_convs=True)                           # idempotent
assert bf.ResBlock.forward._gfla_residual_in_epilogue and bf.ResBlock.forward.__wrapped__.__name__ == 'forward'
torch.manual_seed(0)
net = gen.PoseGenerator(**kw)
assert list(net.state_dict().keys()) == list(plain.state_dict().keys())
net.load_state_dict(plain.state_dict(), strict=True)
inside = set()
for m in net.modules():
    if isinstance(m, bf.ExtractorAttn):
        inside.update(id(s) for s in m.modules())
left = [m for m in net.modules() if type(m) in (nn.Conv2d, nn.ConvTranspose2d) and id(m) not in inside]
# outside the attention blocks only head_conv.py's narrow 3x3 heads remain (the flow / mask heads, fused per call by
# flow_mask_heads, and the second registration of the image head's convolution)
assert left and all(type(m) is nn.Conv2d and m.kernel_size == (3, 3) and m.out_channels <= 3 for m in left), left
assert inside and sum(type(m) is g.InferenceConv for m in net.modules()) >= 30
assert sum(type(m) is g.HeadConv3x3 for m in net.modules()) == 1
# a decoder block: the residual enters the transposed convolution's epilogue, and the host result is the reference's
blk = bf.ResBlockDecoder(8, 6, None, nn.InstanceNorm2d, nn.LeakyReLU(0.1), False, False).eval()
x = torch.randn(2, 8, 5, 4)
with torch.no_grad():
    want = bf.ResBlockDecoder.forward.__wrapped__(blk, x)
    assert torch.equal(blk(x), want)
res = bf.ResBlock(8, None, None, nn.InstanceNorm2d, nn.LeakyReLU(0.1), False, False, False).eval()
with torch.no_grad():
    assert torch.equal(res(x), bf.ResBlock.forward.__wrapped__(res, x))
spect = bf.ResBlock(8, None, None, nn.InstanceNorm2d, nn.LeakyReLU(0.1), False, True, False)     # spectral norm: left alone
assert not any(type(m) is g.InferenceConv for m in spect.modules())
spect(x)
print('ok')
"""


@pytest.mark.skipif(not HAVE_REF, reason="reference checkout not present")
def test_install_inference_convs_into_unmodified_reference():
    out = subprocess.run([sys.executable, "-c", _REFERENCE_CODE % ROOT], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-3000:]
