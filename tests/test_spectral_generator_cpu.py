"""Spectrally normalised generators without a GPU (spectral_norm.py): bit-exact parity of the dim-1 torch composition with
torch's own hook, the generator rewrite of a hooked network (keys, objects, slots, state dicts), bit-exact parity of the
rewritten CPU network with the hooked one, the residual forwards, the mixed entry points' status codes and install()'s
flags."""
import copy
import ctypes
import os
import types

import pytest
import torch
from torch import nn
from torch.nn.utils import spectral_norm as sn

import spectral_generator_util as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair():
    (hooked,), _, images = sg.generators("cpu", copies=1)
    return hooked, copy.deepcopy(hooked), images


# ---- the torch composition along dim 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 1, 2])
@pytest.mark.parametrize("shape", sg.DIM1, ids=lambda s: "x".join(map(str, s)))
def test_torch_composition_equals_the_hook(gfla, shape, iters):
    cin, cout, k = shape
    W, u, v, _ = sg.dim1_inputs(cin, cout, k, seed=7)
    conv, hook = sg.hooked_transpose(W, u, v, iters)
    hook.n_power_iterations = iters
    want = hook.compute_weight(conv, do_power_iteration=iters > 0)
    ui, vi = u.clone(), v.clone()
    got = gfla.torch_spectral_normalize(W, ui, vi, iters, 1e-12, dim=1)
    assert got.shape == W.shape and torch.equal(got, want)
    assert torch.equal(ui, conv.weight_u) and torch.equal(vi, conv.weight_v)
    if iters == 0:
        assert torch.equal(ui, u) and torch.equal(vi, v)
    for impl in ("auto", "torch"):                                      # the functional form on the host takes it
        ui, vi = u.clone(), v.clone()
        out, = gfla.spectral_normalize([W], [ui], [vi], iters, impl=impl, dims=[1])
        assert torch.equal(out, want) and torch.equal(ui, conv.weight_u) and torch.equal(vi, conv.weight_v)


def test_functional_form_checks_dims(gfla):
    W, u, v, _ = sg.dim1_inputs(5, 7, 3, seed=3)
    W0 = torch.randn(7, 45)
    mixed = gfla.spectral_normalize([W, W0], [u.clone(), u.clone()], [v.clone(), v.clone()], dims=[1, 0])
    assert mixed[0].shape == W.shape and mixed[1].shape == W0.shape
    assert torch.equal(mixed[1], gfla.spectral_normalize([W0], [u.clone()], [v.clone()])[0])
    for bad in ([0], [2], [1, 0], [-1]):
        with pytest.raises(ValueError):
            gfla.spectral_normalize([W], [u], [v], dims=bad)
    with pytest.raises(ValueError):
        gfla.spectral_normalize([W], [v], [u], dims=[1])                 # u is (Cout,), v the rest


def test_hook_lookup_by_dim(gfla):
    from global_flow_local_attention_amd import _rewrite
    up, down = sn(nn.ConvTranspose2d(4, 6, 3, 2, 1, 1)), sn(nn.Conv2d(4, 6, 3))
    assert _rewrite.spectral_norm_hook(up) is None and _rewrite.spectral_norm_hook(up, dims=(1,)).dim == 1
    assert _rewrite.spectral_norm_hook(down).dim == 0 and _rewrite.spectral_norm_hook(down, dims=(1,)) is None
    with pytest.raises(ValueError):
        gfla.SpectralConvTranspose(down)
    with pytest.raises(ValueError):
        gfla.SpectralConvTranspose(nn.ConvTranspose2d(4, 6, 3, 2, 1, 1))
    with pytest.raises(ValueError):
        gfla.SpectralConv(down, padding="replicate")
    with pytest.raises(ValueError):
        gfla.SpectralConv(sn(nn.Conv2d(4, 6, 3, 1, 1)), padding="reflect")      # its own zero padding: no pad in front
    with pytest.raises(ValueError):
        gfla.SpectralHead(sn(nn.Conv2d(4, 9, 3)))                        # more than 8 output channels
    with pytest.raises(ValueError):
        gfla.SpectralHead(down, post="relu")


# ---- the rewrite ---------------------------------------------------------------------------------------------------------------
def test_defaults_leave_the_generator_parts_alone(gfla):
    hooked, fused, _ = _pair()
    n = gfla.fuse_spectral_norm(fused)
    # every Conv2d as before -- the jump's and the head's as plain SpectralConv with the pad still in front --, no more
    assert n == sg.hooked_count() - 4
    for dec in fused.decs:
        assert type(dec.model[3]) is nn.ConvTranspose2d and type(dec.shortcut[0]) is nn.ConvTranspose2d
    for part in (fused.jump, fused.out):
        assert type(part.model[0]) is nn.LeakyReLU and type(part.model[1]) is nn.ReflectionPad2d
        assert type(part.model[2]) is gfla.SpectralConv and part.model[2].geometry is None and part.model[2].padding == "zeros"
    assert type(fused.out.model[3]) is nn.Tanh
    assert len(sg.hooked(fused)) == 4


def test_generator_rewrite_keeps_keys_objects_and_slots(gfla):
    hooked, fused, _ = _pair()
    before = sg.hooked(fused)
    assert len(before) == sg.hooked_count() == 15
    assert gfla.fuse_spectral_norm(fused, generator=True) == 15 and not sg.hooked(fused)
    assert gfla.fuse_spectral_norm(fused, generator=True) == 0
    assert len(fused._forward_pre_hooks) == 1 and len(fused._forward_hooks) == 1
    assert list(fused.state_dict().keys()) == list(hooked.state_dict().keys())
    for (k, p), (_, q) in zip(hooked.named_parameters(), fused.named_parameters()):
        assert p.shape == q.shape, k
    made = {id(m.original): m for m in fused.modules()
            if type(m) in (gfla.SpectralConv, gfla.SpectralConvTranspose, gfla.SpectralHead)}
    assert len(made) == 15
    for conv in before:
        new = made[id(conv)]
        assert new.weight_orig is conv.weight_orig and new.bias is conv.bias
        assert new.weight_u is conv.weight_u and new.weight_v is conv.weight_v
        assert list(new.state_dict().keys()) == list(conv.state_dict().keys())
        assert (new.n_power_iterations, new.eps) == (1, 1e-12) and new.dim == (1 if type(conv) is nn.ConvTranspose2d else 0)
    for dec in fused.decs:
        up, short = dec.model[3], dec.shortcut[0]
        assert type(up) is gfla.SpectralConvTranspose and (up.geometry, up.pre_slope, up.dim) == (2, 0.1, 1)
        assert type(dec.model[2]) is nn.Identity and type(short) is gfla.SpectralConvTranspose and short.pre_slope is None
        assert up.weight_u.shape == (up.weight_orig.size(1),)
    jump = fused.jump
    assert [type(m) for m in jump.model] == [nn.Identity, nn.Identity, gfla.SpectralConv] and jump.conv1 is jump.model[2]
    assert (jump.conv1.padding, jump.conv1.geometry, jump.conv1.pre_slope) == ("reflect", 0, 0.1)
    out = fused.out
    assert [type(m) for m in out.model] == [nn.Identity, nn.Identity, gfla.SpectralHead, nn.Identity]
    assert out.conv1 is out.model[2] and (out.conv1.post, out.conv1.pre_slope) == ("tanh", 0.1)
    assert fused.enc0.model[2].geometry == 1 and fused.res.shortcut[0].geometry is None


def test_what_the_generator_rewrite_leaves_alone(gfla):
    class Coord(nn.Module):
        def __init__(self):
            super(Coord, self).__init__()
            self.addcoords = nn.Identity()
            self.conv = sn(nn.ConvTranspose2d(4, 4, 3, 2, 1, 1))

    class Attn(nn.Module):
        def __init__(self):
            super(Attn, self).__init__()
            self.fully_connect_layer = nn.Sequential(nn.ReflectionPad2d(1), sn(nn.Conv2d(4, 4, 3)))

    twice = sn(nn.ConvTranspose2d(4, 4, 3, 2, 1, 1))
    twice.register_forward_hook(lambda m, i, o: o)
    other = sn(nn.ConvTranspose2d(4, 4, 4, 2, 1))                        # no kernel geometry: F.conv_transpose2d
    head = nn.Sequential(nn.ReLU(), nn.ReflectionPad2d(1), sn(nn.Conv2d(4, 2, 3)), nn.Sigmoid())
    net = nn.Sequential(Coord(), Attn(), twice, other, head)
    assert gfla.fuse_spectral_norm(net, generator=True) == 2
    assert type(net[0].conv) is nn.ConvTranspose2d and type(net[1].fully_connect_layer[1]) is nn.Conv2d and net[2] is twice
    assert type(net[3]) is gfla.SpectralConvTranspose and net[3].geometry is None and not net[3].fuses_add
    assert type(head[0]) is nn.ReLU and type(head[1]) is nn.Identity and type(head[3]) is nn.Identity   # only LeakyReLU folds
    assert type(head[2]) is gfla.SpectralHead and (head[2].pre_slope, head[2].post) == (None, "sigmoid")
    x = torch.randn(1, 4, 5, 4)
    want = torch.nn.functional.conv_transpose2d(x, net[3].normalized_weight(), net[3].bias, 2, 1)
    net[3].eval()
    assert net[3](x).shape == want.shape == (1, 4, 10, 8)


def test_state_dicts_interchange_strictly(gfla):
    hooked, fused, images = _pair()
    gfla.fuse_spectral_norm(fused, generator=True)
    fused(images[0])                                                              # move u and v on
    hooked.load_state_dict(fused.state_dict(), strict=True)
    for (k, a), (_, b) in zip(hooked.state_dict().items(), fused.state_dict().items()):
        assert torch.equal(a, b), k
    hooked(images[1])
    fused.load_state_dict(hooked.state_dict(), strict=True)
    for (k, a), (_, b) in zip(hooked.state_dict().items(), fused.state_dict().items()):
        assert torch.equal(a, b), k


# ---- parity with the hooked network on the CPU -------------------------------------------------------------------------------
def test_cpu_parity_with_the_hooked_network(gfla):
    hooked, fused, images = _pair()
    gfla.fuse_spectral_norm(fused, generator=True)
    results = []
    for net in (hooked, fused):
        opt = torch.optim.SGD(net.parameters(), lr=0.05)
        outs = [net(images[0])]
        outs[0].square().mean().backward()
        grads = [p.grad.clone() for p in net.parameters()]
        opt.step()
        outs.append(net(images[1]))                                  # on stepped weights and the u / v the first left
        net.eval()
        outs.append(net(images[0]))
        net.train()
        results.append((outs, grads))
    for a, b in zip(results[0][0], results[1][0]):
        assert a.shape == sg.IMAGE and torch.equal(a, b)
    for (k, _), a, b in zip(hooked.named_parameters(), results[0][1], results[1][1]):
        assert a.abs().max() > 0 and torch.equal(a, b), k
    for (k, a), (_, b) in zip(hooked.named_buffers(), fused.named_buffers()):
        assert torch.equal(a, b), k


def test_modules_called_on_their_own_normalise_themselves(gfla):
    hooked, fused, images = _pair()
    gfla.fuse_spectral_norm(fused, generator=True)
    x = torch.randn(2, 16, 5, 3)
    for name in ("decs.0", "jump", "res"):
        a, b = hooked.get_submodule(name), fused.get_submodule(name)
        assert torch.equal(a(x), b(x)), name
    assert torch.equal(hooked.decs[0].model[3].weight_u, fused.decs[0].model[3].weight_u)
    assert all(m.__dict__["_handed"] is None for m in fused.modules() if hasattr(m, "normalized_weight"))


# ---- the residual forwards -----------------------------------------------------------------------------------------------------
def _block_classes():
    class ResBlock(sg.ResBlock):
        def forward(self, x):
            return sg.ResBlock.forward(self, x)

    class ResBlockDecoder(sg.ResBlockDecoder):
        def forward(self, x):
            return sg.ResBlockDecoder.forward(self, x)
    return types.SimpleNamespace(ResBlock=ResBlock, ResBlockDecoder=ResBlockDecoder)


def test_residual_forwards_take_the_epilogue_for_the_three_slot_kinds(gfla, monkeypatch):
    from global_flow_local_attention_amd import _rewrite, gen_conv
    bf = _block_classes()
    assert gen_conv.install_residual_forwards(bf) == ["ResBlock", "ResBlockDecoder"]
    first = bf.ResBlock.forward
    assert first._gfla_residual_in_epilogue and gen_conv.install_residual_forwards(bf) and bf.ResBlock.forward is first
    routes = []
    real = _rewrite.run_with_add
    monkeypatch.setattr(_rewrite, "run_with_add", lambda seq, x, add: routes.append(type(seq[len(seq) - 1]).__name__) or real(seq, x, add))
    torch.manual_seed(5)
    x = torch.randn(2, 8, 5, 3)
    res, dec = bf.ResBlock(8).eval(), bf.ResBlockDecoder(8, 4).eval()
    unhooked = bf.ResBlock(16).eval()                                    # wider than the narrow heads fuse_inference_convs skips
    unhooked.model = nn.Sequential(nn.LeakyReLU(0.1), nn.Conv2d(16, 16, 3, 1, 1), nn.LeakyReLU(0.1), nn.Conv2d(16, 16, 3, 1, 1))
    x16 = torch.randn(2, 16, 5, 3)
    want = [res(x), dec(x), unhooked(x16)]
    assert routes == []                                                  # hooked modules and plain ones: the original
    gfla.fuse_spectral_norm(res, generator=True), gfla.fuse_spectral_norm(dec, generator=True)
    gfla.fuse_inference_convs(unhooked)
    got = [res(x), dec(x), unhooked(x16)]
    assert routes == ["SpectralConv", "SpectralConvTranspose", "InferenceConv"]
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert _rewrite.epilogue_slot(res.shortcut) is None                   # a 1x1 SpectralConv without pointwise kernels
    assert _rewrite.epilogue_slot(res.model) is res.model[3] and _rewrite.epilogue_slot(nn.Sequential()) is None
    odd = bf.ResBlockDecoder(8, 4).eval()
    odd.model[3] = sn(nn.ConvTranspose2d(8, 4, 4, 2, 1))                  # not the 3x3 kernels: the original forward
    odd.shortcut[0] = sn(nn.ConvTranspose2d(8, 4, 4, 2, 1))
    want = odd.eval()(x)
    gfla.fuse_spectral_norm(odd, generator=True)
    assert torch.equal(odd(x), want) and len(routes) == 3


def test_patch_reference_generators_rewrites_once_per_network(gfla):
    class PoseGenerator(sg.Generator):
        def __init__(self, *args, **kwargs):
            super(PoseGenerator, self).__init__(*args, **kwargs)

    module = types.SimpleNamespace(PoseGenerator=PoseGenerator)
    bf = _block_classes()
    assert gfla.patch_reference_generators(module, bf, grad="kernels", pointwise="kernels") == \
        ["PoseGenerator", "ResBlock", "ResBlockDecoder"]
    assert gfla.patch_reference_generators(module, bf) == ["PoseGenerator", "ResBlock", "ResBlockDecoder"]   # idempotent
    net = module.PoseGenerator()
    assert not sg.hooked(net) and len(net._forward_pre_hooks) == 1
    made = [m for m in net.modules() if hasattr(m, "normalized_weight")]
    assert len(made) == 15 and all(m.grad == "kernels" for m in made if hasattr(m, "grad"))
    assert net.res.shortcut[0].pointwise
    assert all(not sub._forward_pre_hooks for name, sub in net.named_modules() if name)      # one hook, on the network
    with pytest.raises(ValueError):
        gfla.patch_reference_generators(module, bf, grad="vendor")


# ---- entry points --------------------------------------------------------------------------------------------------------------
def test_mixed_entry_points_status_codes(gfla):
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    assert {"gfla_spectral_norm_mixed_fwd_f32", "gfla_spectral_norm_mixed_bwd_f32", "gfla_spectral_norm_mixed_layout",
            "gfla_spectral_norm_mixed_bwd_scratch_floats"} <= set(_lib.extension_symbols()) and _lib.ABI_VERSION == 8
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dims(*triples):
        flat = [n for t in triples for n in t]
        return ctypes.cast((ctypes.c_int64 * len(flat))(*flat), ctypes.c_void_p), len(triples)

    good, n = dims((4, 18, 9), (2, 3, 0))
    off, tot = (ctypes.c_int64 * 6)(), (ctypes.c_int64 * 2)()
    po, pt = ctypes.cast(off, ctypes.c_void_p), ctypes.cast(tot, ctypes.c_void_p)
    layout, floats = L.gfla_spectral_norm_mixed_layout, L.gfla_spectral_norm_mixed_bwd_scratch_floats
    fwd, bwd = L.gfla_spectral_norm_mixed_fwd_f32, L.gfla_spectral_norm_mixed_bwd_f32
    assert layout(good, n, po, pt) == 0
    assert list(off) == [0, 0, 18, 72, 22, 25] and list(tot) == [78, 27] and floats(good, n) == 2
    assert layout(good, n, None, pt) == -1 and layout(None, n, po, pt) == -1
    assert fwd(None, good, n, p, p, p, p, 1, 1e-12, None) == -1 and fwd(p, good, n, None, p, p, p, 1, 1e-12, None) == -1
    assert fwd(p, good, n, p, None, p, p, 1, 1e-12, None) == -1 and fwd(p, None, n, p, p, p, p, 1, 1e-12, None) == -1
    assert bwd(None, good, n, p, p, p, p, p, None) == -1 and bwd(p, good, n, p, p, p, None, p, None) == -1
    assert fwd(p, good, 0, p, p, p, p, 1, 1e-12, None) == -2 and fwd(p, good, n, p, p, p, p, -1, 1e-12, None) == -2
    assert fwd(p, good, n, p, p, p, p, 1, 0.0, None) == -2
    for triple in ((4, 0, 0), (-1, 9, 9), (4, 18, -1), (4, 20, 9)):        # non-positive; negative inner; K no multiple of inner
        bad, m = dims(triple)
        assert fwd(p, bad, m, p, p, p, p, 1, 1e-12, None) == -2 and bwd(p, bad, m, p, p, p, p, p, None) == -2
        assert layout(bad, m, po, pt) == -2 and floats(bad, m) == -2
    for triple in ((2 ** 24 + 1, 1, 1), (1, 2 ** 24 + 1, 1), (2 ** 16, 2 ** 15, 1), (4, 100, 50)):   # beyond the kernels
        big, m = dims(triple)
        assert fwd(p, big, m, p, p, p, p, 1, 1e-12, None) == -3 and bwd(p, big, m, p, p, p, p, p, None) == -3
        assert layout(big, m, po, pt) == -3 and floats(big, m) == -3
    many, m = dims(*[(1, 1, 1)] * 65536)
    assert fwd(p, many, m, p, p, p, p, 1, 1e-12, None) == -3


# ---- install() -----------------------------------------------------------------------------------------------------------------
def test_install_flag_combinations(gfla):
    for flags in (dict(train_convs=True), dict(pointwise_convs=True), dict(temporal_convs=True, generator_spectral=True)):
        with pytest.raises(ValueError):
            gfla.install(**flags)


@pytest.mark.skipif(not os.path.isdir("/root/reference/model/networks"), reason="reference checkout not present")
def test_install_rewrites_the_reference_pose_generator(gfla):
    """train_convs / pointwise_convs accept generator_spectral as the flag they need; a PoseGenerator built afterwards
    (use_spect=True is its default) has no hooked module left outside CoordConv / ExtractorAttn, its keys unchanged"""
    import subprocess
    import sys
    code = r"""
import sys, types
sys.path.insert(0, %r)
import torch
from torch import nn
import global_flow_local_attention_amd as g
sys.modules.setdefault('torchvision', types.ModuleType('torchvision'))
import importlib
g.install('/root/reference')
gen = importlib.import_module('model.networks.generator')
kw = dict(ngf=16, img_f=64, layers=3, norm='instance', activation='LeakyReLU', attn_layer=[2, 3],
          extractor_kz={'2': 5, '3': 3}, use_spect=True)
torch.manual_seed(0)
plain = gen.PoseGenerator(**kw)
bf = g.install('/root/reference', generator_spectral=True, train_convs=True, pointwise_convs=True, fuse_instance_norm=True)
assert bf.ResBlockDecoder.forward._gfla_residual_in_epilogue and bf.ResBlock.forward._gfla_residual_in_epilogue
torch.manual_seed(0)
net = gen.PoseGenerator(**kw)
assert list(net.state_dict().keys()) == list(plain.state_dict().keys())
left = [n for n, m in net.named_modules() if 'weight_orig' in m._parameters and m._forward_pre_hooks]
assert not left, left
made = [m for m in net.modules() if hasattr(m, 'normalized_weight')]
hooked = [m for m in plain.modules() if 'weight_orig' in m._parameters and m._forward_pre_hooks]
assert len(made) == len(hooked) > 20 and len(net._forward_pre_hooks) == 1
ups = [m for m in made if type(m) is g.SpectralConvTranspose]
assert len(ups) == 2 * (3 + 3) and all(m.geometry == 2 and m.grad == 'kernels' and m.dim == 1 for m in ups)
assert type(net.target.outconv.conv1) is g.SpectralHead and net.target.outconv.conv1.post == 'tanh'
assert net.target.outconv.model[2] is net.target.outconv.conv1
jumps = [m for m in net.modules() if type(m).__name__ == 'Jump']
assert jumps and all(type(j.conv1) is g.SpectralConv and j.conv1.padding == 'reflect' and j.model[2] is j.conv1 for j in jumps)
dec = net.target.decoder0[-1]
x = torch.randn(1, 64, 4, 3)
dec.eval()
with torch.no_grad():
    assert torch.equal(dec(x), bf.ResBlockDecoder.forward.__wrapped__(dec, x))
print('ok')
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]
