"""The batched spectral norm without a GPU (spectral_norm.py): the rewrite of a hooked network, bit-exact parity of the
torch composition with torch's own hook on the CPU, the entry points' status codes, and the adversarial loss that goes
with the discriminators."""
import copy
import ctypes
import os

import pytest
import torch
from torch import nn
from torch.nn.utils import spectral_norm as sn

import discriminator_util as du

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(iters=1):
    (hooked,), _, images = du.discriminators("cpu", copies=1, iters=iters)
    return hooked, copy.deepcopy(hooked), images


# ---- the rewrite -----------------------------------------------------------------------------------------------------
def test_rewrite_keeps_keys_objects_and_slots(gfla):
    hooked, fused, _ = _pair()
    convs = du.hooked_convs(fused)
    assert len(convs) == 10 and gfla.fuse_spectral_norm(fused) == 10 and not du.hooked_convs(fused)
    assert gfla.fuse_spectral_norm(fused) == 0                                    # nothing left; one pair of hooks
    assert len(fused._forward_pre_hooks) == 1 and len(fused._forward_hooks) == 1
    assert list(fused.state_dict().keys()) == list(hooked.state_dict().keys())
    made = [m for m in fused.modules() if type(m) is gfla.SpectralConv]
    assert len(made) == 10
    for conv, new in zip(convs, made):
        assert new.weight_orig is conv.weight_orig and new.bias is conv.bias
        assert new.weight_u is conv.weight_u and new.weight_v is conv.weight_v
        assert (new.n_power_iterations, new.eps) == (1, 1e-12)
    for block in fused.blocks:
        assert type(block.model[0]) is nn.Identity and type(block.model[2]) is nn.Identity
        assert (block.model[1].pre_slope, block.model[1].geometry) == (0.1, 0) and block.model[3].geometry == 1
        assert type(block.shortcut[0]) is nn.AvgPool2d and block.shortcut[1].geometry is None
    assert type(fused.act) is nn.LeakyReLU and fused.conv.pre_slope is None        # not in a Sequential: not folded


def test_state_dicts_interchange_strictly(gfla):
    hooked, fused, images = _pair()
    gfla.fuse_spectral_norm(fused)
    fused(images[0])                                                              # move u and v on
    hooked.load_state_dict(fused.state_dict(), strict=True)
    for (k, a), (_, b) in zip(hooked.state_dict().items(), fused.state_dict().items()):
        assert torch.equal(a, b), k
    hooked(images[1])
    fused.load_state_dict(hooked.state_dict(), strict=True)
    for (k, a), (_, b) in zip(hooked.state_dict().items(), fused.state_dict().items()):
        assert torch.equal(a, b), k


class _CoordConv(nn.Module):
    def __init__(self):
        super(_CoordConv, self).__init__()
        self.addcoords = nn.Identity()
        self.conv = sn(nn.Conv2d(5, 8, 3, 1, 1))

    def forward(self, x):
        return self.conv(self.addcoords(x))


def test_what_is_left_alone(gfla):
    twice = sn(nn.Conv2d(8, 8, 3, 1, 1))
    twice.register_forward_hook(lambda m, i, o: o)
    shared = nn.LeakyReLU(0.2)
    net = nn.Sequential(_CoordConv(), sn(nn.ConvTranspose2d(8, 8, 3, 2, 1, 1)), twice, shared, sn(nn.Conv2d(8, 4, 3, 1, 1)),
                        shared, nn.Conv2d(4, 4, 3, 1, 1))
    assert next(iter(net[1]._forward_pre_hooks.values())).dim == 1
    assert gfla.fuse_spectral_norm(net) == 1
    assert type(net[4]) is gfla.SpectralConv and net[4].pre_slope == 0.2 and type(net[3]) is nn.Identity
    assert net[5] is shared                                                       # the object's other slot is untouched
    assert type(net[0].conv) is nn.Conv2d and type(net[1]) is nn.ConvTranspose2d and net[2] is twice
    assert type(net[6]) is nn.Conv2d
    # only an nn.LeakyReLU is folded in, and a second registration of a rewritten convolution gets the same module
    again = nn.Sequential(nn.ReLU(), sn(nn.Conv2d(4, 4, 3, 1, 1)))
    again.alias = again[1]
    assert gfla.fuse_spectral_norm(again) == 1 and type(again[0]) is nn.ReLU
    assert type(again[1]) is gfla.SpectralConv and again[1].pre_slope is None and again.alias is again[1]
    with pytest.raises(ValueError):
        gfla.SpectralConv(nn.Conv2d(4, 4, 3))
    with pytest.raises(ValueError):
        gfla.fuse_spectral_norm(net, grad="vendor")


def test_the_other_rewrites_still_skip_hooked_modules(gfla):
    (hooked,), _, _ = du.discriminators("cpu", copies=1)
    head = nn.Sequential(nn.LeakyReLU(0.1), nn.ReflectionPad2d(1), sn(nn.Conv2d(16, 3, 3)), nn.Tanh())
    net = nn.Sequential(hooked, head)
    assert gfla.fuse_inference_convs(net) == 0 and gfla.fuse_output_heads(net) == 0
    assert len(du.hooked_convs(net)) == 11


# ---- parity with torch's hook on the CPU -----------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 2])
def test_cpu_parity_with_the_hook(gfla, iters):
    hooked, fused, images = _pair(iters)
    gfla.fuse_spectral_norm(fused)
    results = []
    for net in (hooked, fused):
        outs = [net(images[0]), net(images[1])]
        outs[1].square().mean().backward()
        net.eval()
        outs.append(net(images[0]))
        net.train()
        results.append(outs)
    for a, b in zip(*results):
        assert torch.equal(a, b)
    for (k, a), (_, b) in zip(hooked.named_buffers(), fused.named_buffers()):
        assert torch.equal(a, b), k
    for (k, p), (_, q) in zip(hooked.named_parameters(), fused.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k


def test_two_forwards_then_one_backward(gfla):
    hooked, fused, images = _pair()
    gfla.fuse_spectral_norm(fused)
    for net in (hooked, fused):
        (net(images[0]) + net(images[1])).sum().backward()
    for (k, p), (_, q) in zip(hooked.named_parameters(), fused.named_parameters()):
        assert p.grad is not None and p.grad.abs().max() > 0 and torch.equal(p.grad, q.grad), k


def test_a_block_called_on_its_own_normalises_itself(gfla):
    hooked, fused, images = _pair()
    gfla.fuse_spectral_norm(fused)
    assert torch.equal(hooked.blocks[0](images[0]), fused.blocks[0](images[0]))
    assert torch.equal(hooked.blocks[0].model[1].weight_u, fused.blocks[0].model[1].weight_u)
    assert all(m.__dict__["_handed"] is None for m in fused.modules() if type(m) is gfla.SpectralConv)


def test_functional_form_on_the_host(gfla):
    W, u, v, _ = du.matrix_inputs(7, 80, seed=3)
    lin = sn(nn.Linear(80, 7, bias=False))
    with torch.no_grad():
        lin.weight_orig.copy_(W), lin.weight_u.copy_(u), lin.weight_v.copy_(v)
    want = next(iter(lin._forward_pre_hooks.values())).compute_weight(lin, True)
    for impl in ("auto", "torch"):
        ui, vi = u.clone(), v.clone()
        got, = gfla.spectral_normalize([W], [ui], [vi], impl=impl)
        assert torch.equal(got, want) and torch.equal(ui, lin.weight_u) and torch.equal(vi, lin.weight_v)
    u0 = u.clone()
    got64, = gfla.spectral_normalize([W.double()], [u.double()], [v.double()], 0)
    assert got64.dtype == torch.float64 and torch.equal(u, u0)
    for bad in (dict(power_iterations=-1), dict(eps=0.0), dict(impl="vendor")):
        with pytest.raises(ValueError):
            gfla.spectral_normalize([W], [u], [v], **bad)
    with pytest.raises(ValueError):
        gfla.spectral_normalize([W], [u, u], [v])
    with pytest.raises(ValueError):
        gfla.spectral_normalize([W], [v], [u])


# ---- entry points ----------------------------------------------------------------------------------------------------
def test_status_codes_without_gpu(gfla):
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    assert {"gfla_spectral_norm_fwd_f32", "gfla_spectral_norm_bwd_f32", "gfla_spectral_norm_layout",
            "gfla_spectral_norm_bwd_scratch_floats"} <= set(_lib.extension_symbols()) and _lib.ABI_VERSION == 8
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dims(*pairs):
        flat = [n for pair in pairs for n in pair]
        return ctypes.cast((ctypes.c_int64 * len(flat))(*flat), ctypes.c_void_p), len(pairs)

    good, n = dims((4, 6), (2, 3))
    off, tot = (ctypes.c_int64 * 6)(), (ctypes.c_int64 * 2)()
    po, pt = ctypes.cast(off, ctypes.c_void_p), ctypes.cast(tot, ctypes.c_void_p)
    assert L.gfla_spectral_norm_layout(good, n, po, pt) == 0
    assert list(off) == [0, 0, 6, 24, 10, 13] and list(tot) == [30, 15]
    assert L.gfla_spectral_norm_bwd_scratch_floats(good, n) == 2
    assert L.gfla_spectral_norm_layout(good, n, None, pt) == -1 and L.gfla_spectral_norm_layout(None, n, po, pt) == -1
    fwd, bwd = L.gfla_spectral_norm_fwd_f32, L.gfla_spectral_norm_bwd_f32
    assert fwd(None, good, n, p, p, p, p, 1, 1e-12, None) == -1                 # NULL table
    assert fwd(p, good, n, None, p, p, p, 1, 1e-12, None) == -1                 # NULL outputs
    assert fwd(p, good, n, p, None, p, p, 1, 1e-12, None) == -1
    assert bwd(None, good, n, p, p, p, p, p, None) == -1 and bwd(p, good, n, p, p, p, None, p, None) == -1
    assert fwd(p, good, 0, p, p, p, p, 1, 1e-12, None) == -2                    # n <= 0
    assert fwd(p, good, n, p, p, p, p, -1, 1e-12, None) == -2                   # negative power_iterations
    assert fwd(p, good, n, p, p, p, p, 1, 0.0, None) == -2                      # eps <= 0
    for pairs in (((4, 0),), ((-1, 3),)):                                        # a non-positive R or K
        bad, m = dims(*pairs)
        assert fwd(p, bad, m, p, p, p, p, 1, 1e-12, None) == -2 and bwd(p, bad, m, p, p, p, p, p, None) == -2
        assert L.gfla_spectral_norm_layout(bad, m, po, pt) == -2 and L.gfla_spectral_norm_bwd_scratch_floats(bad, m) == -2
    for pairs in (((2 ** 24 + 1, 1),), ((1, 2 ** 24 + 1),), ((2 ** 16, 2 ** 15),)):   # beyond what the kernels index
        big, m = dims(*pairs)
        assert fwd(p, big, m, p, p, p, p, 1, 1e-12, None) == -3 and bwd(p, big, m, p, p, p, p, p, None) == -3
        assert L.gfla_spectral_norm_layout(big, m, po, pt) == -3
    many, m = dims(*[(1, 1)] * 65536)
    assert fwd(p, many, m, p, p, p, p, 1, 1e-12, None) == -3


# ---- the adversarial term --------------------------------------------------------------------------------------------
def test_adversarial_loss_values(gfla):
    import math
    d = torch.tensor([0.5, 2.0, -1.0, 0.25, -3.0, 1.5, 0.0, -0.5]).reshape(2, 1, 2, 2)
    hinge = gfla.AdversarialLoss("hinge")
    assert hinge(d, True, True).item() == pytest.approx((0.5 + 0 + 2 + 0.75 + 4 + 0 + 1 + 1.5) / 8)
    assert hinge(d, False, True).item() == pytest.approx((1.5 + 3 + 0 + 1.25 + 0 + 2.5 + 1 + 0.5) / 8)
    assert hinge(d, True, False).item() == pytest.approx(-d.sum().item() / 8) == hinge(d, False).item()
    lsgan = gfla.AdversarialLoss("lsgan")
    assert lsgan(d, True).item() == pytest.approx(sum((x - 1.0) ** 2 for x in d.flatten().tolist()) / 8)
    assert lsgan(d, False, True).item() == pytest.approx(sum(x ** 2 for x in d.flatten().tolist()) / 8)
    prob = torch.tensor([0.5, 0.9, 0.1, 0.25, 0.75, 0.6, 0.4, 0.99]).reshape(2, 1, 2, 2)
    nsgan = gfla.AdversarialLoss("nsgan")
    assert nsgan(prob, True).item() == pytest.approx(-sum(math.log(x) for x in prob.flatten().tolist()) / 8, rel=1e-6)
    assert nsgan(prob, False).item() == pytest.approx(-sum(math.log(1 - x) for x in prob.flatten().tolist()) / 8, rel=1e-6)
    smooth = gfla.AdversarialLoss("lsgan", target_real_label=0.9)
    assert smooth(d, True).item() == pytest.approx(sum((x - 0.9) ** 2 for x in d.flatten().tolist()) / 8)
    with pytest.raises(ValueError):
        gfla.AdversarialLoss("wgan")


def test_gan_generator_term_freezes_and_restores(gfla):
    (net_D,), _, images = du.discriminators("cpu", copies=1)
    gfla.fuse_spectral_norm(net_D)
    params = list(net_D.parameters())
    params[0].requires_grad_(False)
    flags = [p.requires_grad for p in params]
    term = gfla.gan_generator_term(net_D, gfla.AdversarialLoss("lsgan"))
    generated = images[0].clone().requires_grad_()
    loss = term(generated, images[1])
    assert [p.requires_grad for p in params] == flags
    loss.backward()
    assert generated.grad is not None and generated.grad.abs().max() > 0 and all(p.grad is None for p in params)

    class Broken(nn.Module):
        def __init__(self):
            super(Broken, self).__init__()
            self.w = nn.Parameter(torch.ones(1))

        def forward(self, x):
            raise RuntimeError("no")
    bad = Broken()
    with pytest.raises(RuntimeError):
        gfla.gan_generator_term(bad, gfla.AdversarialLoss("hinge"))(images[0], images[1])
    assert bad.w.requires_grad                                       # restored when D raises as well


# ---- the reference's discriminators ------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir("/root/reference/model/networks"), reason="reference checkout not present")
def test_install_rewrites_the_reference_discriminators(gfla):
    import subprocess
    import sys
    code = r"""
import sys, types
sys.path.insert(0, %r)
import torch
import global_flow_local_attention_amd as g
sys.modules.setdefault('torchvision', types.ModuleType('torchvision'))
try:
    g.install('/root/reference', train_convs=True)
    raise SystemExit('train_convs alone must raise')
except ValueError:
    pass
bf = g.install('/root/reference', discriminator_convs=True, train_convs=True)
import model.networks.discriminator as d
torch.manual_seed(0)
net = d.ResDiscriminator(ndf=32, img_f=128, layers=4)
convs = [m for m in net.modules() if type(m) is g.SpectralConv]
assert len(convs) == 13 and all(c.grad == 'kernels' for c in convs)
assert max(c.weight_orig[0].numel() * c.weight_orig.size(0) for c in convs) == 128 * 2048
assert bf.ResBlockEncoder.forward._gfla_residual_in_epilogue
assert 'block0.model.3.weight_orig' in net.state_dict() and 'conv.weight_u' in net.state_dict()
plain = bf.ResBlockEncoder.forward.__wrapped__
x = torch.randn(1, 3, 32, 32)
net.eval()
with torch.no_grad():
    want = plain(net.block0, x)
    assert torch.equal(net.block0(x), want)
net.train()
net(x).sum().backward()
assert all(p.grad is not None for p in net.parameters())
patch = d.PatchDiscriminator()
assert [m.geometry for m in patch.modules() if type(m) is g.SpectralConv] == [1, 1, 1, None, None]
assert patch(x).shape == (1, 1, 2, 2)
print('ok')
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]
