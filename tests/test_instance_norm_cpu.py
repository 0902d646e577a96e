"""Fused InstanceNorm2d + LeakyReLU without a GPU: the host-side launch plan of csrc/instance_norm.hip swept over shapes,
the rewrite of existing networks (fuse_instance_norm_act, install(fuse_instance_norm=True)), the goldens against the
tests' own truth function, the kink clearance of every GPU case, and the error paths."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import instance_norm_util as iu  # noqa: E402

PLANES = [(2, 1), (3, 7), (8, 6), (32, 22), (64, 44), (256, 176), (512, 512), (1, 5000)]


def test_geometry_invariants(gfla):
    """whatever the plan picks fits the hardware and covers the plane; the regimes land where the design says"""
    seen = 0
    for BC in (1, 3, 64, 2048, 16384):
        for H, W in PLANES:
            for esize in (2, 4, 8):
                for backward in (False, True):
                    g = iu.geometry(1, BC, H, W, esize, backward)
                    N = H * W
                    seen += 1
                    assert g["regime"] in (0, 1, 2)
                    assert g["threads"] % 64 == 0 and 64 <= g["threads"] <= 1024, g
                    assert 0 <= g["lds"] <= 160 * 1024
                    assert g["planes_per_wg"] >= 1 and g["threads"] % g["planes_per_wg"] == 0
                    per_plane = g["threads"] // g["planes_per_wg"]          # threads that share one plane's span
                    assert per_plane % 64 == 0
                    assert g["values_per_thread"] * per_plane * g["wgs_per_plane"] >= N, (BC, H, W, esize, g)
                    assert g["values_per_thread"] <= 49                       # 48 values in 16-byte vectors + one edge value
                    if g["regime"] == 0:
                        assert g["wgs_per_plane"] == 1 and per_plane == 64
                        assert g["workgroups"] == -(-BC // g["planes_per_wg"])
                    else:
                        assert g["planes_per_wg"] == 1 and g["workgroups"] == BC * g["wgs_per_plane"]
                        assert (g["wgs_per_plane"] > 1) == (g["regime"] == 2)
                    assert g == iu.geometry(BC, 1, W, H, esize, backward)      # a function of (B C, H W, element size) only
    assert seen == 5 * 8 * 3 * 2
    for esize in (2, 4):
        for BC in (256, 2048, 16384):
            for backward in (False, True):
                assert iu.geometry(1, BC, 256, 176, esize, backward)["regime"] == 1
    for backward in (False, True):
        assert iu.geometry(1, 64, 256, 176, 4, backward)["regime"] == 2             # configs[1]: 64 planes on 256 CUs
        assert iu.geometry(1, 64, 256, 176, 2, backward)["regime"] == 2
        for BC in (1, 64, 16384):
            assert iu.geometry(1, BC, 512, 512, 4, backward)["regime"] == 2
        assert iu.geometry(32, 512, 8, 6, 4, backward)["regime"] == 0
        assert iu.geometry(32, 256, 32, 22, 2, backward)["regime"] == 0
    assert iu.geometry(32, 128, 64, 44, 4)["regime"] == 1                          # the bench plane


def test_geometry_and_workspace_argument_checks(gfla):
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int64 * 7)()
    po = ctypes.cast(out, ctypes.c_void_p)
    assert L.gfla_instance_norm_geometry(1, 1, 4, 4, 4, 0, None) == -1
    assert L.gfla_instance_norm_geometry(1, 1, 1, 1, 4, 0, po) == -2           # one value per plane
    assert L.gfla_instance_norm_geometry(0, 1, 4, 4, 4, 0, po) == -2
    assert L.gfla_instance_norm_geometry(1, 1, 4, 4, 3, 0, po) == -2           # element size
    assert L.gfla_instance_norm_workspace_bytes(1, 1, 1, 1, 4) == -2
    n = None
    assert L.gfla_instance_norm_fwd_f32(n, n, n, n, n, n, n, 1, 1, 4, 4, 1e-5, 0.1, 1, n) == -1
    assert L.gfla_instance_norm_bwd_bf16(n, n, n, n, n, n, n, n, n, n, 1, 1, 4, 4, 0.1, 1, n) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.gfla_instance_norm_fwd_f32(p, n, n, p, p, p, p, 1, 1, 1, 1, 1e-5, 0.1, 1, n) == -2
    assert L.gfla_instance_norm_bwd_f64(p, p, n, n, p, p, p, n, n, p, 2, 0, 4, 4, 0.1, 1, n) == -2
    # room for (s1, s2) of every plane, and for three float64 per segment of a split plane
    for (B, C, H, W, esize) in ((2, 3, 8, 6, 4), (1, 64, 256, 176, 4), (1, 2, 512, 512, 2), (4, 64, 64, 44, 8)):
        g = iu.geometry(B, C, H, W, esize)
        need = 8 * B * C * (2 + (3 * g["wgs_per_plane"] if g["regime"] == 2 else 0))
        assert L.gfla_instance_norm_workspace_bytes(B, C, H, W, esize) >= need


def test_split_plane_query(gfla):
    for esize in (2, 4, 8):
        B, C, H, W = iu.smallest_split_shape(esize)
        assert iu.geometry(B, C, H, W, esize)["regime"] == 2 and iu.geometry(B, C, H - 1, W, esize)["regime"] == 1


@pytest.mark.parametrize("config", sorted(iu.CONFIGS))
def test_truth_function_reproduces_the_goldens(config):
    g = iu.golden(config)
    _, slope = iu.CONFIGS[config]
    if slope is not None:
        assert not iu.near_kink(g["x"], g["weight"], g["bias"]).any()
    got = iu.truth(g["x"], g["weight"], g["bias"], g["up"], iu.EPS, slope)
    for what, a, b in zip(("y", "g_x", "g_weight", "g_bias"), got, (g["y"], g["g_x"], g["g_weight"], g["g_bias"])):
        assert (a is None) == (b is None), what
        if a is not None:
            assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item(), what


def test_kink_clearance_converges_for_every_gpu_case(gfla):
    """the inputs of every GPU case, built here exactly as tests/test_instance_norm_gpu.py builds them"""
    for dtype in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
        esize = torch.empty((), dtype=dtype).element_size()
        for config in ("affine_leaky", "plain_relu"):
            for shape in list(iu.SWEEP_SHAPES) + [iu.smallest_split_shape(esize)]:
                x, w, b, _, _ = iu.make_case(shape, dtype, config, seed=iu.sweep_seed(shape))
                assert not iu.near_kink(x, w, b).any(), (shape, dtype, config)
    for shape, dtype, config, seed, offset, pdt in iu.OTHER_GPU_CASES:
        if shape == "split":
            shape = iu.smallest_split_shape(torch.empty((), dtype=dtype).element_size())
        x, w, b, _, _ = iu.make_case(shape, dtype, config, seed=seed, offset=offset, param_dtype=pdt)
        assert not iu.near_kink(x, w, b).any(), (shape, dtype, config)
        assert abs(x.double().mean().item() - offset) < 1


class _Net(nn.Module):
    """norm -> activation pairs as the reference builds them: ONE activation object passed around"""

    def __init__(self):
        super().__init__()
        act = nn.LeakyReLU(0.1)
        self.act = act
        self.model = nn.Sequential(nn.InstanceNorm2d(4, affine=True), act, nn.Conv2d(4, 6, 3, 1, 1),
                                   nn.InstanceNorm2d(6, affine=True), act, nn.Conv2d(6, 6, 3, 1, 1))
        self.tail = nn.Sequential(nn.InstanceNorm2d(6), nn.ReLU(), nn.Conv2d(6, 5, 1), nn.InstanceNorm2d(5, affine=True))
        self.kept = nn.Sequential(nn.InstanceNorm2d(5, track_running_stats=True), nn.LeakyReLU(0.2), nn.BatchNorm2d(5), nn.ReLU())
        self.lone = nn.InstanceNorm2d(5)          # not in a Sequential: left alone

    def forward(self, x):
        return self.act(self.lone(self.kept(self.tail(self.model(x)))))


def _grads(net, inputs):
    for p in net.parameters():
        p.grad = None
    out = net(*inputs)
    out = out[0] if isinstance(out, tuple) else out
    out.square().sum().backward()
    return out.detach(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}


def _check_rewrite(gfla, net, inputs, pairs, lone=0):
    keys = list(net.state_dict().keys())
    params = dict(net.named_parameters())
    want_out, want_grads = _grads(net, inputs)
    assert gfla.fuse_instance_norm_act(net) == pairs
    assert list(net.state_dict().keys()) == keys
    after = dict(net.named_parameters())
    assert set(after) == set(params) and all(after[n] is params[n] for n in params)
    fused = [m for m in net.modules() if isinstance(m, gfla.InstanceNormAct)]
    assert len(fused) == pairs + lone
    assert sum(m.negative_slope is None for m in fused) == lone
    for seq in (m for m in net.modules() if isinstance(m, nn.Sequential)):
        mods = list(seq)
        for a, b in zip(mods, mods[1:] + [None]):
            if type(a) is nn.InstanceNorm2d and not a.track_running_stats:
                raise AssertionError("an InstanceNorm2d is left in a Sequential")
            if isinstance(a, gfla.InstanceNormAct) and a.negative_slope is not None:
                assert type(b) is nn.Identity
    got_out, got_grads = _grads(net, inputs)          # CPU tensors: the composition route, the same torch calls
    assert torch.equal(got_out, want_out)
    assert set(got_grads) == set(want_grads) and all(torch.equal(got_grads[n], want_grads[n]) for n in want_grads)
    assert gfla.fuse_instance_norm_act(net) == 0     # nothing left to fuse


def test_fuse_a_hand_built_network(gfla):
    torch.manual_seed(0)
    net = _Net()
    shared = net.act
    _check_rewrite(gfla, net, (torch.randn(2, 4, 9, 7),), pairs=3, lone=1)
    assert net.act is shared and type(net.act) is nn.LeakyReLU                 # the shared object itself is untouched
    assert type(net.kept[0]) is nn.InstanceNorm2d and type(net.kept[1]) is nn.LeakyReLU and type(net.kept[3]) is nn.ReLU
    assert type(net.lone) is nn.InstanceNorm2d
    assert net.model[0].negative_slope == 0.1 and net.model[0].affine and net.tail[0].negative_slope == 0.0
    assert net.tail[3].negative_slope is None and net.tail[3].affine and not net.tail[0].affine
    assert net.model[0].eps == 1e-5 and net.model[0].impl == "auto"


def test_fuse_the_stand_in_generator(gfla):
    import warp_generator

    class _NoAttn(nn.Module):          # the attention block runs on the GPU only; the rewrite does not concern it
        def __init__(self, *args, **kwargs):
            super().__init__()

        def forward(self, source, target, flow):
            return target

    torch.manual_seed(1)
    net = warp_generator.WarpGenerator(3, 6, 3, 8, attn_cls=_NoAttn)
    g = torch.Generator().manual_seed(2)
    inputs = (torch.randn(1, 3, 32, 24, generator=g), torch.rand(1, 6, 32, 24, generator=g), torch.rand(1, 6, 32, 24, generator=g))
    _check_rewrite(gfla, net, inputs, pairs=13)       # nine _Down and two _Res of two pairs each; _Up is no Sequential


def test_module_and_function_error_paths(gfla):
    with pytest.raises(ValueError):
        gfla.InstanceNormAct(4, track_running_stats=True)
    with pytest.raises(ValueError):
        gfla.InstanceNormAct(4, impl="hip")
    with pytest.raises(ValueError):
        gfla.instance_norm_act(torch.zeros(1, 2, 3, 3), impl="fast")
    with pytest.raises(ValueError):
        gfla.fuse_instance_norm_act(nn.Sequential(), impl="fast")
    with pytest.raises(ValueError):
        gfla.instance_norm_act(torch.zeros(2, 3, 4))                                     # not (B,C,H,W)
    with pytest.raises(ValueError):
        gfla.instance_norm_act(torch.zeros(1, 2, 3, 3), torch.ones(3), torch.zeros(3))    # parameters of another width
    with pytest.raises(ValueError):
        gfla.InstanceNormAct(4)(torch.zeros(1, 3, 5, 5))
    with pytest.raises(NotImplementedError):
        gfla.InstanceNormActFunction.apply(torch.zeros(1, 2, 3, 3), None, None, 1e-5, 0.1)   # the kernels are GPU only
    m = gfla.InstanceNormAct(3, affine=True, negative_slope=0.1)
    ref = nn.InstanceNorm2d(3, affine=True)
    assert list(m.state_dict().keys()) == list(ref.state_dict().keys()) == ["weight", "bias"]
    assert list(gfla.InstanceNormAct(3).state_dict().keys()) == []
    ref.load_state_dict(m.state_dict())
    x = torch.randn(2, 3, 5, 4)
    assert torch.equal(m(x), nn.functional.leaky_relu(ref(x), 0.1))                       # CPU: the composition


@pytest.mark.skipif(not os.path.isdir("/root/reference/model/networks"), reason="reference checkout not present")
def test_install_fuses_the_unmodified_reference(gfla):
    code = r"""
import sys, types
sys.path.insert(0, %r)
import torch
from torch import nn
import global_flow_local_attention_amd as g
sys.modules.setdefault('torchvision', types.ModuleType('torchvision'))
FUSE = sys.argv[1] == '1'
bf = g.install('/root/reference', fuse_instance_norm=FUSE)
import model.networks.generator as gen
net = gen.PoseGenerator(image_nc=3, structure_nc=18, ngf=64, img_f=512, layers=3, num_blocks=2, use_spect=False,
                        attn_layer=[2, 3], norm='instance', activation='LeakyReLU', extractor_kz={'2': 5, '3': 3})
fused = [m for m in net.modules() if isinstance(m, g.InstanceNormAct)]
left = 0
for seq in (m for m in net.modules() if isinstance(m, nn.Sequential)):
    mods = list(seq)
    left += sum(type(a) is nn.InstanceNorm2d and type(b) in (nn.LeakyReLU, nn.ReLU) for a, b in zip(mods, mods[1:]))
assert (len(fused) >= 1 and left == 0) if FUSE else (len(fused) == 0 and left >= 1), (len(fused), left)
assert all(m.affine and m.negative_slope == 0.1 for m in fused if m.negative_slope is not None)
assert sum(p.numel() for p in net.parameters()) == 14047395
print('keys', ' '.join(net.state_dict().keys()))
print('ok', len(fused))
""" % ROOT
    keys = []
    for flag in ("1", "0"):
        out = subprocess.run([sys.executable, "-c", code, flag], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]
        keys.append([line for line in out.stdout.splitlines() if line.startswith("keys ")][0])
    assert keys[0] == keys[1]
