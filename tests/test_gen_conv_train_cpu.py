"""The gradients of the generator convolutions without a GPU: grad="kernels" on host tensors is the torch composition, the
keyword is validated, the rewrite keeps keys and Parameters, the new entry points check their arguments before they
launch, and the three adjoint packings (emulated in gen_conv_train_util) reproduce torch's data gradients in float64,
the fold of the reflect case included."""
import ctypes

import pytest
import torch
from torch import nn

import gen_conv_train_util as tu
import gen_conv_util as gu


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("geometry", [gu.S1K3, gu.S2K4, gu.T2K3])
def test_host_tensors_take_the_torch_composition(gfla, geometry):
    x, w, b, add = gu.conv_inputs(geometry, (2, 5, 7, 6, 9), torch.float32, seed=1, with_add=geometry != gu.S2K4)
    results = []
    for grad in ("torch", "kernels"):
        leaves = [t if t is None else t.clone().requires_grad_() for t in (x, w, b, add)]
        kw = dict(pre_slope=0.1, grad=grad)
        if geometry == gu.S1K3:
            y = gfla.conv3x3(leaves[0], leaves[1], leaves[2], padding="reflect", add=leaves[3], **kw)
        elif geometry == gu.S2K4:
            y = gfla.conv4x4_down(leaves[0], leaves[1], leaves[2], **kw)
        else:
            y = gfla.conv_transpose3x3_up(leaves[0], leaves[1], leaves[2], add=leaves[3], **kw)
        y.square().sum().backward()
        results.append([y.detach()] + [t.grad for t in leaves if t is not None])
    assert len(results[0]) == len(results[1]) and all(torch.equal(a, b) for a, b in zip(*results))


def test_an_invalid_grad_raises(gfla):
    x, w, b, _ = gu.conv_inputs(gu.S1K3, (1, 3, 4, 5, 5), torch.float32, seed=2, with_add=False)
    with pytest.raises(ValueError):
        gfla.conv3x3(x, w, b, grad="nonsense")
    with pytest.raises(ValueError):
        gfla.conv4x4_down(x, torch.zeros(4, 3, 4, 4), grad="nonsense")
    with pytest.raises(ValueError):
        gfla.conv_transpose3x3_up(x, torch.zeros(3, 4, 3, 3), grad=None)
    with pytest.raises(ValueError):
        gfla.InferenceConv(nn.Conv2d(3, 16, 3, 1, 1), gu.S1K3, grad="nonsense")
    with pytest.raises(ValueError):
        gfla.fuse_inference_convs(nn.Sequential(nn.Conv2d(3, 16, 3, 1, 1)), grad="nonsense")
    with pytest.raises(ValueError):
        gfla.patch_reference_convs(object(), grad="nonsense")
    assert gfla.InferenceConv(nn.Conv2d(3, 16, 3, 1, 1), gu.S1K3).grad == "torch"            # the default everywhere


def _snapshot(net):
    return list(net.state_dict().keys()), {k: id(p) for k, p in net.named_parameters(remove_duplicate=False)}


def test_rewrite_keeps_keys_and_parameters(gfla):
    torch.manual_seed(0)
    net = tu.ConvGenerator().train()
    x = torch.rand(2, 3, 32, 24)
    keys, ids = _snapshot(net)
    want = net(x)
    want.square().mean().backward()
    grads = {k: p.grad.clone() for k, p in net.named_parameters()}
    net.zero_grad()
    # 3 x 2 + 2 + 3 x 3 + 1 = 18 convolutions of the body, of which the two 3x3 with 8 output channels (enc0, dec2) are
    # head_conv.py's, like the image head
    assert gfla.fuse_inference_convs(net, grad="kernels") == 16
    fused = [m for m in net.modules() if type(m) is gfla.InferenceConv]
    assert _snapshot(net) == (keys, ids) and fused and all(m.grad == "kernels" for m in fused)
    got = net(x)                                              # host tensors: the composition, bit for bit
    got.square().mean().backward()
    assert torch.equal(got, want) and all(torch.equal(p.grad, grads[k]) for k, p in net.named_parameters())


def test_new_entry_points_check_before_they_launch(gfla):
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    UNSUPPORTED = -3
    assert _lib.ABI_VERSION == 8
    # packed bytes of the adjoint: taps x chunks of Cout x padded Cin x 32 bytes; monotone in both channel counts
    for geometry, taps in ((0, 9), (1, 16), (2, 9)):
        for esize in (2, 4):
            ck = 32 // esize
            last = 0
            for cout, cin in ((1, 1), (20, 40), (64, 64), (128, 96), (512, 512)):
                got = L.gfla_gen_conv_grad_packed_bytes(cout, cin, geometry, esize)
                assert got == taps * -(-cout // ck) * -(-cin // 32) * 32 * 32 and got >= last > -1
                last = got
    for args in ((0, 4, 0, 4), (4, -1, 0, 4), (4, 4, 3, 4), (4, 4, -1, 2), (4, 4, 0, 8), (4, 4, 0, 3)):
        assert L.gfla_gen_conv_grad_packed_bytes(*args) == -2, args
    assert L.gfla_gen_conv_grad_packed_bytes(65537, 4, 0, 4) == UNSUPPORTED
    assert L.gfla_gen_conv_grad_packed_bytes(4, 65537, 1, 2) == UNSUPPORTED
    # workspace: positive, and monotone in the three sizes the reduction runs over (B, H, W); the reflect case holds the
    # gradient on the padded domain as well
    ws = L.gfla_gen_conv_bwd_workspace_bytes
    for geometry in (0, 1, 2):
        for esize in (2, 4):
            for cin, cout in ((3, 64), (20, 40), (128, 96), (512, 512)):
                last = 0
                for B, H, W in ((1, 2, 2), (1, 9, 7), (2, 9, 7), (2, 33, 17), (2, 33, 70), (3, 128, 88), (8, 128, 88)):
                    got = ws(B, cin, cout, H, W, geometry, 0, esize)
                    assert got >= last and got > 0, (geometry, esize, cin, cout, B, H, W)
                    last = got
    assert ws(2, 4, 4, 8, 8, 0, 1, 4) >= 2 * 4 * 10 * 10 * 4
    bad_shapes = ((0, 4, 4, 4, 4, 0, 0), (1, 0, 4, 4, 4, 0, 0), (1, 4, -1, 4, 4, 0, 0), (1, 4, 4, 0, 4, 0, 0),
                  (1, 4, 4, 4, 0, 0, 0), (1, 4, 4, 4, 4, 3, 0), (1, 4, 4, 4, 4, -1, 0), (1, 4, 4, 4, 4, 0, 2),
                  (1, 4, 4, 4, 4, 0, -1), (1, 4, 4, 4, 4, 1, 1), (1, 4, 4, 4, 4, 2, 1), (1, 4, 4, 1, 4, 0, 1),
                  (1, 4, 4, 4, 1, 0, 1), (1, 4, 4, 1, 4, 1, 0), (1, 4, 4, 4, 1, 1, 0))
    too_big = ((65536, 4, 4, 4, 4, 0, 0), (1, 65537, 4, 4, 4, 0, 0), (1, 4, 65537, 4, 4, 2, 0),
               (1, 4, 4, 1 << 16, 1 << 15, 0, 0), (1, 4, 4, 1 << 15, 1 << 14, 2, 0))
    for bad in bad_shapes:
        assert ws(*bad, 4) == -2, bad
    assert ws(1, 4, 4, 4, 4, 0, 0, 8) == -2
    for big in too_big + ((65535, 4, 4, 256, 256, 0, 0),):                  # the last: B H W beyond 2^31 - 1
        assert ws(*big, 4) == UNSUPPORTED, big

    # the launching entry points: nothing below reaches a GPU
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n = None
    for sfx in ("f32", "f16", "bf16"):
        data, weight = getattr(L, "gfla_gen_conv_bwd_data_" + sfx), getattr(L, "gfla_gen_conv_bwd_weight_" + sfx)
        pack = getattr(L, "gfla_gen_conv_pack_grad_weights_" + sfx)
        ok = (1, 4, 4, 4, 4, 0, 0, 0, 0.0, n)                  # B, Cin, Cout, H, W, geometry, pad_mode, pre_act, slope
        for nulls in ((n, p, p, p, p), (p, n, p, p, p), (p, p, n, p, p), (p, p, p, n, p)):
            assert data(*nulls, *ok) == -1, (sfx, nulls)
        assert data(p, p, p, p, n, 1, 4, 4, 4, 4, 0, 1, 0, 0.0, n) == -1          # reflect needs the workspace
        for nulls in ((n, p, p, p, p), (p, p, n, n, p), (p, n, p, p, p), (p, p, p, n, n)):
            assert weight(*nulls, *ok) == -1, (sfx, nulls)
        for bad in bad_shapes:
            assert data(p, p, p, p, p, *bad, 0, 0.0, n) == -2, (sfx, bad)
            assert weight(p, p, p, p, p, *bad, 0, 0.0, n) == -2, (sfx, bad)
        for big in too_big:
            assert data(p, p, p, p, p, *big, 0, 0.0, n) == UNSUPPORTED, (sfx, big)
            assert weight(p, p, p, p, p, *big, 0, 0.0, n) == UNSUPPORTED, (sfx, big)
        assert weight(p, p, p, p, p, 65535, 4, 4, 256, 256, 0, 0, 0, 0.0, n) == UNSUPPORTED
        assert pack(n, 0, p, 4, 4, 0, n) == -1 and pack(p, 0, n, 4, 4, 0, n) == -1
        for bad in ((3, 4, 4, 0), (-1, 4, 4, 0), (0, 0, 4, 0), (0, 4, 0, 0), (0, 4, 4, 3), (0, 4, 4, -1)):
            assert pack(p, bad[0], p, *bad[1:], n) == -2, (sfx, bad)
        assert pack(p, 0, p, 65537, 4, 1, n) == UNSUPPORTED
    assert set(_lib.extension_symbols()) >= {"gfla_gen_conv_bwd_data_bf16", "gfla_gen_conv_bwd_weight_f16",
                                             "gfla_gen_conv_pack_grad_weights_f32", "gfla_gen_conv_bwd_workspace_bytes"}


def _grad_a(geometry, a, w, g, reflect):
    a = a.clone().requires_grad_()
    return torch.autograd.grad(gu._conv64(a, w, None, geometry, reflect), a, g)[0]


# (B, Cin, Cout, H, W): channels that are no multiple of either chunk (8, 16) nor of 32; odd maps, maps of two rows
@pytest.mark.parametrize("ck", [8, 16])
@pytest.mark.parametrize("reflect", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 7, 6, 9), (1, 20, 40, 2, 3), (1, 3, 9, 3, 2)])
def test_s1k3_adjoint_packing_reproduces_the_data_gradient(shape, reflect, ck):
    B, Cin, Cout, H, W = shape
    a, w, g = _rand((B, Cin, H, W), 1), _rand((Cout, Cin, 3, 3), 2), _rand((B, Cout, H, W), 3)
    packed = tu.pack_grad_emulated(w, gu.S1K3, ck)
    assert packed.shape == (9, -(-Cout // ck), -(-Cin // 32) * 32, ck) and packed.count_nonzero() == w.numel()
    got = tu.grad_a_from_packed(g, packed, gu.S1K3, Cin, ck, H, W, reflect)
    assert torch.allclose(got, _grad_a(gu.S1K3, a, w, g, reflect), rtol=0, atol=1e-12)


@pytest.mark.parametrize("ck", [8, 16])
@pytest.mark.parametrize("shape", [(2, 5, 7, 6, 8), (1, 20, 40, 33, 17), (1, 3, 4, 2, 2), (1, 9, 33, 3, 7)])
def test_s2k4_adjoint_is_four_phases_of_two_by_two_taps(shape, ck):
    B, Cin, Cout, H, W = shape
    a, w = _rand((B, Cin, H, W), 4), _rand((Cout, Cin, 4, 4), 5)
    g = _rand((B, Cout) + gu.out_size(gu.S2K4, H, W), 6)
    packed = tu.pack_grad_emulated(w, gu.S2K4, ck)
    got = tu.grad_a_from_packed(g, packed, gu.S2K4, Cin, ck, H, W)
    assert got.shape == a.shape and torch.allclose(got, _grad_a(gu.S2K4, a, w, g, False), rtol=0, atol=1e-12)
    per_phase = [[tu.u2k4_tap(t)[1:] for t in range(16) if tu.u2k4_tap(t)[0] == p] for p in range(4)]
    assert [len(p) for p in per_phase] == [4, 4, 4, 4] and all(len(set(p)) == 4 for p in per_phase)


@pytest.mark.parametrize("ck", [8, 16])
@pytest.mark.parametrize("shape", [(2, 5, 7, 3, 4), (1, 20, 40, 1, 1), (1, 9, 33, 5, 2)])
def test_t2k3_adjoint_is_a_strided_convolution_of_the_taps_as_stored(shape, ck):
    B, Cin, Cout, H, W = shape
    a, w, g = _rand((B, Cin, H, W), 7), _rand((Cin, Cout, 3, 3), 8), _rand((B, Cout, 2 * H, 2 * W), 9)
    packed = tu.pack_grad_emulated(w, gu.T2K3, ck)
    got = tu.grad_a_from_packed(g, packed, gu.T2K3, Cin, ck, H, W)
    assert torch.allclose(got, _grad_a(gu.T2K3, a, w, g, False), rtol=0, atol=1e-12)
