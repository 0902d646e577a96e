"""VGG19Features without a GPU: the exported symbols and their argument checks, the reference's state-dict keys and
slicing, the float64 host route against golden values from the reference's own VGG19 class
(tests/golden/make_vgg_golden.py), and the packed-weight index maps of csrc/conv_igemm.h against a direct convolution."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import vgg_util as vu


def test_symbols_and_public_names(gfla):
    from global_flow_local_attention_amd import _lib
    names = set(gfla.exported_symbols())
    want = {"gfla_conv3x3_packed_bytes"}
    for sfx in ("f32", "f16", "bf16"):
        want |= {"gfla_conv3x3_relu_fwd_" + sfx, "gfla_conv3x3_relu_bwd_data_" + sfx, "gfla_conv3x3_pack_weights_" + sfx,
                 "gfla_maxpool2x2_fwd_" + sfx, "gfla_maxpool2x2_bwd_" + sfx}
    assert want <= names
    handle = _lib.lib()
    for name in sorted(want):
        assert hasattr(handle, name), name
    for name in ("VGG19Features", "Conv3x3ReluFunction", "MaxPool2x2Function", "conv3x3_relu", "maxpool2x2"):
        assert hasattr(gfla, name), name
    assert handle.gfla_abi_version() == 8


def test_status_codes(gfla):
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    n = None
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for sfx in ("f32", "f16", "bf16"):
        fwd, bwd = getattr(L, "gfla_conv3x3_relu_fwd_" + sfx), getattr(L, "gfla_conv3x3_relu_bwd_data_" + sfx)
        pack = getattr(L, "gfla_conv3x3_pack_weights_" + sfx)
        pf, pb = getattr(L, "gfla_maxpool2x2_fwd_" + sfx), getattr(L, "gfla_maxpool2x2_bwd_" + sfx)
        assert fwd(n, p, p, p, 1, 3, 4, 5, 5, n) == -1 and fwd(p, n, p, p, 1, 3, 4, 5, 5, n) == -1
        assert fwd(p, p, n, p, 1, 3, 4, 5, 5, n) == -1 and fwd(p, p, p, n, 1, 3, 4, 5, 5, n) == -1
        assert bwd(n, p, p, p, 1, 3, 4, 5, 5, n) == -1 and bwd(p, p, p, n, 1, 3, 4, 5, 5, n) == -1
        assert pack(n, 0, p, 4, 3, 0, n) == -1 and pack(p, 0, n, 4, 3, 0, n) == -1
        assert pf(n, p, 1, 1, 4, 4, n) == -1 and pb(p, p, n, 1, 1, 4, 4, n) == -1
        for bad in ((0, 3, 4, 5, 5), (1, 0, 4, 5, 5), (1, 3, 0, 5, 5), (1, 3, 4, 0, 5), (1, 3, 4, 5, -1)):
            assert fwd(p, p, p, p, *bad, n) == -2 and bwd(p, p, p, p, *bad, n) == -2
        assert pack(p, 0, p, 0, 3, 0, n) == -2 and pack(p, 3, p, 4, 3, 0, n) == -2 and pack(p, 0, p, 4, 3, 2, n) == -2
        assert pf(p, p, 1, 0, 4, 4, n) == -2 and pb(p, p, p, 1, 1, 0, 4, n) == -2
        assert fwd(p, p, p, p, 70000, 3, 4, 5, 5, n) == -3 and fwd(p, p, p, p, 1, 3, 4, 65536, 65536, n) == -3
    assert L.gfla_conv3x3_packed_bytes(0, 3, 0, 4) == -2 and L.gfla_conv3x3_packed_bytes(4, 3, 0, 3) == -2
    assert L.gfla_conv3x3_packed_bytes(1 << 20, 3, 0, 4) == -3
    for cout, cin in ((64, 3), (40, 20), (33, 64)):
        for layout in (0, 1):
            for esize, ck in ((4, 8), (2, 16)):
                nch, mp = vu.packed_dims(cout, cin, layout, ck)
                assert L.gfla_conv3x3_packed_bytes(cout, cin, layout, esize) == 9 * nch * mp * 32


def test_state_dict_keys_and_loading(gfla):
    m = gfla.VGG19Features()
    assert tuple(m.state_dict().keys()) == vu.STATE_KEYS
    assert m.relu1_1[0].weight.shape == (64, 3, 3, 3) and getattr(m.relu5_4, "34").weight.shape == (512, 512, 3, 3)
    assert getattr(m.relu3_1, "10").weight.shape == (256, 128, 3, 3) and len(m.relu3_3) == 0 and len(m.relu3_2) == 4
    assert all(not p.requires_grad for p in m.parameters())
    gold = vu.load_golden()
    narrow = gfla.VGG19Features(widths=vu.GOLDEN_WIDTHS).double()
    res = narrow.load_state_dict(vu.golden_state_dict(gold), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(getattr(narrow.relu3_2, "14").bias, gold["param/relu3_2.14.bias"])
    assert all(not p.requires_grad for p in narrow.parameters())


def test_torchvision_state_dict_round_trip(gfla):
    features = vu.torchvision_features((4, 4, 8, 8, 8), seed=3)
    tv = features.state_dict()                                   # bare "N.weight" keys
    a, b = gfla.VGG19Features(widths=(4, 4, 8, 8, 8)), gfla.VGG19Features(widths=(4, 4, 8, 8, 8))
    a.load_torchvision_state_dict(tv)
    b.load_torchvision_state_dict({"features." + k: v for k, v in tv.items()} | {"classifier.0.weight": torch.zeros(2, 2)})
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    for prefix in vu.PARAM_PREFIXES:
        i = prefix.split(".")[1]
        assert torch.equal(a.state_dict()[prefix + ".weight"], tv[i + ".weight"])
        assert torch.equal(a.state_dict()[prefix + ".bias"], tv[i + ".bias"])
    x = torch.randn(1, 3, 16, 16)
    want = x
    for i in range(36):      # the stack itself, up to relu5_4
        want = features[i](want)
    assert torch.allclose(a(x)["relu5_4"], want, atol=1e-6)
    with pytest.raises(KeyError):
        a.load_torchvision_state_dict({"features.1.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError):
        a.load_torchvision_state_dict({k: v for k, v in tv.items() if not k.startswith("34.")})


@pytest.mark.parametrize("tag", vu.GOLDEN_IMAGES)
def test_host_float64_matches_the_reference_class(gfla, tag):
    gold = vu.load_golden()
    m = gfla.VGG19Features(widths=vu.GOLDEN_WIDTHS).double()
    m.load_state_dict(vu.golden_state_dict(gold), strict=True)
    image = gold[tag + "/image"].clone().requires_grad_()
    out = m(image)
    assert tuple(out.keys()) == vu.LAYERS
    assert out["relu3_3"] is out["relu3_2"]
    total = 0
    for layer in vu.LAYERS:
        want = gold["%s/out/%s" % (tag, layer)]
        assert out[layer].shape == want.shape and out[layer].dtype == torch.float64
        assert (out[layer] - want).abs().max() <= 1e-12 * want.abs().max(), layer
        total = total + (out[layer] * gold["%s/r/%s" % (tag, layer)]).sum()
    total.backward()
    want = gold[tag + "/grad_image"]
    assert (image.grad - want).abs().max() <= 1e-12 * want.abs().max()


def test_impl_values(gfla):
    x, w, b = torch.zeros(1, 3, 4, 4), torch.zeros(2, 3, 3, 3), torch.zeros(2)
    with pytest.raises(ValueError):
        gfla.VGG19Features(impl="fast")
    with pytest.raises(ValueError):
        gfla.conv3x3_relu(x, w, b, impl="fast")
    with pytest.raises(ValueError):
        gfla.maxpool2x2(x, impl="fast")
    m = gfla.VGG19Features(widths=(2, 2, 2, 2, 2))
    with pytest.raises(ValueError):
        m.impl = "fast"
    m.impl = "torch"
    assert m.relu1_1[0].impl == "torch" and getattr(m.relu2_1, "4").impl == "torch"
    # CPU tensors take the composition on either setting
    w, b = torch.randn(2, 3, 3, 3), torch.randn(2)
    x = torch.randn(1, 3, 5, 4)
    assert torch.equal(gfla.conv3x3_relu(x, w, b), F.relu(F.conv2d(x, w, b, padding=1)))
    assert torch.equal(gfla.maxpool2x2(x), F.max_pool2d(x, 2, 2))
    with pytest.raises(NotImplementedError):
        gfla.Conv3x3ReluFunction.apply(x, w, b)
    with pytest.raises(NotImplementedError):
        gfla.MaxPool2x2Function.apply(x)


@pytest.mark.parametrize("cin,cout", [(3, 64), (20, 40), (64, 33)])
@pytest.mark.parametrize("ck", [8, 16])
def test_packing_index_maps(cin, cout, ck):
    g = torch.Generator().manual_seed(cin * 100 + cout)
    w = torch.randn(cout, cin, 3, 3, generator=g).double()
    x = torch.randn(2, cin, 5, 7, generator=g).double()
    fwd = vu.pack_emulated(w, 0, ck)
    assert fwd.shape == (9, -(-cin // ck), -(-cout // 32) * 32, ck)
    got = vu.conv_from_packed(x, fwd, cout, ck)
    want = torch.einsum("omyx,bmhwyx->bohw", w, F.pad(x, (1, 1, 1, 1)).unfold(2, 3, 1).unfold(3, 3, 1))
    assert torch.allclose(got, want, rtol=0, atol=1e-12 * want.abs().max())
    by_k = fwd.permute(0, 2, 1, 3).reshape(9, fwd.shape[2], -1)             # [tap][m][k = chunk * ck + j]
    assert not fwd[:, :, cout:].any() and not by_k[:, :, cin:].any()         # the padding is zero
    # data-gradient layout: the same kernel arithmetic on g gives conv_transpose
    gy = torch.randn(2, cout, 5, 7, generator=g).double()
    bwd = vu.pack_emulated(w, 1, ck)
    assert bwd.shape == (9, -(-cout // ck), -(-cin // 32) * 32, ck)
    got = vu.conv_from_packed(gy, bwd, cin, ck)
    want = F.conv_transpose2d(gy, w, padding=1)
    assert torch.allclose(got, want, rtol=0, atol=1e-12 * want.abs().max())
