"""Style and content loss (VGGLoss, StyleLoss, PerceptualLoss, StyleContentLoss, gram_l1) without a GPU: the ABI surface,
the classes on host tensors against tests/golden/style_golden.npz (the reference's own VGGLoss in float64 around a stub
extractor, tests/golden/make_style_golden.py), the formula the kernels of csrc/gram_l1.hip implement against autograd,
and the argument checks.

Bars: 1e-12 relative in float64; in float32 the project's bars: loss within 2e-6 relative,
gradients within 1e-5 of the largest reference entry."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import style_util as su  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "style_golden.npz"))
CASES = ("small", "ragged", "near")
LAYERS = su.CONTENT_LAYERS + su.STYLE_LAYERS
NEW_SYMBOLS = ["gfla_gram_l1_workspace_bytes"] + ["gfla_gram_l1_%s_%s" % (d, s) for d in ("fwd", "bwd")
                                                  for s in ("f32", "f16", "bf16")]
LOSS_BAR = {torch.float64: 1e-12, torch.float32: 2e-6}
GRAD_BAR = {torch.float64: 1e-12, torch.float32: 1e-5}


def _features(case, dtype):
    feats = []
    for side in ("x", "y"):
        feats.append({l: torch.from_numpy(GOLDEN["%s/%s/%s" % (case, side, l)]).to(dtype).requires_grad_() for l in LAYERS})
    return feats


def test_symbols_exported_and_declared(gfla):
    names = gfla.exported_symbols()
    header = open(os.path.join(ROOT, "include", "gfla_hip.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym in names, sym
        assert re.search(r"\b%s\(" % sym, header), sym
    assert "#define GFLA_ABI_VERSION 8" in header
    for name in ("GramL1Function", "gram_l1", "VGGLoss", "StyleLoss", "PerceptualLoss", "StyleContentLoss"):
        assert hasattr(gfla, name), name


def test_golden_file_is_small_and_data_only():
    path = os.path.join(ROOT, "tests", "golden", "style_golden.npz")
    assert os.path.getsize(path) < 100 * 1024
    assert all(GOLDEN[k].dtype.kind == "f" for k in GOLDEN.files)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("case", CASES)
def test_classes_reproduce_the_reference(gfla, case, dtype):
    x, y = _features(case, dtype)
    vgg = su.TableVGG({0: x, 1: y})
    weights = [float(w) for w in GOLDEN[case + "/weights"]]
    want_c, want_s = float(GOLDEN[case + "/content"]), float(GOLDEN[case + "/style"])
    tags = (torch.tensor(0), torch.tensor(1))
    content, style = gfla.VGGLoss(weights, vgg=vgg)(*tags)
    for what, got, want in (("content", content, want_c), ("style", style, want_s)):
        rel = abs(got.item() - want) / abs(want)
        print("%s %s %s: %.12e, relative error %.2e" % (case, str(dtype)[6:], what, got.item(), rel))
        assert got.dtype == dtype and rel <= LOSS_BAR[dtype], (what, got.item(), want)
    (content + style).backward()
    for side, feats in (("gx", x), ("gy", y)):
        for layer in LAYERS:
            want = torch.from_numpy(GOLDEN["%s/%s/%s" % (case, side, layer)])
            err = (feats[layer].grad.double() - want).abs().max().item()
            assert err <= GRAD_BAR[dtype] * want.abs().max().item(), (side, layer, err)
    assert float(gfla.StyleLoss(vgg=vgg)(*tags)) == float(style)
    assert float(gfla.PerceptualLoss(weights, vgg=vgg)(*tags)) == float(content)
    both = gfla.StyleContentLoss(vgg)(*tags)
    unit = gfla.VGGLoss(vgg=vgg)(*tags)
    assert both.dim() == 0 and float(both) == float(unit[1] * 500.0 + unit[0] * 0.5)
    assert float(gfla.StyleContentLoss(vgg, lambda_style=2.0, lambda_content=3.0)(*tags)) == float(unit[1] * 2.0 + unit[0] * 3.0)
    torch_impl = gfla.VGGLoss(weights, vgg=vgg, impl="torch")(*tags)
    assert float(torch_impl[0]) == float(content) and float(torch_impl[1]) == float(style)   # host tensors: one path


@pytest.mark.parametrize("case", CASES)
def test_compute_gram_is_the_references(gfla, case):
    x, _ = _features(case, torch.float64)
    mod = gfla.VGGLoss(vgg=None)
    for layer in su.STYLE_LAYERS:
        assert torch.equal(mod.compute_gram(x[layer]), su.gram64(x[layer]))
        assert torch.equal(gfla.StyleLoss().compute_gram(x[layer]), su.gram64(x[layer]))


@pytest.mark.parametrize("near", [False, True])
@pytest.mark.parametrize("B,C,H,W", [(2, 24, 7, 5), (1, 40, 9, 7), (3, 16, 4, 4)])
def test_kernel_formula_matches_autograd(gfla, B, C, H, W, near):
    """What csrc/gram_l1.hip evaluates, emulated with float32 torch ops: both Grams separately, D = G(x) - G(y),
    loss = mean |D|, d/dx = +g 2/(B C^3 N) S F_x, d/dy = -g 2/(B C^3 N) S F_y with S = sign(D) -- against autograd through
    the composition on the same float32 values, evaluated in float64."""
    x, y = su.make_features(B, C, H, W, torch.float32, seed=C + H, near=near)
    g = 3.5
    fx, fy = x.reshape(B, C, H * W), y.reshape(B, C, H * W)
    d = fx.bmm(fx.transpose(1, 2)) / (H * W * C) - fy.bmm(fy.transpose(1, 2)) / (H * W * C)
    coef = g * 2.0 / (B * C ** 3 * H * W)
    loss, gx, gy = d.abs().mean(), coef * d.sign().bmm(fx), -coef * d.sign().bmm(fy)
    xd, yd = x.double().requires_grad_(), y.double().requires_grad_()
    want = gfla.gram_l1(xd, yd)
    (want * g).backward()
    assert abs(loss.item() - want.item()) <= 2e-6 * max(abs(want.item()), su.gram64(x).abs().mean().item())
    # a float32 D may resolve the sign of an entry within rounding of 0 the other way: compare on the float64 signs
    _, d64, gx64 = su.reference(x, y)
    clear = d64.abs() > 2e-6 * gx64.abs().max()
    assert torch.equal(d.sign()[clear].double(), d64.sign()[clear])
    s = torch.where(clear, d64.sign(), d.sign().double())
    for got, ref, negate, auto in ((gx, x, False, xd.grad), (gy, y, True, yd.grad)):
        formula = su.reference_grad(ref, s, negate) * g
        top = auto.abs().max().item()
        assert (got.reshape(ref.shape).double() - formula).abs().max().item() <= 1e-5 * top
        if bool(clear.all()):
            assert (formula - auto).abs().max().item() <= 1e-12 * top


def test_identical_inputs_give_zero(gfla):
    x, _ = su.make_features(2, 12, 5, 4, torch.float64, seed=1, near=False)
    x.requires_grad_()
    loss = gfla.gram_l1(x, x.detach().clone())
    loss.backward()
    assert loss.item() == 0.0 and not x.grad.any()


def test_argument_errors(gfla):
    x = torch.zeros(1, 4, 3, 3)
    with pytest.raises(ValueError):
        gfla.gram_l1(x, x, impl="hip")
    with pytest.raises(ValueError):
        gfla.VGGLoss(vgg=None, impl="fast")
    with pytest.raises(ValueError):
        gfla.StyleContentLoss(None, impl="fast")
    with pytest.raises(RuntimeError):
        gfla.VGGLoss()(x, x)           # no feature extractor
    with pytest.raises(RuntimeError):
        gfla.StyleLoss()(x, x)
    with pytest.raises(RuntimeError):
        gfla.PerceptualLoss()(x, x)
    with pytest.raises(NotImplementedError):
        gfla.GramL1Function.apply(x, x)          # host tensors: the kernels run on the GPU only
    with pytest.raises(NotImplementedError):
        gfla.GramL1Function.apply(x.half(), x.half())


def test_install_leaves_the_reference_classes_alone_by_default(gfla):
    import inspect
    assert inspect.signature(gfla.install).parameters["vgg"].default is None
