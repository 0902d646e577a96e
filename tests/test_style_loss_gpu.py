"""Gram-difference L1 (the style term of VGGLoss) on the kernels of csrc/gram_l1.hip.  Reference everywhere: the
reference's composition (compute_gram + L1Loss) evaluated on the host in float64 on the same stored values.

Inputs: features relu(1.5 randn + 0.2); "independent": y drawn separately; "near": y = relu(x + 0.01 noise - 0.01).

Forward bars (the project's float32 forward bar, DESIGN.md section 2, applied to what the GEMM computes; the same for
float16 / bfloat16 features, whose products are exact in the float32 accumulators): every entry of D within 2e-6 of the
largest |G(x)| entry; the loss within 2e-6 relative on independent inputs and within 2e-6 mean|G(x)| on near inputs.

Gradient bar: within 1e-5 of the largest reference entry, plus half an ulp of the storage type per entry for 16-bit
outputs: 2^-11 / 2^-8 of the entry, and for float16 never less than 2^-25, half the spacing of its subnormals (a property
of the format: below 2^-14 float16 values are 2^-24 apart).  16-bit gradients are taken as a GradScaler asks for them,
from loss * 2^16.  An entry of D with |D_ref| <= 2e-6 max|G(x)| has a sign the float32 kernel may legitimately resolve
the other way: for exactly those entries the reference S takes the kernel's sign from its saved D; everywhere else the
signs must agree.  Their share of the entries is capped, from the reference alone, at 1e-3 on independent and 1e-2 on near
inputs (measured on the host for these generators and shapes: <= 2.5e-4 and <= 5e-3)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import style_util as su  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRY_BAR, LOSS_BAR, GRAD_BAR = 2e-6, 2e-6, 1e-5
HALF_ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
HALF_SUBNORMAL = {torch.float16: 2.0 ** -25}
MASK_CAP = {False: 1e-3, True: 1e-2}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# relu2_2, relu3_4, relu4_4, relu5_2 of a 256 x 256 and of a 256 x 176 image, then two ragged shapes
VGG_SHAPES = [(2, 128, 128, 128), (2, 256, 64, 64), (2, 512, 32, 32), (2, 512, 16, 16),
              (2, 128, 128, 88), (2, 256, 64, 44), (2, 512, 32, 22), (2, 512, 16, 11)]
SHAPES = VGG_SHAPES + [(1, 40, 9, 7), (3, 96, 5, 5)]


def _run(gfla, x, y, grad_scale=1.0, y_grad=False):
    """kernel path on the device copies of x, y -> (loss, saved D, d/dx, d/dy or None)"""
    xg = x.to(DEV).requires_grad_()
    yg = y.to(DEV).requires_grad_(y_grad)
    loss = gfla.gram_l1(xg, yg)
    diff = loss.grad_fn.saved_tensors[2]
    (loss * grad_scale).backward()
    return loss.detach(), diff, xg.grad, yg.grad


def _check_forward(what, loss, diff, x, y, near):
    want, d_ref, gx = su.reference(x, y)
    top, mean_g = gx.abs().max().item(), gx.abs().mean().item()
    assert loss.dtype == torch.float32 and loss.dim() == 0 and diff.dtype == torch.float32
    assert diff.shape == d_ref.shape
    e_entry = (diff.cpu().double() - d_ref).abs().max().item()
    e_loss = abs(loss.item() - want)
    print("%s %s %s: loss %.9e (reference %.9e), loss error %.2e relative, %.2e of mean|G|; worst D entry %.2e of max|G|"
          % (what, str(x.dtype)[6:], tuple(x.shape), loss.item(), want, e_loss / max(want, 1e-300), e_loss / mean_g,
             e_entry / top))
    assert e_entry <= ENTRY_BAR * top, (what, e_entry, top)
    if near:
        assert e_loss <= LOSS_BAR * mean_g, (what, loss.item(), want)
    else:
        assert e_loss <= LOSS_BAR * abs(want), (what, loss.item(), want)
    return d_ref, gx


def _check_grad(what, got, diff, feat, d_ref, gx, near, grad_scale=1.0, negate=False):
    dt = feat.dtype
    unclear = d_ref.abs() <= ENTRY_BAR * gx.abs().max()
    share = unclear.double().mean().item()
    assert share <= MASK_CAP[near], (what, share)       # from the reference alone
    s_kernel = diff.cpu().double().sign()
    assert bool(((s_kernel == -1) | (s_kernel == 0) | (s_kernel == 1)).all())
    assert torch.equal(s_kernel[~unclear], d_ref.sign()[~unclear]), what
    assert torch.equal(s_kernel, s_kernel.transpose(1, 2)), what
    sign = torch.where(unclear, s_kernel, d_ref.sign())
    want = su.reference_grad(feat, sign, negate) * grad_scale
    top = want.abs().max().item()
    assert got.dtype == dt and got.shape == feat.shape
    err = (got.cpu().double() - want).abs()
    tol = GRAD_BAR * top + (HALF_ULP.get(dt, 0.0) * want.abs()).clamp_min(HALF_SUBNORMAL.get(dt, 0.0))
    print("%s %s %s: gradient error %.2e of the largest entry (%.3e); %.1e of the entries of D within the sign mask"
          % (what, str(dt)[6:], tuple(feat.shape), err.max().item() / max(top, 1e-300), top, share))
    assert bool((err <= tol).all()), (what, (err - tol).max().item(), top)


@pytest.mark.parametrize("near", [False, True], ids=["independent", "near"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_parity_with_float64_composition(gfla, B, C, H, W, dtype, near):
    x, y = su.make_features(B, C, H, W, dtype, seed=C + H + W, near=near)
    scale = 1.0 if dtype == torch.float32 else 2.0 ** 16
    loss, diff, gx_got, _ = _run(gfla, x, y, grad_scale=scale)
    what = "near" if near else "independent"
    d_ref, gx = _check_forward(what, loss, diff, x, y, near)
    _check_grad(what, gx_got, diff, x, d_ref, gx, near, grad_scale=scale)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("B,C,H,W", [(2, 256, 64, 44), (1, 40, 9, 7)])
def test_identical_inputs_give_exactly_zero(gfla, B, C, H, W, dtype):
    x, _ = su.make_features(B, C, H, W, dtype, seed=3, near=False)
    loss, diff, gx_got, gy_got = _run(gfla, x, x.clone(), y_grad=True)
    assert loss.item() == 0.0 and not diff.any()
    assert not gx_got.any() and not gy_got.any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("B,C,H,W", [(2, 512, 32, 22), (2, 128, 128, 88), (3, 96, 5, 5)])
def test_two_calls_are_bit_identical(gfla, B, C, H, W, dtype):
    x, y = su.make_features(B, C, H, W, dtype, seed=9, near=True)
    a = _run(gfla, x, y, grad_scale=2.0 ** 16, y_grad=True)
    b = _run(gfla, x, y, grad_scale=2.0 ** 16, y_grad=True)
    for p, q in zip(a, b):
        assert torch.equal(p, q)


@pytest.mark.parametrize("near", [False, True], ids=["independent", "near"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_target_gradient_and_scaled_backward(gfla, dtype, near):
    """d/dy is the minus form when y requires a gradient; a scaled backward scales both gradients."""
    B, C, H, W = 2, 256, 64, 44
    x, y = su.make_features(B, C, H, W, dtype, seed=21, near=near)
    base = 1.0 if dtype == torch.float32 else 2.0 ** 16
    loss, diff, gx_got, gy_got = _run(gfla, x, y, grad_scale=base, y_grad=True)
    d_ref, gx = _check_forward("both", loss, diff, x, y, near)
    _check_grad("d/dx", gx_got, diff, x, d_ref, gx, near, grad_scale=base)
    _check_grad("d/dy", gy_got, diff, y, d_ref, gx, near, grad_scale=base, negate=True)
    loss2, diff2, gx2, gy2 = _run(gfla, x, y, grad_scale=base * 3.5, y_grad=True)
    assert torch.equal(loss2, loss) and torch.equal(diff2, diff)
    _check_grad("d/dx x3.5", gx2, diff2, x, d_ref, gx, near, grad_scale=base * 3.5)
    _check_grad("d/dy x3.5", gy2, diff2, y, d_ref, gx, near, grad_scale=base * 3.5, negate=True)
    # the target of a training step needs no gradient: none is computed
    assert _run(gfla, x, y, grad_scale=base)[3] is None


def test_function_argument_errors(gfla):
    x = torch.zeros(2, 8, 4, 4, device=DEV)
    with pytest.raises(ValueError):
        gfla.GramL1Function.apply(x, x[:, :4])
    with pytest.raises(ValueError):
        gfla.GramL1Function.apply(x[0, 0], x[0, 0])
    with pytest.raises(TypeError):
        gfla.GramL1Function.apply(x, x.half())
    with pytest.raises(TypeError):
        gfla.GramL1Function.apply(x.double(), x.double())
    with pytest.raises(NotImplementedError):
        gfla.GramL1Function.apply(x.cpu(), x.cpu())
    lib = gfla._lib.lib()
    assert lib.gfla_gram_l1_workspace_bytes(1, 5000, 64) == -3 and lib.gfla_gram_l1_workspace_bytes(0, 8, 64) == -2
    # float64 and mixed dtypes take the composition
    xd = su.make_features(2, 8, 4, 4, torch.float64, seed=2, near=False)
    got = gfla.gram_l1(xd[0].to(DEV), xd[1].to(DEV))
    assert got.dtype == torch.float64 and abs(got.item() - su.reference(*xd)[0]) <= 1e-12 * got.item()
    mixed = gfla.gram_l1(xd[0].to(DEV).float(), xd[1].to(DEV).half().float().half())
    assert torch.isfinite(mixed)


def test_vgg_loss_runs_no_vendor_gemm(gfla, monkeypatch):
    """VGGLoss(vgg=stub, impl="auto") forward and backward at the VGG shapes of a 256 x 176 image with torch's batched
    and plain matrix products made to raise."""
    shapes = dict(zip(su.STYLE_LAYERS, VGG_SHAPES[4:]))
    shapes.update({l: (2, 4 + i, 6, 5) for i, l in enumerate(su.CONTENT_LAYERS)})
    feats = []
    for side in (0, 1):
        table = {}
        for i, (layer, shp) in enumerate(shapes.items()):
            table[layer] = su.make_features(*shp, torch.float32, seed=40 + i, near=False)[side].to(DEV).requires_grad_(side == 0)
        feats.append(table)
    mod = gfla.VGGLoss(vgg=su.TableVGG({0: feats[0], 1: feats[1]}), impl="auto")
    want = sum(su.reference(feats[0][l], feats[1][l])[0] for l in su.STYLE_LAYERS)

    def refuse(*args, **kwargs):
        raise AssertionError("a vendor GEMM was called")

    monkeypatch.setattr(torch, "bmm", refuse)
    monkeypatch.setattr(torch.Tensor, "bmm", refuse)
    monkeypatch.setattr(torch, "matmul", refuse)
    monkeypatch.setattr(torch.Tensor, "matmul", refuse)
    content, style = mod(torch.tensor(0), torch.tensor(1))
    (content + style).backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert abs(style.item() - want) <= LOSS_BAR * want, (style.item(), want)
    assert all(feats[0][l].grad is not None and bool(feats[0][l].grad.any()) for l in shapes)
    mod.impl = "torch"                        # the composition does go through bmm: the patch above would have caught it
    monkeypatch.setattr(torch.Tensor, "bmm", refuse)
    with pytest.raises(AssertionError):
        mod(torch.tensor(0), torch.tensor(1))


@pytest.mark.parametrize("near", [False, True], ids=["independent", "near"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_under_autocast(gfla, dtype, near):
    """Under torch.autocast the kernels still read the stored 16-bit features and meet the float32 bars; the torch
    composition's error on the same features is printed next to it (not asserted: whether it overflows depends on data
    nobody has measured)."""
    x, y = su.make_features(2, 128, 128, 128, dtype, seed=77, near=near)
    xg, yg = x.to(DEV).requires_grad_(), y.to(DEV)
    with torch.autocast("cuda", dtype=dtype):
        loss = gfla.gram_l1(xg, yg)
        composed = gfla.gram_l1(xg, yg, impl="torch")
    diff = loss.grad_fn.saved_tensors[2]
    (loss * 2.0 ** 16).backward()
    d_ref, gx = _check_forward("autocast", loss.detach(), diff, x, y, near)
    _check_grad("autocast", xg.grad, diff, x, d_ref, gx, near, grad_scale=2.0 ** 16)
    want = su.reference(x, y)[0]
    print("autocast %s %s: kernels %.9e, torch composition %.9e (%s), float64 host %.9e: errors %.2e and %.2e relative"
          % (str(dtype)[6:], "near" if near else "independent", loss.item(), composed.item(), composed.dtype, want,
             abs(loss.item() - want) / want, abs(composed.item() - want) / want))


def test_amp_trainer_step_with_style_content_loss(gfla):
    """One TrainerShell(amp="bf16") step with StyleContentLoss on the stand-in network: the term is reported, finite, and
    its gradient reaches the generator (the step's gradients differ from those of the same step without it)."""
    import trainer_util as tu
    from global_flow_local_attention_amd.trainer import TrainerShell
    vgg = su.ConvStubVGG(seed=4).to(DEV)
    batch = tu.make_batch(2, 64, 48)
    grads = []
    for with_style in (False, True):
        base, net = tu.build_shell(DEV, ngf=16, lr=1e-3)
        base.reducer.remove()
        shell = TrainerShell(net, lr=1e-3, correctness=base.correctness, regularization=base.regularization,
                             attn_layer=(2, 3), amp="bf16",
                             style_content_loss=gfla.StyleContentLoss(vgg) if with_style else None)
        losses, g = tu.run_step(shell, net, batch, DEV)[:2]
        grads.append(g)
        if with_style:
            term = losses["style_content_gen"]
            print("amp bf16 step: style_content_gen %.6e" % term)
            assert term == term and abs(term) != float("inf") and term > 0
        else:
            assert "style_content_gen" not in losses
    assert all(bool(torch.isfinite(v).all()) for v in grads[1].values())
    moved = [n for n in grads[1] if not torch.equal(grads[0][n], grads[1][n])]
    assert moved, "the style and content term left every gradient of the generator unchanged"
