"""Non-finite inputs on the GPU: a value that is non-finite in an op's torch composition must not come out finite from the
kernels, and must not spread beyond where the composition puts it (tests/nonfinite_util.py has the rule and the cases,
tests/test_nonfinite_cpu.py checks the case list on the host; DESIGN.md, "Non-finite values")."""
import pytest
import torch

import discriminator_util as du
import nonfinite_util as nu

pytestmark = pytest.mark.gpu
CASES = nu.all_cases()
NAN = float("nan")


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_non_finite_values_go_where_the_composition_puts_them(gfla, case):
    inputs = case.make()
    want = case.oracle(inputs)
    got = case.run(gfla, inputs)
    comp = case.composition(gfla, inputs) if case.composition is not None else None
    nu.check(case, got, want, comp)
    if case.op == "max_cosine_similarity":
        # the index of a NaN maximum is torch.max's: the row of the column's first NaN
        best, index = want["y"].want, want["y"].index
        at = torch.isnan(best)
        assert at.any() and torch.equal(got["index"].long()[at], index[at])


def test_vgg_loss_of_an_image_with_one_nan_pixel_is_nan(gfla):
    """VGGLoss / PerceptualLoss / StyleLoss of a generated image with one NaN pixel are NaN, and the image gradient is
    non-finite wherever the float64 composition's is (VGG19Features(impl="torch") and gram_l1(impl="torch") on the host)."""
    case = nu.vgg_case()
    inputs = case.make()
    vgg = case.module(gfla, inputs)
    other = torch.rand(inputs["image"].shape, generator=torch.Generator().manual_seed(3))
    host = gfla.VGG19Features(widths=nu.vu.GOLDEN_WIDTHS, impl="torch")
    host.load_state_dict({k: inputs["param/" + k] for k in nu.vu.STATE_KEYS}, strict=True)
    xr = inputs["image"].double().requires_grad_()
    content_r, style_r = gfla.VGGLoss(vgg=host.double(), impl="torch")(xr, other.double())
    assert torch.isnan(content_r) and torch.isnan(style_r)
    (content_r + style_r).backward()
    P = ~torch.isfinite(xr.grad)
    assert P[0].any() and not P[1].any()
    x = inputs["image"].to(nu.DEV).requires_grad_()
    content, style = gfla.VGGLoss(vgg=vgg)(x, other.to(nu.DEV))
    assert torch.isnan(content) and torch.isnan(style)
    (content + style).backward()
    bad = ~torch.isfinite(x.grad).cpu()
    print("image gradient: %d non-finite in the composition, %d on the kernels, %d laundered" % (P.sum(), bad.sum(), (P & ~bad).sum()))
    assert not (P & ~bad).any() and not bad[1].any()
    assert torch.isnan(gfla.PerceptualLoss(vgg=vgg)(x.detach(), other.to(nu.DEV)))
    assert torch.isnan(gfla.StyleLoss(vgg=vgg)(x.detach(), other.to(nu.DEV)))


def _module_pair(gfla, C, k, nan_logit):
    from oracle import cpu_modules
    torch.manual_seed(3)
    mod = gfla.ExtractorAttn(C, k, torch.nn.LeakyReLU(0.1), softmax=True)
    ref = cpu_modules.ExtractorAttnCPU(C, k, torch.nn.LeakyReLU(0.1), softmax=True)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(p.half().float())                     # representable in every dtype the cases run in
        if nan_logit:
            mod.fully_connect_layer[2].bias[k] = NAN
    ref.load_state_dict(mod.state_dict())
    return mod.to(nu.DEV), ref.double()


def _unfold_target_forward(ref, source, target, flow):
    """ExtractorAttnCPU.forward with the target's blocks taken by INDEX (replicate-clamped), which is what BlockExtractor
    at a zero flow selects.  The reference samples them bilinearly with weights (1, 0, 0, 0), and its backward multiplies the
    three zero weights with the gradient: 0 x NaN = NaN on a ring one pixel below and right of the k x k neighbourhood.
    The kernels fold the target half into a plain convolution and have no such taps ("Non-finite values")."""
    from oracle.cpu_modules import _BlockExtractorCPU, _LocalAttnReshapeCPU
    k = ref.kernel_size
    H, W = target.shape[2:]
    ys = (torch.arange(H).view(-1, 1) + torch.arange(k).view(1, -1) - k // 2).clamp(0, H - 1).reshape(-1)
    xs = (torch.arange(W).view(-1, 1) + torch.arange(k).view(1, -1) - k // 2).clamp(0, W - 1).reshape(-1)
    block_source = _BlockExtractorCPU.apply(source, flow, k)
    block_target = target[:, :, ys][:, :, :, xs]
    attn = _LocalAttnReshapeCPU.apply(ref.fully_connect_layer(torch.cat((block_target, block_source), 1)), k)
    return torch.nn.functional.avg_pool2d(attn * block_source, k, k)


# the module-level bars of the suite, each against the float64 host module: float32 smoke()'s (1e-4 of max(1, the largest
# entry)); float16 tests/test_f16_gpu.py's ATTN_TOL (2^-8 of the largest entry); bfloat16 tests/test_gpu_parity.py's (2^-8 of
# the largest entry forward, 2^-7 for the gradients, which leave as bfloat16 after float32 accumulation)
def _module_bar(dtype, truth, gradient):
    top = truth[torch.isfinite(truth)].abs().max().item() if torch.isfinite(truth).any() else 0.0
    if dtype == torch.float32:
        return 1e-4 * max(1.0, top)
    return (2.0 ** -7 if gradient and dtype == torch.bfloat16 else 2.0 ** -8) * top


@pytest.mark.parametrize("dname,mode", [("f32", None), ("f32", 4), ("f16", None), ("bf16", None)],
                         ids=["f32-default", "f32-mode4", "f16", "bf16"])
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("what", ["flow-nan", "flow-inf", "flow-nan-last-sample", "logit-nan"])
def test_extractor_attn_module(gfla, what, k, dname, mode):
    """The whole module (FC layers, softmax, aggregation), forward and backward with an upstream gradient that is non-zero
    everywhere, against the float64 host module (oracle.cpu_modules): a NaN / +inf flow entry, and one NaN attention logit
    (through the last layer's bias: that tap's logit is NaN at every position and the softmax turns the whole output NaN,
    in both).  The output and the gradients of source, target, flow and every parameter: no element that is non-finite on
    the host is finite here.  With a poisoned flow, the output, grad_target and grad_flow of the other sample are finite and
    within the suite's module-level bar; grad_source of the other sample is NaN throughout or finite and within it (the one
    documented deviation from batch isolation: DESIGN.md, "Non-finite values").
    The backward kernels that form tap indices from the flow were read with a NaN and an inf in it before this ran
    (DESIGN.md lists them): every address comes out of clampi() or of a float clamp in front of the conversion."""
    from util import make_flow, randn
    dtype = nu.DTYPES[dname]
    B, C, H, W = 2, 16, 12, 10
    mod, ref = _module_pair(gfla, C, k, what == "logit-nan")
    if mode is not None:
        mod.fc_mode = mode
    s, t = randn((B, C, H, W), seed=1).to(dtype), randn((B, C, H, W), seed=2).to(dtype)
    f = make_flow("coherent", B, H, W, seed=3).to(dtype)
    planted = B - 1 if what.endswith("last-sample") else 0
    if what.startswith("flow"):
        f[planted, 1 if what == "flow-inf" else 0, 5, 4] = float("inf") if what == "flow-inf" else NAN
    up = randn((B, C, H, W), seed=4).to(dtype)
    up = up + (up == 0).to(dtype)
    dev = [x.to(nu.DEV).requires_grad_() for x in (s, t, f)]
    host = [x.double().requires_grad_() for x in (s, t, f)]
    out, want = mod(*dev), ref(*host)
    assert out.dtype == dtype
    out.backward(up.to(nu.DEV))
    want.backward(up.double())
    # grad_target: the zero-weight taps of the reference's target blocks are the one place where its NaN set is larger
    # than the composition's arithmetic makes it (see _unfold_target_forward); the set held to is the index form's, a subset
    alt = [x.double().requires_grad_() for x in (s, t, f)]
    want_alt = _unfold_target_forward(ref, *alt)
    assert torch.equal(torch.nan_to_num(want_alt.detach()), torch.nan_to_num(want.detach()))
    (g_t,) = torch.autograd.grad(want_alt, alt[1], up.double())
    assert not (~torch.isfinite(g_t) & torch.isfinite(host[1].grad)).any()
    finite_both = torch.isfinite(g_t) & torch.isfinite(host[1].grad)
    assert torch.allclose(g_t[finite_both], host[1].grad[finite_both], rtol=1e-12, atol=1e-14)
    rows = [("output", out, want.detach(), "isolated"), ("grad target", dev[1].grad, g_t, "isolated"),
            ("grad flow", dev[2].grad, host[2].grad, "isolated"), ("grad source", dev[0].grad, host[0].grad, "whole")]
    rows += [("grad " + n, p.grad, q.grad, None) for (n, p), (_, q) in zip(mod.named_parameters(), ref.named_parameters())]
    assert not torch.isfinite(want).all()
    other = 1 - planted
    for name, got, truth, rule in rows:
        got = got.detach().double().cpu()
        P, nf = ~torch.isfinite(truth), ~torch.isfinite(got)
        print("%s %s k%d %s: |P| %d of %d, laundered %d, non-finite outside P %d" % (what, dname, k, name, P.sum(), P.numel(),
                                                                                       (P & ~nf).sum(), (nf & ~P).sum()))
        assert not (P & ~nf).any(), name
        if what == "logit-nan" or rule is None:
            continue
        assert not P[other].any(), name
        if rule == "whole" and bool(nf[other].all()):
            continue
        assert not nf[other].any(), name
        err = (got[other] - truth[other]).abs().max().item()
        assert err <= _module_bar(dtype, truth[other], name != "output"), (name, err)


@pytest.mark.parametrize("what,route", [("source-nan", "resample2d"), ("target-nan", "resample2d"), ("source-inf", "resample2d"),
                                        ("flow-nan", "bilinear")])
def test_perceptual_correctness_module(gfla, what, route):
    """PerceptualCorrectness.calculate_loss on injected features (max cosine, the warp, the fused loss map, the mean) against
    the float64 host restatement (oracle.cpu_modules.PerceptualCorrectnessCPU): the loss is NaN where the host's is, and no
    gradient entry that is non-finite on the host is finite here; entries that are finite on the host are finite and within
    the 1e-5 (util.assert_close) that test_correctness_loss_vs_reference_golden holds the gradients to.  A NaN flow runs
    through the bilinear warp, which has no host restatement of the whole loss: there the NaN sets that follow from the
    composition are asserted.  With the Resample2d warp the flow stays finite (tests/nonfinite_util.py has Resample2d's
    own NaN-flow cases)."""
    from oracle.cpu_modules import PerceptualCorrectnessCPU
    from util import make_flow
    B, C, H, W = 2, 12, 10, 8
    src, tgt = nu.cosine_features((B, C, H * W), 31, torch.float32).view(B, C, H, W), \
        nu.cosine_features((B, C, H * W), 32, torch.float32).view(B, C, H, W)
    flow = make_flow("coherent", B, H, W, seed=33)
    if what == "flow-nan":
        flow[0, 0, 4, 3] = NAN
    elif what.startswith("source"):
        src[0, 3, 4, 3] = NAN if what == "source-nan" else float("inf")
    else:
        tgt[0, 5, 6, 2] = NAN
    dev = [x.to(nu.DEV).requires_grad_() for x in (src, tgt, flow)]
    mod = gfla.PerceptualCorrectness()
    mod.target_vgg, mod.source_vgg = {"f": dev[1]}, {"f": dev[0]}
    loss = mod.calculate_loss(dev[2], "f", None, use_bilinear_sampling=route == "bilinear")
    loss.backward()
    assert torch.isnan(loss)
    if route == "bilinear":
        # the host restatement of this route needs the kernels' max cosine: only the NaN sets that follow from the
        # composition are asserted -- the loss, the poisoned pixel's flow gradient, and the other sample's finiteness
        assert not torch.isfinite(dev[2].grad[0, :, 4, 3]).any() and torch.isfinite(dev[2].grad[1]).all()
        assert torch.isfinite(dev[0].grad[1]).all() and torch.isfinite(dev[1].grad[1]).all()
        return
    host = [x.double().requires_grad_() for x in (src, tgt, flow)]
    ref = PerceptualCorrectnessCPU()
    ref.target_vgg, ref.source_vgg = {"f": host[1]}, {"f": host[0]}
    want = ref.calculate_loss(host[2], "f")
    want.backward()
    assert torch.isnan(want)
    for name, d, h in zip(("grad source", "grad target", "grad flow"), dev, host):
        got, truth = d.grad.double().cpu(), h.grad
        P, nf = ~torch.isfinite(truth), ~torch.isfinite(got)
        print("%s %s: |P| %d of %d, laundered %d, non-finite outside P %d" % (what, name, P.sum(), P.numel(), (P & ~nf).sum(),
                                                                              (nf & ~P).sum()))
        assert not (P & ~nf).any(), name
        assert not P[1].any() and not nf[1].any(), name
        scale = max(1.0, truth[torch.isfinite(truth)].abs().max().item())
        ok = ~P & ~nf
        assert ((got - truth).abs()[ok] <= 1e-5 * scale).all(), name


def test_spectral_normalize_one_nan_weight_poisons_its_matrix_alone(gfla):
    """Three matrices in one batched call, a NaN in one weight of the middle one: its W_sn, u, v, sigma and grad_w are NaN
    throughout, as torch's hook makes them (F.normalize keeps a NaN norm); the other two are bit-equal to the same call
    without the NaN."""
    shapes = du.MATRICES[1:4]                                   # (32, 27), (7, 80), (64, 512)

    def run(poison):
        rows = [du.matrix_inputs(R, K, seed=40 + i) for i, (R, K) in enumerate(shapes)]
        if poison:
            rows[1][0][3, 41] = NAN
        ws = [r[0].to(nu.DEV).requires_grad_() for r in rows]
        us, vs = [r[1].to(nu.DEV) for r in rows], [r[2].to(nu.DEV) for r in rows]
        outs = gfla.spectral_normalize(ws, us, vs, power_iterations=1)
        assert all(type(o.grad_fn).__name__ == "SpectralNormFunctionBackward" for o in outs)
        sigma = outs[0].grad_fn.sigma.clone()
        torch.autograd.backward(outs, [r[3].to(nu.DEV) for r in rows])
        return rows, [dict(w_sn=o.detach(), u=u, v=v, sigma=sigma[i], grad_w=w.grad) for i, (o, u, v, w) in
                      enumerate(zip(outs, us, vs, ws))]
    rows, bad = run(True)
    _, clean = run(False)
    W, u, v, G = rows[1]
    truth = du.truth64(W, u, v, G, 1)
    for key, got in bad[1].items():
        assert torch.isnan(truth[key]).all(), key               # the oracle: everything of the poisoned matrix is NaN
        assert torch.isnan(got).all(), "%s of the poisoned matrix: %d of %d NaN" % (key, int(torch.isnan(got).sum()), got.numel())
    for i in (0, 2):
        for key in bad[i]:
            assert torch.isfinite(bad[i][key]).all() and torch.equal(bad[i][key], clean[i][key]), (i, key)
