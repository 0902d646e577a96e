"""float16 storage on the MI355X: every op in f16 against float64 evaluations on the f16 inputs widened exactly (the CPU
oracle, or this library's float64 path where the CPU would be slow -- that path is itself pinned to the reference's
kernels by test_extractor_attn_f64_gpu.py / test_bench_shapes_gpu.py), plus range behaviour (subnormals, overflow, NaN),
hipGraph replay and the face model's two-stream pair.

Bars, as fractions of the largest reference entry (u = 2^-11, f16's unit roundoff):
  LocalAttnReshape bit-exact; other op outputs and gradients 2^-9; ExtractorAttn forward and feature-map gradients 2^-8,
  parameter gradients 2^-7 (the FC biases at +-8 keep every hidden unit off the LeakyReLU kink; f16-representable
  parameters).  The measured errors are printed (pytest -s)."""
import pytest
import torch
import torch.nn.functional as F

from util import make_flow, rand, randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16
OP_TOL, ATTN_TOL, PARAM_TOL = 2 ** -9, 2 ** -8, 2 ** -7
SLOPE = 0.1
FLOW_KINDS6 = ("zero", "coherent", "wild", "smooth", "integer", "oob")


def rel_err(got, want):
    want = want.detach().double()
    err = (got.detach().double().to(want.device) - want).abs().max().item()
    scale = want.abs().max().item()
    return err / scale if scale > 0 else err


def flow16(kind, B, H, W, seed):
    if kind == "oob":
        f = make_flow("coherent", B, H, W, seed=seed)
        f[:, 0] += 1000.0
        f[:, 1] -= 1000.0
        f[::2, 0] -= 2000.0
        f[::2, 1] += 2000.0
        return f.to(F16)
    return make_flow(kind, B, H, W, seed=seed).to(F16)


# ---------------------------------------------------------------------------------------------------------- the ops
@pytest.mark.parametrize("kind", FLOW_KINDS6)
@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_block_extractor_f16(gfla, oracle, k, kind):
    B, C, Hs, Ws, Hf, Wf = 2, 24, 13, 11, 9, 10
    s = randn((B, C, Hs, Ws), seed=10 + k).to(F16)
    f = flow16(kind, B, Hf, Wf, 20 + k)
    up = randn((B, C, k * Hf, k * Wf), seed=30 + k).to(F16)
    a = [s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()]
    out = gfla.BlockExtractor(k)(*a)
    assert out.dtype == F16
    out.backward(up.to(DEV))
    s64, f64, up64 = s.double(), f.double(), up.double()
    want = oracle.block_extractor_fwd(s64, f64, k)
    gs, gf = oracle.block_extractor_bwd(s64, f64, up64, k)
    errs = {"out": rel_err(out.cpu(), want), "source": rel_err(a[0].grad.cpu(), gs), "flow": rel_err(a[1].grad.cpu(), gf)}
    assert a[0].grad.dtype == a[1].grad.dtype == F16
    print("block_extractor f16 k%d %s: %s" % (k, kind, errs))
    assert max(errs.values()) <= OP_TOL, errs


@pytest.mark.parametrize("B,C,H,W", [(1, 256, 64, 44), (1, 512, 32, 22)])
def test_resample2d_f16_vgg_shapes(gfla, B, C, H, W):
    """Resample2d(4, 1, sigma=2) as PerceptualCorrectness uses it, at the VGG relu3_1 / relu4_1 maps of a 256x176 image."""
    i1 = randn((B, C, H, W), seed=41).to(F16)
    fl = make_flow("smooth", B, H, W, seed=42).to(F16)
    up = randn((B, C, H, W), seed=43).to(F16)
    m = gfla.Resample2d(4, 1, sigma=2)
    a = [i1.to(DEV).requires_grad_(), fl.to(DEV).requires_grad_()]
    out = m(*a)
    assert out.dtype == F16
    out.backward(up.to(DEV))
    r = [x.double().to(DEV).requires_grad_() for x in (i1, fl)]
    want = m(*r)
    want.backward(up.double().to(DEV))
    errs = {"out": rel_err(out, want), "input1": rel_err(a[0].grad, r[0].grad), "flow": rel_err(a[1].grad, r[1].grad)}
    print("resample2d f16 %s: %s" % ((B, C, H, W), errs))
    assert max(errs.values()) <= OP_TOL, errs


@pytest.mark.parametrize("k", [3, 5])
def test_aggregate_f16(gfla, k):
    from global_flow_local_attention_amd import extractor_attn as ea
    B, C, H, W = 2, 32, 20, 14
    s = randn((B, C, H, W), seed=51).to(F16)
    f = make_flow("coherent", B, H, W, seed=52).to(F16)
    lg = (randn((B, k * k, H, W), seed=53) * 2).to(F16)
    up = randn((B, C, H, W), seed=54).to(F16)
    a = [x.to(DEV).requires_grad_() for x in (s, f, lg)]
    out, attn = ea.LocalAttnAggregateFunction.apply(*a, k, True)
    assert out.dtype == attn.dtype == F16
    out.backward(up.to(DEV))
    r = [x.double().to(DEV).requires_grad_() for x in (s, f, lg)]
    want, want_attn = ea.LocalAttnAggregateFunction.apply(*r, k, True)
    want.backward(up.double().to(DEV))
    errs = {"out": rel_err(out, want), "attn": rel_err(attn, want_attn)}
    errs.update({n: rel_err(x.grad, y.grad) for n, x, y in zip(("source", "flow", "logits"), a, r)})
    print("aggregate f16 k%d: %s" % (k, errs))
    assert max(errs.values()) <= OP_TOL, errs


@pytest.mark.parametrize("k", [2, 3, 5])
def test_local_attn_reshape_f16_bit_exact(gfla, k):
    B, H, W = 3, 17, 9
    x = (randn((B, k * k, H, W), seed=60) * 100).to(F16).to(DEV).requires_grad_()
    out = gfla.LocalAttnReshape()(x, k)
    assert torch.equal(out, F.pixel_shuffle(x.detach(), k))
    g = (randn(tuple(out.shape), seed=61) * 100).to(F16).to(DEV)
    out.backward(g)
    assert torch.equal(x.grad, F.pixel_unshuffle(g, k))


@pytest.mark.parametrize("k", [3, 5])
def test_config2_full_size_f16_takes_the_float32_backward(gfla, k):
    """BASELINE configs[1]: one (1, 64, 256, 176) map -- planes beyond the LDS budget of the 16-bit backward kernels.  The
    forward runs in f16, the backward is refused by the _f16 entry point and widened to float32 for that call."""
    B, C, H, W = 1, 64, 256, 176
    s = randn((B, C, H, W), seed=70).to(F16)
    f = make_flow("smooth", B, H, W, seed=71).to(F16)
    up = randn((B, C, k * H, k * W), seed=72).to(F16)
    a = [s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()]
    out = gfla.BlockExtractor(k)(*a)
    out.backward(up.to(DEV))
    r = [x.double().to(DEV).requires_grad_() for x in (s, f)]
    want = gfla.BlockExtractor(k)(*r)
    want.backward(up.double().to(DEV))
    errs = {"out": rel_err(out, want), "source": rel_err(a[0].grad, r[0].grad), "flow": rel_err(a[1].grad, r[1].grad)}
    assert a[0].grad.dtype == a[1].grad.dtype == F16
    print("config2 f16 k%d: %s" % (k, errs))
    assert max(errs.values()) <= OP_TOL, errs


# ------------------------------------------------------------------------------------------------- ExtractorAttn
ATTN_SHAPES = [  # (name, B, C, H, W, k)
    ("face_k3", 8, 256, 32, 32, 3),
    ("face_k5", 8, 128, 64, 64, 5),
    ("bench_k5", 32, 128, 64, 44, 5),
    ("bench_k3", 32, 256, 32, 22, 3),
]


def _attn_module(gfla, C, k, seed):
    torch.manual_seed(seed)
    m = gfla.ExtractorAttn(C, k, torch.nn.LeakyReLU(SLOPE), softmax=True)
    with torch.no_grad():
        conv0, conv1 = m.fully_connect_layer[0], m.fully_connect_layer[2]
        conv0.weight.copy_(randn(tuple(conv0.weight.shape), seed=seed + 1) / (2 * C * k * k) ** 0.5)
        conv0.bias.copy_(torch.where(torch.arange(128) % 2 == 0, 8.0, -8.0) + randn((128,), seed=seed + 2) * 0.1)
        conv1.weight.copy_(randn(tuple(conv1.weight.shape), seed=seed + 3) / 128 ** 0.5 * 0.3)
        conv1.bias.copy_(randn((k * k,), seed=seed + 4) * 0.1)
        for p in m.parameters():
            p.copy_(p.half().float())       # f16-representable parameters
    return m


@pytest.mark.parametrize("name,B,C,H,W,k", ATTN_SHAPES, ids=[s[0] for s in ATTN_SHAPES])
def test_extractor_attn_f16_parity(gfla, name, B, C, H, W, k):
    import copy
    from global_flow_local_attention_amd import _lib
    from global_flow_local_attention_amd import extractor_attn as ea
    m = _attn_module(gfla, C, k, 300 + k).to(DEV)
    ref = copy.deepcopy(m).double()
    s, t = randn((B, C, H, W), seed=310).to(F16), randn((B, C, H, W), seed=311).to(F16)
    f = make_flow("smooth", B, H, W, seed=312).to(F16)
    up = randn((B, C, H, W), seed=313).to(F16)
    old = ea.VENDOR_FALLBACK
    ea.VENDOR_FALLBACK = "error"
    try:
        n_vendor, n_pack = ea.vendor_fallback_calls, _lib.path_count(_lib.PATH_FC_PACK_F16)
        a = [x.to(DEV).requires_grad_() for x in (s, t, f)]
        out = m(*a)
        assert out.dtype == F16
        out.backward(up.to(DEV))
        assert _lib.path_count(_lib.PATH_FC_PACK_F16) == n_pack + 1, "the f16 pack path did not run"
        assert ea.vendor_fallback_calls == n_vendor
    finally:
        ea.VENDOR_FALLBACK = old
    r = [x.double().to(DEV).requires_grad_() for x in (s, t, f)]
    want = ref(*r)
    want.backward(up.double().to(DEV))
    errs = {"out": rel_err(out, want)}
    for n_, x, y in zip(("source", "target", "flow"), a, r):
        assert x.grad.dtype == F16
        errs[n_] = rel_err(x.grad, y.grad)
    perrs = {n_: rel_err(p.grad, q.grad) for (n_, p), (_, q) in zip(m.named_parameters(), ref.named_parameters())}
    print("ExtractorAttn f16 %s: %s %s" % (name, errs, perrs))
    assert max(errs.values()) <= ATTN_TOL, errs
    assert max(perrs.values()) <= PARAM_TOL, perrs


def test_extractor_attn_f16_with_float32_flow_and_mixed_inputs(gfla):
    """f16 features with a float32 flow take the 16-bit path; an f16 source with a float32 target is evaluated in float32
    and handed back in f16."""
    from global_flow_local_attention_amd import _lib
    B, C, H, W, k = 2, 32, 16, 12, 3
    m = _attn_module(gfla, C, k, 400).to(DEV)
    s, t = randn((B, C, H, W), seed=401).to(F16).to(DEV), randn((B, C, H, W), seed=402).to(F16).to(DEV)
    f = make_flow("coherent", B, H, W, seed=403).to(DEV)
    n_pack = _lib.path_count(_lib.PATH_FC_PACK_F16)
    with torch.no_grad():
        a = m(s, t, f)
        assert _lib.path_count(_lib.PATH_FC_PACK_F16) == n_pack + 1
        b = m(s, t, f.half())
        with pytest.warns(UserWarning):
            c = m(s, t.float(), f)
    assert a.dtype == b.dtype == c.dtype == F16
    want = m.double()(s.double(), t.double(), f.double())
    for got in (a, c):
        assert rel_err(got, want) <= ATTN_TOL


# ---------------------------------------------------------------------------------------------------------- range
def test_subnormal_features_are_not_flushed(gfla, oracle):
    B, C, H, W, k = 2, 16, 12, 10, 3
    s = (rand((B, C, H, W), seed=80) * 2 ** -15).to(F16)       # f16 subnormals (below 2^-14)
    assert (s != 0).float().mean().item() > 0.99 and s.abs().max().item() < 2 ** -14
    f = make_flow("coherent", B, H, W, seed=81).to(F16)
    out = gfla.BlockExtractor(k)(s.to(DEV), f.to(DEV))
    want = oracle.block_extractor_fwd(s.double(), f.double(), k)
    assert (out.cpu().double() - want).abs().max().item() <= 2 ** -24           # <= 1 ulp of the subnormal range
    assert (out != 0).sum().item() >= 0.99 * (want != 0).sum().item()          # not flushed to zero
    x = (rand((B, k * k, H, W), seed=82) * 2 ** -15).to(F16).to(DEV)
    assert torch.equal(gfla.LocalAttnReshape()(x, k), F.pixel_shuffle(x, k))


def test_overflow_gives_inf_where_the_float32_result_overflows(gfla):
    """An upstream gradient scaled by 2^16 (a GradScaler's first scale) overflows f16 in the source gradient: +-inf exactly
    where the float32 evaluation, cast to f16, overflows; the finite entries agree."""
    B, C, H, W, k = 2, 16, 12, 10, 3
    s = randn((B, C, H, W), seed=90).to(F16).to(DEV)
    f = make_flow("integer", B, H, W, seed=91).to(F16).to(DEV)
    up = (randn((B, C, k * H, k * W), seed=92) * 2 ** 16 / 8).to(F16).to(DEV)   # finite: |up| < 65504
    assert torch.isfinite(up).all()
    a = s.clone().requires_grad_()
    gfla.BlockExtractor(k)(a, f).backward(up)
    r = s.float().requires_grad_()
    gfla.BlockExtractor(k)(r, f.float()).backward(up.float())
    want = r.grad.half()
    assert torch.isinf(want).any(), "the case does not overflow"
    assert torch.equal(torch.isinf(a.grad), torch.isinf(want))
    assert torch.equal(a.grad[torch.isinf(a.grad)], want[torch.isinf(want)])   # same signs
    fin = torch.isfinite(want)
    assert (a.grad[fin].float() - want[fin].float()).abs().max().item() <= OP_TOL * want[fin].float().abs().max().item()


def test_nan_in_gives_nan_out(gfla):
    B, C, H, W, k = 1, 8, 10, 9, 3
    s = randn((B, C, H, W), seed=95).to(F16)
    s[0, 3, 4, 5] = float("nan")
    f = make_flow("coherent", B, H, W, seed=96).to(F16)
    out = gfla.BlockExtractor(k)(s.to(DEV), f.to(DEV))
    want = gfla.BlockExtractor(k)(s.float().to(DEV), f.float().to(DEV))
    assert torch.isnan(want).any()
    assert torch.equal(torch.isnan(out), torch.isnan(want))
    x = randn((B, k * k, H, W), seed=97).to(F16)
    x[0, 2, 1, 1] = float("nan")
    assert torch.isnan(gfla.LocalAttnReshape()(x.to(DEV), k)).sum().item() == 1


# ------------------------------------------------------------------------------------------- hipGraph and face step
def test_graphed_inference_f16_equals_eager(gfla):
    m = _attn_module(gfla, 32, 3, 500).to(DEV).eval()
    mk = lambda seed: (randn((1, 32, 32, 22), seed=seed).to(F16).to(DEV), randn((1, 32, 32, 22), seed=seed + 1).to(F16).to(DEV),
                       make_flow("coherent", 1, 32, 22, seed=seed + 2).to(F16).to(DEV))
    g = gfla.graphed_inference(m, mk(91))
    for seed in (91, 95):
        inp = mk(seed)
        with torch.no_grad():
            want = m(*inp)
        got = g(*inp)
        assert got.dtype == F16
        assert torch.equal(got, want)


@pytest.mark.parametrize("C,H,W,k", [(32, 16, 12, 3), (16, 24, 20, 5)])
def test_dual_stream_pair_f16_equals_sequential(gfla, C, H, W, k):
    B = 3
    torch.manual_seed(0)
    attn_p = gfla.ExtractorAttn(C, k, torch.nn.LeakyReLU(SLOPE), softmax=True).to(DEV)
    attn_r = gfla.ExtractorAttn(C, k, torch.nn.LeakyReLU(SLOPE), softmax=True).to(DEV)
    t = lambda x: x.to(F16).to(DEV).requires_grad_()
    out, prev, ref = (t(randn((B, C, H, W), seed=10 + i)) for i in range(3))
    fp, fr = t(make_flow("smooth", B, H, W, seed=13)), t(make_flow("coherent", B, H, W, seed=14))
    mp, mr = rand((B, 1, H, W), seed=15).to(F16).to(DEV), rand((B, 1, H, W), seed=16).to(F16).to(DEV)
    args = (out, prev, ref, fp, fr, mp, mr)
    up = randn((B, C, H, W), seed=50).to(F16).to(DEV)
    params = list(attn_p.parameters()) + list(attn_r.parameters())
    results = []
    for dual in (True, False):
        for x in list(args[:5]) + params:
            x.grad = None
        res = gfla.DualStreamAttn(attn_p, attn_r, enabled=dual)(*args)
        assert res.dtype == F16
        res.backward(up)
        torch.cuda.synchronize()
        results.append((res.detach().float(), [x.grad.float() for x in list(args[:5]) + params]))
    (r2, g2), (r1, g1) = results
    assert torch.equal(r2, r1)
    for a, b in zip(g2, g1):
        assert (a - b).abs().max().item() <= 2 ** -9 * max(1e-30, b.abs().max().item())
    # the fused f16 blend equals the op-by-op f16 expression bit for bit
    with torch.no_grad():
        a_p, a_r = attn_p(prev, out, fp), attn_r(ref, out, fr)
        want = (out * (1 - mp) + a_p * mp) + (out * (1 - mr) + a_r * mr)
    assert torch.equal(r1, want.float())
