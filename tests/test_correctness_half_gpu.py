"""Sampling-correctness loss on 16-bit features: the float16 / bfloat16 best-match kernel (16-bit matrix cores), the fused
loss map with a 16-bit target and `PerceptualCorrectness(half_features="native")`.

The reference of every comparison is the float64 host evaluation on the SAME 16-bit-rounded inputs (`x.to(dtype).double()`),
never a GPU kernel of this package.  Forward values are held to the float32 bar of tests/test_correctness_gpu.py (2e-6 under
assert_close): a product of two float16 or two bfloat16 values is exact in the float32 accumulator, so what is left is the
float32 accumulation and the float32 norms that bar was set for.  Gradients stored in 16 bits are compared with the float64
reference rounded to that type at one unit in the last place (2^-10 / 2^-7, relative under assert_close); float32
gradients at the existing 1e-5."""
import pytest
import torch

from oracle.cpu_modules import PerceptualCorrectnessCPU, max_cosine_cpu
from util import assert_close, make_flow, randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}


def features(shape, seed, dtype):
    """post-ReLU-like features (non-negative, a few exact zeros, different norms per position), rounded to `dtype`"""
    x = randn(shape, seed=seed).relu() * (1 + randn(shape[:1] + (1,) + shape[2:], seed=seed + 1).abs())
    return x.to(dtype).contiguous()


def check_best(best, index, src, tgt, tol=2e-6):
    """value against the float64 host bmm/max on the rounded inputs; index by the value it points at (ties may resolve
    either way)"""
    assert best.dtype == torch.float32 and index.dtype == torch.int32
    want, _ = max_cosine_cpu(src.double(), tgt.double())
    e1 = assert_close(best.cpu(), want, tol, "best")
    s = src.double() / (src.double().norm(dim=1, keepdim=True) + 1e-8)
    t = tgt.double() / (tgt.double().norm(dim=1, keepdim=True) + 1e-8)
    picked = torch.gather(s, 2, index.cpu().long().unsqueeze(1).expand(-1, s.size(1), -1))
    e2 = assert_close((picked * t).sum(1), want, tol, "value at index")
    assert int(index.min()) >= 0 and int(index.max()) < src.size(2)
    print("best: max abs err %.3e, value at index: %.3e" % (e1, e2))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,Ns,Nt", [
    (2, 16, 120, 120),      # one ragged tile
    (1, 64, 128, 128),      # exactly one source tile, two channel chunks
    (3, 20, 300, 257),      # C not a multiple of the MFMA K, Nt odd (element-wise staging), ragged both ways
    (2, 7, 130, 5),         # fewer channels than one k step, a handful of targets
    (1, 33, 1, 200),        # a single source position
    (2, 256, 704, 704),     # relu3_1-like channel count, 32x22 positions: the 256-column resident tile at its largest
    (1, 48, 1023, 515),     # Ns odd
    (1, 512, 392, 264),     # relu4_1 channel count: the 128-column resident tile at its largest
    (1, 1100, 200, 136),    # the target tile does not fit the LDS: re-staged in passes of 512 channels
])
def test_max_cosine_half_matches_host_bmm_max(gfla, dtype, B, C, Ns, Nt):
    src, tgt = features((B, C, Ns), 1, dtype), features((B, C, Nt), 2, dtype)
    best, index = gfla.max_cosine_similarity(src.to(DEV), tgt.to(DEV), return_index=True)
    assert best.shape == (B, Nt)
    check_best(best, index, src, tgt)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", [1, 2, 3, 64])
def test_max_cosine_half_source_range_split(gfla, dtype, split):
    """units over ranges of source tiles merge through the packed atomic max (tuning key 5 forces the split)"""
    src, tgt = features((2, 32, 1000), 11, dtype), features((2, 32, 260), 12, dtype)
    with gfla.tuned({gfla.TUNE_SPLIT: split}):
        best, index = gfla.max_cosine_similarity(src.to(DEV), tgt.to(DEV), return_index=True)
    check_best(best, index, src, tgt)


@pytest.mark.parametrize("dtype", DTYPES)
def test_max_cosine_half_mixed_sign_and_zero_vectors(gfla, dtype):
    src, tgt = randn((2, 24, 200), seed=3).to(dtype), randn((2, 24, 150), seed=4).to(dtype)
    src[:, :, 7] = 0          # zero vectors: 0/(0+eps) = 0 similarity, as in the reference
    tgt[:, :, 11] = 0
    best, index = gfla.max_cosine_similarity(src.to(DEV), tgt.to(DEV), return_index=True)
    check_best(best, index, src, tgt)
    assert best[:, 11].abs().max().item() == 0.0
    # all similarities negative: the maximum must not be the zero of a padded row
    neg_src = (-features((1, 16, 130), 5, torch.float32) - 0.1).to(dtype)
    pos_tgt = (features((1, 16, 40), 6, torch.float32) + 0.1).to(dtype)
    best, index = gfla.max_cosine_similarity(neg_src.to(DEV), pos_tgt.to(DEV), return_index=True)
    assert best.max().item() < 0
    check_best(best, index, neg_src, pos_tgt)


@pytest.mark.parametrize("dtype", DTYPES)
def test_max_cosine_half_full_size_properties(gfla, dtype):
    """BASELINE shapes (B=32/GPU, relu3_1 (256, 64x44), relu4_1 (512, 32x22)) on 16-bit-rounded randn: every position
    matches itself when target is a permutation of source (best = 1, index = the permutation)."""
    for B, C, N in ((32, 256, 64 * 44), (32, 512, 32 * 22)):
        g = torch.Generator(device=DEV).manual_seed(N)
        src = torch.randn(B, C, N, device=DEV, generator=g).to(dtype)
        perm = torch.randperm(N, device=DEV, generator=g)
        best, index = gfla.max_cosine_similarity(src, src[:, :, perm].contiguous(), return_index=True)
        err = (best - 1).abs().max().item()
        print("permutation (%d, %d, %d) %s: max |best - 1| = %.3e" % (B, C, N, dtype, err))
        assert best.dtype == torch.float32 and err <= 2e-6
        assert torch.equal(index.long(), perm.unsqueeze(0).expand(B, -1))
        # and a slice of the real thing against the host
        tgt = torch.randn(B, C, N, device=DEV, generator=g).to(dtype)
        best = gfla.max_cosine_similarity(src, tgt)
        want, _ = max_cosine_cpu(src[:2].cpu().double(), tgt[:2, :, :256].cpu().double())
        assert_close(best[:2, :256].cpu(), want, 2e-6, "slice")


@pytest.mark.parametrize("dtype", DTYPES)
def test_max_cosine_half_gradients(gfla, dtype):
    """winning-pairs backward in float32, gradients returned in the features' dtype: against float64 autograd on the
    rounded inputs, rounded to the storage type, at one unit in its last place"""
    src, tgt = features((2, 12, 90), 7, dtype), features((2, 12, 70), 8, dtype)
    up = randn((2, 70), seed=9)
    rs, rt = src.double().requires_grad_(), tgt.double().requires_grad_()
    want, _ = max_cosine_cpu(rs, rt)
    (want * up.double()).sum().backward()
    s, t = src.to(DEV).requires_grad_(), tgt.to(DEV).requires_grad_()
    best = gfla.max_cosine_similarity(s, t)
    assert best.dtype == torch.float32
    (best * up.to(DEV)).sum().backward()
    assert s.grad.dtype == dtype and t.grad.dtype == dtype
    e_s = assert_close(s.grad.cpu(), rs.grad.to(dtype), ULP[dtype], "grad source")
    e_t = assert_close(t.grad.cpu(), rt.grad.to(dtype), ULP[dtype], "grad target")
    print("max_cosine gradients %s: source %.3e, target %.3e" % (dtype, e_s, e_t))
    # only one side requested
    s2 = src.to(DEV).requires_grad_()
    gfla.max_cosine_similarity(s2, tgt.to(DEV)).sum().backward()
    assert s2.grad is not None and s2.grad.dtype == dtype


def test_max_cosine_mixed_dtypes_still_raise(gfla):
    a, b = torch.zeros(1, 8, 16, device=DEV), torch.zeros(1, 8, 16, device=DEV)
    for da, db in ((torch.float16, torch.float32), (torch.float16, torch.bfloat16), (torch.float32, torch.bfloat16)):
        with pytest.raises(TypeError):
            gfla.max_cosine_similarity(a.to(da), b.to(db))
    with pytest.raises(TypeError):
        gfla.CorrectnessMapFunction.apply(a.half(), b.half(), torch.ones(1, 16, device=DEV), 1e-8)   # 16-bit warped
    with pytest.raises(TypeError):
        gfla.CorrectnessMapFunction.apply(a, b.half(), torch.ones(1, 16, device=DEV).half(), 1e-8)   # 16-bit best


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,N", [(2, 12, 70), (1, 64, 64), (3, 7, 129), (2, 256, 704)])
def test_correctness_map_half_target_vs_torch(gfla, dtype, B, C, N):
    """exp(-cosine_similarity(x, t) / (best + eps)) with a float32 warped map x and a 16-bit target t, and its three
    gradients, against torch in float64 on the host on the rounded target.  One warped vector is zero (and with C = 7 a
    few more are by chance).  The target is kept clear of zero vectors by a small offset: the gradient with respect to a
    zero target vector is of order 1 / cosine_similarity's eps = 1e8, beyond float16, so the rounded reference and the
    result are both inf there and compare as nan; float32 targets cover that case in tests/test_correctness_gpu.py."""
    x = features((B, C, N), 21, torch.float32)
    t = (features((B, C, N), 22, torch.float32) + 0.05).to(dtype)
    x[0, :, 3] = 0
    best = (randn((B, N), seed=23).abs() * 0.5 + 0.2).contiguous()
    up = randn((B, N), seed=24)
    ref = [v.double().requires_grad_() for v in (x, t, best)]
    want = torch.exp(-torch.nn.functional.cosine_similarity(ref[0], ref[1]) / (ref[2] + 1e-8))
    (want * up.double()).sum().backward()
    dev = [v.to(DEV).requires_grad_() for v in (x, t, best)]
    got = gfla.CorrectnessMapFunction.apply(dev[0], dev[1], dev[2], 1e-8)
    (got * up.to(DEV)).sum().backward()
    assert got.dtype == torch.float32
    assert_close(got.detach().cpu(), want.detach(), 2e-6, "loss map")
    assert dev[0].grad.dtype == torch.float32 and dev[1].grad.dtype == dtype and dev[2].grad.dtype == torch.float32
    assert_close(dev[0].grad.cpu(), ref[0].grad, 1e-5, "grad warped")
    assert_close(dev[1].grad.cpu(), ref[1].grad.to(dtype), ULP[dtype], "grad target")
    assert_close(dev[2].grad.cpu(), ref[2].grad, 1e-5, "grad best")
    # only some gradients requested
    only = [x.to(DEV).requires_grad_(), t.to(DEV), best.to(DEV)]
    gfla.CorrectnessMapFunction.apply(*only, 1e-8).sum().backward()
    assert only[0].grad is not None and only[1].grad is None


def _layers(dtype):
    """two injected feature layers, (B, C, H, W) -> 16-bit-rounded source and target features"""
    out = {}
    for name, shape, seed in (("relu3_1", (2, 40, 12, 10), 31), ("relu4_1", (2, 72, 6, 5), 41)):
        out[name] = (features(shape, seed, dtype), features(shape, seed + 2, dtype))
    return out


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_loss_native_vs_float64_host(gfla, dtype, masked):
    """PerceptualCorrectness(half_features="native") on injected 16-bit features, float32 flow requiring grad: loss and flow
    gradient against PerceptualCorrectnessCPU in float64 on the rounded features"""
    feats = _layers(dtype)
    mod = gfla.PerceptualCorrectness(half_features="native")
    ref = PerceptualCorrectnessCPU()
    mod.source_vgg = {k: v[0].to(DEV) for k, v in feats.items()}
    mod.target_vgg = {k: v[1].to(DEV) for k, v in feats.items()}
    ref.source_vgg = {k: v[0].double() for k, v in feats.items()}
    ref.target_vgg = {k: v[1].double() for k, v in feats.items()}
    mask = (randn((2, 1, 24, 20), seed=51) > -0.3).float() if masked else None
    for layer, (h, w), seed in (("relu3_1", (12, 10), 61), ("relu4_1", (6, 5), 62)):
        flow = make_flow("coherent", 2, h, w, seed=seed)
        fd, fr = flow.to(DEV).requires_grad_(), flow.double().requires_grad_()
        got = mod.calculate_loss(fd, layer, None if mask is None else mask.to(DEV))
        want = ref.calculate_loss(fr, layer, None if mask is None else mask.double())
        got.backward()
        want.backward()
        assert got.dtype == torch.float32 and fd.grad.dtype == torch.float32
        err = abs(got.item() - want.item())
        print("native loss %s %s masked=%s: |err| %.3e" % (layer, dtype, masked, err))
        assert err <= 2e-6
        assert_close(fd.grad.cpu(), fr.grad, 1e-5, "grad flow")


@pytest.mark.parametrize("dtype", DTYPES)
def test_loss_default_is_the_float32_upcast_bit_for_bit(gfla, dtype):
    """half_features defaults to "float32": the same bits as up-casting features, flow and mask by hand and evaluating the
    float32 loss.  The Resample2d backward sums the flow gradient's partials of several channel groups with float atomics,
    in whatever order they arrive, so two runs of the SAME route differ in the last bits there; tuning keys 6 = 1 (plain
    kernels instead of the planes-in-LDS ones) and 1 = 4096 (one thread walks all channels: one channel group, a plain
    store) select the backward without that freedom, for both routes alike."""
    feats = _layers(dtype)
    mod, plain = gfla.PerceptualCorrectness(), gfla.PerceptualCorrectness()
    assert mod.half_features == "float32"
    mod.source_vgg = {k: v[0].to(DEV) for k, v in feats.items()}
    mod.target_vgg = {k: v[1].to(DEV) for k, v in feats.items()}
    plain.source_vgg = {k: v.float() for k, v in mod.source_vgg.items()}
    plain.target_vgg = {k: v.float() for k, v in mod.target_vgg.items()}
    mask = (randn((2, 1, 24, 20), seed=51) > -0.3).float().to(DEV)
    with gfla.tuned({gfla.TUNE_RS: 1, gfla.TUNE_GLOBAL_CPT: 4096}):
        for layer, (h, w), seed in (("relu3_1", (12, 10), 61), ("relu4_1", (6, 5), 62)):
            for m in (None, mask):
                f1 = make_flow("coherent", 2, h, w, seed=seed).to(DEV).requires_grad_()
                f2 = f1.detach().clone().requires_grad_()
                a = mod.calculate_loss(f1, layer, m)
                b = plain.calculate_loss(f2.float(), layer, None if m is None else m.float())
                a.backward()
                b.backward()
                print("default vs explicit %s: loss %.9g / %.9g, max |grad difference| %.3e"
                      % (layer, a.item(), b.item(), (f1.grad - f2.grad).abs().max().item()))
                assert a.dtype == torch.float32 and torch.equal(a, b)
                assert torch.equal(f1.grad, f2.grad)
    with pytest.raises(ValueError):
        gfla.PerceptualCorrectness(half_features="bfloat16")


def test_amp_steps_with_native_correctness(gfla, monkeypatch):
    """three TrainerShell(amp="fp16") steps (built as tests/test_amp_gpu.py builds them) with the correctness module set to
    "native": the best match sees the float16 features, loss and gradients stay finite, no vendor fallback"""
    import trainer_util as tu
    from global_flow_local_attention_amd import correctness
    from global_flow_local_attention_amd import extractor_attn as ea
    from global_flow_local_attention_amd.trainer import TrainerShell
    base, net = tu.build_shell(DEV, ngf=16, lr=1e-3)
    base.reducer.remove()
    shell = TrainerShell(net, lr=1e-3, correctness=base.correctness, regularization=base.regularization, attn_layer=(2, 3),
                         amp="fp16")
    shell.correctness.half_features = "native"
    seen = []
    inner = correctness.max_cosine_similarity
    monkeypatch.setattr(correctness, "max_cosine_similarity",
                        lambda s, t, *a, **k: (seen.append((s.dtype, t.dtype)), inner(s, t, *a, **k))[1])
    batch = tu.make_batch(2, 64, 48)
    old = ea.VENDOR_FALLBACK
    ea.VENDOR_FALLBACK = "error"
    try:
        n_vendor = ea.vendor_fallback_calls
        for step in range(3):
            skipped = shell.skipped_steps
            losses, grads, before, after = tu.run_step(shell, net, batch, DEV)
            assert all(torch.isfinite(torch.tensor(v)) for v in losses.values()), losses
            if shell.skipped_steps == skipped:   # a step the GradScaler took: every (unscaled) gradient is finite
                assert grads and all(torch.isfinite(g).all() for g in grads.values())
        assert ea.vendor_fallback_calls == n_vendor
    finally:
        ea.VENDOR_FALLBACK = old
    assert len(seen) == 6 and all(d == (torch.float16, torch.float16) for d in seen), seen
    assert shell.skipped_steps < 3
