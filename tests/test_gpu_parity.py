"""Parity of the gfx950 kernels (called through the C ABI) with the CPU oracle, with the real
reference kernels (oracle/_ref, when built) and with the committed golden vectors.

Tolerances: the north-star asks for <= 1e-4 max-abs in fp32 and bit-exact index/reshape work.
We hold fp32 forward ops to 2e-6 (they differ from the oracle only by FMA contraction),
fp64 to 1e-12, gradients to 1e-5 relative to the largest gradient entry (atomic accumulation
order), and the reshape to exact equality.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import FLOW_KINDS, assert_close, make_flow, max_abs, rand, randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

F32_FWD, F64_FWD, F32_GRAD, F64_GRAD = 2e-6, 1e-12, 1e-5, 1e-11


def tol(dtype, grad=False):
    if dtype == torch.float64:
        return F64_GRAD if grad else F64_FWD
    return F32_GRAD if grad else F32_FWD


@pytest.fixture(params=["lds", "global"], autouse=True)
def kernel_variant(request, gfla):
    """Every test runs twice: default dispatch (planes in LDS where they fit) and with the
    global-memory kernels forced (include/gfla_hip.h: enum gfla_tuning_key)."""
    force = 1 if request.param == "global" else 0
    with gfla.tuned({key: force for key in (gfla.TUNE_BE_FWD, gfla.TUNE_BE_BWD, gfla.TUNE_AGG, gfla.TUNE_RS, gfla.TUNE_NO_WINDOWS)}):
        yield request.param


@pytest.fixture(scope="module", autouse=True)
def _native_library_is_loaded(gfla):
    from global_flow_local_attention_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libgfla_hip.so missing on the GPU box"
    _lib.lib()
    loaded = open("/proc/self/maps").read()
    assert "libgfla_hip.so" in loaded


# ------------------------------------------------------------------------------ block_extractor
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", FLOW_KINDS)
@pytest.mark.parametrize("k", [3, 5])
def test_block_extractor_fwd_bwd(gfla, oracle, dtype, kind, k):
    B, C, H, W = 2, 7, 14, 10
    s = randn((B, C, H, W), dtype, seed=1)
    f = make_flow(kind, B, H, W, dtype, seed=2)
    sd, fd = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
    out = gfla.BlockExtractor(k)(sd, fd)
    want = oracle.block_extractor_fwd(s, f, k)
    assert out.shape == want.shape
    assert_close(out.cpu(), want, tol(dtype), "fwd")
    g = randn(tuple(want.shape), dtype, seed=3)
    out.backward(g.to(DEV))
    gs, gf = oracle.block_extractor_bwd(s, f, g, k)
    assert_close(sd.grad.cpu(), gs, tol(dtype, True), "grad_source")
    assert_close(fd.grad.cpu(), gf, tol(dtype, True), "grad_flow")


@pytest.mark.parametrize("k", [1, 2, 4, 6, 7])
def test_block_extractor_other_kernel_sizes(gfla, oracle, k):
    s, f = randn((2, 3, 9, 11), seed=4), make_flow("coherent", 2, 9, 11, seed=5)
    sd, fd = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
    out = gfla.BlockExtractor(k)(sd, fd)
    assert_close(out.cpu(), oracle.block_extractor_fwd(s, f, k), F32_FWD)
    g = randn(tuple(out.shape), seed=6)
    out.backward(g.to(DEV))
    gs, gf = oracle.block_extractor_bwd(s, f, g, k)
    assert_close(sd.grad.cpu(), gs, F32_GRAD)
    assert_close(fd.grad.cpu(), gf, F32_GRAD)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1, 1), (1, 2, 5, 3, 3, 1), (3, 1, 12, 9, 10, 7), (2, 33, 8, 64, 8, 64),
                                   (1, 4, 6, 7, 9, 13)])
def test_block_extractor_ragged_shapes_and_source_flow_mismatch(gfla, oracle, shape):
    # Hs != Hf is legal (external_function.py:62-66); widths that defeat the 16-byte store path
    B, C, Hs, Ws, Hf, Wf = shape
    s, f = randn((B, C, Hs, Ws), seed=7), make_flow("coherent", B, Hf, Wf, seed=8)
    for k in (3, 5):
        out = gfla.BlockExtractor(k)(s.to(DEV), f.to(DEV))
        assert out.shape == (B, C, k * Hf, k * Wf)
        assert_close(out.cpu(), oracle.block_extractor_fwd(s, f, k), F32_FWD, str(shape))


def test_block_extractor_zero_flow_identity_kat(gfla):
    # test_block_extractor.py:46-55 of the reference
    s = randn((4, 6, 14, 10), seed=9).to(DEV)
    out = gfla.BlockExtractor(3)(s, torch.zeros(4, 2, 14, 10, device=DEV))
    assert torch.equal(out[:, :, 3:6, 3:6], s[:, :, 0:3, 0:3])
    assert torch.equal(out[:, :, 1::3, 1::3], s)


def test_block_extractor_grad_skipped_when_not_needed(gfla):
    s = randn((1, 2, 6, 6), seed=10).to(DEV).requires_grad_()
    f = make_flow("coherent", 1, 6, 6, seed=11).to(DEV)  # no grad, like zeros_like(flow) in ExtractorAttn
    gfla.BlockExtractor(3)(s, f).sum().backward()
    assert s.grad is not None and f.grad is None


def test_block_extractor_gradcheck_reference_shapes(gfla):
    # test_block_extractor.py:74-78
    s = torch.rand(4, 6, 14, 10, dtype=torch.float64, device=DEV, requires_grad=True)
    f = (torch.rand(4, 2, 14, 10, dtype=torch.float64, device=DEV) * 1.8).requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b: gfla.BlockExtractorFunction.apply(a, b, 3), (s, f),
                                    eps=1e-6, atol=1e-5, nondet_tol=1e-9)


def test_block_extractor_bf16_forward(gfla, oracle):
    s, f = randn((2, 8, 16, 12), seed=12).bfloat16(), make_flow("coherent", 2, 16, 12, seed=13).bfloat16()
    out = gfla.BlockExtractor(3)(s.to(DEV), f.to(DEV))
    want = oracle.block_extractor_fwd(s.float(), f.float(), 3)  # bf16-rounded inputs through the fp32 oracle
    assert out.dtype == torch.bfloat16
    assert max_abs(out.float().cpu(), want) <= 2 ** -8 * max(1.0, want.abs().max().item())


def _to_unfold(t, k):
    """(B,C,kH,kW) reference layout -> (B, C*k*k, H, W) unfold layout."""
    B, C, kH, kW = t.shape
    H, W = kH // k, kW // k
    return t.view(B, C, H, k, W, k).permute(0, 1, 3, 5, 2, 4).reshape(B, C * k * k, H, W).contiguous()


def _from_unfold(t, k, C):
    B, _, H, W = t.shape
    return t.view(B, C, k, k, H, W).permute(0, 1, 4, 2, 5, 3).reshape(B, C, k * H, k * W).contiguous()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", ["zero", "coherent", "wild", "integer"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_block_extractor_unfold_layout(gfla, oracle, dtype, kind, k):
    B, C, H, W = 2, 7, 13, 9
    s, f = randn((B, C, H, W), dtype, seed=50), make_flow(kind, B, H, W, dtype, seed=51)
    sd, fd = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
    out = gfla.BlockExtractorUnfoldFunction.apply(sd, fd, k)
    want = oracle.block_extractor_fwd(s, f, k)
    assert out.shape == (B, C * k * k, H, W)
    out_bi = gfla.BlockExtractorUnfoldFunction.apply(sd.detach(), fd.detach(), k, True)   # (C*k*k, B, H, W)
    assert torch.equal(out_bi.permute(1, 0, 2, 3), out.detach())
    assert_close(out.cpu(), _to_unfold(want, k), tol(dtype), "unfold fwd")
    # identical samples to the reference-layout entry point
    assert_close(_from_unfold(out.detach(), k, C), gfla.BlockExtractorFunction.apply(sd.detach(), fd.detach(), k), tol(dtype))
    g = randn(tuple(out.shape), dtype, seed=52)
    out.backward(g.to(DEV))
    gs, gf = oracle.block_extractor_bwd(s, f, _from_unfold(g, k, C), k)
    assert_close(sd.grad.cpu(), gs, tol(dtype, True), "unfold grad_source")
    assert_close(fd.grad.cpu(), gf, tol(dtype, True), "unfold grad_flow")
    s2, f2 = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()                          # batch-inner layout
    gfla.BlockExtractorUnfoldFunction.apply(s2, f2, k, True).backward(g.to(DEV).permute(1, 0, 2, 3).contiguous())
    assert_close(s2.grad.cpu(), gs, tol(dtype, True), "unfold(batch-inner) grad_source")
    assert_close(f2.grad.cpu(), gf, tol(dtype, True), "unfold(batch-inner) grad_flow")


def test_unfold_supported_query(gfla):
    from global_flow_local_attention_amd import _lib
    assert _lib.unfold_supported(64, 64, 5, 4) and _lib.unfold_supported(32, 22, 3, 4)
    assert not _lib.unfold_supported(256, 176, 3, 4)      # 180 KB plane: reference layout + global kernels
    assert not _lib.unfold_supported(32, 32, 7, 4)


def test_empty_inputs(gfla):
    # zero-sized batch / channel dims: the reference launches zero blocks; we return empty tensors
    out = gfla.BlockExtractor(3)(torch.zeros(0, 4, 6, 5, device=DEV), torch.zeros(0, 2, 6, 5, device=DEV))
    assert out.shape == (0, 4, 18, 15)
    s = torch.zeros(2, 0, 6, 5, device=DEV, requires_grad=True)
    f = torch.zeros(2, 2, 6, 5, device=DEV, requires_grad=True)
    out = gfla.BlockExtractor(3)(s, f)
    assert out.shape == (2, 0, 18, 15)
    out.sum().backward()
    assert f.grad.abs().sum().item() == 0
    assert gfla.LocalAttnReshape()(torch.zeros(0, 9, 4, 4, device=DEV), 3).shape == (0, 1, 12, 12)
    assert gfla.Resample2d(4, 1, 2)(torch.zeros(0, 3, 4, 4, device=DEV), torch.zeros(0, 2, 4, 4, device=DEV)).shape == (0, 3, 4, 4)


def test_more_than_2_to_31_output_elements(gfla, oracle):
    # The reference indexes with a 32-bit `int index` (block_extractor_kernel.cu:33) and overflows past
    # 2^31 elements; here offsets are 64-bit.  (B,C,k) chosen so the output has 2.31e9 elements (9.2 GB).
    B, C, H, W, k = 256, 128, 64, 44, 5
    assert B * C * k * H * k * W > 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    if free < 14 * 2 ** 30:
        pytest.skip("needs ~11 GB of free HBM")
    s = torch.randn(B, C, H, W, device=DEV)
    f = make_flow("smooth", B, H, W, seed=70).to(DEV)
    out = gfla.BlockExtractor(k)(s, f)
    for b in (0, B // 2, B - 1):   # samples below, across and above the 2^31 boundary
        want = oracle.block_extractor_fwd(s[b:b + 1].cpu(), f[b:b + 1].cpu(), k)
        assert_close(out[b:b + 1].cpu(), want, F32_FWD, "sample %d" % b)
    out0 = gfla.BlockExtractor(k)(s, torch.zeros_like(f))
    assert torch.equal(out0[:, :, k // 2::k, k // 2::k], s)
    del out, out0
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", [3, 5])
def test_bf16_forward_ops(gfla, oracle, k):
    # config 5: bf16 features.  bf16-rounded inputs through the fp32 oracle, 2^-8 relative.
    B, C, H, W = 2, 8, 16, 12
    s = randn((B, C, H, W), seed=71).bfloat16()
    f = make_flow("coherent", B, H, W, seed=72).bfloat16()
    lg = randn((B, k * k, H, W), seed=73).bfloat16()
    sf, ff, lf = s.float(), f.float(), lg.float()
    bs = oracle.block_extractor_fwd(sf, ff, k)

    def close(got, want, what):
        assert got.dtype == torch.bfloat16
        assert max_abs(got.float().cpu(), want) <= 2 ** -7 * max(1.0, want.abs().max().item()), what

    unf = gfla.BlockExtractorUnfoldFunction.apply(s.to(DEV), f.to(DEV), k)
    close(unf, _to_unfold(bs, k), "unfold bf16")
    a = torch.softmax(lf, 1)
    want = F.avg_pool2d(F.pixel_shuffle(a, k) * bs, k, k)
    out, attn = gfla.LocalAttnAggregateFunction.apply(s.to(DEV), f.to(DEV), lg.to(DEV), k, True)
    close(out, want, "aggregate bf16")
    close(attn, a, "attn bf16")
    i2 = torch.cat((ff, torch.full((B, 1, H, W), 2.0)), 1).contiguous()
    rs = gfla.Resample2d(4, 1, 2)(s.to(DEV), f.to(DEV))
    close(rs, oracle.resample2d_fwd(sf, i2, 4, 1), "resample2d bf16")


# --------------------------------------------------------------------------- local_attn_reshape
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_local_attn_reshape_bit_exact(gfla, k, dtype):
    x = randn((3, k * k, 14, 10), seed=14).to(dtype)
    xd = x.to(DEV).requires_grad_()
    out = gfla.LocalAttnReshape()(xd, k)
    assert torch.equal(out.cpu(), F.pixel_shuffle(x, k))
    g = randn(tuple(out.shape), seed=15).to(dtype)
    out.backward(g.to(DEV))
    assert torch.equal(xd.grad.cpu(), F.pixel_unshuffle(g, k))


def test_local_attn_reshape_kat_and_gradcheck(gfla):
    # test_local_attn_reshape.py:29-43 and :66-69
    x = torch.arange(9.0).view(1, 9, 1, 1).expand(4, 9, 14, 10).contiguous().to(DEV)
    out = gfla.LocalAttnReshape()(x, 3)
    assert torch.equal(out[0, 0, :3, :3].cpu(), torch.tensor([[0., 1., 2.], [3., 4., 5.], [6., 7., 8.]]))
    xin = torch.rand(4, 9, 14, 10, dtype=torch.float64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a: gfla.LocalAttnReshapeFunction.apply(a, 3), (xin,), eps=1e-6, atol=1e-6)
    with pytest.raises(AssertionError):  # C != k*k (local_attn_reshape.py:13)
        gfla.LocalAttnReshape()(torch.zeros(1, 8, 4, 4, device=DEV), 3)


# ----------------------------------------------------------------------------------- resample2d
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", ["zero", "coherent", "wild", "smooth"])
@pytest.mark.parametrize("k,d", [(2, 1), (4, 1), (4, 2)])
def test_resample2d_fwd_bwd(gfla, oracle, dtype, kind, k, d):
    B, C, H, W = 2, 6, 11, 9
    i1 = randn((B, C, H, W), dtype, seed=16)
    fl = make_flow(kind, B, H, W, dtype, seed=17)
    sigma = 2.0
    i1d, fld = i1.to(DEV).requires_grad_(), fl.to(DEV).requires_grad_()
    out = gfla.Resample2d(k, d, sigma)(i1d, fld)
    i2 = torch.cat((fl, torch.full((B, 1, H, W), sigma, dtype=dtype)), 1).contiguous()
    want = oracle.resample2d_fwd(i1, i2, k, d)
    assert_close(out.cpu(), want, tol(dtype) * 2, "fwd")
    g = randn(tuple(want.shape), dtype, seed=18)
    out.backward(g.to(DEV))
    g1, g2 = oracle.resample2d_bwd(i1, i2, g, k, d, trunc_compat=True)
    assert_close(i1d.grad.cpu(), g1, tol(dtype, True), "grad_input1 (reference int() quirk)")
    assert_close(fld.grad.cpu(), g2[:, :2], tol(dtype, True) * 4, "grad_flow")


def test_resample2d_function_sigma_channel_and_floor_variant(gfla, oracle):
    from global_flow_local_attention_amd import resample2d as rs
    B, C, H, W = 2, 5, 10, 12
    i1 = randn((B, C, H, W), torch.float64, seed=19)
    i2 = torch.cat((make_flow("wild", B, H, W, torch.float64, seed=20),
                    rand((B, 1, H, W), torch.float64, seed=21) * 3 + 0.3), 1).contiguous()
    i1d, i2d = i1.to(DEV).requires_grad_(), i2.to(DEV).requires_grad_()
    g = randn((B, C, H, W), torch.float64, seed=22)
    out = gfla.Resample2dFunction.apply(i1d, i2d, 4, 1)
    assert_close(out.cpu(), oracle.resample2d_fwd(i1, i2, 4, 1), F64_FWD)
    out.backward(g.to(DEV))
    g1, g2 = oracle.resample2d_bwd(i1, i2, g, 4, 1, trunc_compat=True)
    assert_close(i1d.grad.cpu(), g1, F64_GRAD)
    assert_close(i2d.grad.cpu(), g2, F64_GRAD, "d/d(dx,dy,sigma)")
    # floor variant == true gradient of the forward
    rs.TRUNC_COMPAT = False
    try:
        i1e = i1.to(DEV).requires_grad_()
        gfla.Resample2dFunction.apply(i1e, i2.to(DEV), 4, 1).backward(g.to(DEV))
        g1f, _ = oracle.resample2d_bwd(i1, i2, g, 4, 1, trunc_compat=False)
        assert_close(i1e.grad.cpu(), g1f, F64_GRAD)
    finally:
        rs.TRUNC_COMPAT = True


def test_resample2d_input_larger_than_flow_and_many_channels(gfla, oracle):
    # output takes b,h,w from input2 and d from input1 (resample2d.py:17-19); C large enough to chunk
    i1 = randn((2, 70, 16, 20), seed=23)
    fl = make_flow("coherent", 2, 12, 10, seed=24)
    i1d, fld = i1.to(DEV).requires_grad_(), fl.to(DEV).requires_grad_()
    out = gfla.Resample2d(4, 1, 2)(i1d, fld)
    i2 = torch.cat((fl, torch.full((2, 1, 12, 10), 2.0)), 1).contiguous()
    assert_close(out.cpu(), oracle.resample2d_fwd(i1, i2, 4, 1), 4e-6)
    g = randn(tuple(out.shape), seed=25)
    out.backward(g.to(DEV))
    g1, g2 = oracle.resample2d_bwd(i1, i2, g, 4, 1)
    assert_close(i1d.grad.cpu(), g1, F32_GRAD)
    assert_close(fld.grad.cpu(), g2[:, :2], 1e-4)


# ------------------------------------------------------------- fused softmax + aggregate / ExtractorAttn
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", ["zero", "coherent", "wild", "integer"])
@pytest.mark.parametrize("k", [3, 5])
def test_aggregate_matches_unfused_composition(gfla, oracle, dtype, kind, k):
    B, C, H, W = 2, 9, 12, 10
    s = randn((B, C, H, W), dtype, seed=26)
    f = make_flow(kind, B, H, W, dtype, seed=27)
    lg = randn((B, k * k, H, W), dtype, seed=28) * 2
    sd, fd, ld = (t.to(DEV).requires_grad_() for t in (s, f, lg))
    out, attn = gfla.LocalAttnAggregateFunction.apply(sd, fd, ld, k, True)
    # oracle: the reference chain on the CPU (base_function.py:803-809)
    s64, f64, l64 = s.double().requires_grad_(), f.double().requires_grad_(), lg.double().requires_grad_()
    a = torch.softmax(l64, 1)
    bs = oracle.block_extractor_gather(s64, f64, k)
    ref = F.avg_pool2d(F.pixel_shuffle(a, k) * bs, k, k)
    assert_close(attn.cpu(), a.detach().to(dtype), tol(dtype) * 2, "attn")
    assert_close(out.cpu(), ref.detach().to(dtype), tol(dtype) * 4, "out")
    # and the literal oracle ops give the same forward
    lit = F.avg_pool2d(oracle.local_attn_reshape_fwd(a.detach().contiguous(), k) * oracle.block_extractor_fwd(s.double(), f.double(), k), k, k)
    assert max_abs(lit, ref.detach()) < 1e-12
    g = randn((B, C, H, W), dtype, seed=29)
    out.backward(g.to(DEV))
    ref.backward(g.double())
    assert_close(sd.grad.cpu(), s64.grad.to(dtype), tol(dtype, True), "grad_source")
    assert_close(ld.grad.cpu(), l64.grad.to(dtype), tol(dtype, True), "grad_logits")
    if kind != "integer":  # at integer flows the bilinear kink makes autograd's one-sided choice arbitrary
        assert_close(fd.grad.cpu(), f64.grad.to(dtype), tol(dtype, True) * 4, "grad_flow")


@pytest.mark.parametrize("k,C", [(3, 16), (5, 8), (4, 6)])
@pytest.mark.parametrize("softmax", [True, None])
def test_extractor_attn_fused_equals_unfused_and_oracle(gfla, oracle, k, C, softmax):
    torch.manual_seed(30)
    B, H, W = 2, 10, 8
    m = gfla.ExtractorAttn(C, k, torch.nn.LeakyReLU(0.1), softmax=softmax).to(DEV)
    s, t = randn((B, C, H, W), seed=31), randn((B, C, H, W), seed=32)
    f = make_flow("coherent", B, H, W, seed=33)
    args = [x.to(DEV).requires_grad_() for x in (s, t, f)]
    m.fused = True
    m.unfold_gemm = False  # fused tail, FC on the reference-layout block tensor
    attn_c, out_c = m.hook_attn_param(*args)
    (out_c.square().sum()).backward()
    grads_c = [a.grad.clone() for a in args] + [p.grad.clone() for p in m.parameters()]
    for a in args:
        a.grad = None
    m.zero_grad()
    m.unfold_gemm = True   # extractor writes the GEMM operand, FC = one GEMM ...
    m.fuse_source_backward = False  # ... but the two gradient streams into (source, flow) scatter separately
    attn_s, out_s = m.hook_attn_param(*args)
    (out_s.square().sum()).backward()
    grads_s = [a.grad.clone() for a in args] + [p.grad.clone() for p in m.parameters()]
    for a in args:
        a.grad = None
    m.zero_grad()
    m.fuse_source_backward = True   # default: one scatter pass for both streams
    attn_f, out_f = m.hook_attn_param(*args)
    (out_f.square().sum()).backward()
    grads_f = [a.grad.clone() for a in args] + [p.grad.clone() for p in m.parameters()]
    assert_close(out_c.detach().cpu(), out_f.detach().cpu(), 2e-5, "conv vs GEMM formulation of the FC")
    for gc_, gf_ in zip(grads_c, grads_f):
        assert_close(gc_.cpu(), gf_.cpu(), 2e-4, "conv vs GEMM grads")
    for gs_, gf_ in zip(grads_s, grads_f):
        assert_close(gs_.cpu(), gf_.cpu(), 2e-5, "separate vs fused scatter of the two gradient streams")
    for a in args:
        a.grad = None
    m.zero_grad()
    m.fused = False
    attn_u, out_u = m.hook_attn_param(*args)
    (out_u.square().sum()).backward()
    grads_u = [a.grad.clone() for a in args] + [p.grad.clone() for p in m.parameters()]
    assert_close(out_f.detach().cpu(), out_u.detach().cpu(), 2e-5, "fused vs unfused forward")
    assert_close(attn_f.detach().cpu(), attn_u.detach().cpu(), 2e-5, "attn")
    for gf_, gu_ in zip(grads_f, grads_u):
        assert_close(gf_.cpu(), gu_.cpu(), 2e-4, "fused vs unfused grads")
    for a in args:
        a.grad = None
    m.zero_grad()
    m.fused, m.fuse_fc_tail = True, False   # torch ops for add / LeakyReLU / 1x1 convolution
    attn_t, out_t = m.hook_attn_param(*args)
    (out_t.square().sum()).backward()
    grads_t = [a.grad.clone() for a in args] + [p.grad.clone() for p in m.parameters()]
    m.fuse_fc_tail = True
    assert_close(out_f.detach().cpu(), out_t.detach().cpu(), 2e-5, "fused FC tail vs torch ops")
    for gf_, gt_ in zip(grads_f, grads_t):
        assert_close(gf_.cpu(), gt_.cpu(), 2e-4, "fused FC tail vs torch ops, grads")
    if softmax:  # CPU oracle of the whole block (reference composition with literal ops)
        fc = m.fully_connect_layer
        want = oracle.extractor_attn_fwd(s, t, f, fc[0].weight.detach().cpu(), fc[0].bias.detach().cpu(),
                                         fc[2].weight.detach().cpu(), fc[2].bias.detach().cpu(), k, 0.1)
        assert_close(out_u.detach().cpu(), want, 2e-5, "unfused vs CPU oracle")
        assert_close(out_f.detach().cpu(), want, 2e-5, "fused vs CPU oracle")


# ------------------------------------------------------ planes larger than LDS: row windows + outliers
@pytest.mark.parametrize("kind,scale", [("smooth", 1.0), ("wild", 1.0), ("wild", 6.0)])
@pytest.mark.parametrize("k", [3, 5])
def test_windowed_planes_with_outlier_flows(gfla, oracle, kind, scale, k):
    # 200x120 floats = 96 KB per plane: does not fit the 64 KB LDS budget, so the kernels keep a row
    # window per band of flow rows; flows beyond the window margin (scale 6 -> +-50 px) must take the
    # per-pixel global path and still match.
    B, C, H, W = 1, 3, 200, 120
    s = randn((B, C, H, W), seed=60)
    f = (make_flow(kind, B, H, W, seed=61) * scale).contiguous()
    sd, fd = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
    out = gfla.BlockExtractor(k)(sd, fd)
    assert_close(out.cpu(), oracle.block_extractor_fwd(s, f, k), F32_FWD, "windowed fwd")
    g = randn(tuple(out.shape), seed=62)
    out.backward(g.to(DEV))
    gs, gf = oracle.block_extractor_bwd(s, f, g, k)
    # wild*6 flows clamp thousands of taps onto the same border pixels: both sides accumulate them in
    # fp32 (ours with float atomics on the outlier path), so the bar here is the north-star 1e-4
    assert_close(sd.grad.cpu(), gs, 1e-4, "windowed grad_source")
    assert_close(fd.grad.cpu(), gf, 1e-4, "windowed grad_flow")


@pytest.mark.parametrize("scale", [1.0, 6.0])
def test_windowed_resample2d(gfla, oracle, scale):
    B, C, H, W = 1, 5, 200, 120
    i1 = randn((B, C, H, W), seed=63)
    fl = (make_flow("wild", B, H, W, seed=64) * scale).contiguous()
    i1d, fld = i1.to(DEV).requires_grad_(), fl.to(DEV).requires_grad_()
    out = gfla.Resample2d(4, 1, 2)(i1d, fld)
    i2 = torch.cat((fl, torch.full((B, 1, H, W), 2.0)), 1).contiguous()
    assert_close(out.cpu(), oracle.resample2d_fwd(i1, i2, 4, 1), 4e-6, "windowed resample fwd")
    g = randn(tuple(out.shape), seed=65)
    out.backward(g.to(DEV))
    g1, g2 = oracle.resample2d_bwd(i1, i2, g, 4, 1)
    assert_close(i1d.grad.cpu(), g1, F32_GRAD, "windowed resample grad_input1")
    assert_close(fld.grad.cpu(), g2[:, :2], 1e-4, "windowed resample grad_flow")


@pytest.mark.parametrize("kz", [3, 5])
def test_affine_regularization_loss_collapsed_vs_op_by_op(gfla, kz):
    # external_function.py:31-77 through BlockExtractor/LocalAttnReshape (Hs != Hf, C = 1, constant flow)
    # against the collapsed quadratic form, values and gradients w.r.t. the flow field
    flow = make_flow("coherent", 3, 32, 22, seed=80).to(DEV)
    from oracle.cpu_modules import AffineRegularizationLossOpByOp
    f1, f2 = flow.clone().requires_grad_(), flow.clone().requires_grad_()
    l1 = gfla.AffineRegularizationLoss(kz)(f1)
    # the reference's op-by-op composition (oracle/cpu_modules.py) running on THIS library's GPU ops
    l2 = AffineRegularizationLossOpByOp(kz, gfla.BlockExtractor(kz), gfla.LocalAttnReshape())(f2)
    assert abs(l1.item() - l2.item()) <= 2e-4 * max(1.0, abs(l2.item()))
    l1.backward()
    l2.backward()
    assert_close(f1.grad.cpu(), f2.grad.cpu(), 2e-4, "d loss / d flow")
    multi = gfla.MultiAffineRegularizationLoss({'2': 5, '3': 3})
    fl = [make_flow("coherent", 2, 32, 22, seed=81).to(DEV), make_flow("coherent", 2, 64, 44, seed=82).to(DEV)]
    assert torch.isfinite(multi(fl))


def test_affine_regularization_loss_reference_golden_gpu(gfla):
    """Value and d/d flow against what the reference's own class produced (tests/golden/make_affine_golden.py), for
    the collapsed form and for the op-by-op composition on this library's GPU ops."""
    from oracle.cpu_modules import AffineRegularizationLossOpByOp
    z = np.load(os.path.join(GOLDEN, "affine_golden.npz"))
    for name in sorted({k.split("/")[0] for k in z.files}):
        kz = int(name[2])
        want, want_g = float(z[name + "/loss"]), torch.from_numpy(z[name + "/g_flow"])
        for impl in ("collapsed", "op_by_op"):
            f = torch.from_numpy(z[name + "/flow"]).to(DEV).requires_grad_()
            mod = gfla.AffineRegularizationLoss(kz) if impl == "collapsed" else \
                AffineRegularizationLossOpByOp(kz, gfla.BlockExtractor(kz), gfla.LocalAttnReshape())
            loss = mod(f)
            loss.backward()
            assert abs(loss.item() - want) <= 2e-5 * max(1.0, abs(want)), (name, impl, loss.item(), want)
            assert_close(f.grad.cpu(), want_g, 1e-4, "%s %s d loss / d flow" % (name, impl))


def test_hipgraph_captured_inference_matches_eager(gfla, kernel_variant):
    if kernel_variant != "lds":
        pytest.skip("one variant is enough")
    torch.manual_seed(90)
    m = gfla.ExtractorAttn(32, 3, torch.nn.LeakyReLU(0.1), softmax=True).to(DEV).eval()
    mk = lambda seed: (randn((1, 32, 32, 22), seed=seed).to(DEV), randn((1, 32, 32, 22), seed=seed + 1).to(DEV),
                       make_flow("coherent", 1, 32, 22, seed=seed + 2).to(DEV))
    g = gfla.graphed_inference(m, mk(91))
    for seed in (91, 95, 99):                      # replay with new inputs of the same shape
        inp = mk(seed)
        with torch.no_grad():
            want = m(*inp)
        got = g(*inp)
        assert_close(got, want, 1e-6, "graph replay vs eager")


# ------------------------------------------------------------------------------- BASELINE sizes
@pytest.mark.parametrize("k", [3, 5])
def test_config2_block_extractor_full_size(gfla, oracle, k):
    # BASELINE.json configs[1]: 64 x 256 x 176 fp32 feature map, <= 1e-4 vs reference
    s, f = randn((1, 64, 256, 176), seed=34), make_flow("smooth", 1, 256, 176, seed=35)
    sd, fd = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
    out = gfla.BlockExtractor(k)(sd, fd)
    err = assert_close(out.cpu(), oracle.block_extractor_fwd(s, f, k), F32_FWD, "config2 fwd")
    assert err <= 1e-4
    g = randn(tuple(out.shape), seed=36)
    out.backward(g.to(DEV))
    gs, gf = oracle.block_extractor_bwd(s, f, g, k)
    assert_close(sd.grad.cpu(), gs, 1e-4, "config2 grad_source")
    assert_close(fd.grad.cpu(), gf, 1e-4, "config2 grad_flow")


def test_config2_resample2d_full_size(gfla, oracle):
    i1, fl = randn((1, 64, 256, 176), seed=37), make_flow("smooth", 1, 256, 176, seed=38)
    i1d, fld = i1.to(DEV).requires_grad_(), fl.to(DEV).requires_grad_()
    out = gfla.Resample2d(4, 1, 2)(i1d, fld)
    i2 = torch.cat((fl, torch.full((1, 1, 256, 176), 2.0)), 1).contiguous()
    err = assert_close(out.cpu(), oracle.resample2d_fwd(i1, i2, 4, 1), 4e-6, "config2 resample fwd")
    assert err <= 1e-4
    g = randn(tuple(out.shape), seed=39)
    out.backward(g.to(DEV))
    g1, g2 = oracle.resample2d_bwd(i1, i2, g, 4, 1)
    assert_close(i1d.grad.cpu(), g1, 1e-4)
    assert_close(fld.grad.cpu(), g2[:, :2], 1e-4)


def test_config3_size_properties(gfla, oracle):
    # B=32 PoseGenerator attention-layer shapes: too big to ship back whole, so check size-
    # independent properties plus two full samples against the oracle.
    for (C, H, W, k) in ((256, 32, 32, 3), (128, 64, 64, 5)):
        B = 32
        s = torch.randn(B, C, H, W, device=DEV)
        z = torch.zeros(B, 2, H, W, device=DEV)
        out = gfla.BlockExtractor(k)(s, z)
        assert torch.equal(out[:, :, k // 2::k, k // 2::k], s)             # zero flow: centre tap = identity
        f = make_flow("smooth", B, H, W, seed=40).to(DEV)
        o1 = gfla.BlockExtractor(k)(s, f)
        o2 = gfla.BlockExtractor(k)(2.5 * s, f)
        assert max_abs(o2, 2.5 * o1) <= 1e-5 * o1.abs().max().item()         # linear in source
        for b in (0, B - 1):
            want = oracle.block_extractor_fwd(s[b:b + 1].cpu(), f[b:b + 1].cpu(), k)
            assert_close(o1[b:b + 1].cpu(), want, F32_FWD, "config3 sample %d" % b)
        # uniform attention (a = 1/k^2) + zero flow = k x k box filter with replicate padding, then
        # avg_pool2d divides by k^2 once more (base_function.py:809)
        lg = torch.zeros(B, k * k, H, W, device=DEV)
        agg, attn = gfla.LocalAttnAggregateFunction.apply(s, z, lg, k, True)
        box = F.avg_pool2d(F.pad(s, (k // 2,) * 4, mode="replicate"), k, 1) / (k * k)
        assert max_abs(agg, box) <= 2e-6 * max(1.0, box.abs().max().item())
        assert torch.allclose(attn.sum(1), torch.ones(B, H, W, device=DEV), atol=1e-6)
        del out, o1, o2
        torch.cuda.empty_cache()


# ----------------------------------------------------------------- real reference kernels + goldens
def _ref():
    from oracle import ref_ext
    if not ref_ext.available():
        pytest.skip("oracle/_ref not built (needs /root/reference at build time)")
    return ref_ext


def test_against_real_reference_kernels(gfla, oracle):
    ref = _ref()
    for k in (3, 5):
        s, f = randn((2, 6, 14, 10), seed=41).to(DEV), make_flow("wild", 2, 14, 10, seed=42).to(DEV)
        r = ref.block_extractor_fwd(s, f, k)
        assert_close(gfla.BlockExtractorFunction.apply(s, f, k), r, F32_FWD, "vs reference kernel")
        assert_close(oracle.block_extractor_fwd(s.cpu(), f.cpu(), k), r.cpu(), F32_FWD, "oracle vs reference kernel")
        g = randn(tuple(r.shape), seed=43).to(DEV)
        rgs, rgf = ref.block_extractor_bwd(s, f, g, k)
        ogs, ogf = oracle.block_extractor_bwd(s.cpu(), f.cpu(), g.cpu(), k)
        assert_close(ogs, rgs.cpu(), F32_GRAD)
        assert_close(ogf, rgf.cpu(), F32_GRAD)
    x = randn((2, 9, 7, 5), seed=44).to(DEV)
    assert torch.equal(gfla.LocalAttnReshapeFunction.apply(x, 3), ref.local_attn_reshape_fwd(x, 3))
    i1 = randn((2, 5, 9, 8), seed=45).to(DEV)
    i2 = torch.cat((make_flow("wild", 2, 9, 8, seed=46), rand((2, 1, 9, 8), seed=47) * 2 + 0.5), 1).contiguous().to(DEV)
    r = ref.resample2d_fwd(i1, i2, 4, 1)
    assert_close(gfla.Resample2dFunction.apply(i1, i2, 4, 1), r, 4e-6)
    assert_close(oracle.resample2d_fwd(i1.cpu(), i2.cpu(), 4, 1), r.cpu(), 4e-6)
    g = randn(tuple(r.shape), seed=48).to(DEV)
    r1, r2 = ref.resample2d_bwd(i1, i2, g, 4, 1)
    o1, o2 = oracle.resample2d_bwd(i1.cpu(), i2.cpu(), g.cpu(), 4, 1, trunc_compat=True)
    assert_close(o1, r1.cpu(), F32_GRAD, "oracle reproduces the int() quirk of the real kernel")
    assert_close(o2, r2.cpu(), 1e-4)


def test_golden_vectors(gfla):
    path = os.path.join(GOLDEN, "ref_golden.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/ref_golden.npz not generated yet")
    z = np.load(path)
    t = lambda name: torch.from_numpy(z[name]).to(DEV)
    for k in (3, 5):
        out = gfla.BlockExtractorFunction.apply(t("be_source"), t("be_flow"), k)
        assert_close(out.cpu(), torch.from_numpy(z["be_out_k%d" % k]), F32_FWD, "golden block_extractor k=%d" % k)
    assert torch.equal(gfla.LocalAttnReshapeFunction.apply(t("lar_in"), 3).cpu(), torch.from_numpy(z["lar_out"]))
    out = gfla.Resample2dFunction.apply(t("rs_in1"), t("rs_in2"), 4, 1)
    assert_close(out.cpu(), torch.from_numpy(z["rs_out"]), 4e-6, "golden resample2d")


def test_golden_vectors_backward(gfla):
    """The HIP backward kernels against the gradients the REAL reference kernels produced for the golden inputs
    (be_gsrc / be_gflow, lar_gin, rs_gin1 / rs_gin2 in tests/golden/ref_golden.npz)."""
    path = os.path.join(GOLDEN, "ref_golden.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/ref_golden.npz not generated yet")
    z = np.load(path)
    t = lambda name: torch.from_numpy(z[name]).to(DEV)
    for k in (3, 5):
        s, f = t("be_source").requires_grad_(), t("be_flow").requires_grad_()
        gfla.BlockExtractorFunction.apply(s, f, k).backward(t("be_gout_k%d" % k))
        assert_close(s.grad.cpu(), torch.from_numpy(z["be_gsrc_k%d" % k]), F32_GRAD, "golden grad_source k=%d" % k)
        assert_close(f.grad.cpu(), torch.from_numpy(z["be_gflow_k%d" % k]), F32_GRAD, "golden grad_flow k=%d" % k)
    x = t("lar_in").requires_grad_()
    gfla.LocalAttnReshapeFunction.apply(x, 3).backward(t("lar_gout"))
    assert torch.equal(x.grad.cpu(), torch.from_numpy(z["lar_gin"]))
    i1, i2 = t("rs_in1").requires_grad_(), t("rs_in2").requires_grad_()
    gfla.Resample2dFunction.apply(i1, i2, 4, 1).backward(t("rs_gout"))
    assert_close(i1.grad.cpu(), torch.from_numpy(z["rs_gin1"]), F32_GRAD, "golden resample2d grad input1 (int() quirk)")
    assert_close(i2.grad.cpu(), torch.from_numpy(z["rs_gin2"]), 1e-4, "golden resample2d grad input2")


# ------------------------------------------------------------------------- replicate-pad gradient
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape,pad", [((2, 3, 7, 5), (2, 2, 2, 2)), ((1, 4, 6, 9), (1, 2, 1, 2)),
                                       ((2, 2, 1, 4), (2, 1, 3, 0)), ((1, 1, 5, 1), (0, 3, 2, 2)),
                                       ((3, 8, 32, 22), (1, 1, 1, 1))])
def test_replicate_pad_gradient_matches_torch(gfla, kernel_variant, dtype, shape, pad):
    if kernel_variant != "lds":
        pytest.skip("no kernel variants")
    from global_flow_local_attention_amd.extractor_attn import _ReplicatePad
    x = randn(shape, dtype, seed=71)
    a = x.to(DEV).requires_grad_()
    b = x.to(DEV).requires_grad_()
    ya = _ReplicatePad.apply(a, pad)
    yb = F.pad(b, pad, mode="replicate")
    assert torch.equal(ya, yb)
    up = randn(tuple(yb.shape), dtype, seed=72).to(DEV)
    ya.backward(up)
    yb.backward(up)
    assert_close(a.grad, b.grad, 1e-6 if dtype == torch.float32 else 1e-13, "replicate pad grad")


# ------------------------------------------------------------------------- non-finite flow values
@pytest.mark.parametrize("k", [3, 5])
def test_non_finite_flows_stay_in_bounds(gfla, oracle, k):
    """NaN / inf / 1e30 flow entries must neither crash nor disturb other pixels: indices are clamped after the
    float->int conversion (which saturates on the GPU as it does in the reference's CUDA), so the only
    affected outputs are the taps of the poisoned pixels themselves."""
    B, C, H, W = 2, 8, 20, 14
    s, f = randn((B, C, H, W), seed=80), make_flow("coherent", B, H, W, seed=81)
    bad = f.clone()
    poison = [(0, 3, 4, float("nan")), (0, 7, 9, float("inf")), (1, 11, 2, -float("inf")), (1, 15, 13, 1e30),
              (1, 0, 0, -1e30)]
    for b, y, x, v in poison:
        bad[b, :, y, x] = v
    clean = torch.ones(B, 1, H, W, dtype=torch.bool)
    for b, y, x, _ in poison:
        clean[b, 0, y, x] = False
    sd = s.to(DEV).requires_grad_()
    out = gfla.BlockExtractor(k)(sd, bad.to(DEV))
    want = oracle.block_extractor_fwd(s, f, k)
    mask = clean.repeat_interleave(k, 2).repeat_interleave(k, 3).expand(-1, C, -1, -1)
    assert_close(out.detach().cpu()[mask], want[mask], F32_FWD, "clean pixels, extractor")
    up = torch.where(mask, randn(tuple(out.shape), seed=82), torch.zeros(())).to(DEV)
    out.backward(up)                      # poisoned pixels receive zero upstream gradient
    gs, _ = oracle.block_extractor_bwd(s, f, up.cpu(), k)
    got = sd.grad.cpu()
    # a NaN/inf weight times a zero gradient is NaN (in the reference's atomicAdd as well): only the few
    # source positions the poisoned pixels' clamped taps land on may be non-finite, all others must agree
    finite = torch.isfinite(got)
    assert (~finite).sum().item() <= len(poison) * 4 * k * k * C
    assert_close(got[finite], gs[finite], F32_GRAD, "grad source away from the poisoned taps")
    r = gfla.Resample2d(4, 1, 2)(s.to(DEV), bad.to(DEV))
    rw = oracle.resample2d_module_fwd(s, f, 4, 1, 2.0)
    m2 = clean.expand(-1, C, -1, -1)
    assert_close(r.cpu()[m2], rw[m2], F32_FWD, "clean pixels, resample2d")
    att = gfla.ExtractorAttn(C, k, torch.nn.LeakyReLU(0.1), softmax=True).to(DEV)
    res = att(s.to(DEV), s.flip(0).to(DEV).contiguous(), bad.to(DEV))
    assert res.shape == (B, C, H, W)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- FC tail (LeakyReLU + 1x1 conv)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("KK,Hc,slope,bias,gemm_layout", [(25, 128, 0.1, True, True), (9, 128, 0.2, True, False),
                                                          (16, 40, 0.0, False, True), (4, 7, 0.01, True, True),
                                                          (1, 3, 0.1, False, False)])
def test_fc_tail_matches_torch_ops(gfla, kernel_variant, dtype, KK, Hc, slope, bias, gemm_layout):
    if kernel_variant != "lds":
        pytest.skip("no kernel variants")
    B, H, W = 3, 9, 31     # 279 positions: one full tile of 256 + a ragged one
    hs0, ht0 = randn((Hc, B, H, W) if gemm_layout else (B, Hc, H, W), dtype, seed=91), randn((B, Hc, H, W), dtype, seed=92)
    w1, b0, b1 = randn((KK, Hc), dtype, seed=93), randn((Hc,), dtype, seed=94), randn((KK,), dtype, seed=95)
    up = randn((B, KK, H, W), dtype, seed=96)

    def run(fused):
        leaves = [x.to(DEV).requires_grad_() for x in (hs0, ht0, w1)] + \
                 [x.to(DEV).requires_grad_() if bias else None for x in (b0, b1)]
        hs_l, ht_l, w_l, b0_l, b1_l = leaves
        hs = hs_l.permute(1, 0, 2, 3) if gemm_layout else hs_l
        if fused:
            out = gfla.FcTailFunction.apply(hs, ht_l, b0_l, w_l, b1_l, slope)
        else:
            pre = hs + ht_l + (b0_l.view(1, -1, 1, 1) if bias else 0)
            out = F.conv2d(F.leaky_relu(pre, slope), w_l.view(KK, Hc, 1, 1), b1_l)
        out.backward(up.to(DEV))
        return out.detach(), [l.grad for l in leaves if l is not None]

    got, g_got = run(True)
    want, g_want = run(False)
    t = 1e-5 if dtype == torch.float32 else 1e-12
    assert_close(got, want, t, "fc tail forward")
    for a, b_ in zip(g_got, g_want):
        assert a.shape == b_.shape
        assert_close(a, b_, t * 10, "fc tail gradient")



# ------------------------------------------------------------------------------ bf16 storage, backward (config 5)
def _rel(got, want):
    want = want.double()
    return (got.double().cpu() - want).abs().max().item() / max(1e-30, want.abs().max().item())


@pytest.mark.parametrize("k", [3, 5])
def test_bf16_backward_ops(gfla, oracle, kernel_variant, k):
    """bf16 storage for the backward entry points: bf16-rounded inputs through the f32 oracle, 2^-7 of the largest
    entry (gradients leave as bf16 after f32 / f64-in-LDS accumulation; grad_flow / grad_logits accumulate in float32
    inside the library and are cast at the end)."""
    if kernel_variant == "global":
        pytest.skip("bf16 storage exists for the planes-in-LDS kernels only (the forced-global knob does not apply)")
    B, C, H, W = 2, 8, 16, 12
    tol = 2 ** -7
    s = randn((B, C, H, W), seed=171).bfloat16()
    f = make_flow("coherent", B, H, W, seed=172).bfloat16()
    sf, ff = s.float(), f.float()
    # block_extractor (reference layout)
    sd, fd = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
    out = gfla.BlockExtractor(k)(sd, fd)
    g = randn(tuple(out.shape), seed=173).bfloat16()
    out.backward(g.to(DEV))
    gs, gf = oracle.block_extractor_bwd(sf, ff, g.float(), k)
    assert sd.grad.dtype == torch.bfloat16 and fd.grad.dtype == torch.bfloat16
    assert _rel(sd.grad.float(), gs) <= tol and _rel(fd.grad.float(), gf) <= tol
    # unfold layout
    sd, fd = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
    unf = gfla.BlockExtractorUnfoldFunction.apply(sd, fd, k)
    gu = _to_unfold(g.float(), k).bfloat16()
    unf.backward(gu.to(DEV))
    assert _rel(sd.grad.float(), gs) <= tol and _rel(fd.grad.float(), gf) <= tol
    # softmax / aggregate: against autograd of the f32 composition on the oracle's extractor
    lg = randn((B, k * k, H, W), seed=174).bfloat16()
    go = randn((B, C, H, W), seed=175).bfloat16()
    sd, fd, ld = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_(), lg.to(DEV).requires_grad_()
    res, _ = gfla.LocalAttnAggregateFunction.apply(sd, fd, ld, k, True)
    res.backward(go.to(DEV))
    from oracle import cpu_modules
    sc, fc, lc = sf.clone().requires_grad_(), ff.clone().requires_grad_(), lg.float().clone().requires_grad_()
    bs = cpu_modules._BlockExtractorCPU.apply(sc, fc, k)
    want = F.avg_pool2d(F.pixel_shuffle(torch.softmax(lc, 1), k) * bs, k, k)
    want.backward(go.float())
    assert sd.grad.dtype == fd.grad.dtype == ld.grad.dtype == torch.bfloat16
    assert _rel(sd.grad.float(), sc.grad) <= tol, "aggregate grad source"
    assert _rel(fd.grad.float(), fc.grad) <= tol, "aggregate grad flow"
    assert _rel(ld.grad.float(), lc.grad) <= tol, "aggregate grad logits"
    # resample2d
    i1 = randn((B, C, H, W), seed=176).bfloat16()
    i1d, fd = i1.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
    w = gfla.Resample2d(4, 1, 2)(i1d, fd)
    gw = randn((B, C, H, W), seed=177).bfloat16()
    w.backward(gw.to(DEV))
    i2 = torch.cat((ff, torch.full((B, 1, H, W), 2.0)), 1).contiguous()
    g1, g2 = oracle.resample2d_bwd(i1.float(), i2, gw.float(), 4, 1)
    assert i1d.grad.dtype == torch.bfloat16 and fd.grad.dtype == torch.bfloat16
    assert _rel(i1d.grad.float(), g1) <= tol, "resample grad input1"
    assert _rel(fd.grad.float(), g2[:, :2]) <= tol, "resample grad flow"


def test_bf16_backward_at_bench_shape(gfla, oracle, kernel_variant):
    """The same at one attention-layer shape of the bench (one plane per workgroup, 256 channel groups): sample slice
    against the f32 oracle."""
    if kernel_variant == "global":
        pytest.skip("bf16 storage exists for the planes-in-LDS kernels only (the forced-global knob does not apply)")
    B, C, H, W, k = 4, 256, 32, 22, 3
    s = randn((B, C, H, W), seed=181).bfloat16()
    f = make_flow("smooth", B, H, W, seed=182).bfloat16()
    lg = randn((B, k * k, H, W), seed=183).bfloat16()
    go = randn((B, C, H, W), seed=184).bfloat16()
    sd, fd, ld = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_(), lg.to(DEV).requires_grad_()
    res, _ = gfla.LocalAttnAggregateFunction.apply(sd, fd, ld, k, True)
    res.backward(go.to(DEV))
    from oracle import cpu_modules
    sc, fc, lc = s.float().requires_grad_(), f.float().requires_grad_(), lg.float().requires_grad_()
    bs = cpu_modules._BlockExtractorCPU.apply(sc, fc, k)
    want = F.avg_pool2d(F.pixel_shuffle(torch.softmax(lc, 1), k) * bs, k, k)
    want.backward(go.float())
    assert _rel(res.float(), want.detach()) <= 2 ** -7
    for got, ref, nm in ((sd.grad, sc.grad, "source"), (fd.grad, fc.grad, "flow"), (ld.grad, lc.grad, "logits")):
        assert _rel(got.float(), ref) <= 2 ** -7, nm


# ------------------------------------------------------- aggregate forward: coefficient-table / streaming kernels
@pytest.mark.parametrize("shape", [(2, 9, 12, 10), (1, 37, 33, 22), (3, 4, 6, 6), (2, 70, 64, 44), (1, 5, 9, 4), (2, 6, 7, 13)])
@pytest.mark.parametrize("kind", ["zero", "smooth", "wild", "integer", "near_integer"])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_aggregate_forward_table_path(gfla, oracle, kernel_variant, shape, kind, k):
    """gfla_local_attn_aggregate_fwd_ws_f32 with the table path forced for every odd k (tuning key 8 = 2; the default
    takes it from k = 5) against the float64 oracle chain: ragged tile overhangs, a map as narrow as one patch (4 / 6
    columns), an odd width (falls back to the plain kernels), several channel chunks and ranges (C = 70), flows far
    outside the map (the x clamp is folded into the coefficients), and flows within rounding of an integer, where the
    taps of a pixel stop forming a dense patch and the kernel evaluates it tap by tap."""
    if kernel_variant == "global":
        pytest.skip("table path is part of the default dispatch only")
    from global_flow_local_attention_amd import _lib
    B, C, H, W = shape
    s = randn((B, C, H, W), seed=71)
    if kind == "near_integer":
        f = make_flow("integer", B, H, W, seed=72)
        f = f + torch.where(randn((B, 2, H, W), seed=73) > 0, 1.0, -1.0) * 2.0 ** -22   # one or two ulps off an integer
    else:
        f = make_flow(kind, B, H, W, seed=72)
    lg = randn((B, k * k, H, W), seed=74) * 2
    a = torch.softmax(lg.double(), 1)
    ref = F.avg_pool2d(F.pixel_shuffle(a, k) * oracle.block_extractor_gather(s.double(), f.double(), k), k, k)
    sd, fd, ld = s.to(DEV), f.to(DEV), lg.to(DEV)
    out, attn = torch.empty_like(sd), torch.empty_like(ld)
    with gfla.tuned({gfla.TUNE_AGG_STREAM: 2}):
        _lib.aggregate_fwd(sd, fd, ld, out, attn, k, True)
    assert_close(attn.cpu(), a.float(), F32_FWD * 2, "attn")
    assert_close(out.cpu(), ref.float(), F32_FWD * 4, "out")
    if W % 2 == 0 and W >= k + 1:   # bf16 storage through the same kernels
        sb, fb, lb = (t.bfloat16() for t in (s, f, lg))
        ab = torch.softmax(lb.double(), 1)
        refb = F.avg_pool2d(F.pixel_shuffle(ab, k) * oracle.block_extractor_gather(sb.double(), fb.double(), k), k, k)
        ob, atb = torch.empty_like(sb, device=DEV), torch.empty_like(lb, device=DEV)
        with gfla.tuned({gfla.TUNE_AGG_STREAM: 2}):
            _lib.aggregate_fwd(sb.to(DEV), fb.to(DEV), lb.to(DEV), ob, atb, k, True)
        err = max_abs(ob.float().cpu(), refb.float()) / max(1e-30, refb.abs().max().item())
        assert err <= 2 ** -7, err


@pytest.mark.parametrize("shape", [(2, 9, 12, 10), (1, 37, 33, 22), (3, 4, 6, 6), (2, 70, 64, 44), (2, 6, 7, 13)])
@pytest.mark.parametrize("kind", ["zero", "smooth", "wild", "near_integer"])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_aggregate_backward_stream_path(gfla, oracle, kernel_variant, shape, kind, k):
    """d/d logits and d/d flow of the aggregation through agg_ga_stream_kernel, forced for every odd k (tuning key 8 = 2;
    default from k = 5), against autograd through the float64 oracle chain: the window sums have to map back onto the
    patch for clamped columns (wild flows, maps one patch wide), tile overhangs, several chunks and channel ranges, and
    pixels that are not a dense patch."""
    if kernel_variant == "global":
        pytest.skip("stream path is part of the default dispatch only")
    from global_flow_local_attention_amd import _lib
    B, C, H, W = shape
    s = randn((B, C, H, W), seed=81)
    if kind == "near_integer":
        f = make_flow("integer", B, H, W, seed=82)
        f = f + torch.where(randn((B, 2, H, W), seed=83) > 0, 1.0, -1.0) * 2.0 ** -22
    else:
        f = make_flow(kind, B, H, W, seed=82)
    lg = randn((B, k * k, H, W), seed=84) * 2
    go = randn((B, C, H, W), seed=85)
    s64, f64, l64 = s.double(), f.double().requires_grad_(), lg.double().requires_grad_()
    a = torch.softmax(l64, 1)
    ref = F.avg_pool2d(F.pixel_shuffle(a, k) * oracle.block_extractor_gather(s64, f64, k), k, k)
    ref.backward(go.double())
    sd, fd, ad, god = s.to(DEV), f.to(DEV), a.detach().float().to(DEV).contiguous(), go.to(DEV)
    gl, gf = torch.zeros_like(ad), torch.zeros_like(fd)
    with gfla.tuned({gfla.TUNE_AGG_STREAM: 2}):
        _lib.call("gfla_local_attn_aggregate_bwd_f32", sd, _lib.ptr(sd), _lib.ptr(fd), _lib.ptr(ad), _lib.ptr(god), None,
                  _lib.ptr(gf), _lib.ptr(gl), B, C, H, W, H, W, k, 1)
    assert_close(gl.cpu(), l64.grad.float(), F32_GRAD, "grad_logits")
    if kind != "near_integer":   # at (near-)integer flows the bilinear kink makes autograd's one-sided choice arbitrary
        assert_close(gf.cpu(), f64.grad.float(), F32_GRAD * 4, "grad_flow")


@pytest.mark.parametrize("case", [(2, 8, 12, 10, 4, 1), (1, 4, 200, 176, 4, 1), (2, 6, 16, 14, 4, 2), (4, 64, 32, 22, 4, 1),
                                  (2, 5, 9, 7, 2, 1)])
def test_resample2d_backward_overwrite_flag(gfla, kernel_variant, case):
    """GFLA_RESAMPLE_OVERWRITE_IN1 (bit 1 of the flag word): grad_in1 handed over full of NaNs comes back equal to the
    accumulate-into-zeros result on every path -- planes in LDS with one writer (plain stores), row windows and the
    global-memory kernels (internal zero fill + atomics), the matrix-core product with its device-side fallback."""
    from global_flow_local_attention_amd import _lib
    B, C, H, W, k, d = case
    i1 = randn((B, C, H, W), seed=91).to(DEV)
    i2 = torch.cat((make_flow("smooth", B, H, W, seed=92), torch.full((B, 1, H, W), 2.0)), 1).contiguous().to(DEV)
    go = randn((B, C, H, W), seed=93).to(DEV)
    ws = _lib.scatter_workspace(i1, B, H, W, k * k)
    for use_ws in (False, True):
        want = torch.zeros_like(i1)
        got = torch.full_like(i1, float("nan"))
        for buf, flags in ((want, 1), (got, 3)):
            if use_ws:
                _lib.call("gfla_resample2d_bwd_ws_f32", i1, _lib.ptr(i1), _lib.ptr(i2), _lib.ptr(go), _lib.ptr(buf), None,
                          _lib.ptr(ws), B, C, H, W, H, W, k, d, flags)
            else:
                _lib.call("gfla_resample2d_bwd_f32", i1, _lib.ptr(i1), _lib.ptr(i2), _lib.ptr(go), _lib.ptr(buf), None,
                          B, C, H, W, H, W, k, d, flags)
        assert torch.isfinite(got).all()
        assert_close(got.cpu(), want.cpu(), F32_GRAD, "overwrite vs accumulate (ws=%s)" % use_ws)


def test_streaming_kernels_random_shapes_against_round1_kernels(gfla, kernel_variant):
    """Forty random shapes (odd and even widths, maps one patch wide, C not a multiple of the chunk, B = 1, flows from
    zero to far outside the map) through the streaming kernels -- aggregation forward, d/d logits + d/d flow,
    resample2d d/d input2 -- against round 1's kernels (tuning keys 8 / 22), which the oracle tests pin."""
    if kernel_variant == "global":
        pytest.skip("stream kernels are part of the default dispatch only")
    from global_flow_local_attention_amd import _lib
    rng = np.random.RandomState(1234)
    for it in range(40):
        B, C = int(rng.randint(1, 4)), int(rng.randint(1, 41))
        H, W = int(rng.randint(2, 40)), int(rng.randint(4, 50))
        k = int(rng.choice([1, 3, 5]))
        scale = float(rng.choice([0.0, 0.7, 3.0, 25.0]))
        g = torch.Generator().manual_seed(1000 + it)
        src = torch.randn(B, C, H, W, generator=g).to(DEV)
        flow = (torch.randn(B, 2, H, W, generator=g) * scale).to(DEV)
        lg = (torch.randn(B, k * k, H, W, generator=g) * 2).to(DEV)
        go = torch.randn(B, C, H, W, generator=g).to(DEV)
        res = {}
        for tag, key8 in (("old", 1), ("new", 2)):
            with gfla.tuned({gfla.TUNE_AGG_STREAM: key8, gfla.TUNE_RS_BWD2_NO_STREAM: 1 if tag == "old" else 0}):
                out, attn = torch.empty_like(src), torch.empty_like(lg)
                _lib.aggregate_fwd(src, flow, lg, out, attn, k, True)
                gl, gf = torch.zeros_like(attn), torch.zeros_like(flow)
                _lib.call("gfla_local_attn_aggregate_bwd_f32", src, _lib.ptr(src), _lib.ptr(flow), _lib.ptr(attn), _lib.ptr(go),
                          None, _lib.ptr(gf), _lib.ptr(gl), B, C, H, W, H, W, k, 1)
                i2 = torch.cat((flow, torch.full((B, 1, H, W), 1.5, device=DEV)), 1).contiguous()
                g2 = torch.zeros_like(i2)
                _lib.call("gfla_resample2d_bwd_f32", src, _lib.ptr(src), _lib.ptr(i2), _lib.ptr(go), None, _lib.ptr(g2),
                          B, C, H, W, H, W, 4, 1, 0)
                res[tag] = (out, attn, gl, gf, g2)
        for name, a, b in zip(("out", "attn", "grad_logits", "grad_flow", "grad_in2"), res["new"], res["old"]):
            scale_ = max(1e-30, b.abs().max().item())
            err = (a - b).abs().max().item() / scale_
            assert err <= 2e-5, (it, (B, C, H, W, k, scale), name, err)


# ------------------------------------------------------------------------------ dispatch: defaults and tuning
def test_default_fc_arithmetic_is_float32(gfla, kernel_variant):
    """A module built through the reference surface, WITHOUT an explicit fc_mode, runs float32-grade arithmetic -- the
    reference's precision (base_function.py:799-810): the Winograd-domain kernels whose operands are two-term f16 splits
    exact to 2^-24 with all four cross products (mode 5, round 6) in forward and backward, never one of the lossy f16-split
    modes (1 / 2 / 3); fc_mode = 4 / 0 select the float32 Winograd / direct kernels; a map whose tiles modes 5 / 4 do not
    take falls back to mode 0 by itself."""
    if kernel_variant == "global":
        pytest.skip("dispatch test, independent of the gather/scatter variant")
    from global_flow_local_attention_amd import _lib, fc_mfma
    assert fc_mfma.DEFAULT_MODE == 5
    fc_ids = [_lib.fc_path(m, bwd) for m in range(6) for bwd in (False, True)]
    counts = lambda: {i: _lib.path_count(i) for i in fc_ids}

    def delta_of(before):
        after = counts()
        return {i: after[i] - before[i] for i in fc_ids if after[i] != before[i]}

    mod = gfla.ExtractorAttn(16, 3, torch.nn.LeakyReLU(0.1), softmax=True).to(DEV)
    assert not hasattr(mod, "fc_mode")
    s, t = (randn((2, 16, 12, 10), seed=i).to(DEV).requires_grad_() for i in (1, 2))
    f = make_flow("smooth", 2, 12, 10, seed=3).to(DEV).requires_grad_()
    for mode, want in ((None, 5), (4, 4), (0, 0)):
        if mode is not None:
            mod.fc_mode = mode                                                    # the float32 kernels on request
        before = counts()
        mod(s, t, f).sum().backward()
        torch.cuda.synchronize()
        assert delta_of(before) == {_lib.fc_path(want): 1, _lib.fc_path(want, True): 1}, (mode, delta_of(before))   # nothing else ran
    assert fc_mfma.resolve_mode(16, 12, 10, 3) == 5
    wide = fc_mfma.resolve_mode(8, 8, 700, 5)                                     # a span of 10 rows x 708 pixels: no LDS for it
    assert wide in (0, None) and not fc_mfma.supported(8, 8, 700, 5, 4) and not fc_mfma.supported(8, 8, 700, 5, 5)


def test_tuning_reaches_the_autograd_backward_thread(gfla, kernel_variant):
    """Tuning keys are process-global: a key set on the main thread must steer a backward that autograd runs on its
    own worker thread (a thread_local table silently lost the forced-global backward coverage)."""
    from global_flow_local_attention_amd import _lib
    s = randn((2, 5, 9, 8), seed=1).to(DEV).requires_grad_()
    f = make_flow("coherent", 2, 9, 8, seed=2).to(DEV).requires_grad_()
    lds0, glob0 = _lib.path_count(_lib.PATH_BE_BWD_LDS), _lib.path_count(_lib.PATH_BE_BWD_GLOBAL)
    gfla.BlockExtractor(3)(s, f).sum().backward()
    torch.cuda.synchronize()
    lds1, glob1 = _lib.path_count(_lib.PATH_BE_BWD_LDS), _lib.path_count(_lib.PATH_BE_BWD_GLOBAL)
    if kernel_variant == "global":
        assert (lds1 - lds0, glob1 - glob0) == (0, 1)
    else:
        assert (lds1 - lds0, glob1 - glob0) == (1, 0)


def test_resample2d_backward_with_empty_flow_returns_zeros(gfla):
    """An empty input2 skips the native call; d/d input1 must then be zeros, not uninitialised memory."""
    i1 = randn((2, 3, 6, 5), seed=1).to(DEV).requires_grad_()
    i2 = torch.zeros(2, 2, 0, 5, device=DEV)
    out = gfla.Resample2d(4, 1, 2)(i1, i2)
    assert out.shape == (2, 3, 0, 5)
    out.sum().backward()
    assert torch.equal(i1.grad, torch.zeros_like(i1))


def _rs_bwd_in1(gfla, i1, i2, go, ws=None, k=4):
    from global_flow_local_attention_amd import _lib
    B, C, H, W = i1.shape
    g1 = torch.full_like(i1, float("nan"))
    tail = (B, C, H, W, i2.shape[2], i2.shape[3], k, 1, 1 | 2)   # reference int() quirk + overwrite
    if ws is None:
        _lib.call("gfla_resample2d_bwd_f32", i1, _lib.ptr(i1), _lib.ptr(i2), _lib.ptr(go), _lib.ptr(g1), None, *tail)
    else:
        _lib.call("gfla_resample2d_bwd_ws_f32", i1, _lib.ptr(i1), _lib.ptr(i2), _lib.ptr(go), _lib.ptr(g1), None, _lib.ptr(ws),
                  *tail)
    torch.cuda.synchronize()
    return g1


@pytest.mark.parametrize("shape", [(3, 20, 64, 44), (2, 7, 33, 21)])
def test_resample2d_input1_gradient_fixed_point_planes(gfla, kernel_variant, shape):
    """d/d input1 on the 64-bit fixed-point LDS planes (csrc/lds_plane.h): (1) an integer sum does not depend on the order
    the lanes arrive in -- two runs are bit-identical, on rough flows too; (2) the tap-record path (scratch given) equals
    the in-kernel setup bit for bit; (3) it agrees with round 1's double planes (tuning key 23 = 1) to float rounding."""
    if kernel_variant == "global":
        pytest.skip("the global-memory kernels scatter with float atomics")
    from global_flow_local_attention_amd import _lib
    B, C, H, W = shape
    i1 = randn((B, C, H, W), seed=1).to(DEV)
    go = (randn((B, C, H, W), seed=2) * 3.0).to(DEV)
    for kind, seed in (("smooth", 3), ("wild", 4)):
        flow = make_flow(kind, B, H, W, seed=seed).to(DEV)
        i2 = torch.cat((flow, torch.full((B, 1, H, W), 2.0, device=DEV)), 1).contiguous()
        a, b = _rs_bwd_in1(gfla, i1, i2, go), _rs_bwd_in1(gfla, i1, i2, go)
        assert torch.equal(a, b), kind
        ws = _lib.scatter_workspace(i1, B, H, W, 16)
        with gfla.tuned({gfla.TUNE_PM: 1}):   # never the matrix-core scatter -> the LDS kernel reading tap records
            c = _rs_bwd_in1(gfla, i1, i2, go, ws)
        assert torch.equal(a, c), kind
        with gfla.tuned({gfla.TUNE_RS_BWD1_PLANES: 1}):
            d = _rs_bwd_in1(gfla, i1, i2, go)
        assert max_abs(a, d) <= 2e-6 * d.abs().max().item(), kind


def test_resample2d_input1_gradient_non_finite_is_not_silently_lost(gfla, kernel_variant):
    """A non-finite incoming gradient cannot be represented in fixed point: the workgroup's planes come out NaN (the
    reference would poison only the taps the value reaches) -- never a finite garbage value."""
    if kernel_variant == "global":
        pytest.skip("fixed-point planes are the LDS kernels'")
    B, C, H, W = 1, 4, 16, 12
    i1 = randn((B, C, H, W), seed=1).to(DEV)
    go = randn((B, C, H, W), seed=2).to(DEV)
    go[0, 1, 5, 6] = float("inf")
    flow = make_flow("smooth", B, H, W, seed=3).to(DEV)
    i2 = torch.cat((flow, torch.full((B, 1, H, W), 2.0, device=DEV)), 1).contiguous()
    g = _rs_bwd_in1(gfla, i1, i2, go)
    assert not torch.isfinite(g[0, 1]).all()
    assert torch.isfinite(g[0, 3]).all() or not torch.isfinite(g[0, 3]).any()   # a plane is poisoned as a whole or not at all


def test_bf16_features_beyond_the_lds_backward_fall_back_to_f32(gfla, oracle, kernel_variant):
    """128x128 bf16 maps: the bf16 aggregation backward (planes in LDS) does not take planes that large.  The
    block must still train.  Round 5: with the default float32 aggregation backward the bf16 path has no such
    limit any more and takes these maps itself; with extractor_attn.BF16_BACKWARD_F32_AGGREGATE = False the block is
    evaluated through the float32 view of the module (a warning; the per-call shadow of _fused_attention_f32_module) and
    the results are handed back in bf16.  Both ways: the module deep-copies afterwards and the parity bars hold."""
    if kernel_variant == "global":
        pytest.skip("gate test")
    import copy
    import warnings
    from global_flow_local_attention_amd import extractor_attn as ea
    from oracle import cpu_modules
    B, C, H, W, k = 1, 16, 128, 128, 3
    torch.manual_seed(0)
    mod = gfla.ExtractorAttn(C, k, torch.nn.LeakyReLU(0.1), softmax=True)
    ref = cpu_modules.ExtractorAttnCPU(C, k, torch.nn.LeakyReLU(0.1), softmax=True)
    ref.load_state_dict(mod.state_dict())
    mod = mod.to(DEV)
    bf = lambda x: x.to(torch.bfloat16)
    s, t = bf(randn((B, C, H, W), seed=1)), bf(randn((B, C, H, W), seed=2))
    f = bf(make_flow("smooth", B, H, W, seed=3))
    sc, tc, fc = (x.float().requires_grad_() for x in (s, t, f))
    want = ref(sc, tc, fc)
    want.sum().backward()
    old = ea.BF16_BACKWARD_F32_AGGREGATE
    try:
        for f32_aggregate, expect_warning in ((True, False), (False, True)):
            ea.BF16_BACKWARD_F32_AGGREGATE = f32_aggregate
            mod.__dict__.pop("_library_warned", None)
            sd, td, fd = (x.to(DEV).requires_grad_() for x in (s, t, f))
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                out = mod(sd, td, fd)
            assert any("float32" in str(x.message) for x in w) == expect_warning, (f32_aggregate, [str(x.message)[:80] for x in w])
            assert out.dtype == torch.bfloat16
            out.float().sum().backward()
            what = "bf16 128x128, float32 aggregation backward %s: " % f32_aggregate
            assert_close(out.float().cpu(), want.detach(), 2 ** -7, what + "forward")
            assert_close(sd.grad.float().cpu(), sc.grad, 2 ** -6, what + "grad source")
            assert_close(fd.grad.float().cpu(), fc.grad, 2 ** -5, what + "grad flow")
            copy.deepcopy(mod)        # nothing non-leaf left on the module (the float32 view is built per call)
    finally:
        ea.BF16_BACKWARD_F32_AGGREGATE = old
