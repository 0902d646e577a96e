"""float64 ExtractorAttn on the FP64 matrix cores (csrc/gemm_f64.hip, fc_f64.py): gfla_gemm_f64 on exact integer data,
strict mode with no vendor fallback, parity with the CPU oracle, gradcheck."""
import warnings

import pytest
import torch

from util import make_flow, randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------- the GEMM itself
def _ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).double()


def _strided(fc_f64, t, transposed):
    """A 2-D matrix M as (storage tensor, view descriptor): row-major, or stored transposed."""
    r, c = t.shape
    if transposed:
        st = t.t().contiguous().to(DEV)
        return st, fc_f64.view(fc_f64.axis((r, 1)), fc_f64.axis((c, r)))
    return t.contiguous().to(DEV), fc_f64.view(fc_f64.axis((r, c)), fc_f64.axis((c, 1)))


SIZES = (1, 3, 17, 129)


@pytest.mark.parametrize("ta,tb,tc", [(False, False, False), (True, False, False), (False, True, False),
                                      (True, True, True)])
def test_gemm_f64_exact_integer_data(gfla, ta, tb, tc):
    """M, N, K over ragged sizes, operands stored plain or transposed, beta 0 and 1, split-K on and off: integer data in
    [-8, 8] make every sum exact, so the result must EQUAL torch.matmul on the CPU (a wrong accumulator row map of the f64
    MFMA or a swapped C index cannot pass)."""
    from global_flow_local_attention_amd import _lib, fc_f64
    n0 = _lib.path_count(_lib.PATH_GEMM_F64)
    calls = 0
    for M in SIZES:
        for N in SIZES:
            for K in SIZES + (1000,):
                seed = M * 10007 + N * 101 + K
                a, b, c0 = _ints((M, K), seed), _ints((K, N), seed + 1), _ints((M, N), seed + 2)
                A, av = _strided(fc_f64, a, ta)
                B, bv = _strided(fc_f64, b, tb)
                for beta in (0, 1):
                    for split in (1, 4):
                        C, cv = _strided(fc_f64, c0, tc)
                        fc_f64.gemm(C, cv, A, av, B, bv, M, N, K, beta=beta, split_k=split)
                        calls += 1
                        got = C.cpu().t() if tc else C.cpu()
                        want = a @ b + (c0 if beta else 0)
                        assert torch.equal(got, want), (M, N, K, beta, split, ta, tb, tc)
    assert _lib.path_count(_lib.PATH_GEMM_F64) == n0 + calls


def test_gemm_f64_three_index_views_and_determinism(gfla):
    """The views of the FC layers: weight half (offset into (128, 2C*k*k)) times the reference block layout
    (K = (c, i, j), N = (b, h, w)) into a (B, 128, H, W) map, and the weight gradient d hid . U^T with a long split-K
    reduction -- exact on integer data, and bit-identical from run to run."""
    from global_flow_local_attention_amd import fc_f64
    B, C, H, W, k = 3, 5, 7, 9, 3
    ckk, hw = C * k * k, H * W
    w0 = _ints((128, 2 * C, k, k), 1)
    blocks = _ints((B, C, H * k, W * k), 2)
    u = blocks.view(B, C, H, k, W, k).permute(1, 3, 5, 0, 2, 4).reshape(ckk, B * hw)   # (c,i,j) x (b,h,w)
    want = (w0.view(128, 2 * ckk)[:, ckk:] @ u).view(128, B, H, W).permute(1, 0, 2, 3)
    kax = fc_f64.axis((C, H * k * W * k), (k, W * k), (k, 1))
    nax = fc_f64.axis((B, C * H * k * W * k), (H, k * W * k), (W, k))
    hid_view = fc_f64.view(fc_f64.axis((128, hw)), fc_f64.axis((B, 128 * hw), (hw, 1)))
    w0d, bd = w0.to(DEV), blocks.to(DEV)
    out = torch.full((B, 128, H, W), float("nan"), dtype=torch.float64, device=DEV)   # beta = 0 never reads C
    fc_f64.gemm(out, hid_view, w0d, fc_f64.view(fc_f64.axis((128, 2 * ckk)), fc_f64.axis((ckk, 1))), bd,
                fc_f64.view(kax, nax), 128, B * hw, ckk, offsets=(0, ckk, 0))
    assert torch.equal(out.cpu(), want)
    # d W0[:, C:] = g . U^T, K = B*H*W reduced in split-K slices, written into the second half of a (128, 2C, k, k) buffer
    g = _ints((B, 128, H, W), 3)
    want_w = g.permute(1, 0, 2, 3).reshape(128, B * hw) @ u.t()
    for split in (0, 1, 7):
        gw = torch.zeros(128, 2 * C, k, k, dtype=torch.float64, device=DEV)
        fc_f64.gemm(gw, fc_f64.view(fc_f64.axis((128, 2 * ckk)), fc_f64.axis((ckk, 1))), g.to(DEV), hid_view, bd,
                    fc_f64.view(nax, kax), 128, ckk, B * hw, split_k=split, offsets=(ckk, 0, 0))
        assert torch.equal(gw.cpu().view(128, 2 * ckk)[:, ckk:], want_w), split
        assert not gw.cpu().view(128, 2 * ckk)[:, :ckk].any()
    # non-integer data: the same split twice gives the same bits
    gr = randn((B, 128, H, W), torch.float64, seed=4).to(DEV)
    br = randn((B, C, H * k, W * k), torch.float64, seed=5).to(DEV)
    res = []
    for _ in range(2):
        gw = torch.empty(128, 2 * C, k, k, dtype=torch.float64, device=DEV)
        for at in (0, ckk):
            fc_f64.gemm(gw, fc_f64.view(fc_f64.axis((128, 2 * ckk)), fc_f64.axis((ckk, 1))), gr, hid_view, br,
                        fc_f64.view(nax, kax), 128, ckk, B * hw, split_k=5, offsets=(at, 0, 0))
        res.append(gw.cpu())
    assert torch.equal(res[0], res[1])


# ---------------------------------------------------------------------------------------------- the module
def _module_pair(C, k, softmax, seed, B, H, W, flow_kind, flow_scale=1.0, kink=1e-10):
    """float64 module + CPU oracle with the same parameters, and inputs whose hidden activations stay off the
    LeakyReLU kink and whose flows stay off the integer lattice (one-sided derivatives there)."""
    import global_flow_local_attention_amd as gfla
    from oracle import cpu_modules
    for s in range(seed, seed + 30):
        torch.manual_seed(s)
        mod = gfla.ExtractorAttn(C, k, torch.nn.LeakyReLU(0.1), softmax=softmax).double()
        ref = cpu_modules.ExtractorAttnCPU(C, k, torch.nn.LeakyReLU(0.1), softmax=softmax).double()
        ref.load_state_dict(mod.state_dict())
        src = randn((B, C, H, W), torch.float64, seed=s + 1)
        tgt = randn((B, C, H, W), torch.float64, seed=s + 2)
        flow = make_flow(flow_kind, B, H, W, torch.float64, seed=s + 3) * flow_scale
        frac = flow - flow.round()
        flow = torch.where(frac.abs() < 1e-3, flow + 0.01, flow)
        hidden = []
        hook = ref.fully_connect_layer[0].register_forward_hook(lambda m, i, o: hidden.append(o.detach()))
        with torch.no_grad():
            ref(src, tgt, flow)
        hook.remove()
        if hidden[0].abs().min().item() > kink:
            return mod, ref, (src, tgt, flow)
    raise AssertionError("no seed keeps the hidden activations off the kink")


def _rel(got, want):
    return (got.detach().cpu() - want.detach()).abs().max().item() / max(1e-300, want.detach().abs().max().item())


def _check_parity(mod, ref, inputs, hook=False):
    from global_flow_local_attention_amd import _lib
    from global_flow_local_attention_amd import extractor_attn as ea
    gpu = [x.to(DEV).requires_grad_() for x in inputs]
    cpu = [x.clone().requires_grad_() for x in inputs]
    mod = mod.to(DEV)
    n0, v0 = _lib.path_count(_lib.PATH_GEMM_F64), ea.vendor_fallback_calls
    old = ea.VENDOR_FALLBACK
    ea.VENDOR_FALLBACK = "error"
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = mod.hook_attn_param(*gpu)[1] if hook else mod(*gpu)
        assert not any("rocBLAS" in str(x.message) for x in w)
    finally:
        ea.VENDOR_FALLBACK = old
    want = ref(*cpu)
    assert _lib.path_count(_lib.PATH_GEMM_F64) == n0 + 2, "the float64 FC layers did not run on gfla_gemm_f64"
    assert ea.vendor_fallback_calls == v0
    up = randn(tuple(want.shape), torch.float64, seed=99)
    out.backward(up.to(DEV))
    want.backward(up)
    assert _rel(out, want) <= 1e-12, ("forward", _rel(out, want))
    pairs = list(zip(gpu, cpu)) + list(zip(mod.parameters(), ref.parameters()))
    names = ["source", "target", "flow", "w0", "b0", "w1", "b1"]
    for name, (g, c) in zip(names, pairs):
        assert _rel(g.grad, c.grad) <= 1e-11, (name, _rel(g.grad, c.grad))


@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_strict_mode_float64_takes_no_vendor_path(gfla, oracle, k):
    """Strict mode (what install(strict_mfma=True) sets): a float64 block of every kernel size the fused block takes runs
    forward and backward without VendorFallbackError, without a warning, on gfla_gemm_f64."""
    mod, ref, inputs = _module_pair(6, k, True, 10 * k, 2, 9, 7, "coherent")
    _check_parity(mod, ref, inputs)


@pytest.mark.parametrize("flow_kind,scale", [("smooth", 1.0), ("wild", 1.0), ("wild", 4.0)])
@pytest.mark.parametrize("k,C,B,H,W", [(3, 16, 2, 12, 10), (5, 7, 3, 11, 9)])
def test_float64_parity_with_cpu_oracle(gfla, oracle, flow_kind, scale, k, C, B, H, W):
    """Smooth, wild and far out-of-bounds flows (scale 4: +-30 pixels), ragged shapes."""
    mod, ref, inputs = _module_pair(C, k, True, 7, B, H, W, flow_kind, scale)
    _check_parity(mod, ref, inputs)


@pytest.mark.parametrize("k", [3, 4])
def test_float64_softmax_none_and_hook(gfla, oracle, k):
    mod, ref, inputs = _module_pair(5, k, None, 3, 2, 8, 6, "smooth")
    _check_parity(mod, ref, inputs)
    mod, ref, inputs = _module_pair(5, k, True, 4, 2, 8, 6, "smooth")
    _check_parity(mod, ref, inputs, hook=True)


def test_float64_block_layout_operand(gfla, oracle, monkeypatch):
    """Planes beyond the unfold kernels' LDS budget (80 x 72 doubles) and unfold_gemm = False read the reference
    block layout in place."""
    from global_flow_local_attention_amd import _lib, fc_f64
    seen = []
    real = fc_f64._operand_axes
    monkeypatch.setattr(fc_f64, "_operand_axes", lambda u, blocks, k: seen.append(blocks) or real(u, blocks, k))
    assert not _lib.unfold_supported(80, 72, 3, 8)
    mod, ref, inputs = _module_pair(4, 3, True, 5, 1, 80, 72, "smooth")
    _check_parity(mod, ref, inputs)
    assert seen and all(seen)
    seen.clear()
    mod, ref, inputs = _module_pair(6, 5, True, 6, 2, 10, 8, "wild")
    mod.unfold_gemm = False
    _check_parity(mod, ref, inputs)
    assert seen and all(seen)
    seen.clear()
    mod.unfold_gemm = True
    _check_parity(mod, ref, inputs)
    assert seen and not any(seen)


def test_float64_bench_shape_slice(gfla, oracle):
    """Two samples of attn2_256x176 (C = 128, 64 x 44, k = 5)."""
    mod, ref, inputs = _module_pair(128, 5, True, 1, 2, 64, 44, "smooth")
    _check_parity(mod, ref, inputs)


def test_float64_library_request_is_unchanged(gfla):
    """fc_impl = 'library' keeps the torch-op path, counted as a vendor call."""
    from global_flow_local_attention_amd import _lib
    from global_flow_local_attention_amd import extractor_attn as ea
    m = gfla.ExtractorAttn(4, 3, torch.nn.LeakyReLU(0.1), softmax=True).double().to(DEV)
    m.fc_impl = "library"
    s, t = randn((1, 4, 6, 6), torch.float64, seed=1).to(DEV), randn((1, 4, 6, 6), torch.float64, seed=2).to(DEV)
    f = make_flow("coherent", 1, 6, 6, torch.float64, seed=3).to(DEV)
    n0, v0 = _lib.path_count(_lib.PATH_GEMM_F64), ea.vendor_fallback_calls
    m(s, t, f)
    assert ea.vendor_fallback_calls == v0 + 1 and _lib.path_count(_lib.PATH_GEMM_F64) == n0


@pytest.mark.parametrize("k", [3, 5])
def test_float64_gradcheck_strict(gfla, oracle, k):
    """torch.autograd.gradcheck of the whole block over (source, target, flow, conv0.weight, conv0.bias, conv1.weight,
    conv1.bias) in strict mode."""
    from global_flow_local_attention_amd import extractor_attn as ea
    mod, _, (s, t, f) = _module_pair(3, k, True, 20 + k, 1, 4, 3, "coherent", kink=1e-4)
    mod = mod.to(DEV)
    fc = mod.fully_connect_layer
    conv0, conv1 = fc[0], fc[2]

    def block(s, t, f, w0, b0, w1, b1):
        conv0.weight, conv0.bias, conv1.weight, conv1.bias = w0, b0, w1, b1
        return mod(s, t, f)

    params = [p.detach().clone() for p in (conv0.weight, conv0.bias, conv1.weight, conv1.bias)]
    for name in ("weight", "bias"):
        delattr(conv0, name)
        delattr(conv1, name)
    ins = [x.to(DEV).requires_grad_() for x in (s, t, f)] + [p.to(DEV).requires_grad_() for p in params]
    old = ea.VENDOR_FALLBACK
    ea.VENDOR_FALLBACK = "error"
    try:
        # nondet_tol: the scatters into (source, flow) accumulate with float atomics, so two backward passes may differ in
        # the last bits (the FC products themselves are bit-reproducible: test_gemm_f64_three_index_views_and_determinism)
        assert torch.autograd.gradcheck(block, ins, eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=1e-12, fast_mode=True)
    finally:
        ea.VENDOR_FALLBACK = old
