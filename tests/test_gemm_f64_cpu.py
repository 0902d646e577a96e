"""gfla_gemm_f64 without a GPU: host-side argument validation of the C ABI, and the strided operand views fc_f64.py
hands it, checked against torch ops through a CPU model of the view descriptor (include/gfla_hip.h)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F


def _as_matrix(t, desc, offset, rows, cols):
    """The (rows x cols) matrix a 12-int64 view descriptor selects from t's storage (a torch view: writable)."""
    d = list(desc)
    sizes, strides = d[0:3] + d[6:9], d[3:6] + d[9:12]
    return t.as_strided(sizes, strides, t.storage_offset() + offset), (rows, cols)


def _cpu_gemm(c, c_view, a, a_view, b, b_view, M, N, K, beta=0, split_k=0, offsets=(0, 0, 0)):
    """What gfla_gemm_f64 computes, on CPU tensors."""
    cv, _ = _as_matrix(c, c_view, offsets[0], M, N)
    av, _ = _as_matrix(a, a_view, offsets[1], M, K)
    bv, _ = _as_matrix(b, b_view, offsets[2], K, N)
    prod = av.reshape(M, K) @ bv.reshape(K, N)
    cv.copy_((cv.reshape(M, N) + prod if beta else prod).reshape(cv.shape))


@pytest.fixture
def cpu_gemm(monkeypatch):
    from global_flow_local_attention_amd import fc_f64
    monkeypatch.setattr(fc_f64, "gemm", _cpu_gemm)
    return fc_f64


def test_gemm_f64_argument_validation_without_gpu(gfla):
    from global_flow_local_attention_amd import _lib, fc_f64
    L = _lib.lib()
    n = None
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    v = fc_f64.view(fc_f64.axis((4, 4)), fc_f64.axis((4, 1)))       # a 4 x 4 row-major matrix
    assert L.gfla_gemm_f64(n, v, p, v, p, v, 4, 4, 4, 0, 0, n, n) == -1
    assert L.gfla_gemm_f64(p, v, p, n, p, v, 4, 4, 4, 0, 0, n, n) == -1
    assert L.gfla_gemm_f64(p, v, p, v, p, v, -1, 4, 4, 0, 0, n, n) == -2     # negative extent
    assert L.gfla_gemm_f64(p, v, p, v, p, v, 4, 4, 4, 2, 0, n, n) == -2      # beta not 0 / 1
    assert L.gfla_gemm_f64(p, v, p, v, p, v, 4, 4, 4, 0, -1, n, n) == -2     # negative split_k
    assert L.gfla_gemm_f64(p, v, p, v, p, v, 4, 5, 4, 0, 0, n, n) == -2      # C's view does not tile N = 5
    bad = fc_f64.view(fc_f64.axis((0, 4)), fc_f64.axis((4, 1)))      # a sub-index of size 0
    assert L.gfla_gemm_f64(p, bad, p, v, p, v, 4, 4, 4, 0, 0, n, n) == -2
    # a split-K run needs its workspace
    assert L.gfla_gemm_f64_workspace_bytes(4, 4, 4096, 4) == 4 * 4 * 4 * 8
    big = fc_f64.view(fc_f64.axis((4, 4096)), fc_f64.axis((4096, 1)))
    bt = fc_f64.view(fc_f64.axis((4096, 4)), fc_f64.axis((4, 1)))
    assert L.gfla_gemm_f64(p, v, p, big, p, bt, 4, 4, 4096, 0, 4, n, n) == -1
    assert L.gfla_gemm_f64_workspace_bytes(4, 4, 4, 1) == 0
    assert L.gfla_gemm_f64_workspace_bytes(-1, 4, 4, 0) == -1
    assert L.gfla_gemm_f64_workspace_bytes(128, 3200, 90112, 0) > 0   # the weight gradient of attn2_256x176 splits K


def _blocks_from_unfold(u, c, k):
    """(C*k*k, B, H, W) unfold layout -> the reference block layout (B, C, H*k, W*k)."""
    _, b, h, w = u.shape
    return u.view(c, k, k, b, h, w).permute(3, 0, 4, 1, 5, 2).reshape(b, c, h * k, w * k).contiguous()


@pytest.mark.parametrize("k,C,B,H,W", [(3, 4, 2, 5, 3), (5, 3, 1, 4, 6), (2, 5, 3, 3, 2), (1, 2, 2, 3, 3)])
@pytest.mark.parametrize("blocks", [False, True])
def test_fc0_operand_views_match_conv2d(cpu_gemm, k, C, B, H, W, blocks):
    """Fc0F64Function's views (weight halves, unfold / block layout, (B, 128, H, W) maps, the transposes of the
    backward) compute the stride-k convolution of the reference's block tensors, and its gradients."""
    g = torch.Generator().manual_seed(k * 100 + C)
    w0 = torch.randn(128, 2 * C, k, k, generator=g, dtype=torch.float64)
    u_t = torch.randn(C * k * k, B, H, W, generator=g, dtype=torch.float64)
    u_s = torch.randn(C * k * k, B, H, W, generator=g, dtype=torch.float64)
    bt, bs = _blocks_from_unfold(u_t, C, k), _blocks_from_unfold(u_s, C, k)
    args = (bt, bs) if blocks else (u_t, u_s)
    hs, ht = cpu_gemm.Fc0F64Function.apply(w0, *args, k, blocks)
    assert torch.allclose(ht, F.conv2d(bt, w0[:, :C], stride=k), rtol=0, atol=1e-12)
    assert torch.allclose(hs, F.conv2d(bs, w0[:, C:], stride=k), rtol=0, atol=1e-12)
    ins = [w0.clone().requires_grad_()] + [x.clone().requires_grad_() for x in args]
    assert torch.autograd.gradcheck(lambda w, a, b: cpu_gemm.Fc0F64Function.apply(w, a, b, k, blocks), ins, fast_mode=True)


def test_fc1_weight_gradient_view(cpu_gemm):
    g = torch.Generator().manual_seed(5)
    gl = torch.randn(3, 9, 4, 5, generator=g, dtype=torch.float64)
    act = torch.randn(3, 128, 4, 5, generator=g, dtype=torch.float64)
    want = torch.bmm(gl.view(3, 9, 20), act.view(3, 128, 20).transpose(1, 2)).sum(0)
    assert torch.allclose(cpu_gemm.wgrad_fc1(gl, act), want, rtol=0, atol=1e-12)
