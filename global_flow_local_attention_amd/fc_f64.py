"""ExtractorAttn's fully_connect_layer in float64 on the FP64 matrix cores (csrc/gemm_f64.hip).

The same formulation as the library path of extractor_attn._fused_attention, with every vendor product replaced by
gfla_gemm_f64, which reads and writes its operands in place through strided views:

  hid_t = W0[:, :C] . U_t      U_t = the zero-flow unfold of target (= its replicate-padded unfold)
  hid_s = W0[:, C:] . U_s      U_s = unfold(source, flow)
  logits = FcTailFunction(hid_s, hid_t, ...)   (csrc/fc_tail.hip; its dW1 on gfla_gemm_f64 too)

U is the extractor's unfold layout (C*k*k, B, H, W) when the source planes fit its LDS budget, the reference block
layout (B, C, H*k, W*k) otherwise -- both read in place (K = (c, i, j), N = (b, h, w)).  Backward: dW0 = d hid . U^T
straight into the two halves of conv0.weight's gradient, dU = W0^T . d hid into U's layout, which the extractor's
backward node then scatters into (source, flow) / target.
"""
import ctypes

import torch
from torch.autograd import Function

from . import _lib


def axis(*dims):
    """One logical index of a GEMM operand as up to three (size, stride) sub-indices, outermost first."""
    dims = list(dims)
    if not 1 <= len(dims) <= 3:
        raise ValueError("gemm_f64: an index has 1 to 3 sub-indices, got %d" % len(dims))
    dims = [(1, 0)] * (3 - len(dims)) + [(int(n), int(s)) for n, s in dims]
    return [n for n, _ in dims] + [s for _, s in dims]


def view(rows, cols):
    """The 12-int64 view descriptor of include/gfla_hip.h from two axis(...) lists."""
    return (ctypes.c_int64 * 12)(*(rows + cols))


def gemm(c, c_view, a, a_view, b, b_view, M, N, K, beta=0, split_k=0, offsets=(0, 0, 0)):
    """C = beta*C + A.B on float64 CUDA tensors (gfla_gemm_f64); each operand is its tensor's storage seen through a
    view(...) descriptor, starting `offsets[i]` elements past its data pointer.  Enqueued on c's current stream."""
    for t in (c, a, b):
        if t.dtype != torch.float64:
            raise TypeError("gemm_f64: float64 operands only (got %s)" % t.dtype)
    _lib.require_gpu(c, a, b)
    n = _lib.workspace_bytes("gfla_gemm_f64_workspace_bytes", M, N, K, split_k, what="gemm_f64 (M, N, K, split_k)")
    ws = torch.empty(n, dtype=torch.uint8, device=c.device) if n > 0 else None   # no split: NULL, as the header allows
    p = [ctypes.c_void_p(t.data_ptr() + 8 * int(o)) for t, o in zip((c, a, b), offsets)]
    _lib.call("gfla_gemm_f64", c, p[0], c_view, p[1], a_view, p[2], b_view, int(M), int(N), int(K), int(beta),
              int(split_k), _lib.ptr(ws))


def _operand_axes(u, blocks, k):
    """(K axis, N axis, C, B, H, W) of an extractor output: unfold (C*k*k, B, H, W) or block layout (B, C, H*k, W*k)."""
    if blocks:
        b, c, hk, wk = u.shape
        h, w = hk // k, wk // k
        kax = axis((c, hk * wk), (k, wk), (k, 1))
        nax = axis((b, c * hk * wk), (h, k * wk), (w, k))
    else:
        ckk, b, h, w = u.shape
        c = ckk // (k * k)
        kax = axis((ckk, b * h * w))
        nax = axis((b * h * w, 1))
    return kax, nax, c, b, h, w


class Fc0F64Function(Function):
    """The two halves of ExtractorAttn's first FC convolution, without bias: (w0, u_t, u_s) -> (hid_s, hid_t), both
    (B, 128, H, W).  w0 (128, 2C, k, k); u_t / u_s the extractor outputs of target (zero flow) and source, in the unfold
    layout or (blocks=True) the reference block layout."""

    @staticmethod
    def forward(ctx, w0, u_t, u_s, k, blocks):
        k = int(k)
        w0c = w0.contiguous()
        kax, nax, c, b, h, w = _operand_axes(u_s, blocks, k)
        hc, ckk, hw = w0c.size(0), c * k * k, h * w
        if tuple(w0c.shape) != (hc, 2 * c, k, k) or u_t.shape != u_s.shape:
            raise ValueError("fc_f64: w0 %s does not match the operands %s / %s" % (tuple(w0.shape), tuple(u_t.shape),
                                                                                    tuple(u_s.shape)))
        hid_s, hid_t = (u_s.new_empty((b, hc, h, w)) for _ in range(2))
        hid_view = view(axis((hc, hw)), axis((b, hc * hw), (hw, 1)))
        w_view = view(axis((hc, 2 * ckk)), axis((ckk, 1)))
        u_view = view(kax, nax)
        for out, u, at in ((hid_t, u_t, 0), (hid_s, u_s, ckk)):
            gemm(out, hid_view, w0c, w_view, u, u_view, hc, b * hw, ckk, offsets=(0, at, 0))
        ctx.save_for_backward(w0c, u_t, u_s)
        ctx.geom = (k, bool(blocks))
        return hid_s, hid_t

    @staticmethod
    def backward(ctx, g_s, g_t):
        w0c, u_t, u_s = ctx.saved_tensors
        k, blocks = ctx.geom
        kax, nax, c, b, h, w = _operand_axes(u_s, blocks, k)
        hc, ckk, hw = w0c.size(0), c * k * k, h * w
        need_w, need_t, need_s = ctx.needs_input_grad[:3]
        g_t, g_s = g_t.contiguous(), g_s.contiguous()
        g_view = view(axis((hc, hw)), axis((b, hc * hw), (hw, 1)))          # d hid (B, Hc, H, W) as (o, (b, p))
        w_view = view(axis((hc, 2 * ckk)), axis((ckk, 1)))                  # a half of W0 (or of dW0) as (o, (c, i, j))
        wt_view = view(axis((ckk, 1)), axis((hc, 2 * ckk)))                 # its transpose
        halves = ((g_t, u_t, 0, need_t), (g_s, u_s, ckk, need_s))
        g_w0 = torch.empty_like(w0c) if need_w else None
        g_u = []
        for g, u, at, need in halves:
            if need_w:    # dW0[:, half] = d hid . U^T
                gemm(g_w0, w_view, g, g_view, u, view(nax, kax), hc, ckk, b * hw, offsets=(at, 0, 0))
            g_u.append(None)
            if need:      # dU = W0[:, half]^T . d hid, in U's layout
                g_u[-1] = torch.empty_like(u)
                gemm(g_u[-1], view(kax, nax), w0c, wt_view, g, g_view, ckk, b * hw, hc, offsets=(0, at, 0))
        return g_w0, g_u[0], g_u[1], None, None


def wgrad_fc1(g_logits, act):
    """dW1[q, o] = sum_b g_logits_b . act_b^T: g_logits (B, KK, H, W), act (B, Hc, H, W) -> (KK, Hc), deterministic
    split-K over (b, p)."""
    b, kk, h, w = g_logits.shape
    hc, hw = act.size(1), h * w
    g_logits, act = g_logits.contiguous(), act.contiguous()
    out = g_logits.new_empty((kk, hc))
    gemm(out, view(axis((kk, hc)), axis((hc, 1))), g_logits, view(axis((kk, hw)), axis((b, kk * hw), (hw, 1))),
         act, view(axis((b, hc * hw), (hw, 1)), axis((hc, hw))), kk, hc, b * hw)
    return out
