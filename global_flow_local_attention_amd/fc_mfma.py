"""fully_connect_layer of ExtractorAttn on the matrix cores (reference: model/networks/base_function.py:799-807).

`FcMfmaFunction` maps (source, target, flow, conv0.weight, conv0.bias, conv1.weight, conv1.bias) to the attention
logits (B, k*k, H, W) -- what the reference computes as
    fully_connect_layer[:3](cat(extractor(target, 0), extractor(source, flow)))
-- through gfla_fc_forward_f32 / gfla_fc_backward_f32 (csrc/fc_block.hip): no block tensor, no library GEMM or
convolution.  `mode` picks the arithmetic of the contraction (include/gfla_hip.h):
  4  float32 throughout, Winograd-domain convolutions and weight gradient (csrc/fc_wino.hip: F(2x2,5x5) / F(4x4,3x3),
     2.78x / 4x fewer multiplies); errors against float64 at the bench shapes 1e-6 .. 9e-6, held to the same test bars as
     mode 0;
  0  float32, direct convolution: a k-ordered fma chain per output (what mode 4 falls back to for maps its tiles do not fit);
  5  float32 tensors; every operand of a product as TWO f16 terms (hi + lo = the value to 2^-24 after a power-of-two scaling
     from the tensor's max |x|) on the f16 matrix cores, f32 accumulation -- THE DEFAULT (round 6).  Which kernel runs what is
     decided per convolution by measurement (csrc/fc_block.hip: fc_plan): the k = 5 convolutions and every data gradient on the
     direct kernels (three cross products, mode 2's arithmetic) reading the float32 maps in place; the k = 3 forward and the
     k = 5 weight gradient in the Winograd domain (all four cross products: csrc/fc_wino16.hip); the k = 3 weight
     gradient is mode 4's kernel.  Same measured error as mode 4, same test bars;
  3 / 2  operands split into three / two f16 terms, f32 accumulation (labelled experiments);  1  one f16 term (bf16 path).
"""
import ctypes

import torch
from torch.autograd import Function

from . import _lib

MODES = (0, 1, 2, 3, 4, 5)
# float32 is what the reference computes this layer in (base_function.py:799-810): a module without an explicit `fc_mode`
# gets float32-grade arithmetic -- two f16 terms per operand on the f16 matrix cores (5: every operand represented to
# 2^-24, f32 accumulation; measured error = mode 4's), the float32 Winograd kernels (4) or the
# float32 direct kernels (0) where the shape does not fit the faster one; 2 / 3 are labelled experiments (lower / other
# precision trade-offs), 1 belongs to the bf16-feature path
DEFAULT_MODE = 5
MODE_NAMES = {0: "f32 MFMA, direct convolution", 1: "one f16 term per operand (exact for bf16 values), f32 accumulate",
              2: "two f16 terms per operand, f32 accumulate", 3: "three f16 terms per operand, f32 accumulate",
              4: "f32 MFMA, Winograd-domain convolutions F(2x2,5x5) / F(4x4,3x3)",
              5: "two f16 terms per operand on f16 MFMA, f32 accumulate: direct kernels (k5 convolutions, data gradients) + "
                 "Winograd domain F(2x2,5x5) / F(4x4,3x3) (k3 forward, k5 weight gradient)"}


def supported(C, H, W, k, mode=DEFAULT_MODE):
    return bool(_lib.lib().gfla_fc_supported(int(C), int(H), int(W), int(k), int(mode)))


def resolve_mode(C, H, W, k, mode=None):
    """The arithmetic mode a call will run in: `mode` (DEFAULT_MODE when None) if the kernels take the shape; the float32
    direct kernels (0) when the float32 Winograd kernels (4) do not; None when nothing does."""
    mode = DEFAULT_MODE if mode is None else int(mode)
    if mode not in MODES:
        return None
    if supported(C, H, W, k, mode):
        return mode
    if mode == 5 and supported(C, H, W, k, 4):
        return 4
    if mode in (4, 5) and supported(C, H, W, k, 0):
        return 0
    return None


def workspace_bytes(B, C, H, W, k, mode, which):
    return _lib.workspace_bytes("gfla_fc_workspace_bytes", B, C, H, W, k, mode, which,
                                what="fc_mfma: unsupported shape (B, C, H, W, k, mode, which)")


def geometry(H, W, k, is_source):
    out = (ctypes.c_int64 * 13)()
    rc = _lib.lib().gfla_fc_geometry(int(H), int(W), int(k), 1 if is_source else 0, ctypes.cast(out, ctypes.c_void_p))
    if rc != 0:
        raise ValueError("gfla_fc_geometry: status %d" % rc)
    names = ("Hp", "Wp", "Ho", "Wo", "pad_t", "pad_l", "M", "Md", "lead", "Sx", "Sz", "Mg", "Mdg")
    return dict(zip(names, (int(v) for v in out)))


def _check(source, target, flow, w0, w1, k):
    _lib.require_gpu(source, target, flow, w0, w1)
    B, C, H, W = source.shape
    if tuple(target.shape) != (B, C, H, W) or tuple(flow.shape) != (B, 2, H, W):
        raise ValueError("fc_mfma: source %s, target %s and flow %s must share B, C (features) and H, W" %
                         (tuple(source.shape), tuple(target.shape), tuple(flow.shape)))
    if tuple(w0.shape) != (128, 2 * C, k, k) or tuple(w1.shape[:2]) != (k * k, 128):
        raise ValueError("fc_mfma: weights %s / %s do not belong to an ExtractorAttn(%d, %d)" %
                         (tuple(w0.shape), tuple(w1.shape), C, k))
    for t in (source, target, flow, w0, w1):
        if t.dtype != torch.float32:
            raise TypeError("fc_mfma: float32 only (got %s)" % t.dtype)


def _f32c(t):
    return None if t is None else t.detach().float().contiguous()


def forward_call(source, target, flow, w0, b0, w1, b1, k, slope, mode):
    """The FC forward on contiguous maps: gfla_fc_forward_f32 in `mode` for float32 source / target, gfla_fc_forward_f16
    (mode 1: the records packed straight from the maps) for float16 ones; flow float32.  The parameters are taken as float32.
    Returns (logits (B, k*k, H, W) float32, the workspace, conv1.weight as (k*k, 128)): what backward_call needs."""
    B, C, H, W = source.shape
    w0c, w1c, b0c, b1c = _f32c(w0), _f32c(w1).reshape(k * k, 128), _f32c(b0), _f32c(b1)
    ws = torch.empty(workspace_bytes(B, C, H, W, k, mode, 0), dtype=torch.uint8, device=source.device)
    logits = torch.empty((B, k * k, H, W), dtype=torch.float32, device=source.device)
    P = _lib.ptr
    if source.dtype == torch.float16:
        assert mode == 1, "gfla_fc_forward_f16 feeds the mode-1 backward"
        _lib.call("gfla_fc_forward_f16", source, P(source), P(target), P(flow), P(w0c), P(b0c), P(w1c), P(b1c), P(ws), P(logits),
                  B, C, H, W, k, float(slope))
    else:
        _lib.call("gfla_fc_forward_f32", source, P(source), P(target), P(flow), P(w0c), P(b0c), P(w1c), P(b1c), P(ws), P(logits),
                  B, C, H, W, k, float(slope), mode)
    return logits, ws, w1c


def backward_call(ws, flow, w1c, g_logits, dims, w_shapes, need, flags=0, g_source=None, g_flow=None):
    """gfla_fc_backward_f32 on the workspace of forward_call.  dims = (B, C, H, W, k, slope, mode); w_shapes = (conv0.weight
    shape, conv1.weight shape, has conv0.bias, has conv1.bias); need = the needs_input_grad of (source, target, flow, conv0.weight,
    conv0.bias, conv1.weight, conv1.bias).  g_source / g_flow: float32 buffers the call adds into (flags
    GFLA_FC_ACCUMULATE_SOURCE = 1 / GFLA_FC_ACCUMULATE_FLOW = 2); otherwise every wanted gradient gets a fresh float32 tensor.
    Returns (g_source, g_target, g_flow, g_w0, g_b0, g_w1, g_b1)."""
    B, C, H, W, k, slope, mode = dims
    w0_shape, w1_shape, has_b0, has_b1 = w_shapes
    dev = flow.device
    g_logits = g_logits.contiguous()

    def new(shape, wanted):
        return torch.empty(shape, dtype=torch.float32, device=dev) if wanted else None

    g = (new((B, C, H, W), need[0]) if g_source is None else g_source, new((B, C, H, W), need[1]),
         new((B, 2, H, W), need[2]) if g_flow is None else g_flow, new(w0_shape, need[3]), new((128,), need[4] and has_b0),
         new(w1_shape, need[5]), new((k * k,), need[6] and has_b1))
    scratch = torch.empty(workspace_bytes(B, C, H, W, k, mode, 1), dtype=torch.uint8, device=dev)
    _lib.call("gfla_fc_backward_f32", flow, _lib.ptr(ws), _lib.ptr(flow), _lib.ptr(w1c), _lib.ptr(g_logits),
              _lib.ptr(scratch), *[_lib.ptr(t) for t in g], B, C, H, W, k, slope, mode, flags)
    return g


def aggregate_backward_f32(source, flow, attn, g_out, g_source, g_flow, g_logits, k, apply_softmax=True):
    """gfla_local_attn_aggregate_bwd_ws_f32 on float32 operands: ADDS d/d source (the block-sparse product on the matrix
    cores, through its scatter table) and d/d flow into g_source / g_flow and writes d/d logits; None = not wanted."""
    b, c, hs, ws = source.shape
    h, w = flow.shape[2:]
    table = _lib.scatter_workspace(source, b, h, w, (k + 1) ** 2) if g_source is not None else None
    _lib.call("gfla_local_attn_aggregate_bwd_ws_f32", source, _lib.ptr(source), _lib.ptr(flow), _lib.ptr(attn), _lib.ptr(g_out),
              _lib.ptr(g_source), _lib.ptr(g_flow), _lib.ptr(g_logits), _lib.ptr(table), b, c, hs, ws, h, w, k,
              1 if apply_softmax else 0)


class FcMfmaFunction(Function):
    @staticmethod
    def forward(ctx, source, target, flow, w0, b0, w1, b1, kernel_size, slope, mode):
        k, mode = int(kernel_size), int(mode)
        _check(source, target, flow, w0, w1, k)
        source, target, flow = source.contiguous(), target.contiguous(), flow.contiguous()
        logits, ws, w1c = forward_call(source, target, flow, w0, b0, w1, b1, k, slope, mode)
        ctx.save_for_backward(flow, w1c, ws)
        ctx.dims = tuple(source.shape) + (k, float(slope), mode)
        ctx.w_shapes = (w0.shape, w1.shape, b0 is not None, b1 is not None)
        return logits

    @staticmethod
    def backward(ctx, g_logits):
        flow, w1c, ws = ctx.saved_tensors
        return backward_call(ws, flow, w1c, g_logits, ctx.dims, ctx.w_shapes, ctx.needs_input_grad) + (None, None, None)
