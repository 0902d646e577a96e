"""The convolutions of the generators' bodies on the library's own kernels (csrc/gen_conv.hip; the gradients:
csrc/gen_conv_bwd.hip, csrc/gen_conv_wgrad.hip).

Every EncoderBlock, ResBlock, ResBlockDecoder and Jump of the reference (base_function.py:334-391, 508-531, 672-691) is
built from three convolutions: Conv2d(k 3, s 1) with zero or reflection padding, Conv2d(k 4, s 2, p 1) and
ConvTranspose2d(k 3, s 2, p 1, output_padding 1), each behind a LeakyReLU, two of them in front of a residual sum.  Here
each is one launch on the matrix cores, with the activation applied while the input is staged and the residual added in
the epilogue:

    conv3x3, conv4x4_down, conv_transpose3x3_up     functional forms
    conv1x1                                         the 1x1 convolution, optionally behind AvgPool2d(2) (csrc/conv1x1.hip)
    GenConvFunction, Conv1x1Function                the autograd Functions on the kernels (grad="kernels")
    InferenceConv                                   module with the replaced convolution's Parameters and names
    fuse_inference_convs                            rewrite the convolutions of a network in place
    patch_reference_convs                           the reference's block classes, rewritten as they are built

Whenever a gradient could be asked for -- grad mode is on and x, the weight, the bias or the addend requires one -- the
keyword `grad` decides: "torch" (the default everywhere) takes the exact torch composition (F.leaky_relu -> F.pad(reflect)
-> F.conv2d / F.conv_transpose2d -> + add), so training is untouched; "kernels" runs GenConvFunction, whose backward is
the library's data, weight and bias gradient kernels.  CPU tensors, float64 and impl="torch" always take the composition.
"""
import ctypes

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from ._conv_common import SFX as _SFX, SRC_TYPE as _SRC_TYPE, autocast_dtype, cached, rounded_bias
from .head_conv import MAX_COUT as _HEAD_MAX_COUT

IMPLS = _lib.IMPLS
PADDINGS = ("zeros", "reflect")
GRADS = ("torch", "kernels")
S1K3, S2K4, T2K3 = 0, 1, 2
P1K1 = 3            # InferenceConv's name for Conv2d(k 1, s 1, p 0): conv1x1, entry points of its own, never a C `geometry`
_KERNEL_SIZE = {S1K3: 3, S2K4: 4, T2K3: 3, P1K1: 1}
_NAMES = {S1K3: "conv3x3", S2K4: "conv4x4_down", T2K3: "conv_transpose3x3_up", P1K1: "conv1x1"}
POOLS = (1, 2)


def out_size(geometry, H, W):
    """(Hout, Wout) of a geometry (gfla_gen_conv_out_size)"""
    ho, wo = ctypes.c_int64(), ctypes.c_int64()
    status = _lib.lib().gfla_gen_conv_out_size(int(geometry), int(H), int(W), ctypes.addressof(ho), ctypes.addressof(wo))
    if status != 0:
        raise ValueError("%s: no output for a %d x %d map (%s)" % (_NAMES.get(geometry, "gen_conv"), H, W,
                                                                  _lib.lib().gfla_status_string(status).decode()))
    return ho.value, wo.value


def packed_weights(weight, dtype, geometry):
    """torch's `weight` ((Cout,Cin,k,k); T2K3: (Cin,Cout,3,3)) packed in compute type `dtype`, once per frozen parameter."""
    def make():
        w = weight.detach().contiguous()
        cout, cin = (w.size(1), w.size(0)) if geometry == T2K3 else (w.size(0), w.size(1))
        esize = torch.empty((), dtype=dtype).element_size()
        packed = _lib.workspace("gfla_gen_conv_packed_bytes", w, cout, cin, geometry, esize, what="gen_conv packed weights")
        _lib.call("gfla_gen_conv_pack_weights_" + _SFX[dtype], w, _lib.ptr(w), _SRC_TYPE[w.dtype], _lib.ptr(packed), cout,
                  cin, geometry)
        return packed
    return cached(weight, "gen_conv%d" % geometry, dtype, make)


def packed_grad_weights(weight, dtype, geometry):
    """torch's `weight` packed for the data gradient (the adjoint geometry) in compute type `dtype`; cached on the
    parameter's version, so a stepped optimizer repacks"""
    def make():
        w = weight.detach().contiguous()
        cout, cin = (w.size(1), w.size(0)) if geometry == T2K3 else (w.size(0), w.size(1))
        esize = torch.empty((), dtype=dtype).element_size()
        packed = _lib.workspace("gfla_gen_conv_grad_packed_bytes", w, cout, cin, geometry, esize,
                                what="gen_conv packed gradient weights")
        _lib.call("gfla_gen_conv_pack_grad_weights_" + _SFX[dtype], w, _lib.ptr(w), _SRC_TYPE[w.dtype], _lib.ptr(packed),
                  cout, cin, geometry)
        return packed
    return cached(weight, "gen_conv_grad%d" % geometry, dtype, make)


def _check_grad(grad):
    if grad not in GRADS:
        raise ValueError("grad: one of %s (got %r)" % (GRADS, grad))


def _validate(x, weight, bias, geometry, padding, pre_slope, add):
    """Everything that can be wrong with a call, before anything is launched.  Returns (Cout, Hout, Wout)."""
    name, k = _NAMES[geometry], _KERNEL_SIZE[geometry]
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError("%s: a non-empty (B,Cin,H,W) map (got %s)" % (name, tuple(x.shape)))
    if padding not in PADDINGS:
        raise ValueError("%s: padding is one of %s (got %r)" % (name, PADDINGS, padding))
    cin_axis = 0 if geometry == T2K3 else 1
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (k, k) or weight.size(cin_axis) != x.size(1) or \
            weight.size(1 - cin_axis) < 1:
        raise ValueError("%s: weight %s with Cin = %d (got %s)" % (
            name, "(Cin,Cout,3,3)" if geometry == T2K3 else "(Cout,Cin,%d,%d)" % (k, k), x.size(1), tuple(weight.shape)))
    cout = weight.size(1 - cin_axis)
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError("%s: bias (Cout,) = (%d,) (got %s)" % (name, cout, tuple(bias.shape)))
    H, W = x.shape[2:]
    if padding == "reflect" and (H < 2 or W < 2):
        raise ValueError("%s: reflect padding of one pixel needs H, W >= 2 (got %s)" % (name, tuple(x.shape)))
    if geometry == S2K4 and (H < 2 or W < 2):
        raise ValueError("%s: H, W >= 2 (got %s)" % (name, tuple(x.shape)))
    if pre_slope is not None and not float(pre_slope) >= 0:
        raise ValueError("%s: pre_slope is None or a slope >= 0 (got %r)" % (name, pre_slope))
    ho, wo = (H, W) if geometry == S1K3 else ((H - 2) // 2 + 1, (W - 2) // 2 + 1) if geometry == S2K4 else (2 * H, 2 * W)
    if add is not None and tuple(add.shape) != (x.size(0), cout, ho, wo):
        raise ValueError("%s: add has the output's shape %s (got %s)" % (name, (x.size(0), cout, ho, wo), tuple(add.shape)))
    return cout, ho, wo


def torch_gen_conv(x, weight, bias, geometry, padding="zeros", pre_slope=None, add=None):
    """The same map as the composition the reference runs: F.leaky_relu, F.pad(mode="reflect") or the convolution's own
    zero padding, F.conv2d / F.conv_transpose2d, + add.  Any dtype, any device."""
    a = x if pre_slope is None else F.leaky_relu(x, pre_slope)
    if weight.dtype != a.dtype and not torch.is_autocast_enabled():
        weight = weight.to(a.dtype)
        bias = None if bias is None else bias.to(a.dtype)
    if geometry == S1K3 and padding == "reflect":
        y = F.conv2d(F.pad(a, (1, 1, 1, 1), mode="reflect"), weight, bias)
    elif geometry == S1K3:
        y = F.conv2d(a, weight, bias, stride=1, padding=1)
    elif geometry == S2K4:
        y = F.conv2d(a, weight, bias, stride=2, padding=1)
    else:
        y = F.conv_transpose2d(a, weight, bias, stride=2, padding=1, output_padding=1)
    return y if add is None else y + add


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _kernel_inputs(x, weight, bias, add):
    if not x.is_cuda or not x.is_floating_point() or x.dtype == torch.float64:
        return False
    if x.dtype not in _SFX and not torch.is_autocast_enabled():
        return False
    for p in (weight, bias):
        if p is not None and (not p.is_cuda or p.dtype not in _SRC_TYPE):
            return False
    return add is None or (add.is_cuda and add.is_floating_point() and add.dtype != torch.float64)


def _launch(x, weight, bias, geometry, padding, pre_slope, add, cout, ho, wo):
    if torch.is_autocast_enabled():
        x = x.to(autocast_dtype())
    if x.dtype not in _SFX:
        raise _lib.Unsupported("%s: no kernel for %s" % (_NAMES[geometry], x.dtype))
    x = x.contiguous()
    B, Cin, H, W = x.shape
    wp = packed_weights(weight, x.dtype, geometry)
    b32 = None if bias is None else rounded_bias(bias, x.dtype, "gen_conv_b")
    if add is not None:
        add = add.detach().to(x.dtype).contiguous()
    y = x.new_empty((B, cout, ho, wo))
    _lib.call("gfla_gen_conv_fwd_" + _SFX[x.dtype], x, _lib.ptr(x), _lib.ptr(wp), _lib.ptr(b32), _lib.ptr(add), _lib.ptr(y),
              B, Cin, cout, H, W, geometry, PADDINGS.index(padding), int(pre_slope is not None), float(pre_slope or 0.0))
    return y


class GenConvFunction(Function):
    """(x, weight, bias | None, add | None, geometry, padding, pre_slope, (Cout, Hout, Wout)) -> y on the library's kernels,
    with the gradients of all four tensors.

    x: float32 / float16 / bfloat16 on the GPU (under torch.autocast the caller casts it first, so a float32 x gets a
    float32 gradient through the cast).  Saved for the backward: x and the weight, nothing else -- act(x) is recomputed
    while the gradient kernels stage it.  The backward launches only what needs_input_grad asks for: the data gradient
    (x's dtype), the weight and bias gradients (float32 sums, rounded once to the parameter's dtype); the addend's
    gradient is grad_y in the addend's dtype.  No atomics anywhere: bit-identical from call to call.
    The decision is made here, in the forward: whatever the backward would need that the library refuses raises
    _lib.Unsupported before anything is launched, and the caller takes the torch composition for the whole call."""

    @staticmethod
    def forward(ctx, x, weight, bias, add, geometry, padding, pre_slope, dims):
        cout, ho, wo = dims
        need_x, need_w, need_b, need_add = ctx.needs_input_grad[:4]
        need_b = need_b and bias is not None
        B, Cin, H, W = x.shape
        if need_x or need_w or need_b:
            esize = x.element_size()
            _lib.workspace_bytes("gfla_gen_conv_bwd_workspace_bytes", B, Cin, cout, H, W, geometry, PADDINGS.index(padding),
                                 esize, what="gen_conv backward")
            _lib.workspace_bytes("gfla_gen_conv_grad_packed_bytes", cout, Cin, geometry, esize, what="gen_conv backward")
        y = _launch(x, weight, bias, geometry, padding, pre_slope, add, cout, ho, wo)
        ctx.conf = (cout, geometry, PADDINGS.index(padding), int(pre_slope is not None), float(pre_slope or 0.0))
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.add_dtype = None if add is None else add.dtype
        if need_x or need_w or need_b:
            ctx.save_for_backward(x.contiguous(), weight)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        need_x, need_w, need_b, need_add = ctx.needs_input_grad[:4]
        need_b = need_b and ctx.bias_dtype is not None
        need_add = need_add and ctx.add_dtype is not None
        g_add = g.to(ctx.add_dtype) if need_add else None
        dx = dw = db = None
        if need_x or need_w or need_b:
            x, weight = ctx.saved_tensors
            cout, geometry, pad_mode, pre_act, slope = ctx.conf
            B, Cin, H, W = x.shape
            sfx = _SFX[x.dtype]
            gy = g.to(x.dtype).contiguous()
            ws = _lib.workspace("gfla_gen_conv_bwd_workspace_bytes", x, B, Cin, cout, H, W, geometry, pad_mode,
                                x.element_size(), what="gen_conv backward")
            tail = (B, Cin, cout, H, W, geometry, pad_mode, pre_act, slope)
            if need_x:
                dx = torch.empty_like(x)
                wp = packed_grad_weights(weight, x.dtype, geometry)
                _lib.call("gfla_gen_conv_bwd_data_" + sfx, x, _lib.ptr(gy), _lib.ptr(x), _lib.ptr(wp), _lib.ptr(dx),
                          _lib.ptr(ws), *tail)
            if need_w or need_b:
                dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device) if need_w else None
                db = torch.empty(cout, dtype=torch.float32, device=x.device) if need_b else None
                _lib.call("gfla_gen_conv_bwd_weight_" + sfx, x, _lib.ptr(gy), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(db),
                          _lib.ptr(ws), *tail)
                if dw is not None and dw.dtype != weight.dtype:
                    dw = dw.to(weight.dtype)
                if db is not None and db.dtype != ctx.bias_dtype:
                    db = db.to(ctx.bias_dtype)
        return dx, dw, db, g_add, None, None, None, None


def _gen_conv(x, weight, bias, geometry, padding, pre_slope, add, impl, grad="torch"):
    _lib.check_impl(impl)
    _check_grad(grad)
    cout, ho, wo = _validate(x, weight, bias, geometry, padding, pre_slope, add)
    if impl == "auto" and _kernel_inputs(x, weight, bias, add):
        needs = _needs_grad(x, weight, bias, add)
        try:
            if not needs:
                return _launch(x.detach(), weight, bias, geometry, padding, pre_slope, add, cout, ho, wo)
            if grad == "kernels":
                xk = x.to(autocast_dtype()) if torch.is_autocast_enabled() else x
                if xk.dtype in _SFX:
                    return GenConvFunction.apply(xk, weight, bias, add, geometry, padding, pre_slope, (cout, ho, wo))
        except _lib.Unsupported:
            pass
    return torch_gen_conv(x, weight, bias, geometry, padding, pre_slope, add)


def conv3x3(x, weight, bias=None, padding="zeros", pre_slope=None, add=None, impl="auto", grad="torch"):
    """conv2d(pad(leaky_relu(x, pre_slope)), weight (Cout,Cin,3,3)) + bias (+ add), stride 1, one pixel of padding "zeros"
    | "reflect" (reflect needs H, W >= 2), output H x W.  pre_slope None: no pre-activation.  add: a tensor of the output's
    shape, added in float32 before the one rounding of a 16-bit result.
    impl "auto": a GPU map of float32 / float16 / bfloat16 runs on the kernels when no gradient can be asked for (grad mode
    off, or none of x, weight, bias, add requires one); parameters stored in another float type are packed into x's
    dtype; under torch.autocast x is cast to the autocast dtype.  Everything else -- CPU tensors, float64, a gradient
    needed, shapes the library refuses (_lib.Unsupported) -- takes the torch composition (torch_gen_conv), as "torch"
    always does.
    grad "torch" (default): as above.  "kernels": a GPU call in float32 / float16 / bfloat16 that needs a gradient runs
    GenConvFunction -- the same forward launch, and the library's data / weight / bias gradient kernels behind it; if the
    library refuses any part of that, the whole call takes the composition.  Anything else raises ValueError."""
    return _gen_conv(x, weight, bias, S1K3, padding, pre_slope, add, impl, grad)


def conv4x4_down(x, weight, bias=None, pre_slope=None, impl="auto", grad="torch", add=None):
    """conv2d(leaky_relu(x, pre_slope), weight (Cout,Cin,4,4), bias, stride=2, padding=1) (+ add): H, W >= 2, odd sizes as
    torch (output (H-2)//2+1 x (W-2)//2+1).  Dispatch as conv3x3."""
    return _gen_conv(x, weight, bias, S2K4, "zeros", pre_slope, add, impl, grad)


def conv_transpose3x3_up(x, weight, bias=None, add=None, impl="auto", pre_slope=None, grad="torch"):
    """conv_transpose2d(leaky_relu(x, pre_slope), weight (Cin,Cout,3,3), bias, stride=2, padding=1, output_padding=1)
    (+ add): output 2H x 2W, computed as four output phases of 1 / 2 / 2 / 4 taps, never on a zero-stuffed map.  Dispatch
    as conv3x3."""
    return _gen_conv(x, weight, bias, T2K3, "zeros", pre_slope, add, impl, grad)


# ---- the 1x1 convolution (csrc/conv1x1.hip; its weight and bias gradients: csrc/gen_conv_wgrad.hip) --------------------
def _packed_1x1(weight, dtype, grad):
    """torch's (Cout,Cin,1,1) `weight` packed in compute type `dtype` for the forward, or transposed for the data gradient"""
    query, pack = ("gfla_conv1x1_grad_packed_bytes", "gfla_conv1x1_pack_grad_weights_") if grad else \
        ("gfla_conv1x1_packed_bytes", "gfla_conv1x1_pack_weights_")

    def make():
        w = weight.detach().contiguous()
        esize = torch.empty((), dtype=dtype).element_size()
        packed = _lib.workspace(query, w, w.size(0), w.size(1), esize, what="conv1x1 packed weights")
        _lib.call(pack + _SFX[dtype], w, _lib.ptr(w), _SRC_TYPE[w.dtype], _lib.ptr(packed), w.size(0), w.size(1))
        return packed
    return cached(weight, "conv1x1_grad" if grad else "conv1x1", dtype, make)


def _validate_1x1(x, weight, bias, pre_slope, pool):
    """Everything that can be wrong with a conv1x1 call, before anything is launched.  Returns (Cout, Hout, Wout)."""
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError("conv1x1: a non-empty (B,Cin,H,W) map (got %s)" % (tuple(x.shape),))
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (1, 1) or weight.size(1) != x.size(1) or weight.size(0) < 1:
        raise ValueError("conv1x1: weight (Cout,Cin,1,1) with Cin = %d (got %s)" % (x.size(1), tuple(weight.shape)))
    cout = weight.size(0)
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError("conv1x1: bias (Cout,) = (%d,) (got %s)" % (cout, tuple(bias.shape)))
    if pool not in POOLS:
        raise ValueError("conv1x1: pool is 1 or 2 (got %r)" % (pool,))
    if pre_slope is not None and not float(pre_slope) >= 0:
        raise ValueError("conv1x1: pre_slope is None or a slope >= 0 (got %r)" % (pre_slope,))
    if pool == 2 and pre_slope is not None:
        raise ValueError("conv1x1: pool=2 takes no pre-activation (got pre_slope=%r)" % (pre_slope,))
    H, W = x.shape[2:]
    if pool == 2 and (H < 2 or W < 2):
        raise ValueError("conv1x1: pool=2 needs H, W >= 2 (got %s)" % (tuple(x.shape),))
    return cout, H // pool, W // pool


def torch_conv1x1(x, weight, bias=None, pre_slope=None, pool=1):
    """The composition the reference runs: F.avg_pool2d(x, 2, 2) or F.leaky_relu, then F.conv2d.  Any dtype, any device."""
    a = F.avg_pool2d(x, 2, 2) if pool == 2 else x if pre_slope is None else F.leaky_relu(x, pre_slope)
    if weight.dtype != a.dtype and not torch.is_autocast_enabled():
        weight = weight.to(a.dtype)
        bias = None if bias is None else bias.to(a.dtype)
    return F.conv2d(a, weight, bias)


def _launch_1x1(x, weight, bias, pre_slope, pool, cout, ho, wo):
    if torch.is_autocast_enabled():
        x = x.to(autocast_dtype())
    if x.dtype not in _SFX:
        raise _lib.Unsupported("conv1x1: no kernel for %s" % x.dtype)
    x = x.contiguous()
    B, Cin, H, W = x.shape
    wp = _packed_1x1(weight, x.dtype, False)
    b32 = None if bias is None else rounded_bias(bias, x.dtype, "gen_conv_b")
    y = x.new_empty((B, cout, ho, wo))
    _lib.call("gfla_conv1x1_fwd_" + _SFX[x.dtype], x, _lib.ptr(x), _lib.ptr(wp), _lib.ptr(b32), _lib.ptr(y), B, Cin, cout,
              H, W, pool, int(pre_slope is not None), float(pre_slope or 0.0))
    return y


class Conv1x1Function(Function):
    """(x, weight, bias | None, pre_slope, pool, (Cout, Hout, Wout)) -> y on the library's kernels, with the gradients of
    all three tensors; GenConvFunction's contract: x in float32 / float16 / bfloat16 on the GPU, saved for the backward are
    x and the weight and nothing else (the pooled or activated map is recomputed while the weight gradient stages it), the
    backward launches only what needs_input_grad asks for, grad_x is allocated uninitialised (the kernel writes every
    element, the zero row and column of an odd map included), no atomics.  Whatever the backward would need that the
    library refuses raises _lib.Unsupported in the forward, before anything is launched."""

    @staticmethod
    def forward(ctx, x, weight, bias, pre_slope, pool, dims):
        cout, ho, wo = dims
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and bias is not None
        B, Cin, H, W = x.shape
        if need_x or need_w or need_b:
            esize = x.element_size()
            _lib.workspace_bytes("gfla_conv1x1_bwd_workspace_bytes", B, Cin, cout, H, W, pool, esize, what="conv1x1 backward")
            _lib.workspace_bytes("gfla_conv1x1_grad_packed_bytes", cout, Cin, esize, what="conv1x1 backward")
        y = _launch_1x1(x, weight, bias, pre_slope, pool, cout, ho, wo)
        ctx.conf = (cout, pool, int(pre_slope is not None), float(pre_slope or 0.0))
        ctx.bias_dtype = None if bias is None else bias.dtype
        if need_x or need_w or need_b:
            ctx.save_for_backward(x.contiguous(), weight)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and ctx.bias_dtype is not None
        dx = dw = db = None
        if need_x or need_w or need_b:
            x, weight = ctx.saved_tensors
            cout, pool, pre_act, slope = ctx.conf
            B, Cin, H, W = x.shape
            sfx = _SFX[x.dtype]
            gy = g.to(x.dtype).contiguous()
            tail = (B, Cin, cout, H, W, pool, pre_act, slope)
            if need_x:
                dx = torch.empty_like(x)
                wp = _packed_1x1(weight, x.dtype, True)
                _lib.call("gfla_conv1x1_bwd_data_" + sfx, x, _lib.ptr(gy), _lib.ptr(x), _lib.ptr(wp), _lib.ptr(dx), *tail)
            if need_w or need_b:
                ws = _lib.workspace("gfla_conv1x1_bwd_workspace_bytes", x, B, Cin, cout, H, W, pool, x.element_size(),
                                    what="conv1x1 backward")
                dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device) if need_w else None
                db = torch.empty(cout, dtype=torch.float32, device=x.device) if need_b else None
                _lib.call("gfla_conv1x1_bwd_weight_" + sfx, x, _lib.ptr(gy), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(db),
                          _lib.ptr(ws), *tail)
                if dw is not None and dw.dtype != weight.dtype:
                    dw = dw.to(weight.dtype)
                if db is not None and db.dtype != ctx.bias_dtype:
                    db = db.to(ctx.bias_dtype)
        return dx, dw, db, None, None, None


def conv1x1(x, weight, bias=None, pre_slope=None, pool=1, impl="auto", grad="torch"):
    """conv2d(p, weight (Cout,Cin,1,1)) + bias with p = avg_pool2d(x, 2, 2) for pool=2 (H, W >= 2; output H//2 x W//2, an
    odd trailing row or column dropped as torch drops it), p = leaky_relu(x, pre_slope) or p = x for pool=1.  pool=2 with a
    pre_slope is a ValueError: no network of the reference has both.  The pooled value of a 16-bit map is the float32 sum of
    its four stored values times 0.25, rounded once while it is staged, as F.avg_pool2d hands it on.
    Dispatch as conv3x3: impl "auto" runs a GPU map of float32 / float16 / bfloat16 on the kernels when no gradient can be
    asked for; when one can, grad "torch" (default) takes the exact torch composition (torch_conv1x1: F.avg_pool2d /
    F.leaky_relu, then F.conv2d) and grad "kernels" runs Conv1x1Function -- the same forward launch with the library's
    data, weight and bias gradient kernels behind it.  CPU tensors, float64, impl "torch" and shapes the library refuses
    (_lib.Unsupported) take the composition for the whole call."""
    _lib.check_impl(impl)
    _check_grad(grad)
    dims = _validate_1x1(x, weight, bias, pre_slope, pool)
    if impl == "auto" and _kernel_inputs(x, weight, bias, None):
        try:
            if not _needs_grad(x, weight, bias):
                return _launch_1x1(x.detach(), weight, bias, pre_slope, pool, *dims)
            if grad == "kernels":
                xk = x.to(autocast_dtype()) if torch.is_autocast_enabled() else x
                if xk.dtype in _SFX:
                    return Conv1x1Function.apply(xk, weight, bias, pre_slope, pool, dims)
        except _lib.Unsupported:
            pass
    return torch_conv1x1(x, weight, bias, pre_slope, pool)


class InferenceConv(nn.Module):
    """[LeakyReLU(pre_slope)] -> [ReflectionPad2d(1)] -> the convolution `conv` (+ add) as one op.  `weight` and `bias` are
    conv's own Parameter objects under conv's names, so state dicts interchange; conv itself is kept (unregistered) and
    runs whenever the kernels do not: CPU, float64, a gradient needed (unless grad="kernels": then GenConvFunction),
    impl="torch".  geometry P1K1 (Conv2d(k 1, s 1, p 0), what fuse_inference_convs makes with pointwise=True) is conv1x1
    with pool=1, which has the same dispatch and its torch composition for everything else."""

    def __init__(self, conv, geometry, padding="zeros", pre_slope=None, impl="auto", grad="torch"):
        super(InferenceConv, self).__init__()
        _lib.check_impl(impl)
        _check_grad(grad)
        if geometry not in _NAMES or padding not in PADDINGS or (padding == "reflect" and geometry != S1K3):
            raise ValueError("InferenceConv: geometry 0 / 1 / 2 / 3, padding 'zeros' or (geometry 0) 'reflect' (got %r, %r)"
                             % (geometry, padding))
        self.geometry, self.padding, self.impl, self.grad = geometry, padding, impl, grad
        self.pre_slope = None if pre_slope is None else float(pre_slope)
        self.weight = conv.weight
        if conv.bias is not None:
            self.bias = conv.bias
        else:
            self.register_parameter("bias", None)
        self.__dict__["original"] = conv           # not a submodule: no second set of state-dict keys
        self.train(conv.training)

    def forward(self, x, add=None):
        if self.geometry == P1K1:
            y = conv1x1(x, self.weight, self.bias, self.pre_slope, 1, self.impl, self.grad)
            return y if add is None else y + add
        if self.impl == "auto" and _kernel_inputs(x, self.weight, self.bias, add):
            needs = _needs_grad(x, self.weight, self.bias, add)
            if not needs:
                return _gen_conv(x, self.weight, self.bias, self.geometry, self.padding, self.pre_slope, add, self.impl)
            if self.grad == "kernels":
                xk = x.to(autocast_dtype()) if torch.is_autocast_enabled() else x
                if xk.dtype in _SFX:
                    try:
                        dims = _validate(x, self.weight, self.bias, self.geometry, self.padding, self.pre_slope, add)
                        return GenConvFunction.apply(xk, self.weight, self.bias, add, self.geometry, self.padding,
                                                     self.pre_slope, dims)
                    except _lib.Unsupported:
                        pass
        a = x if self.pre_slope is None else F.leaky_relu(x, self.pre_slope)
        if self.padding == "reflect":
            a = F.pad(a, (1, 1, 1, 1), mode="reflect")
        conv = self.original
        if conv.weight is not self.weight or conv.bias is not self.bias:      # a conversion that replaced the Parameters
            conv.weight, conv.bias = self.weight, self.bias
        y = conv(a)
        return y if add is None else y + add

    def extra_repr(self):
        return "%s, %d -> %d, padding=%r, pre_slope=%s, impl=%r, grad=%r" % (
            _NAMES[self.geometry], self.original.in_channels, self.original.out_channels, self.padding, self.pre_slope,
            self.impl, self.grad)


def _is_reflect_pad(module):
    return type(module) is nn.ReflectionPad2d and tuple(module.padding) == (1, 1, 1, 1)


def _plain(module, cls):
    """a plain convolution the op can stand in for: its own Parameters, no hook of any kind (spectral norm recomputes the
    weight in one; any other would silently stop firing), groups 1, dilation 1"""
    if type(module) is not cls or "weight" not in module._parameters:
        return False
    if module._forward_pre_hooks or module._forward_hooks or module._backward_hooks or module._backward_pre_hooks:
        return False
    return module.groups == 1 and tuple(module.dilation) == (1, 1)


def _geometry_of(module, has_pad, pointwise=False):
    """(geometry, padding) the kernels have for `module`, or None; the 1x1 convolution only with `pointwise`"""
    if _plain(module, nn.Conv2d):
        k, s, p = tuple(module.kernel_size), tuple(module.stride), tuple(module.padding)
        if pointwise and k == (1, 1) and s == (1, 1) and p == (0, 0):
            return P1K1, "zeros"
        if k == (3, 3) and s == (1, 1) and module.out_channels > _HEAD_MAX_COUT:    # narrower ones belong to head_conv.py
            if has_pad and p == (0, 0):
                return S1K3, "reflect"
            if p == (1, 1) and module.padding_mode == "zeros":
                return S1K3, "zeros"
        if k == (4, 4) and s == (2, 2) and p == (1, 1) and module.padding_mode == "zeros":
            return S2K4, "zeros"
    if _plain(module, nn.ConvTranspose2d):
        if (tuple(module.kernel_size), tuple(module.stride), tuple(module.padding), tuple(module.output_padding)) == \
                ((3, 3), (2, 2), (1, 1), (1, 1)) and module.padding_mode == "zeros":
            return T2K3, "zeros"
    return None


def fuse_inference_convs(net, impl="auto", grad="torch", pointwise=False):
    """Rewrite, in place and recursively, the convolutions of `net` that sit in an nn.Sequential and that the kernels have:
    plain nn.Conv2d (k 3, s 1, p 1, zeros), (k 3, s 1, p 0) directly behind nn.ReflectionPad2d(1), (k 4, s 2, p 1, zeros)
    and plain nn.ConvTranspose2d (k 3, s 2, p 1, output_padding 1); with pointwise=True also plain nn.Conv2d (k 1, s 1,
    p 0), the learnable shortcut of a ResBlock (conv1x1).  The convolution's slot becomes an InferenceConv
    holding the same Parameter objects, the pad's slot nn.Identity(), and an nn.LeakyReLU directly in front of the pad or
    the convolution is folded in (its slot becomes nn.Identity(); a shared activation object is left as it is: only slots
    change).  Indices and state-dict keys do not change; a convolution also registered under another name (the
    reference's Jump keeps its own as `conv1` and `model.N`) is replaced there by the same InferenceConv.
    Left alone, uncounted: modules with any hook (spectral norm), CoordConv, groups / dilation other than 1, other padding
    modes, 1x1 convolutions unless pointwise=True, anything inside an ExtractorAttn (`fully_connect_layer`), 3x3
    convolutions of at most 8 output channels (head_conv.py's: HeadConv3x3 slots and the flow / mask heads).  grad: the
    `grad` of every InferenceConv made ("kernels": training runs on GenConvFunction).  Returns the number of convolutions
    rewritten."""
    _lib.check_impl(impl)
    _check_grad(grad)
    inside_attn = set()
    for m in net.modules():
        if hasattr(m, "fully_connect_layer"):
            inside_attn.update(id(s) for s in m.modules())
    replaced = {}
    for seq in [m for m in net.modules() if isinstance(m, nn.Sequential) and id(m) not in inside_attn]:
        names = list(seq._modules.keys())
        for i, name in enumerate(names):
            conv = seq._modules[name]
            prev = seq._modules[names[i - 1]] if i >= 1 else None
            has_pad = prev is not None and _is_reflect_pad(prev)
            found = _geometry_of(conv, has_pad, pointwise)
            if found is None or id(conv) in replaced:
                continue
            geometry, padding = found
            has_pad = padding == "reflect"
            at = i - 1 if has_pad else i
            before = seq._modules[names[at - 1]] if at >= 1 else None
            slope = float(before.negative_slope) if type(before) is nn.LeakyReLU else None
            fused = InferenceConv(conv, geometry, padding, slope, impl, grad)
            seq._modules[name] = fused
            if has_pad:
                seq._modules[names[i - 1]] = nn.Identity()
            if slope is not None:
                seq._modules[names[at - 1]] = nn.Identity()
            replaced[id(conv)] = (conv, fused)
    for m in net.modules():               # the same convolution under another name
        for name, sub in m._modules.items():
            if sub is not None and id(sub) in replaced and replaced[id(sub)][0] is sub:
                m._modules[name] = replaced[id(sub)][1]
    return len(replaced)


def _last_inference_conv(seq):
    if not isinstance(seq, nn.Sequential) or len(seq) == 0:
        return None
    last = seq[len(seq) - 1]
    return last if type(last) is InferenceConv else None


def _run_with_add(seq, x, add):
    """seq(x) with `add` handed to its last module"""
    mods = list(seq)
    for m in mods[:-1]:
        x = m(x)
    return mods[-1](x, add)


_REFERENCE_CONV_BLOCKS = ("EncoderBlock", "ResBlock", "ResBlockDecoder", "Jump")


def patch_reference_convs(base_function, impl="auto", grad="torch", pointwise=False):
    """Wrap the constructors of the reference's EncoderBlock, ResBlock, ResBlockDecoder and Jump so that every block built
    from now on comes out rewritten (fuse_inference_convs on the finished block), and replace ResBlock.forward and
    ResBlockDecoder.forward by versions that hand the residual (x, or shortcut(x)) as `add` to the last InferenceConv of
    `self.model`; whenever that slot is no InferenceConv they call the original forward.  With grad="kernels" the blocks
    train on GenConvFunction and the residual's gradient flows through its `add`.  pointwise=True: the learnable 1x1
    shortcut of a ResBlock is rewritten as well (fuse_inference_convs).  Idempotent.  Returns the names of the classes
    wrapped."""
    _check_grad(grad)
    wrapped = []
    for name in _REFERENCE_CONV_BLOCKS:
        cls = getattr(base_function, name, None)
        init = None if cls is None else cls.__dict__.get("__init__")
        if init is None:
            continue
        wrapped.append(name)
        if getattr(init, "_gfla_fuses_inference_convs", False):
            continue

        def make(orig):
            def __init__(self, *args, **kwargs):
                orig(self, *args, **kwargs)
                fuse_inference_convs(self, impl, grad, pointwise)
            __init__._gfla_fuses_inference_convs = True
            __init__.__wrapped__ = orig
            __init__.__doc__ = orig.__doc__
            return __init__
        cls.__init__ = make(init)
        if name not in ("ResBlock", "ResBlockDecoder") or "forward" not in cls.__dict__:
            continue

        def make_forward(orig, decoder):
            def forward(self, x):
                last = _last_inference_conv(self.model)
                if last is None:
                    return orig(self, x)
                if decoder or self.learnable_shortcut:
                    return _run_with_add(self.model, x, self.shortcut(x))
                return _run_with_add(self.model, x, x)
            forward._gfla_residual_in_epilogue = True
            forward.__wrapped__ = orig
            forward.__doc__ = orig.__doc__
            return forward
        cls.forward = make_forward(cls.__dict__["forward"], name == "ResBlockDecoder")
    return wrapped
