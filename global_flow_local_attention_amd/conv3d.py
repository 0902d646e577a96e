"""The 3-D convolutions of the video discriminator on the library's own kernels, on FRAMES-MAJOR activations
(csrc/conv3d.hip, csrc/gen_conv_wgrad.hip, csrc/avg_pool_frames.hip; include/gfla_conv3d.h).

The two ResBlock3DEncoder of the reference's TemporalDiscriminator (base_function.py:43-67) are built from Conv3d(k (3,3,3),
s 1, p 1), Conv3d(k (3,4,4), s (1,2,2), p (0,1,1)) and a shortcut of AvgPool3d((3,2,2), (1,2,2)) and a 1x1x1 convolution.
With the activations kept as (B, L, C, H, W) instead of torch's (B, C, L, H, W) every frame is an NCHW sample and the three
frames a temporal tap window covers are one contiguous (3 C, H, W) map: a Conv3d of temporal stride 1 is then a 2-D
convolution over a sliding channel window, one launch of the implicit-GEMM kernels of gen_conv.py per call, nothing
unfolded, no rounding between the temporal taps.

    to_frames_major, from_frames_major          (B,C,L,H,W) <-> (B,L,C,H,W), plain permute copies
    conv3d_frames, avg_pool_frames              functional forms
    Conv3dFramesFunction, AvgPoolFramesFunction the autograd Functions on the kernels (grad="kernels")
    torch_conv3d_frames, torch_avg_pool_frames  the torch compositions: permute -> F.conv3d / F.avg_pool3d -> permute

Dispatch is gen_conv.py's: impl "auto" runs a GPU map of float32 / float16 / bfloat16 on the kernels when no gradient can
be asked for; when one can, grad "torch" (the default) takes the torch composition and grad "kernels" the Function.  CPU
tensors, float64, impl="torch" and shapes the library refuses (_lib.Unsupported) take the composition for the whole call.
"""
import ctypes

import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from ._conv_common import SFX as _SFX, SRC_TYPE as _SRC_TYPE, autocast_dtype, cached, check_grad, param_grad, rounded_bias

IMPLS = _lib.IMPLS
# the `geometry` of the gfla_conv3d_* entry points; each is the 2-D geometry of the same number per frame window
K333, K344 = 0, 1
GEOMETRIES = ("k333", "k344")
KT = 3                                        # temporal kernel size of both
_K = {K333: 3, K344: 4}                       # spatial kernel size
_STRIDE = {K333: (1, 1, 1), K344: (1, 2, 2)}
_PADDING = {K333: (1, 1, 1), K344: (0, 1, 1)}


def _geometry(geometry):
    if geometry in GEOMETRIES:
        return GEOMETRIES.index(geometry)
    raise ValueError("geometry: one of %s (got %r)" % (GEOMETRIES, geometry))


def to_frames_major(x):
    """torch's (B, C, L, H, W) as a contiguous (B, L, C, H, W): one permute copy"""
    if x.dim() != 5:
        raise ValueError("to_frames_major: a (B,C,L,H,W) map (got %s)" % (tuple(x.shape),))
    return x.permute(0, 2, 1, 3, 4).contiguous()


def from_frames_major(x):
    """a (B, L, C, H, W) map as torch's contiguous (B, C, L, H, W): one permute copy"""
    if x.dim() != 5:
        raise ValueError("from_frames_major: a (B,L,C,H,W) map (got %s)" % (tuple(x.shape),))
    return x.permute(0, 2, 1, 3, 4).contiguous()


class _ContiguousGrad(Function):
    """Identity whose gradient arrives contiguous.  The compositions permute torch's result back to frames-major; without
    this the convolution's backward would be handed a permuted view of the frames-major gradient, and torch's reductions
    (the bias gradient) walk a strided tensor in another order than the contiguous one the reference's network gives them:
    with it the composition on the host is the hooked network bit for bit, gradients included."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.contiguous()


def frames_major_result(y):
    """torch's (B,C,L,H,W) result of a composition as a contiguous frames-major map (see _ContiguousGrad)"""
    return from_frames_major(_ContiguousGrad.apply(y) if y.requires_grad else y)


def out_size(geometry, L, H, W):
    """(Lout, Hout, Wout) of a geometry (gfla_conv3d_out_size)"""
    g = _geometry(geometry)
    lo, ho, wo = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    status = _lib.lib().gfla_conv3d_out_size(g, int(L), int(H), int(W), ctypes.addressof(lo), ctypes.addressof(ho),
                                             ctypes.addressof(wo))
    if status != 0:
        raise ValueError("conv3d_frames %s: no output for %d frames of %d x %d (%s)"
                         % (geometry, L, H, W, _lib.lib().gfla_status_string(status).decode()))
    return lo.value, ho.value, wo.value


def _validate(g, x, weight, bias, pre_slope, add):
    """Everything that can be wrong with a call, before anything is launched.  Returns (Cout, Lout, Hout, Wout)."""
    name, k = "conv3d_frames " + GEOMETRIES[g], _K[g]
    if x.dim() != 5 or x.numel() == 0:
        raise ValueError("%s: a non-empty frames-major (B,L,C,H,W) map (got %s)" % (name, tuple(x.shape)))
    B, L, C, H, W = x.shape
    if weight.dim() != 5 or tuple(weight.shape[1:]) != (C, KT, k, k) or weight.size(0) < 1:
        raise ValueError("%s: weight (Cout,C,%d,%d,%d) with C = %d (got %s)" % (name, KT, k, k, C, tuple(weight.shape)))
    cout = weight.size(0)
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError("%s: bias (Cout,) = (%d,) (got %s)" % (name, cout, tuple(bias.shape)))
    if g == K344 and (L < KT or H < 2 or W < 2):
        raise ValueError("%s: L >= 3 and H, W >= 2 (got %s)" % (name, tuple(x.shape)))
    if pre_slope is not None and not float(pre_slope) >= 0:
        raise ValueError("%s: pre_slope is None or a slope >= 0 (got %r)" % (name, pre_slope))
    lo, ho, wo = (L, H, W) if g == K333 else (L - 2, (H - 2) // 2 + 1, (W - 2) // 2 + 1)
    if add is not None and tuple(add.shape) != (B, lo, cout, ho, wo):
        raise ValueError("%s: add has the output's shape %s (got %s)" % (name, (B, lo, cout, ho, wo), tuple(add.shape)))
    return cout, lo, ho, wo


def torch_conv3d_frames(x, weight, bias=None, geometry="k333", pre_slope=None, add=None):
    """The composition the reference runs, on a frames-major map: F.leaky_relu, permute, F.conv3d with the geometry's
    stride and padding, permute back, + add.  Any dtype, any device."""
    g = _geometry(geometry)
    a = x if pre_slope is None else F.leaky_relu(x, pre_slope)
    if weight.dtype != a.dtype and not torch.is_autocast_enabled():
        weight = weight.to(a.dtype)
        bias = None if bias is None else bias.to(a.dtype)
    y = frames_major_result(F.conv3d(a.permute(0, 2, 1, 3, 4), weight, bias, stride=_STRIDE[g], padding=_PADDING[g]))
    return y if add is None else y + add


def torch_avg_pool_frames(x):
    """permute -> F.avg_pool3d(kernel (3,2,2), stride (1,2,2)) -> permute on a frames-major map.  Any dtype, any device."""
    return frames_major_result(F.avg_pool3d(x.permute(0, 2, 1, 3, 4), (3, 2, 2), (1, 2, 2)))


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _kernel_inputs(x, weight=None, bias=None, add=None):
    if not x.is_cuda or not x.is_floating_point() or x.dtype == torch.float64:
        return False
    if x.dtype not in _SFX and not torch.is_autocast_enabled():
        return False
    for p in (weight, bias):
        if p is not None and (not p.is_cuda or p.dtype not in _SRC_TYPE):
            return False
    return add is None or (add.is_cuda and add.is_floating_point() and add.dtype != torch.float64)


def _packed(g, weight, dtype, grad):
    """torch's Conv3d `weight` (Cout,C,3,k,k) packed in compute type `dtype` for the forward -- reduced channel kt C + c,
    (Cout, 3 C, k, k) -- or (`grad`) for the data gradient: the temporal taps reversed on the rows, (3 Cout, C, k, k).  The
    2-D family's own pack entry points, on the permuted weight."""
    cout, c = weight.size(0), weight.size(1)
    esize = torch.empty((), dtype=dtype).element_size()
    what = "conv3d_frames %s%s" % (GEOMETRIES[g], " gradient" if grad else "")

    def make():
        w = weight.detach()
        if grad:
            w = w.flip(2).permute(2, 0, 1, 3, 4).contiguous()
            rows, cols, query, pack = KT * cout, c, "gfla_gen_conv_grad_packed_bytes", "gfla_gen_conv_pack_grad_weights_"
        else:
            w = w.permute(0, 2, 1, 3, 4).contiguous()
            rows, cols, query, pack = cout, KT * c, "gfla_gen_conv_packed_bytes", "gfla_gen_conv_pack_weights_"
        buf = _lib.workspace(query, w, rows, cols, g, esize, what=what + " packed weights")
        _lib.call(pack + _SFX[dtype], w, _lib.ptr(w), _SRC_TYPE[w.dtype], _lib.ptr(buf), rows, cols, g)
        return buf
    return cached(weight, what, dtype, make)


def _launch(g, x, weight, bias, add, pre_slope, dims):
    if torch.is_autocast_enabled():
        x = x.to(autocast_dtype())
    if x.dtype not in _SFX:
        raise _lib.Unsupported("conv3d_frames: no kernel for %s" % x.dtype)
    x = x.contiguous()
    B, L, C, H, W = x.shape
    cout, lo, ho, wo = dims
    wp = _packed(g, weight, x.dtype, False)
    b32 = None if bias is None else rounded_bias(bias, x.dtype, "gen_conv_b")
    if add is not None:
        add = add.detach().to(x.dtype).contiguous()
    y = x.new_empty((B, lo, cout, ho, wo))
    _lib.call("gfla_conv3d_fwd_" + _SFX[x.dtype], x, _lib.ptr(x), _lib.ptr(wp), _lib.ptr(b32), _lib.ptr(add), _lib.ptr(y),
              B, L, C, cout, H, W, g, int(pre_slope is not None), float(pre_slope or 0.0))
    return y


class Conv3dFramesFunction(Function):
    """(x, weight, bias | None, add | None, geometry number, pre_slope, (Cout, Lout, Hout, Wout)) -> y on the library's
    kernels, with the gradients of all four tensors; GenConvFunction's contract.  x: frames-major (B,L,C,H,W) in float32 /
    float16 / bfloat16 on the GPU; weight in torch's Conv3d layout.  Saved for the backward: x and the weight, nothing
    else.  The backward launches only what needs_input_grad asks for: the windowed data gradient (x's dtype), the windowed
    weight gradient (float32 (Cout, 3 C, k, k), permuted back to the weight's layout and rounded once to its dtype) and the
    bias gradient; the addend's gradient is grad_y in the addend's dtype.  No atomics: bit-identical from call to call.
    Whatever the backward would need that the library refuses raises _lib.Unsupported in the forward, before anything is
    launched."""

    @staticmethod
    def forward(ctx, x, weight, bias, add, g, pre_slope, dims):
        cout = dims[0]
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and bias is not None
        B, L, C, H, W = x.shape
        if need_x or need_w or need_b:
            esize = x.element_size()
            _lib.workspace_bytes("gfla_conv3d_bwd_workspace_bytes", B, L, C, cout, H, W, g, esize,
                                 what="conv3d_frames backward")
            _lib.workspace_bytes("gfla_gen_conv_grad_packed_bytes", KT * cout, C, g, esize, what="conv3d_frames backward")
        y = _launch(g, x, weight, bias, add, pre_slope, dims)
        ctx.g, ctx.cout = g, cout
        ctx.tail = (g, int(pre_slope is not None), float(pre_slope or 0.0))
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.add_dtype = None if add is None else add.dtype
        if need_x or need_w or need_b:
            ctx.save_for_backward(x.contiguous(), weight)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and ctx.bias_dtype is not None
        g_add = grad.to(ctx.add_dtype) if ctx.needs_input_grad[3] and ctx.add_dtype is not None else None
        dx = dw = db = None
        if need_x or need_w or need_b:
            x, weight = ctx.saved_tensors
            B, L, C, H, W = x.shape
            cout, sfx, g = ctx.cout, _SFX[x.dtype], ctx.g
            gy = grad.to(x.dtype).contiguous()
            sizes = (B, L, C, cout, H, W)
            if need_x:
                dx = torch.empty_like(x)
                wp = _packed(g, weight, x.dtype, True)
                _lib.call("gfla_conv3d_bwd_data_" + sfx, x, _lib.ptr(gy), _lib.ptr(x), _lib.ptr(wp), _lib.ptr(dx), *sizes,
                          *ctx.tail)
            if need_w or need_b:
                ws = _lib.workspace("gfla_conv3d_bwd_workspace_bytes", x, *sizes, g, x.element_size(),
                                    what="conv3d_frames backward")
                k = _K[g]
                dw = torch.empty((cout, KT, C, k, k), dtype=torch.float32, device=x.device) if need_w else None
                db = torch.empty(cout, dtype=torch.float32, device=x.device) if need_b else None
                _lib.call("gfla_conv3d_bwd_weight_" + sfx, x, _lib.ptr(gy), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(db),
                          _lib.ptr(ws), *sizes, *ctx.tail)
                if dw is not None:
                    dw = dw.permute(0, 2, 1, 3, 4).contiguous()           # (Cout, 3, C, k, k) -> torch's (Cout, C, 3, k, k)
                dw, db = param_grad(dw, weight.dtype), param_grad(db, ctx.bias_dtype)
        return dx, dw, db, g_add, None, None, None


def conv3d_frames(x, weight, bias=None, geometry="k333", pre_slope=None, add=None, grad="torch", impl="auto"):
    """conv3d(leaky_relu(x, pre_slope), weight) + bias (+ add) on a frames-major map x (B,L,C,H,W) -> (B,Lout,Cout,Hout,Wout).
    weight: torch's Conv3d layout (Cout,C,3,k,k), as stored.
    geometry "k333": kernel (3,3,3), stride 1, padding (1,1,1), the output has x's frames and size.
    geometry "k344": kernel (3,4,4), stride (1,2,2), padding (0,1,1): L - 2 frames of (H-2)//2+1 x (W-2)//2+1; needs L >= 3
    and H, W >= 2.
    pre_slope None: no pre-activation.  add: a tensor of the output's shape, added in float32 before the one rounding of a
    16-bit result.  impl and grad: as gen_conv.conv3x3 -- "auto" runs a GPU map of float32 / float16 / bfloat16 on the
    kernels when no gradient can be asked for, and with grad "kernels" Conv3dFramesFunction when one can; everything else
    takes torch_conv3d_frames.  Anything else raises ValueError."""
    _lib.check_impl(impl)
    check_grad(grad)
    g = _geometry(geometry)
    dims = _validate(g, x, weight, bias, pre_slope, add)
    y = None
    if impl == "auto" and _kernel_inputs(x, weight, bias, add):
        needs = _needs_grad(x, weight, bias, add)
        if not needs or grad == "kernels":
            try:
                # the cast is the caller's, outside the Function: a float32 x gets a float32 gradient through it
                xk = x.detach() if not needs else x.to(autocast_dtype()) if torch.is_autocast_enabled() else x
                if not needs:
                    y = _launch(g, xk, weight, bias, add, pre_slope, dims)
                else:
                    y = Conv3dFramesFunction.apply(xk, weight, bias, add, g, pre_slope, dims)
            except _lib.Unsupported:
                y = None
    if y is None:
        y = torch_conv3d_frames(x, weight, bias, geometry, pre_slope, add)
    return y


def _pool_launch(name, src, out_shape):
    B, L, C, H, W = out_shape if name == "bwd" else src.shape
    out = src.new_empty(out_shape)
    _lib.call("gfla_avg_pool_frames_%s_%s" % (name, _SFX[src.dtype]), src, _lib.ptr(src), _lib.ptr(out), B, L, C, H, W)
    return out


class AvgPoolFramesFunction(Function):
    """x (B,L,C,H,W) -> the 3 x 2 x 2 mean (B,L-2,C,H//2,W//2) on the library's kernels, with x's gradient: owner-computes,
    every element of grad_x written once (the zero row and column of an odd map included), no atomics.  Saves nothing."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        B, L, C, H, W = x.shape
        ctx.shape = tuple(x.shape)
        return _pool_launch("fwd", x, (B, L - 2, C, H // 2, W // 2))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return _pool_launch("bwd", grad.contiguous(), ctx.shape)


def avg_pool_frames(x, grad="torch", impl="auto"):
    """avg_pool3d(kernel (3,2,2), stride (1,2,2)) of a frames-major map x (B,L,C,H,W) -> (B,L-2,C,H//2,W//2); needs L >= 3
    and H, W >= 2.  One float32 sum of the twelve stored values in a fixed order, times 1/12, rounded once.  Dispatch as
    conv3d_frames; the composition is torch_avg_pool_frames."""
    _lib.check_impl(impl)
    check_grad(grad)
    if x.dim() != 5 or x.numel() == 0 or x.size(1) < KT or x.size(3) < 2 or x.size(4) < 2:
        raise ValueError("avg_pool_frames: a frames-major (B,L,C,H,W) map with L >= 3 and H, W >= 2 (got %s)"
                         % (tuple(x.shape),))
    if impl == "auto" and _kernel_inputs(x) and x.dtype in _SFX:
        needs = _needs_grad(x)
        if not needs or grad == "kernels":
            try:
                return AvgPoolFramesFunction.apply(x if needs else x.detach())
            except _lib.Unsupported:
                pass
    return torch_avg_pool_frames(x)
