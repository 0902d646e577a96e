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

The four ops are rows of one table (_OPS); validation, the torch composition, the launch, the Function body and the
dispatch rule (run) are each written once against a row.
"""
import collections
import ctypes

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from . import _rewrite
from ._conv_common import (GRADS, P1K1, PADDINGS, S1K3, S2K4, SFX as _SFX, SRC_TYPE as _SRC_TYPE, T2K3,  # noqa: F401
                           autocast_dtype, check_conv_args, check_grad, conv_geometry, packed, param_grad, rounded_bias)
from .head_conv import MAX_COUT as _HEAD_MAX_COUT

IMPLS = _lib.IMPLS
POOLS = (1, 2)

# One kernel family as the wrappers see it.  name: in messages and reprs; k: kernel size; cin_axis: the weight's Cin axis;
# modes(padding, pool): the integers its launching entry points and its workspace query take after (B, Cin, Cout, H, W);
# pack_modes: those its pack entry points and packed-bytes queries take after (Cout, Cin); has_add: the forward takes an
# addend; data_ws: the data gradient takes the workspace (then one allocation serves both gradient calls).
_Op = collections.namedtuple("_Op", "name geometry k cin_axis modes pack_modes has_add data_ws fwd bwd_data bwd_weight "
                                    "pack pack_grad packed_bytes grad_packed_bytes bwd_workspace_bytes")
_GEN_ENTRIES = dict(fwd="gfla_gen_conv_fwd_", bwd_data="gfla_gen_conv_bwd_data_", bwd_weight="gfla_gen_conv_bwd_weight_",
                    pack="gfla_gen_conv_pack_weights_", pack_grad="gfla_gen_conv_pack_grad_weights_",
                    packed_bytes="gfla_gen_conv_packed_bytes", grad_packed_bytes="gfla_gen_conv_grad_packed_bytes",
                    bwd_workspace_bytes="gfla_gen_conv_bwd_workspace_bytes")
_OPS = {g: _Op(name, g, k, cin_axis, lambda padding, pool, g=g: (g, PADDINGS.index(padding)), (g,), True, True,
               **_GEN_ENTRIES)
        for g, name, k, cin_axis in ((S1K3, "conv3x3", 3, 1), (S2K4, "conv4x4_down", 4, 1),
                                     (T2K3, "conv_transpose3x3_up", 3, 0))}
_OPS[P1K1] = _Op("conv1x1", P1K1, 1, 1, lambda padding, pool: (pool,), (), False, False,
                 fwd="gfla_conv1x1_fwd_", bwd_data="gfla_conv1x1_bwd_data_", bwd_weight="gfla_conv1x1_bwd_weight_",
                 pack="gfla_conv1x1_pack_weights_", pack_grad="gfla_conv1x1_pack_grad_weights_",
                 packed_bytes="gfla_conv1x1_packed_bytes", grad_packed_bytes="gfla_conv1x1_grad_packed_bytes",
                 bwd_workspace_bytes="gfla_conv1x1_bwd_workspace_bytes")


def out_size(geometry, H, W):
    """(Hout, Wout) of a geometry (gfla_gen_conv_out_size)"""
    ho, wo = ctypes.c_int64(), ctypes.c_int64()
    status = _lib.lib().gfla_gen_conv_out_size(int(geometry), int(H), int(W), ctypes.addressof(ho), ctypes.addressof(wo))
    if status != 0:
        raise ValueError("%s: no output for a %d x %d map (%s)" % (_OPS[geometry].name if geometry in _OPS else "gen_conv",
                                                                  H, W, _lib.lib().gfla_status_string(status).decode()))
    return ho.value, wo.value


def _packed(op, weight, dtype, grad):
    """`weight` packed in compute type `dtype` for op's forward, or (`grad`) for its data gradient: the adjoint geometry"""
    if grad:
        return packed(weight, dtype, op.name + " gradient", op.grad_packed_bytes, op.pack_grad, op.pack_modes, op.cin_axis)
    return packed(weight, dtype, op.name, op.packed_bytes, op.pack, op.pack_modes, op.cin_axis)


def packed_weights(weight, dtype, geometry):
    """torch's `weight` ((Cout,Cin,k,k); T2K3: (Cin,Cout,3,3)) packed in compute type `dtype`, once per frozen parameter."""
    return _packed(_OPS[geometry], weight, dtype, False)


def _validate(op, x, weight, bias, padding, pre_slope, add, pool):
    """Everything that can be wrong with a call, before anything is launched.  Returns (Cout, Hout, Wout)."""
    name = op.name
    cout = check_conv_args(name, x, weight, bias, op.k, padding, pre_slope, op.cin_axis)
    H, W = x.shape[2:]
    if op.geometry == P1K1:
        if pool not in POOLS:
            raise ValueError("%s: pool is 1 or 2 (got %r)" % (name, pool))
        if pool == 2 and pre_slope is not None:
            raise ValueError("%s: pool=2 takes no pre-activation (got pre_slope=%r)" % (name, pre_slope))
        if pool == 2 and (H < 2 or W < 2):
            raise ValueError("%s: pool=2 needs H, W >= 2 (got %s)" % (name, tuple(x.shape)))
    if op.geometry == S2K4 and (H < 2 or W < 2):
        raise ValueError("%s: H, W >= 2 (got %s)" % (name, tuple(x.shape)))
    ho, wo = {S1K3: (H, W), S2K4: ((H - 2) // 2 + 1, (W - 2) // 2 + 1), T2K3: (2 * H, 2 * W),
              P1K1: (H // pool, W // pool)}[op.geometry]
    if add is not None and tuple(add.shape) != (x.size(0), cout, ho, wo):
        raise ValueError("%s: add has the output's shape %s (got %s)" % (name, (x.size(0), cout, ho, wo), tuple(add.shape)))
    return cout, ho, wo


def _composition(op, x, weight, bias, padding, pre_slope, pool):
    """The composition the reference runs for `op`, without the addend.  Any dtype, any device."""
    a = F.avg_pool2d(x, 2, 2) if pool == 2 else x if pre_slope is None else F.leaky_relu(x, pre_slope)
    if weight.dtype != a.dtype and not torch.is_autocast_enabled():
        weight = weight.to(a.dtype)
        bias = None if bias is None else bias.to(a.dtype)
    if op.geometry == T2K3:
        return F.conv_transpose2d(a, weight, bias, stride=2, padding=1, output_padding=1)
    if op.geometry == S1K3 and padding == "reflect":
        return F.conv2d(F.pad(a, (1, 1, 1, 1), mode="reflect"), weight, bias)
    stride, pad = {S1K3: (1, 1), S2K4: (2, 1), P1K1: (1, 0)}[op.geometry]
    return F.conv2d(a, weight, bias, stride=stride, padding=pad)


def torch_gen_conv(x, weight, bias, geometry, padding="zeros", pre_slope=None, add=None):
    """The same map as the composition the reference runs: F.leaky_relu, F.pad(mode="reflect") or the convolution's own
    zero padding, F.conv2d / F.conv_transpose2d, + add.  Any dtype, any device."""
    y = _composition(_OPS[geometry], x, weight, bias, padding, pre_slope, 1)
    return y if add is None else y + add


def torch_conv1x1(x, weight, bias=None, pre_slope=None, pool=1):
    """The composition the reference runs: F.avg_pool2d(x, 2, 2) or F.leaky_relu, then F.conv2d.  Any dtype, any device."""
    return _composition(_OPS[P1K1], x, weight, bias, "zeros", pre_slope, pool)


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


def _launch(op, modes, x, weight, bias, add, pre_slope, dims):
    if torch.is_autocast_enabled():
        x = x.to(autocast_dtype())
    if x.dtype not in _SFX:
        raise _lib.Unsupported("%s: no kernel for %s" % (op.name, x.dtype))
    x = x.contiguous()
    B, Cin, H, W = x.shape
    cout, ho, wo = dims
    wp = _packed(op, weight, x.dtype, False)
    b32 = None if bias is None else rounded_bias(bias, x.dtype, "gen_conv_b")
    if add is not None:
        add = add.detach().to(x.dtype).contiguous()
    y = x.new_empty((B, cout, ho, wo))
    _lib.call(op.fwd + _SFX[x.dtype], x, _lib.ptr(x), _lib.ptr(wp), _lib.ptr(b32), *((_lib.ptr(add),) if op.has_add else ()),
              _lib.ptr(y), B, Cin, cout, H, W, *modes, int(pre_slope is not None), float(pre_slope or 0.0))
    return y


def _forward(ctx, op, modes, x, weight, bias, add, pre_slope, dims):
    """The forward of both Functions.  The first inputs of either are (x, weight, bias): needs_input_grad[:3]."""
    cout = dims[0]
    need_x, need_w, need_b = ctx.needs_input_grad[:3]
    need_b = need_b and bias is not None
    B, Cin, H, W = x.shape
    if need_x or need_w or need_b:      # what the backward will ask the library for: refused now, nothing is launched
        esize = x.element_size()
        _lib.workspace_bytes(op.bwd_workspace_bytes, B, Cin, cout, H, W, *modes, esize, what=op.name + " backward")
        _lib.workspace_bytes(op.grad_packed_bytes, cout, Cin, *op.pack_modes, esize, what=op.name + " backward")
    y = _launch(op, modes, x, weight, bias, add, pre_slope, dims)
    ctx.op, ctx.cout = op, cout
    ctx.tail = modes + (int(pre_slope is not None), float(pre_slope or 0.0))
    ctx.bias_dtype = None if bias is None else bias.dtype
    ctx.add_dtype = None if add is None else add.dtype
    if need_x or need_w or need_b:
        ctx.save_for_backward(x.contiguous(), weight)
    return y


def _backward(ctx, g):
    """The backward of both Functions: (grad x, grad weight, grad bias, grad add)"""
    op = ctx.op
    need_x, need_w, need_b = ctx.needs_input_grad[:3]
    need_b = need_b and ctx.bias_dtype is not None
    g_add = g.to(ctx.add_dtype) if op.has_add and ctx.needs_input_grad[3] and ctx.add_dtype is not None else None
    dx = dw = db = None
    if need_x or need_w or need_b:
        x, weight = ctx.saved_tensors
        B, Cin, H, W = x.shape
        cout, sfx = ctx.cout, _SFX[x.dtype]
        gy = g.to(x.dtype).contiguous()
        tail = (B, Cin, cout, H, W) + ctx.tail

        def workspace():
            return _lib.workspace(op.bwd_workspace_bytes, x, *tail[:-2], x.element_size(), what=op.name + " backward")
        ws = workspace() if op.data_ws else None
        if need_x:
            dx = torch.empty_like(x)
            wp = _packed(op, weight, x.dtype, True)
            _lib.call(op.bwd_data + sfx, x, _lib.ptr(gy), _lib.ptr(x), _lib.ptr(wp), _lib.ptr(dx),
                      *((_lib.ptr(ws),) if op.data_ws else ()), *tail)
        if need_w or need_b:
            if ws is None:
                ws = workspace()
            dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device) if need_w else None
            db = torch.empty(cout, dtype=torch.float32, device=x.device) if need_b else None
            _lib.call(op.bwd_weight + sfx, x, _lib.ptr(gy), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), *tail)
            dw, db = param_grad(dw, weight.dtype), param_grad(db, ctx.bias_dtype)
    return dx, dw, db, g_add


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
        op = _OPS[geometry]
        return _forward(ctx, op, op.modes(padding, 1), x, weight, bias, add, pre_slope, dims)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return _backward(ctx, g) + (None, None, None, None)


class Conv1x1Function(Function):
    """(x, weight, bias | None, pre_slope, pool, (Cout, Hout, Wout)) -> y on the library's kernels, with the gradients of
    all three tensors; GenConvFunction's contract: x in float32 / float16 / bfloat16 on the GPU, saved for the backward are
    x and the weight and nothing else (the pooled or activated map is recomputed while the weight gradient stages it), the
    backward launches only what needs_input_grad asks for, grad_x is allocated uninitialised (the kernel writes every
    element, the zero row and column of an odd map included), no atomics.  Whatever the backward would need that the
    library refuses raises _lib.Unsupported in the forward, before anything is launched."""

    @staticmethod
    def forward(ctx, x, weight, bias, pre_slope, pool, dims):
        return _forward(ctx, _OPS[P1K1], (pool,), x, weight, bias, None, pre_slope, dims)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return _backward(ctx, g)[:3] + (None, None, None)


def run(geometry, x, weight, bias, padding, pre_slope, add, pool, impl, grad, otherwise=None):
    """The dispatch rule of the four ops, once.  impl "auto" and inputs the kernels take: no gradient needed -> the
    launch on x detached; one needed and grad "kernels" -> the op's Function on x cast as autocast would cast it;
    _lib.Unsupported from either, and everything else -> otherwise(x), the caller's own convolution without the addend,
    or (None) the functional composition.  The functional forms are checked in full before anything runs, as they always
    were; a caller with a convolution of its own leaves what the kernels do not take to that convolution's checks.
    geometry None (no kernel for the caller's convolution) is otherwise(x) + add.  An addend the op does not take (conv1x1)
    is added to whatever ran, here and nowhere else."""
    op = _OPS.get(geometry)
    y = fused = dims = None
    if op is not None:
        fused = add if op.has_add else None
        if otherwise is None:
            dims = _validate(op, x, weight, bias, padding, pre_slope, fused, pool)
        if impl == "auto" and _kernel_inputs(x, weight, bias, fused):
            needs = _needs_grad(x, weight, bias, fused)
            if not needs or grad == "kernels":
                try:
                    if dims is None:
                        dims = _validate(op, x, weight, bias, padding, pre_slope, fused, pool)
                    # the cast is the caller's, outside the Function: a float32 x gets a float32 gradient through it
                    xk = x.detach() if not needs else x.to(autocast_dtype()) if torch.is_autocast_enabled() else x
                    if not needs:
                        y = _launch(op, op.modes(padding, pool), xk, weight, bias, fused, pre_slope, dims)
                    elif op.has_add:
                        y = GenConvFunction.apply(xk, weight, bias, fused, geometry, padding, pre_slope, dims)
                    else:
                        y = Conv1x1Function.apply(xk, weight, bias, pre_slope, pool, dims)
                except _lib.Unsupported:
                    pass
    if y is None:
        fused = None
        y = otherwise(x) if otherwise is not None else _composition(op, x, weight, bias, padding, pre_slope, pool)
    return y if add is fused else y + add


def _functional(geometry, x, weight, bias, padding, pre_slope, add, pool, impl, grad):
    _lib.check_impl(impl)
    check_grad(grad)
    return run(geometry, x, weight, bias, padding, pre_slope, add, pool, impl, grad)


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
    return _functional(S1K3, x, weight, bias, padding, pre_slope, add, 1, impl, grad)


def conv4x4_down(x, weight, bias=None, pre_slope=None, impl="auto", grad="torch", add=None):
    """conv2d(leaky_relu(x, pre_slope), weight (Cout,Cin,4,4), bias, stride=2, padding=1) (+ add): H, W >= 2, odd sizes as
    torch (output (H-2)//2+1 x (W-2)//2+1).  Dispatch as conv3x3."""
    return _functional(S2K4, x, weight, bias, "zeros", pre_slope, add, 1, impl, grad)


def conv_transpose3x3_up(x, weight, bias=None, add=None, impl="auto", pre_slope=None, grad="torch"):
    """conv_transpose2d(leaky_relu(x, pre_slope), weight (Cin,Cout,3,3), bias, stride=2, padding=1, output_padding=1)
    (+ add): output 2H x 2W, computed as four output phases of 1 / 2 / 2 / 4 taps, never on a zero-stuffed map.  Dispatch
    as conv3x3."""
    return _functional(T2K3, x, weight, bias, "zeros", pre_slope, add, 1, impl, grad)


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
    return _functional(P1K1, x, weight, bias, "zeros", pre_slope, None, pool, impl, grad)


class InferenceConv(nn.Module):
    """[LeakyReLU(pre_slope)] -> [ReflectionPad2d(1)] -> the convolution `conv` (+ add) as one op.  `weight` and `bias` are
    conv's own Parameter objects under conv's names, so state dicts interchange; conv itself is kept (unregistered) and
    runs whenever the kernels do not: CPU, float64, a gradient needed (unless grad="kernels": then GenConvFunction),
    impl="torch".  geometry P1K1 (Conv2d(k 1, s 1, p 0), what fuse_inference_convs makes with pointwise=True) is conv1x1
    with pool=1, which has the same dispatch and its torch composition for everything else."""

    fuses_add = True                           # _rewrite.epilogue_slot: forward(x, add) adds in the kernel's epilogue

    def __init__(self, conv, geometry, padding="zeros", pre_slope=None, impl="auto", grad="torch"):
        super(InferenceConv, self).__init__()
        _lib.check_impl(impl)
        check_grad(grad)
        if geometry not in _OPS or padding not in PADDINGS or (padding == "reflect" and geometry != S1K3):
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

    def _original(self, x):
        a = x if self.pre_slope is None else F.leaky_relu(x, self.pre_slope)
        if self.padding == "reflect":
            a = F.pad(a, (1, 1, 1, 1), mode="reflect")
        conv = self.original
        if conv.weight is not self.weight or conv.bias is not self.bias:      # a conversion that replaced the Parameters
            conv.weight, conv.bias = self.weight, self.bias
        return conv(a)

    def forward(self, x, add=None):
        return run(self.geometry, x, self.weight, self.bias, self.padding, self.pre_slope, add, 1, self.impl, self.grad,
                    None if self.geometry == P1K1 else self._original)

    def extra_repr(self):
        return "%s, %d -> %d, padding=%r, pre_slope=%s, impl=%r, grad=%r" % (
            _OPS[self.geometry].name, self.original.in_channels, self.original.out_channels, self.padding, self.pre_slope,
            self.impl, self.grad)


def fuse_inference_convs(net, impl="auto", grad="torch", pointwise=False):
    """Rewrite, in place and recursively, the convolutions of `net` that sit in an nn.Sequential and that the kernels have:
    plain nn.Conv2d (k 3, s 1, p 1, zeros), (k 3, s 1, p 0) directly behind nn.ReflectionPad2d(1), (k 4, s 2, p 1, zeros)
    and plain nn.ConvTranspose2d (k 3, s 2, p 1, output_padding 1); with pointwise=True also plain nn.Conv2d (k 1, s 1,
    p 0), the learnable shortcut of a ResBlock (conv1x1).  The convolution's slot becomes an InferenceConv
    holding the same Parameter objects, the pad's slot nn.Identity(), and an nn.LeakyReLU directly in front of the pad or
    the convolution is folded in (its slot becomes nn.Identity(); a shared activation object is left as it is: only slots
    change).  Indices and state-dict keys do not change; a convolution also registered under another name (the
    reference's Jump keeps its own as `conv1` and `model.N`) is replaced there by the same InferenceConv.
    Left alone, uncounted: modules with any hook (spectral norm: spectral_norm.fuse_spectral_norm rewrites those), CoordConv, groups / dilation other than 1, other padding
    modes, 1x1 convolutions unless pointwise=True, anything inside an ExtractorAttn (`fully_connect_layer`), 3x3
    convolutions of at most 8 output channels (head_conv.py's: HeadConv3x3 slots and the flow / mask heads).  grad: the
    `grad` of every InferenceConv made ("kernels": training runs on GenConvFunction).  Returns the number of convolutions
    rewritten."""
    _lib.check_impl(impl)
    check_grad(grad)
    inside_attn = set()
    for m in net.modules():
        if hasattr(m, "fully_connect_layer"):
            inside_attn.update(id(s) for s in m.modules())
    replaced = {}
    for seq in [m for m in net.modules() if isinstance(m, nn.Sequential) and id(m) not in inside_attn]:
        names = list(seq._modules.keys())
        for i, name in enumerate(names):
            conv = seq._modules[name]
            found = conv_geometry(conv, i >= 1 and _rewrite.is_reflect_pad(seq._modules[names[i - 1]]))
            if found is None or id(conv) in replaced or not _rewrite.plain(conv):
                continue
            geometry, padding = found
            if (geometry == P1K1 and not pointwise) or (geometry == S1K3 and conv.out_channels <= _HEAD_MAX_COUT):
                continue                  # the narrow 3x3 ones belong to head_conv.py
            at = i - 1 if padding == "reflect" else i
            slope = _rewrite.slope_of(seq._modules[names[at - 1]], relu=False) if at >= 1 else None
            fused = InferenceConv(conv, geometry, padding, slope, impl, grad)
            seq._modules[name] = fused
            if padding == "reflect":
                seq._modules[names[i - 1]] = nn.Identity()
            if slope is not None:
                seq._modules[names[at - 1]] = nn.Identity()
            replaced[id(conv)] = (conv, fused)
    _rewrite.replace_aliases(net, replaced)
    return len(replaced)


def install_residual_forwards(base_function):
    """Replace ResBlock.forward and ResBlockDecoder.forward of the reference's base_function (base_function.py:386-391,
    529-531) by versions that hand the residual (x, or shortcut(x)) as `add` to the last slot of `self.model` when
    _rewrite.epilogue_slot finds one there -- an InferenceConv, a SpectralConv on a kernel geometry or a
    SpectralConvTranspose on the transposed 3x3 kernels --; otherwise they call the original forward.  One flag
    (`_gfla_residual_in_epilogue`) whoever installs them: idempotent.  Returns the names of the classes found."""
    def make_forward(orig, decoder):
        def forward(self, x):
            if _rewrite.epilogue_slot(self.model) is None:
                return orig(self, x)
            if decoder or self.learnable_shortcut:
                return _rewrite.run_with_add(self.model, x, self.shortcut(x))
            return _rewrite.run_with_add(self.model, x, x)
        return forward
    return [name for name in ("ResBlock", "ResBlockDecoder")
            if _rewrite.wrap_method(getattr(base_function, name, None), "forward", "_gfla_residual_in_epilogue",
                                    lambda orig, decoder=name == "ResBlockDecoder": make_forward(orig, decoder))]


_REFERENCE_CONV_BLOCKS = ("EncoderBlock", "ResBlock", "ResBlockDecoder", "Jump")


def patch_reference_convs(base_function, impl="auto", grad="torch", pointwise=False):
    """Wrap the constructors of the reference's EncoderBlock, ResBlock, ResBlockDecoder and Jump so that every block built
    from now on comes out rewritten (fuse_inference_convs on the finished block), and replace ResBlock.forward and
    ResBlockDecoder.forward by versions that hand the residual (x, or shortcut(x)) as `add` to the last slot of `self.model`
    when it adds in its epilogue (install_residual_forwards); otherwise they call the original forward.  With grad="kernels" the blocks
    train on GenConvFunction and the residual's gradient flows through its `add`.  pointwise=True: the learnable 1x1
    shortcut of a ResBlock is rewritten as well (fuse_inference_convs).  Idempotent.  Returns the names of the classes
    wrapped."""
    check_grad(grad)
    wrapped = []
    for name in _REFERENCE_CONV_BLOCKS:
        cls = getattr(base_function, name, None)
        if not _rewrite.wrap_init(cls, "_gfla_fuses_inference_convs",
                                  lambda self: fuse_inference_convs(self, impl, grad, pointwise)):
            continue
        wrapped.append(name)
    install_residual_forwards(base_function)
    return wrapped
