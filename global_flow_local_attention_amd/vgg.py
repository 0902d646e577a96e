"""VGG19 feature extractor on the library's own kernels (csrc/conv3x3.hip on csrc/conv_igemm.h, csrc/maxpool2x2.hip).

The reference builds its extractor from torchvision (`VGG19`, external_function.py:323-444): sixteen 3x3 convolutions
with ReLU and four 2x2 max pools, frozen, which VGGLoss / StyleLoss / PerceptualLoss / PerceptualCorrectness push two
images through on every step.  `VGG19Features` is that network with the reference's module names, slicing and
state-dict keys, running `conv3x3 + bias + ReLU` as an implicit GEMM on the matrix cores and the pools on their own
kernels: no vendor convolution library on the path.  Weights are not part of this package: load a state dict saved from
the reference's class (`load_state_dict`, strict) or torchvision's (`load_torchvision_state_dict`).
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from ._conv_common import SFX as _SFX, SRC_TYPE as _SRC_TYPE, autocast_dtype, packed, rounded_bias

IMPLS = _lib.IMPLS

# torchvision's configuration E: index in `features` of every convolution, by stage; a pool closes stages 1-4
_CONV_INDEX = ((0, 2), (5, 7), (10, 12, 14, 16), (19, 21, 23, 25), (28, 30, 32, 34))
_POOL_INDEX = (4, 9, 18, 27)
# the reference's slicing (:348-394): module name -> the `features` indices it holds.  features[12:14] and [14:16] both
# land in relu3_2 and relu3_3 stays empty (:363-370), so relu3_2 is the third convolution of stage 3.
_SLICES = (("relu1_1", (0, 1)), ("relu1_2", (2, 3)), ("relu2_1", (4, 5, 6)), ("relu2_2", (7, 8)),
           ("relu3_1", (9, 10, 11)), ("relu3_2", (12, 13, 14, 15)), ("relu3_3", ()), ("relu3_4", (16, 17)),
           ("relu4_1", (18, 19, 20)), ("relu4_2", (21, 22)), ("relu4_3", (23, 24)), ("relu4_4", (25, 26)),
           ("relu5_1", (27, 28, 29)), ("relu5_2", (30, 31)), ("relu5_3", (32, 33)), ("relu5_4", (34, 35)))
LAYERS = tuple(name for name, _ in _SLICES)


def packed_weights(weight, dtype, layout):
    """`weight` (Cout,Cin,3,3) packed for the kernels in compute type `dtype`: layout 0 for the forward, 1 for the data
    gradient (taps mirrored, Cin and Cout swapped).  Cached per parameter: a frozen network packs once."""
    return packed(weight, dtype, "w%d" % layout, "gfla_conv3x3_packed_bytes", "gfla_conv3x3_pack_weights_", (layout,))


class Conv3x3ReluFunction(Function):
    """(x (B,Cin,H,W), weight (Cout,Cin,3,3), bias (Cout,)) -> relu(conv2d(x, weight, bias, stride 1, padding 1)) on the
    matrix cores (csrc/conv3x3.hip).  x: float32 / float16 / bfloat16 on the GPU, read as stored; sums are float32, a
    16-bit result is rounded once.  Parameters stored in another float type are packed into x's dtype.  Only d/dx exists
    (the extractor is frozen): dx = conv3x3(g [not y <= 0], weight mirrored), launched only when x needs a gradient;
    otherwise nothing is saved.  A NaN sum stays NaN through the ReLU and passes its gradient on, as torch.relu does."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _lib.require_gpu(x, weight, bias)
        if x.dtype not in _SFX or weight.dtype not in _SRC_TYPE or bias.dtype not in _SRC_TYPE:
            raise TypeError("conv3x3_relu: float32, float16 or bfloat16 (got %s, %s, %s)" % (x.dtype, weight.dtype, bias.dtype))
        if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[1:]) != (x.size(1), 3, 3) or \
                tuple(bias.shape) != (weight.size(0),):
            raise ValueError("conv3x3_relu: x (B,Cin,H,W), weight (Cout,Cin,3,3), bias (Cout,) (got %s, %s, %s)"
                             % (tuple(x.shape), tuple(weight.shape), tuple(bias.shape)))
        if x.numel() == 0:
            raise ValueError("conv3x3_relu: empty input %s" % (tuple(x.shape),))
        x = x.contiguous()
        B, Cin, H, W = x.shape
        Cout = weight.size(0)
        wp, b32 = packed_weights(weight, x.dtype, 0), rounded_bias(bias, x.dtype, "b")
        y = x.new_empty((B, Cout, H, W))
        _lib.call("gfla_conv3x3_relu_fwd_" + _SFX[x.dtype], x, _lib.ptr(x), _lib.ptr(wp), _lib.ptr(b32), _lib.ptr(y), B, Cin,
                  Cout, H, W)
        if ctx.needs_input_grad[0]:
            ctx.weight = weight
            ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (y,) = ctx.saved_tensors
        B, Cout, H, W = y.shape
        Cin = ctx.weight.size(1)
        grad_y = grad_y.to(y.dtype).contiguous()
        wp = packed_weights(ctx.weight, y.dtype, 1)
        grad_x = y.new_empty((B, Cin, H, W))
        _lib.call("gfla_conv3x3_relu_bwd_data_" + _SFX[y.dtype], y, _lib.ptr(grad_y), _lib.ptr(y), _lib.ptr(wp),
                  _lib.ptr(grad_x), B, Cin, Cout, H, W)
        return grad_x, None, None


class MaxPool2x2Function(Function):
    """x (B,C,H,W) -> max_pool2d(x, 2, 2), floor mode, on csrc/maxpool2x2.hip.  The backward finds each window's winner
    again from x (no index tensor) and writes every element of dx once; ties go to the first maximum in scan order."""

    @staticmethod
    def forward(ctx, x):
        _lib.require_gpu(x)
        if x.dtype not in _SFX:
            raise TypeError("maxpool2x2: float32, float16 or bfloat16 (got %s)" % x.dtype)
        if x.dim() != 4 or x.numel() == 0:
            raise ValueError("maxpool2x2: a non-empty (B,C,H,W) map (got %s)" % (tuple(x.shape),))
        x = x.contiguous()
        B, C, H, W = x.shape
        y = x.new_empty((B, C, H // 2, W // 2))
        if y.numel():      # H or W of 1: an empty map, nothing to launch
            _lib.call("gfla_maxpool2x2_fwd_" + _SFX[x.dtype], x, _lib.ptr(x), _lib.ptr(y), B, C, H, W)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        (x,) = ctx.saved_tensors
        B, C, H, W = x.shape
        grad_y = grad_y.to(x.dtype).contiguous()
        grad_x = torch.empty_like(x)
        _lib.call("gfla_maxpool2x2_bwd_" + _SFX[x.dtype], x, _lib.ptr(x), _lib.ptr(grad_y) if grad_y.numel() else None,
                  _lib.ptr(grad_x), B, C, H, W)
        return grad_x


def conv3x3_relu(x, weight, bias, impl="auto"):
    """relu(conv2d(x, weight, bias, stride=1, padding=1)).  impl "auto": a GPU map of float32 / float16 / bfloat16 with
    frozen float parameters runs on the kernels (Conv3x3ReluFunction).  CPU tensors, float64, a weight or bias that
    requires a gradient, and shapes the library refuses (_lib.Unsupported) take the torch composition.  "torch": always
    the composition."""
    _lib.check_impl(impl)
    if impl == "auto" and x.is_cuda and weight.is_cuda and bias.is_cuda and x.dtype in _SFX and x.numel() > 0 and \
            weight.dtype in _SRC_TYPE and bias.dtype in _SRC_TYPE and not (weight.requires_grad or bias.requires_grad):
        try:
            return Conv3x3ReluFunction.apply(x, weight, bias)
        except _lib.Unsupported:
            pass
    if weight.dtype != x.dtype and not torch.is_autocast_enabled():
        weight, bias = weight.to(x.dtype), bias.to(x.dtype)
    return F.relu(F.conv2d(x, weight, bias, stride=1, padding=1))


def maxpool2x2(x, impl="auto"):
    """max_pool2d(x, kernel_size=2, stride=2).  impl "auto": GPU maps of float32 / float16 / bfloat16 run on the kernels
    (MaxPool2x2Function); anything else, and "torch", take F.max_pool2d."""
    _lib.check_impl(impl)
    if impl == "auto" and x.is_cuda and x.dtype in _SFX and x.dim() == 4 and x.numel() > 0:
        try:
            return MaxPool2x2Function.apply(x)
        except _lib.Unsupported:
            pass
    return F.max_pool2d(x, kernel_size=2, stride=2)


class _Conv(nn.Conv2d):
    """a 3x3 convolution of the extractor: nn.Conv2d's parameters and state-dict keys; the ReLU that follows it in
    `features` is fused into its call"""

    def __init__(self, cin, cout, impl):
        super(_Conv, self).__init__(cin, cout, kernel_size=3, stride=1, padding=1)
        self.impl = impl

    def forward(self, x):
        return conv3x3_relu(x, self.weight, self.bias, self.impl)


class _Relu(nn.Module):
    """placeholder for the ReLU of `features` (already applied by the convolution before it)"""

    def forward(self, x):
        return x


class _Pool(nn.Module):
    def __init__(self, impl):
        super(_Pool, self).__init__()
        self.impl = impl

    def forward(self, x):
        return maxpool2x2(x, self.impl)


class VGG19Features(nn.Module):
    """The reference's `VGG19` (external_function.py:323-444): image (B,3,H,W) -> {relu1_1 .. relu5_4: feature map}.

    Module names, slicing and state-dict keys are the reference's (`relu1_1.0.weight` ... `relu5_4.34.bias`), so a state
    dict saved from its class loads with strict=True; `out['relu3_3'] is out['relu3_2']`, the third convolution of stage
    3, as there.  Parameters are frozen (requires_grad=False) and start from nn.Conv2d's random initialisation: load
    weights before use.  `widths`: channels of the five stages (tests use narrow networks).  `impl`: "auto" (the
    library's kernels on the GPU) or "torch" (F.conv2d / F.max_pool2d).  The network follows the image's dtype; under
    torch.autocast a GPU image is cast to the autocast dtype and the 16-bit kernels run, as F.conv2d would."""

    def __init__(self, widths=(64, 128, 256, 512, 512), impl="auto"):
        super(VGG19Features, self).__init__()
        _lib.check_impl(impl)
        if len(widths) != 5 or any(int(w) < 1 for w in widths):
            raise ValueError("widths: five positive channel counts (got %r)" % (widths,))
        self._impl = impl
        self.widths = tuple(int(w) for w in widths)
        features, cin = {}, 3
        for stage, convs in enumerate(_CONV_INDEX):
            for i in convs:
                features[i] = _Conv(cin, self.widths[stage], impl)
                features[i + 1] = _Relu()
                cin = self.widths[stage]
        for i in _POOL_INDEX:
            features[i] = _Pool(impl)
        for name, idx in _SLICES:
            seq = nn.Sequential()
            for i in idx:
                seq.add_module(str(i), features[i])
            setattr(self, name, seq)
        for p in self.parameters():
            p.requires_grad = False

    @property
    def impl(self):
        return self._impl

    @impl.setter
    def impl(self, value):
        _lib.check_impl(value)
        self._impl = value
        for m in self.modules():
            if isinstance(m, (_Conv, _Pool)):
                m.impl = value

    def forward(self, image):
        if image.is_cuda and torch.is_autocast_enabled():
            image = image.to(autocast_dtype())
        out, x = {}, image
        for name in LAYERS:
            x = getattr(self, name)(x)
            out[name] = x
        return out

    def load_torchvision_state_dict(self, state_dict):
        """Load torchvision's vgg19 weights: keys `features.N.weight` / `features.N.bias` or bare `N.*`; classifier
        entries are ignored."""
        convs = {i for stage in _CONV_INDEX for i in stage}
        where = {i: name for name, idx in _SLICES for i in idx if i in convs}
        own = {}
        for key, value in state_dict.items():
            parts = key.split(".")
            if parts[0] == "features":
                parts = parts[1:]
            if len(parts) != 2 or not parts[0].isdigit() or parts[1] not in ("weight", "bias"):
                continue
            i = int(parts[0])
            if i not in where:
                raise KeyError("not a convolution of vgg19.features: %r" % key)
            own["%s.%d.%s" % (where[i], i, parts[1])] = value
        return self.load_state_dict(own, strict=True)
