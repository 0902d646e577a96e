"""What the convolution wrappers share (vgg.py, gen_conv.py, head_conv.py, spectral_norm.py, instance_norm.py; the kernels:
csrc/conv_igemm.h): the dtype tables, the cache of packed weights and rounded biases with the one pack function, the
autocast dtype, the geometries the generator kernels have and the classifier of an nn.Conv2d / nn.ConvTranspose2d into
them, the argument checks the convolutions have in common, the `grad` check and the rounding of a parameter's gradient."""
import weakref

import torch
from torch import nn

from . import _lib

SFX = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}        # entry-point suffix of a compute type
SRC_TYPE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}                # `src_type` of the pack entry points
# packed weights and rounded biases of frozen parameters: (data_ptr, _version, dtype, device, shape, what) ->
# (weak reference to the parameter, tensor); `what` names the caller and the layout
_PACK_CACHE = {}
_PACK_CACHE_MAX = 512
PADDINGS = ("zeros", "reflect")
GRADS = ("torch", "kernels")
# the `geometry` of the gfla_gen_conv_* entry points, and P1K1: the wrappers' name for Conv2d(k 1, s 1, p 0), which has
# entry points of its own (gfla_conv1x1_*) and is never a C `geometry`
S1K3, S2K4, T2K3, P1K1 = 0, 1, 2, 3


def cached(param, what, dtype, make):
    key = (param.data_ptr(), param._version, dtype, param.device, tuple(param.shape), what)
    hit = _PACK_CACHE.get(key)
    if hit is not None and hit[0]() is param:
        return hit[1]
    if len(_PACK_CACHE) >= _PACK_CACHE_MAX:
        _PACK_CACHE.clear()
    value = make()
    _PACK_CACHE[key] = (weakref.ref(param), value)
    return value


def rounded_bias(bias, dtype, what):        # the bias as the kernel reads it: rounded to `dtype`, held in float32
    return cached(bias, what, dtype, lambda: bias.detach().to(dtype).float().contiguous())


def packed(weight, dtype, what, query, pack, modes=(), cin_axis=1):
    """torch's `weight` (Cin on axis `cin_axis`, Cout on the other of the first two) packed in compute type `dtype` by the
    entry point `pack` + suffix into the bytes `query` asks for; `modes`: the integers both take after (Cout, Cin).
    Cached under `what`, which names the caller and the layout, on the parameter's version: a frozen network packs once,
    a stepped optimizer repacks."""
    def make():
        w = weight.detach().contiguous()
        cout, cin = w.size(1 - cin_axis), w.size(cin_axis)
        esize = torch.empty((), dtype=dtype).element_size()
        buf = _lib.workspace(query, w, cout, cin, *modes, esize, what=what + " packed weights")
        _lib.call(pack + SFX[dtype], w, _lib.ptr(w), SRC_TYPE[w.dtype], _lib.ptr(buf), cout, cin, *modes)
        return buf
    return cached(weight, what, dtype, make)


def autocast_dtype():                       # the dtype torch.autocast casts GPU convolutions to
    get = getattr(torch, "get_autocast_dtype", None)
    return get("cuda") if get is not None else torch.get_autocast_gpu_dtype()


def check_grad(grad):
    if grad not in GRADS:
        raise ValueError("grad: one of %s (got %r)" % (GRADS, grad))


def param_grad(grad, dtype):                # a float32 gradient sum, rounded once to the parameter's dtype
    return grad if grad is None or grad.dtype == dtype else grad.to(dtype)


def conv_geometry(module, has_pad=False):
    """(geometry, padding) the kernels have for the convolution `module`, or None -- by its class, kernel size, stride,
    padding, output padding, padding mode, groups and dilation alone; whose Parameters and hooks it has is the caller's
    question.  has_pad: an nn.ReflectionPad2d(1) stands directly in front, which makes Conv2d(k 3, s 1, p 0) the
    reflect-padded S1K3."""
    if type(module) not in (nn.Conv2d, nn.ConvTranspose2d) or module.groups != 1 or tuple(module.dilation) != (1, 1):
        return None
    k, s, p = tuple(module.kernel_size), tuple(module.stride), tuple(module.padding)
    zeros = module.padding_mode == "zeros"
    if type(module) is nn.ConvTranspose2d:
        return (T2K3, "zeros") if (k, s, p, tuple(module.output_padding), zeros) == ((3, 3), (2, 2), (1, 1), (1, 1), True) \
            else None
    if k == (1, 1) and s == (1, 1) and p == (0, 0):
        return P1K1, "zeros"
    if k == (3, 3) and s == (1, 1) and has_pad and p == (0, 0):
        return S1K3, "reflect"
    if k == (3, 3) and s == (1, 1) and p == (1, 1) and zeros:
        return S1K3, "zeros"
    if k == (4, 4) and s == (2, 2) and p == (1, 1) and zeros:
        return S2K4, "zeros"
    return None


def check_conv_args(name, x, weight, bias, k, padding, pre_slope, cin_axis=1):
    """What can be wrong with the arguments every k x k convolution here takes, as `name`'s ValueError.  Returns Cout."""
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError("%s: a non-empty (B,Cin,H,W) map (got %s)" % (name, tuple(x.shape)))
    if padding not in PADDINGS:
        raise ValueError("%s: padding is one of %s (got %r)" % (name, PADDINGS, padding))
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (k, k) or weight.size(cin_axis) != x.size(1) or \
            weight.size(1 - cin_axis) < 1:
        raise ValueError("%s: weight %s with Cin = %d (got %s)" % (
            name, "(Cin,Cout,%d,%d)" % (k, k) if cin_axis == 0 else "(Cout,Cin,%d,%d)" % (k, k), x.size(1),
            tuple(weight.shape)))
    cout = weight.size(1 - cin_axis)
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError("%s: bias (Cout,) = (%d,) (got %s)" % (name, cout, tuple(bias.shape)))
    if padding == "reflect" and (x.size(2) < 2 or x.size(3) < 2):
        raise ValueError("%s: reflect padding of one pixel needs H, W >= 2 (got %s)" % (name, tuple(x.shape)))
    if pre_slope is not None and not float(pre_slope) >= 0:
        raise ValueError("%s: pre_slope is None or a slope >= 0 (got %r)" % (name, pre_slope))
    return cout
