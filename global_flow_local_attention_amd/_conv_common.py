"""Plumbing shared by the implicit-GEMM convolutions (vgg.py, gen_conv.py; csrc/conv_igemm.h): the dtype tables, the cache
of packed weights and rounded biases of frozen parameters, and the autocast dtype."""
import weakref

import torch

SFX = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}        # entry-point suffix of a compute type
SRC_TYPE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}                # `src_type` of the pack entry points
# packed weights and rounded biases of frozen parameters: (data_ptr, _version, dtype, device, shape, what) ->
# (weak reference to the parameter, tensor); `what` names the caller and the layout
_PACK_CACHE = {}
_PACK_CACHE_MAX = 512


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


def autocast_dtype():                       # the dtype torch.autocast casts GPU convolutions to
    get = getattr(torch, "get_autocast_dtype", None)
    return get("cuda") if get is not None else torch.get_autocast_gpu_dtype()
