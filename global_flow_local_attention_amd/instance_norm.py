"""Fused InstanceNorm2d (+ affine) + LeakyReLU / ReLU on gfx950 (csrc/instance_norm.hip).

The reference opens every convolution of its generator blocks with `norm_layer(C) -> nonlinearity` (EncoderBlock, ResBlock,
ResBlockDecoder, ResBlockEncoder, base_function.py:334-556); the pose, face and shapenet models build them with
`nn.InstanceNorm2d(affine=True)` and `nn.LeakyReLU(0.1)` (pose_model.py:62-64).  Here the pair is one op: the forward reads
x once and writes y once, the backward reads x and dy once and writes dx once, and nothing is kept between the two but x
itself and two numbers per plane.

    InstanceNormActFunction   the autograd Function on the kernels
    instance_norm_act         functional form, with the torch composition as the other route
    InstanceNormAct           module with nn.InstanceNorm2d's parameter names
    fuse_instance_norm_act    rewrite the norm -> activation pairs of an existing network in place
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from . import _rewrite
from ._conv_common import param_grad

IMPLS = _lib.IMPLS


def _acc_dtype(dtype):
    return torch.float64 if dtype == torch.float64 else torch.float32


def _aligned(t):
    """contiguous, and on a 16-byte boundary: the tensor itself when it already is.  The kernels take any element-aligned
    pointer, but they split a plane into head / vectors / tail by x's address, and the sums regroup with it: from a copy
    the result is the same bit for bit wherever the caller's tensor starts"""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _workspace(x):
    B, C, H, W = x.shape
    return _lib.workspace("gfla_instance_norm_workspace_bytes", x, B, C, H, W, x.element_size(), what="instance_norm_act")


class InstanceNormActFunction(Function):
    """(x (B,C,H,W), weight, bias, eps, negative_slope) -> act(instance_norm(x) * weight + bias), on the library's kernels.

    x: float32 / float64 / float16 / bfloat16 on the GPU, read as stored; arithmetic is float32 (float64 for float64), the
    output has x's dtype and is rounded once.  weight / bias: None or (C,) float tensors; a float32 parameter with a 16-bit
    map is read as stored (parameters of another float type are cast to the arithmetic type, C values).
    negative_slope: None = no activation (plain instance norm), 0 = ReLU.  Statistics are per plane, biased variance, as
    nn.InstanceNorm2d without running statistics.
    Saved for the backward: x itself (no copy when it is contiguous), mean and rstd (B*C values each) and the parameters.
    The backward recomputes z from x; dx, d weight and d bias are each computed only when needed, without atomics:
    gradients are bit-identical from call to call."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, negative_slope):
        _lib.require_gpu(x, weight, bias)
        sfx = _lib.suffix(x, "instance_norm_act")
        for name, p in (("weight", weight), ("bias", bias)):
            if p is not None and not p.is_floating_point():
                raise TypeError("instance_norm_act: %s must be a float tensor (got %s)" % (name, p.dtype))
        if x.dim() != 4 or x.numel() == 0:
            raise ValueError("instance_norm_act: a non-empty (B,C,H,W) map (got %s)" % (tuple(x.shape),))
        B, C, H, W = x.shape
        if H * W == 1:
            raise ValueError("instance_norm_act: more than one value per plane is needed (got %s)" % (tuple(x.shape),))
        for name, p in (("weight", weight), ("bias", bias)):
            if p is not None and tuple(p.shape) != (C,):
                raise ValueError("instance_norm_act: %s (C,) = (%d,) (got %s)" % (name, C, tuple(p.shape)))
        if not float(eps) >= 0:
            raise ValueError("instance_norm_act: eps >= 0 (got %r)" % (eps,))
        x = _aligned(x)
        acc = _acc_dtype(x.dtype)
        w = None if weight is None else weight.detach().to(acc).contiguous()
        b = None if bias is None else bias.detach().to(acc).contiguous()
        y = torch.empty_like(x)
        mean = torch.empty(B * C, dtype=acc, device=x.device)
        rstd = torch.empty(B * C, dtype=acc, device=x.device)
        act = negative_slope is not None
        ctx.slope = float(negative_slope) if act else 0.0
        ctx.act = int(act)
        ws = _workspace(x)
        _lib.call("gfla_instance_norm_fwd_" + sfx, x, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), _lib.ptr(mean),
                  _lib.ptr(rstd), _lib.ptr(ws), B, C, H, W, float(eps), ctx.slope, ctx.act)
        need = ctx.needs_input_grad
        if need[0] or (weight is not None and need[1]) or (bias is not None and need[2]):
            ctx.has = (weight is not None, bias is not None)
            ctx.save_for_backward(x, mean, rstd, *[p for p in (weight, bias) if p is not None])
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, mean, rstd = ctx.saved_tensors[:3]
        rest = list(ctx.saved_tensors[3:])
        weight = rest.pop(0) if ctx.has[0] else None
        bias = rest.pop(0) if ctx.has[1] else None
        need_x = ctx.needs_input_grad[0]
        need_w = weight is not None and ctx.needs_input_grad[1]
        need_b = bias is not None and ctx.needs_input_grad[2]
        if not (need_x or need_w or need_b):
            return None, None, None, None, None
        B, C, H, W = x.shape
        acc = mean.dtype
        w = None if weight is None else weight.detach().to(acc).contiguous()
        b = None if bias is None else bias.detach().to(acc).contiguous()
        grad_y = _aligned(grad_y.to(x.dtype))
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty(C, dtype=acc, device=x.device) if need_w else None
        db = torch.empty(C, dtype=acc, device=x.device) if need_b else None
        ws = _workspace(x)
        _lib.call("gfla_instance_norm_bwd_" + _lib.suffix(x, "instance_norm_act"), x, _lib.ptr(x), _lib.ptr(grad_y),
                  _lib.ptr(w), _lib.ptr(b), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db),
                  _lib.ptr(ws), B, C, H, W, ctx.slope, ctx.act)
        return (dx, param_grad(dw, weight.dtype if need_w else None), param_grad(db, bias.dtype if need_b else None),
                None, None)


def torch_instance_norm_act(x, weight=None, bias=None, eps=1e-5, negative_slope=None):
    """The same map as the torch composition: F.instance_norm (no running statistics), then F.leaky_relu, or F.relu for a
    slope of 0, or nothing for None."""
    y = F.instance_norm(x, None, None, weight, bias, True, 0.0, eps)
    if negative_slope is None:
        return y
    return F.relu(y) if negative_slope == 0 else F.leaky_relu(y, negative_slope)


def _kernel_inputs(x, weight, bias):
    if not x.is_cuda or x.dtype not in _lib.SUFFIX or x.dim() != 4 or x.numel() == 0:
        return False
    return all(p is None or (p.is_cuda and p.is_floating_point()) for p in (weight, bias))


def instance_norm_act(x, weight=None, bias=None, eps=1e-5, negative_slope=None, impl="auto"):
    """act(instance_norm(x) * weight + bias) for x (B,C,H,W); negative_slope None: no activation, 0: ReLU.

    impl "auto": a GPU map of float32 / float64 / float16 / bfloat16 runs on the kernels (InstanceNormActFunction; under
    torch.autocast a float32 map stays float32, as F.instance_norm keeps it).  CPU tensors, other dtypes and shapes the
    library refuses (_lib.Unsupported) take the torch composition (torch_instance_norm_act).  "torch": always the
    composition."""
    _lib.check_impl(impl)
    if x.dim() != 4:
        raise ValueError("instance_norm_act: x (B,C,H,W) (got %s)" % (tuple(x.shape),))
    for name, p in (("weight", weight), ("bias", bias)):
        if p is not None and tuple(p.shape) != (x.size(1),):
            raise ValueError("instance_norm_act: %s (C,) = (%d,) (got %s)" % (name, x.size(1), tuple(p.shape)))
    if impl == "auto" and _kernel_inputs(x, weight, bias):
        try:
            return InstanceNormActFunction.apply(x, weight, bias, eps, negative_slope)
        except _lib.Unsupported:
            pass
    return torch_instance_norm_act(x, weight, bias, eps, negative_slope)


class InstanceNormAct(nn.Module):
    """nn.InstanceNorm2d(num_features, eps, affine) followed by LeakyReLU(negative_slope) (0: ReLU, None: nothing) as one
    op.  Parameter names are nn.InstanceNorm2d's (`weight`, `bias`, present when affine), so state dicts interchange.
    Running statistics are not supported."""

    def __init__(self, num_features, eps=1e-5, affine=False, negative_slope=None, impl="auto", track_running_stats=False):
        super(InstanceNormAct, self).__init__()
        if track_running_stats:
            raise ValueError("InstanceNormAct: track_running_stats is not supported")
        _lib.check_impl(impl)
        if int(num_features) < 1:
            raise ValueError("num_features: a positive channel count (got %r)" % (num_features,))
        if negative_slope is not None and not float(negative_slope) >= 0:
            raise ValueError("negative_slope: None or a slope >= 0 (got %r)" % (negative_slope,))
        self.num_features = int(num_features)
        self.eps = float(eps)
        self.affine = bool(affine)
        self.negative_slope = None if negative_slope is None else float(negative_slope)
        self.impl = impl
        if self.affine:
            self.weight = nn.Parameter(torch.ones(self.num_features))
            self.bias = nn.Parameter(torch.zeros(self.num_features))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)

    def forward(self, x):
        if x.dim() != 4 or x.size(1) != self.num_features:
            raise ValueError("InstanceNormAct(%d): x (B,%d,H,W) (got %s)" % (self.num_features, self.num_features,
                                                                           tuple(x.shape)))
        return instance_norm_act(x, self.weight, self.bias, self.eps, self.negative_slope, self.impl)

    def extra_repr(self):
        return "%d, eps=%g, affine=%s, negative_slope=%s, impl=%r" % (self.num_features, self.eps, self.affine,
                                                                    self.negative_slope, self.impl)


def _fusable_norm(module):
    return type(module) is nn.InstanceNorm2d and not module.track_running_stats


def _from_norm(norm, negative_slope, impl):
    fused = InstanceNormAct(norm.num_features, norm.eps, norm.affine, negative_slope, impl)
    if norm.affine:
        fused.weight, fused.bias = norm.weight, norm.bias      # the same Parameter objects
    fused.train(norm.training)
    return fused


def fuse_instance_norm_act(module, impl="auto"):
    """Rewrite, in place and recursively, every nn.Sequential of `module` in which an nn.InstanceNorm2d (without running
    statistics) is directly followed by nn.LeakyReLU or nn.ReLU: the norm's slot becomes an InstanceNormAct holding the
    same Parameter objects, the activation's slot nn.Identity().  Indices and state-dict keys do not change, and an
    activation instance shared with other places of the network (the reference passes one object around) is left as it
    is: only slots are replaced.  An nn.InstanceNorm2d of a Sequential with no activation after it becomes
    InstanceNormAct(negative_slope=None).  Anything else is left alone.  Returns the number of pairs fused."""
    _lib.check_impl(impl)
    pairs = 0
    for seq in [m for m in module.modules() if isinstance(m, nn.Sequential)]:
        names = list(seq._modules.keys())
        for i, name in enumerate(names):
            norm = seq._modules[name]
            if not _fusable_norm(norm):
                continue
            nxt = names[i + 1] if i + 1 < len(names) else None
            slope = _rewrite.slope_of(seq._modules[nxt], relu=True) if nxt is not None else None
            seq._modules[name] = _from_norm(norm, slope, impl)
            if slope is not None:
                seq._modules[nxt] = nn.Identity()
                pairs += 1
    return pairs


# the reference's block classes that build `norm_layer(C), nonlinearity, conv` sequences (base_function.py:334-556)
_REFERENCE_BLOCKS = ("EncoderBlock", "ResBlock", "ResBlockDecoder", "ResBlockEncoder")


def patch_reference_blocks(base_function, impl="auto"):
    """Wrap the constructors of the reference's block classes -- the four named above and any other class of
    `base_function` whose constructor takes `norm_layer` -- so that every block built from now on comes out fused
    (fuse_instance_norm_act on the finished block).  Idempotent.  Returns the names of the classes wrapped."""
    import inspect
    wrapped = []
    for name, cls in sorted(vars(base_function).items()):
        if not (inspect.isclass(cls) and issubclass(cls, nn.Module)) or cls.__module__ != base_function.__name__:
            continue
        init = cls.__dict__.get("__init__")
        if init is None:
            continue
        if not getattr(init, "_gfla_fuses_instance_norm", False):
            try:
                takes_norm = "norm_layer" in inspect.signature(init).parameters
            except (TypeError, ValueError):
                takes_norm = False
            if not (takes_norm or name in _REFERENCE_BLOCKS):
                continue
        _rewrite.wrap_init(cls, "_gfla_fuses_instance_norm", lambda self: fuse_instance_norm_act(self, impl))
        wrapped.append(name)
    return wrapped
