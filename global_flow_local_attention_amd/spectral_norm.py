"""Spectral normalisation as one batched op (csrc/spectral_norm.hip), and the discriminators' convolutions on the library's
own kernels.

torch.nn.utils.spectral_norm is a forward pre-hook: per convolution and per forward it runs three gemv, two
normalisations, a dot and a division.  Here all normalised convolutions of a network are one call of a fixed number of
launches, and what they convolve with is an ordinary tensor, so their 3x3 and 4x4 stride-2 convolutions run through
gen_conv.py, forward and backward -- and with pointwise="kernels" the 1x1 ones as well, the AvgPool2d(2) in front of a
shortcut folded into the convolution (gen_conv.conv1x1).

    spectral_normalize      the functional form over a batch of (weight, u, v)
    SpectralNormFunction    the autograd Function on the kernels
    SpectralConv            module with the hooked convolution's Parameters, buffers and names
    fuse_spectral_norm      rewrite the hooked convolutions of a network in place
    patch_reference_discriminators   the reference's discriminators, rewritten as they are built

Float32 parameters on the GPU run on the kernels (under torch.autocast as well: parameters stay float32).  CPU tensors,
float64, 16-bit parameters and impl="torch" take the torch composition: the operations of the hook's compute_weight in
the hook's order, so on the CPU it is bit-identical to the hook.
"""
import ctypes

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from . import _rewrite
from . import gen_conv as _gc
from ._conv_common import P1K1, S1K3, S2K4, check_grad, conv_geometry

POINTWISE = ("torch", "kernels")
_TABLE_CACHE = {}
_TABLE_CACHE_MAX = 64


class _Table(object):
    """The device table of a batch (include/gfla_spectral_norm.h) with the host numbers that go with it."""

    def __init__(self, weights, us, vs):
        n = len(weights)
        self.n = n
        self.shapes = [tuple(w.shape) for w in weights]
        self.dims = (ctypes.c_int64 * (2 * n))()
        for i, w in enumerate(weights):
            self.dims[2 * i], self.dims[2 * i + 1] = w.size(0), w.numel() // max(w.size(0), 1)
        offsets, totals = (ctypes.c_int64 * (3 * n))(), (ctypes.c_int64 * 2)()
        status = _lib.lib().gfla_spectral_norm_layout(ctypes.addressof(self.dims), n, ctypes.addressof(offsets),
                                                      ctypes.addressof(totals))
        if status != 0:
            err = _lib.Unsupported if status == _lib._ERR_UNSUPPORTED else ValueError
            raise err("spectral_normalize: %s" % _lib.lib().gfla_status_string(status).decode())
        self.elems, self.vecs = int(totals[0]), int(totals[1])
        self.elem_off = [int(offsets[3 * i]) for i in range(n)]
        self.bwd_scratch = int(_lib.lib().gfla_spectral_norm_bwd_scratch_floats(ctypes.addressof(self.dims), n))
        rows = [[w.data_ptr(), u.data_ptr(), v.data_ptr(), self.dims[2 * i], self.dims[2 * i + 1], offsets[3 * i],
                 offsets[3 * i + 1], offsets[3 * i + 2]] for i, (w, u, v) in enumerate(zip(weights, us, vs))]
        self.device = weights[0].device
        self.table = torch.tensor(rows, dtype=torch.int64).to(self.device)

    def dims_ptr(self):
        return ctypes.c_void_p(ctypes.addressof(self.dims))


def _table(weights, us, vs):
    """the table of this batch: built once, rebuilt only when a pointer or a shape changes"""
    key = tuple((w.data_ptr(), u.data_ptr(), v.data_ptr(), tuple(w.shape)) for w, u, v in zip(weights, us, vs))
    key = (weights[0].device, key)
    hit = _TABLE_CACHE.get(key)
    if hit is None:
        if len(_TABLE_CACHE) >= _TABLE_CACHE_MAX:
            _TABLE_CACHE.clear()
        hit = _TABLE_CACHE[key] = _Table(weights, us, vs)
    return hit


class SpectralNormFunction(Function):
    """(table, power_iterations, eps, *weight_origs) -> (*W_sn) on the library's kernels: the whole batch in
    2 power_iterations + 1 launches (2 in eval mode), the backward in 2.  u and v, the buffers the table points at, are
    updated in place.  Saved per call: the u, v and sigma the outputs were computed with (written by the forward's own
    launches), so that a backward after a later forward -- D(real), D(fake), one backward -- uses its own call's values."""

    @staticmethod
    def forward(ctx, table, power_iterations, eps, *weights):
        dev = table.device
        needs = any(ctx.needs_input_grad[3:])
        flat = torch.empty(table.elems, dtype=torch.float32, device=dev)
        sigma = torch.empty(table.n, dtype=torch.float32, device=dev)
        saved = torch.empty(table.vecs, dtype=torch.float32, device=dev) if needs else None
        scratch = torch.empty(table.vecs, dtype=torch.float32, device=dev)
        _lib.call("gfla_spectral_norm_fwd_f32", flat, _lib.ptr(table.table), table.dims_ptr(), table.n, _lib.ptr(flat),
                  _lib.ptr(sigma), _lib.ptr(saved), _lib.ptr(scratch), int(power_iterations), float(eps))
        ctx.table = table
        ctx.sigma = sigma
        if needs:
            ctx.save_for_backward(saved, sigma, *weights)     # the weights: autograd's version check; read through the table
        return tuple(flat[o:o + w.numel()].view(w.shape) for o, w in zip(table.elem_off, weights))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        table = ctx.table
        saved, sigma = ctx.saved_tensors[:2]
        parts = [torch.zeros(int(torch.Size(s).numel()), dtype=torch.float32, device=table.device) if g is None
                 else g.to(torch.float32).reshape(-1) for g, s in zip(grads, table.shapes)]
        grad_sn = parts[0].contiguous() if len(parts) == 1 else torch.cat(parts)
        grad_w = torch.empty(table.elems, dtype=torch.float32, device=table.device)
        scratch = torch.empty(max(table.bwd_scratch, 1), dtype=torch.float32, device=table.device)
        _lib.call("gfla_spectral_norm_bwd_f32", grad_w, _lib.ptr(table.table), table.dims_ptr(), table.n, _lib.ptr(grad_sn),
                  _lib.ptr(saved), _lib.ptr(sigma), _lib.ptr(grad_w), _lib.ptr(scratch))
        out = [grad_w[o:o + torch.Size(s).numel()].view(s) if need else None
               for o, s, need in zip(table.elem_off, table.shapes, ctx.needs_input_grad[3:])]
        return (None, None, None) + tuple(out)


def torch_spectral_normalize(weight, u, v, power_iterations=1, eps=1e-12):
    """One weight by the operations of torch's SpectralNorm.compute_weight (dim 0), in its order; u and v in place."""
    weight_mat = weight.reshape(weight.size(0), -1)
    if power_iterations > 0:
        with torch.no_grad():
            for _ in range(power_iterations):
                v = F.normalize(torch.mv(weight_mat.t(), u), dim=0, eps=eps, out=v)
                u = F.normalize(torch.mv(weight_mat, v), dim=0, eps=eps, out=u)
            u = u.clone(memory_format=torch.contiguous_format)
            v = v.clone(memory_format=torch.contiguous_format)
    sigma = torch.dot(u, torch.mv(weight_mat, v))
    return weight / sigma


def _kernel_batch(weights, us, vs):
    dev = weights[0].device
    for w, u, v in zip(weights, us, vs):
        for t in (w, u, v):
            if not t.is_cuda or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
                return False
    return True


def spectral_normalize(weights, us, vs, power_iterations=1, eps=1e-12, impl="auto"):
    """[W / sigma for every weight (Cout, ...) of `weights`], with `power_iterations` rounds of the power iteration on the
    vectors us[i] (Cout) and vs[i] (the rest), updated in place; 0 (eval mode) leaves them untouched.  Arithmetic and
    gradient (u, v, sigma constants) as torch.nn.utils.spectral_norm with dim 0.
    impl "auto": contiguous float32 GPU tensors run as ONE batched call on the kernels (SpectralNormFunction); anything
    else -- CPU, float64, 16-bit, sizes the library refuses -- and impl "torch" take torch_spectral_normalize per weight."""
    _lib.check_impl(impl)
    weights, us, vs = list(weights), list(us), list(vs)
    if not (len(weights) == len(us) == len(vs)) or not weights:
        raise ValueError("spectral_normalize: as many us and vs as weights, at least one (got %d, %d, %d)"
                         % (len(weights), len(us), len(vs)))
    if int(power_iterations) < 0 or not float(eps) > 0:
        raise ValueError("spectral_normalize: power_iterations >= 0 and eps > 0 (got %r, %r)" % (power_iterations, eps))
    for w, u, v in zip(weights, us, vs):
        if w.dim() < 1 or w.numel() == 0 or tuple(u.shape) != (w.size(0),) or tuple(v.shape) != (w.numel() // w.size(0),):
            raise ValueError("spectral_normalize: weight (R, ...), u (R,), v (K,) (got %s, %s, %s)"
                             % (tuple(w.shape), tuple(u.shape), tuple(v.shape)))
    if impl == "auto" and _kernel_batch(weights, us, vs):
        try:
            return list(SpectralNormFunction.apply(_table(weights, us, vs), int(power_iterations), float(eps), *weights))
        except _lib.Unsupported:
            pass
    return [torch_spectral_normalize(w, u, v, int(power_iterations), float(eps)) for w, u, v in zip(weights, us, vs)]


def _check_pointwise(pointwise):
    if pointwise not in POINTWISE:
        raise ValueError("pointwise: one of %s (got %r)" % (POINTWISE, pointwise))


def _is_pool2(module):
    """nn.AvgPool2d(2, 2): what conv1x1's pool=2 computes"""
    def pair(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    return type(module) is nn.AvgPool2d and pair(module.kernel_size) == (2, 2) and pair(module.stride) == (2, 2) and \
        pair(module.padding) == (0, 0) and not module.ceil_mode and module.divisor_override is None


class SpectralConv(nn.Module):
    """[LeakyReLU(pre_slope)] -> the convolution `conv` under torch's spectral_norm hook (+ add), with the normalisation
    on the batched op.  `weight_orig`, `bias`, `weight_u` and `weight_v` are conv's own Parameter and buffer objects under
    conv's names and in conv's order, so state dicts interchange with the hooked form in both directions;
    n_power_iterations and eps are the hook's.  Training mode iterates, eval mode does not.
    Conv2d(k 3, s 1, p 1) and Conv2d(k 4, s 2, p 1) run through gen_conv.conv3x3 / conv4x4_down (grad="kernels": the
    library's gradient kernels; the normalised weight's gradient comes back through SpectralNormFunction).  Conv2d(k 1,
    s 1, p 0) runs through gen_conv.conv1x1 with pointwise="kernels" -- `pool` 2: behind the AvgPool2d(2) that
    fuse_spectral_norm folded in, which needs that route --, and with the default pointwise="torch" through F.conv2d on the
    normalised weight, as every other geometry does (groups, dilation, k 4 with s 1).
    Inside a forward of a network rewritten by fuse_spectral_norm the weight was normalised with all the others in one
    call; called on its own, the module normalises itself, a batch of one."""

    def __init__(self, conv, pre_slope=None, impl="auto", grad="torch", pointwise="torch", pool=1):
        super(SpectralConv, self).__init__()
        _lib.check_impl(impl)
        check_grad(grad)
        _check_pointwise(pointwise)
        hook = _rewrite.spectral_norm_hook(conv)
        if type(conv) is not nn.Conv2d or hook is None:
            raise ValueError("SpectralConv: an nn.Conv2d under torch.nn.utils.spectral_norm (name 'weight', dim 0) and no "
                             "other hook")
        self.impl, self.grad = impl, grad
        self.pre_slope = None if pre_slope is None else float(pre_slope)
        self.n_power_iterations, self.eps = int(hook.n_power_iterations), float(hook.eps)
        geometry = (conv_geometry(conv) or (None,))[0]
        self.geometry = geometry if geometry in (S1K3, S2K4) else None
        self.pointwise = pointwise == "kernels" and geometry == P1K1
        if pool not in _gc.POOLS or (pool == 2 and (not self.pointwise or pre_slope is not None)):
            raise ValueError("SpectralConv: pool is 1, or 2 on a 1x1 convolution with pointwise='kernels' and no pre_slope "
                             "(got %r)" % (pool,))
        self.pool = pool
        for name, p in conv._parameters.items():
            self.register_parameter(name, p)
        for name, b in conv._buffers.items():
            self.register_buffer(name, b, persistent=name not in conv._non_persistent_buffers_set)
        self.__dict__["original"] = conv           # not a submodule: its geometry, and F.conv2d for what the kernels lack
        self.__dict__["_handed"] = None
        self.train(conv.training)

    def power_iterations(self):
        return self.n_power_iterations if self.training else 0

    def hand(self, weight):
        """the normalised weight for the next forward (fuse_spectral_norm's network hook)"""
        self.__dict__["_handed"] = weight

    def normalized_weight(self):
        weight, self.__dict__["_handed"] = self.__dict__["_handed"], None
        if weight is None:
            weight = spectral_normalize([self.weight_orig], [self.weight_u], [self.weight_v], self.power_iterations(),
                                        self.eps, self.impl)[0]
        return weight

    def forward(self, x, add=None):
        weight = self.normalized_weight()
        geometry = P1K1 if self.pointwise else self.geometry

        def own(x):                      # the convolution's own arithmetic on the normalised weight
            a = x if self.pre_slope is None else F.leaky_relu(x, self.pre_slope)
            return self.original._conv_forward(a, weight, self.bias)
        # a geometry of the kernels runs as its functional form does; only the others need the convolution's own
        return _gc.run(geometry, x, weight, self.bias, "zeros", self.pre_slope, add, self.pool, self.impl, self.grad,
                       own if geometry is None else None)

    def extra_repr(self):
        c = self.original
        return "%d -> %d, kernel_size=%s, stride=%s, n_power_iterations=%d, pre_slope=%s, impl=%r, grad=%r%s" % (
            c.in_channels, c.out_channels, tuple(c.kernel_size), tuple(c.stride), self.n_power_iterations, self.pre_slope,
            self.impl, self.grad, ", pointwise='kernels', pool=%d" % self.pool if self.pointwise else "")


def _normalize_all(convs, impl):
    """one batched call per (power iterations, eps) present among `convs` -- one in all for a network in one mode"""
    groups = {}
    for c in convs:
        groups.setdefault((c.power_iterations(), c.eps), []).append(c)
    for (iters, eps), members in groups.items():
        normed = spectral_normalize([c.weight_orig for c in members], [c.weight_u for c in members],
                                    [c.weight_v for c in members], iters, eps, impl)
        for c, w in zip(members, normed):
            c.hand(w)


def fuse_spectral_norm(net, impl="auto", grad="torch", pointwise="torch"):
    """Rewrite, in place and recursively, every nn.Conv2d of `net` that carries torch.nn.utils.spectral_norm's hook (name
    "weight", dim 0) and no other: its slot becomes a SpectralConv with the same Parameter and buffer objects.  Indices
    and state-dict keys do not change.  Inside an nn.Sequential an nn.LeakyReLU directly in front is folded into the
    convolution (its slot becomes nn.Identity(); a shared activation object is left as it is: only slots change).
    One forward pre-hook on `net` normalises all rewritten convolutions in one batched call per forward and hands each
    its weight; a forward hook drops what a forward did not use.
    Left alone, uncounted: ConvTranspose2d under spectral norm (dim 1), the convolution inside a CoordConv, modules with
    any other hook.  grad: the `grad` of every SpectralConv ("kernels": the convolutions train on GenConvFunction).
    pointwise "kernels": every rewritten Conv2d(k 1, s 1, p 0) runs gen_conv.conv1x1, and inside an nn.Sequential an
    nn.AvgPool2d(kernel 2, stride 2, padding 0, ceil_mode False, divisor_override None) directly in front of one is folded
    into it (the pool's slot becomes nn.Identity(), the convolution gets pool=2); a pool of any other geometry stays.  The
    default "torch" leaves the 1x1 convolutions on F.conv2d and every pool in place.
    Returns the number of convolutions rewritten."""
    _lib.check_impl(impl)
    check_grad(grad)
    _check_pointwise(pointwise)
    replaced = {}
    for parent in list(net.modules()):
        if hasattr(parent, "addcoords"):                     # CoordConv: its convolution sees two more channels
            continue
        names = list(parent._modules.keys())
        for i, name in enumerate(names):
            conv = parent._modules[name]
            if type(conv) is not nn.Conv2d or id(conv) in replaced or _rewrite.spectral_norm_hook(conv) is None:
                continue
            before = parent._modules[names[i - 1]] if isinstance(parent, nn.Sequential) and i >= 1 else None
            slope = _rewrite.slope_of(before, relu=False)
            pool = 2 if slope is None and pointwise == "kernels" and conv_geometry(conv) == (P1K1, "zeros") and \
                _is_pool2(before) else 1
            if slope is not None or pool == 2:
                parent._modules[names[i - 1]] = nn.Identity()
            replaced[id(conv)] = (conv, SpectralConv(conv, slope, impl, grad, pointwise, pool))
            parent._modules[name] = replaced[id(conv)][1]
    _rewrite.replace_aliases(net, replaced)
    if replaced and not getattr(net, "_gfla_spectral_norm_hooks", None):
        def before(module, inputs):
            convs = [m for m in module.modules() if type(m) is SpectralConv]
            if convs:
                _normalize_all(convs, impl)

        def after(module, inputs, output):
            for m in module.modules():
                if type(m) is SpectralConv:
                    m.hand(None)
        handles = (net.register_forward_pre_hook(before), net.register_forward_hook(after, always_call=True))
        net.__dict__["_gfla_spectral_norm_hooks"] = handles
    return len(replaced)


_REFERENCE_DISCRIMINATORS = ("ResDiscriminator", "PatchDiscriminator", "TemporalDiscriminator")


def patch_reference_discriminators(discriminator, base_function=None, impl="auto", grad="torch", pointwise="torch"):
    """Wrap the constructors of the reference's ResDiscriminator, PatchDiscriminator and TemporalDiscriminator
    (discriminator.py) so that every one built from now on comes out rewritten (fuse_spectral_norm on the finished
    network), and, given base_function, replace ResBlockEncoder.forward (base_function.py:533-556: model(x) + shortcut(x))
    by a version that hands shortcut(x) as `add` to the last convolution of `self.model` when that slot is a SpectralConv
    on the 4x4 stride-2 kernels; otherwise it calls the original forward.  pointwise: fuse_spectral_norm's.  Idempotent.
    Returns the names of the classes wrapped."""
    _lib.check_impl(impl)
    check_grad(grad)
    _check_pointwise(pointwise)
    wrapped = [name for name in _REFERENCE_DISCRIMINATORS
               if _rewrite.wrap_init(getattr(discriminator, name, None), "_gfla_fuses_spectral_norm",
                                     lambda self: fuse_spectral_norm(self, impl, grad, pointwise))]

    def make_forward(orig):
        def forward(self, x):
            seq = self.model
            last = seq[len(seq) - 1] if isinstance(seq, nn.Sequential) and len(seq) else None
            if type(last) is not SpectralConv or last.geometry != S2K4:
                return orig(self, x)
            return _rewrite.run_with_add(seq, x, self.shortcut(x))
        return forward
    cls = None if base_function is None else getattr(base_function, "ResBlockEncoder", None)
    if _rewrite.wrap_method(cls, "forward", "_gfla_residual_in_epilogue", make_forward):
        wrapped.append("ResBlockEncoder")
    return wrapped
