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
    SpectralConv3d          the same for the Conv3d of a ResBlock3DEncoder, on frames-major maps (conv3d.py)
    SpectralConvTranspose   the same for an nn.ConvTranspose2d, which torch normalises along dim 1
    SpectralHead            a hooked narrow 3x3 convolution behind a reflection pad, on head_conv.head_conv3x3
    fuse_spectral_norm      rewrite the hooked convolutions of a network in place
    patch_reference_discriminators   the reference's discriminators, rewritten as they are built
    patch_reference_generators       the reference's generators, rewritten as they are built

A weight normalised along dim 1 -- (Cin, Cout, kh, kw), the matrix being weight.permute(1,0,2,3).reshape(Cout, -1) -- is
read by the kernels where it lies: W_sn and the gradients keep the weight's storage layout and no permuted copy is made.

Float32 parameters on the GPU run on the kernels (under torch.autocast as well: parameters stay float32).  CPU tensors,
float64, 16-bit parameters and impl="torch" take the torch composition: the operations of the hook's compute_weight in
the hook's order, so on the CPU it is bit-identical to the hook.
"""
import ctypes
import types

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from . import _rewrite
from . import conv3d as _c3
from . import gen_conv as _gc
from . import head_conv as _hc
from ._conv_common import P1K1, PADDINGS, S1K3, S2K4, T2K3, check_grad, conv_geometry

POINTWISE = ("torch", "kernels")
TEMPORAL = ("torch", "kernels")
_TABLE_CACHE = {}
_TABLE_CACHE_MAX = 64


class _Table(object):
    """The device table of a batch (include/gfla_spectral_norm.h) with the host numbers that go with it."""

    def __init__(self, weights, us, vs, dims=None):
        n = len(weights)
        self.n = n
        self.shapes = [tuple(w.shape) for w in weights]
        # a batch of dim-0 matrices only: the entry points and the 8-word records it always had; otherwise the mixed ones,
        # (R, K, inner) and 9 words per matrix
        self.mixed = dims is not None and any(dims)
        per = 3 if self.mixed else 2
        self.entry = "gfla_spectral_norm_mixed_" if self.mixed else "gfla_spectral_norm_"
        self.dims = (ctypes.c_int64 * (per * n))()
        for i, w in enumerate(weights):
            self.dims[per * i: per * i + per] = _matrix_dims(w, dims[i] if self.mixed else 0)[:per]
        offsets, totals = (ctypes.c_int64 * (3 * n))(), (ctypes.c_int64 * 2)()
        status = getattr(_lib.lib(), self.entry + "layout")(ctypes.addressof(self.dims), n, ctypes.addressof(offsets),
                                                            ctypes.addressof(totals))
        if status != 0:
            err = _lib.Unsupported if status == _lib._ERR_UNSUPPORTED else ValueError
            raise err("spectral_normalize: %s" % _lib.lib().gfla_status_string(status).decode())
        self.elems, self.vecs = int(totals[0]), int(totals[1])
        self.elem_off = [int(offsets[3 * i]) for i in range(n)]
        self.bwd_scratch = int(getattr(_lib.lib(), self.entry + "bwd_scratch_floats")(ctypes.addressof(self.dims), n))
        rows = [[w.data_ptr(), u.data_ptr(), v.data_ptr(), self.dims[per * i], self.dims[per * i + 1], offsets[3 * i],
                 offsets[3 * i + 1], offsets[3 * i + 2]] + ([self.dims[per * i + 2]] if self.mixed else [])
                for i, (w, u, v) in enumerate(zip(weights, us, vs))]
        self.device = weights[0].device
        self.table = torch.tensor(rows, dtype=torch.int64).to(self.device)

    def dims_ptr(self):
        return ctypes.c_void_p(ctypes.addressof(self.dims))


def _matrix_dims(w, dim):
    """(R, K, inner) of the weight `w` normalised along `dim` (include/gfla_spectral_norm.h): inner 0 is dim 0, the matrix
    as stored; dim 1 is (Cin, R, ...) with inner = the elements behind the first two axes"""
    rows = w.size(dim)
    return rows, w.numel() // max(rows, 1), 0 if dim == 0 else w.numel() // max(w.size(0) * rows, 1)


def _table(weights, us, vs, dims=None):
    """the table of this batch: built once, rebuilt only when a pointer, a shape or a dim changes"""
    dims = None if dims is None or not any(dims) else tuple(dims)
    key = tuple((w.data_ptr(), u.data_ptr(), v.data_ptr(), tuple(w.shape)) for w, u, v in zip(weights, us, vs))
    key = (weights[0].device, key, dims)
    hit = _TABLE_CACHE.get(key)
    if hit is None:
        if len(_TABLE_CACHE) >= _TABLE_CACHE_MAX:
            _TABLE_CACHE.clear()
        hit = _TABLE_CACHE[key] = _Table(weights, us, vs, dims)
    return hit


class SpectralNormFunction(Function):
    """(table, power_iterations, eps, *weight_origs) -> (*W_sn) on the library's kernels: the whole batch in
    2 power_iterations + 1 launches (2 in eval mode), the backward in 2, whether the table holds dim-0 matrices, dim-1
    matrices or both.  u and v, the buffers the table points at, are updated in place.  Saved per call: the u, v and sigma the outputs were computed with (written by the forward's own
    launches), so that a backward after a later forward -- D(real), D(fake), one backward -- uses its own call's values."""

    @staticmethod
    def forward(ctx, table, power_iterations, eps, *weights):
        dev = table.device
        needs = any(ctx.needs_input_grad[3:])
        flat = torch.empty(table.elems, dtype=torch.float32, device=dev)
        sigma = torch.empty(table.n, dtype=torch.float32, device=dev)
        saved = torch.empty(table.vecs, dtype=torch.float32, device=dev) if needs else None
        # the mixed entry points keep the dim-1 matrices' t and s in float64 behind the float32 vector arrays
        scratch = torch.empty(3 * table.vecs + 2 if table.mixed else table.vecs, dtype=torch.float32, device=dev)
        _lib.call(table.entry + "fwd_f32", flat, _lib.ptr(table.table), table.dims_ptr(), table.n, _lib.ptr(flat),
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
        _lib.call(table.entry + "bwd_f32", grad_w, _lib.ptr(table.table), table.dims_ptr(), table.n, _lib.ptr(grad_sn),
                  _lib.ptr(saved), _lib.ptr(sigma), _lib.ptr(grad_w), _lib.ptr(scratch))
        out = [grad_w[o:o + torch.Size(s).numel()].view(s) if need else None
               for o, s, need in zip(table.elem_off, table.shapes, ctx.needs_input_grad[3:])]
        return (None, None, None) + tuple(out)


def torch_spectral_normalize(weight, u, v, power_iterations=1, eps=1e-12, dim=0):
    """One weight by the operations of torch's SpectralNorm.compute_weight, in its order; u and v in place.  dim: the
    hook's -- 0, or 1 for a transposed convolution, whose matrix is the hook's reshape_weight_to_matrix (a permute)."""
    weight_mat = weight
    if dim != 0:
        weight_mat = weight_mat.permute(dim, *[d for d in range(weight_mat.dim()) if d != dim])
    weight_mat = weight_mat.reshape(weight_mat.size(0), -1)
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


def spectral_normalize(weights, us, vs, power_iterations=1, eps=1e-12, impl="auto", dims=None):
    """[W / sigma for every weight (Cout, ...) of `weights`], with `power_iterations` rounds of the power iteration on the
    vectors us[i] (Cout) and vs[i] (the rest), updated in place; 0 (eval mode) leaves them untouched.  Arithmetic and
    gradient (u, v, sigma constants) as torch.nn.utils.spectral_norm.
    dims: one 0 or 1 per weight, the hook's `dim`; None: all 0.  A weight with dim 1 is (Cin, Cout, ...), the layout of
    an nn.ConvTranspose2d: u is (Cout,), v (numel / Cout,) in the order of weight.permute(1, 0, ...).reshape(Cout, -1), and
    the result has the weight's own layout.  Both kinds go in one call.
    impl "auto": contiguous float32 GPU tensors run as ONE batched call on the kernels (SpectralNormFunction); anything
    else -- CPU, float64, 16-bit, sizes the library refuses -- and impl "torch" take torch_spectral_normalize per weight."""
    _lib.check_impl(impl)
    weights, us, vs = list(weights), list(us), list(vs)
    dims = [0] * len(weights) if dims is None else [int(d) for d in dims]
    if len(dims) != len(weights) or any(d not in (0, 1) for d in dims):
        raise ValueError("spectral_normalize: dims is None or one 0 / 1 per weight (got %r)" % (dims,))
    if not (len(weights) == len(us) == len(vs)) or not weights:
        raise ValueError("spectral_normalize: as many us and vs as weights, at least one (got %d, %d, %d)"
                         % (len(weights), len(us), len(vs)))
    if int(power_iterations) < 0 or not float(eps) > 0:
        raise ValueError("spectral_normalize: power_iterations >= 0 and eps > 0 (got %r, %r)" % (power_iterations, eps))
    for w, u, v, d in zip(weights, us, vs, dims):
        if w.dim() <= d or w.numel() == 0 or tuple(u.shape) != (w.size(d),) or tuple(v.shape) != (w.numel() // w.size(d),):
            raise ValueError("spectral_normalize: weight (R, ...) or with dim 1 (Cin, R, ...), u (R,), v (K,) (got %s, %s, %s)"
                             % (tuple(w.shape), tuple(u.shape), tuple(v.shape)))
    if impl == "auto" and _kernel_batch(weights, us, vs):
        try:
            return list(SpectralNormFunction.apply(_table(weights, us, vs, dims), int(power_iterations), float(eps), *weights))
        except _lib.Unsupported:
            pass
    return [torch_spectral_normalize(w, u, v, int(power_iterations), float(eps), d)
            for w, u, v, d in zip(weights, us, vs, dims)]


def _check_pointwise(pointwise):
    if pointwise not in POINTWISE:
        raise ValueError("pointwise: one of %s (got %r)" % (POINTWISE, pointwise))


def _is_pool2(module):
    """nn.AvgPool2d(2, 2): what conv1x1's pool=2 computes"""
    def pair(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    return type(module) is nn.AvgPool2d and pair(module.kernel_size) == (2, 2) and pair(module.stride) == (2, 2) and \
        pair(module.padding) == (0, 0) and not module.ceil_mode and module.divisor_override is None


class _Normalized(nn.Module):
    """What SpectralConv and SpectralConv3d share: the hooked convolution's Parameters and buffers under its names and in
    its order, the hook's numbers, and the weight that the network's batched call hands over."""

    def _adopt(self, conv, hook):
        self.n_power_iterations, self.eps, self.dim = int(hook.n_power_iterations), float(hook.eps), int(hook.dim)
        for name, p in conv._parameters.items():
            self.register_parameter(name, p)
        for name, b in conv._buffers.items():
            self.register_buffer(name, b, persistent=name not in conv._non_persistent_buffers_set)
        self.__dict__["original"] = conv           # not a submodule: its geometry, and its own forward for what the kernels lack
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
                                        self.eps, self.impl, [self.dim])[0]
        return weight


class SpectralConv(_Normalized):
    """[LeakyReLU(pre_slope)] -> the convolution `conv` under torch's spectral_norm hook (+ add), with the normalisation
    on the batched op.  `weight_orig`, `bias`, `weight_u` and `weight_v` are conv's own Parameter and buffer objects under
    conv's names and in conv's order, so state dicts interchange with the hooked form in both directions;
    n_power_iterations and eps are the hook's.  Training mode iterates, eval mode does not.
    Conv2d(k 3, s 1, p 1) and Conv2d(k 4, s 2, p 1) run through gen_conv.conv3x3 / conv4x4_down (grad="kernels": the
    library's gradient kernels; the normalised weight's gradient comes back through SpectralNormFunction).  Conv2d(k 1,
    s 1, p 0) runs through gen_conv.conv1x1 with pointwise="kernels" -- `pool` 2: behind the AvgPool2d(2) that
    fuse_spectral_norm folded in, which needs that route --, and with the default pointwise="torch" through F.conv2d on the
    normalised weight, as every other geometry does (groups, dilation, k 4 with s 1).
    padding "reflect": `conv` is a Conv2d(k 3, s 1, p 0) that stood directly behind an nn.ReflectionPad2d(1) -- every Jump
    of the reference's generators --, and the module stands for both: gen_conv.conv3x3(padding="reflect").
    Inside a forward of a network rewritten by fuse_spectral_norm the weight was normalised with all the others in one
    call; called on its own, the module normalises itself, a batch of one."""

    def __init__(self, conv, pre_slope=None, impl="auto", grad="torch", pointwise="torch", pool=1, padding="zeros"):
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
        if padding not in PADDINGS or (padding == "reflect" and conv_geometry(conv, True) != (S1K3, "reflect")):
            raise ValueError("SpectralConv: padding 'zeros', or 'reflect' for a Conv2d(k 3, s 1, p 0) (got %r)" % (padding,))
        self.padding = padding
        geometry = (conv_geometry(conv, padding == "reflect") or (None,))[0]
        self.geometry = geometry if geometry in (S1K3, S2K4) else None
        self.pointwise = pointwise == "kernels" and geometry == P1K1
        if pool not in _gc.POOLS or (pool == 2 and (not self.pointwise or pre_slope is not None)):
            raise ValueError("SpectralConv: pool is 1, or 2 on a 1x1 convolution with pointwise='kernels' and no pre_slope "
                             "(got %r)" % (pool,))
        self.pool = pool
        self._adopt(conv, hook)

    def forward(self, x, add=None):
        weight = self.normalized_weight()
        geometry = P1K1 if self.pointwise else self.geometry

        def own(x):                      # the convolution's own arithmetic on the normalised weight
            a = x if self.pre_slope is None else F.leaky_relu(x, self.pre_slope)
            return self.original._conv_forward(a, weight, self.bias)
        # a geometry of the kernels runs as its functional form does; only the others need the convolution's own
        return _gc.run(geometry, x, weight, self.bias, self.padding, self.pre_slope, add, self.pool, self.impl, self.grad,
                       own if geometry is None else None)

    @property
    def fuses_add(self):                 # _rewrite.epilogue_slot: `add` goes into the epilogue of the 3x3 / 4x4 kernels
        return self.geometry is not None

    def extra_repr(self):
        c = self.original
        return "%d -> %d, kernel_size=%s, stride=%s, n_power_iterations=%d, pre_slope=%s, impl=%r, grad=%r%s%s" % (
            c.in_channels, c.out_channels, tuple(c.kernel_size), tuple(c.stride), self.n_power_iterations, self.pre_slope,
            self.impl, self.grad, ", pointwise='kernels', pool=%d" % self.pool if self.pointwise else "",
            ", padding='reflect'" if self.padding == "reflect" else "")


class SpectralConvTranspose(_Normalized):
    """[LeakyReLU(pre_slope)] -> the nn.ConvTranspose2d `conv` under torch's spectral_norm hook (+ add), with the
    normalisation on the batched op.  torch normalises a transposed convolution along dim 1: the matrix is
    weight.permute(1,0,2,3).reshape(Cout, -1), `weight_u` is (Cout,), `weight_v` (Cin kh kw,).  The kernels read that matrix
    in the weight's storage (Cin, Cout, kh, kw), so the normalised weight is what the convolution takes, as it is.
    SpectralConv's contract otherwise: conv's own `weight_orig`, `bias`, `weight_u`, `weight_v` under conv's names and in
    conv's order, the hook's n_power_iterations and eps, one batched call for the whole network inside a forward of a
    network rewritten by fuse_spectral_norm(generator=True).
    ConvTranspose2d(k 3, s 2, p 1, output_padding 1) runs through gen_conv.run(T2K3, ...), i.e. conv_transpose3x3_up with
    its dispatch (grad="kernels": the library's gradient kernels); every other geometry runs F.conv_transpose2d with conv's
    own arguments on the normalised weight."""

    def __init__(self, conv, pre_slope=None, impl="auto", grad="torch"):
        super(SpectralConvTranspose, self).__init__()
        _lib.check_impl(impl)
        check_grad(grad)
        hook = _rewrite.spectral_norm_hook(conv, dims=(1,))
        if type(conv) is not nn.ConvTranspose2d or hook is None:
            raise ValueError("SpectralConvTranspose: an nn.ConvTranspose2d under torch.nn.utils.spectral_norm (name 'weight', "
                             "dim 1) and no other hook")
        self.impl, self.grad = impl, grad
        self.pre_slope = None if pre_slope is None else float(pre_slope)
        self.geometry = T2K3 if conv_geometry(conv) == (T2K3, "zeros") else None
        self._adopt(conv, hook)

    def forward(self, x, add=None):
        weight = self.normalized_weight()

        def own(x):                      # the convolution's own arithmetic on the normalised weight
            c = self.original
            a = x if self.pre_slope is None else F.leaky_relu(x, self.pre_slope)
            return F.conv_transpose2d(a, weight, self.bias, c.stride, c.padding, c.output_padding, c.groups, c.dilation)
        return _gc.run(self.geometry, x, weight, self.bias, "zeros", self.pre_slope, add, 1, self.impl, self.grad,
                       own if self.geometry is None else None)

    @property
    def fuses_add(self):                 # _rewrite.epilogue_slot
        return self.geometry == T2K3

    def extra_repr(self):
        c = self.original
        return "%d -> %d, kernel_size=%s, stride=%s, n_power_iterations=%d, pre_slope=%s, impl=%r, grad=%r" % (
            c.in_channels, c.out_channels, tuple(c.kernel_size), tuple(c.stride), self.n_power_iterations, self.pre_slope,
            self.impl, self.grad)


class SpectralHead(_Normalized):
    """[LeakyReLU(pre_slope)] -> ReflectionPad2d(1) -> the Conv2d(C, at most 8, 3) `conv` under torch's spectral_norm hook
    -> [Tanh | Sigmoid] as one op: the reference's `Output` under spectral norm.  The normalised weight goes to
    head_conv.head_conv3x3(x, W_sn, bias, "reflect", pre_slope, post), whose gradient reaches `weight_orig` through
    SpectralNormFunction.  SpectralConv's contract otherwise (conv's own Parameters and buffers, names and order)."""

    def __init__(self, conv, pre_slope=None, post=None, impl="auto"):
        super(SpectralHead, self).__init__()
        _lib.check_impl(impl)
        hook = _rewrite.spectral_norm_hook(conv)
        if type(conv) is not nn.Conv2d or hook is None or conv_geometry(conv, True) != (S1K3, "reflect") or \
                conv.out_channels > _hc.MAX_COUT:
            raise ValueError("SpectralHead: an nn.Conv2d(k 3, s 1, p 0) of at most %d output channels under "
                             "torch.nn.utils.spectral_norm (name 'weight', dim 0) and no other hook" % _hc.MAX_COUT)
        if post not in _hc.POSTS:
            raise ValueError("SpectralHead: post is one of %s (got %r)" % (_hc.POSTS, post))
        self.impl, self.post = impl, post
        self.pre_slope = None if pre_slope is None else float(pre_slope)
        self._adopt(conv, hook)

    def forward(self, x):
        return _hc.head_conv3x3(x, self.normalized_weight(), self.bias, "reflect", self.pre_slope, self.post, None, self.impl)

    def extra_repr(self):
        c = self.original
        return "%d -> %d, n_power_iterations=%d, pre_slope=%s, post=%s, impl=%r" % (
            c.in_channels, c.out_channels, self.n_power_iterations, self.pre_slope, self.post, self.impl)


def conv3d_geometry(module):
    """"k333" / "k344" / "k111" for an nn.Conv3d of one of the three shapes a ResBlock3DEncoder has, else None"""
    if type(module) is not nn.Conv3d or module.groups != 1 or tuple(module.dilation) != (1, 1, 1) or \
            module.padding_mode != "zeros":
        return None
    return {((3, 3, 3), (1, 1, 1), (1, 1, 1)): "k333", ((3, 4, 4), (1, 2, 2), (0, 1, 1)): "k344",
            ((1, 1, 1), (1, 1, 1), (0, 0, 0)): "k111"}.get((tuple(module.kernel_size), tuple(module.stride),
                                                            tuple(module.padding)))


class SpectralConv3d(_Normalized):
    """[LeakyReLU(pre_slope)] -> the Conv3d `conv` under torch's spectral_norm hook (+ add) on a FRAMES-MAJOR map
    (B,L,C,H,W) -> (B,Lout,Cout,Hout,Wout), for the three convolutions of a ResBlock3DEncoder: k (3,3,3) s 1 p 1 and
    k (3,4,4) s (1,2,2) p (0,1,1) through conv3d.conv3d_frames, the 1x1x1 bypass through gen_conv.conv1x1 on the
    (B L, C, H, W) batch its input is.  SpectralConv's contract otherwise: conv's own `weight_orig`, `bias`, `weight_u`,
    `weight_v` under conv's names and in conv's order, the normalisation through spectral_normalize -- which flattens the
    5-D weight to (Cout, -1), so u and v keep torch's order --, with all the others of the network in one call; the
    frames-major permutation is applied to the NORMALISED weight, when it is packed.  Whatever the kernels do not run (CPU,
    float64, impl="torch", a gradient needed without grad="kernels") is conv's own forward on the permuted map."""

    def __init__(self, conv, pre_slope=None, impl="auto", grad="torch"):
        super(SpectralConv3d, self).__init__()
        _lib.check_impl(impl)
        check_grad(grad)
        hook = _rewrite.spectral_norm_hook(conv)
        self.geometry = conv3d_geometry(conv)
        if self.geometry is None or hook is None:
            raise ValueError("SpectralConv3d: an nn.Conv3d of kernel (3,3,3) / (3,4,4) stride (1,2,2) / 1 under "
                             "torch.nn.utils.spectral_norm (name 'weight', dim 0) and no other hook")
        if self.geometry == "k111" and pre_slope is not None:
            raise ValueError("SpectralConv3d: the 1x1x1 convolution takes no pre-activation (got %r)" % (pre_slope,))
        self.impl, self.grad = impl, grad
        self.pre_slope = None if pre_slope is None else float(pre_slope)
        self._adopt(conv, hook)

    def _own(self, x, weight):               # the convolution's own arithmetic on the normalised weight, in torch's layout
        a = x if self.pre_slope is None else F.leaky_relu(x, self.pre_slope)
        return _c3.frames_major_result(self.original._conv_forward(a.permute(0, 2, 1, 3, 4), weight, self.bias))

    def forward(self, x, add=None):
        weight = self.normalized_weight()
        if self.geometry != "k111":
            if self.impl == "torch" or not x.is_cuda:
                y = self._own(x, weight)
                return y if add is None else y + add
            return _c3.conv3d_frames(x, weight, self.bias, self.geometry, self.pre_slope, add, self.grad, self.impl)
        if x.dim() != 5:
            raise ValueError("SpectralConv3d: a frames-major (B,L,C,H,W) map (got %s)" % (tuple(x.shape),))
        B, L, C, H, W = x.shape
        cout = weight.size(0)
        y = _gc.run(P1K1, x.reshape(B * L, C, H, W), weight.reshape(cout, C, 1, 1), self.bias, "zeros", None, None, 1,
                    self.impl, self.grad, lambda _: self._own(x, weight).reshape(B * L, cout, H, W))
        y = y.reshape(B, L, cout, H, W)
        return y if add is None else y + add

    def extra_repr(self):
        c = self.original
        return "%s, %d -> %d, n_power_iterations=%d, pre_slope=%s, impl=%r, grad=%r" % (
            self.geometry, c.in_channels, c.out_channels, self.n_power_iterations, self.pre_slope, self.impl, self.grad)


def _is_pool322(module):
    """nn.AvgPool3d((3,2,2), (1,2,2)): what conv3d.avg_pool_frames computes"""
    def triple(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v, v)
    return type(module) is nn.AvgPool3d and triple(module.kernel_size) == (3, 2, 2) and triple(module.stride) == (1, 2, 2) \
        and triple(module.padding) == (0, 0, 0) and not module.ceil_mode and module.divisor_override is None and \
        _rewrite.no_hooks(module)


def _temporal_block(block):
    """(conv k333, conv k344, pool, conv k111) of a module shaped like the reference's ResBlock3DEncoder without a norm
    layer -- model = Sequential(LeakyReLU, Conv3d k333, LeakyReLU, Conv3d k344), shortcut = Sequential(AvgPool3d((3,2,2),
    (1,2,2)), Conv3d 1x1x1), all three convolutions under the spectral-norm hook and nothing else hooked --, else None"""
    model, shortcut = block._modules.get("model"), block._modules.get("shortcut")
    if type(model) is not nn.Sequential or type(shortcut) is not nn.Sequential or len(model) != 4 or len(shortcut) != 2:
        return None
    if not all(_rewrite.no_hooks(m) for m in (block, model, shortcut)):
        return None
    act1, conv1, act2, conv2 = list(model)
    pool, bypass = list(shortcut)
    if _rewrite.slope_of(act1, relu=False) is None or _rewrite.slope_of(act2, relu=False) is None or not _is_pool322(pool):
        return None
    if not _rewrite.no_hooks(act1) or not _rewrite.no_hooks(act2):
        return None
    if len({id(conv1), id(conv2), id(bypass)}) != 3:
        return None
    for conv, geometry in ((conv1, "k333"), (conv2, "k344"), (bypass, "k111")):
        if conv3d_geometry(conv) != geometry or _rewrite.spectral_norm_hook(conv) is None:
            return None
    if conv1.in_channels != bypass.in_channels or conv2.out_channels != bypass.out_channels:
        return None
    return conv1, conv2, pool, bypass


class AvgPoolFrames(nn.Module):
    """conv3d.avg_pool_frames in the slot of an nn.AvgPool3d((3,2,2), (1,2,2)), on a frames-major map"""

    def __init__(self, impl="auto", grad="torch"):
        super(AvgPoolFrames, self).__init__()
        _lib.check_impl(impl)
        check_grad(grad)
        self.impl, self.grad = impl, grad

    def forward(self, x):
        return _c3.avg_pool_frames(x, self.grad, self.impl)

    def extra_repr(self):
        return "kernel_size=(3, 2, 2), stride=(1, 2, 2), impl=%r, grad=%r" % (self.impl, self.grad)


def is_frames_major_block(block):
    """a block rewritten by fuse_spectral_norm(temporal="kernels"): its model and shortcut take frames-major maps"""
    return block is not None and bool(block.__dict__.get("_gfla_frames_major"))


def frames_major_block_forward(self, x, frames_major=False):
    """The forward of a rewritten ResBlock3DEncoder: model(x) with shortcut(x) in the epilogue of its last convolution.
    Called on its own it takes and returns torch's (B,C,L,H,W), one permute copy each way; frames_major=True: (B,L,C,H,W)
    in and out (the rewritten TemporalDiscriminator keeps both blocks in that layout)."""
    if not frames_major:
        x = _c3.to_frames_major(x)
    y = _rewrite.run_with_add(self.model, x, self.shortcut(x))
    return y if frames_major else _c3.from_frames_major(y)


frames_major_block_forward._gfla_frames_major_block = True


def _rewrite_temporal_block(block, found, impl, grad, replaced):
    conv1, conv2, pool, bypass = found
    model, shortcut = block._modules["model"], block._modules["shortcut"]
    names, snames = list(model._modules.keys()), list(shortcut._modules.keys())
    slopes = [_rewrite.slope_of(model._modules[names[i]], relu=False) for i in (0, 2)]
    for at, conv, slope in ((1, conv1, slopes[0]), (3, conv2, slopes[1])):
        replaced[id(conv)] = (conv, SpectralConv3d(conv, slope, impl, grad))
        model._modules[names[at]] = replaced[id(conv)][1]
        model._modules[names[at - 1]] = nn.Identity()
    shortcut._modules[snames[0]] = AvgPoolFrames(impl, grad)
    replaced[id(bypass)] = (bypass, SpectralConv3d(bypass, None, impl, grad))
    shortcut._modules[snames[1]] = replaced[id(bypass)][1]
    block.__dict__["_gfla_frames_major"] = True
    if not getattr(type(block).forward, "_gfla_frames_major_block", False):      # no class-wide wrapper: this instance's own
        block.__dict__["forward"] = types.MethodType(frames_major_block_forward, block)


def _normalize_all(convs, impl):
    """one batched call per (power iterations, eps) present among `convs` -- one in all for a network in one mode"""
    groups = {}
    for c in convs:
        groups.setdefault((c.power_iterations(), c.eps), []).append(c)
    for (iters, eps), members in groups.items():
        normed = spectral_normalize([c.weight_orig for c in members], [c.weight_u for c in members],
                                    [c.weight_v for c in members], iters, eps, impl, [c.dim for c in members])
        for c, w in zip(members, normed):
            c.hand(w)


def fuse_spectral_norm(net, impl="auto", grad="torch", pointwise="torch", temporal="torch", generator=False):
    """Rewrite, in place and recursively, every nn.Conv2d of `net` that carries torch.nn.utils.spectral_norm's hook (name
    "weight", dim 0) and no other: its slot becomes a SpectralConv with the same Parameter and buffer objects.  Indices
    and state-dict keys do not change.  Inside an nn.Sequential an nn.LeakyReLU directly in front is folded into the
    convolution (its slot becomes nn.Identity(); a shared activation object is left as it is: only slots change).
    One forward pre-hook on `net` normalises all rewritten convolutions in one batched call per forward and hands each
    its weight; a forward hook drops what a forward did not use.
    Left alone, uncounted: ConvTranspose2d under spectral norm (dim 1) unless generator=True, the convolution inside a
    CoordConv, modules with any other hook.  grad: the `grad` of every SpectralConv ("kernels": the convolutions train on GenConvFunction).
    pointwise "kernels": every rewritten Conv2d(k 1, s 1, p 0) runs gen_conv.conv1x1, and inside an nn.Sequential an
    nn.AvgPool2d(kernel 2, stride 2, padding 0, ceil_mode False, divisor_override None) directly in front of one is folded
    into it (the pool's slot becomes nn.Identity(), the convolution gets pool=2); a pool of any other geometry stays.  The
    default "torch" leaves the 1x1 convolutions on F.conv2d and every pool in place.
    temporal "kernels": every module shaped like the reference's ResBlock3DEncoder without a norm layer (_temporal_block:
    model = Sequential(LeakyReLU, Conv3d k333, LeakyReLU, Conv3d k344), shortcut = Sequential(AvgPool3d((3,2,2), (1,2,2)),
    Conv3d 1x1x1), the three convolutions hooked) runs on frames-major maps: the convolutions become SpectralConv3d with the
    activations folded in, the pool an AvgPoolFrames, the shortcut goes into the last convolution's epilogue, and the
    block's forward (frames_major_block_forward) converts on the way in and out when it is called on its own.  The three
    weights join the one batched normalisation.  A block with norm layers, another pool, a CoordConv or a foreign hook is
    left alone, uncounted.  The default "torch" looks at no Conv3d, as before.
    generator True: what a generator under spectral norm has besides.  Every nn.ConvTranspose2d under the hook (name
    "weight", dim 1, no other hook) becomes a SpectralConvTranspose, an nn.LeakyReLU directly in front folded in.  Inside an
    nn.Sequential a hooked Conv2d(k 3, s 1, p 0) directly behind an nn.ReflectionPad2d(1) becomes ONE module for both: with
    more than 8 output channels a SpectralConv(padding="reflect") (the reference's Jump), with at most 8 a SpectralHead
    (the reference's Output), which also absorbs an nn.Tanh / nn.Sigmoid directly behind; an nn.LeakyReLU in front of the
    pad is folded in.  The slots of the pad, the activation in front and the absorbed post-activation become
    nn.Identity().  nn.Sequential containers are visited first, so that a convolution also registered outside one (Jump
    and Output keep theirs as `conv1` and `model.2`) is rewritten where its neighbours can be seen; the other name gets
    the same module.  All weights, both dims, join the one batched call.  Left alone as before: CoordConv, foreign hooks;
    and anything inside a module with a `fully_connect_layer` (ExtractorAttn).  The default False does exactly what the
    function did before.
    Returns the number of convolutions rewritten."""
    _lib.check_impl(impl)
    check_grad(grad)
    _check_pointwise(pointwise)
    if temporal not in TEMPORAL:
        raise ValueError("temporal: one of %s (got %r)" % (TEMPORAL, temporal))
    replaced = {}
    if temporal == "kernels":
        for block in list(net.modules()):
            found = _temporal_block(block)
            if found is not None and not any(id(c) in replaced for c in (found[0], found[1], found[3])):
                _rewrite_temporal_block(block, found, impl, grad, replaced)
    parents, skip = list(net.modules()), set()
    if generator:
        parents.sort(key=lambda m: not isinstance(m, nn.Sequential))         # stable: containers first
        for m in net.modules():
            if hasattr(m, "fully_connect_layer"):
                skip.update(id(sub) for sub in m.modules())
    for parent in parents:
        if hasattr(parent, "addcoords") or id(parent) in skip:   # CoordConv: its convolution sees two more channels
            continue
        names = list(parent._modules.keys())
        in_seq = isinstance(parent, nn.Sequential)
        for i, name in enumerate(names):
            conv = parent._modules[name]
            if conv is None or id(conv) in replaced:
                continue
            if generator and type(conv) is nn.ConvTranspose2d and _rewrite.spectral_norm_hook(conv, dims=(1,)) is not None:
                slope = _rewrite.slope_of(parent._modules[names[i - 1]], relu=False) if in_seq and i >= 1 else None
                if slope is not None:
                    parent._modules[names[i - 1]] = nn.Identity()
                replaced[id(conv)] = (conv, SpectralConvTranspose(conv, slope, impl, grad))
                parent._modules[name] = replaced[id(conv)][1]
                continue
            if type(conv) is not nn.Conv2d or _rewrite.spectral_norm_hook(conv) is None:
                continue
            pad = parent._modules[names[i - 1]] if generator and in_seq and i >= 1 else None
            if pad is not None and _rewrite.is_reflect_pad(pad) and _rewrite.no_hooks(pad) and \
                    conv_geometry(conv, True) == (S1K3, "reflect"):
                slope = _rewrite.slope_of(parent._modules[names[i - 2]], relu=False) if i >= 2 else None
                if conv.out_channels <= _hc.MAX_COUT:
                    after = parent._modules[names[i + 1]] if i + 1 < len(names) else None
                    post = None if after is None or not _rewrite.no_hooks(after) else \
                        "tanh" if type(after) is nn.Tanh else "sigmoid" if type(after) is nn.Sigmoid else None
                    fused = SpectralHead(conv, slope, post, impl)
                    if post is not None:
                        parent._modules[names[i + 1]] = nn.Identity()
                else:
                    fused = SpectralConv(conv, slope, impl, grad, pointwise, 1, "reflect")
                parent._modules[names[i - 1]] = nn.Identity()
                if slope is not None:
                    parent._modules[names[i - 2]] = nn.Identity()
                replaced[id(conv)] = (conv, fused)
                parent._modules[name] = fused
                continue
            before = parent._modules[names[i - 1]] if in_seq and i >= 1 else None
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
            convs = [m for m in module.modules() if isinstance(m, _Normalized)]
            if convs:
                _normalize_all(convs, impl)

        def after(module, inputs, output):
            for m in module.modules():
                if isinstance(m, _Normalized):
                    m.hand(None)
        handles = (net.register_forward_pre_hook(before), net.register_forward_hook(after, always_call=True))
        net.__dict__["_gfla_spectral_norm_hooks"] = handles
    return len(replaced)


_REFERENCE_GENERATORS = ("PoseGenerator", "PoseFlowNetGenerator", "DanceGenerator", "FaceGenerator", "ShapeNetGenerator",
                         "ShapeNetFlowNetGenerator")


def patch_reference_generators(generator_module, base_function=None, impl="auto", grad="torch", pointwise="torch"):
    """Wrap the constructors of the reference's PoseGenerator, PoseFlowNetGenerator, DanceGenerator, FaceGenerator,
    ShapeNetGenerator and ShapeNetFlowNetGenerator (generator.py) so that every one built from now on comes out rewritten:
    fuse_spectral_norm(generator=True) once on the finished network -- per network, so that all its convolutions, of the
    flow net and of the target net, share ONE batched normalisation per forward, not one per block.  Given base_function,
    ResBlock.forward and ResBlockDecoder.forward hand the residual to the last convolution's epilogue
    (gen_conv.install_residual_forwards: the same forwards and the same flag patch_reference_convs installs).  A generator
    built without spectral norm has nothing to rewrite and stays as it is.  Idempotent.  Returns the names of the classes
    wrapped."""
    _lib.check_impl(impl)
    check_grad(grad)
    _check_pointwise(pointwise)
    wrapped = [name for name in _REFERENCE_GENERATORS
               if _rewrite.wrap_init(getattr(generator_module, name, None), "_gfla_fuses_spectral_norm",
                                     lambda self: fuse_spectral_norm(self, impl, grad, pointwise, generator=True))]
    if base_function is not None:
        wrapped += _gc.install_residual_forwards(base_function)
    return wrapped


_REFERENCE_DISCRIMINATORS = ("ResDiscriminator", "PatchDiscriminator", "TemporalDiscriminator")


def patch_reference_discriminators(discriminator, base_function=None, impl="auto", grad="torch", pointwise="torch",
                                   temporal="torch"):
    """Wrap the constructors of the reference's ResDiscriminator, PatchDiscriminator and TemporalDiscriminator
    (discriminator.py) so that every one built from now on comes out rewritten (fuse_spectral_norm on the finished
    network), and, given base_function, replace ResBlockEncoder.forward (base_function.py:533-556: model(x) + shortcut(x))
    by a version that hands shortcut(x) as `add` to the last convolution of `self.model` when that slot is a SpectralConv
    on the 4x4 stride-2 kernels; otherwise it calls the original forward.  pointwise: fuse_spectral_norm's.
    temporal "kernels" (fuse_spectral_norm's; needs base_function): ResBlock3DEncoder.forward becomes
    frames_major_block_forward for rewritten blocks, and TemporalDiscriminator.forward (discriminator.py:130-140) converts
    to frames-major once at entry, runs block0 and block1 in that layout and returns to the reference's out.view(b, c l,
    h, w) with one permute copy before the 2-D encoders; unrewritten instances call the original forwards.  Idempotent.
    Returns the names of the classes wrapped."""
    _lib.check_impl(impl)
    check_grad(grad)
    _check_pointwise(pointwise)
    if temporal not in TEMPORAL:
        raise ValueError("temporal: one of %s (got %r)" % (TEMPORAL, temporal))
    if temporal == "kernels":                      # before any network is built: fuse_spectral_norm looks for the flag
        def make_block_forward(orig):
            def forward(self, x, frames_major=False):
                if not is_frames_major_block(self):
                    return orig(self, x)
                return frames_major_block_forward(self, x, frames_major)
            forward._gfla_frames_major_block = True
            return forward

        def make_net_forward(orig):
            def forward(self, x):
                blocks = [getattr(self, "block0", None), getattr(self, "block1", None)]
                if not all(is_frames_major_block(b) for b in blocks):
                    return orig(self, x)
                out = blocks[1](blocks[0](_c3.to_frames_major(x), frames_major=True), frames_major=True)
                b, l, c, h, w = out.shape
                out = out.permute(0, 2, 1, 3, 4).reshape(b, c * l, h, w)        # channel c l_count + l, one copy
                for i in range(self.layers - 2):
                    out = getattr(self, "encoder" + str(i))(out)
                return self.conv(self.nonlinearity(out))
            return forward
        block_cls = None if base_function is None else getattr(base_function, "ResBlock3DEncoder", None)
        _rewrite.wrap_method(block_cls, "forward", "_gfla_frames_major_forward", make_block_forward)
        _rewrite.wrap_method(getattr(discriminator, "TemporalDiscriminator", None), "forward", "_gfla_frames_major_forward",
                             make_net_forward)
    wrapped = [name for name in _REFERENCE_DISCRIMINATORS
               if _rewrite.wrap_init(getattr(discriminator, name, None), "_gfla_fuses_spectral_norm",
                                     lambda self: fuse_spectral_norm(self, impl, grad, pointwise, temporal))]

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
