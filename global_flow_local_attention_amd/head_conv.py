"""Narrow 3x3 convolution heads with fused surroundings on gfx950 (csrc/head_conv3x3.hip).

The reference's generators end in layers whose convolution has a handful of output channels: the image head `Output`
(base_function.py:650-670: LeakyReLU -> ReflectionPad2d(1) -> Conv2d(ngf, 3, 3) -> Tanh at full resolution) and, per
attention layer, a flow head Conv2d(C, 2 | 4, 3, 1, 1) next to a mask head Conv2d(C, 1 | 2, 3, 1, 1) -> Sigmoid on the
same tensor (generator.py:203-209, 237-242).  Here each is one op:

    a = x if pre_slope is None else leaky_relu(x, pre_slope)
    s = conv3x3(pad(a), weight) + bias          pad "zeros" | "reflect", stride 1, output H x W
    y_c = post_c(s_c)                           identity | tanh | sigmoid per OUTPUT channel, Cout <= 8

one read of x forward, no activated and no padded map in memory, and the flow and the mask leave one launch as two
contiguous tensors.

    HeadConv3x3Function      the autograd Function on the kernels
    head_conv3x3             functional form, with the torch composition (torch_head_conv3x3) as the other route
    HeadConv3x3              module with nn.Conv2d's parameter names
    fuse_output_heads        rewrite the [activation] [reflection pad] conv [tanh | sigmoid] runs of a network in place
    flow_mask_heads          a flow convolution and a mask head on the same input, one launch
    patch_reference_flow_heads   the reference's attn_output on flow_mask_heads
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from . import _rewrite
from ._conv_common import PADDINGS, S1K3, check_conv_args, conv_geometry, param_grad

IMPLS = _lib.IMPLS
POSTS = (None, "tanh", "sigmoid")
MAX_COUT = 8
_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _posts(post, cout):
    """`post` as a tuple of one entry per output channel"""
    if post is None or isinstance(post, str):
        post = (post,) * cout
    post = tuple(post)
    if len(post) != cout:
        raise ValueError("head_conv3x3: post needs one entry per output channel, %d (got %d)" % (cout, len(post)))
    for p in post:
        if p not in POSTS:
            raise ValueError("head_conv3x3: post entries are None, 'tanh' or 'sigmoid' (got %r)" % (p,))
    return post


def _validate(x, weight, bias, padding, pre_slope, post, split):
    """Everything that can be wrong with a call, before anything is launched.  Returns (posts, split or None)."""
    cout = check_conv_args("head_conv3x3", x, weight, bias, 3, padding, pre_slope)
    posts = _posts(post, cout)
    if split is not None:
        split = int(split)
        if not 1 <= split < cout:
            raise ValueError("head_conv3x3: split in [1, Cout) = [1, %d) (got %d)" % (cout, split))
    return posts, split


def _masks(posts):
    tanh = sum(1 << i for i, p in enumerate(posts) if p == "tanh")
    sig = sum(1 << i for i, p in enumerate(posts) if p == "sigmoid")
    return tanh, sig


def _workspace(x, cout):
    B, C, H, W = x.shape
    return _lib.workspace("gfla_head_conv3x3_workspace_bytes", x, B, C, cout, H, W, x.element_size(), what="head_conv3x3")


class HeadConv3x3Function(Function):
    """(x (B,Cin,H,W), weight (Cout,Cin,3,3), bias (Cout,) | None, padding, pre_slope, posts, split) -> y, or (y0, y1)
    with a split, on the library's kernels.

    x: float32 / float16 / bfloat16 on the GPU, read as stored; sums are float32 and the outputs have x's dtype, rounded
    once.  weight / bias cross into the library as float32 (other float types are cast: at most 18,440 values).
    Cout <= 8.  posts: one of None / "tanh" / "sigmoid" per output channel.  split: None, or C0 -- then channels [0, C0)
    and [C0, Cout) are returned as two contiguous tensors.
    Saved for the backward: x itself, the outputs and the parameters; nothing else of x's size.  The gradients of x,
    weight and bias are each computed only when needed, without atomics: bit-identical from call to call.  An output that
    the loss does not use (the mask, say) costs nothing: its gradient enters as NULL."""

    @staticmethod
    def forward(ctx, x, weight, bias, padding, pre_slope, posts, split):
        if weight.dim() == 4 and weight.size(0) > MAX_COUT:
            raise ValueError("head_conv3x3: at most %d output channels on the kernels (got %d)" % (MAX_COUT, weight.size(0)))
        _lib.require_gpu(x, weight, bias)
        if x.dtype not in _KERNEL_DTYPES:
            raise TypeError("head_conv3x3: float32, float16 or bfloat16 maps (got %s)" % x.dtype)
        for name, p in (("weight", weight), ("bias", bias)):
            if p is not None and not p.is_floating_point():
                raise TypeError("head_conv3x3: %s must be a float tensor (got %s)" % (name, p.dtype))
        posts, split = _validate(x, weight, bias, padding, pre_slope, posts, split)
        cout = weight.size(0)
        sfx = _lib.suffix(x, "head_conv3x3")
        x = x.contiguous()
        B, Cin, H, W = x.shape
        w32 = weight.detach().to(torch.float32).contiguous()
        b32 = None if bias is None else bias.detach().to(torch.float32).contiguous()
        c0 = cout if split is None else split
        y0 = torch.empty(B, c0, H, W, dtype=x.dtype, device=x.device)
        y1 = None if split is None else torch.empty(B, cout - c0, H, W, dtype=x.dtype, device=x.device)
        tanh, sig = _masks(posts)
        ctx.conf = (c0, PADDINGS.index(padding), int(pre_slope is not None), float(pre_slope or 0.0), tanh, sig)
        _lib.call("gfla_head_conv3x3_fwd_" + sfx, x, _lib.ptr(x), _lib.ptr(w32), _lib.ptr(b32), _lib.ptr(y0), _lib.ptr(y1),
                  B, Cin, cout, c0, H, W, *ctx.conf[1:])
        need = ctx.needs_input_grad
        if need[0] or need[1] or (bias is not None and need[2]):
            ctx.has_bias = bias is not None
            ctx.save_for_backward(x, weight, y0, *([] if y1 is None else [y1]))
            ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.set_materialize_grads(False)      # an unused output's gradient arrives as None and enters the library as NULL
        return y0 if y1 is None else (y0, y1)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        x, weight, y0 = ctx.saved_tensors[:3]
        y1 = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        none = (None,) * 7
        if not (need_x or need_w or need_b):
            return none
        g0 = grads[0]
        g1 = grads[1] if len(grads) > 1 else None
        g0 = None if g0 is None else g0.to(x.dtype).contiguous()
        g1 = None if g1 is None else g1.to(x.dtype).contiguous()
        B, Cin, H, W = x.shape
        cout = weight.size(0)
        w32 = weight.detach().to(torch.float32).contiguous()
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty(cout, Cin, 3, 3, dtype=torch.float32, device=x.device) if need_w else None
        db = torch.empty(cout, dtype=torch.float32, device=x.device) if need_b else None
        ws = _workspace(x, cout) if (need_w or need_b) else None
        c0 = ctx.conf[0]
        _lib.call("gfla_head_conv3x3_bwd_" + _lib.suffix(x, "head_conv3x3"), x, _lib.ptr(x), _lib.ptr(w32), _lib.ptr(y0),
                  _lib.ptr(y1), _lib.ptr(g0), _lib.ptr(g1), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws),
                  B, Cin, cout, c0, H, W, *ctx.conf[1:])
        return (dx, param_grad(dw, weight.dtype), param_grad(db, ctx.bias_dtype)) + none[3:]


def _apply_post(s, posts):
    if all(p is None for p in posts):
        return s
    if all(p == posts[0] for p in posts):
        return torch.tanh(s) if posts[0] == "tanh" else torch.sigmoid(s)
    out, i = [], 0
    while i < len(posts):        # runs of equal post-activations
        j = i
        while j < len(posts) and posts[j] == posts[i]:
            j += 1
        part = s[:, i:j]
        out.append(part if posts[i] is None else torch.tanh(part) if posts[i] == "tanh" else torch.sigmoid(part))
        i = j
    return torch.cat(out, 1)


def torch_head_conv3x3(x, weight, bias=None, padding="zeros", pre_slope=None, post=None, split=None):
    """The same map as the torch composition: F.leaky_relu (F.relu for a slope of 0), F.pad(mode="reflect") or the
    convolution's own zero padding, F.conv2d, torch.tanh / torch.sigmoid.  Any dtype, any device, any Cout."""
    posts, split = _validate(x, weight, bias, padding, pre_slope, post, split)
    a = x if pre_slope is None else F.relu(x) if pre_slope == 0 else F.leaky_relu(x, pre_slope)
    if padding == "reflect":
        s = F.conv2d(F.pad(a, (1, 1, 1, 1), mode="reflect"), weight, bias)
    else:
        s = F.conv2d(a, weight, bias, padding=1)
    y = _apply_post(s, posts)
    if split is None:
        return y
    return y[:, :split].contiguous(), y[:, split:].contiguous()


def _kernel_inputs(x, weight, bias):
    if not x.is_cuda or x.dtype not in _KERNEL_DTYPES or weight.size(0) > MAX_COUT:
        return False
    return all(p is None or (p.is_cuda and p.is_floating_point() and p.dtype != torch.float64) for p in (weight, bias))


def head_conv3x3(x, weight, bias=None, padding="zeros", pre_slope=None, post=None, split=None, impl="auto"):
    """post(conv3x3(pad(leaky_relu(x, pre_slope)), weight) + bias) for x (B,Cin,H,W), weight (Cout,Cin,3,3).

    padding "zeros" | "reflect" (one pixel; reflect needs H, W >= 2).  pre_slope None: no pre-activation, 0: ReLU.  post:
    None | "tanh" | "sigmoid", or one of those per output channel.  split=C0 returns the pair (y[:, :C0], y[:, C0:]) as two
    contiguous tensors.
    impl "auto": a GPU map of float32 / float16 / bfloat16 with Cout <= 8 runs on the kernels (HeadConv3x3Function).
    Float64 tensors, CPU tensors, Cout > 8 and shapes the library refuses (_lib.Unsupported) take the torch composition
    (torch_head_conv3x3).  "torch": always the composition."""
    _lib.check_impl(impl)
    posts, split = _validate(x, weight, bias, padding, pre_slope, post, split)
    if impl == "auto" and _kernel_inputs(x, weight, bias):
        try:
            return HeadConv3x3Function.apply(x, weight, bias, padding, pre_slope, posts, split)
        except _lib.Unsupported:
            pass
    return torch_head_conv3x3(x, weight, bias, padding, pre_slope, posts, split)


class HeadConv3x3(nn.Module):
    """[LeakyReLU(pre_slope)] -> [ReflectionPad2d(1)] -> Conv2d(in_channels, out_channels, 3) -> [Tanh | Sigmoid] as one
    op.  Parameter names are nn.Conv2d's (`weight` (Cout,Cin,3,3), `bias`), initialised as nn.Conv2d initialises them, so
    state dicts interchange."""

    def __init__(self, in_channels, out_channels, bias=True, padding="zeros", pre_slope=None, post=None, split=None,
                 impl="auto"):
        super(HeadConv3x3, self).__init__()
        _lib.check_impl(impl)
        if int(in_channels) < 1 or int(out_channels) < 1:
            raise ValueError("HeadConv3x3: positive channel counts (got %r, %r)" % (in_channels, out_channels))
        if padding not in PADDINGS:
            raise ValueError("HeadConv3x3: padding is one of %s (got %r)" % (PADDINGS, padding))
        if pre_slope is not None and not float(pre_slope) >= 0:
            raise ValueError("HeadConv3x3: pre_slope is None or a slope >= 0 (got %r)" % (pre_slope,))
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.padding = padding
        self.pre_slope = None if pre_slope is None else float(pre_slope)
        self.post = _posts(post, self.out_channels)
        if split is not None and not 1 <= int(split) < self.out_channels:
            raise ValueError("HeadConv3x3: split in [1, %d) (got %r)" % (self.out_channels, split))
        self.split = None if split is None else int(split)
        self.impl = impl
        conv = nn.Conv2d(self.in_channels, self.out_channels, 3, bias=bool(bias))
        self.weight = conv.weight
        if bias:
            self.bias = conv.bias
        else:
            self.register_parameter("bias", None)

    def forward(self, x):
        return head_conv3x3(x, self.weight, self.bias, self.padding, self.pre_slope, self.post, self.split, self.impl)

    def extra_repr(self):
        return "%d, %d, padding=%r, pre_slope=%s, post=%s, split=%s, impl=%r" % (
            self.in_channels, self.out_channels, self.padding, self.pre_slope, self.post, self.split, self.impl)


def _narrow_conv(module, pad):
    """a plain nn.Conv2d the op can stand in for: its own Parameters and no hook of any kind, 3x3, stride 1, groups 1,
    dilation 1, at most MAX_COUT output channels, zero padding `pad` (0: behind an nn.ReflectionPad2d(1))"""
    return conv_geometry(module, pad == 0) == (S1K3, "zeros" if pad else "reflect") and \
        module.out_channels <= MAX_COUT and _rewrite.plain(module)


def _from_conv(conv, padding, pre_slope, post, impl):
    fused = HeadConv3x3(conv.in_channels, conv.out_channels, conv.bias is not None, padding, pre_slope, post, None, impl)
    fused.weight = conv.weight            # the same Parameter objects
    if conv.bias is not None:
        fused.bias = conv.bias
    fused.train(conv.training)
    return fused


def fuse_output_heads(module, impl="auto"):
    """Rewrite, in place and recursively, every nn.Sequential of `module` in which an optional nn.LeakyReLU | nn.ReLU, an
    optional nn.ReflectionPad2d(1), an nn.Conv2d(kernel 3, stride 1, groups 1, dilation 1, at most 8 output channels;
    padding 1 without the reflection pad, 0 with it) and an optional nn.Tanh | nn.Sigmoid follow each other: the
    convolution's slot becomes a HeadConv3x3 holding the same Parameter objects, the other slots nn.Identity().  Indices
    and state-dict keys do not change (a convolution that is also registered under another name -- the reference's
    `Output` keeps its own as `conv1` and as `model.2` -- stays there untouched: the Parameters are shared), and an
    activation instance shared with other places of the network is left as it is: only slots are replaced.  Convolutions
    that carry any forward or backward hook (spectral norm recomputes the weight in one) are left alone here:
    spectral_norm.fuse_spectral_norm(generator=True) makes a SpectralHead of a spectrally normalised head.  An activation
    built with inplace=True no longer overwrites the caller's input once it is fused: the op reads x and leaves it as it
    is.  Returns the number of heads fused."""
    _lib.check_impl(impl)
    heads = 0
    for seq in [m for m in module.modules() if isinstance(m, nn.Sequential)]:
        names = list(seq._modules.keys())
        for i, name in enumerate(names):
            prev = seq._modules[names[i - 1]] if i >= 1 else None
            has_pad = prev is not None and _rewrite.is_reflect_pad(prev)
            if not _narrow_conv(seq._modules[name], 0 if has_pad else 1):
                continue
            at = i - 1 if has_pad else i
            before = seq._modules[names[at - 1]] if at >= 1 else None
            slope = _rewrite.slope_of(before, relu=True)
            after = seq._modules[names[i + 1]] if i + 1 < len(names) else None
            post = "tanh" if type(after) is nn.Tanh else "sigmoid" if type(after) is nn.Sigmoid else None
            seq._modules[name] = _from_conv(seq._modules[name], "reflect" if has_pad else "zeros", slope, post, impl)
            if has_pad:
                seq._modules[names[i - 1]] = nn.Identity()
            if slope is not None:
                seq._modules[names[at - 1]] = nn.Identity()
            if post is not None:
                seq._modules[names[i + 1]] = nn.Identity()
            heads += 1
    return heads


def _mask_parts(mask_head):
    """(module with weight / bias, impl) of a mask head: Sequential(Conv2d, Sigmoid), or what fuse_output_heads made of it"""
    if isinstance(mask_head, nn.Sequential) and len(mask_head) == 2:
        conv, act = mask_head[0], mask_head[1]
        if _narrow_conv(conv, 1) and type(act) is nn.Sigmoid:
            return conv
        if (type(conv) is HeadConv3x3 and type(act) is nn.Identity and conv.padding == "zeros" and conv.pre_slope is None
                and all(p == "sigmoid" for p in conv.post)):
            return conv
    if (type(mask_head) is HeadConv3x3 and mask_head.padding == "zeros" and mask_head.pre_slope is None
            and all(p == "sigmoid" for p in mask_head.post)):
        return mask_head
    return None


def _flow_part(flow_conv):
    if _narrow_conv(flow_conv, 1):
        return flow_conv
    if (type(flow_conv) is HeadConv3x3 and flow_conv.padding == "zeros" and flow_conv.pre_slope is None
            and all(p is None for p in flow_conv.post) and flow_conv.split is None):
        return flow_conv
    return None


def flow_mask_heads(x, flow_conv, mask_head, impl="auto"):
    """(flow, mask) = (flow_conv(x), mask_head(x)) from one launch, for a flow head nn.Conv2d(C, F, 3, 1, 1) and a mask
    head nn.Sequential(nn.Conv2d(C, M, 3, 1, 1), nn.Sigmoid()) on the same input (either may already have been rewritten
    by fuse_output_heads), F + M <= 8.  The two convolutions' parameters are concatenated (at most 18,440 values;
    autograd splits the gradient back), identity on the flow channels and sigmoid on the mask channels; the two results
    are contiguous tensors of their own.  Heads of any other form are simply called one after the other."""
    fc, mc = _flow_part(flow_conv), _mask_parts(mask_head)
    if fc is None or mc is None or (fc.bias is None) != (mc.bias is None) or fc.weight.size(0) + mc.weight.size(0) > MAX_COUT:
        return flow_conv(x), mask_head(x)
    nf, nm = fc.weight.size(0), mc.weight.size(0)
    weight = torch.cat((fc.weight, mc.weight), 0)
    bias = None if fc.bias is None else torch.cat((fc.bias, mc.bias), 0)
    return head_conv3x3(x, weight, bias, "zeros", None, (None,) * nf + ("sigmoid",) * nm, nf, impl)


_REFERENCE_FLOW_NETS = ("PoseFlowNet", "FaceFlowNet", "ShapeNetFlowNet")


def patch_reference_flow_heads(generator_module, impl="auto"):
    """Replace `attn_output` of the reference's PoseFlowNet, FaceFlowNet and ShapeNetFlowNet (generator.py:237-242,
    578-585, 743-749: `output{i}` and `mask{i}` applied to the same tensor) with flow_mask_heads.  Idempotent.  Returns
    the names of the classes patched."""
    def make(orig):
        def attn_output(self, out, i):
            return flow_mask_heads(out, getattr(self, "output" + str(i)), getattr(self, "mask" + str(i)), impl)
        return attn_output
    return [name for name in _REFERENCE_FLOW_NETS
            if _rewrite.wrap_method(getattr(generator_module, name, None), "attn_output", "_gfla_fused_heads", make)]


def patch_reference_outputs(base_function, impl="auto"):
    """Wrap the constructor of the reference's `Output` so that every image head built from now on comes out fused
    (fuse_output_heads on the finished module).  Idempotent.  Returns True when the class was found."""
    return _rewrite.wrap_init(getattr(base_function, "Output", None), "_gfla_fuses_heads",
                              lambda self: fuse_output_heads(self, impl))
