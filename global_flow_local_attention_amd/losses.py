"""Loss-side consumers of the hot path, restated so they need fewer passes.

`AffineRegularizationLoss` (reference: model/networks/external_function.py:31-77) runs, per flow field
and per axis, conv2d(grid, K) -> LocalAttnReshape -> BlockExtractor(grid, const flow k//2) -> multiply
-> avg_pool2d -> mean * k^2.  With u = the k x k patch of the sampling grid at a valid position,
conv2d gives (M u), the extractor at the constant integer flow k//2 returns exactly u (bilinear
weights 1/0), and avg_pool of the product is u.(M u)/k^2.  So the whole chain is

        loss_axis = mean over (b, valid positions) of  u^T M u ,      M = K^T K  (k^2 x k^2, fixed)

one unfold + one small GEMM + one reduction (`calculate_loss`: the torch composition, which CPU tensors take).  The
reference's op-by-op composition lives in oracle/cpu_modules.py (AffineRegularizationLossOpByOp, test infrastructure);
goldens produced by the reference's own class pin both (tests/golden/make_affine_golden.py).

On the GPU the loss runs on the library's own kernels (`AffineRegFunction`, csrc/affine_reg.hip).  M = I - P with P the
projector on the affine functions of the patch, and the pixel coordinates inside u are such a function, so

        u^T M u = f^T M f = |f - P f|^2 ,      f = the k x k patch of the FLOW of one axis

the squared residual of the least-squares plane through the flow patch.  The kernels read the flow as it is stored
(float16 / bfloat16 included) and never form flow + grid; under torch.autocast the composition rounds u (coordinates up
to the map size) and M to 16 bits before a product whose result is the small difference of large numbers (DESIGN.md
section 5).

`VGGLoss` / `StyleLoss` / `PerceptualLoss` (external_function.py:121-220) keep the reference's surface around an injected
feature extractor.  The style term, L1 of the difference of two Gram matrices, runs on csrc/gram_l1.hip for GPU features
(`gram_l1`, `GramL1Function`): float32 sums on the matrix cores from the features as stored, where the composition's bmm
is on autocast's 16-bit list and rounds -- or overflows -- each Gram entry before the subtraction.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib

KZ_MIN, KZ_MAX = 2, 7   # window sizes the kernels take (kz = 1 has no projector: A^T A is singular)


def affine_projector(kz):
    """M = K^T K with K = A (A^T A)^-1 A^T - I, A = [x, y, 1] over the kz x kz patch
    (external_function.py:41-47)."""
    temp = np.arange(kz)
    A = np.ones([kz * kz, 3])
    A[:, 0] = temp.repeat(kz)
    A[:, 1] = temp.repeat(kz).reshape((kz, kz)).transpose().reshape(kz ** 2)
    AH = A.transpose()
    k = np.dot(A, np.dot(np.linalg.inv(np.dot(AH, A)), AH)) - np.identity(kz ** 2)
    return torch.from_numpy(np.dot(k.transpose(), k))


class AffineRegFunction(Function):
    """(flow (B,2,H,W), kz) -> loss_x + loss_y of AffineRegularizationLoss as one 0-dim tensor: float32 for float32 /
    float16 / bfloat16 flows, float64 for float64.  One forward and one backward kernel (gfla_affine_reg_fwd / _bwd); the
    flow is read in its storage type, the fit and the sums are float64 whatever torch.autocast says, and loss and d/d flow
    are rounded once, at their stores (d/d flow in the flow's dtype).  Bit-identical from call to call (no atomics)."""

    @staticmethod
    def forward(ctx, flow, kz):
        _lib.require_gpu(flow)
        sfx, kz = _lib.suffix(flow, "affine regularisation loss"), int(kz)
        if flow.dim() != 4 or flow.size(1) != 2:
            raise ValueError("affine regularisation loss: flow must be (B,2,H,W), got %s" % (tuple(flow.shape),))
        B, _, H, W = flow.shape
        if H < kz or W < kz:
            raise ValueError("affine regularisation loss: a %dx%d map has no %dx%d window" % (H, W, kz, kz))
        flow = flow.contiguous()
        scratch = _lib.workspace("gfla_affine_reg_workspace_bytes", flow, B, H, W, kz, what="affine regularisation loss")
        loss = torch.empty((), dtype=torch.float64 if flow.dtype == torch.float64 else torch.float32, device=flow.device)
        _lib.call("gfla_affine_reg_fwd_" + sfx, flow, _lib.ptr(flow), _lib.ptr(scratch), _lib.ptr(loss), B, H, W, kz)
        ctx.kz = kz
        ctx.save_for_backward(flow)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None
        flow, = ctx.saved_tensors
        B, _, H, W = flow.shape
        grad_loss = grad_loss.to(torch.float64 if flow.dtype == torch.float64 else torch.float32).contiguous()
        grad_flow = torch.empty_like(flow)
        _lib.call("gfla_affine_reg_bwd_" + _lib.suffix(flow, "affine regularisation loss"), flow, _lib.ptr(flow),
                  _lib.ptr(grad_loss), None, _lib.ptr(grad_flow), B, H, W, ctx.kz)
        return grad_flow, None


class AffineRegularizationLoss(nn.Module):
    """Same constructor/call as the reference (external_function.py:31-77).

    `impl` (instance attribute): "auto" -- GPU flows of float32 / float64 / float16 / bfloat16 with 2 <= kz <= 7 take the
    library's kernels (AffineRegFunction), everything else the torch composition below; "torch" -- always the composition
    (cross-checks, tools/bench_affine_reg.py)."""

    IMPLS = _lib.IMPLS

    def __init__(self, kz, impl="auto"):
        super(AffineRegularizationLoss, self).__init__()
        _lib.check_impl(impl)
        self.kz = kz
        self.kernel = affine_projector(kz).view(kz ** 2, kz ** 2)
        self.impl = impl

    def __call__(self, flow_fields):
        if self.impl == "auto" and flow_fields.is_cuda and flow_fields.dtype in _lib.SUFFIX and \
                KZ_MIN <= self.kz <= KZ_MAX:
            return AffineRegFunction.apply(flow_fields, self.kz)
        grid = self.flow2grid(flow_fields)
        weights = self.kernel.type_as(flow_fields)
        loss_x = self.calculate_loss(grid[:, 0:1], weights)
        loss_y = self.calculate_loss(grid[:, 1:2], weights)
        return loss_x + loss_y

    def calculate_loss(self, grid, weights):
        u = F.unfold(grid, self.kz)          # (B, kz^2, L): the valid kz x kz patches
        mu = torch.matmul(weights, u)        # M u
        return (u * mu).sum(1).mean()

    def flow2grid(self, flow_field):
        b, c, h, w = flow_field.size()
        x = torch.arange(w).view(1, -1).expand(h, -1).type_as(flow_field).float()
        y = torch.arange(h).view(-1, 1).expand(-1, w).type_as(flow_field).float()
        grid = torch.stack([x, y], dim=0).unsqueeze(0).expand(b, -1, -1, -1)
        return flow_field + grid


class MultiAffineRegularizationLoss(nn.Module):
    """external_function.py:12-27: one AffineRegularizationLoss per attention layer."""

    def __init__(self, kz_dic, impl="auto"):
        super(MultiAffineRegularizationLoss, self).__init__()
        self.kz_dic = kz_dic
        self.method_dic = {}
        for key in kz_dic:
            self.method_dic[key] = AffineRegularizationLoss(kz_dic[key], impl)
        self.layers = sorted(kz_dic, reverse=True)
        self.impl = impl   # "auto" | "torch", handed to every layer's loss at each call

    def __call__(self, flow_fields):
        loss = 0
        for i in range(len(flow_fields)):
            method = self.method_dic[self.layers[i]]
            method.impl = self.impl
            loss += method(flow_fields[i])
        return loss


# ---- style and content loss (VGGLoss, external_function.py:121-220) --------------------------------------------------
STYLE_LAYERS = ("relu2_2", "relu3_4", "relu4_4", "relu5_2")
CONTENT_LAYERS = ("relu1_1", "relu2_1", "relu3_1", "relu4_1", "relu5_1")
GRAM_IMPLS = _lib.IMPLS
_GRAM_SUFFIX = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}


def compute_gram(x):
    """external_function.py:134-139: G = F F^T / (h w ch), F = x viewed as (b, ch, h w)."""
    b, ch, h, w = x.size()
    f = x.reshape(b, ch, w * h)
    f_T = f.transpose(1, 2)
    return f.bmm(f_T) / (h * w * ch)


class GramL1Function(Function):
    """(x, y), both (B,C,H,W) or (B,C,N), one dtype of float32 / float16 / bfloat16, on the GPU -> mean |G(x) - G(y)| as a
    0-dim float32 tensor (csrc/gram_l1.hip).  The features are read as stored; both Grams are summed in float32 on the
    matrix cores whatever torch.autocast says, separately and in the same order (x == y gives exactly 0), and D = G(x) -
    G(y) is saved for the backward: d/dx = +g 2/(B C^3 N) sign(D) F_x, d/dy = -g 2/(B C^3 N) sign(D) F_y, each stored once
    in the features' dtype and only for an input that needs it.  Bit-identical from call to call (no atomics)."""

    @staticmethod
    def forward(ctx, x, y):
        _lib.require_gpu(x, y)
        if x.dtype != y.dtype:
            raise TypeError("gram l1 loss: x and y must have one dtype (got %s and %s)" % (x.dtype, y.dtype))
        if x.dtype not in _GRAM_SUFFIX:
            raise TypeError("gram l1 loss: unsupported dtype %s (float32, float16, bfloat16)" % x.dtype)
        if x.dim() not in (3, 4) or x.shape != y.shape:
            raise ValueError("gram l1 loss: x and y must be (B,C,H,W) or (B,C,N) of one shape, got %s and %s"
                             % (tuple(x.shape), tuple(y.shape)))
        if x.numel() == 0:
            raise ValueError("gram l1 loss: empty features %s" % (tuple(x.shape),))
        sfx = _GRAM_SUFFIX[x.dtype]
        x, y = x.contiguous(), y.contiguous()
        B, C = x.shape[:2]
        N = x.numel() // (B * C)
        scratch = _lib.workspace("gfla_gram_l1_workspace_bytes", x, B, C, N, what="gram l1 loss")
        diff = torch.empty((B, C, C), dtype=torch.float32, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        _lib.call("gfla_gram_l1_fwd_" + sfx, x, _lib.ptr(x), _lib.ptr(y), _lib.ptr(scratch), _lib.ptr(diff),
                  _lib.ptr(loss), B, C, N)
        ctx.save_for_backward(x, y, diff)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        x, y, diff = ctx.saved_tensors
        B, C = x.shape[:2]
        N = x.numel() // (B * C)
        grad_loss = grad_loss.to(torch.float32).contiguous()
        grads = [None, None]
        for i, feat in enumerate((x, y)):
            if ctx.needs_input_grad[i]:
                grads[i] = torch.empty_like(feat)
                _lib.call("gfla_gram_l1_bwd_" + _GRAM_SUFFIX[feat.dtype], feat, _lib.ptr(feat), _lib.ptr(diff),
                          _lib.ptr(grad_loss), _lib.ptr(grads[i]), B, C, N, i)
        return grads[0], grads[1]


def gram_l1(x, y, impl="auto"):
    """L1Loss(compute_gram(x), compute_gram(y)): one style layer of VGGLoss.  impl "auto": GPU features of one dtype among
    float32 / float16 / bfloat16 take the library's kernels (GramL1Function); CPU tensors, float64, mixed dtypes and
    shapes the kernels refuse (_lib.Unsupported) take the torch composition, the reference's arithmetic.  "torch": always
    the composition."""
    _lib.check_impl(impl)
    if impl == "auto" and x.is_cuda and y.is_cuda and x.dtype == y.dtype and x.dtype in _GRAM_SUFFIX:
        try:
            return GramL1Function.apply(x, y)
        except _lib.Unsupported:
            pass
    return F.l1_loss(compute_gram(x), compute_gram(y))


class _VggLossBase(nn.Module):
    """The feature extractor is injected (`vgg`: callable image -> {layer name: feature map}), as in
    PerceptualCorrectness: neither torchvision nor its weights are part of this package."""

    def __init__(self, vgg, impl):
        super(_VggLossBase, self).__init__()
        _lib.check_impl(impl)
        if isinstance(vgg, nn.Module):
            self.add_module('vgg', vgg)
        else:
            self.vgg = vgg
        self.criterion = torch.nn.L1Loss()
        self.impl = impl   # "auto" | "torch": how the Gram term is evaluated (gram_l1)

    def compute_gram(self, x):
        return compute_gram(x)

    def _features(self, x, y):
        if self.vgg is None:
            raise RuntimeError("%s needs a feature extractor: pass vgg=... (image -> dict of feature maps)"
                               % type(self).__name__)
        return self.vgg(x), self.vgg(y)

    def _content(self, x_vgg, y_vgg):
        content_loss = 0.0
        for weight, layer in zip(self.weights, CONTENT_LAYERS):
            content_loss += weight * self.criterion(x_vgg[layer], y_vgg[layer])
        return content_loss

    def _style(self, x_vgg, y_vgg):
        style_loss = 0.0
        for layer in STYLE_LAYERS:
            style_loss += gram_l1(x_vgg[layer], y_vgg[layer], self.impl)
        return style_loss


class VGGLoss(_VggLossBase):
    """external_function.py:121-160: (x, y) -> (content_loss, style_loss).  Content: weighted L1 over relu1_1 .. relu5_1
    (F.l1_loss: float32 under autocast, not a GEMM).  Style: gram_l1 over relu2_2, relu3_4, relu4_4, relu5_2."""

    def __init__(self, weights=[1.0, 1.0, 1.0, 1.0, 1.0], vgg=None, impl="auto"):
        super(VGGLoss, self).__init__(vgg, impl)
        self.weights = weights

    def __call__(self, x, y):
        x_vgg, y_vgg = self._features(x, y)
        return self._content(x_vgg, y_vgg), self._style(x_vgg, y_vgg)


class StyleLoss(_VggLossBase):
    """external_function.py:162-193: (x, y) -> style_loss."""

    def __init__(self, vgg=None, impl="auto"):
        super(StyleLoss, self).__init__(vgg, impl)

    def __call__(self, x, y):
        return self._style(*self._features(x, y))


class PerceptualLoss(_VggLossBase):
    """external_function.py:197-220: (x, y) -> content_loss."""

    def __init__(self, weights=[1.0, 1.0, 1.0, 1.0, 1.0], vgg=None, impl="auto"):
        super(PerceptualLoss, self).__init__(vgg, impl)
        self.weights = weights

    def __call__(self, x, y):
        return self._content(*self._features(x, y))


class StyleContentLoss(nn.Module):
    """(generated, target) -> lambda_style * style + lambda_content * content of VGGLoss (pose_model.py:35-36, 174-176):
    the callable TrainerShell(style_content_loss=...) expects."""

    def __init__(self, vgg, lambda_style=500.0, lambda_content=0.5, impl="auto"):
        super(StyleContentLoss, self).__init__()
        self.vgg_loss = VGGLoss(vgg=vgg, impl=impl)
        self.lambda_style, self.lambda_content = lambda_style, lambda_content

    def forward(self, generated, target):
        content, style = self.vgg_loss(generated, target)
        return style * self.lambda_style + content * self.lambda_content


class AdversarialLoss(nn.Module):
    """The adversarial term of the reference's models (external_function.py AdversarialLoss), from the formulas:
    nsgan  binary cross entropy of D, a probability, against the label (nn.BCELoss, as the reference: a discriminator
           that ends in a sigmoid)                                 lsgan  mean squared error against the label
    hinge  for the discriminator mean(relu(1 - D)) on real and mean(relu(1 + D)) on fake samples, for the generator
           -mean(D)
    Call: (outputs, is_real, for_dis=None); the label is target_real_label / target_fake_label, constant over outputs."""

    TYPES = ("nsgan", "lsgan", "hinge")

    def __init__(self, type="nsgan", target_real_label=1.0, target_fake_label=0.0):
        super(AdversarialLoss, self).__init__()
        if type not in self.TYPES:
            raise ValueError("AdversarialLoss: type is one of %s (got %r)" % (self.TYPES, type))
        self.type = type
        self.real_label, self.fake_label = float(target_real_label), float(target_fake_label)

    def forward(self, outputs, is_real, for_dis=None):
        if self.type == "hinge":
            if for_dis:
                return F.relu(1.0 - outputs if is_real else 1.0 + outputs).mean()
            return -outputs.mean()
        labels = torch.full_like(outputs, self.real_label if is_real else self.fake_label)
        if self.type == "nsgan":
            return F.binary_cross_entropy(outputs, labels)
        return F.mse_loss(outputs, labels)


def gan_generator_term(net_D, loss, weight=1.0):
    """(generated, target) -> weight * loss(net_D(generated), True, False): the callable TrainerShell(gan_loss=...)
    expects (pose_model.py:150-153).  D runs with its parameters' requires_grad off, as the reference's _freeze does, so the
    generator's step leaves no gradient on D; the flags are restored as they were found."""
    def term(generated, target):
        params = list(net_D.parameters())
        flags = [p.requires_grad for p in params]
        for p in params:
            p.requires_grad_(False)
        try:
            return loss(net_D(generated), True, False) * weight
        finally:
            for p, flag in zip(params, flags):
                p.requires_grad_(flag)
    return term
