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
        n = _lib.lib().gfla_affine_reg_workspace_bytes(B, H, W, kz)
        if n < 0:
            err = _lib.Unsupported if n == -3 else RuntimeError
            raise err("gfla_affine_reg_workspace_bytes%s: %s" % ((B, H, W, kz), _lib.lib().gfla_status_string(n).decode()))
        scratch = torch.empty(int(n), dtype=torch.uint8, device=flow.device)
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

    IMPLS = ("auto", "torch")

    def __init__(self, kz, impl="auto"):
        super(AffineRegularizationLoss, self).__init__()
        if impl not in self.IMPLS:
            raise ValueError("impl: one of %s (got %r)" % (self.IMPLS, impl))
        self.kz = kz
        self.kernel = affine_projector(kz).view(kz ** 2, kz ** 2)
        self.impl = impl

    def __call__(self, flow_fields):
        if self.impl == "auto" and flow_fields.is_cuda and flow_fields.dtype in _lib._SUFFIX and \
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
