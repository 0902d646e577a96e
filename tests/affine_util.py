"""Shared by tests/test_affine_reg_cpu.py and tests/test_affine_reg_gpu.py: flow fields, the float64 host reference and the
torch emulation of the residual form that csrc/affine_reg.hip evaluates."""
import math

import torch
import torch.nn.functional as F


def smooth_flow(B, H, W, amplitude, dtype=torch.float32, seed=0):
    """(B,2,H,W): per (b, axis) a sum of three plane waves of at most 1.5 periods across the map, peak `amplitude` px --
    the regime the regulariser drives training into (a flow that is nearly affine inside every window)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1) / H
    x = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W) / W
    f = torch.zeros(B, 2, H, W, dtype=torch.float64)
    for _ in range(3):
        fy, fx = (torch.rand(B, 2, 1, 1, generator=g, dtype=torch.float64) * 3 - 1.5 for _ in range(2))
        phase = torch.rand(B, 2, 1, 1, generator=g, dtype=torch.float64) * 2 * math.pi
        f = f + torch.sin(2 * math.pi * (fy * y + fx * x) + phase)
    f = f * (amplitude / f.abs().amax(dim=(2, 3), keepdim=True))
    return f.to(dtype).contiguous()


def noise_flow(B, H, W, sigma, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 2, H, W, generator=g, dtype=torch.float64) * sigma).to(dtype).contiguous()


def reference(flow, kz):
    """(loss, d loss / d flow) of today's torch composition (AffineRegularizationLoss.calculate_loss on flow + grid) on the
    host in float64, on the values of `flow` as stored."""
    from global_flow_local_attention_amd.losses import AffineRegularizationLoss
    f = flow.detach().cpu().double().requires_grad_()
    loss = AffineRegularizationLoss(kz)(f)
    loss.backward()
    return loss.item(), f.grad


def residual_form(flow, kz):
    """The formulation of csrc/affine_reg.hip in torch ops, in flow's dtype: per window subtract its first element, fit
    the least-squares plane a + bx dx + by dy, sum the squared residuals; mean over (b, windows), summed over the axes."""
    B, _, H, W = flow.shape
    c = (kz - 1) / 2.0
    ramp = torch.arange(kz, dtype=flow.dtype) - c
    dy = ramp.repeat_interleave(kz).view(1, -1, 1)
    dx = ramp.repeat(kz).view(1, -1, 1)
    s = kz ** 2 * (kz ** 2 - 1) / 12.0
    total = 0
    for axis in range(2):
        f = F.unfold(flow[:, axis:axis + 1], kz)          # (B, kz^2, L)
        f = f - f[:, 0:1]
        a = f.mean(1, keepdim=True)
        by = (f * dy).sum(1, keepdim=True) / s
        bx = (f * dx).sum(1, keepdim=True) / s
        r = f - a - by * dy - bx * dx
        total = total + (r * r).sum(1).mean()
    return total
