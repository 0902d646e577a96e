"""Bilinear flow warp on gfx950 (csrc/flow_warp.hip): the reference's three `grid_sample` warps as one op.

For an output position (x, y) of an H x W flow and an Hs x Ws source the sampling position in source pixels is
    ix = (x + gx * flow_x) * mx ,   iy = (y + gy * flow_y) * my
and the output is the bilinear interpolation of the source there, with zero padding: `grid_sample(mode="bilinear",
padding_mode="zeros", align_corners=True)` (the convention of the torch the reference targets, correctness.py) without
the normalised grid.  The reference's three warps differ in the four scalars only:

    "correctness"  PerceptualCorrectness.bilinear_warp (external_function.py:309-319)   gx = (w-1)/w, gy = (h-1)/h
    "block"        BilinearSamplingBlock.forward (base_function.py:490-506): both axes are divided by w - 1, a quirk
                   that is kept                                                          my = (h-1)/(w-1)
    "pixel"        the `visi` warp (poseflownet_model.py:86-103): the flow is a pixel offset, all four scalars are 1

(h, w: the SOURCE's size, which is what the reference's formulas use; scalars not listed are 1.)
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function

from . import _lib

CONVENTIONS = ("correctness", "block", "pixel")
IMPLS = _lib.IMPLS


def convention_scalars(convention, hs, ws):
    """(gx, gy, mx, my) of `convention` for an hs x ws source."""
    if convention == "correctness":
        return (ws - 1) / ws, (hs - 1) / hs, 1.0, 1.0
    if convention == "block":
        # (w = 1 divides by zero in the reference too; the identity keeps a one-column map usable)
        return 1.0, 1.0, 1.0, ((hs - 1) / (ws - 1) if ws > 1 else 1.0)
    if convention == "pixel":
        return 1.0, 1.0, 1.0, 1.0
    raise ValueError("convention: one of %s (got %r)" % (CONVENTIONS, convention))


class FlowWarpFunction(Function):
    """(source (B,C,Hs,Ws), flow (B,2,H,W), gx, gy, mx, my) -> warped (B,C,H,W), on the library's kernels.

    source: float32 / float64 / float16 / bfloat16, read as stored.  flow: float32 (float64 with a float64 source).  The
    warped map is in the FLOW's dtype: float32 for 16-bit sources (interpolated in float32, rounded once at the store).
    d/d flow has one writer per element and a fixed summation order: it is bit-identical from call to call.  d/d source
    is accumulated with float atomics into a buffer of the flow's dtype (zero-filled by the library) and rounded to the
    source's dtype once; it is the one output of the op that is NOT bit-reproducible, and it is only launched when the
    source needs a gradient."""

    @staticmethod
    def forward(ctx, source, flow, gx, gy, mx, my):
        _lib.require_gpu(source, flow)
        sfx = _lib.suffix(source, "flow_warp")
        want = torch.float64 if source.dtype == torch.float64 else torch.float32
        if flow.dtype != want:
            raise TypeError("flow_warp: a %s source takes a %s flow (got %s)" % (source.dtype, want, flow.dtype))
        if source.dim() != 4 or flow.dim() != 4 or flow.size(1) != 2 or flow.size(0) != source.size(0):
            raise ValueError("flow_warp: source (B,C,Hs,Ws) and flow (B,2,H,W) (got %s, %s)"
                             % (tuple(source.shape), tuple(flow.shape)))
        source, flow = source.contiguous(), flow.contiguous()
        B, C, Hs, Ws = source.shape
        H, W = flow.shape[2:]
        ctx.scalars = (float(gx), float(gy), float(mx), float(my))
        ctx.save_for_backward(source, flow)
        out = flow.new_empty((B, C, H, W))
        if out.numel() == 0 or source.numel() == 0:
            return out.zero_()
        _lib.call("gfla_flow_warp_fwd_" + sfx, source, _lib.ptr(source), _lib.ptr(flow), _lib.ptr(out), B, C, Hs, Ws, H, W,
                  *ctx.scalars)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        source, flow = ctx.saved_tensors
        need_s, need_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g_src = torch.empty(source.shape, dtype=flow.dtype, device=source.device) if need_s else None
        g_flow = torch.empty_like(flow) if need_f else None
        if need_s or need_f:
            if grad_out.numel() == 0 or source.numel() == 0:
                for g in (g_src, g_flow):
                    if g is not None:
                        g.zero_()
            else:
                B, C, Hs, Ws = source.shape
                H, W = flow.shape[2:]
                grad_out = grad_out.to(flow.dtype).contiguous()
                _lib.call("gfla_flow_warp_bwd_" + _lib.suffix(source, "flow_warp"), source, _lib.ptr(source), _lib.ptr(flow),
                          _lib.ptr(grad_out), _lib.ptr(g_src), _lib.ptr(g_flow), B, C, Hs, Ws, H, W, *ctx.scalars)
        if g_src is not None and g_src.dtype != source.dtype:
            g_src = g_src.to(source.dtype)
        return g_src, g_flow, None, None, None, None


def torch_flow_warp(source, flow, gx, gy, mx, my):
    """The same warp as a torch composition: the normalised grid of the pixel position, then `F.grid_sample(...,
    align_corners=True)`.  The result is in the flow's dtype (a source of another dtype is cast to it, as autocast does
    for grid_sample).  A source axis of size 1 has no normalised coordinate (0 / 0); it is padded with one zero row /
    column, which zero padding makes the same map."""
    if source.dtype != flow.dtype:
        source = source.to(flow.dtype)
    h, w = flow.shape[2:]
    pad_x, pad_y = int(source.size(3) == 1), int(source.size(2) == 1)
    if pad_x or pad_y:
        source = F.pad(source, (0, pad_x, 0, pad_y))
    hs, ws = source.shape[2:]
    xs = torch.arange(w, device=flow.device, dtype=flow.dtype).view(1, 1, w)
    ys = torch.arange(h, device=flow.device, dtype=flow.dtype).view(1, h, 1)
    ix = (xs + gx * flow[:, 0]) * mx
    iy = (ys + gy * flow[:, 1]) * my
    grid = torch.stack([2 * ix / (ws - 1) - 1, 2 * iy / (hs - 1) - 1], dim=-1)
    return F.grid_sample(source, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def _kernel_dtypes(source, flow):
    if not (source.is_cuda and flow.is_cuda) or source.dtype not in _lib.SUFFIX:
        return False
    return flow.dtype == (torch.float64 if source.dtype == torch.float64 else torch.float32)


def flow_warp(source, flow, convention="pixel", impl="auto"):
    """Warp `source` (B,C,Hs,Ws) by `flow` (B,2,H,W) in one of the reference's conventions -> (B,C,H,W).

    impl "auto": GPU tensors (float32 / float16 / bfloat16 source with a float32 flow, float64 with float64) run on the
    kernels of csrc/flow_warp.hip.  CPU tensors and any other dtype pairing take the torch composition (torch_flow_warp).
    impl "torch": always the composition.  On either route a 16-bit flow is up-cast to float32 first (a 16-bit flow of
    32-64 px has steps of 0.25-0.5 px in bfloat16; its gradient is cast back), and 16-bit sources give a float32 map."""
    _lib.check_impl(impl)
    scalars = convention_scalars(convention, source.size(2), source.size(3))
    if flow.dtype in _lib.HALF_TYPES:
        flow = flow.float()     # (autograd casts the flow's gradient back)
    if impl == "auto" and _kernel_dtypes(source, flow):
        return FlowWarpFunction.apply(source, flow, *scalars)
    return torch_flow_warp(source, flow, *scalars)


class FlowWarp(nn.Module):
    """flow_warp as a module: `FlowWarp(convention, impl)(source, flow)`."""

    def __init__(self, convention="pixel", impl="auto"):
        super(FlowWarp, self).__init__()
        if convention not in CONVENTIONS:
            raise ValueError("convention: one of %s (got %r)" % (CONVENTIONS, convention))
        _lib.check_impl(impl)
        self.convention = convention
        self.impl = impl

    def forward(self, source, flow):
        return flow_warp(source, flow, self.convention, self.impl)


class BilinearSamplingBlock(nn.Module):
    """The reference's class (base_function.py:490-506), same constructor and call; the grid is never built, so nothing
    is moved to a device here."""

    def __init__(self):
        super(BilinearSamplingBlock, self).__init__()

    def forward(self, source, flow_field):
        return flow_warp(source, flow_field, "block", "auto")
