"""Sampling-correctness loss on the gfx950 ops.

Reference: `PerceptualCorrectness` (model/networks/external_function.py:223-319).  Per flow field it
  1. normalises the VGG features of source and target over channels and takes, for every target
     position, the best cosine similarity over ALL source positions -- through a materialised
     [b, N^2, N^2] `bmm` (:255-268);
  2. warps the source features with `Resample2d(4, 1, sigma=2)` (or `grid_sample`), takes the cosine
     similarity with the target features at the same position, and
  3. averages exp(-sample / (best + eps)), optionally under a mask (:270-277).

Step 1 is `max_cosine_similarity` below: one MFMA kernel in libgfla_hip.so that keeps the
similarity matrix in registers (gfla_max_cosine_fwd_f32; float16 / bfloat16 features run on the 16-bit
matrix cores, gfla_max_cosine_fwd_f16 / _bf16).  Step 2 uses this package's Resample2d, or its bilinear
flow warp (flow_warp.py) for `use_bilinear_sampling=True`.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

from . import _lib
from .flow_warp import IMPLS as WARP_IMPLS, flow_warp
from .resample2d import Resample2d


class MaxCosineFunction(Function):
    """(source (B,C,Ns), target (B,C,Nt), eps) -> (best (B,Nt), index (B,Nt) int32).

    best[b,j] = max_i <source[b,:,i]/(|.|+eps), target[b,:,j]/(|.|+eps)>  (external_function.py:260-268).
    Backward re-evaluates the winning pairs only (B*C*Nt work): the max routes the gradient to one source
    position per target position, exactly as torch.max(dim=1) does in the reference.

    float32, or float16 / bfloat16 with source and target of one dtype.  For 16-bit features `best` is float32 (it
    divides a loss term; the kernel accumulates in float32 and nothing is gained by rounding it), the backward is
    evaluated in float32 and the gradients are returned in the features' dtype.
    """

    @staticmethod
    def forward(ctx, source, target, eps):
        _lib.require_gpu(source, target)
        if source.dtype != target.dtype or source.dtype not in (torch.float32,) + _lib.HALF_TYPES:
            raise TypeError("max_cosine_similarity: float32, float16 or bfloat16 features, source and target of one dtype "
                            "(got %s, %s)" % (source.dtype, target.dtype))
        assert source.is_contiguous() and target.is_contiguous()
        assert source.dim() == 3 and target.dim() == 3
        B, C, Ns = source.shape
        assert target.size(0) == B and target.size(1) == C
        Nt = target.size(2)
        best = torch.empty(B, Nt, dtype=torch.float32, device=source.device)
        index = torch.empty(B, Nt, dtype=torch.int32, device=source.device)
        scratch = _lib.workspace("gfla_max_cosine_workspace_bytes", source, B, Ns, Nt, what="max_cosine_similarity")
        _lib.call("gfla_max_cosine_fwd_" + _lib.suffix(source, "max_cosine_similarity"), source, _lib.ptr(source), _lib.ptr(target), _lib.ptr(scratch),
                  _lib.ptr(best), _lib.ptr(index), B, C, Ns, Nt, float(eps))
        ctx.eps = eps
        ctx.save_for_backward(source, target, index)
        ctx.mark_non_differentiable(index)
        return best, index

    @staticmethod
    def backward(ctx, grad_best, _grad_index):
        source, target, index = ctx.saved_tensors
        need_s, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_s or need_t):
            return None, None, None
        half = source.dtype in _lib.HALF_TYPES
        with torch.enable_grad():
            # the winners are gathered in the storage type (no float32 copy of a 16-bit source map); from there on
            # float32, with the winners and the target as the leaves
            gather_at = index.long().unsqueeze(1).expand(-1, source.size(1), -1)
            winners = torch.gather(source.detach(), 2, gather_at).float().requires_grad_(need_s)
            t = target.detach().float().requires_grad_(need_t)
            leaf_s = winners
            winners = winners / (winners.norm(dim=1, keepdim=True) + ctx.eps)
            t_unit = t / (t.norm(dim=1, keepdim=True) + ctx.eps)
            best = (winners * t_unit).sum(1)
            wanted = [x for x, need in ((leaf_s, need_s), (t, need_t)) if need]
            grads = list(torch.autograd.grad(best, wanted, grad_best.float()))
        if need_s:
            # Route the winners' gradients to their source positions: float32 sums, one rounding at the end.  The positions
            # that won nothing get 0 -- or NaN where the reference gets NaN: its bmm multiplies their zero gradient with
            # EVERY normalised target position, so one non-finite target position makes the whole sample's source gradient
            # NaN (0 x NaN).  The sums start from that value: 0, or NaN for such a sample (the normalised target has entries
            # of at most 1 and NaN for a non-finite position, so its sum is NaN exactly then).
            taint = (t_unit.detach().sum(dim=(1, 2)) * 0).view(-1, 1, 1)
            g_src = taint.expand(source.shape).contiguous()
            grads[0] = g_src.scatter_add_(2, gather_at, grads[0])
        if half:
            grads = [g.to(source.dtype) for g in grads]
        return (grads.pop(0) if need_s else None), (grads.pop(0) if need_t else None), None


class CorrectnessMapFunction(Function):
    """(warped (B,C,N), target (B,C,N), best (B,N), eps) -> exp(-cosine_similarity(warped, target) / (best + eps)),
    external_function.py:275-276, as one pass forward and one backward.

    All float32, or a float32 `warped` with a float16 / bfloat16 `target`: the target is read in its storage type, the
    loss map and the gradients of `warped` and `best` are float32, the gradient of `target` is returned in its dtype."""

    COS_EPS = 1e-8  # F.cosine_similarity's default

    @staticmethod
    def forward(ctx, warped, target, best, eps):
        _lib.require_gpu(warped, target, best)
        if warped.dtype != torch.float32 or best.dtype != torch.float32 or \
                target.dtype not in (torch.float32,) + _lib.HALF_TYPES:
            raise TypeError("correctness map: float32 warped and best, float32 / float16 / bfloat16 target (got %s, %s, %s)"
                            % (warped.dtype, target.dtype, best.dtype))
        for x in (warped, target, best):
            assert x.is_contiguous()
        B, C, N = warped.shape
        assert target.shape == warped.shape and best.shape == (B, N)
        loss_map = warped.new_empty(B, N)
        stats = warped.new_empty(B, N, 3)
        _lib.call("gfla_correctness_map_fwd_" + _lib.suffix(target, "correctness map"), warped, _lib.ptr(warped), _lib.ptr(target), _lib.ptr(best),
                  _lib.ptr(loss_map), _lib.ptr(stats), B, C, N, CorrectnessMapFunction.COS_EPS, float(eps))
        ctx.eps = eps
        ctx.save_for_backward(warped, target, best, stats, loss_map)
        return loss_map

    @staticmethod
    def backward(ctx, grad_map):
        warped, target, best, stats, loss_map = ctx.saved_tensors
        B, C, N = warped.shape
        need = ctx.needs_input_grad
        g_warped = torch.empty_like(warped) if need[0] else None
        g_target = torch.empty_like(target) if need[1] else None
        g_best = torch.empty_like(best) if need[2] else None
        if any(need[:3]):
            _lib.call("gfla_correctness_map_bwd_" + _lib.suffix(target, "correctness map"), warped, _lib.ptr(warped), _lib.ptr(target), _lib.ptr(best),
                      _lib.ptr(stats), _lib.ptr(loss_map), _lib.ptr(grad_map.contiguous()), _lib.ptr(g_warped),
                      _lib.ptr(g_target), _lib.ptr(g_best), B, C, N, CorrectnessMapFunction.COS_EPS, float(ctx.eps))
        return g_warped, g_target, g_best, None


def max_cosine_similarity(source, target, eps=1e-8, return_index=False):
    """Best cosine match over all source positions for every target position.

    source (B,C,...) and target (B,C,...) feature maps (any trailing spatial shape); returns (B, Nt)
    [and the int32 index of the winning source position]."""
    B, C = source.shape[:2]
    best, index = MaxCosineFunction.apply(source.reshape(B, C, -1).contiguous(),
                                          target.reshape(B, C, -1).contiguous(), eps)
    return (best, index) if return_index else best


class PerceptualCorrectness(nn.Module):
    """Same call surface as the reference class (external_function.py:223-319).

    The reference builds a pretrained torchvision VGG19 in its constructor; here the feature extractor
    is injected (`vgg`: callable image -> {layer name: feature map}), because neither torchvision nor
    its weights are part of this package.  `calculate_loss` works on `self.target_vgg` /
    `self.source_vgg` exactly as the reference's does, so it can also be driven with precomputed
    features.

    `half_features`: what `calculate_loss` does with float16 / bfloat16 features (torch.autocast).  "float32" (default):
    features, flow and mask are up-cast and the float32 kernels run.  "native": the best match runs on the 16-bit
    features as they are (16-bit matrix cores) and the target map is never up-cast.  The flow stays float32 (a 16-bit
    flow of 32-64 px has steps of 0.25-0.5 px in bfloat16).  With the Resample2d warp the source map is up-cast once,
    for the warp; with `use_bilinear_sampling=True` the flow-warp kernel reads the 16-bit source as stored and returns
    the float32 warped map, so nothing is up-cast.  The loss map, the mask arithmetic and the returned loss are float32
    either way.  "native" needs the fused loss map and source and target of one 16-bit dtype; `fused = False` and mixed
    feature dtypes are evaluated as under "float32".

    `warp_impl` (instance attribute, "auto" | "torch"): how `bilinear_warp` is evaluated.  "auto": GPU features go
    through the kernels of csrc/flow_warp.hip in the "correctness" convention, anything else through torch.  "torch":
    the normalised grid and `F.grid_sample`, as the reference writes it.
    """

    HALF_FEATURES = ("float32", "native")

    def __init__(self, layer=['rel1_1', 'relu2_1', 'relu3_1', 'relu4_1'], vgg=None, half_features="float32"):
        super(PerceptualCorrectness, self).__init__()
        if isinstance(vgg, nn.Module):
            self.add_module('vgg', vgg)
        else:
            self.vgg = vgg
        self.layer = layer
        self.eps = 1e-8
        self.resample = Resample2d(4, 1, sigma=2)
        # grid_sample convention of `bilinear_warp`: the reference targets PyTorch 1.0.0 (README.md:93),
        # whose grid_sample had no align_corners argument and behaved as align_corners=True
        self.align_corners = True
        self.fused = True   # False: cosine_similarity / exp through torch ops, as the reference writes them
        if half_features not in self.HALF_FEATURES:
            raise ValueError("half_features: one of %s (got %r)" % (self.HALF_FEATURES, half_features))
        self.half_features = half_features
        self.warp_impl = "auto"

    def __call__(self, target, source, flow_list, used_layers, mask=None, use_bilinear_sampling=False):
        if self.vgg is None:
            raise RuntimeError("PerceptualCorrectness needs a feature extractor: pass vgg=... "
                               "(the reference's VGG19 requires torchvision weights)")
        used_layers = sorted(used_layers, reverse=True)
        self.target_vgg, self.source_vgg = self.vgg(target), self.vgg(source)
        total = 0
        for flow, which in zip(flow_list, used_layers):
            total = total + self.calculate_loss(flow, self.layer[which], mask, use_bilinear_sampling)
        return total

    def calculate_loss(self, flow, layer, mask=None, use_bilinear_sampling=False):
        target_feat = self.target_vgg[layer]
        source_feat = self.source_vgg[layer]
        half = _lib.HALF_TYPES
        if target_feat.dtype in half or source_feat.dtype in half or flow.dtype in half:
            # 16-bit features (torch.autocast): the loss is evaluated in float32 on the library's own kernels (max_cosine,
            # resample2d, the fused correctness map) and returned in float32, as autocast returns losses
            with torch.autocast(device_type=target_feat.device.type, enabled=False):
                if self.half_features == "native" and target_feat.dtype in half and \
                        source_feat.dtype == target_feat.dtype and self.fused:
                    return self._loss(flow.float(), target_feat, source_feat, None if mask is None else mask.float(),
                                      use_bilinear_sampling)
                return self._loss(flow.float(), target_feat.float(), source_feat.float(),
                                  None if mask is None else mask.float(), use_bilinear_sampling)
        return self._loss(flow, target_feat, source_feat, mask, use_bilinear_sampling)

    def _loss(self, flow, target_feat, source_feat, mask, use_bilinear_sampling):
        b, c, h, w = target_feat.shape
        flow = F.interpolate(flow, [h, w])

        best = max_cosine_similarity(source_feat, target_feat, self.eps)              # :255-268
        if use_bilinear_sampling:
            warped = self.bilinear_warp(source_feat, flow)
        else:
            # 16-bit features (half_features="native"): the warp itself stays float32, on one up-cast of the source map
            if source_feat.dtype in _lib.HALF_TYPES:
                source_feat = source_feat.float()
            warped = self.resample(source_feat, flow).view(b, c, -1)                  # :273
        if self.fused and warped.dtype == torch.float32:
            loss_map = CorrectnessMapFunction.apply(warped.contiguous(), target_feat.reshape(b, c, -1).contiguous(),
                                                    best, self.eps)                   # :275-276
        else:
            sampled = F.cosine_similarity(warped, target_feat.view(b, c, -1))
            loss_map = torch.exp(-sampled / (best + self.eps))
        floor = torch.exp(torch.tensor(-1.0)).type_as(loss_map)
        if mask is None:
            return torch.mean(loss_map) - floor
        mask = F.interpolate(mask, size=(h, w)).view(-1, h * w)
        return torch.sum(mask * (loss_map - floor)) / (torch.sum(mask) + self.eps)

    def bilinear_warp(self, source, flow):
        """grid_sample alternative of the reference (:308-318), same normalisation of the flow; (b, c, h*w)."""
        b, c, h, w = source.shape
        if self.warp_impl not in WARP_IMPLS:
            raise ValueError("warp_impl: one of %s (got %r)" % (WARP_IMPLS, self.warp_impl))
        if self.warp_impl != "torch" and self.align_corners:
            return flow_warp(source, flow, "correctness", self.warp_impl).view(b, c, -1)
        if source.dtype != flow.dtype:
            source = source.type_as(flow)
        xs = torch.arange(w, device=source.device).view(1, -1).expand(h, -1).type_as(source) / (w - 1)
        ys = torch.arange(h, device=source.device).view(-1, 1).expand(-1, w).type_as(source) / (h - 1)
        grid = 2 * torch.stack([xs, ys], dim=0).unsqueeze(0).expand(b, -1, -1, -1) - 1
        scale = torch.tensor([w, h], device=flow.device).view(1, 2, 1, 1).type_as(flow)
        grid = (grid + 2 * flow / scale).permute(0, 2, 3, 1)
        return F.grid_sample(source, grid, align_corners=self.align_corners).view(b, c, -1)
