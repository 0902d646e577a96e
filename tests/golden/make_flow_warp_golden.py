#!/usr/bin/env python3
"""Golden vectors for the bilinear flow warp, produced on the host in float64 by the REFERENCE's own code:
`PerceptualCorrectness.bilinear_warp` (model/networks/external_function.py:309-319) called unbound, and
`BilinearSamplingBlock.forward` (model/networks/base_function.py:490-506), each with the gradients of source and flow
for a fixed upstream gradient.

Three things are patched for the calls, none of them in the reference's files:
  * `F.grid_sample`'s default: the reference targets a torch whose grid_sample had no align_corners argument and behaved
    as align_corners=True (global_flow_local_attention_amd/correctness.py); today's default is False, so the calls run
    with the default set to True;
  * `torch.Tensor.cuda` is the identity while BilinearSamplingBlock.forward runs (base_function.py:500 moves its grid to
    the GPU unconditionally);
  * torchvision is stubbed, as in make_correctness_golden.py.
The reference builds its grid in float32 (`.float()`) whatever the source's dtype.  The cases use sizes with w - 1 and
h - 1 powers of two, for which that grid is exact, so the goldens are float64-accurate.

The "pixel" convention (poseflownet_model.py:86-103) equals "block" on a square map: the case `square` pins it.  Its
model module cannot be imported without the reference's data pipeline, and `visi` resizes the source to the flow's size
before it samples, so a source of another size never reaches its grid_sample; the case `resize` (Hs x Ws != H x W) is
therefore torch's own grid_sample on the grid of the pixel position, written out below -- not reference code.

Every flow is built so that samples leave the map on every side, and is nudged until no sampling position is within
1e-3 px of an integer (d/d flow jumps there).

Needs the reference checkout (GFLA_REFERENCE, as for __graft_entry__.build()):  python tests/golden/make_flow_warp_golden.py
"""
import os, sys, types
import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import global_flow_local_attention_amd as gfla  # noqa: E402
from global_flow_local_attention_amd.flow_warp import convention_scalars  # noqa: E402

sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
sys.modules.setdefault("torchvision.models", types.ModuleType("torchvision.models"))
sys.modules["torchvision"].models = sys.modules["torchvision.models"]
bf = gfla.install(os.environ.get("GFLA_REFERENCE", "/root/reference"), fuse_extractor_attn=False)
import model.networks.external_function as ef  # noqa: E402

CASES = [  # name, B, C, (Hs, Ws), (H, W)
    ("tall", 2, 3, (9, 5), (9, 5)),
    ("wide", 1, 5, (5, 17), (5, 17)),
    ("square", 2, 4, (9, 9), (9, 9)),
    ("resize", 2, 3, (5, 9), (7, 6)),
]
CLEAR = 1e-3


def positions(flow, scalars):
    gx, gy, mx, my = scalars
    h, w = flow.shape[2:]
    xs = torch.arange(w, dtype=flow.dtype).view(1, 1, w)
    ys = torch.arange(h, dtype=flow.dtype).view(1, h, 1)
    return (xs + gx * flow[:, 0]) * mx, (ys + gy * flow[:, 1]) * my


def make_flow(B, hs, ws, h, w, gen, conventions):
    """half the samples near the map, half far away; the four corners of the first map leave on the four sides"""
    flow = torch.randn(B, 2, h, w, generator=gen, dtype=torch.float64) * 1.5
    far = torch.rand(B, 1, h, w, generator=gen) < 0.4
    flow = torch.where(far, flow * max(hs, ws), flow)
    flow[0, 0, 0, 0], flow[0, 1, 0, 0] = -(ws + 2.3), 0.4          # left
    flow[0, 0, 0, -1], flow[0, 1, 0, -1] = ws + 2.3, 0.4           # right
    flow[0, 0, -1, 0], flow[0, 1, -1, 0] = 0.4, -(hs + h + 2.3)    # top
    flow[0, 0, -1, -1], flow[0, 1, -1, -1] = 0.4, hs + 2.3         # bottom
    for _ in range(100):
        bad = torch.zeros_like(flow, dtype=torch.bool)
        for conv in conventions:
            ix, iy = positions(flow, convention_scalars(conv, hs, ws))
            bad[:, 0] |= (ix - ix.round()).abs() < CLEAR
            bad[:, 1] |= (iy - iy.round()).abs() < CLEAR
        if not bad.any():
            return flow
        flow = torch.where(bad, flow + 0.0137, flow)
    raise RuntimeError("could not clear the kinks")


def with_grads(fn, src, flow, up):
    s, f = src.clone().requires_grad_(), flow.clone().requires_grad_()
    out = fn(s, f)
    (out.reshape(up.shape) * up).sum().backward()
    return out.detach().reshape(up.shape), s.grad, f.grad


def main():
    real_grid_sample, real_cuda = F.grid_sample, torch.Tensor.cuda

    def aligned(input, grid, mode="bilinear", padding_mode="zeros", align_corners=True):
        return real_grid_sample(input, grid, mode=mode, padding_mode=padding_mode, align_corners=align_corners)

    out = {}
    F.grid_sample = aligned
    try:
        for i, (name, B, C, (hs, ws), (h, w)) in enumerate(CASES):
            gen = torch.Generator().manual_seed(500 + i)
            same = (hs, ws) == (h, w)
            flow = make_flow(B, hs, ws, h, w, gen, ("correctness", "block", "pixel") if same else ("pixel",))
            src = torch.randn(B, C, hs, ws, generator=gen, dtype=torch.float64)
            up = torch.randn(B, C, h, w, generator=gen, dtype=torch.float64)
            out["%s/src" % name], out["%s/flow" % name], out["%s/up" % name] = src.numpy(), flow.numpy(), up.numpy()
            results = {}
            if same:
                results["correctness"] = with_grads(lambda s, f: ef.PerceptualCorrectness.bilinear_warp(None, s, f),
                                                    src, flow, up)
                torch.Tensor.cuda = lambda self, *a, **k: self
                try:
                    results["block"] = with_grads(bf.BilinearSamplingBlock().forward, src, flow, up)
                finally:
                    torch.Tensor.cuda = real_cuda
                if hs == ws:
                    results["pixel"] = results["block"]
            else:
                def pixel(s, f):
                    ix, iy = positions(f, (1.0, 1.0, 1.0, 1.0))
                    grid = torch.stack([2 * ix / (ws - 1) - 1, 2 * iy / (hs - 1) - 1], dim=-1)
                    return real_grid_sample(s, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
                results["pixel"] = with_grads(pixel, src, flow, up)
            for conv, (o, gs, gf) in results.items():
                out["%s/%s/out" % (name, conv)] = o.numpy()
                out["%s/%s/g_source" % (name, conv)] = gs.numpy()
                out["%s/%s/g_flow" % (name, conv)] = gf.numpy()
                print(name, conv, float(o.abs().sum()), float((o == 0).double().mean()))
    finally:
        F.grid_sample = real_grid_sample
    assert all(v.dtype == np.float64 for v in out.values())
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "flow_warp_golden.npz"), **out)


if __name__ == "__main__":
    main()
