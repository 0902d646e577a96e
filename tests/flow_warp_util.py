"""Shared by the flow-warp tests: the goldens, a float64 emulation of exactly what csrc/flow_warp.hip computes, and the
construction of flows that stay clear of the kinks of d/d flow."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "flow_warp_golden.npz")
CONVENTIONS = ("correctness", "block", "pixel")
CLEAR = 1e-3       # px: every sampling position is at least this far from an integer


def golden_cases():
    """[(case, convention)] present in the golden file"""
    g = np.load(GOLDEN_PATH)
    return sorted({tuple(k.split("/")[:2]) for k in g.files if k.count("/") == 2})


def golden(case, convention, dtype=torch.float64, device="cpu"):
    g = np.load(GOLDEN_PATH)
    out = {k: torch.from_numpy(g["%s/%s" % (case, k)]) for k in ("src", "flow", "up")}
    out.update({k: torch.from_numpy(g["%s/%s/%s" % (case, convention, k)]) for k in ("out", "g_source", "g_flow")})
    return {k: v.to(dtype).to(device) for k, v in out.items()}


def positions(flow, scalars):
    """sampling positions (ix, iy), each (B,H,W), in float64 on the host"""
    gx, gy, mx, my = scalars
    flow = flow.detach().double().cpu()
    h, w = flow.shape[2:]
    xs = torch.arange(w, dtype=torch.float64).view(1, 1, w)
    ys = torch.arange(h, dtype=torch.float64).view(1, h, 1)
    return (xs + gx * flow[:, 0]) * mx, (ys + gy * flow[:, 1]) * my


def near_kink(flow, scalars, clear=CLEAR):
    """bool (B,2,H,W): the entries of `flow` whose sampling coordinate is within `clear` px of an integer -- where d/d flow
    jumps (integers include the map's borders -1, 0, Ws - 1, Ws)"""
    ix, iy = positions(flow, scalars)
    return torch.stack([(ix - ix.round()).abs() < clear, (iy - iy.round()).abs() < clear], dim=1)


def clear_of_kinks(flow, scalar_sets, clear=CLEAR):
    """`flow` (any float dtype, host) with offending entries nudged, in its own dtype, until none is left for any of
    `scalar_sets`; raises if that does not converge.  The result is checked again by the caller."""
    flow = flow.clone()
    for _ in range(200):
        bad = torch.zeros(flow.shape, dtype=torch.bool)
        for scalars in scalar_sets:
            bad |= near_kink(flow, scalars, clear)
        if not bad.any():
            return flow
        flow = torch.where(bad, (flow.double() + 0.0137).to(flow.dtype), flow)
    raise AssertionError("flow could not be cleared of kinks")


def emulate(src, flow, scalars, up):
    """What the kernels compute, in float64 torch ops: pixel-space position, floor and fractions, four corners with zero
    padding through clamped addresses and in-range flags, the forward's weighted sum, the analytic d/d flow
    (gx mx sum_c up ((1-ay)(v01-v00) + ay (v11-v10)), and the same along y) and d/d source (weight x gradient scattered to
    every in-range corner).  Returns (out, g_source, g_flow)."""
    src, flow, up = src.double(), flow.double(), up.double()
    gx, gy, mx, my = scalars
    B, C, Hs, Ws = src.shape
    H, W = flow.shape[2:]
    ix, iy = positions(flow, scalars)
    x0, y0 = ix.floor(), iy.floor()
    ax, ay = (ix - x0).unsqueeze(1), (iy - y0).unsqueeze(1)
    flat = src.reshape(B, C, Hs * Ws)

    def corner(yy, xx):
        inside = ((xx >= 0) & (xx <= Ws - 1) & (yy >= 0) & (yy <= Hs - 1)).unsqueeze(1).double()
        at = (yy.clamp(0, Hs - 1) * Ws + xx.clamp(0, Ws - 1)).long().view(B, 1, H * W).expand(-1, C, -1)
        return torch.gather(flat, 2, at).view(B, C, H, W) * inside, at, inside

    (v00, a00, i00), (v01, a01, i01) = corner(y0, x0), corner(y0, x0 + 1)
    (v10, a10, i10), (v11, a11, i11) = corner(y0 + 1, x0), corner(y0 + 1, x0 + 1)
    w00, w01, w10, w11 = (1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay
    out = w00 * v00 + w01 * v01 + w10 * v10 + w11 * v11
    g_flow = torch.stack([gx * mx * (up * ((1 - ay) * (v01 - v00) + ay * (v11 - v10))).sum(1),
                          gy * my * (up * ((1 - ax) * (v10 - v00) + ax * (v11 - v01))).sum(1)], dim=1)
    g_src = torch.zeros(B, C, Hs * Ws, dtype=torch.float64)
    for w, at, inside in ((w00, a00, i00), (w01, a01, i01), (w10, a10, i10), (w11, a11, i11)):
        g_src.scatter_add_(2, at, (w * up * inside).reshape(B, C, H * W))
    return out, g_src.view(B, C, Hs, Ws), g_flow


def truth(src, flow, scalars, up):
    """float64 host evaluation of the torch composition (grid + grid_sample, align_corners=True) on the inputs as given
    (already rounded to their storage types), with autograd: (out, g_source, g_flow)"""
    from global_flow_local_attention_amd.flow_warp import torch_flow_warp
    s = src.detach().double().cpu().requires_grad_()
    f = flow.detach().double().cpu().requires_grad_()
    out = torch_flow_warp(s, f, *scalars)
    (out * up.detach().double().cpu()).sum().backward()
    return out.detach(), s.grad, f.grad
