"""Shared by the head-convolution tests: the hand-written torch composition, its float64 host truth with the derived
summation bounds, the sweep's cases and the goldens."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "head_conv_golden.npz")

# name -> (shape (B,Cin,H,W), Cout, post per channel, split, padding, pre_slope): what the goldens record
GOLDENS = {
    "output": ((2, 3, 3, 5), 3, ("tanh",) * 3, None, "reflect", 0.1),
    "pose_heads": ((2, 3, 3, 5), 3, (None, None, "sigmoid"), 2, "zeros", None),
    "face_heads": ((2, 20, 9, 13), 6, (None,) * 4 + ("sigmoid",) * 2, 4, "zeros", None),
}

# the GPU sweep: (shape, Cout, post, split); every one runs for each dtype, padding mode (where legal) and pre_slope
SWEEP = [
    ((1, 1, 2, 2), 1, None, None),                                   # smallest reflect case: both ring rows fold
    ((1, 2, 1, 5), 2, None, None),                                   # H = 1, zeros only
    ((2, 3, 3, 5), 3, "tanh", None),                                 # the golden
    ((1, 5, 2, 7), 2, None, None),                                   # H = 2 with W odd
    ((2, 20, 9, 13), 6, (None,) * 4 + ("sigmoid",) * 2, 4),          # the face heads; Cin no multiple of any chunk
    ((3, 16, 16, 11), 8, None, None),                                # maximum Cout; batch > 1 through the dW reduction
    ((1, 4, 70, 45), 3, None, None),                                 # several pixel tiles per plane
    ((1, 70, 8, 6), 1, None, None),                                  # many channel chunks, one pixel tile
]
OUTPUT_PLANE = ((1, 64, 64, 44), 3, "tanh", None)                    # one real Output plane: reflect, slope 0.1 only


def posts_of(post, cout):
    return (post,) * cout if post is None or isinstance(post, str) else tuple(post)


def composition(x, weight, bias, padding, pre_slope, post, split):
    """the torch ops the head replaces, written out; returns a tuple of one or two tensors"""
    a = x if pre_slope is None else F.leaky_relu(x, pre_slope)
    if padding == "reflect":
        s = F.conv2d(F.pad(a, (1, 1, 1, 1), mode="reflect"), weight, bias)
    else:
        s = F.conv2d(a, weight, bias, padding=1)
    posts = posts_of(post, weight.size(0))
    cols = []
    for c, p in enumerate(posts):
        col = s[:, c:c + 1]
        cols.append(col if p is None else torch.tanh(col) if p == "tanh" else torch.sigmoid(col))
    y = torch.cat(cols, 1)
    return (y,) if split is None else (y[:, :split], y[:, split:])


def ulp(dtype, at):
    if at == 0:
        return 0.0
    return math.ldexp(torch.finfo(dtype).eps, math.frexp(at)[1] - 1)


def unit_roundoff(dtype):
    return torch.finfo(dtype).eps / 2


def make_case(shape, cout, dtype, seed, zeros_in_x=False, bias=True, param_dtype=None):
    """(x, weight, bias, upstream for all Cout channels) on the host, every tensor stored in `dtype` (the parameters in
    `param_dtype` when given); weights scaled so that the sums are O(1).  Both routes and the truth read these very
    values, and a parameter's gradient comes back in the parameter's type."""
    B, Cin, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64).to(dtype)
    if zeros_in_x:
        x[torch.rand(x.shape, generator=g) < 0.25] = 0
    w = (torch.randn(cout, Cin, 3, 3, generator=g, dtype=torch.float64) * (1.5 / math.sqrt(9 * Cin))).to(param_dtype or dtype)
    b = (0.3 * torch.randn(cout, generator=g, dtype=torch.float64)).to(param_dtype or dtype) if bias else None
    up = torch.randn(B, cout, H, W, generator=g, dtype=torch.float64).to(dtype)
    return x, w, b, up


def truth(x, w, b, up, padding, pre_slope, post, split, up_mask=None):
    """float64 host evaluation of the composition on the inputs as given, with autograd, and the derived bound of every
    result.  up_mask: None, or a 0/1 per output tensor (0: that output is not used by the loss).
    Returns {"y": [..], "gx", "gw", "gb"} and the same keys under "S" for the sums of absolute values."""
    xs = x.detach().double().cpu().requires_grad_()
    ws = w.detach().double().cpu().requires_grad_()
    bs = None if b is None else b.detach().double().cpu().requires_grad_()
    ups = up.detach().double().cpu()
    cout = ws.size(0)
    ys = composition(xs, ws, bs, padding, pre_slope, post, split)
    parts = (ups,) if split is None else (ups[:, :split], ups[:, split:])
    use = (1,) * len(ys) if up_mask is None else up_mask
    loss = sum((y * u).sum() for y, u, m in zip(ys, parts, use) if m)
    loss.backward()
    out = {"y": [y.detach() for y in ys], "gx": xs.grad, "gw": ws.grad, "gb": None if bs is None else bs.grad}
    # sums of absolute values: the same linear maps with |.| operands
    with torch.no_grad():
        a = xs if pre_slope is None else F.leaky_relu(xs, pre_slope)
        pad = (lambda t: F.pad(t, (1, 1, 1, 1), mode="reflect")) if padding == "reflect" else (lambda t: F.pad(t, (1, 1, 1, 1)))
        s_fwd = F.conv2d(pad(a.abs()), ws.abs(), None if bs is None else bs.abs())
        y_all = torch.cat(out["y"], 1)
        gate = torch.ones_like(y_all)
        for c, p in enumerate(posts_of(post, cout)):
            if p == "tanh":
                gate[:, c] = 1 - y_all[:, c] ** 2
            elif p == "sigmoid":
                gate[:, c] = y_all[:, c] * (1 - y_all[:, c])
        used = torch.cat([torch.full_like(y, float(m)) for y, m in zip(out["y"], use)], 1)
        gp = (ups * gate * used).abs()
    a0 = torch.zeros_like(xs).requires_grad_()
    (F.conv2d(pad(a0), ws.detach().abs()) * gp).sum().backward()
    slope_factor = torch.ones_like(xs) if pre_slope is None else torch.where(xs.detach() > 0, 1.0, float(pre_slope))
    w0 = torch.zeros_like(ws).requires_grad_()
    (F.conv2d(pad(a.abs()), w0) * gp).sum().backward()
    out["S"] = {"y": [s_fwd] if split is None else [s_fwd[:, :split], s_fwd[:, split:]],
                "gx": a0.grad * slope_factor.abs(), "gw": w0.grad, "gb": gp.sum(dim=(0, 2, 3))}
    return out


def summation_bound(n, S, t, dtype):
    """2 (n + 2) 2^-24 S + u_T |t|, the largest value over the tensor is NOT taken: elementwise"""
    return 2.0 * (n + 2) * 2.0 ** -24 * S + unit_roundoff(dtype) * t.abs()


def term_counts(shape, cout):
    B, Cin, H, W = shape
    return {"y": 9 * Cin, "gx": 36 * cout, "gw": B * H * W, "gb": B * H * W}


def golden(name):
    g = np.load(GOLDEN_PATH)
    return {k.split("/", 1)[1]: torch.from_numpy(g[k]) for k in g.files if k.startswith(name + "/")}


def geometry(B, Cin, Cout, H, W, backward=False):
    """gfla_head_conv3x3_geometry as a dict (host only)"""
    import ctypes
    from global_flow_local_attention_amd import _lib
    out = (ctypes.c_int64 * 7)()
    rc = _lib.lib().gfla_head_conv3x3_geometry(B, Cin, Cout, H, W, int(backward), ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0, (B, Cin, Cout, H, W, rc)
    return dict(zip(("tile_w", "tile_h", "threads", "tiles_per_plane", "slab_rows", "slabs", "channel_groups"), list(out)))
