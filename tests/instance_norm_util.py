"""Shared by the instance-norm tests: the goldens, the float64 truth, and inputs that stay clear of the activation's kink."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "instance_norm_golden.npz")
CLEAR = 1e-4       # no |z| of the float64 truth is closer to zero than this
EPS = 1e-5
# name -> (affine, negative_slope): None = no activation, 0 = ReLU
CONFIGS = {"affine_leaky": (True, 0.1), "plain_relu": (False, 0.0), "affine_noact": (True, None)}
GOLDEN_SHAPES = {"affine_leaky": (2, 3, 5, 7), "plain_relu": (1, 4, 6, 3), "affine_noact": (2, 2, 4, 9)}


def composition(x, weight, bias, eps, negative_slope):
    """the torch composition the op replaces"""
    y = F.instance_norm(x, None, None, weight, bias, True, 0.0, eps)
    if negative_slope is None:
        return y
    return F.relu(y) if negative_slope == 0 else F.leaky_relu(y, negative_slope)


def pre_activation(x, weight, bias, eps=EPS):
    """z of the float64 truth, on the host"""
    x = x.detach().double().cpu()
    w = None if weight is None else weight.detach().double().cpu()
    b = None if bias is None else bias.detach().double().cpu()
    return F.instance_norm(x, None, None, w, b, True, 0.0, eps)


def near_kink(x, weight, bias, eps=EPS, clear=CLEAR):
    return pre_activation(x, weight, bias, eps).abs() < clear


def spacing(t):
    """spacing of t's dtype at each entry's magnitude (float64 tensor)"""
    mag = t.detach().double().abs().clamp_min(float(torch.finfo(t.dtype).tiny))
    return torch.exp2(torch.floor(torch.log2(mag))) * torch.finfo(t.dtype).eps


def clear_of_kinks(x, weight, bias, eps=EPS, clear=CLEAR):
    """`x` (host, any float dtype) with the entries whose z is within `clear` of zero moved away from it, by a whole
    number of steps of x's own spacing, until none is left (moving an entry shifts the plane's mean and variance a
    little, hence the loop); raises if that does not converge.  The caller checks the result again."""
    x = x.clone()
    for _ in range(100):
        z = pre_activation(x, weight, bias, eps)
        bad = z.abs() < clear
        if not bad.any():
            return x
        xd = x.double()
        var = xd.var(dim=(2, 3), unbiased=False, keepdim=True)
        gain = 1.0 / torch.sqrt(var + eps)
        if weight is not None:
            gain = gain * weight.detach().double().view(1, -1, 1, 1)
        gain = gain.expand_as(xd)
        toward = torch.where(z >= 0, 1.0, -1.0) * torch.where(gain >= 0, 1.0, -1.0)       # direction of x that grows |z|
        ulp = spacing(x)
        steps = torch.ceil(2.5 * clear / gain.abs().clamp_min(1e-30) / ulp).clamp_min(1)
        x = torch.where(bad, (xd + toward * steps * ulp).to(x.dtype), x)
    raise AssertionError("x could not be cleared of kinks")


def truth(x, weight, bias, up, eps, negative_slope):
    """float64 host evaluation of the torch composition on the inputs as given (already rounded to their storage types),
    with autograd: (y, d x, d weight, d bias); the last two are None without parameters"""
    xs = x.detach().double().cpu().requires_grad_()
    w = None if weight is None else weight.detach().double().cpu().requires_grad_()
    b = None if bias is None else bias.detach().double().cpu().requires_grad_()
    y = composition(xs, w, b, eps, negative_slope)
    (y * up.detach().double().cpu()).sum().backward()
    return y.detach(), xs.grad, None if w is None else w.grad, None if b is None else b.grad


def ulp(dtype, at):
    """spacing of `dtype` at magnitude `at`"""
    if at == 0:
        return 0.0
    return math.ldexp(torch.finfo(dtype).eps, math.frexp(at)[1] - 1)


def make_case(shape, dtype, config, seed, offset=0.0, param_dtype=None):
    """(x, weight, bias, up, negative_slope) on the host in their storage types, x clear of the kink"""
    affine, slope = CONFIGS[config]
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = (offset + torch.randn(B, C, H, W, generator=g, dtype=torch.float64)).to(dtype)
    up = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).to(dtype)
    pdt = dtype if param_dtype is None else param_dtype
    weight = bias = None
    if affine:
        weight = (1.0 + 0.5 * torch.randn(C, generator=g, dtype=torch.float64)).to(pdt)
        bias = (0.3 * torch.randn(C, generator=g, dtype=torch.float64)).to(pdt)
    if slope is not None:
        x = clear_of_kinks(x, weight, bias)
    return x, weight, bias, up, slope


def golden(config, dtype=torch.float64, device="cpu"):
    g = np.load(GOLDEN_PATH)
    out = {}
    for k in ("x", "weight", "bias", "up", "y", "g_x", "g_weight", "g_bias"):
        key = "%s/%s" % (config, k)
        out[k] = torch.from_numpy(g[key]).to(dtype).to(device) if key in g.files else None
    return out


# the GPU sweep's shapes: the smallest that reach each code path (tests/test_instance_norm_gpu.py says which)
SWEEP_SHAPES = [(2, 3, 1, 2), (2, 5, 3, 7), (3, 70, 8, 6), (2, 3, 33, 19), (1, 4, 64, 44), (2, 130, 16, 11), (1, 2, 256, 176)]
# the largest register-resident plane with enough planes to stay in regime 1 (f32 and bf16, affine + LeakyReLU only)
FULL_PLANE_SHAPE = (1, 256, 256, 176)


def geometry(B, C, H, W, elem_size, backward=False):
    """gfla_instance_norm_geometry as a dict (host only)"""
    import ctypes
    from global_flow_local_attention_amd import _lib
    out = (ctypes.c_int64 * 7)()
    rc = _lib.lib().gfla_instance_norm_geometry(B, C, H, W, elem_size, int(backward), ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0, (B, C, H, W, elem_size, rc)
    keys = ("regime", "threads", "planes_per_wg", "wgs_per_plane", "values_per_thread", "lds", "workgroups")
    return dict(zip(keys, list(out)))


def smallest_split_shape(elem_size, width=64):
    """(1, 2, H, width) with the smallest H that the library itself puts into regime 2 for two planes"""
    for H in range(1, 4097):
        if geometry(1, 2, H, width, elem_size)["regime"] == 2:
            return (1, 2, H, width)
    raise AssertionError("no split plane up to 4096 x %d" % width)


def sweep_seed(shape):
    return shape[1] * 100 + shape[3]


# every other make_case call of tests/test_instance_norm_gpu.py: (shape or "split", dtype, config, seed, offset, param dtype)
OTHER_GPU_CASES = (
    [(s, d, "affine_leaky", 17, 0.0, None) for s in ((2, 3, 1030, 1), (1, 3, 37, 29)) for d in (torch.float32, torch.bfloat16)]
    + [(FULL_PLANE_SHAPE, d, "affine_leaky", 9, 0.0, None) for d in (torch.float32, torch.bfloat16)]
    + [(s, d, "affine_leaky", 3, o, None) for s in ((2, 4, 64, 44), "split") for d, o in ((torch.float32, 1000.0), (torch.float16, 100.0))]
    + [(s, d, "affine_leaky", 5, 0.0, None) for s in ((3, 70, 8, 6), (2, 6, 64, 44), "split") for d in (torch.float32, torch.bfloat16)]
    + [((2, 6, 33, 19), d, "affine_leaky", 8, 0.0, None) for d in (torch.float32, torch.bfloat16)]
    + [((2, 5, 33, 19), d, "affine_leaky", 12, 0.0, torch.float32) for d in (torch.float16, torch.bfloat16)]
    + [((4, 64, 64, 44), d, "affine_leaky", 13, 0.0, torch.float32) for d in (torch.float32, torch.bfloat16)]
    + [((2, 4, 16, 11), torch.float32, "affine_leaky", 15, 0.0, None)])
