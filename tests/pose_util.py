"""Helpers of tests/test_pose_inputs_cpu.py, tests/test_pose_inputs_gpu.py and tests/golden/make_pose_golden.py.

The goldens (tests/golden/pose_golden.npz) are outputs of the reference's own util/pose_utils.cords_to_map and
map_to_cord.  Bars: the reference rounds exp() of one float64 quotient to float32; the library rounds a product of two
float64 exponentials, which differs from that quotient's exponential by a few float64 ulps, so the two float32 results are
equal or neighbours: 1 ulp, counted on the bit patterns so that denormals count like everything else."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_golden.npz")
REFERENCE = os.environ.get("GFLA_REFERENCE", "/root/reference")
HAVE_REF = os.path.isdir(os.path.join(REFERENCE, "model", "networks"))
# x = (x / 176) * 176 comes back one ulp short at these columns, and truncation puts the centre one pixel to the left
QUIRK_COLUMNS_176 = (15, 30, 49, 60, 98, 109, 120)
FLOAT32_MIN_NORMAL = 1.1754943508222875e-38
_golden = []


def golden():
    """the fixture file as a dict, read once"""
    if not _golden:
        with np.load(GOLDEN) as z:
            _golden.append({k: z[k] for k in z.files})
    return _golden[0]


def map_cases():
    """[(name, cords (B, J, 2), size, old_size, affine or None, sigma, maps (B, J, H, W) float32)] as tensors"""
    g, out = golden(), []
    for name in [str(n) for n in g["map_cases"]]:
        affine = torch.from_numpy(g["affine_" + name]) if "affine_" + name in g else None
        out.append((name, torch.from_numpy(g["cords_" + name]), tuple(int(s) for s in g["size_" + name]),
                    tuple(int(s) for s in g["old_" + name]), affine, float(g["sigma_" + name]),
                    torch.from_numpy(g["maps_" + name])))
    return out


def cord_cases():
    """[(name, maps (B, 18, H, W) float32, threshold, cords (B, 18, 2) int64)] as tensors"""
    g = golden()
    return [(name, torch.from_numpy(g["cm_" + name]), float(g["ct_" + name]), torch.from_numpy(g["cc_" + name]))
            for name in [str(n) for n in g["cord_cases"]]]


def ordered(t):
    """the bit patterns of a float32 / float16 / bfloat16 tensor as integers that sort like the values (-0 and +0 both 0)"""
    wide = t.element_size() == 4
    i = t.contiguous().view(torch.int32 if wide else torch.int16).to(torch.int64)
    return torch.where(i < 0, -(i & (0x7FFFFFFF if wide else 0x7FFF)), i)


def ulp_distance(a, b):
    """largest distance of the bit patterns of a and b, in ulps of their common storage type (so denormals count like
    everything else); NaN against NaN counts 0, NaN against a number 2^32"""
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.dtype == b.dtype and a.dtype.is_floating_point and a.element_size() <= 4 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    na, nb = torch.isnan(a), torch.isnan(b)
    d = (ordered(a) - ordered(b)).abs()
    d = torch.where(na & nb, torch.zeros_like(d), torch.where(na | nb, torch.full_like(d, 2 ** 32), d))
    return int(d.max())


def denormals(t):
    """mask of the float32 denormals of t"""
    return (t != 0) & (t.abs() < FLOAT32_MIN_NORMAL)


def reference_pose_utils(root=REFERENCE):
    """the reference's util/pose_utils module, with the drawing libraries it imports at the top and never uses in
    cords_to_map / map_to_cord stubbed"""
    for name in ("skimage", "skimage.draw", "skimage.measure", "skimage.transform", "matplotlib", "matplotlib.pyplot",
                 "matplotlib.patches"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    draw = sys.modules["skimage.draw"]
    for attr in ("circle", "line_aa", "polygon"):
        if not hasattr(draw, attr):
            setattr(draw, attr, None)
    if not hasattr(sys.modules["matplotlib"], "use"):
        sys.modules["matplotlib"].use = lambda *a, **k: None
    for parent, child in (("skimage", "draw"), ("skimage", "measure"), ("skimage", "transform"), ("matplotlib", "pyplot"),
                          ("matplotlib", "patches")):
        if not hasattr(sys.modules[parent], child):
            setattr(sys.modules[parent], child, sys.modules[parent + "." + child])
    try:
        importlib.import_module("scipy.ndimage.filters")
    except ImportError:
        stub = types.ModuleType("scipy.ndimage.filters")
        stub.gaussian_filter = None
        sys.modules["scipy.ndimage.filters"] = stub
    spec = importlib.util.spec_from_file_location("reference_pose_utils", os.path.join(root, "util", "pose_utils.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def reference_maps(pose_utils, cords, size, old_size, affine, sigma):
    """cords_to_map per sample, as (B, J, H, W) float32"""
    out = []
    for b in range(cords.shape[0]):
        a = None if affine is None else np.array(affine[b], dtype=np.float64)
        m = pose_utils.cords_to_map(np.array(cords[b]), tuple(size), tuple(old_size), a, sigma)
        out.append(np.transpose(m, (2, 0, 1)))
    return np.stack(out).astype(np.float32)


def reference_cords(pose_utils, maps, threshold):
    """map_to_cord per sample of (B, 18, H, W) maps, as (B, 18, 2) int64"""
    return np.stack([np.asarray(pose_utils.map_to_cord(np.transpose(m, (1, 2, 0)), threshold=threshold), dtype=np.int64)
                     for m in maps])


def real_cords(B=10, J=18, H=256, W=176):
    """every column 0 .. W - 1 as a key point's x at least once, rows spread over the image"""
    k = torch.arange(B * J)
    return torch.stack([(k * 37) % H, k % W], dim=1).view(B, J, 2)
