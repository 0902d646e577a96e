"""Helpers of tests/test_image_inputs_cpu.py, tests/test_image_inputs_gpu.py and tests/golden/make_image_golden.py.

The goldens (tests/golden/image_golden.npz) are outputs of Pillow's own Image.transform(AFFINE, NEAREST) and Image.resize
on seeded random uint8 images, with the matrices they were made with.  Every bar is 0: a byte equals Pillow's byte, a
float equals normalize_images' float of Pillow's byte, bit for bit."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_golden.npz")
REFERENCE = os.environ.get("GFLA_REFERENCE", "/root/reference")
HAVE_REF = os.path.isfile(os.path.join(REFERENCE, "data", "base_dataset.py"))
PIL_MODES = {1: "L", 3: "RGB", 4: "RGBA"}
_golden = []


def golden():
    """the fixture file as a dict, read once"""
    if not _golden:
        with np.load(GOLDEN) as z:
            _golden.append({k: z[k] for k in z.files})
    return _golden[0]


def affine_cases():
    """[(name, image (H, W, C) uint8, (angle, tx, ty, scale), fill (C,) ints, inverse (2, 3), forward (3, 3), Pillow's
    (H, W, C) uint8)] as tensors"""
    g = golden()
    return [(name, torch.from_numpy(g["ai_" + name]), tuple(float(v) for v in g["ap_" + name]),
             tuple(int(v) for v in g["af_" + name]), torch.from_numpy(g["am_" + name]), torch.from_numpy(g["aw_" + name]),
             torch.from_numpy(g["ao_" + name])) for name in [str(n) for n in g["affine_cases"]]]


def resize_cases():
    """[(name, image (h, w, C) uint8, (H, W), filter name, Pillow's (H, W, C) uint8)] as tensors"""
    g = golden()
    return [(name, torch.from_numpy(g["ri_" + name]), tuple(int(s) for s in g["rs_" + name]), str(g["rf_" + name]),
             torch.from_numpy(g["ro_" + name])) for name in [str(n) for n in g["resize_cases"]]]


def pil_image(array):
    from PIL import Image
    array = np.ascontiguousarray(array)
    return Image.fromarray(array[:, :, 0] if array.shape[2] == 1 else array, PIL_MODES[array.shape[2]])


def pil_affine(array, inverse, fill):
    """Image.transform(size, AFFINE, inverse, NEAREST, fillcolor=fill) of an (H, W, C) uint8 array, as (H, W, C)"""
    from PIL import Image
    H, W, C = array.shape
    colour = int(fill[0]) if C == 1 else tuple(int(f) for f in fill)
    out = pil_image(array).transform((W, H), Image.AFFINE, [float(v) for v in np.asarray(inverse).reshape(-1)], Image.NEAREST,
                                     fillcolor=colour)
    return np.asarray(out).reshape(H, W, C)


def pil_resize(array, size, interpolation):
    """Image.resize((W, H), BILINEAR | BICUBIC) of an (h, w, C) uint8 array, C 1 or 3, as (H, W, C)"""
    from PIL import Image
    assert array.shape[2] in (1, 3)              # LA and RGBA go through premultiplied alpha: not the 8-bit filter alone
    out = pil_image(array).resize((size[1], size[0]), {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[interpolation])
    return np.asarray(out).reshape(size[0], size[1], array.shape[2])


def reference_base_dataset(root=REFERENCE):
    """the reference's data/base_dataset module, with the libraries it imports at the top and get_inverse_affine_matrix /
    get_affine_matrix never use stubbed for the time of the import"""
    names = ("torchvision", "torchvision.transforms", "torchvision.transforms.functional", "pandas", "util", "util.pose_utils",
             "PIL", "PIL.Image")
    saved = {}                                           # what stood in sys.modules where a stub goes, put back afterwards
    try:
        for n in names:
            try:
                if n.startswith("util"):
                    raise ImportError(n)                 # the reference's package, never the tests' util.py
                importlib.import_module(n)
            except ImportError:
                saved[n] = sys.modules.get(n)
                sys.modules[n] = types.ModuleType(n)
        for parent, child in (("torchvision", "transforms"), ("torchvision.transforms", "functional"), ("util", "pose_utils"),
                              ("PIL", "Image")):
            if not hasattr(sys.modules[parent], child):
                setattr(sys.modules[parent], child, sys.modules[parent + "." + child])
        spec = importlib.util.spec_from_file_location("reference_base_dataset", os.path.join(root, "data", "base_dataset.py"))
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return module


def reference_matrices(module, angle, translate, scale, size):
    """(inverse (2, 3), forward (3, 3)) as the reference's dataset forms them for an image of `size` (H, W)"""
    dataset = module.BaseDataset.__new__(module.BaseDataset)
    centre = (size[1] * 0.5 + 0.5, size[0] * 0.5 + 0.5)
    inverse = dataset.get_inverse_affine_matrix(centre, angle, translate, scale, 0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", PendingDeprecationWarning)           # np.matrix
        forward = dataset.get_affine_matrix(center=centre, angle=angle, translate=translate, scale=scale, shear=0)
    return np.array(inverse, dtype=np.float64).reshape(2, 3), np.asarray(forward, dtype=np.float64).reshape(3, 3)
