#!/usr/bin/env python3
"""Golden vectors for affine_images / resize_images / augmentation_matrices, produced by PILLOW itself: seeded random uint8
images through Image.transform(size, AFFINE, matrix, NEAREST, fillcolor) and Image.resize(size, BILINEAR | BICUBIC).
Stored per affine case: the image, (angle, tx, ty, scale), the fill, the inverse and forward matrices and Pillow's bytes;
per resize case: the image, the size, the filter and Pillow's bytes; the Pillow version.  The matrices come from
image_inputs.augmentation_matrices and are compared bit for bit with the reference's get_inverse_affine_matrix /
get_affine_matrix when a checkout is given.  Asserted here and not stored: the torch compositions equal every stored byte,
and equal Pillow at 256 x 176 and at 1101 x 750 -> 256 x 176; at least one angle-0 case differs between the two branches.
    python tests/golden/make_image_golden.py [REFERENCE_ROOT]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import PIL  # noqa: E402
import image_util as iu  # noqa: E402
from global_flow_local_attention_amd import image_inputs as ii  # noqa: E402

ref = iu.reference_base_dataset(sys.argv[1]) if len(sys.argv) == 2 else None
rng = np.random.RandomState(20261021)
MAX_BYTES = 200 * 1024
store, affine_cases, resize_cases = {"pillow_version": np.array(PIL.__version__)}, [], []


def add_affine(name, size, C, angle, shift, scale, fill):
    H, W = size
    image = rng.randint(0, 256, (H, W, C)).astype(np.uint8)
    inverse, forward = ii.augmentation_matrices([angle], [shift], [scale], size)
    inverse, forward = inverse[0].numpy(), forward[0].numpy()
    if ref is not None:
        want_inverse, want_forward = iu.reference_matrices(ref, angle, shift, scale, size)
        assert np.array_equal(inverse.view(np.int64), want_inverse.view(np.int64)), name
        assert np.array_equal(forward.view(np.int64), want_forward.view(np.int64)), name
    fills = (fill,) * C
    out = iu.pil_affine(image, inverse, fills)
    mine, bad = ii.torch_affine_bytes(torch.from_numpy(image)[None], torch.from_numpy(inverse)[None], fills)
    assert not bad.any() and np.array_equal(mine[0].numpy(), out), name
    store.update({"ai_" + name: image, "ap_" + name: np.array([angle, shift[0], shift[1], scale], dtype=np.float64),
                  "af_" + name: np.array(fills), "am_" + name: inverse, "aw_" + name: forward, "ao_" + name: out})
    affine_cases.append(name)
    other, _ = ii.torch_affine_bytes(torch.from_numpy(image)[None], torch.from_numpy(inverse)[None], fills, scale_branch=False)
    return int((other[0].numpy() != out).sum()), float((out == fill).all(2).mean())


def add_resize(name, shape, size, interpolation):
    image = rng.randint(0, 256, shape).astype(np.uint8)
    out = iu.pil_resize(image, size, interpolation)
    assert np.array_equal(ii.torch_resize_images(torch.from_numpy(image)[None], size, interpolation)[0].numpy(), out), name
    store.update({"ri_" + name: image, "rs_" + name: np.array(size), "rf_" + name: np.array(interpolation), "ro_" + name: out})
    resize_cases.append(name)


# ---- affine: rotations, angle 0 with fractional and whole shifts and scale != 1, the identity, out of frame ---------------
add_affine("rot_7x5_c3", (7, 5), 3, 17.0, (0.4, -0.7), 1.0, 128)
add_affine("rot_33x17_c1", (33, 17), 1, -25.0, (1.5, 2.25), 1.1, 255)
add_affine("rot_33x17_c4", (33, 17), 4, 8.5, (-2.0, 1.0), 0.9, 0)
add_affine("rot_64x40_c3", (64, 40), 3, 12.3, (3.3, -2.1), 0.93, 128)
add_affine("rot90_33x17_c3", (33, 17), 3, 90.0, (0.0, 0.0), 1.0, 255)
add_affine("rot180_7x5_c1", (7, 5), 1, 180.0, (0.0, 0.0), 1.0, 0)
differing = {}
for name, size, C, shift, scale, fill in (("shift_frac_33x17_c3", (33, 17), 3, (2.5, -1.25), 1.0, 128),
                                          ("shift_whole_33x17_c3", (33, 17), 3, (3.0, -2.0), 1.0, 255),
                                          ("scale_64x40_c3", (64, 40), 3, (1.0, -2.0), 1.0 / 1.1, 0),
                                          ("scale_64x40_c1", (64, 40), 1, (-3.21, 4.6), 0.77, 255),
                                          ("scale_7x5_c4", (7, 5), 4, (0.0, 0.0), 1.25, 128),
                                          ("scale_33x17_c1", (33, 17), 1, (0.5, 0.5), 0.7, 0),
                                          ("identity_33x17_c3", (33, 17), 3, (0.0, 0.0), 1.0, 128),
                                          ("identity_7x5_c4", (7, 5), 4, (0.0, 0.0), 1.0, 0)):
    differing[name], _ = add_affine(name, size, C, 0.0, shift, scale, fill)
print("angle 0: bytes at which the fixed-point branch would differ from Pillow:", differing)
assert max(differing.values()) > 0
_, gone = add_affine("outside_33x17_c3", (33, 17), 3, 0.0, (100.0, -80.0), 1.0, 128)
assert gone == 1.0
_, gone = add_affine("outside_rot_7x5_c1", (7, 5), 1, 10.0, (200.0, 200.0), 1.0, 255)
assert gone == 1.0

# ---- resize: both directions, one axis alone, the identity, both filters ---------------------------------------------------
for interpolation in ("bilinear", "bicubic"):
    add_resize("down_%s" % interpolation, (37, 53, 3), (16, 16), interpolation)
    add_resize("up_%s" % interpolation, (16, 16, 3), (37, 53), interpolation)
    add_resize("width_%s" % interpolation, (20, 32, 3), (20, 13), interpolation)
    add_resize("height_%s" % interpolation, (20, 32, 1), (31, 32), interpolation)
    add_resize("same_%s" % interpolation, (9, 9, 3), (9, 9), interpolation)

# ---- the real sizes: asserted, not stored ----------------------------------------------------------------------------------
pixels = 0
for trial in range(12):
    C = (3, 1, 4)[trial % 3]
    angle = 0.0 if trial % 4 == 0 else float(rng.uniform(-30, 30))
    shift, scale = (float(rng.uniform(-20, 20)), float(rng.uniform(-20, 20))), float(rng.uniform(0.8, 1.3))
    image = rng.randint(0, 256, (256, 176, C)).astype(np.uint8)
    inverse = ii.augmentation_matrices([angle], [shift], [scale], (256, 176))[0]
    fills = ((128, 255, 0)[trial % 3],) * C
    mine, _ = ii.torch_affine_bytes(torch.from_numpy(image)[None], inverse, fills)
    assert np.array_equal(mine[0].numpy(), iu.pil_affine(image, inverse[0].numpy(), fills)), trial
    pixels += 256 * 176
big = rng.randint(0, 256, (1101, 750, 3)).astype(np.uint8)
for interpolation in ("bilinear", "bicubic"):
    mine = ii.torch_resize_images(torch.from_numpy(big)[None], (256, 176), interpolation)
    assert np.array_equal(mine[0].numpy(), iu.pil_resize(big, (256, 176), interpolation)), interpolation
print("256 x 176: %d pixels of 12 warps equal Pillow's; 1101 x 750 -> 256 x 176 equals Pillow's with both filters" % pixels)

store["affine_cases"], store["resize_cases"] = np.array(affine_cases), np.array(resize_cases)
np.savez_compressed(iu.GOLDEN, **store)
size = os.path.getsize(iu.GOLDEN)
print("%s: %d bytes, %d affine cases, %d resize cases, Pillow %s, reference %s"
      % (iu.GOLDEN, size, len(affine_cases), len(resize_cases), PIL.__version__, "compared" if ref else "not given"))
assert size <= MAX_BYTES, size
