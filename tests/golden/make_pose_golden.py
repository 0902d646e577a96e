#!/usr/bin/env python3
"""Golden vectors for pose_maps / pose_cords, produced by the REFERENCE's own util/pose_utils.py: cords_to_map and
map_to_cord run unchanged on the host (skimage and matplotlib, which that module imports for its drawing functions, are
stubbed).  Stored: key points, sizes, affine matrices, sigma and the float32 maps of small cases; float32 maps and the key
points map_to_cord finds in them.  Asserted here and not stored: the stored maps hold float32 denormals; every transformed
coordinate of the affine cases is at least 1e-6 from an integer; at the real sizes (256 x 176 with every column as a key
point's x, 128 x 64) the host composition is within 1 ulp of the reference for every element.  Needs a checkout of the
reference:
    python tests/golden/make_pose_golden.py REFERENCE_ROOT
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import pose_util as pu  # noqa: E402
import global_flow_local_attention_amd as gfla  # noqa: E402

if len(sys.argv) != 2:
    sys.exit(__doc__)
ref = pu.reference_pose_utils(sys.argv[1])
rng = np.random.RandomState(20261020)
MAX_BYTES = 512 * 1024


def random_cords(B, J, H0, W0, missing=True, outside=True):
    """integer key points in the old frame; joints 1-3 of every sample missing (y, x, both), joints 4-7 of sample 0 off
    the four sides"""
    c = np.stack([rng.randint(0, H0, size=(B, J)), rng.randint(0, W0, size=(B, J))], axis=2).astype(np.int64)
    if missing and J >= 4:
        c[:, 1, 0] = -1
        c[:, 2, 1] = -1
        c[:, 3] = -1
    if outside and J >= 8:
        c[0, 4] = (-3 - H0 // 4, W0 // 2)
        c[0, 5] = (H0 + 2 + H0 // 4, W0 // 3)
        c[0, 6] = (H0 // 2, -2 - W0 // 4)
        c[0, 7] = (H0 // 3, W0 + 1 + W0 // 4)
    return c


def forward_affine(angle, scale, shift, centre):
    """[x, y, 1] -> the position after a rotation by `angle` degrees and a scaling about `centre`, then a shift"""
    co, si = scale * math.cos(math.radians(angle)), scale * math.sin(math.radians(angle))
    cx, cy = centre
    return np.array([[co, -si, cx - co * cx + si * cy + shift[0]], [si, co, cy - si * cx - co * cy + shift[1]], [0.0, 0.0, 1.0]])


def transformed(cords, size, old_size, affine):
    """(r0, r1) per joint, as the reference forms them, for the distance-from-an-integer check"""
    out = []
    for b in range(cords.shape[0]):
        for y, x in cords[b].astype(float):
            if y == -1 or x == -1:
                continue
            p0, p1 = y / old_size[0] * size[0], x / old_size[1] * size[1]
            r = np.dot(affine[b], np.array([p1, p0, 1.0]))
            out += [float(r[0]), float(r[1])]
    return np.array(out)


def nudged(cords, size, old_size, affine):
    """shift the translation of every matrix in steps of 1e-3 until no transformed coordinate is within 1e-6 of an integer,
    so that the summation order of np.dot cannot matter"""
    affine = affine.copy()
    for _ in range(1000):
        r = transformed(cords, size, old_size, affine)
        if np.abs(r - np.round(r)).min() >= 1e-6:
            return affine
        affine[:, 0:2, 2] += 1e-3
    raise AssertionError("no nudge found")


store, map_cases, cord_cases = {}, [], []


def add_maps(name, cords, size, old_size=None, affine=None, sigma=6):
    old_size = size if old_size is None else old_size
    maps = pu.reference_maps(ref, cords, size, old_size, affine, sigma)
    mine = gfla.torch_pose_maps(torch.from_numpy(cords), size, old_size, None if affine is None else torch.from_numpy(affine),
                                sigma)
    assert pu.ulp_distance(mine, torch.from_numpy(maps)) <= 1, name
    store.update({"cords_" + name: cords, "size_" + name: np.array(size), "old_" + name: np.array(old_size),
                  "sigma_" + name: np.float64(sigma), "maps_" + name: maps})
    if affine is not None:
        store["affine_" + name] = affine
    map_cases.append(name)
    return maps


def add_cords(name, maps, threshold):
    store.update({"cm_" + name: maps, "ct_" + name: np.float64(threshold), "cc_" + name: pu.reference_cords(ref, maps, threshold)})
    cord_cases.append(name)


# ---- small cases, stored whole -------------------------------------------------------------------------------------------
tiny = add_maps("tiny", random_cords(3, 18, 7, 5), (7, 5), sigma=1.5)
odd = add_maps("odd", random_cords(1, 18, 33, 19), (33, 19), sigma=1.5)
add_maps("one", np.array([[[0, 0]]], dtype=np.int64), (1, 1), sigma=0.5)
add_maps("narrow", random_cords(1, 1, 33, 19), (33, 19), sigma=0.5)
add_maps("sigma6", random_cords(1, 1, 33, 19), (33, 19), sigma=6)
add_maps("wide", random_cords(1, 1, 33, 19), (33, 19), sigma=40)
# floating key points, as a loader that augments them itself would hand over
floating = random_cords(1, 18, 7, 5).astype(np.float64)
floating += np.where((rng.rand(1, 18, 2) < 0.5) & (floating != -1), 0.25, 0.0)
add_maps("floating", floating, (7, 5), sigma=1.5)
scaled_cords = random_cords(1, 18, 256, 176)
scaled_cords[0, 8:12, 1] = (15, 30, 60, 120)                # 176 -> 22: 15 lands one pixel to the left; 176 -> 44: 60 and 120
scaled = add_maps("scaled", scaled_cords, (32, 22), (256, 176), sigma=6)
aff_cords = random_cords(3, 2, 256, 176, missing=False, outside=False)
aff_cords[0, 0] = (40, 20)
aff = np.stack([np.array([[1.0, 0.0, -5.5], [0.0, 1.0, 3.25], [0.0, 0.0, 1.0]]),      # joint (40, 20): column in (-1, 0)
                forward_affine(11.0, 1.08, (3.3, -2.1), (22.5, 32.5)),
                forward_affine(-7.0, 0.93, (-40.2, 70.4), (22.5, 32.5))])               # off the image
aff = nudged(aff_cords, (64, 44), (256, 176), aff)
r = transformed(aff_cords, (64, 44), (256, 176), aff)
assert np.abs(r - np.round(r)).min() >= 1e-6 and -1 < r[0] < 0, r[:2]
add_maps("affine", aff_cords, (64, 44), (256, 176), aff, sigma=6)
add_maps("affine23", aff_cords[:, :1], (64, 44), (256, 176), np.ascontiguousarray(aff[:, :2]), sigma=6)
assert np.array_equal(store["maps_affine23"], store["maps_affine"][:, :1])

stored = np.concatenate([store["maps_" + n].ravel() for n in map_cases])
n_denormal = int(pu.denormals(torch.from_numpy(stored)).sum())
assert n_denormal > 100, n_denormal

# ---- map_to_cord -----------------------------------------------------------------------------------------------------------
add_cords("tiny", tiny, 0.1)
add_cords("odd", odd, 0.1)
add_cords("scaled", scaled, 0.1)
above = np.nextafter(np.float32(0.1), np.float32(1))
crafted = np.zeros((1, 18, 7, 5), dtype=np.float32)
crafted[0, 0, 2, 3] = crafted[0, 0, 4, 1] = 0.5             # a tie: the first in row-major order
crafted[0, 1, 6, 4] = crafted[0, 1, 0, 0] = 0.25            # a tie of the first and the last element
crafted[0, 2, 3, 2] = np.float32(0.1)                       # equal to the threshold as float32 (above it as float64): no peak
crafted[0, 3, 3, 2] = above                                 # the next float32: a peak
crafted[0, 4] = 0.75
crafted[0, 4, 5, 1] = np.nan                                # a NaN plane
crafted[0, 5] = np.nan
crafted[0, 6] = 0.5                                         # every element the maximum
crafted[0, 7, 1, 1], crafted[0, 7, 1, 2] = 0.5, np.inf
crafted[0, 8] = -0.0
add_cords("crafted", crafted, 0.1)
signed = np.full((1, 18, 7, 5), -3.0, dtype=np.float32)
signed[0, 0] = -0.0
signed[0, 0, 4, 2] = 0.0                                    # -0 == +0: the first element is the first maximum
signed[0, 1] = 0.0
signed[0, 1, 0, 0] = -2.0
signed[0, 1, 0, 1] = -0.0                                   # the first zero is a negative one
signed[0, 2, 6, 4] = -1.0                                   # equal to the threshold
signed[0, 3, 6, 4] = -0.5
signed[0, 4] = -np.inf
add_cords("signed", signed, -1.0)
assert store["cc_crafted"][0, :9].tolist() == [[2, 3], [0, 0], [-1, -1], [3, 2], [-1, -1], [-1, -1], [0, 0], [1, 2], [-1, -1]]
assert store["cc_signed"][0, :5].tolist() == [[0, 0], [0, 1], [-1, -1], [6, 4], [-1, -1]], store["cc_signed"][0, :5]
for name in cord_cases:
    got = gfla.torch_pose_cords(torch.from_numpy(store["cm_" + name]), float(store["ct_" + name]))
    assert np.array_equal(got.numpy(), store["cc_" + name]), name

# ---- the real sizes: asserted, not stored ----------------------------------------------------------------------------------
real = pu.real_cords().numpy()
assert set(real[..., 1].ravel().tolist()) == set(range(176))
for cords, size, old_size in ((real, (256, 176), (256, 176)), (real[:2], (128, 64), (256, 176))):
    want = torch.from_numpy(pu.reference_maps(ref, cords, size, old_size, None, 6))
    mine = gfla.torch_pose_maps(torch.from_numpy(cords), size, old_size, None, 6)
    d = pu.ulp_distance(mine, want)
    print("%s from %s: composition within %d ulp of the reference, %d of %d elements differ, %d denormals"
          % (size, old_size, d, int((mine != want).sum()), want.numel(), int(pu.denormals(want).sum())))
    assert d <= 1, d

store["map_cases"], store["cord_cases"] = np.array(map_cases), np.array(cord_cases)
np.savez_compressed(pu.GOLDEN, **store)
size = os.path.getsize(pu.GOLDEN)
print("%s: %d bytes, %d map cases, %d cord cases, %d denormals stored" % (pu.GOLDEN, size, len(map_cases), len(cord_cases), n_denormal))
assert size <= MAX_BYTES, size
