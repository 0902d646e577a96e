"""Pose inputs without a GPU (pose_inputs.py, include/gfla_pose.h): the torch compositions against the reference's own
cords_to_map / map_to_cord (tests/golden/pose_golden.npz, tests/golden/make_pose_golden.py), the exact cases, the argument
errors and the ABI.  Bars: tests/pose_util.py."""
import numpy as np
import pytest
import torch

import global_flow_local_attention_amd as gfla
from global_flow_local_attention_amd import _lib, pose_inputs

import pose_util as pu

MAP_CASES = pu.map_cases()
CORD_CASES = pu.cord_cases()


# ---- pose_maps --------------------------------------------------------------------------------------------------------------
def test_the_goldens_cover_what_they_are_there_for():
    by_name = {c[0]: c for c in MAP_CASES}
    assert {c[2] for c in MAP_CASES} >= {(7, 5), (33, 19), (1, 1), (32, 22), (64, 44)}
    assert {c[5] for c in MAP_CASES} >= {0.5, 1.5, 6.0, 40.0}
    assert {c[1].shape[1] for c in MAP_CASES} >= {1, 18} and {c[1].shape[0] for c in MAP_CASES} >= {1, 3}
    assert by_name["scaled"][3] == (256, 176) and by_name["affine"][4].shape == (3, 3, 3) and by_name["affine23"][4].shape == (3, 2, 3)
    cords = by_name["tiny"][1]
    assert (cords[:, 1, 0] == -1).all() and (cords[:, 1, 1] != -1).all() and (cords[:, 2, 1] == -1).all() and (cords[:, 3] == -1).all()
    assert cords[0, 4, 0] < 0 and cords[0, 5, 0] >= 7 and cords[0, 6, 1] < 0 and cords[0, 7, 1] >= 5      # off every side
    assert sum(int(pu.denormals(c[6]).sum()) for c in MAP_CASES) > 100
    assert by_name["floating"][1].dtype == torch.float64 and (by_name["floating"][1] % 1 != 0).any()


@pytest.mark.parametrize("case", MAP_CASES, ids=[c[0] for c in MAP_CASES])
def test_composition_is_within_one_ulp_of_every_golden_map(case):
    name, cords, size, old_size, affine, sigma, want = case
    got = gfla.pose_maps(cords, size, old_size, affine, sigma)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert pu.ulp_distance(got, want) <= 1
    assert torch.equal(pu.denormals(got), pu.denormals(want))
    assert torch.equal(gfla.pose_maps(cords, size, old_size, affine, sigma, impl="torch"), got)
    missing = (cords[..., 0] == -1) | (cords[..., 1] == -1)
    assert not got[missing].any() and (got[~missing].flatten(1).max(1).values >= 0).all()


def test_a_coordinate_between_minus_one_and_zero_truncates_to_zero():
    name, cords, size, old_size, affine, sigma, want = [c for c in MAP_CASES if c[0] == "affine"][0]
    y, x = cords[0, 0].double()
    p0, p1 = (y / old_size[0]) * size[0], (x / old_size[1]) * size[1]
    r0 = affine[0, 0, 0] * p1 + affine[0, 0, 1] * p0 + affine[0, 0, 2]
    assert -1 < r0 < 0
    row = int(affine[0, 1, 0] * p1 + affine[0, 1, 1] * p0 + affine[0, 1, 2])
    assert want[0, 0, row, 0] == 1.0 and gfla.pose_maps(cords, size, old_size, affine, sigma)[0, 0, row, 0] == 1.0


@pytest.mark.skipif(not pu.HAVE_REF, reason="reference checkout not present")
def test_composition_against_the_live_reference_at_256_by_176():
    ref = pu.reference_pose_utils()
    cords = pu.real_cords(B=2)
    want = torch.from_numpy(pu.reference_maps(ref, cords.numpy(), (256, 176), (256, 176), None, 6))
    got = gfla.pose_maps(cords, (256, 176))
    assert pu.ulp_distance(got, want) <= 1
    assert int(pu.denormals(want).sum()) > 10000 and torch.equal(pu.denormals(got), pu.denormals(want))
    peaks = torch.from_numpy(pu.reference_cords(ref, want.numpy(), 0.1))
    assert torch.equal(gfla.pose_cords(got), peaks)


def test_the_seven_quirk_columns_of_width_176_land_one_pixel_to_the_left():
    xs = torch.arange(176)
    cords = torch.stack([torch.full_like(xs, 3), xs], dim=1).view(1, 176, 2)
    maps = gfla.pose_maps(cords, (8, 176))
    peak = gfla.pose_cords(maps)[0]
    assert (peak[:, 0] == 3).all()
    shifted = [int(x) for x in xs if peak[x, 1] != x]
    assert tuple(shifted) == pu.QUIRK_COLUMNS_176 and all(int(peak[x, 1]) == x - 1 for x in shifted)
    # the same key points given in a frame of another width come through another division: 176 -> 44 moves 60 and 120
    small = gfla.pose_cords(gfla.pose_maps(cords, (8, 44), old_size=(8, 176)))[0]
    assert int(small[60, 1]) == 14 and int(small[120, 1]) == 29 and int(small[61, 1]) == 15


def test_sixteen_bit_maps_are_the_float32_maps_rounded_once():
    name, cords, size, old_size, affine, sigma, want = MAP_CASES[0]
    full = gfla.pose_maps(cords, size, old_size, affine, sigma)
    for dtype in _lib.HALF_TYPES:
        assert torch.equal(gfla.pose_maps(cords, size, old_size, affine, sigma, dtype=dtype), full.to(dtype))


def test_non_finite_inputs_poison_their_channels_and_no_other():
    cords = torch.tensor([[[2.0, 1.0], [float("nan"), 1.0], [2.0, float("inf")], [-1.0, float("nan")], [3.0, 3.0]],
                          [[2.0, 1.0], [1.0, 1.0], [2.0, 2.0], [-1.0, 2.0], [3.0, 3.0]]])
    got = gfla.pose_maps(cords, (7, 5))
    nan = got.isnan().flatten(2)
    assert nan.all(2).tolist() == [[False, True, True, False, False], [False] * 5] and nan.any(2).tolist() == nan.all(2).tolist()
    assert not got[:, 3].any()                                      # a missing joint stays missing, as in the reference
    affine = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    affine[1, 2, 0] = float("nan")                                  # any entry of the sample's matrix
    got = gfla.pose_maps(cords, (7, 5), affine=affine)
    nan = got.isnan().flatten(2).all(2)
    assert nan.tolist() == [[False, True, True, False, False], [True, True, True, False, True]]


def test_centres_far_outside_are_clamped_and_the_map_is_zero():
    cords = torch.tensor([[[1e300, 2.0], [3.0, -1e18], [2 ** 40, 2 ** 40]]], dtype=torch.float64)
    assert not gfla.pose_maps(cords, (7, 5)).any()


# ---- pose_cords -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CORD_CASES, ids=[c[0] for c in CORD_CASES])
def test_pose_cords_equals_the_goldens(case):
    name, maps, threshold, want = case
    got = gfla.pose_cords(maps, threshold)
    assert got.dtype == torch.int64 and torch.equal(got, want)


def test_the_crafted_goldens_hold_the_edge_cases():
    by_name = {c[0]: c for c in CORD_CASES}
    maps, threshold, want = by_name["crafted"][1:]
    assert want[0, 0].tolist() == [2, 3] and maps[0, 0, 4, 1] == maps[0, 0, 2, 3]                    # a tie
    assert want[0, 1].tolist() == [0, 0] and maps[0, 1, 6, 4] == maps[0, 1, 0, 0]                    # first and last element
    assert maps[0, 2].max() == np.float32(threshold) and want[0, 2].tolist() == [-1, -1]            # equal to the threshold
    assert float(maps[0, 2].max()) > threshold                     # which a float64 comparison would let through
    assert want[0, 3].tolist() == [3, 2]
    assert maps[0, 4].isnan().sum() == 1 and maps[0, 5].isnan().all() and want[0, 4:6].tolist() == [[-1, -1]] * 2
    maps, threshold, want = by_name["signed"][1:]
    assert torch.signbit(maps[0, 0, 0, 0]) and not torch.signbit(maps[0, 0, 4, 2]) and want[0, 0].tolist() == [0, 0]
    assert torch.signbit(maps[0, 1, 0, 1]) and want[0, 1].tolist() == [0, 1]


def test_pose_cords_on_16_bit_storage_widens_first():
    maps = CORD_CASES[0][1]
    for dtype in _lib.HALF_TYPES:
        stored = maps.to(dtype)
        assert torch.equal(gfla.pose_cords(stored), gfla.pose_cords(stored.float()))


def test_round_trip_gives_the_truncated_key_points():
    cords = torch.tensor([[[3.75, 2.25], [0.0, 0.0], [6.0, 4.0], [-1.0, 2.0]]])
    got = gfla.pose_cords(gfla.pose_maps(cords, (7, 5), sigma=1.5))
    assert got.tolist() == [[[3, 2], [0, 0], [6, 4], [-1, -1]]]


# ---- normalize_images -------------------------------------------------------------------------------------------------------
def test_normalize_images_is_exact_on_all_256_values():
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).expand(2, 16, 16, 3).contiguous()
    got = gfla.normalize_images(u8)
    v = np.arange(256, dtype=np.float32)
    want = ((v / np.float32(255)) - np.float32(0.5)) / np.float32(0.5)            # numpy float32: IEEE operations, one by one
    assert got.shape == (2, 3, 16, 16) and got.dtype == torch.float32
    assert np.array_equal(got[1, 2].reshape(-1).numpy().view(np.int32), want.view(np.int32))
    assert got.min() == -1 and got.max() == 1
    for dtype in _lib.HALF_TYPES:
        assert torch.equal(gfla.normalize_images(u8, dtype=dtype), got.to(dtype))
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    per = gfla.normalize_images(u8, mean, std)
    for c in range(3):
        want = ((v / np.float32(255)) - np.float32(mean[c])) / np.float32(std[c])
        assert np.array_equal(per[0, c].reshape(-1).numpy().view(np.int32), want.view(np.int32))


def test_normalize_images_de_interleaves():
    u8 = torch.arange(2 * 5 * 7 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(2, 5, 7, 3)
    got = gfla.normalize_images(u8)
    assert torch.equal(got, u8.permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5))


# ---- argument errors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs", [dict(sigma=0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
                                    dict(old_size=(0, 5)), dict(old_size=(7, -1)), dict(size=(0, 5)), dict(size=(7, 0)),
                                    dict(cords=torch.zeros(0, 18, 2)), dict(cords=torch.zeros(2, 0, 2)),
                                    dict(cords=torch.zeros(2, 18, 3)), dict(affine=torch.zeros(2, 3, 3, dtype=torch.float64)),
                                    dict(affine=torch.zeros(1, 3, 2, dtype=torch.float64)), dict(impl="hip")],
                         ids=lambda k: "-".join("%s" % key for key in k))
def test_pose_maps_argument_errors_raise_value_error(kwargs):
    args = dict(cords=torch.zeros(1, 18, 2), size=(7, 5))
    args.update(kwargs)
    with pytest.raises(ValueError):
        gfla.pose_maps(**args)


def test_type_errors():
    with pytest.raises(TypeError):
        gfla.pose_maps(torch.zeros(1, 2, 2), (7, 5), dtype=torch.float64)
    with pytest.raises(TypeError):
        gfla.pose_maps(torch.zeros(1, 2, 2), (7, 5), affine=torch.zeros(1, 3, 3))          # float32 matrices
    with pytest.raises(TypeError):
        gfla.pose_cords(torch.zeros(1, 1, 2, 2, dtype=torch.float64))
    with pytest.raises(TypeError):
        gfla.normalize_images(torch.zeros(1, 2, 2, 3))
    with pytest.raises(ValueError):
        gfla.pose_cords(torch.zeros(1, 1, 2, 2), threshold=float("nan"))
    with pytest.raises(ValueError):
        gfla.pose_cords(torch.zeros(1, 1, 0, 2))
    for bad in (dict(std=0.0), dict(mean=float("nan")), dict(mean=(0.5, 0.5)), dict(std=1e-60)):
        with pytest.raises(ValueError):
            gfla.normalize_images(torch.zeros(1, 2, 2, 3, dtype=torch.uint8), **bad)
    with pytest.raises(ValueError):
        gfla.normalize_images(torch.zeros(1, 2, 2, 5, dtype=torch.uint8))
    with pytest.raises(ValueError):
        gfla.pose_maps(torch.zeros(1, 2, 2), (7, 5), out=torch.zeros(1, 2, 7, 6))


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_the_header_is_bound_and_the_abi_is_as_pinned():
    names = {"gfla_pose_maps_band_rows"} | {"gfla_%s_%s" % (op, sfx) for op in ("pose_maps", "pose_cords", "normalize_images")
                                            for sfx in ("f32", "f16", "bf16")}
    assert names <= set(_lib.extension_symbols()) and not names & set(_lib.exported_symbols())
    assert len(_lib.exported_symbols()) == 154 and _lib.ABI_VERSION == 8 and _lib.PATH_COUNT == 22
    assert any(p.endswith("gfla_pose.h") for p in _lib.EXTENSION_HEADER_PATHS)
    handle = _lib.lib()
    for name in names:
        assert getattr(handle, name).argtypes is not None
    assert handle.gfla_pose_maps_band_rows() > 0


def test_the_abi_refuses_bad_arguments_before_anything_is_launched():
    """with a pointer that is never dereferenced: every one of these returns before a launch"""
    import ctypes
    handle, p = _lib.lib(), ctypes.c_void_p(4096)
    maps = handle.gfla_pose_maps_f32
    assert maps(None, None, 0, p, 1, 1, 7, 5, 7, 5, 72.0, None) == -1
    for B, J, H, W, H0, W0, two in ((0, 1, 7, 5, 7, 5, 72.0), (1, 0, 7, 5, 7, 5, 72.0), (1, 1, 0, 5, 7, 5, 72.0),
                                    (1, 1, 7, 0, 7, 5, 72.0), (1, 1, 7, 5, 0, 5, 72.0), (1, 1, 7, 5, 7, -1, 72.0),
                                    (1, 1, 7, 5, 7, 5, 0.0), (1, 1, 7, 5, 7, 5, -1.0), (1, 1, 7, 5, 7, 5, float("nan")),
                                    (1, 1, 7, 5, 7, 5, float("inf"))):
        assert maps(p, None, 0, p, B, J, H, W, H0, W0, two, None) == -2, (B, J, H, W, H0, W0, two)
    assert maps(p, p, 7, p, 1, 1, 7, 5, 7, 5, 72.0, None) == -2
    assert maps(p, None, 0, p, 1, 1, 7, 5000, 7, 5, 72.0, None) == _lib._ERR_UNSUPPORTED
    assert handle.gfla_pose_cords_f16(None, p, 1, 2, 2, 0.1, None) == -1
    assert handle.gfla_pose_cords_f16(p, p, 0, 2, 2, 0.1, None) == -2
    assert handle.gfla_pose_cords_f16(p, p, 1, 2, 2, float("nan"), None) == -2
    assert handle.gfla_pose_cords_bf16(p, p, 1, 1 << 20, 1 << 20, 0.1, None) == _lib._ERR_UNSUPPORTED
    half = (ctypes.c_double * 4)(0.5, 0.5, 0.5, 0.5)
    zero = (ctypes.c_double * 4)(0.5, 0.0, 0.5, 0.5)
    at = lambda a: ctypes.c_void_p(ctypes.addressof(a))      # noqa: E731
    norm = handle.gfla_normalize_images_bf16
    assert norm(p, p, 1, 2, 2, 3, None, at(half), None) == -1
    assert norm(p, p, 1, 2, 2, 5, at(half), at(half), None) == -2 and norm(p, p, 1, 2, 2, 0, at(half), at(half), None) == -2
    assert norm(p, p, 1, 2, 2, 3, at(half), at(zero), None) == -2
    assert norm(p, p, 1, 1 << 20, 1 << 20, 3, at(half), at(half), None) == _lib._ERR_UNSUPPORTED


def test_routes_that_need_the_gpu_refuse_cpu_tensors():
    with pytest.raises(NotImplementedError):
        pose_inputs._launch_pose_maps(torch.zeros(1, 2, 2), None, 1, 2, 7, 5, 7, 5, 72.0, torch.float32)
    with pytest.raises(NotImplementedError):
        pose_inputs._launch_pose_cords(torch.zeros(1, 1, 2, 2), 0.1)
    with pytest.raises(NotImplementedError):
        pose_inputs._launch_normalize_images(torch.zeros(1, 2, 2, 3, dtype=torch.uint8), [0.5] * 3, [0.5] * 3, torch.float32)
    with pytest.raises(NotImplementedError):
        gfla.PoseInputs((7, 5), device="cpu")
    assert {"PoseInputs", "pose_maps", "pose_cords", "normalize_images"} <= set(dir(gfla))
