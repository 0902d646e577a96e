"""Image inputs without a GPU (image_inputs.py, include/gfla_image.h): the torch compositions against Pillow's own bytes
(tests/golden/image_golden.npz, tests/golden/make_image_golden.py) and against live Pillow where it is installed, the
matrices against the reference's, the poisoned samples, the argument errors and the ABI.  Every bar is 0: tests/image_util.py."""
import ctypes

import numpy as np
import pytest
import torch

import global_flow_local_attention_amd as gfla
from global_flow_local_attention_amd import _lib, image_inputs

import image_util as iu

AFFINE_CASES = iu.affine_cases()
RESIZE_CASES = iu.resize_cases()


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


# ---- the goldens --------------------------------------------------------------------------------------------------------------
def test_the_goldens_cover_what_they_are_there_for():
    assert str(iu.golden()["pillow_version"])
    by_name = {c[0]: c for c in AFFINE_CASES}
    assert {tuple(c[1].shape[:2]) for c in AFFINE_CASES} == {(7, 5), (33, 17), (64, 40)}
    assert {c[1].shape[2] for c in AFFINE_CASES} == {1, 3, 4} and {c[3][0] for c in AFFINE_CASES} == {128, 255, 0}
    rotated = [c for c in AFFINE_CASES if c[2][0] != 0]
    plain = [c for c in AFFINE_CASES if c[2][0] == 0]
    assert len(rotated) >= 5 and all(c[4][0, 1] != 0 and c[4][1, 0] != 0 for c in rotated)
    assert all(c[4][0, 1] == 0 and c[4][1, 0] == 0 for c in plain)
    assert any(c[2][3] == 1 and c[2][1] % 1 != 0 for c in plain) and any(c[2][3] == 1 and c[2][1] % 1 == 0 and c[2][1] != 0 for c in plain)
    assert any(c[2][3] != 1 for c in plain)
    for name in ("identity_33x17_c3", "identity_7x5_c4"):
        assert by_name[name][2] == (0.0, 0.0, 0.0, 1.0) and torch.equal(by_name[name][6], by_name[name][1])
    for name in ("outside_33x17_c3", "outside_rot_7x5_c1"):
        c = by_name[name]
        assert (c[6] == torch.tensor(c[3], dtype=torch.uint8)).all()
    geometries = {(tuple(c[1].shape[:2]), c[2]) for c in RESIZE_CASES}
    assert {((37, 53), (16, 16)), ((16, 16), (37, 53)), ((20, 32), (20, 13)), ((20, 32), (31, 32)), ((9, 9), (9, 9))} == geometries
    assert len(RESIZE_CASES) == 10 and {c[3] for c in RESIZE_CASES} == {"bilinear", "bicubic"}


@pytest.mark.parametrize("case", AFFINE_CASES, ids=[c[0] for c in AFFINE_CASES])
def test_affine_composition_equals_every_golden_byte(case):
    name, image, params, fill, inverse, forward, want = case
    got, bad = image_inputs.torch_affine_bytes(image[None], inverse[None], fill)
    assert not bad.any() and got.dtype == torch.uint8 and torch.equal(got[0], want)
    for mean, std in ((0.5, 0.5), (0.0, 1.0)):                       # the image route and the mask route
        out = gfla.affine_images(image[None], inverse[None], fill, mean, std)
        assert out.dtype == torch.float32 and out.shape == (1, image.shape[2]) + tuple(image.shape[:2])
        assert torch.equal(bits(out), bits(gfla.torch_normalize_images(want[None], mean, std)))
        assert torch.equal(bits(gfla.affine_images(image[None], inverse[None], fill, mean, std, impl="torch")), bits(out))


def test_at_least_one_angle_0_golden_differs_between_the_two_branches():
    differing = {}
    for name, image, params, fill, inverse, forward, want in AFFINE_CASES:
        if params[0] == 0:
            fixed, _ = image_inputs.torch_affine_bytes(image[None], inverse[None], fill, scale_branch=False)
            differing[name] = int((fixed[0] != want).sum())
    assert sum(n > 0 for n in differing.values()) >= 2, differing
    rotated = [c for c in AFFINE_CASES if c[2][0] != 0][0]              # with a rotation the switch changes nothing
    assert torch.equal(image_inputs.torch_affine_bytes(rotated[1][None], rotated[4][None], rotated[3], scale_branch=False)[0][0], rotated[6])


@pytest.mark.parametrize("case", RESIZE_CASES, ids=[c[0] for c in RESIZE_CASES])
def test_resize_composition_equals_every_golden_byte(case):
    name, image, size, interpolation, want = case
    got = gfla.resize_images(image[None], size, interpolation)
    assert got.dtype == torch.uint8 and torch.equal(got[0], want)
    assert torch.equal(gfla.resize_images(image[None], size, interpolation, impl="torch"), got)
    if tuple(image.shape[:2]) == size:
        assert torch.equal(got[0], image) and got.data_ptr() != image.data_ptr()           # a copy


def test_a_batch_is_its_samples_one_by_one():
    cases = [c for c in AFFINE_CASES if tuple(c[1].shape) == (33, 17, 3)]
    assert len(cases) >= 4 and len({c[2][0] == 0 for c in cases}) == 2                    # both branches in one batch
    images, inverse = torch.stack([c[1] for c in cases]), torch.stack([c[4] for c in cases])
    got, bad = image_inputs.torch_affine_bytes(images, inverse, 128)
    for i, c in enumerate(cases):
        alone, _ = image_inputs.torch_affine_bytes(c[1][None], c[4][None], 128)
        assert torch.equal(got[i], alone[0])


# ---- live Pillow ---------------------------------------------------------------------------------------------------------------
def test_compositions_against_live_pillow_at_256_by_176():
    pytest.importorskip("PIL")
    rng = np.random.RandomState(7)
    H, W = 256, 176
    angles, shifts, scales = [0.0, 14.2, -28.0, 0.0], [(3.0, -2.0), (7.7, -11.3), (-19.0, 4.4), (0.31, 12.9)], [1.0, 1.17, 0.84, 1.0 / 1.1]
    inverse, _ = gfla.augmentation_matrices(angles, shifts, scales, (H, W))
    for C, fill in ((3, 128), (1, 255), (4, 0)):
        images = rng.randint(0, 256, (4, H, W, C)).astype(np.uint8)
        got, bad = image_inputs.torch_affine_bytes(torch.from_numpy(images), inverse, fill)
        assert not bad.any()
        want = np.stack([iu.pil_affine(images[b], inverse[b].numpy(), (fill,) * C) for b in range(4)])
        assert np.array_equal(got.numpy(), want), (C, fill)
        floats = gfla.affine_images(torch.from_numpy(images), inverse, fill)
        assert torch.equal(bits(floats), bits(gfla.torch_normalize_images(torch.from_numpy(want))))
    for shape, size in (((300, 240, 3), (H, W)), ((256, 256, 1), (H, W)), ((64, 44, 3), (H, W))):
        image = rng.randint(0, 256, shape).astype(np.uint8)
        for interpolation in ("bilinear", "bicubic"):
            got = gfla.resize_images(torch.from_numpy(image)[None], size, interpolation)[0]
            assert np.array_equal(got.numpy(), iu.pil_resize(image, size, interpolation)), (shape, interpolation)


# ---- augmentation_matrices ------------------------------------------------------------------------------------------------------
def test_augmentation_matrices_equal_the_goldens_bit_for_bit():
    for size in ((7, 5), (33, 17), (64, 40)):
        cases = [c for c in AFFINE_CASES if tuple(c[1].shape[:2]) == size]
        inverse, forward = gfla.augmentation_matrices([c[2][0] for c in cases], [c[2][1:3] for c in cases], [c[2][3] for c in cases], size)
        assert inverse.dtype == forward.dtype == torch.float64 and inverse.shape == (len(cases), 2, 3) and forward.shape == (len(cases), 3, 3)
        assert torch.equal(inverse.view(torch.int64), torch.stack([c[4] for c in cases]).view(torch.int64))
        assert torch.equal(forward.view(torch.int64), torch.stack([c[5] for c in cases]).view(torch.int64))
    inverse, forward = gfla.augmentation_matrices(torch.tensor([0.0]), torch.tensor([[0.0, 0.0]]), torch.tensor([1.0]), (7, 5))
    assert inverse[0].tolist() == [[1, 0, 0], [0, 1, 0]] and forward[0].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]


@pytest.mark.skipif(not iu.HAVE_REF, reason="reference checkout not present")
def test_augmentation_matrices_equal_the_live_reference_bit_for_bit():
    ref = iu.reference_base_dataset()
    rng = np.random.RandomState(3)
    angles = [0.0, 90.0] + rng.uniform(-30, 30, 6).tolist()
    shifts = [(0.0, 0.0), (1.0, -2.0)] + [tuple(v) for v in rng.uniform(-20, 20, (6, 2)).tolist()]
    scales = [1.0, 1.0] + rng.uniform(0.8, 1.3, 6).tolist()
    inverse, forward = gfla.augmentation_matrices(angles, shifts, scales, (256, 176))
    for b in range(8):
        want_inverse, want_forward = iu.reference_matrices(ref, angles[b], shifts[b], scales[b], (256, 176))
        assert np.array_equal(inverse[b].numpy().view(np.int64), want_inverse.view(np.int64)), b
        assert np.array_equal(forward[b].numpy().view(np.int64), want_forward.view(np.int64)), b


def test_forward_matrices_move_key_points_with_the_pixels():
    """a bright pixel and its key point land in the same place: the two matrices of one augmentation agree"""
    H, W = 33, 17
    inverse, forward = gfla.augmentation_matrices([10.0], [(1.0, 2.0)], [1.1], (H, W))
    image = torch.zeros(1, H, W, 1, dtype=torch.uint8)
    image[0, 14:17, 7:10] = 255
    warped, _ = image_inputs.torch_affine_bytes(image, inverse, 0)
    ys, xs = warped[0, :, :, 0].nonzero(as_tuple=True)
    peak = gfla.pose_cords(gfla.pose_maps(torch.tensor([[[15, 8]]]), (H, W), affine=forward, sigma=1.5))[0, 0]
    assert abs(float(ys.float().mean()) - int(peak[0])) <= 1 and abs(float(xs.float().mean()) - int(peak[1])) <= 1


# ---- poisoned samples, 16-bit outputs ------------------------------------------------------------------------------------------
def test_a_poisoned_sample_is_nan_and_leaves_its_neighbours_untouched():
    cases = [c for c in AFFINE_CASES if tuple(c[1].shape) == (33, 17, 3)][:3]
    images, inverse = torch.stack([c[1] for c in cases]), torch.stack([c[4] for c in cases])
    clean = gfla.affine_images(images, inverse)
    far = inverse[1].clone()
    far[0, 2] = 32767.0 - far[0, 0] * 17                               # the corner (W, 0) reaches 32767 exactly
    assert float(far[0, 0]) * 17 + float(far[0, 2]) == 32767.0
    endless = inverse[1].clone()
    endless[1, 1] = float("inf")
    for poison in (torch.full((2, 3), float("nan"), dtype=torch.float64), endless, far,
                   torch.tensor([[1e308, -1e308, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64)):      # inf - inf at a corner
        m = inverse.clone()
        m[1] = poison
        got = gfla.affine_images(images, m)
        assert got[1].isnan().all() and torch.equal(bits(got[0]), bits(clean[0])) and torch.equal(bits(got[2]), bits(clean[2]))
        _, bad = image_inputs.torch_affine_bytes(images, m)
        assert bad.tolist() == [False, True, False]
    near = inverse[1].clone()
    near[0, 2] = 32766.0 - near[0, 0] * 17                             # just inside the bound: every pixel is the fill
    m = inverse.clone()
    m[1] = near
    got, bad = image_inputs.torch_affine_bytes(images, m, 7)
    assert not bad.any() and (got[1] == 7).all()


def test_sixteen_bit_outputs_are_the_float32_outputs_rounded_once():
    name, image, params, fill, inverse, forward, want = AFFINE_CASES[0]
    full = gfla.affine_images(image[None], inverse[None], fill, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    for dtype in _lib.HALF_TYPES:
        got = gfla.affine_images(image[None], inverse[None], fill, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), dtype=dtype)
        assert got.dtype == dtype and torch.equal(bits(got), bits(full.to(dtype)))
    out = torch.empty_like(full)
    assert gfla.affine_images(image[None], inverse[None], fill, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), out=out) is out
    assert torch.equal(bits(out), bits(full))


def test_a_fill_per_channel():
    name, image, params, fill, inverse, forward, want = [c for c in AFFINE_CASES if c[0] == "outside_33x17_c3"][0]
    got, _ = image_inputs.torch_affine_bytes(image[None], inverse[None], (1, 2, 3))
    assert (got[0] == torch.tensor([1, 2, 3], dtype=torch.uint8)).all()


# ---- the resize coefficients ---------------------------------------------------------------------------------------------------
def test_resize_coefficients_are_pillows_shape():
    ksize, bounds, coeffs = image_inputs.resize_coefficients(750, 176, "bicubic")
    assert ksize == 19 and len(bounds) == len(coeffs) == 176 and all(len(k) == ksize for k in coeffs)
    assert all(0 <= first and first + count <= 750 and 0 < count <= ksize for first, count in bounds)
    assert all(abs(sum(k) - (1 << 22)) <= ksize for k in coeffs) and any(v < 0 for k in coeffs for v in k)
    ksize, bounds, coeffs = image_inputs.resize_coefficients(16, 37, "bilinear")
    assert ksize == 3 and min(min(k) for k in coeffs) >= 0
    assert image_inputs.resize_coefficients(16, 37, "bilinear") is image_inputs.resize_coefficients(16, 37, "bilinear")      # cached


# ---- argument errors -----------------------------------------------------------------------------------------------------------
U8 = torch.zeros(2, 7, 5, 3, dtype=torch.uint8)
EYE = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64).repeat(2, 1, 1)


@pytest.mark.parametrize("kwargs", [dict(fill=256), dict(fill=-1), dict(fill=1.5), dict(fill=(1, 2)), dict(fill="grey"), dict(fill=float("nan")),
                                    dict(std=0.0), dict(mean=float("nan")), dict(mean=(0.5, 0.5)), dict(impl="hip"),
                                    dict(inverse=EYE[:1]), dict(inverse=torch.zeros(2, 3, 3, dtype=torch.float64)),
                                    dict(images_u8=torch.zeros(2, 7, 5, 5, dtype=torch.uint8)), dict(images_u8=torch.zeros(2, 0, 5, 3, dtype=torch.uint8)),
                                    dict(images_u8=torch.zeros(7, 5, 3, dtype=torch.uint8)), dict(out=torch.zeros(2, 3, 7, 6))],
                         ids=lambda k: "-".join("%s" % key for key in k))
def test_affine_images_argument_errors_raise_value_error(kwargs):
    args = dict(images_u8=U8, inverse=EYE)
    args.update(kwargs)
    with pytest.raises(ValueError):
        gfla.affine_images(**args)


def test_type_errors_and_the_other_value_errors():
    with pytest.raises(TypeError):
        gfla.affine_images(U8.float(), EYE)
    with pytest.raises(TypeError):
        gfla.affine_images(U8, EYE.float())
    with pytest.raises(TypeError):
        gfla.affine_images(U8, EYE, dtype=torch.float64)
    with pytest.raises(TypeError):
        gfla.resize_images(U8.float(), (7, 5))
    for bad in (dict(size=(0, 5)), dict(size=(7,)), dict(size=(7, 5), interpolation="nearest"), dict(size=(7, 5), impl="hip"),
                dict(size=(7, 5), out=torch.zeros(2, 7, 5, 3)), dict(size=(9, 5), out=torch.zeros(2, 7, 5, 3, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            gfla.resize_images(U8, **bad)
    with pytest.raises(ValueError):
        gfla.resize_images(torch.zeros(2, 7, 5, 5, dtype=torch.uint8), (7, 5))
    for bad in (dict(angle=[0.0, 1.0]), dict(scale=[0.0]), dict(scale=[float("inf")]), dict(translate=[0.0]), dict(size=(0, 5)), dict(angle=[])):
        args = dict(angle=[0.0], translate=[(0.0, 0.0)], scale=[1.0], size=(7, 5))
        args.update(bad)
        with pytest.raises(ValueError):
            gfla.augmentation_matrices(**args)
    with pytest.raises(ValueError):
        gfla.PoseInputs((7, 5), device="cuda", fill=300)


# ---- ABI -----------------------------------------------------------------------------------------------------------------------
NAMES = {"gfla_affine_images_workspace_bytes", "gfla_resize_pass_u8"} | {"gfla_affine_images_" + sfx for sfx in ("f32", "f16", "bf16")}


def test_the_header_is_bound_and_the_abi_is_as_pinned():
    assert NAMES <= set(_lib.extension_symbols()) and not NAMES & set(_lib.exported_symbols())
    assert len(_lib.exported_symbols()) == 154 and _lib.ABI_VERSION == 8 and _lib.PATH_COUNT == 22
    assert any(p.endswith("gfla_image.h") for p in _lib.EXTENSION_HEADER_PATHS)
    handle = _lib.lib()
    for name in NAMES:
        assert getattr(handle, name).argtypes is not None
    assert handle.gfla_affine_images_workspace_bytes(2, 7, 5) == 2 * (8 + 7 + 5) * 4
    assert {"affine_images", "resize_images", "augmentation_matrices", "torch_affine_images", "torch_resize_images"} <= set(dir(gfla))


def test_the_abi_refuses_bad_arguments_before_anything_is_launched():
    """with a pointer that is never dereferenced: every one of these returns before a launch"""
    handle, p = _lib.lib(), ctypes.c_void_p(4096)
    at = lambda a: ctypes.c_void_p(ctypes.addressof(a))      # noqa: E731
    half, grey = (ctypes.c_double * 4)(0.5, 0.5, 0.5, 0.5), (ctypes.c_double * 4)(128, 128, 128, 128)
    zero, frac, big = (ctypes.c_double * 4)(0.5, 0.0, 0.5, 0.5), (ctypes.c_double * 4)(128, 1.5, 128, 128), (ctypes.c_double * 4)(128, 256, 128, 128)
    affine = handle.gfla_affine_images_f16
    good = (at(grey), at(half), at(half))
    for i in range(4):
        ptrs = [p, p, p, p]
        ptrs[i] = None
        assert affine(*ptrs, 1, 7, 5, 3, *good, None) == -1, i
    for i in range(3):
        host = list(good)
        host[i] = None
        assert affine(p, p, p, p, 1, 7, 5, 3, *host, None) == -1, i
    for B, H, W, C in ((0, 7, 5, 3), (1, 0, 5, 3), (1, 7, -1, 3), (1, 7, 5, 0), (1, 7, 5, 5)):
        assert affine(p, p, p, p, B, H, W, C, *good, None) == -2, (B, H, W, C)
    assert affine(p, p, p, p, 1, 7, 5, 3, at(frac), at(half), at(half), None) == -2
    assert affine(p, p, p, p, 1, 7, 5, 3, at(big), at(half), at(half), None) == -2
    assert affine(p, p, p, p, 1, 7, 5, 3, at(grey), at(half), at(zero), None) == -2
    assert affine(p, p, p, p, 1, 7, 40000, 3, *good, None) == _lib._ERR_UNSUPPORTED
    assert affine(p, p, p, p, 1 << 40, 7, 5, 3, *good, None) == _lib._ERR_UNSUPPORTED
    query = handle.gfla_affine_images_workspace_bytes
    assert query(0, 7, 5) == -2 and query(1, 7, 0) == -2 and query(1, 40000, 5) == _lib._ERR_UNSUPPORTED
    resize = handle.gfla_resize_pass_u8
    for i in range(4):
        ptrs = [p, p, p, p]
        ptrs[i] = None
        assert resize(*ptrs, 2, 16, 37, 3, 3, None) == -1, i
    for sizes in ((0, 16, 37, 3, 3), (2, 0, 37, 3, 3), (2, 16, 0, 3, 3), (2, 16, 37, 0, 3), (2, 16, 37, 3, 0)):
        assert resize(p, p, p, p, *sizes, None) == -2, sizes
    assert resize(p, p, p, p, 2, 16, 37, 3, 5000, None) == _lib._ERR_UNSUPPORTED
    assert resize(p, p, p, p, 1 << 20, 1 << 10, 37, 3, 3, None) == _lib._ERR_UNSUPPORTED
    assert resize(p, p, p, p, 1 << 20, 16, 1 << 10, 3, 3, None) == _lib._ERR_UNSUPPORTED


def test_routes_that_need_the_gpu_refuse_cpu_tensors():
    with pytest.raises(NotImplementedError):
        image_inputs._launch_affine_images(U8, EYE, (128,) * 3, [0.5] * 3, [0.5] * 3, torch.float32)
    with pytest.raises(NotImplementedError):
        image_inputs._launch_resize_images(U8, 9, 5, "bilinear")
