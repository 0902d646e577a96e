"""Image inputs on the GPU (csrc/image_inputs.hip): the kernels against Pillow's bytes (tests/golden/image_golden.npz) and
against the torch compositions that tests/test_image_inputs_cpu.py pins to Pillow; every placement of their pointers inside
red zones; poisoned samples; PoseInputs with warps from host records, without a synchronisation, and captured in a graph.
Nothing here reads the reference or needs Pillow.  Every bar is 0: tests/image_util.py."""
import functools

import pytest
import torch

import global_flow_local_attention_amd as gfla
import image_util as iu
import placement_util as plu
from global_flow_local_attention_amd import image_inputs
from global_flow_local_attention_amd.extractor_attn import GraphedCall

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
AFFINE_CASES = iu.affine_cases()
RESIZE_CASES = iu.resize_cases()
IMAGENET = ((0.485, 0.456, 0.406, 0.4), (0.229, 0.224, 0.225, 0.25))


def dev(t):
    return None if t is None else t.to(DEV)


def bits(t):
    return plu.bits(t.detach().contiguous()).cpu()


# ---- affine_images ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AFFINE_CASES, ids=[c[0] for c in AFFINE_CASES])
def test_affine_kernel_equals_the_goldens_and_the_composition(case):
    name, image, params, fill, inverse, forward, want = case
    C = image.shape[2]
    args = (dev(image[None]), dev(inverse[None]), fill)
    for dtype in DTYPES.values():
        for mean, std in ((0.5, 0.5), (0.0, 1.0), (IMAGENET[0][:C], IMAGENET[1][:C])):
            got = gfla.affine_images(*args, mean, std, dtype=dtype)
            assert got.is_cuda and got.dtype == dtype and got.shape == (1, C) + tuple(image.shape[:2]) and got.is_contiguous()
            assert torch.equal(bits(got), bits(gfla.torch_normalize_images(want[None], mean, std, dtype))), (dtype, mean)
            assert torch.equal(bits(got), bits(gfla.affine_images(*args, mean, std, dtype=dtype, impl="torch")))
            assert torch.equal(bits(got), bits(gfla.affine_images(*args, mean, std, dtype=dtype)))          # and again: the same bits


def test_a_batch_of_golden_cases_takes_both_branches_in_one_launch():
    cases = [c for c in AFFINE_CASES if tuple(c[1].shape) == (33, 17, 3)]
    assert len({c[2][0] == 0 for c in cases}) == 2
    images, inverse = torch.stack([c[1] for c in cases]), torch.stack([c[4] for c in cases])
    got = gfla.affine_images(dev(images), dev(inverse), 128)
    assert torch.equal(bits(got), bits(gfla.affine_images(images, inverse, 128)))
    for i, c in enumerate(cases):
        if c[3][0] == 128:                                            # the fill this golden was made with
            assert torch.equal(bits(got[i]), bits(gfla.torch_normalize_images(c[6][None])[0])), c[0]


@functools.lru_cache(maxsize=None)
def real_case():
    g = torch.Generator().manual_seed(256176)
    images = torch.randint(0, 256, (2, 256, 176, 3), dtype=torch.uint8, generator=g)
    inverse, _ = gfla.augmentation_matrices([11.5, 0.0], [(4.25, -7.5), (-3.0, 6.5)], [1.12, 1.0 / 1.1], (256, 176))
    return images, inverse, gfla.affine_images(images, inverse, 128)


def test_affine_kernel_at_256_by_176_against_the_composition():
    images, inverse, composed = real_case()
    fixed, _ = image_inputs.torch_affine_bytes(images[1:], inverse[1:], 128, scale_branch=False)
    assert not torch.equal(fixed, image_inputs.torch_affine_bytes(images[1:], inverse[1:], 128)[0])       # sample 1 tells the branches apart
    got = gfla.affine_images(dev(images), dev(inverse), 128)
    assert torch.equal(bits(got), bits(composed))
    for dtype in (torch.float16, torch.bfloat16):
        assert torch.equal(bits(gfla.affine_images(dev(images), dev(inverse), 128, dtype=dtype)), bits(composed.to(dtype)))


def test_a_nan_matrix_in_sample_1_of_3_poisons_only_sample_1():
    cases = [c for c in AFFINE_CASES if tuple(c[1].shape) == (64, 40, 3)] * 2
    images, inverse = torch.stack([c[1] for c in cases[:3]]), torch.stack([c[4] for c in cases[:3]])
    clean = gfla.affine_images(images, inverse)
    far = inverse[1].clone()
    far[0, 2] = 40000.0
    for poison in (torch.full((2, 3), float("nan"), dtype=torch.float64), far,
                   torch.tensor([[1.0, 0.0, 0.0], [float("inf"), 1.0, 0.0]], dtype=torch.float64)):
        m = inverse.clone()
        m[1] = poison
        for dtype in DTYPES.values():
            out = torch.zeros((3, 3, 64, 40), dtype=dtype, device=DEV)
            got = gfla.affine_images(dev(images), dev(m), dtype=dtype, out=out).cpu()
            assert got[1].isnan().all() and not got[0].isnan().any() and not got[2].isnan().any()
            assert torch.equal(bits(got[0]), bits(clean[0].to(dtype))) and torch.equal(bits(got[2]), bits(clean[2].to(dtype)))
            assert torch.equal(got.isnan(), gfla.affine_images(images, m, dtype=dtype).isnan())


# ---- placement --------------------------------------------------------------------------------------------------------------
def placed_out(shape, dtype, phase):
    """an output buffer full of NaN (0xA5 for integers) at `phase` elements, inside red zones"""
    filler = torch.full(shape, float("nan"), dtype=dtype) if dtype.is_floating_point else torch.full(shape, 0xA5, dtype=dtype)
    view, rec = plu.place(filler, phase, DEV)
    rec.kind = "inout"
    return view, rec


@functools.lru_cache(maxsize=None)
def placement_case(W):
    H = {5: 211, 17: 67, 40: 33}[W]                                   # more than 1024 pixels: two workgroups per sample
    images = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(W))
    inverse, _ = gfla.augmentation_matrices([0.0, -9.0], [(0.5, 1.5), (1.0, -2.0)], [1.0 / 1.1, 0.95], (H, W))
    return images, inverse, gfla.affine_images(images, inverse, (7, 128, 255))


@pytest.mark.parametrize("W", [5, 17, 40])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_affine_images_at_every_phase_of_its_pointers(name, W):
    dtype = DTYPES[name]
    images, inverse, composed = placement_case(W)
    want = composed.to(dtype)
    assert not want.isnan().any()
    steps = 16 // dtype.itemsize
    for phase in range(16):
        src, rec_in = plu.place(images, phase, DEV)
        mat, rec_mat = plu.place(inverse, phase % 2, DEV)
        out, rec_out = placed_out(want.shape, dtype, phase % steps)
        assert src.data_ptr() % 16 == phase and mat.data_ptr() % 16 == 8 * (phase % 2)
        assert out.data_ptr() % 16 == (phase % steps) * dtype.itemsize
        gfla.affine_images(src, mat, (7, 128, 255), dtype=dtype, out=out)
        plu.check_zones([rec_in, rec_mat, rec_out])
        assert plu.bit_equal(out.cpu(), want), phase                  # every element written: none of the NaN is left


def test_resize_at_every_phase_of_its_pointers():
    name, image, size, interpolation, want = [c for c in RESIZE_CASES if c[0] == "down_bicubic"][0]
    for phase in range(16):
        src, rec_in = plu.place(image[None], phase, DEV)
        out, rec_out = placed_out((1,) + tuple(want.shape), torch.uint8, (phase * 7) % 16)
        assert src.data_ptr() % 16 == phase and out.data_ptr() % 16 == (phase * 7) % 16
        gfla.resize_images(src, size, interpolation, out=out)
        plu.check_zones([rec_in, rec_out])
        assert torch.equal(out.cpu()[0], want), phase


# ---- resize_images ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RESIZE_CASES, ids=[c[0] for c in RESIZE_CASES])
def test_resize_kernels_equal_the_goldens(case):
    name, image, size, interpolation, want = case
    src = dev(image[None])
    got = gfla.resize_images(src, size, interpolation)
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous() and torch.equal(got.cpu()[0], want)
    assert torch.equal(gfla.resize_images(src, size, interpolation).cpu()[0], want)                  # and again
    assert torch.equal(gfla.resize_images(src, size, interpolation, impl="torch").cpu()[0], want)
    if tuple(image.shape[:2]) == size:
        assert got.data_ptr() != src.data_ptr()
    both = torch.stack([image, image.flip(0)])                        # a batch of two
    assert torch.equal(gfla.resize_images(dev(both), size, interpolation).cpu(), gfla.resize_images(both, size, interpolation))


def test_resize_then_warp_is_the_loaders_pipeline():
    g = torch.Generator().manual_seed(5)
    raw = torch.randint(0, 256, (2, 300, 240, 3), dtype=torch.uint8, generator=g)
    inverse, _ = gfla.augmentation_matrices([7.0, 0.0], [(3.0, 2.0), (0.5, -4.0)], [1.05, 0.9], (256, 176))
    got = gfla.affine_images(gfla.resize_images(dev(raw), (256, 176), "bicubic"), dev(inverse), 255)
    want = gfla.affine_images(gfla.resize_images(raw, (256, 176), "bicubic"), inverse, 255)
    assert torch.equal(bits(got), bits(want))


# ---- PoseInputs -------------------------------------------------------------------------------------------------------------
SIZE, B, J = (64, 44), 2, 18


def records(seed):
    g = torch.Generator().manual_seed(seed)
    images = [torch.randint(0, 256, (B, SIZE[0], SIZE[1], 3), dtype=torch.uint8, generator=g) for _ in range(2)]
    cords = [torch.stack([torch.randint(0, 256, (B, J), generator=g), torch.randint(0, 176, (B, J), generator=g)], dim=2)
             for _ in range(2)]
    angles = (torch.rand(2, B, generator=g) * 40 - 20).tolist()
    angles[1][0] = 0.0                                                 # the scale branch too
    shifts = (torch.rand(2, B, 2, generator=g) * 12 - 6).tolist()
    scales = (torch.rand(2, B, generator=g) * 0.4 + 0.8).tolist()
    inverse1, forward1 = gfla.augmentation_matrices(angles[0], shifts[0], scales[0], SIZE)
    inverse2, forward2 = gfla.augmentation_matrices(angles[1], shifts[1], scales[1], SIZE)
    return images + cords + [forward1, forward2, inverse1, inverse2]


def expected(recs, dtype, fill):
    P1, P2, c1, c2, a1, a2, w1, w2 = recs
    maps = dict(size=SIZE, old_size=(256, 176), sigma=6.0, dtype=dtype)
    return {"P1": gfla.affine_images(P1, w1, fill, dtype=dtype), "P2": gfla.affine_images(P2, w2, fill, dtype=dtype),
            "BP1": gfla.pose_maps(c1, affine=a1, **maps), "BP2": gfla.pose_maps(c2, affine=a2, **maps)}


def check_batch(batch, want, dtype):
    import pose_util as pu
    assert sorted(batch) == ["BP1", "BP2", "P1", "P2"]
    for key, t in batch.items():
        assert t.is_cuda and t.dtype == dtype and t.shape == want[key].shape
    for key in ("P1", "P2"):
        assert torch.equal(bits(batch[key]), bits(want[key])), key
    for key in ("BP1", "BP2"):
        assert pu.ulp_distance(batch[key], want[key]) <= 1, key          # tests/pose_util.py's bar for the maps


@pytest.mark.parametrize("name", ["f32", "f16"])
def test_pose_inputs_with_warps_from_host_records_without_a_synchronisation(name):
    dtype = DTYPES[name]
    inputs = gfla.PoseInputs(SIZE, old_size=(256, 176), dtype=dtype, fill=(128, 128, 128))
    rounds = [records(seed) for seed in range(4)]
    inputs(*rounds[0][:6], warp1=rounds[0][6], warp2=rounds[0][7])
    inputs(*rounds[1][:6], warp1=rounds[1][6], warp2=rounds[1][7])    # both staging sets exist now
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [inputs(*recs[:6], warp1=recs[6], warp2=recs[7]) for recs in rounds[2:]]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for batch, recs in zip(got, rounds[2:]):
        check_batch(batch, expected(recs, dtype, 128), dtype)


def test_pose_inputs_with_one_warp_leaves_the_other_image_to_normalize_images():
    recs = records(21)
    inputs = gfla.PoseInputs(SIZE, old_size=(256, 176), fill=0)
    batch = inputs(*recs[:5], None, warp1=recs[6])
    assert torch.equal(bits(batch["P1"]), bits(gfla.affine_images(recs[0], recs[6], 0)))
    assert torch.equal(bits(batch["P2"]), bits(gfla.normalize_images(recs[1])))
    plain = inputs(*recs[:6])
    assert torch.equal(bits(plain["P1"]), bits(gfla.normalize_images(recs[0])))


def test_pose_inputs_captured_in_a_graph_follows_its_matrices():
    inputs = gfla.PoseInputs(SIZE, old_size=(256, 176), fill=128)
    first, second = ([dev(t) for t in records(seed)] for seed in (11, 12))

    def call(*r):
        return inputs(*r[:6], warp1=r[6], warp2=r[7])
    graphed = GraphedCall(call, first)
    batch = graphed(*first)
    check_batch(batch, expected(records(11), torch.float32, 128), torch.float32)
    for static, new in zip(graphed.static_inputs[4:], second[4:]):      # the matrices alone, overwritten in place; one replay
        static.copy_(new)
    graphed.graph.replay()
    torch.cuda.synchronize()
    mixed = records(11)[:4] + records(12)[4:]
    check_batch(graphed.static_outputs, expected(mixed, torch.float32, 128), torch.float32)
    eager = call(*(dev(t) for t in mixed))
    for key in ("P1", "P2", "BP1", "BP2"):
        assert torch.equal(bits(graphed.static_outputs[key]), bits(eager[key])), key
    assert not torch.equal(bits(graphed.static_outputs["P1"]), bits(expected(records(11), torch.float32, 128)["P1"]))
