"""Pose inputs on the GPU (csrc/pose_inputs.hip): the three kernels against the goldens of the reference
(tests/golden/pose_golden.npz) and against the torch compositions that tests/test_pose_inputs_cpu.py pins to the reference;
every placement of their pointers inside red zones; PoseInputs with host records, without a synchronisation, and captured
in a graph.  Nothing here reads the reference.  Bars: tests/pose_util.py."""
import functools

import pytest
import torch

import global_flow_local_attention_amd as gfla
import placement_util as plu
import pose_util as pu
from global_flow_local_attention_amd import _lib
from global_flow_local_attention_amd.extractor_attn import GraphedCall

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
MAP_CASES = pu.map_cases()
CORD_CASES = pu.cord_cases()


def dev(t):
    return None if t is None else t.to(DEV)


def bits(t):
    return plu.bits(t.detach().contiguous()).cpu()


# ---- pose_maps --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MAP_CASES, ids=[c[0] for c in MAP_CASES])
def test_pose_maps_kernel_against_the_goldens_and_the_composition(case):
    name, cords, size, old_size, affine, sigma, want = case
    args = (dev(cords), size, old_size, dev(affine), sigma)
    got = gfla.pose_maps(*args)
    composed = gfla.pose_maps(*args, impl="torch")
    d_gold, d_comp = pu.ulp_distance(got, want), pu.ulp_distance(got, composed)
    tiny = pu.denormals(want)
    print("%s: %d ulp from the golden, %d from the composition, %d denormals" % (name, d_gold, d_comp, int(tiny.sum())))
    assert got.dtype == torch.float32 and got.is_cuda and d_gold <= 1 and d_comp <= 1
    assert torch.equal(bits(got)[tiny], bits(want)[tiny]) and torch.equal(pu.denormals(got.cpu()), tiny)
    for dtype in _lib.HALF_TYPES:                            # the same call's float32 output, rounded to nearest even once
        assert torch.equal(bits(gfla.pose_maps(*args, dtype=dtype)), bits(got.to(dtype)))


def test_the_goldens_the_kernel_is_held_to_contain_denormals():
    assert sum(int(pu.denormals(c[6]).sum()) for c in MAP_CASES) > 100


def test_missing_channels_are_written_as_zeros_into_a_buffer_full_of_nan():
    name, cords, size, old_size, affine, sigma, want = MAP_CASES[0]
    missing = (cords[..., 0] == -1) | (cords[..., 1] == -1)
    assert missing.any() and not missing.all()
    for dtype in DTYPES.values():
        out = torch.full(want.shape, float("nan"), dtype=dtype, device=DEV)
        assert gfla.pose_maps(dev(cords), size, old_size, dev(affine), sigma, dtype=dtype, out=out) is out
        got = out.cpu()
        assert not got.isnan().any() and not bits(got[missing]).any()        # +0, every bit
        assert (got[~missing].flatten(1).float().max(1).values >= 0).all()


@functools.lru_cache(maxsize=None)
def real_case():
    cords = pu.real_cords(B=2).to(DEV)
    return cords, gfla.pose_maps(cords, (256, 176), impl="torch")


def test_pose_maps_kernel_at_256_by_176_against_the_composition():
    cords, composed = real_case()
    got = gfla.pose_maps(cords, (256, 176))
    d = pu.ulp_distance(got, composed)
    print("256 x 176, B = 2, J = 18: %d ulp from the composition, %d denormals" % (d, int(pu.denormals(got.cpu()).sum())))
    assert d <= 1 and int(pu.denormals(got.cpu()).sum()) > 10000
    assert torch.equal(pu.denormals(got.cpu()), pu.denormals(composed.cpu()))
    assert torch.equal(bits(gfla.pose_maps(cords, (256, 176), dtype=torch.float16)), bits(got.to(torch.float16)))
    small = gfla.pose_maps(cords, (128, 64), old_size=(256, 176))
    assert pu.ulp_distance(small, gfla.pose_maps(cords, (128, 64), old_size=(256, 176), impl="torch")) <= 1


def test_the_quirk_columns_on_the_kernel():
    xs = torch.arange(176)
    cords = torch.stack([torch.full_like(xs, 3), xs], dim=1).view(1, 176, 2).to(DEV)
    peak = gfla.pose_cords(gfla.pose_maps(cords, (8, 176)))[0].cpu()
    assert tuple(int(x) for x in xs if peak[x, 1] != x) == pu.QUIRK_COLUMNS_176
    assert all(int(peak[x, 1]) == x - 1 for x in pu.QUIRK_COLUMNS_176) and (peak[:, 0] == 3).all()


def test_non_finite_key_points_give_nan_channels_and_only_those():
    cords = torch.tensor([[[2.0, 1.0], [float("nan"), 1.0], [2.0, float("inf")], [-1.0, float("nan")], [3.0, 3.0]],
                          [[2.0, 1.0], [1.0, 1.0], [2.0, 2.0], [-1.0, 2.0], [3.0, 3.0]]])
    affine = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    affine[1, 2, 0] = float("nan")
    for a, want in ((None, [[False, True, True, False, False], [False] * 5]),
                    (affine, [[False, True, True, False, False], [True, True, True, False, True]])):
        for dtype in DTYPES.values():
            got = gfla.pose_maps(dev(cords), (35, 19), affine=dev(a), dtype=dtype).cpu()
            nan = got.isnan().flatten(2)
            assert nan.all(2).tolist() == want and nan.any(2).tolist() == want
            composed = gfla.pose_maps(cords, (35, 19), affine=a, dtype=dtype)
            assert torch.equal(got.isnan(), composed.isnan())
            assert pu.ulp_distance(got, composed) <= 1


# ---- pose_cords -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CORD_CASES, ids=[c[0] for c in CORD_CASES])
def test_pose_cords_kernel_equals_the_goldens(case):
    name, maps, threshold, want = case
    got = gfla.pose_cords(dev(maps), threshold)
    assert got.dtype == torch.int64 and got.is_cuda and torch.equal(got.cpu(), want)
    assert torch.equal(gfla.pose_cords(dev(maps), threshold).cpu(), want)                # and again: the same bits
    for dtype in _lib.HALF_TYPES:
        stored = maps.to(dtype)
        assert torch.equal(gfla.pose_cords(dev(stored), threshold).cpu(), gfla.pose_cords(stored, threshold))
        if torch.equal(stored.float().nan_to_num(), maps.nan_to_num()):                 # representable: the golden holds as it is
            assert torch.equal(gfla.pose_cords(dev(stored), threshold).cpu(), want)


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_pose_cords_ties_across_waves_a_single_element_and_a_large_plane(name):
    dtype = DTYPES[name]
    n = 65537
    maps = torch.zeros(6, 1, 1, n, dtype=dtype)
    maps[0, 0, 0, 300] = maps[0, 0, 0, 40000] = 0.5                   # two waves' ranges: the lower index
    maps[1, 0, 0, 0] = maps[1, 0, 0, n - 1] = 0.5                     # the first and the last element
    maps[2, 0, 0, n - 1] = 0.5                                        # the last element alone
    maps[3, 0, 0, 70] = maps[3, 0, 0, 5] = 0.25
    maps[3, 0, 0, 60000] = 0.5                                        # a later, larger value wins over earlier ties
    maps[4, 0, 0, 1234] = float("nan")
    maps[4, 0, 0, 99] = 0.75
    maps[5, 0, 0, 4097] = 0.0625                                      # below the threshold
    want = [[0, 300], [0, 0], [0, n - 1], [0, 60000], [-1, -1], [-1, -1]]
    assert gfla.pose_cords(dev(maps)).view(6, 2).tolist() == want
    assert gfla.pose_cords(maps).view(6, 2).tolist() == want
    tall = maps.view(6, 1, n, 1)                                      # the same planes as one column
    assert gfla.pose_cords(dev(tall)).view(6, 2).tolist() == [[y, x] if x < 0 else [x, 0] for y, x in want]
    one = torch.tensor([0.5, 0.0625, float("nan"), 0.125], dtype=dtype).view(2, 2, 1, 1)
    assert gfla.pose_cords(dev(one)).tolist() == [[[0, 0], [-1, -1]], [[-1, -1], [0, 0]]]


def test_round_trip_gives_the_truncated_key_points():
    cords = torch.stack([torch.rand(3, 18) * 255.9, torch.rand(3, 18) * 175.9], dim=2).double()
    cords[1, 4] = -1
    for dtype in DTYPES.values():
        got = gfla.pose_cords(gfla.pose_maps(dev(cords), (256, 176), dtype=dtype)).cpu()
        p = torch.stack([(cords[..., 0] / 256) * 256, (cords[..., 1] / 176) * 176], dim=2)
        want = torch.where(cords == -1, cords, torch.trunc(p)).long()
        assert torch.equal(got, want)


# ---- normalize_images -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 3), (2, 5, 7, 3), (1, 3, 5, 1), (1, 4, 6, 4), (1, 40, 30, 2), (2, 256, 176, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_normalize_images_kernel_is_exact(shape):
    g = torch.Generator().manual_seed(sum(shape))
    u8 = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    u8.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)[:u8.numel()]
    for dtype in DTYPES.values():
        for mean, std in ((0.5, 0.5), ((0.485, 0.456, 0.406, 0.4)[:shape[3]], (0.229, 0.224, 0.225, 0.25)[:shape[3]])):
            got = gfla.normalize_images(dev(u8), mean, std, dtype=dtype)
            assert got.shape == (shape[0], shape[3], shape[1], shape[2]) and got.dtype == dtype and got.is_contiguous()
            assert torch.equal(bits(got), bits(gfla.normalize_images(dev(u8), mean, std, dtype=dtype, impl="torch")))
            assert torch.equal(bits(got), bits(gfla.normalize_images(u8, mean, std, dtype=dtype)))


# ---- placement --------------------------------------------------------------------------------------------------------------
def placed_out(shape, dtype, phase):
    """an output buffer full of NaN (0xA5 for integers) at `phase` elements, inside red zones"""
    filler = torch.full(shape, float("nan"), dtype=dtype) if dtype.is_floating_point else torch.full(shape, -6510615555426900571, dtype=dtype)
    view, rec = plu.place(filler, phase, DEV)
    rec.kind = "inout"
    return view, rec


@pytest.mark.parametrize("W", [5, 19, 22])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_pose_maps_at_every_phase_of_its_output(name, W):
    dtype = DTYPES[name]
    cords = torch.tensor([[[3, 2], [-1, 4], [40, W + 3]], [[34, W - 1], [0, 0], [17, 3]]]).to(DEV)     # H = 35: two bands
    want = gfla.pose_maps(cords, (35, W), sigma=1.5, dtype=dtype)
    assert pu.ulp_distance(want, gfla.pose_maps(cords, (35, W), sigma=1.5, dtype=dtype, impl="torch")) <= 1
    for phase in range(16 // dtype.itemsize):
        out, rec = placed_out(want.shape, dtype, phase)
        assert out.data_ptr() % 16 == phase * dtype.itemsize
        gfla.pose_maps(cords, (35, W), sigma=1.5, dtype=dtype, out=out)
        plu.check_zones([rec])
        assert plu.bit_equal(out, want), phase


@pytest.mark.parametrize("W", [5, 19, 22])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_pose_cords_at_every_phase_of_its_pointers(name, W):
    dtype = DTYPES[name]
    cords = torch.tensor([[[3, 2], [-1, 4], [40, W + 3]], [[34, W - 1], [0, 0], [17, 3]]])
    maps = gfla.pose_maps(cords, (35, W), sigma=1.5, dtype=dtype)
    want = gfla.pose_cords(maps)
    assert want.tolist() == [[[3, 2], [-1, -1], [-1, -1]], [[34, W - 1], [0, 0], [17, 3]]]
    for phase in range(16 // dtype.itemsize):
        src, rec_in = plu.place(maps, phase, DEV)
        out, rec_out = placed_out(want.shape, torch.int64, phase % 2)
        assert src.data_ptr() % 16 == phase * dtype.itemsize and out.data_ptr() % 16 == 8 * (phase % 2)
        gfla.pose_cords(src, out=out)
        plu.check_zones([rec_in, rec_out])
        assert torch.equal(out.cpu(), want), phase


@pytest.mark.parametrize("W", [5, 19, 22])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_normalize_images_at_every_phase_of_its_pointers(name, W):
    dtype = DTYPES[name]
    u8 = torch.randint(0, 256, (2, 60, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(W))    # 60 * 19 > 1024 pixels
    want = gfla.normalize_images(u8, dtype=dtype)
    steps = 16 // dtype.itemsize
    for phase in range(16):
        src, rec_in = plu.place(u8, phase, DEV)
        out, rec_out = placed_out(want.shape, dtype, phase % steps)
        assert src.data_ptr() % 16 == phase and out.data_ptr() % 16 == (phase % steps) * dtype.itemsize
        gfla.normalize_images(src, dtype=dtype, out=out)
        plu.check_zones([rec_in, rec_out])
        assert plu.bit_equal(out.cpu(), want), phase


# ---- PoseInputs -------------------------------------------------------------------------------------------------------------
def records(seed, B=2, H=64, W=44, J=18):
    g = torch.Generator().manual_seed(seed)
    images = [torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g) for _ in range(2)]
    cords = [torch.stack([torch.randint(0, 256, (B, J), generator=g), torch.randint(0, 176, (B, J), generator=g)], dim=2)
             for _ in range(2)]
    cords[0][0, 3] = -1
    affine = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1)
    affine[:, 0, 2], affine[:, 1, 2] = 2.3 + seed, -1.7
    return images + cords + [affine, None]


def expected(recs, dtype):
    P1, P2, c1, c2, a1, a2 = recs
    maps = dict(size=(64, 44), old_size=(256, 176), sigma=6.0, dtype=dtype)
    return {"P1": gfla.normalize_images(P1, dtype=dtype), "P2": gfla.normalize_images(P2, dtype=dtype),
            "BP1": gfla.pose_maps(c1, affine=a1, **maps), "BP2": gfla.pose_maps(c2, affine=a2, **maps)}


def check_batch(batch, want, dtype):
    assert sorted(batch) == ["BP1", "BP2", "P1", "P2"]
    for key, t in batch.items():
        assert t.is_cuda and t.dtype == dtype and t.shape == want[key].shape
        if key.startswith("P"):
            assert torch.equal(bits(t), bits(want[key])), key
    for key in ("BP1", "BP2"):
        assert pu.ulp_distance(batch[key], want[key]) <= 1, key          # in ulps of the storage type


@pytest.mark.parametrize("name", ["f32", "f16"])
def test_pose_inputs_from_host_records_without_a_synchronisation(name):
    dtype = DTYPES[name]
    inputs = gfla.PoseInputs((64, 44), old_size=(256, 176), dtype=dtype)
    rounds = [records(seed) for seed in range(4)]
    inputs(*rounds[0])
    inputs(*rounds[1])                                      # both staging sets exist now
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [inputs(*recs) for recs in rounds[2:]]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for batch, recs in zip(got, rounds[2:]):
        check_batch(batch, expected(recs, dtype), dtype)


def test_pose_inputs_captured_in_a_graph_follows_its_key_points():
    inputs = gfla.PoseInputs((64, 44), old_size=(256, 176))
    first, second = ([dev(t) for t in records(seed)[:5]] for seed in (11, 12))
    graphed = GraphedCall(lambda *r: inputs(*r), first)
    batch = graphed(*first)
    check_batch(batch, expected(records(11), torch.float32), torch.float32)
    for static, new in zip(graphed.static_inputs, second):  # overwritten in place, one replay
        static.copy_(new)
    graphed.graph.replay()
    torch.cuda.synchronize()
    check_batch(graphed.static_outputs, expected(records(12), torch.float32), torch.float32)
    assert not torch.equal(bits(graphed.static_outputs["BP1"]), bits(expected(records(11), torch.float32)["BP1"]))
