"""Reconstruction metrics on the GPU (csrc/recon_metrics.hip): the kernels against the fixture of
tests/golden/make_recon_metrics_golden.py (the reference's pipeline, restated on the host) at 5e-7 per number, closed forms,
the extent of the window, independence of the batch and repeatability bit for bit, every byte phase of the pointers inside
red zones, images_to_uint8 against the composition byte for byte, and a profile without copies or synchronisation.
Nothing here reads the reference or needs scipy; tests/test_recon_metrics_cpu.py pins the composition to both."""
import math

import numpy as np
import pytest
import torch

import placement_util as pu
import recon_metrics_util as ru

pytestmark = pytest.mark.gpu
CASES, SIZES = ru.fixture()
DEV = "cuda"


def bits(t):
    return t.view(torch.int64)


def same_bits(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in a) and a.keys() == b.keys()


def test_fixture_was_made_for_these_kernels():
    """the fixture's strip and band cases bracket the tile sizes it was made for: the kernels' own"""
    from global_flow_local_attention_amd import recon_metrics
    for win in (3, 7, 51):
        g = recon_metrics.kernel_geometry(win)
        assert g["strip"] == SIZES["threads"] - (win - 1) and g["band"] == g["gauss_band"] == SIZES["band"], (
            "regenerate tests/golden/recon_metrics.npz with --threads / --band of csrc/recon_metrics.hip", g, SIZES)
        assert g["gauss_strip"] == SIZES["threads"] - 10


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_kernels_against_the_fixture(gfla, case):
    got = gfla.reconstruction_metrics(case.pred.to(DEV), case.gt.to(DEV), case.win, case.metrics)
    assert all(v.dtype == torch.float64 and v.is_cuda and tuple(v.shape) == (case.pred.shape[0],) for v in got.values())
    worst = ru.check(got, case.want, case.name, case.metrics)
    print("%s: largest distance from the fixture %.2e" % (case.name, worst))


def test_more_pieces_than_pixel_workgroups_and_a_wide_window(gfla):
    """an image of more than 64 pieces of 16 KB (a pixel-sum workgroup then walks several) and a window above 129 (1024
    threads per strip), against the composition on the device"""
    g = torch.Generator().manual_seed(5)
    gt = torch.randint(0, 256, (1, 600, 620, 3), dtype=torch.uint8, generator=g)
    pred = (gt.to(torch.int32) + torch.randint(-20, 21, gt.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    got = gfla.reconstruction_metrics(pred.to(DEV), gt.to(DEV), 3, ("psnr", "l1", "mae", "ssim_256"))
    want = gfla.torch_reconstruction_metrics(pred.to(DEV), gt.to(DEV), 3, ("psnr", "l1", "mae", "ssim_256"))
    ru.check(got, {k: v.cpu().numpy() for k, v in want.items()}, "600x620x3", tuple(want))
    small_p, small_g = pred[:, :140, :900 // 3].contiguous(), gt[:, :140, :900 // 3].contiguous()
    got = gfla.reconstruction_metrics(small_p.to(DEV), small_g.to(DEV), 131, ("ssim",))
    want = gfla.torch_reconstruction_metrics(small_p, small_g, 131, ("ssim",))
    ru.check(got, {k: v.numpy() for k, v in want.items()}, "140x300x3 window 131", ("ssim",))


# ---- closed forms ------------------------------------------------------------------------------------------------------------
def constant(value, shape=(1, 14, 13, 3)):
    return torch.full(shape, value, dtype=torch.uint8, device=DEV)


def test_equal_images(gfla):
    case = next(c for c in CASES if c.name == "plus_one_gauss")
    gt = case.gt.to(DEV)
    got = {k: v.cpu() for k, v in gfla.reconstruction_metrics(gt, gt.clone(), 7).items()}
    for b in range(gt.shape[0]):
        assert abs(got["ssim"][b].item() - 1) <= ru.BAR and abs(got["ssim_256"][b].item() - 1) <= ru.BAR
        assert got["psnr"][b].item() == math.inf and got["l1"][b].item() == 0 and got["mae"][b].item() == 0


@pytest.mark.parametrize("p,q", [(200, 90), (1, 255), (17, 16), (128, 127)])
def test_two_constants(gfla, p, q):
    """ssim = (2 p q + C1) / (p^2 + q^2 + C1) on the 0..1 scale; the prediction's range is 0, so ssim_256 has C1 = C2 = 0 and
    is whatever IEEE makes of the formula in include/gfla_metrics.h's order: the composition evaluates the same operations
    in the same order, and the two agree in kind (NaN, an infinity) or, where finite, within the bar.  128 against 127 is the
    pair whose psnr integer sums of x - y would miss by 6.5e-5: the kernel sums the reference's own float32(v) / 255."""
    got = {k: v.cpu() for k, v in gfla.reconstruction_metrics(constant(p), constant(q), 7).items()}
    a, b, C1 = q / 255.0, p / 255.0, 0.01 ** 2
    assert abs(got["ssim"].item() - (2 * a * b + C1) / (a * a + b * b + C1)) <= ru.BAR
    want = gfla.torch_reconstruction_metrics(constant(p).cpu(), constant(q).cpu(), 7)
    print("constants %d, %d: ssim_256 %r on the kernels, %r by the composition" % (p, q, got["ssim_256"].item(), want["ssim_256"].item()))
    ru.check(got, {k: v.numpy() for k, v in want.items()}, "constants %d %d" % (p, q))


def test_largest_sums_and_black_images(gfla):
    """all 0 against all 255 at window 51: every window sum at its largest (255^2 * 51^2 needs 28 bits, N Sxx 40)"""
    shape = (1, 53, 52, 4)
    got = {k: v.cpu() for k, v in gfla.reconstruction_metrics(constant(0, shape), constant(255, shape), 51).items()}
    C1 = 0.01 ** 2
    assert abs(got["ssim"].item() - C1 / (1 + C1)) <= ru.BAR
    assert got["psnr"].item() == 0 and got["l1"].item() == 1 and got["mae"].item() == 1
    got = {k: v.cpu() for k, v in gfla.reconstruction_metrics(constant(255, shape), constant(255, shape), 51).items()}
    assert abs(got["ssim"].item() - 1) <= ru.BAR and got["psnr"].item() == math.inf and got["mae"].item() == 0
    got = {k: v.cpu() for k, v in gfla.reconstruction_metrics(constant(0), constant(0), 3).items()}
    assert math.isnan(got["mae"].item()) and got["psnr"].item() == math.inf and got["l1"].item() == 0
    assert abs(got["ssim"].item() - 1) <= ru.BAR


# ---- the extent of the window ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win,H,W", [(7, 12, 11), (51, 64, 60)])
def test_window_extent(gfla, win, H, W):
    """One byte of the prediction moved by 100 at each corner, on each edge and in the middle of a smooth pair: a window
    that starts one place late, or is one place short, misses or misweighs it.  tests/test_recon_metrics_cpu.py shows with
    the same images and a deliberately shifted or shortened window that such a mistake moves ssim by more than 100 bars;
    here every image is within one bar of the exact-integer value and of the composition."""
    pred, gt, places = ru.changed_byte_batch(H, W)
    got = {k: v.cpu() for k, v in gfla.reconstruction_metrics(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), win).items()}
    want = gfla.torch_reconstruction_metrics(torch.from_numpy(pred), torch.from_numpy(gt), win)
    ru.check(got, {k: v.numpy() for k, v in want.items()}, "changed byte, window %d" % win)
    for i, place in enumerate(places):
        exact = ru.ssim_uniform_numpy(pred[i], gt[i], win)
        assert abs(got["ssim"][i].item() - exact) <= ru.BAR, (place, got["ssim"][i].item(), exact)


# ---- independence and repeatability --------------------------------------------------------------------------------------------
def test_batch_independence_and_repeatability(gfla):
    case = next(c for c in CASES if c.name == "band_plus_gauss")      # 43 x 12 x 3: two bands
    g = torch.Generator().manual_seed(3)
    pred = torch.randint(0, 256, (5,) + tuple(case.pred.shape[1:]), dtype=torch.uint8, generator=g)
    gt = torch.randint(0, 256, pred.shape, dtype=torch.uint8, generator=g)
    pred[1], gt[1] = case.pred[0], case.gt[0]
    pred, gt = pred.to(DEV), gt.to(DEV)
    whole = gfla.reconstruction_metrics(pred, gt, 7)
    assert same_bits(whole, gfla.reconstruction_metrics(pred, gt, 7))                    # two calls, equal bits
    alone = gfla.reconstruction_metrics(pred[1:2].contiguous(), gt[1:2].contiguous(), 7)
    for at in (0, 2, 4):                                                                 # first, middle, last
        order = [i for i in range(5) if i != 1]
        order.insert(at, 1)
        moved = gfla.reconstruction_metrics(pred[order].contiguous(), gt[order].contiguous(), 7)
        assert all(torch.equal(bits(moved[k][at:at + 1]), bits(alone[k])) for k in alone), at
    one, three = gfla.ReconstructionMetrics(7), gfla.ReconstructionMetrics(7)
    one.update(pred, gt)
    for lo, hi in ((0, 2), (2, 3), (3, 5)):
        three.update(pred[lo:hi].contiguous(), gt[lo:hi].contiguous())
    assert same_bits(one.per_image(), three.per_image()) and same_bits(one.per_image(), whole)
    assert one.compute() == three.compute()


def test_float_maps_go_through_images_to_uint8(gfla):
    g = torch.Generator().manual_seed(9)
    x, y = (torch.rand(2, 3, 16, 15, generator=g) * 2 - 1 for _ in range(2))
    got = gfla.reconstruction_metrics(x.to(DEV).half(), y.to(DEV), 5)
    want = gfla.reconstruction_metrics(gfla.images_to_uint8(x.to(DEV).half()), gfla.images_to_uint8(y.to(DEV)), 5)
    assert same_bits(got, want)
    ru.check(got, {k: v.numpy() for k, v in gfla.reconstruction_metrics(x.half(), y, 5).items()}, "float maps")


def test_captured_in_a_graph(gfla):
    from global_flow_local_attention_amd import GraphedCall
    first, second = (next(c for c in CASES if c.name == n) for n in ("band_minus_7", "band_plus_7"))
    shape = (1, 37, 13, 3)
    crop = lambda c: [t[:, :shape[1], :shape[2], :shape[3]].contiguous().to(DEV) for t in (c.pred, c.gt)]   # noqa: E731
    graphed = GraphedCall(lambda p, g: gfla.reconstruction_metrics(p, g, 7), crop(first))
    out = graphed(*crop(first))
    assert same_bits({k: v.clone() for k, v in out.items()}, gfla.reconstruction_metrics(*crop(first), 7))
    for static, new in zip(graphed.static_inputs, crop(second)):      # overwritten in place, one replay
        static.copy_(new)
    graphed.graph.replay()
    torch.cuda.synchronize()
    assert same_bits(graphed.static_outputs, gfla.reconstruction_metrics(*crop(second), 7))


# ---- placement ---------------------------------------------------------------------------------------------------------------
def test_every_byte_phase_inside_red_zones(gfla):
    """Both ops with their byte pointers at each of the 16 phases of a 16-byte line (pred and gt at different ones), the
    float map at each element phase, every buffer between red zones -- the inputs, the outputs and, through the placing
    mode, the output and the workspace the wrapper allocates: equal bits at every phase, nothing outside written."""
    case = next(c for c in CASES if c.name == "band_plus_gauss")
    pred, gt = case.pred, case.gt
    aligned = gfla.reconstruction_metrics(pred.to(DEV), gt.to(DEV), 7)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 3, 9, 23, generator=g) * 2 - 1
    want_bytes = gfla.torch_images_to_uint8(x)
    for phase in range(16):
        records = []
        p, rec = pu.place(pred, phase, DEV)
        records.append(rec)
        q, rec = pu.place(gt, (5 * phase + 3) % 16, DEV)
        records.append(rec)
        mode = pu.Placing(pu.Placement("uniform1", 0))
        with mode:
            got = gfla.reconstruction_metrics(p, q, 7)
        assert len(mode.records) >= 2, "the placing mode saw the output and the workspace"
        assert same_bits(got, aligned), phase
        src, rec = pu.place(x, phase % 4, DEV)
        records.append(rec)
        dst, rec = pu.place(torch.zeros(want_bytes.shape, dtype=torch.uint8), phase, DEV)
        rec.kind = "inout"
        records.append(rec)
        gfla.images_to_uint8(src, out=dst)
        assert torch.equal(dst.cpu(), want_bytes), phase
        torch.cuda.synchronize()
        pu.check_zones(records + mode.records)


# ---- images_to_uint8 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_images_to_uint8_against_the_composition(gfla, dtype):
    x = torch.from_numpy(ru.boundary_inputs()).to(dtype)
    maps = x.view(1, 1, 1, -1)
    got = gfla.images_to_uint8(maps.to(DEV))
    assert got.dtype == torch.uint8 and got.shape == (1, 1, x.numel(), 1)
    assert torch.equal(got.cpu(), gfla.torch_images_to_uint8(maps))
    if dtype == torch.float32:
        assert np.array_equal(got.cpu().view(-1).numpy(), ru.expected_bytes(x.numpy()))
    g = torch.Generator().manual_seed(4)
    # one element; an odd small one; rows of 3 * 37 = 111 bytes, no multiple of the 16-byte store; more than one workgroup
    for shape in ((1, 1, 1, 1), (2, 3, 5, 7), (2, 3, 4, 37), (1, 4, 33, 35), (3, 2, 40, 41)):
        y = (torch.rand(shape, generator=g) * 2.2 - 1.1).to(dtype)
        for scale in (255.0, 200.0):
            assert torch.equal(gfla.images_to_uint8(y.to(DEV), bytes=scale).cpu(), gfla.torch_images_to_uint8(y, scale)), (shape, scale)
        assert torch.equal(gfla.images_to_uint8(y.to(DEV), impl="torch").cpu(), gfla.torch_images_to_uint8(y))


# ---- no host traffic ---------------------------------------------------------------------------------------------------------
def test_steady_state_call_is_kernels_only(gfla):
    from torch.profiler import ProfilerActivity, profile, record_function
    case = next(c for c in CASES if c.name == "plus_one_gauss")
    pred, gt = case.pred.to(DEV), case.gt.to(DEV)
    maps = torch.rand(2, 3, 16, 16, device=DEV)
    for _ in range(2):
        gfla.reconstruction_metrics(pred, gt, 7)
        gfla.images_to_uint8(maps)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with record_function("the_two_calls"):
            gfla.reconstruction_metrics(pred, gt, 7)
            gfla.images_to_uint8(maps)
        torch.cuda.synchronize()
    events = list(prof.events())
    device = [e.name for e in events if e.device_type == torch.autograd.DeviceType.CUDA and e.name != "the_two_calls"]
    span = next(e for e in events if e.name == "the_two_calls" and e.device_type != torch.autograd.DeviceType.CUDA).time_range
    host = [e.name for e in events if e.device_type != torch.autograd.DeviceType.CUDA
            and e.name != "the_two_calls" and span.start <= e.time_range.start and e.time_range.end <= span.end]
    print("device events: %s\nhost events inside the calls: %s" % (device, sorted(set(host))))
    kernels = ("pixel_sums_kernel", "ssim_uniform_kernel", "ssim_gauss_kernel", "metrics_finish_kernel", "images_to_uint8_kernel")
    assert len(device) == 5 and all(any(k in name for name in device) for k in kernels)
    assert any("LaunchKernel" in n for n in host), "the profile shows the host side of the calls"
    assert not [n for n in device + host if "memcpy" in n.lower() or "memset" in n.lower() or "synchronize" in n.lower()]
