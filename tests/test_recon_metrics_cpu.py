"""Reconstruction metrics without a GPU (recon_metrics.py, include/gfla_metrics.h): the torch compositions against the
fixture of tests/golden/make_recon_metrics_golden.py -- the reference's pipeline restated with numpy and scipy.ndimage, each
number within 5e-7 -- and against numpy's float32 expression of tensor2im; the accumulator against np.mean / np.var /
round(., 6); the errors; the entry points' argument checks, which are decided before anything is launched."""
import ctypes
import math

import numpy as np
import pytest
import torch

import recon_metrics_util as ru

CASES, SIZES = ru.fixture()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_composition_against_the_fixture(gfla, case):
    got = gfla.torch_reconstruction_metrics(case.pred, case.gt, case.win, case.metrics)
    assert all(v.dtype == torch.float64 and tuple(v.shape) == (case.pred.shape[0],) for v in got.values())
    ru.check(got, case.want, case.name, case.metrics)
    assert gfla.reconstruction_metrics(case.pred, case.gt, case.win, case.metrics).keys() == got.keys()       # the CPU route


def test_fixture_covers_what_it_must():
    """windows 3, 7, 51 and the Gaussian 11, one window and one pixel more, both sides of a strip and of a band (the sizes
    the fixture was made for are checked against the kernels' on the GPU), C = 1, 3, 4, B = 1, 3, the workload's shape"""
    shapes = {(c.win,) + tuple(c.pred.shape) for c in CASES}
    T, band = SIZES["threads"], SIZES["band"]
    assert {s[0] for s in shapes} == {3, 7, 51} and {s[4] for s in shapes} == {1, 3, 4} and {s[1] for s in shapes} == {1, 3}
    for win in (3, 7, 51, 11):
        assert any(s[2] == s[3] == win and (s[0] == win or win == 11) for s in shapes), win
        assert any(s[2] == s[3] == win + 1 and (s[0] == win or win == 11) for s in shapes), win
    assert {s[3] for s in shapes if s[0] in (3, 7)} >= {T - 1, T + 1}
    assert {s[2] - 6 for s in shapes if s[0] == 7} >= {band - 1, band + 1} and {s[2] - 10 for s in shapes} >= {band - 1, band + 1}
    assert (51, 1, 256, 176, 3) in shapes


def test_images_to_uint8_composition_is_numpys_float32_expression(gfla):
    x = ru.boundary_inputs()
    t, want, inside = ru.numpy_tensor2im(x)
    assert inside.sum() > 1200 and (~inside).sum() >= 8
    maps = torch.from_numpy(x).view(1, 1, 1, -1)
    got = gfla.torch_images_to_uint8(maps).view(-1).numpy()
    assert np.array_equal(got[inside], want[inside])                  # bit for bit where numpy's cast is defined
    assert np.array_equal(got, ru.expected_bytes(x))                  # saturation and NaN -> 0 elsewhere
    # every whole number is reached from both sides: the inputs do straddle the crossings
    near = want[:5 * 257].reshape(257, 5)
    assert all(list(near[v]) == [v - 1, v - 1, v, v, v] for v in range(1, 256))
    assert torch.equal(gfla.images_to_uint8(maps), gfla.torch_images_to_uint8(maps))
    # layout: (B, C, H, W) -> (B, H, W, C); another scale
    y = torch.rand(2, 3, 5, 7) * 2 - 1
    want = ((y.numpy().transpose(0, 2, 3, 1) + 1) / 2.0 * 200.0).astype(np.uint8)
    assert np.array_equal(gfla.images_to_uint8(y, bytes=200.0).numpy(), want)
    for dtype in (torch.float16, torch.bfloat16):                     # widened first, as .float() does
        assert torch.equal(gfla.images_to_uint8(y.to(dtype)), gfla.images_to_uint8(y.to(dtype).float()))
    with pytest.raises(TypeError):
        gfla.images_to_uint8(y.double())
    with pytest.raises(ValueError):
        gfla.images_to_uint8(y[0])


def _record(values):
    want = {}
    with np.errstate(all="ignore"):
        for name in ("psnr", "ssim", "ssim_256", "mae", "l1"):
            want[name] = round(np.mean(values[name]), 6)
            want[name + "_variance"] = round(np.var(values[name]), 6)
    return want


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def test_accumulator_against_numpy(gfla):
    case = next(c for c in CASES if c.name == "plus_one_gauss")       # B = 3, every metric
    more = next(c for c in CASES if c.name == "band_plus_gauss")
    scores = gfla.ReconstructionMetrics(win_size=3)
    with pytest.raises(ValueError):
        scores.compute()
    scores.update(more.pred, more.gt)
    record = scores.compute()
    assert list(record) == ["psnr", "psnr_variance", "ssim", "ssim_variance", "ssim_256", "ssim_256_variance", "mae", "mae_variance",
                            "l1", "l1_variance"]
    assert all(type(v) is float for v in record.values())
    want = _record(more.want)
    for name, v in record.items():
        assert abs(v - want[name]) <= 1.5e-6, (name, v, want[name])   # a unit of the sixth decimal: both sides are rounded
    # one update against three: the same bits
    whole, parts = gfla.ReconstructionMetrics(win_size=7), gfla.ReconstructionMetrics(win_size=7)
    whole.update(case.pred, case.gt)
    for b in range(3):
        parts.update(case.pred[b:b + 1], case.gt[b:b + 1])
    for name in ru.METRICS:
        assert torch.equal(whole.per_image()[name], parts.per_image()[name]), name
    assert whole.compute() == parts.compute()
    ru.check(whole.per_image(), case.want, "accumulated " + case.name)
    # a pair of equal images among them: PSNR +inf, its mean +inf and its variance NaN, as numpy gives
    whole.update(case.gt[:1], case.gt[:1])
    values = {k: v.numpy() for k, v in whole.per_image().items()}
    assert values["psnr"][3] == np.inf and values["l1"][3] == 0 and abs(values["ssim"][3] - 1) <= ru.BAR
    record, want = whole.compute(), _record(values)
    assert record["psnr"] == np.inf and math.isnan(record["psnr_variance"])
    assert all(_same(record[k], float(want[k])) for k in want)
    whole.reset()
    with pytest.raises(ValueError):
        whole.per_image()


def test_closed_forms_of_the_composition(gfla):
    black = torch.zeros(1, 12, 12, 3, dtype=torch.uint8)
    got = gfla.torch_reconstruction_metrics(black, black, 3)
    assert math.isnan(got["mae"].item()) and got["psnr"].item() == np.inf and got["l1"].item() == 0
    p, q = 200, 90
    got = gfla.torch_reconstruction_metrics(torch.full_like(black, p), torch.full_like(black, q), 7, ("ssim",))
    a, b, C1 = np.float32(q) / np.float32(255), np.float32(p) / np.float32(255), 0.01 ** 2
    want = (2 * float(a) * float(b) + C1) / (float(a) ** 2 + float(b) ** 2 + C1)
    assert abs(got["ssim"].item() - want) <= ru.BAR


@pytest.mark.parametrize("win,H,W", [(7, 12, 11), (51, 64, 60)])
def test_a_wrong_window_is_far_beyond_the_bar(gfla, win, H, W):
    """The images of the GPU test of the window's extent: the exact-integer SSIM in numpy agrees with the composition, and
    with its window started one place late or made one place short it is more than 100 bars away on every image."""
    pred, gt, places = ru.changed_byte_batch(H, W)
    want = gfla.torch_reconstruction_metrics(torch.from_numpy(pred), torch.from_numpy(gt), win, ("ssim",))["ssim"]
    for i, place in enumerate(places):
        assert abs(ru.ssim_uniform_numpy(pred[i], gt[i], win) - want[i].item()) <= ru.BAR / 10
        late = ru.ssim_uniform_numpy(pred[i], gt[i], win, start=1)
        short = ru.ssim_uniform_numpy(pred[i], gt[i], win, length=win - 1)
        print("window %d, byte changed at %s: ssim %.9f, started late %.9f, one short %.9f" % (win, place, want[i].item(), late, short))
        assert abs(late - want[i].item()) > 100 * ru.BAR and abs(short - want[i].item()) > 100 * ru.BAR, place


def test_errors(gfla):
    u8 = torch.zeros(1, 12, 12, 3, dtype=torch.uint8)
    for fn in (gfla.reconstruction_metrics, gfla.torch_reconstruction_metrics):
        with pytest.raises(ValueError, match="win_size"):
            fn(u8, u8, win_size=4)
        with pytest.raises(ValueError, match="win_size"):
            fn(u8, u8, win_size=257)
        with pytest.raises(ValueError, match="window"):
            fn(u8, u8, win_size=13)                                   # the image is smaller than the window
        with pytest.raises(ValueError, match="window"):
            fn(u8[:, :10], u8[:, :10], win_size=3)                    # ... than the Gaussian one
        assert set(fn(u8[:, :10], u8[:, :10], 3, ("ssim", "psnr"))) == {"ssim", "psnr"}     # which nobody asked for here
        with pytest.raises(ValueError):
            fn(u8, u8[:, :11], 3)
        with pytest.raises(ValueError):
            fn(u8, u8, 3, ("ssim", "fid"))
        with pytest.raises(TypeError):
            fn(u8.to(torch.int32), u8, 3)
    with pytest.raises(ValueError):
        gfla.reconstruction_metrics(u8, u8, 3, impl="numpy")
    # float maps go through images_to_uint8 first
    x = torch.rand(2, 3, 12, 12) * 2 - 1
    y = torch.rand(2, 3, 12, 12) * 2 - 1
    got = gfla.reconstruction_metrics(x, y, 3)
    want = gfla.reconstruction_metrics(gfla.images_to_uint8(x), gfla.images_to_uint8(y), 3)
    assert all(torch.equal(got[k], want[k]) for k in want)


def test_entry_points_and_their_argument_checks(gfla):
    from global_flow_local_attention_amd import _lib, recon_metrics
    names = {"gfla_images_to_uint8_f32", "gfla_images_to_uint8_f16", "gfla_images_to_uint8_bf16", "gfla_recon_metrics",
             "gfla_recon_metrics_workspace_bytes", "gfla_recon_metrics_geometry"}
    assert names <= set(_lib.extension_symbols()) and not names & set(_lib.exported_symbols())
    assert any(p.endswith("gfla_metrics.h") for p in _lib.EXTENSION_HEADER_PATHS) and _lib.ABI_VERSION == 8
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p, n = ctypes.cast(buf, ctypes.c_void_p), None
    assert L.gfla_recon_metrics(n, p, p, p, 1, 12, 12, 3, 3, 7, p, n) == -1
    assert L.gfla_recon_metrics(p, p, p, p, 1, 12, 12, 3, 3, 2, n, n) == -1             # Gaussian window without taps
    assert L.gfla_recon_metrics(p, p, p, p, 1, 12, 12, 3, 4, 7, p, n) == -2             # even window: the bad-shape code
    assert L.gfla_recon_metrics(p, p, p, p, 1, 12, 12, 3, 13, 7, p, n) == -2            # image smaller than the window
    assert L.gfla_recon_metrics(p, p, p, p, 1, 10, 12, 3, 3, 7, p, n) == -2             # ... than the Gaussian one
    assert L.gfla_recon_metrics(p, p, p, p, 1, 12, 12, 5, 3, 7, p, n) == -2
    assert L.gfla_recon_metrics(p, p, p, p, 1, 12, 12, 3, 3, 0, p, n) == -2
    assert L.gfla_recon_metrics(p, p, p, p, 1, 40000, 12, 3, 3, 7, p, n) == _lib._ERR_UNSUPPORTED
    assert L.gfla_recon_metrics(p, p, p, p, 70000, 12, 12, 3, 3, 7, p, n) == _lib._ERR_UNSUPPORTED
    assert L.gfla_recon_metrics_workspace_bytes(1, 12, 12, 3, 4, 7) == -2
    assert L.gfla_recon_metrics_workspace_bytes(1, 10, 12, 3, 3, 5) > 0                 # no Gaussian window asked for
    assert L.gfla_images_to_uint8_f32(n, p, 1, 3, 4, 4, 255.0, n) == -1
    assert L.gfla_images_to_uint8_f32(p, p, 1, 0, 4, 4, 255.0, n) == -2
    assert L.gfla_images_to_uint8_f32(p, p, 1, 3, 4, 4, float("inf"), n) == -2
    assert L.gfla_images_to_uint8_f16(p, p, 1, 5, 4, 4, 255.0, n) == _lib._ERR_UNSUPPORTED
    # the workspace: 4 doubles per pixel-sum workgroup and one per SSIM workgroup
    g = recon_metrics.kernel_geometry(51)
    assert g["strip"] == SIZES["threads"] - 50 and g["band"] == SIZES["band"] and g["gauss_strip"] == SIZES["threads"] - 10
    assert recon_metrics.kernel_geometry(255)["strip"] >= 256
    B, H, W, C = 2, 256, 176, 3
    pieces = -(-H * W * C // g["pixel_piece"])
    bands = lambda win: -(-(H - win + 1) // g["band"])                                   # noqa: E731
    assert L.gfla_recon_metrics_workspace_bytes(B, H, W, C, 51, 7) == 8 * B * (4 * pieces + C * (bands(51) + bands(11)))


def test_taps_are_scipys():
    from global_flow_local_attention_amd import recon_metrics
    gaussian_filter = pytest.importorskip("scipy.ndimage").gaussian_filter
    delta = np.zeros(21)
    delta[10] = 1
    assert np.allclose(recon_metrics.gaussian_taps(), gaussian_filter(delta, sigma=1.5, truncate=3.5)[5:16], rtol=0, atol=1e-16)
