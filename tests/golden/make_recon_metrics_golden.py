#!/usr/bin/env python3
"""Golden values for reconstruction_metrics: the reference's pipeline (script/metrics.py:322-344 on the skimage it was
written against) restated with numpy and scipy.ndimage for a list of small byte image pairs.

Per pair: float32(byte) / 255; psnr, l1 and mae as float64 formulas of those; ssim through uniform_filter on the float64
copies, sample covariance, data range 1; ssim_256 through gaussian_filter(sigma 1.5, truncate 3.5) on float32(a * 255),
population covariance, data range max - min of the prediction; the crop by (win_size - 1) / 2; the mean over channels.

The maker anchors itself.  Both SSIMs are computed again by brute force from exact integer window sums (numpy int64
cumulative sums, no filter; for the Gaussian window the integer moments weighed with the outer product of the taps), and
    exact_vs_filter   |integer route - filter route on v / 255.0 in float64| (for ssim_256: on the same integers)
    float32_shift     |filter route on float32(v) / 255 - filter route on v / 255.0|: what the reference's own rounding moves
are stored per case and asserted below: the first within 1e-12, the second within 5e-8, a tenth of the tests' bar.

The sizes that bracket the kernels' tiles are arguments: --threads (input columns per strip; a strip of the uniform window
has threads - (win_size - 1) output columns), --band (output rows per band), defaults = csrc/recon_metrics.hip's.
    python tests/golden/make_recon_metrics_golden.py [--threads 256] [--band 32]
"""
import argparse
import os

import numpy as np
from scipy.ndimage import gaussian_filter, uniform_filter

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--threads", type=int, default=256)
ap.add_argument("--band", type=int, default=32)
args = ap.parse_args()
rng = np.random.RandomState(20261021)
K1, K2, GAUSS = 0.01, 0.03, 11


def pair(B, H, W, C, change=24):
    """structured images: a ramp, a wave and noise; the prediction is the ground truth blurred a little, shifted and noisy"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    gts, preds = [], []
    for _ in range(B):
        planes = []
        for c in range(C):
            f = rng.uniform(0.05, 0.6, 2)
            base = 128 + 70 * np.sin(f[0] * x + c) * np.cos(f[1] * y) + 40 * (x / max(W - 1, 1) - 0.5) + rng.normal(0, 12, (H, W))
            planes.append(base)
        gt = np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)
        pred = np.clip(gt.astype(np.float64) * rng.uniform(0.8, 1.0) + rng.normal(4, change, gt.shape), 0, 255).astype(np.uint8)
        gts.append(gt)
        preds.append(pred)
    return np.stack(preds), np.stack(gts)


def ssim_from_moments(ux, uy, uxx, uyy, uxy, cov_norm, C1, C2):
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    return (A1 * A2) / (B1 * B2)


def ssim_filter(X, Y, win, gaussian, data_range):
    """compare_ssim(X, Y, multichannel=True, ...) of (H, W, C) arrays, which it converts to float64 first"""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    if gaussian:
        filt, cov_norm, pad = (lambda a: gaussian_filter(a, sigma=1.5, truncate=3.5)), 1.0, (GAUSS - 1) // 2
    else:
        filt, cov_norm, pad = (lambda a: uniform_filter(a, size=win)), win * win / (win * win - 1.0), (win - 1) // 2
    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    means = []
    for c in range(X.shape[2]):
        x, y = X[..., c], Y[..., c]
        S = ssim_from_moments(filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y), cov_norm, C1, C2)
        means.append(S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean())
    return np.mean(means)


def window_sums(v, win):
    """exact sums of an int64 (H, W) array over every win x win window inside it, from its integral image"""
    I = np.zeros((v.shape[0] + 1, v.shape[1] + 1), np.int64)
    I[1:, 1:] = v.cumsum(0).cumsum(1)
    return I[win:, win:] - I[:-win, win:] - I[win:, :-win] + I[:-win, :-win]


def ssim_exact_uniform(X, Y, win):
    """bytes -> ssim on the 0..1 scale, every window sum an exact integer"""
    N = win * win
    means = []
    for c in range(X.shape[2]):
        x, y = X[..., c].astype(np.int64), Y[..., c].astype(np.int64)
        sx, sy, sxx, syy, sxy = (window_sums(v, win).astype(np.float64) for v in (x, y, x * x, y * y, x * y))
        S = ssim_from_moments(sx / N / 255.0, sy / N / 255.0, sxx / N / 255.0 ** 2, syy / N / 255.0 ** 2, sxy / N / 255.0 ** 2,
                              N / (N - 1.0), K1 ** 2, K2 ** 2)
        means.append(S.mean())
    return np.mean(means)


def gaussian_taps():
    x = np.arange(-5, 6)
    phi = np.exp(-0.5 / (1.5 * 1.5) * x ** 2)
    return phi / phi.sum()


def ssim_exact_gauss(X, Y, data_range):
    window = np.outer(gaussian_taps(), gaussian_taps())
    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    means = []
    for c in range(X.shape[2]):
        x, y = X[..., c].astype(np.int64), Y[..., c].astype(np.int64)
        u = [np.tensordot(np.lib.stride_tricks.sliding_window_view(v.astype(np.float64), (GAUSS, GAUSS)), window, 2)
             for v in (x, y, x * x, y * y, x * y)]
        means.append(ssim_from_moments(*u, 1.0, C1, C2).mean())
    return np.mean(means)


store, names = {}, []


def add(name, win, B, H, W, C, change=24):
    pred, gt = pair(B, H, W, C, change)
    rows = {k: [] for k in ("ssim", "ssim_256", "psnr", "l1", "mae", "exact_vs_filter", "float32_shift",
                            "exact_vs_filter_256")}
    for b in range(B):
        img_gt, img_pred = gt[b].astype(np.float32) / 255.0, pred[b].astype(np.float32) / 255.0      # metrics.py:322-323
        assert img_gt.dtype == np.float32
        a, p = img_gt.astype(np.float64), img_pred.astype(np.float64)
        mse = np.mean((a - p) ** 2)
        with np.errstate(divide="ignore"):
            rows["psnr"].append(10 * np.log10(1.0 / mse))
        rows["l1"].append(np.mean(np.abs(a - p)))
        rows["mae"].append(np.sum(np.abs(a - p)) / np.sum(a + p))
        ssim = ssim_filter(img_gt, img_pred, win, False, 1)
        on_doubles = ssim_filter(gt[b] / 255.0, pred[b] / 255.0, win, False, 1)
        rows["ssim"].append(ssim)
        rows["exact_vs_filter"].append(abs(ssim_exact_uniform(gt[b], pred[b], win) - on_doubles))
        rows["float32_shift"].append(abs(ssim - on_doubles))
        if min(H, W) >= GAUSS:
            gt256, pred256 = img_gt * 255.0, img_pred * 255.0                                        # metrics.py:340-341
            assert gt256.dtype == np.float32 and np.array_equal(gt256, gt[b]) and np.array_equal(pred256, pred[b])
            # a float32 scalar; the numpy of the reference's day multiplied it with K1 in float64, today's would in float32
            R = float(pred256.max() - pred256.min())
            assert R > 0
            ssim256 = ssim_filter(gt256, pred256, None, True, R)
            rows["ssim_256"].append(ssim256)
            rows["exact_vs_filter_256"].append(abs(ssim_exact_gauss(gt[b], pred[b], R) - ssim256))
        else:
            rows["ssim_256"].append(np.nan)                                                          # no such window: not asked for
            rows["exact_vs_filter_256"].append(0.0)
    assert max(rows["exact_vs_filter"]) <= 1e-12 and max(rows["exact_vs_filter_256"]) <= 1e-12, (name, rows)
    assert max(rows["float32_shift"]) <= 5e-8, (name, rows)
    store[name + "/pred"], store[name + "/gt"], store[name + "/win"] = pred, gt, np.array(win)
    for k, v in rows.items():
        store[name + "/" + k] = np.array(v, np.float64)
    names.append(name)
    print("%-22s win %2d  %s x %d: ssim %.6f ssim_256 %.6f psnr %.4f | exact vs filter %.1e (256: %.1e), float32 shift %.1e"
          % (name, win, "x".join(map(str, (H, W, C))), B, rows["ssim"][0], rows["ssim_256"][0], rows["psnr"][0],
             max(rows["exact_vs_filter"]), max(rows["exact_vs_filter_256"]), max(rows["float32_shift"])))


T, BAND = args.threads, args.band
# one window, and one pixel more in each direction; every channel count; batches of 1 and 3
add("one_window_3", 3, 1, 3, 3, 1)
add("plus_one_3", 3, 3, 4, 4, 3)
add("one_window_7", 7, 1, 7, 7, 4)
add("plus_one_7", 7, 1, 8, 8, 1)
add("one_window_gauss", 3, 1, 11, 11, 1)
add("plus_one_gauss", 7, 3, 12, 12, 4)
add("one_window_51", 51, 1, 51, 51, 1)
add("plus_one_51", 51, 1, 52, 52, 3)
add("anchor_64x56_7", 7, 1, 64, 56, 3)
add("anchor_64x56_51", 51, 1, 64, 56, 3)
# a strip's input extent is T columns: one narrower (every window's strip is one column short of full) and one wider (a
# second strip of one column, at win 3, 7 and the Gaussian 11 alike)
add("strip_minus_3", 3, 1, 12, T - 1, 1)
add("strip_plus_3", 3, 1, 12, T + 1, 3)
add("strip_minus_7", 7, 1, 12, T - 1, 3)
add("strip_plus_7", 7, 3, 12, T + 1, 1)
# a band is BAND output rows: one short and one more, for the uniform window (win 7) and for the Gaussian one
add("band_minus_7", 7, 1, BAND + 6 - 1, 14, 3)
add("band_plus_7", 7, 1, BAND + 6 + 1, 13, 4)
add("band_minus_gauss", 3, 1, BAND + 10 - 1, 13, 1)
add("band_plus_gauss", 3, 3, BAND + 10 + 1, 12, 3)
add("near_equal", 7, 1, 20, 18, 3, change=0.6)
# the workload's own shape, once
add("workload_256x176", 51, 1, 256, 176, 3)
store["names"] = np.array(names)
store["threads"], store["band"] = np.array(T), np.array(BAND)
for key in ("exact_vs_filter", "exact_vs_filter_256", "float32_shift"):
    print("largest %s: %.2e" % (key, max(store[n + "/" + key].max() for n in names)))
out = os.path.join(HERE, "recon_metrics.npz")
np.savez_compressed(out, **store)
print("wrote %s: %d cases, %d bytes" % (out, len(names), os.path.getsize(out)))
assert os.path.getsize(out) < 1 << 20
