"""Shared by tests/test_recon_metrics_cpu.py and tests/test_recon_metrics_gpu.py: the fixture of
tests/golden/make_recon_metrics_golden.py, the bar, the inputs of the images_to_uint8 tests and an exact-integer SSIM in
numpy whose window can be moved or shortened on purpose."""
import functools
import os

import numpy as np
import torch

# half a unit of the sixth decimal: the precision at which the reference records each of the five numbers
# (script/metrics.py:371-380, round(., 6)); absolute, per image
BAR = 5e-7
METRICS = ("ssim", "ssim_256", "psnr", "l1", "mae")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recon_metrics.npz")


class Case(object):
    def __init__(self, z, name):
        self.name, self.win = name, int(z[name + "/win"])
        self.pred, self.gt = torch.from_numpy(z[name + "/pred"]), torch.from_numpy(z[name + "/gt"])
        self.want = {m: z[name + "/" + m] for m in METRICS}
        # ssim_256 is not defined below 11 x 11: the fixture holds NaN there and the case does not ask for it
        self.metrics = tuple(m for m in METRICS if m != "ssim_256" or min(self.pred.shape[1:3]) >= 11)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=1)
def fixture():
    """(cases, {"threads", "band"} the fixture's tile-bracketing sizes were made for), loaded once and left unchanged"""
    z = np.load(GOLDEN)
    return [Case(z, str(n)) for n in z["names"]], {"threads": int(z["threads"]), "band": int(z["band"])}


def check(got, want, what, metrics=METRICS):
    """every number of `got` ({name: (B,) tensor}) within BAR of `want` ({name: (B,) array}), inf and NaN matching in kind;
    prints each distance before it asserts; returns the largest"""
    worst, failures = 0.0, []
    for m in metrics:
        g, w = got[m].detach().cpu().numpy().astype(np.float64), np.asarray(want[m], np.float64)
        assert g.shape == w.shape, (what, m, g.shape, w.shape)
        for b in range(len(w)):
            if not np.isfinite(w[b]):
                same = (np.isnan(w[b]) and np.isnan(g[b])) or g[b] == w[b]
                print("%s %s[%d]: %r, want %r" % (what, m, b, g[b], w[b]))
                if not same:
                    failures.append("%s %s[%d]: %r, want %r" % (what, m, b, g[b], w[b]))
                continue
            d = abs(g[b] - w[b])
            print("%s %s[%d]: %.12g, want %.12g, |difference| %.2e (bar %.0e)" % (what, m, b, g[b], w[b], d, BAR))
            worst = max(worst, d) if np.isfinite(d) else float("inf")
            if not d <= BAR:
                failures.append("%s %s[%d]: %.12g is %.2e from %.12g, bar %.0e" % (what, m, b, g[b], d, w[b], BAR))
    assert not failures, "\n".join(failures)
    return worst


# ---- images_to_uint8 ---------------------------------------------------------------------------------------------------------
def numpy_tensor2im(x, scale=255.0):
    """(t, bytes where t is in range) of a float32 array: the reference's expression, util/util.py:19-21"""
    t = (x + 1) / 2.0 * scale
    assert t.dtype == np.float32
    inside = (t >= 0) & (t < 256)
    with np.errstate(invalid="ignore"):
        return t, np.where(inside, t, 0).astype(np.uint8), inside


def boundary_inputs():
    """float32 inputs on both sides of every place where t = ((x + 1) / 2) * 255 crosses a whole number v = 0 .. 256 -- the
    first float32 x with t(x) >= v, found by walking, its two successors and its two predecessors, five per v --, then -1, 1,
    values beyond both, infinities and NaN"""
    def t(x):
        return (np.float32(x) + 1) / 2.0 * 255.0
    down, up = np.float32(-np.inf), np.float32(np.inf)
    values = []
    for v in range(257):
        x = np.float32(2.0 * v / 255.0 - 1.0)
        while t(x) >= v:
            x = np.nextafter(x, down)
        while t(x) < v:
            x = np.nextafter(x, up)
        assert t(x) >= v > t(np.nextafter(x, down)) and t(x).dtype == np.float32
        values += [np.nextafter(np.nextafter(x, down), down), np.nextafter(x, down), x, np.nextafter(x, up),
                   np.nextafter(np.nextafter(x, up), up)]
    values += [-1.0, 1.0, -1.0000001, 1.0000001, -1.01, 1.004, 1.01, -3.0, 3.0, -1e30, 1e30, np.inf, -np.inf, np.nan, 0.0, -0.0]
    return np.array(values, np.float32)


def expected_bytes(x):
    """what images_to_uint8 owes for a float32 array: numpy's bytes where its cast is defined, the documented saturation
    elsewhere"""
    t, inside_bytes, inside = numpy_tensor2im(x)
    out = inside_bytes.copy()
    out[~inside & (t >= 256)] = 255
    out[~inside & ~(t >= 256)] = 0                                    # negative, or NaN
    return out


# ---- an exact-integer SSIM whose window can be wrong on purpose --------------------------------------------------------------
def ssim_uniform_numpy(pred, gt, win, start=0, length=None):
    """ssim of (H, W, C) uint8 arrays from exact integer window sums.  start, length: the window of position (y, x) covers
    rows y + start .. y + start + length - 1 (and columns likewise) instead of y .. y + win - 1; positions whose window
    leaves the image are dropped.  The defaults are the definition."""
    length = win if length is None else length
    N = length * length
    H, W, C = gt.shape
    means = []
    for c in range(C):
        x, y = gt[..., c].astype(np.int64), pred[..., c].astype(np.int64)
        sums = []
        for v in (x, y, x * x, y * y, x * y):
            I = np.zeros((H + 1, W + 1), np.int64)
            I[1:, 1:] = v.cumsum(0).cumsum(1)
            s = I[length:, length:] - I[:-length, length:] - I[length:, :-length] + I[:-length, :-length]
            sums.append(s[start:start + H - win + 1, start:start + W - win + 1].astype(np.float64))
        sx, sy, sxx, syy, sxy = sums
        c1, c2 = (0.01 * 255) ** 2 * N * N, (0.03 * 255) ** 2 * N * (N - 1)
        S = ((2 * sx * sy + c1) * (2 * (N * sxy - sx * sy) + c2)) / ((sx * sx + sy * sy + c1) * ((N * sxx - sx * sx) + (N * syy - sy * sy) + c2))
        means.append(S.mean())
    return float(np.mean(means))


def smooth_pair(H, W, C=1):
    """a smooth ground truth and a prediction a little off it, as uint8 (H, W, C) arrays"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    gt = np.stack([120 + 60 * np.sin(0.21 * x + c) * np.cos(0.17 * y) + 0.5 * x for c in range(C)], -1)
    pred = gt * 0.8 + 20 + 14 * np.cos(0.4 * x[..., None] + 0.3 * y[..., None])
    return np.clip(pred, 0, 255).astype(np.uint8), np.clip(gt, 0, 255).astype(np.uint8)


def changed_byte_batch(H, W):
    """(pred (9, H, W, 1), gt (9, H, W, 1), the places): the smooth pair nine times, the prediction with one byte moved by
    100 at each corner, at the middle of each edge and in the middle"""
    pred, gt = smooth_pair(H, W)
    places = [(r, c) for r in (0, H // 2, H - 1) for c in (0, W // 2, W - 1)]
    preds = []
    for r, c in places:
        p = pred.copy()
        p[r, c, 0] = (int(p[r, c, 0]) + 100) % 256
        preds.append(p)
    return np.stack(preds), np.stack([gt] * len(places)), places
