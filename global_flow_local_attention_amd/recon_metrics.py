"""Reconstruction metrics on the device (csrc/recon_metrics.hip, include/gfla_metrics.h): what the reference does to a
generator's output after the step -- util.tensor2im, then script/metrics.py's Reconstruction_Metrics on the saved bytes.

    images_to_uint8(x, bytes)                  (B, C, H, W) float -> (B, H, W, C) uint8: tensor2im for a whole batch
    reconstruction_metrics(pred_u8, gt_u8)     per image pair: ssim, ssim_256, psnr, l1, mae as (B,) float64 tensors
    ReconstructionMetrics(win_size)            the accumulator: update() per batch, compute() the reference's record

GPU tensors run on the library's kernels.  CPU tensors, and impl="torch" on any device, take the torch compositions below:
the same definitions in float64 tensor operations, which the tests pin to the reference's pipeline (numpy and scipy.ndimage)
on the host and compare the kernels with on the device.  Shapes the kernels do not take go to the compositions as well.
"""
import ctypes
import math

import torch

from . import _lib
from .pose_inputs import _check_out, _storage

METRICS = ("ssim", "ssim_256", "psnr", "l1", "mae")                 # the rows of gfla_recon_metrics' output, in order
_FLAG = {"ssim": 1, "ssim_256": 2, "psnr": 4, "l1": 4, "mae": 4}
_K1, _K2 = 0.01, 0.03


def gaussian_taps(sigma=1.5, truncate=3.5):
    """One axis of scipy.ndimage.gaussian_filter's window: exp(-x^2 / (2 sigma^2)) for x = -r .. r, r = int(truncate sigma +
    0.5), divided by their sum, in float64 on the host.  The defaults are the 11 taps of ssim_256."""
    radius = int(truncate * sigma + 0.5)
    phi = [math.exp(-0.5 / (sigma * sigma) * (x * x)) for x in range(-radius, radius + 1)]
    total = 0.0
    for v in phi:
        total += v
    return [v / total for v in phi]


_TAPS = gaussian_taps()
_TAPS_C = (ctypes.c_double * len(_TAPS))(*_TAPS)


# ---- images_to_uint8 --------------------------------------------------------------------------------------------------------
def _check_float_images(x, what):
    if x.dim() != 4 or 0 in x.shape:
        raise ValueError("%s: x is (B, C, H, W), nothing empty (got %s)" % (what, tuple(x.shape)))
    _storage(x.dtype, what + ": x")


def _bytes_value(bytes):
    value = ctypes.c_float(float(bytes)).value                              # rounded to float32 on the host
    if not math.isfinite(value):
        raise ValueError("images_to_uint8: bytes is finite in float32 (got %r)" % (bytes,))
    return value


def torch_images_to_uint8(x, bytes=255.0):
    """images_to_uint8 as a torch composition on x's device: float32 tensor operations, one per step (every operand a
    tensor: a division by a host scalar may become a multiplication by its reciprocal)."""
    _check_float_images(x, "images_to_uint8")
    one, two, scale, top = (torch.full((), v, dtype=torch.float32, device=x.device) for v in (1.0, 2.0, _bytes_value(bytes), 256.0))
    t = ((x.to(torch.float32) + one) / two) * scale
    t = torch.where(t >= 0, t, torch.zeros_like(t))                        # NaN compares false: 0
    t = torch.where(t >= top, torch.full_like(t, 255.0), t)
    return t.to(torch.int32).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def images_to_uint8(x, bytes=255.0, out=None, impl="auto"):
    """(B, C, H, W) float32, float16 or bfloat16 -> (B, H, W, C) uint8, interleaved (the layout normalize_images reads): the
    reference's tensor2im, `(x + 1) / 2.0 * bytes` cast to uint8, for every image of the batch (the reference converts
    image 0 only).  16-bit inputs are widened first, as .float() does there.  The arithmetic is numpy's on a float32 array:
    t = ((x + 1) / 2) * bytes with every operation rounded to float32, and the byte is t truncated toward zero for
    0 <= t < 256.  Outside that range numpy's cast is platform-defined; here it saturates -- t < 0 gives 0, t >= 256 gives
    255 -- and NaN gives 0.  A generator's tanh never gets there.
    impl "auto": GPU tensors run on the kernel, CPU tensors on the composition; "torch": always the composition.
    out: a contiguous uint8 tensor to write into (any address)."""
    _lib.check_impl(impl)
    _check_float_images(x, "images_to_uint8")
    value = _bytes_value(bytes)
    B, C, H, W = x.shape
    if out is not None:
        _check_out(out, (B, H, W, C), torch.uint8, x.device, "images_to_uint8")
    if impl != "torch" and x.is_cuda:
        try:
            return _launch_images_to_uint8(x, value, out)
        except _lib.Unsupported:
            pass
    got = torch_images_to_uint8(x, value)
    return got if out is None else out.copy_(got)


def _launch_images_to_uint8(x, value, out=None):
    _lib.require_gpu(x, out)
    B, C, H, W = x.shape
    x = x.contiguous()
    made = torch.empty((B, H, W, C), dtype=torch.uint8, device=x.device) if out is None else out
    _lib.call("gfla_images_to_uint8_" + _lib.SUFFIX[x.dtype], x, _lib.ptr(x), _lib.ptr(made), B, C, H, W, value)
    return made


# ---- argument checks, shared by both routes -------------------------------------------------------------------------------
def _check_metrics_args(pred_u8, gt_u8, win_size, metrics):
    """-> (win_size, the metrics asked for in METRICS' order); ValueError as skimage raises it"""
    for t, name in ((pred_u8, "pred_u8"), (gt_u8, "gt_u8")):
        if t.dim() != 4 or 0 in t.shape or not 1 <= t.shape[3] <= 4:
            raise ValueError("reconstruction_metrics: %s is (B, H, W, C) with C in 1..4, nothing empty (got %s)"
                             % (name, tuple(t.shape)))
        if t.dtype != torch.uint8:
            raise TypeError("reconstruction_metrics: %s is uint8 (got %s)" % (name, t.dtype))
    if pred_u8.shape != gt_u8.shape or pred_u8.device != gt_u8.device:
        raise ValueError("reconstruction_metrics: pred and gt of one shape on one device (got %s on %s, %s on %s)"
                         % (tuple(pred_u8.shape), pred_u8.device, tuple(gt_u8.shape), gt_u8.device))
    names = (metrics,) if isinstance(metrics, str) else tuple(metrics)
    if not names or any(m not in METRICS for m in names):
        raise ValueError("reconstruction_metrics: metrics out of %s (got %r)" % (METRICS, metrics))
    win = int(win_size)
    if win != win_size or win % 2 == 0 or not 3 <= win <= 255:
        raise ValueError("reconstruction_metrics: win_size is odd, from 3 to 255 (got %r)" % (win_size,))
    H, W = pred_u8.shape[1], pred_u8.shape[2]
    for name, side in (("ssim", win), ("ssim_256", len(_TAPS))):
        if name in names and (H < side or W < side):
            raise ValueError("reconstruction_metrics: %s needs images of at least %d x %d, its window (got %d x %d)"
                             % (name, side, side, H, W))
    return win, tuple(m for m in METRICS if m in names)


def _as_bytes(t, impl):
    return images_to_uint8(t, impl=impl) if t.dtype.is_floating_point else t


# ---- the torch composition ------------------------------------------------------------------------------------------------
def _valid_windows(v, taps):
    """correlation of (B, C, H, W) with `taps` along H, then along W, at the positions whose window lies inside: taps in
    order, one product and one sum at a time (gfla_metrics.h's order)"""
    for dim in (2, 3):
        n = v.shape[dim] - len(taps) + 1
        acc = None
        for i, t in enumerate(taps):
            term = v.narrow(dim, i, n) * t
            acc = term if acc is None else acc + term
        v = acc
    return v


def _box_sums(v, win):
    return v.unfold(2, win, 1).sum(-1).unfold(3, win, 1).sum(-1)


def _ssim_map(ux, uy, uxx, uyy, uxy, cov_norm, C1, C2):
    """skimage's compare_ssim from the filtered moments on"""
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    A1, A2 = 2 * ux * uy + C1, 2 * vxy + C2
    B1, B2 = ux * ux + uy * uy + C1, vx + vy + C2
    return (A1 * A2) / (B1 * B2)


def torch_reconstruction_metrics(pred_u8, gt_u8, win_size=51, metrics=METRICS):
    """reconstruction_metrics as a torch composition on the inputs' device: float32(byte) / 255 first, exactly as the
    reference reads its files, then skimage's formulas (of the version the reference was written against: inputs converted
    to float64 before filtering) in float64 tensor operations."""
    win, names = _check_metrics_args(pred_u8, gt_u8, win_size, metrics)
    dev = pred_u8.device
    scale = torch.full((), 255.0, dtype=torch.float32, device=dev)
    b32, a32 = (t.permute(0, 3, 1, 2).to(torch.float32) / scale for t in (pred_u8, gt_u8))       # img_pred, img_gt
    out = {}
    if "ssim" in names:
        x, y = a32.to(torch.float64), b32.to(torch.float64)
        N = win * win
        ux, uy, uxx, uyy, uxy = (_box_sums(v, win) / N for v in (x, y, x * x, y * y, x * y))
        S = _ssim_map(ux, uy, uxx, uyy, uxy, N / (N - 1.0), (_K1 * 1) ** 2, (_K2 * 1) ** 2)
        out["ssim"] = S.mean((2, 3)).mean(1)
    if "ssim_256" in names:
        p256 = b32 * scale
        x, y = (a32 * scale).to(torch.float64), p256.to(torch.float64)
        R = (p256.amax((1, 2, 3)) - p256.amin((1, 2, 3))).to(torch.float64).view(-1, 1, 1, 1)
        ux, uy, uxx, uyy, uxy = (_valid_windows(v, _TAPS) for v in (x, y, x * x, y * y, x * y))
        S = _ssim_map(ux, uy, uxx, uyy, uxy, 1.0, (_K1 * R) * (_K1 * R), (_K2 * R) * (_K2 * R))
        out["ssim_256"] = S.mean((2, 3)).mean(1)
    if set(names) & {"psnr", "l1", "mae"}:
        a, b = a32.to(torch.float64), b32.to(torch.float64)
        d = a - b
        mse = (d * d).mean((1, 2, 3))
        out["psnr"] = 10 * torch.log10(1.0 / mse)
        out["l1"] = d.abs().mean((1, 2, 3))
        out["mae"] = d.abs().sum((1, 2, 3)) / (a + b).sum((1, 2, 3))
    return {name: out[name] for name in names}


# ---- the op ---------------------------------------------------------------------------------------------------------------
def reconstruction_metrics(pred_u8, gt_u8, win_size=51, metrics=METRICS, impl="auto"):
    """Per image pair of (B, H, W, C) uint8 batches, C in 1..4: a dict of (B,) float64 tensors on the inputs' device, one
    per name in `metrics`, as script/metrics.py computes them from the saved files (a = float32(gt) / 255, b =
    float32(pred) / 255):

        psnr      10 log10(1 / mean((a - b)^2)), +inf for equal images
        l1        mean |a - b|
        mae       sum |a - b| / sum (a + b), NaN for two black images
        ssim      skimage's structural similarity of a and b with a uniform win_size x win_size window (odd, 3..255), sample
                  covariance, data range 1: per channel the mean over the positions whose window lies inside the image,
                  then the mean over channels
        ssim_256  the same of 255 a and 255 b with Gaussian weights (sigma 1.5, 11 x 11), population covariance and the
                  data range max - min of the prediction; a constant prediction gives range 0 and whatever IEEE makes of it

    A float (B, C, H, W) argument goes through images_to_uint8 first: that is what scoring the saved PNG scores.
    ValueError for an even win_size and for an image smaller than a window that is asked for, as skimage raises.
    impl "auto": GPU tensors run on the kernels (include/gfla_metrics.h has the arithmetic; the same bits in every call and
    at every position of every batch), CPU tensors on the composition; "torch": always the composition.  Nothing is read
    back and nothing is copied to the device: the call can be captured in a graph."""
    _lib.check_impl(impl)
    pred_u8, gt_u8 = _as_bytes(pred_u8, impl), _as_bytes(gt_u8, impl)
    win, names = _check_metrics_args(pred_u8, gt_u8, win_size, metrics)
    if impl != "torch" and pred_u8.is_cuda:
        try:
            return _launch_reconstruction_metrics(pred_u8, gt_u8, win, names)
        except _lib.Unsupported:
            pass
    return torch_reconstruction_metrics(pred_u8, gt_u8, win, names)


def _launch_reconstruction_metrics(pred_u8, gt_u8, win, names):
    _lib.require_gpu(pred_u8, gt_u8)
    B, H, W, C = pred_u8.shape
    p, g = pred_u8.contiguous(), gt_u8.contiguous()
    flags = 0
    for name in names:
        flags |= _FLAG[name]
    scratch = _lib.workspace("gfla_recon_metrics_workspace_bytes", p, B, H, W, C, win, flags, what="reconstruction_metrics")
    out = torch.empty((len(METRICS), B), dtype=torch.float64, device=p.device)
    _lib.call("gfla_recon_metrics", p, _lib.ptr(p), _lib.ptr(g), _lib.ptr(out), _lib.ptr(scratch), B, H, W, C, win, flags,
              ctypes.c_void_p(ctypes.addressof(_TAPS_C)))
    return {name: out[METRICS.index(name)] for name in names}


def kernel_geometry(win_size=51):
    """{"strip", "band"}: output columns and rows per workgroup of the uniform-window kernel at win_size; "gauss_strip",
    "gauss_band": of the Gaussian one; "pixel_piece": bytes per step of the pixel sums (gfla_recon_metrics_geometry)"""
    out = (ctypes.c_int64 * 5)()
    status = _lib.lib().gfla_recon_metrics_geometry(int(win_size), ctypes.c_void_p(ctypes.addressof(out)))
    if status != 0:
        raise ValueError("kernel_geometry: win_size is odd, from 3 to 255 (got %r)" % (win_size,))
    return dict(zip(("strip", "band", "gauss_strip", "gauss_band", "pixel_piece"), (int(v) for v in out)))


# ---- the accumulator ------------------------------------------------------------------------------------------------------
class ReconstructionMetrics(object):
    """The reference's Reconstruction_Metrics.calculate_from_disk without the disk:

        scores = ReconstructionMetrics(win_size=51)
        for batch in validation:
            scores.update(fake_image, target_image)      # float (B, C, H, W) maps or (B, H, W, C) uint8, on any device
        record = scores.compute()                        # {"psnr": ..., "psnr_variance": ..., "ssim": ..., ...}

    update appends the per-image values on the inputs' device and waits for nothing; compute is the one place that reads
    them back: np.mean and np.var (population) of each metric over every image seen, rounded to 6 decimals as the reference
    records them, as plain floats.  per_image returns the unrounded tensors, reset forgets them."""

    def __init__(self, win_size=51, impl="auto"):
        _lib.check_impl(impl)
        self.win_size, self.impl = win_size, impl
        self.reset()

    def reset(self):
        self._seen = {name: [] for name in METRICS}

    def update(self, pred, gt):
        got = reconstruction_metrics(pred, gt, self.win_size, METRICS, self.impl)
        for name in METRICS:
            self._seen[name].append(got[name])

    def per_image(self):
        if not self._seen[METRICS[0]]:
            raise ValueError("ReconstructionMetrics: no image seen yet")
        return {name: torch.cat(self._seen[name]) for name in METRICS}

    def compute(self):
        import numpy as np
        values = self.per_image()
        record = {}
        with np.errstate(all="ignore"):                                     # an inf PSNR: mean inf, variance NaN, as there
            for name in ("psnr", "ssim", "ssim_256", "mae", "l1"):
                v = values[name].cpu().numpy()
                record[name] = float(round(np.mean(v), 6))
                record[name + "_variance"] = float(round(np.var(v), 6))
        return record
