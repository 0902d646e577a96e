"""Image inputs on the device (csrc/image_inputs.hip, include/gfla_image.h): what a loader does to the decoded pixels with
PIL before ToTensor -- Image.resize and the nearest-neighbour Image.transform(AFFINE) behind torchvision's F.affine --, on
uint8 tensors, byte for byte what Pillow writes.

    augmentation_matrices(angle, translate, scale, size)   host: the reference's get_inverse_affine_matrix / get_affine_matrix
    affine_images(images_u8, inverse, fill, ...)           (B, H, W, C) uint8 -> warped, normalised (B, C, H, W)
    resize_images(images_u8, size, interpolation)          (B, h, w, C) uint8 -> (B, H, W, C) uint8, bilinear or bicubic

GPU tensors run on the library's kernels.  CPU tensors, and impl="torch" on any device, take the torch compositions below:
the same integer and float64 expressions in the same order, which the tests pin to Pillow on the host and compare the
kernels with on the device.  The channels of a resize are filtered one by one: Pillow's detour through premultiplied alpha
for its LA and RGBA modes is a matter of those modes, not of the 8-bit filter, and is not taken.
"""
import ctypes
import functools
import math

import torch

from . import _lib
from .pose_inputs import _channel_values, _check_out, _size, _storage, torch_normalize_images

_LIMIT = 32767.0                       # Pillow's fixed-point route holds below 32768; below 32767 every sum fits an int32
_FILTERS = {"bilinear": 1.0, "bicubic": 2.0}
_PRECISION_BITS = 22                   # Pillow's 8-bit resampling: coefficients in 2^-22, 32-bit accumulation


# ---- augmentation_matrices -------------------------------------------------------------------------------------------------
def _per_sample(value, what, width=None):
    t = torch.as_tensor(value, dtype=torch.float64).cpu()
    if t.dim() == 0:
        t = t.view(1)
    if (t.dim() != 1 if width is None else t.dim() != 2 or t.shape[1] != width) or t.shape[0] == 0:
        raise ValueError("augmentation_matrices: %s is one %s per sample (got shape %s)"
                         % (what, "number" if width is None else "row of %d" % width, tuple(t.shape)))
    return t.tolist()


def augmentation_matrices(angle, translate, scale, size):
    """(inverse (B, 2, 3), forward (B, 3, 3)), float64 on the host, of B augmentations: angle in degrees, translate rows
    (tx, ty) in pixels, scale; size (H, W).  inverse is the reference's get_inverse_affine_matrix with shear 0 and the centre
    (W * 0.5 + 0.5, H * 0.5 + 0.5), evaluated with math.cos / math.sin in that function's order: what affine_images takes
    (and PIL's Image.transform).  forward is np.linalg.inv of the padded inverse, as in get_affine_matrix: what
    pose_maps(affine=...) takes."""
    import numpy as np
    H, W = _size(size, "augmentation_matrices: size")
    angles, scales = _per_sample(angle, "angle"), _per_sample(scale, "scale")
    shifts = _per_sample(translate, "translate", 2)
    if not len(angles) == len(scales) == len(shifts):
        raise ValueError("augmentation_matrices: as many angles, translations and scales as samples (got %d, %d, %d)"
                         % (len(angles), len(shifts), len(scales)))
    if any(s == 0 or not math.isfinite(s) for s in scales):
        raise ValueError("augmentation_matrices: scale is finite and not 0 (got %r)" % (scales,))
    centre = (W * 0.5 + 0.5, H * 0.5 + 0.5)
    inverse, forward = [], []
    for a, t, s in zip(angles, shifts, scales):
        a = math.radians(a)
        s = 1.0 / s
        d = math.cos(a) * math.cos(a) + math.sin(a) * math.sin(a)
        m = [math.cos(a), math.sin(a), 0, -math.sin(a), math.cos(a), 0]
        m = [s / d * v for v in m]
        m[2] += m[0] * (-centre[0] - t[0]) + m[1] * (-centre[1] - t[1])
        m[5] += m[3] * (-centre[0] - t[0]) + m[4] * (-centre[1] - t[1])
        m[2] += centre[0]
        m[5] += centre[1]
        inverse.append(m)
        forward.append(np.linalg.inv(np.array(m + [0.0, 0.0, 1.0], dtype=np.float64).reshape(3, 3)))
    return (torch.tensor(inverse, dtype=torch.float64).view(-1, 2, 3),
            torch.from_numpy(np.stack(forward)).to(torch.float64).contiguous())


# ---- argument checks, shared by both routes -------------------------------------------------------------------------------
def _check_images(images_u8, what):
    if images_u8.dim() != 4 or 0 in images_u8.shape or not 1 <= images_u8.shape[3] <= 4:
        raise ValueError("%s: images are (B, H, W, C) with C in 1..4, nothing empty (got %s)" % (what, tuple(images_u8.shape)))
    if images_u8.dtype != torch.uint8:
        raise TypeError("%s: uint8 images (got %s)" % (what, images_u8.dtype))


def _fill_values(fill, C):
    try:
        values = tuple(fill) if isinstance(fill, (tuple, list)) else (fill,) * C
        ints = tuple(int(v) for v in values)
    except (TypeError, ValueError):
        raise ValueError("affine_images: fill is an integer 0..255 or one per channel (got %r)" % (fill,))
    if len(ints) != C or any(i != v or not 0 <= i <= 255 for i, v in zip(ints, values)):
        raise ValueError("affine_images: fill is an integer 0..255, or one per channel (C = %d, got %r)" % (C, fill))
    return ints


def _check_inverse(images_u8, inverse):
    B = images_u8.shape[0]
    if inverse.dim() != 3 or tuple(inverse.shape) != (B, 2, 3):
        raise ValueError("affine_images: inverse is (B, 2, 3) with the images' B = %d (got %s)" % (B, tuple(inverse.shape)))
    if inverse.dtype != torch.float64:
        raise TypeError("affine_images: inverse is float64 (got %s)" % inverse.dtype)
    if inverse.device != images_u8.device:
        raise ValueError("affine_images: inverse on the images' device (%s, got %s)" % (images_u8.device, inverse.device))


# ---- the torch compositions -----------------------------------------------------------------------------------------------
def torch_affine_bytes(images_u8, inverse, fill=128, scale_branch=True):
    """Image.transform(size, AFFINE, inverse[b], NEAREST, fillcolor=fill) of every image, as a torch composition on the
    images' device: (the warped (B, H, W, C) uint8 images, the (B,) mask of poisoned samples, whose bytes are the fill).
    The expressions of include/gfla_image.h in their order: float64 and int64 tensor operations, one per step.
    scale_branch=False sends every sample through the fixed-point branch, which is not what Pillow does for a matrix
    without rotation: the tests show with it that the two branches differ."""
    _check_images(images_u8, "affine_images")
    _check_inverse(images_u8, inverse)
    B, H, W, C = images_u8.shape
    dev = images_u8.device
    fills = torch.tensor(_fill_values(fill, C), dtype=torch.uint8, device=dev)
    m = inverse.reshape(B, 6)
    bad = ~torch.isfinite(m).all(1)
    for x in (0.0, float(W)):
        for y in (0.0, float(H)):
            for r in (0, 3):
                reach = ((x * m[:, r] + y * m[:, r + 1]) + m[:, r + 2]).abs()
                bad = bad | ~(reach < _LIMIT)
    m = torch.where(bad[:, None], torch.zeros_like(m), m)              # a poisoned sample's coordinates are never used
    m0, m1, m2, m3, m4, m5 = m.unbind(1)
    scaled = (m1 == 0) & (m3 == 0) if scale_branch else torch.zeros_like(bad)

    def table(start, step, n):                                         # ImagingScaleAffine: n additions, one after another
        o, cols = start + step * 0.5, []
        for _ in range(n):
            cols.append(torch.where(o < 0, torch.full_like(o, -1.0), o).to(torch.int64))
            o = o + step
        return torch.stack(cols, dim=1)
    xin_s, yin_s = table(m2, m0, W)[:, None, :], table(m5, m4, H)[:, :, None]

    def fix(v):                                                        # affine_fixed: 16.16 fixed point
        return torch.floor(v * 65536.0 + 0.5).to(torch.int64)[:, None, None]
    a0, a1, a3, a4 = fix(m0), fix(m1), fix(m3), fix(m4)
    a2, a5 = fix((m2 + m0 * 0.5) + m1 * 0.5), fix((m5 + m3 * 0.5) + m4 * 0.5)
    xs = torch.arange(W, dtype=torch.int64, device=dev)[None, None, :]
    ys = torch.arange(H, dtype=torch.int64, device=dev)[None, :, None]
    xin_f, yin_f = (a2 + a0 * xs + a1 * ys) >> 16, (a5 + a3 * xs + a4 * ys) >> 16
    pick = scaled[:, None, None]
    xin, yin = torch.where(pick, xin_s, xin_f), torch.where(pick, yin_s, yin_f)
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H) & ~bad[:, None, None]
    at = (yin.clamp(0, H - 1) * W + xin.clamp(0, W - 1)).view(B, H * W, 1).expand(B, H * W, C)
    picked = images_u8.reshape(B, H * W, C).gather(1, at).view(B, H, W, C)
    return torch.where(inside[..., None], picked, fills.view(1, 1, 1, C).expand(B, H, W, C)).contiguous(), bad


def torch_affine_images(images_u8, inverse, fill=128, mean=0.5, std=0.5, dtype=torch.float32):
    """affine_images as a torch composition: torch_affine_bytes, then torch_normalize_images of the chosen bytes in float32,
    NaN over the poisoned samples, rounded once more for a 16-bit dtype."""
    warped, bad = torch_affine_bytes(images_u8, inverse, fill)
    x = torch_normalize_images(warped, mean, std, torch.float32)
    x = torch.where(bad[:, None, None, None], torch.full_like(x, float("nan")), x)
    return x.to(dtype)


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=256)
def resize_coefficients(n_in, n_out, interpolation):
    """Pillow's precompute_coeffs / normalize_coeffs_8bpc for one axis, in float64 on the host:
    (ksize, [(xmin, xmax)] per output index, [ksize integer coefficients in 2^-22] per output index)."""
    S, filt = _FILTERS[interpolation], _bilinear if interpolation == "bilinear" else _bicubic
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = S * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, coeffs = [], []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [filt((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(v * (1 << _PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << _PRECISION_BITS) - 0.5) for v in w]
        bounds.append((xmin, xmax))
        coeffs.append(k + [0] * (ksize - xmax))
    return ksize, bounds, coeffs


@functools.lru_cache(maxsize=256)
def _device_coefficients(n_in, n_out, interpolation, device):
    """(ksize, coefficients (n_out, ksize) int32, bounds (n_out, 2) int32) on `device`: built and uploaded once"""
    ksize, bounds, coeffs = resize_coefficients(n_in, n_out, interpolation)
    return (ksize, torch.tensor(coeffs, dtype=torch.int32).to(device), torch.tensor(bounds, dtype=torch.int32).to(device))


def _check_resize_args(images_u8, size, interpolation):
    _check_images(images_u8, "resize_images")
    if interpolation not in _FILTERS:
        raise ValueError("resize_images: interpolation is one of %s (got %r)" % (sorted(_FILTERS), interpolation))
    return _size(size, "resize_images: size")


def _torch_resize_pass(x, dim, n_out, interpolation):
    """one axis of (B, h, w, C) int64 values: 2^21 + the weighted sum in integers, shifted and clamped to a byte"""
    n_in = x.shape[dim]
    ksize, coeffs, bounds = _device_coefficients(n_in, n_out, interpolation, x.device)
    taps = torch.arange(ksize, device=x.device)[None, :]
    at = (bounds[:, :1].to(torch.int64) + taps).clamp(max=n_in - 1)            # (n_out, ksize); coefficients past xmax are 0
    k = torch.where(taps < bounds[:, 1:].to(torch.int64), coeffs.to(torch.int64), torch.zeros((), dtype=torch.int64, device=x.device))
    moved = x.movedim(dim, -1)                                                 # (..., n_in)
    acc = (moved[..., at] * k).sum(-1) + (1 << (_PRECISION_BITS - 1))          # (..., n_out)
    return (acc >> _PRECISION_BITS).clamp(0, 255).movedim(-1, dim)


def torch_resize_images(images_u8, size, interpolation="bilinear"):
    """Image.resize(size, BILINEAR | BICUBIC) of 8-bit channels as a torch composition in int64: the horizontal pass into
    bytes, then the vertical one; a pass whose size does not change is skipped."""
    H, W = _check_resize_args(images_u8, size, interpolation)
    x = images_u8.to(torch.int64)
    if W != x.shape[2]:
        x = _torch_resize_pass(x, 2, W, interpolation)
    if H != x.shape[1]:
        x = _torch_resize_pass(x, 1, H, interpolation)
    return x.to(torch.uint8).contiguous()


# ---- the ops --------------------------------------------------------------------------------------------------------------
def affine_images(images_u8, inverse, fill=128, mean=0.5, std=0.5, dtype=torch.float32, impl="auto", out=None):
    """(B, H, W, C) uint8 images, C in 1..4, warped and normalised into the network's input (B, C, H, W): PIL's
    Image.transform(size, AFFINE, inverse[b], NEAREST, fillcolor=fill) -- what torchvision's F.affine does to a PIL image --
    followed by ToTensor and Normalize, in one kernel.  The value of a pixel is exactly normalize_images' of the chosen byte.

    inverse: (B, 2, 3) float64 on the images' device, output pixel -> source pixel (augmentation_matrices' first result).
    fill: an integer 0..255 or one per channel; 0 is the reference's fillcolor=None.  mean=0, std=1: ToTensor alone, the
    route of a mask.  A sample whose matrix has a non-finite entry, or sends a corner of the image to +-32767 or beyond, is
    poisoned: its whole image is NaN and no other sample is touched (include/gfla_image.h has the arithmetic).
    impl "auto": GPU tensors run on the kernels, CPU tensors on the composition; "torch": always the composition.
    out: a contiguous tensor to write into (any element-aligned address).  Nothing is read back: the call can be captured
    in a graph."""
    _lib.check_impl(impl)
    _check_images(images_u8, "affine_images")
    _check_inverse(images_u8, inverse)
    _storage(dtype, "affine_images: dtype")
    B, H, W, C = images_u8.shape
    fills = _fill_values(fill, C)
    means, stds = _channel_values(mean, C, "affine_images", "mean"), _channel_values(std, C, "affine_images", "std")
    if out is not None:
        _check_out(out, (B, C, H, W), dtype, images_u8.device, "affine_images")
    if impl == "torch" or not images_u8.is_cuda:
        got = torch_affine_images(images_u8, inverse, fills, means, stds, dtype)
        return got if out is None else out.copy_(got)
    return _launch_affine_images(images_u8, inverse, fills, means, stds, dtype, out)


def _launch_affine_images(images_u8, inverse, fills, means, stds, dtype, out=None):
    _lib.require_gpu(images_u8, inverse, out)
    B, H, W, C = images_u8.shape
    x, m = images_u8.contiguous(), inverse.contiguous()
    if out is None:
        out = torch.empty((B, C, H, W), dtype=dtype, device=x.device)
    tables = _lib.workspace("gfla_affine_images_workspace_bytes", x, B, H, W, what="affine_images")
    f, mu, s = ((ctypes.c_double * C)(*v) for v in (fills, means, stds))
    _lib.call("gfla_affine_images_" + _lib.SUFFIX[dtype], x, _lib.ptr(x), _lib.ptr(m), _lib.ptr(out), _lib.ptr(tables), B, H, W, C,
              *(ctypes.c_void_p(ctypes.addressof(v)) for v in (f, mu, s)))
    return out


def resize_images(images_u8, size, interpolation="bilinear", impl="auto", out=None):
    """(B, h, w, C) uint8 images, C in 1..4 -> (B, H, W, C) uint8: PIL's Image.resize((W, H), BILINEAR | BICUBIC) for 8-bit
    channels, every channel on its own -- the horizontal pass into bytes, then the vertical one, integer coefficients in
    2^-22 built per axis in float64 on the host and kept on the device per (input size, output size, filter).  A pass whose
    size does not change is skipped; the same size on both axes gives a copy.  size: (H, W)."""
    _lib.check_impl(impl)
    H, W = _check_resize_args(images_u8, size, interpolation)
    B, h, w, C = images_u8.shape
    if out is not None:
        _check_out(out, (B, H, W, C), torch.uint8, images_u8.device, "resize_images")
    if impl == "torch" or not images_u8.is_cuda:
        got = torch_resize_images(images_u8, (H, W), interpolation)
        return got if out is None else out.copy_(got)
    return _launch_resize_images(images_u8, H, W, interpolation, out)


def _launch_resize_images(images_u8, H, W, interpolation, out=None):
    _lib.require_gpu(images_u8, out)
    B, h, w, C = images_u8.shape
    x = images_u8.contiguous()
    if out is None:
        out = torch.empty((B, H, W, C), dtype=torch.uint8, device=x.device)
    if (H, W) == (h, w):
        return out.copy_(x)
    # (outer, length, inner) of each pass: the rows of every image with C bytes per pixel, then whole rows of W C bytes
    passes = ([(B * h, w, W, C)] if W != w else []) + ([(B, h, H, W * C)] if H != h else [])
    for i, (outer, n_in, n_out, inner) in enumerate(passes):
        ksize, coeffs, bounds = _device_coefficients(n_in, n_out, interpolation, x.device)
        dst = out if i == len(passes) - 1 else torch.empty((B, h, W, C), dtype=torch.uint8, device=x.device)
        _lib.call("gfla_resize_pass_u8", x, _lib.ptr(x), _lib.ptr(dst), _lib.ptr(coeffs), _lib.ptr(bounds), outer, n_in, n_out,
                  inner, ksize)
        x = dst
    return out
