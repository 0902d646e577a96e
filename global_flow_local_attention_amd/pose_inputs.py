"""Pose inputs on the device (csrc/pose_inputs.hip, include/gfla_pose.h): the arithmetic between what a loader reads --
key points and uint8 pixels -- and the tensors PoseGenerator.forward takes.

    pose_maps(cords, size, ...)        key points -> Gaussian heat maps      the reference's util/pose_utils.cords_to_map
    pose_cords(maps, threshold)        heat maps -> key points               the reference's util/pose_utils.map_to_cord
    normalize_images(images_u8, ...)   (B, H, W, C) uint8 -> (B, C, H, W)    ToTensor followed by Normalize
    PoseInputs(size, ...)              the three put together: a loader's records -> {P1, BP1, P2, BP2} on the device

GPU tensors run on the library's kernels.  CPU tensors, and impl="torch" on any device, take the torch compositions
below: the same float64 / float32 expressions in the same order, which the tests pin to the reference on the host and
compare the kernels with on the device.  The PIL augmentation of the pixels is image_inputs.py's: PoseInputs takes its inverse
matrices as warp1 / warp2.
"""
import ctypes
import functools
import math

import torch

from . import _lib

_STORAGE = (torch.float32,) + _lib.HALF_TYPES
_CLAMP = float(2 ** 30)


# ---- argument checks, shared by both routes -------------------------------------------------------------------------------
def _size(size, what):
    try:
        h, w = (int(s) for s in size)
    except (TypeError, ValueError):
        raise ValueError("%s: (H, W) (got %r)" % (what, size))
    if h <= 0 or w <= 0:
        raise ValueError("%s: positive sizes (got %r)" % (what, tuple(size)))
    return h, w


def _storage(dtype, what):
    if dtype not in _STORAGE:
        raise TypeError("%s: float32, float16 or bfloat16 (got %s)" % (what, dtype))
    return dtype


def _two_sigma_sq(sigma):
    sigma = float(sigma)
    two = 2.0 * (sigma * sigma)
    if not (math.isfinite(sigma) and sigma > 0 and math.isfinite(two) and two > 0):
        raise ValueError("pose_maps: sigma is a finite number > 0 whose square is one too (got %r)" % (sigma,))
    return two


def _check_maps_args(cords, affine):
    if cords.dim() != 3 or cords.shape[2] != 2 or cords.shape[0] == 0 or cords.shape[1] == 0:
        raise ValueError("pose_maps: cords is (B, J, 2), rows (y, x), B and J at least 1 (got %s)" % (tuple(cords.shape),))
    if cords.dtype == torch.bool or cords.is_complex():
        raise TypeError("pose_maps: cords of an integer or floating dtype (got %s)" % cords.dtype)
    if affine is not None:
        if affine.dim() != 3 or affine.shape[0] != cords.shape[0] or tuple(affine.shape[1:]) not in ((3, 3), (2, 3)):
            raise ValueError("pose_maps: affine is (B, 3, 3) or (B, 2, 3) with cords' B = %d (got %s)"
                             % (cords.shape[0], tuple(affine.shape)))
        if affine.dtype != torch.float64:
            raise TypeError("pose_maps: affine is float64 (got %s)" % affine.dtype)
        if affine.device != cords.device:
            raise ValueError("pose_maps: affine on cords' device (%s, got %s)" % (cords.device, affine.device))


def _check_out(out, shape, dtype, device, what):
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise ValueError("%s: out is a contiguous %s tensor of shape %s on %s (got %s %s on %s, strides %s)"
                         % (what, dtype, tuple(shape), device, out.dtype, tuple(out.shape), out.device, out.stride()))
    return out


def _channel_values(value, C, what, name):
    try:
        values = tuple(float(v) for v in value) if isinstance(value, (tuple, list)) else (float(value),) * C
    except (TypeError, ValueError):
        raise ValueError("%s: %s is a number or a sequence of C numbers (got %r)" % (what, name, value))
    if len(values) != C:
        raise ValueError("%s: %s has one entry per channel (C = %d, got %d)" % (what, name, C, len(values)))
    return _float32_values(values, what, name)


@functools.lru_cache(maxsize=64)
def _float32_values(values, what, name):
    """the float32 roundings the kernels and the composition work on"""
    values = [torch.tensor(v, dtype=torch.float32).item() for v in values]
    if not all(math.isfinite(v) for v in values) or (name == "std" and any(v == 0 for v in values)):
        raise ValueError("%s: %s is finite%s in float32 (got %r)" % (what, name, " and not 0" if name == "std" else "", values))
    return values


# ---- the torch compositions -----------------------------------------------------------------------------------------------
def torch_pose_maps(cords, size, old_size=None, affine=None, sigma=6.0, dtype=torch.float32):
    """cords_to_map as a torch composition in float64, batched, on cords' device: the expressions of include/gfla_pose.h
    in their order."""
    H, W = _size(size, "pose_maps: size")
    H0, W0 = (H, W) if old_size is None else _size(old_size, "pose_maps: old_size")
    two = _two_sigma_sq(sigma)
    _storage(dtype, "pose_maps: dtype")
    _check_maps_args(cords, affine)
    c = cords.to(torch.float64)
    y, x = c[..., 0], c[..., 1]
    missing = (y == -1) | (x == -1)
    bad = ~(torch.isfinite(y) & torch.isfinite(x))
    # divisors as tensors on the device: a division by a host scalar may become a multiplication by its reciprocal
    h0, w0, two = (torch.full((), float(v), dtype=torch.float64, device=c.device) for v in (H0, W0, two))
    p0, p1 = (y / h0) * H, (x / w0) * W
    r0, r1 = p1, p0                                         # r0: column, r1: row
    if affine is not None:
        a = affine[:, :, :, None]                           # a[b, i, k] against (B, J)
        bad = bad | ~torch.isfinite(affine).flatten(1).all(1)[:, None]
        r0 = a[:, 0, 0] * p1 + a[:, 0, 1] * p0 + a[:, 0, 2]
        r1 = a[:, 1, 0] * p1 + a[:, 1, 1] * p0 + a[:, 1, 2]
    bad = (bad | torch.isnan(r0) | torch.isnan(r1)) & ~missing
    plain = ~(bad | missing)

    def factor(r, n):
        centre = torch.where(plain, torch.trunc(r).clamp(-_CLAMP, _CLAMP), torch.zeros_like(r)).to(torch.int64)
        d = torch.arange(n, dtype=torch.int64, device=c.device) - centre[..., None]
        return torch.exp(-(d * d).to(torch.float64) / two)

    maps = (factor(r1, H)[..., :, None] * factor(r0, W)[..., None, :]).to(torch.float32)
    maps = torch.where(bad[..., None, None], torch.full_like(maps, float("nan")), maps)
    maps = torch.where(missing[..., None, None], torch.zeros_like(maps), maps)
    return maps.to(dtype)


def torch_pose_cords(maps, threshold=0.1):
    """map_to_cord as a torch composition: float32 comparisons, first maximum in row-major order"""
    B, J, H, W = maps.shape
    m = maps.to(torch.float32).flatten(2)
    top = m.max(dim=2, keepdim=True).values                 # NaN when the plane holds one: equal to nothing
    hit = (m == top) & (m > torch.full((), float(threshold), dtype=torch.float32, device=m.device))
    n = H * W
    first = torch.where(hit, torch.arange(n, device=m.device), torch.full((), n, dtype=torch.int64, device=m.device)).amin(2)
    found = first < n
    minus = torch.full_like(first, -1)
    return torch.stack([torch.where(found, first // W, minus), torch.where(found, first % W, minus)], dim=2)


def torch_normalize_images(images_u8, mean=0.5, std=0.5, dtype=torch.float32):
    """ToTensor followed by Normalize: ((v / 255) - mean) / std in float32.  Every operand is a tensor on the images'
    device, so each step is the elementwise operation itself (a division by a host scalar may become a multiplication by
    its reciprocal)."""
    B, H, W, C = images_u8.shape
    dev = images_u8.device
    m, s = (torch.tensor(_channel_values(v, C, "normalize_images", n), dtype=torch.float32).view(1, C, 1, 1)
            for v, n in ((mean, "mean"), (std, "std")))
    if dev.type != "cpu":
        m, s = m.to(dev), s.to(dev)
    x = images_u8.permute(0, 3, 1, 2).to(torch.float32)
    x = ((x / torch.full((1,), 255.0, dtype=torch.float32, device=dev)) - m) / s
    return x.contiguous().to(dtype)


# ---- the ops --------------------------------------------------------------------------------------------------------------
def pose_maps(cords, size, old_size=None, affine=None, sigma=6.0, dtype=torch.float32, impl="auto", out=None):
    """Gaussian heat maps (B, J, H, W) of key points `cords` (B, J, 2), rows (y, x), of an integer or floating dtype: the
    reference's cords_to_map, quirks included (include/gfla_pose.h has the arithmetic).

    size (H, W); old_size (H0, W0), the frame the key points are given in (default: size); affine None or (B, 3, 3) /
    (B, 2, 3) float64, the forward matrix applied to [x, y, 1]; dtype float32, float16 or bfloat16.  A joint with y == -1 or
    x == -1 is missing: an all-zero channel.  A joint that is not missing and has a non-finite coordinate or a non-finite
    affine entry fills its channel with NaN.
    impl "auto": GPU tensors run on the kernel, CPU tensors on the composition; "torch": always the composition.
    out: a contiguous tensor to write into (any element-aligned address)."""
    _lib.check_impl(impl)
    H, W = _size(size, "pose_maps: size")
    H0, W0 = (H, W) if old_size is None else _size(old_size, "pose_maps: old_size")
    two = _two_sigma_sq(sigma)
    _storage(dtype, "pose_maps: dtype")
    _check_maps_args(cords, affine)
    B, J = cords.shape[0], cords.shape[1]
    if out is not None:
        _check_out(out, (B, J, H, W), dtype, cords.device, "pose_maps")
    if impl == "torch" or not cords.is_cuda:
        maps = torch_pose_maps(cords, (H, W), (H0, W0), affine, sigma, dtype)
        return maps if out is None else out.copy_(maps)
    return _launch_pose_maps(cords, affine, B, J, H, W, H0, W0, two, dtype, out)


def _launch_pose_maps(cords, affine, B, J, H, W, H0, W0, two, dtype, out=None):
    _lib.require_gpu(cords, affine, out)
    c = cords.to(torch.float64).contiguous()               # exact for every integer and floating dtype
    a = None if affine is None else affine.contiguous()
    if out is None:
        out = torch.empty((B, J, H, W), dtype=dtype, device=cords.device)
    _lib.call("gfla_pose_maps_" + _lib.SUFFIX[dtype], out, _lib.ptr(c), _lib.ptr(a), 0 if a is None else a.shape[1] * 3,
              _lib.ptr(out), B, J, H, W, H0, W0, two)
    return out


def pose_cords(maps, threshold=0.1, impl="auto", out=None):
    """Key points (B, J, 2) int64, rows (y, x), of heat maps (B, J, H, W) in float32, float16 or bfloat16: the reference's
    map_to_cord.  Per channel the first position (row-major) of the maximum if that is > threshold -- a strict float32
    comparison --, else (-1, -1); a channel that holds a NaN gives (-1, -1)."""
    _lib.check_impl(impl)
    if maps.dim() != 4 or 0 in maps.shape:
        raise ValueError("pose_cords: maps is (B, J, H, W), nothing empty (got %s)" % (tuple(maps.shape),))
    _storage(maps.dtype, "pose_cords: maps")
    threshold = float(threshold)
    if math.isnan(threshold):
        raise ValueError("pose_cords: threshold is NaN")
    B, J, H, W = maps.shape
    if out is not None:
        _check_out(out, (B, J, 2), torch.int64, maps.device, "pose_cords")
    if impl == "torch" or not maps.is_cuda:
        got = torch_pose_cords(maps, threshold)
        return got if out is None else out.copy_(got)
    return _launch_pose_cords(maps, threshold, out)


def _launch_pose_cords(maps, threshold, out=None):
    _lib.require_gpu(maps, out)
    B, J, H, W = maps.shape
    m = maps.contiguous()
    if out is None:
        out = torch.empty((B, J, 2), dtype=torch.int64, device=maps.device)
    _lib.call("gfla_pose_cords_" + _lib.SUFFIX[maps.dtype], m, _lib.ptr(m), _lib.ptr(out), B * J, H, W, threshold)
    return out


def normalize_images(images_u8, mean=0.5, std=0.5, dtype=torch.float32, impl="auto", out=None):
    """(B, H, W, C) uint8 images, C in 1..4, as the network's input (B, C, H, W): ((v / 255) - mean) / std in float32 -- a
    true division, a subtraction, a division: ToTensor followed by Normalize --, rounded once more for a 16-bit dtype.
    mean, std: a number, or one per channel."""
    _lib.check_impl(impl)
    if images_u8.dim() != 4 or 0 in images_u8.shape or not 1 <= images_u8.shape[3] <= 4:
        raise ValueError("normalize_images: images are (B, H, W, C) with C in 1..4, nothing empty (got %s)"
                         % (tuple(images_u8.shape),))
    if images_u8.dtype != torch.uint8:
        raise TypeError("normalize_images: uint8 images (got %s)" % images_u8.dtype)
    _storage(dtype, "normalize_images: dtype")
    B, H, W, C = images_u8.shape
    means, stds = _channel_values(mean, C, "normalize_images", "mean"), _channel_values(std, C, "normalize_images", "std")
    if out is not None:
        _check_out(out, (B, C, H, W), dtype, images_u8.device, "normalize_images")
    if impl == "torch" or not images_u8.is_cuda:
        got = torch_normalize_images(images_u8, means, stds, dtype)
        return got if out is None else out.copy_(got)
    return _launch_normalize_images(images_u8, means, stds, dtype, out)


def _launch_normalize_images(images_u8, means, stds, dtype, out=None):
    _lib.require_gpu(images_u8, out)
    B, H, W, C = images_u8.shape
    x = images_u8.contiguous()
    if out is None:
        out = torch.empty((B, C, H, W), dtype=dtype, device=x.device)
    m, s = (ctypes.c_double * C)(*means), (ctypes.c_double * C)(*stds)
    _lib.call("gfla_normalize_images_" + _lib.SUFFIX[dtype], x, _lib.ptr(x), _lib.ptr(out), B, H, W, C,
              ctypes.c_void_p(ctypes.addressof(m)), ctypes.c_void_p(ctypes.addressof(s)))
    return out


# ---- the pieces put together ----------------------------------------------------------------------------------------------
class _Staging(object):
    """Pinned host buffers of one turn, by (slot, shape, dtype), and the event behind their last copies"""

    def __init__(self):
        self.buffers, self.event = {}, None


class PoseInputs(object):
    """A loader's small records -> what TrainerShell.optimize_parameters((P1, BP1, BP2), target=P2, source=P1) takes.

        inputs = PoseInputs((256, 176), old_size=(256, 176))
        batch = inputs(P1_u8, P2_u8, cords1, cords2, affine1, affine2)      # {"P1", "BP1", "P2", "BP2"} on the device
        inverse, forward = augmentation_matrices(angle, shift, scale, (256, 176))
        batch = inputs(P1_u8, P2_u8, cords1, cords2, forward, None, warp1=inverse)          # P1 augmented on the device

    P*_u8: (B, H, W, C) uint8; cords*: (B, J, 2) key points, rows (y, x); affine*: None or the (B, 3, 3) / (B, 2, 3) float64
    forward matrices the key points are augmented with; warp*: None -- the image is already augmented, or is not to be --
    or the (B, 2, 3) float64 inverse matrices affine_images warps it with, out-of-frame pixels taking `fill`
    (image_inputs.augmentation_matrices makes both kinds).  Host tensors are copied non_blocking from
    pinned staging this object owns: two sets take turns, each behind the event of its last copies, so a set is never
    rewritten while a copy may still read it; nothing else waits for the device and nothing reads from it.  With device
    tensors no copy is made, and the call may be captured in a graph: replaying after the key points (or the pixels) were
    overwritten in place gives the new tensors."""

    def __init__(self, size, old_size=None, sigma=6.0, dtype=torch.float32, device="cuda", mean=0.5, std=0.5, fill=128):
        self.size = _size(size, "PoseInputs: size")
        self.old_size = self.size if old_size is None else _size(old_size, "PoseInputs: old_size")
        _two_sigma_sq(sigma)
        self.sigma, self.dtype = float(sigma), _storage(dtype, "PoseInputs: dtype")
        from .image_inputs import _fill_values
        _fill_values(fill, len(fill) if isinstance(fill, (tuple, list)) else 1)
        self.mean, self.std, self.fill = mean, std, fill
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NotImplementedError("GFLA ops run on the GPU only (got device %s); there is no CPU path" % (self.device,))
        self._staging, self._turn = [_Staging(), _Staging()], 0

    def _to_device(self, stage, slot, t):
        if t is None or t.is_cuda:
            return t
        key = (slot, tuple(t.shape), t.dtype)
        pinned = stage.buffers.get(key)
        if pinned is None:
            pinned = stage.buffers[key] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        pinned.copy_(t)
        return pinned.to(self.device, non_blocking=True)

    def _image(self, images_u8, warp):
        if warp is None:
            return normalize_images(images_u8, self.mean, self.std, self.dtype)
        from .image_inputs import affine_images
        return affine_images(images_u8, warp, self.fill, self.mean, self.std, self.dtype)

    def __call__(self, P1_u8, P2_u8, cords1, cords2, affine1=None, affine2=None, warp1=None, warp2=None):
        records = (P1_u8, P2_u8, cords1, cords2, affine1, affine2, warp1, warp2)
        if any(t is not None and not t.is_cuda for t in records):
            stage = self._staging[self._turn]
            self._turn = 1 - self._turn
            if stage.event is not None and not stage.event.query():
                stage.event.synchronize()                    # the copies of two calls ago: done long since
            with torch.cuda.device(self.device):
                records = [self._to_device(stage, i, t) for i, t in enumerate(records)]
                if stage.event is None:
                    stage.event = torch.cuda.Event()
                stage.event.record(torch.cuda.current_stream(self.device))
        P1_u8, P2_u8, cords1, cords2, affine1, affine2, warp1, warp2 = records
        maps = dict(size=self.size, old_size=self.old_size, sigma=self.sigma, dtype=self.dtype)
        return {"P1": self._image(P1_u8, warp1),
                "BP1": pose_maps(cords1, affine=affine1, **maps),
                "P2": self._image(P2_u8, warp2),
                "BP2": pose_maps(cords2, affine=affine2, **maps)}
