"""Shared by tests/test_agg_stream_family_gpu.py and tests/golden/make_agg_stream_digests.py: the cases of the aggregation
streaming kernels (csrc/agg_stream.h: agg_coef_kernel, agg_fwd_stream_kernel, agg_ga_stream_kernel with both epilogues)
whose outputs are pinned bit for bit, and their SHA-256 digests.  Everything goes through _lib.aggregate_fwd and the C
entry points, so the same code runs on any revision of the library.

Why a float gradient can be pinned at all: agg_ga_stream_kernel publishes its sums with ONE float atomic per output
element and channel range.  Every gradient case runs with tuning key 5 (the number of channel ranges) at 1 or 2 into
zeroed buffers: at most two addends onto +0, and a + b == b + a exactly.  The one exception is a pixel whose taps are not
a dense patch (the near_integer flows): its d/d logits are published once per CHANNEL, in program order of one lane --
fixed with one range, interleaved freely with two -- so the near_integer gradient cases run with one range only.
grad_source is never digested (its matrix-core scatter's fallback uses float atomics in free order).  The forward has no
atomics: key 5 at 0 (the launcher's choice) and at 2."""
import ctypes
import hashlib

import torch

from global_flow_local_attention_amd import _lib
from util import make_flow, randn

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
KS = (1, 3, 5)
# (B, C, H, W), source and flow maps the same size: the smallest that reach each compile-time chunk size (CHT = 2 with
# one plane, 2, 4, 6, 8) and each tail -- see geometry() and the table in DESIGN.md:
#   one wave, one tile | two chunks + a one-plane tail | a map one patch wide at k = 3 (k = 5: the plain kernels) |
#   two tiles of 8 columns | three chunks with a three-plane tail, 16-wide tiles, overhang in y | two tile groups of 512
#   threads, 104 KB of dynamic LDS, overhang in x and y | nine chunks per range, four tile groups of 768 threads, the XCD
#   remap with padding (two ranges only: key 5 = 2)
SHAPES = [(1, 1, 6, 8), (1, 3, 8, 6), (1, 5, 9, 4), (2, 7, 10, 8), (1, 19, 12, 10), (1, 23, 33, 22), (2, 70, 64, 44)]
TWO_RANGES_ONLY = (2, 70, 64, 44)
# smooth: the common case; wild: clamped columns folded into the coefficients, the window-to-patch select;
# near_integer: the tap-by-tap branch of both kernels
KINDS = ("smooth", "wild", "near_integer")
CASES = [(s, kind) for s in SHAPES for kind in KINDS]
FWD_KEY5 = (0, 2)


def grad_key5(shape, kind):
    """the values of tuning key 5 a gradient case runs with (module docstring)"""
    if kind == "near_integer":
        return (1,)
    return (2,) if shape == TWO_RANGES_ONLY else (1, 2)


def shape_id(shape):
    return "x".join(map(str, shape))


def case_id(v):
    return shape_id(v) if isinstance(v, tuple) else str(v)


def digest(t):
    """SHA-256 of the raw bytes of t + 0 (a signed zero cannot matter)"""
    return hashlib.sha256((t + 0).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def geometry(shape, k):
    """gfla_aggregate_fwd_geometry under the current tuning keys: the nine values, or None where the plain kernels run"""
    B, C, H, W = shape
    out = (ctypes.c_int64 * 9)()
    st = _lib.lib().gfla_aggregate_fwd_geometry(B, C, H, W, H, W, k, out)
    return list(out) if st == 0 else None


def _Tuning(key5):
    """the streaming kernels for every odd k and `key5` channel ranges, for a `with` block (the name is the one
    tests/golden/make_agg_stream_digests.py calls)"""
    return _lib.tuned({_lib.TUNE_AGG_STREAM: 2, _lib.TUNE_SPLIT: key5})


_INPUTS = {}


def inputs(shape, kind):
    """Seeded float32 host tensors of a case, made once: source, flow, grad_out, {k: logits}.  No NaN."""
    if (shape, kind) not in _INPUTS:
        B, C, H, W = shape
        seed = 1000 * sum(shape) + 10 * KINDS.index(kind)
        if kind == "near_integer":   # one or two ulps off an integer, as in test_gpu_parity.py
            flow = make_flow("integer", B, H, W, seed=seed + 1)
            flow = flow + torch.where(randn((B, 2, H, W), seed=seed + 2) > 0, 1.0, -1.0) * 2.0 ** -22
        else:
            flow = make_flow(kind, B, H, W, seed=seed + 1)
        _INPUTS[(shape, kind)] = (randn(shape, seed=seed), flow.contiguous(), randn(shape, seed=seed + 3),
                                  {k: randn((B, k * k, H, W), seed=seed + 4 + k) * 2 for k in KS})
    return _INPUTS[(shape, kind)]


def _forward(src, flow, logits, k, key5):
    out, attn = torch.empty_like(src), torch.empty_like(logits)
    with _Tuning(key5):
        _lib.aggregate_fwd(src, flow, logits, out, attn, k, True)
    return out, attn


def forward_digests(shape, kind):
    s, f, _, lgs = inputs(shape, kind)
    got = {}
    for name, dt in DTYPES.items():
        sd, fd = s.to(dt).to(DEV), f.to(dt).to(DEV)
        for k in KS:
            ld = lgs[k].to(dt).to(DEV)
            for key5 in FWD_KEY5:
                out, attn = _forward(sd, fd, ld, k, key5)
                key = "fwd/%s/%s/%s/k%d/ranges%d" % (shape_id(shape), kind, name, k, key5)
                got[key + "/out"], got[key + "/attn"] = digest(out), digest(attn)
    return got


def gradient_digests(shape, kind, ranges_seen=None):
    """grad_logits (+ grad_flow, f32 at k = 3, 5 with grad_source and the scatter workspace: the only route on which
    launch_agg_ga produces it).  attn is the library's own forward output, pinned by forward_digests.  ranges_seen, when given, collects
    the number of channel ranges the geometry query reports for every case that takes the streaming kernels."""
    B, C, H, W = shape
    s, f, go, lgs = inputs(shape, kind)
    got = {}
    for name, dt in DTYPES.items():
        sd, fd, god = s.to(dt).to(DEV), f.to(dt).to(DEV), go.to(dt).to(DEV)
        for k in KS:
            _, attn = _forward(sd, fd, lgs[k].to(dt).to(DEV), k, 0)
            for key5 in grad_key5(shape, kind):
                gl = torch.zeros((B, k * k, H, W), dtype=torch.float32, device=DEV)
                gf = torch.zeros((B, 2, H, W), dtype=torch.float32, device=DEV)
                key = "bwd/%s/%s/%s/k%d/ranges%d" % (shape_id(shape), kind, name, k, key5)
                with _Tuning(key5):
                    geo = geometry(shape, k)
                    if ranges_seen is not None and geo is not None:
                        ranges_seen[key] = geo[2]
                    if name == "f32":
                        gs = torch.zeros_like(sd)
                        ws = _lib.scatter_workspace(sd, B, H, W, (k + 1) * (k + 1))
                        _lib.call("gfla_local_attn_aggregate_bwd_ws_f32", sd, _lib.ptr(sd), _lib.ptr(fd), _lib.ptr(attn),
                                  _lib.ptr(god), _lib.ptr(gs), _lib.ptr(gf), _lib.ptr(gl), _lib.ptr(ws), B, C, H, W, H, W, k, 1)
                        if k > 1:   # k = 1 has no matrix-core scatter: grad_flow comes from be_bwd_lds's free-order atomics
                            got[key + "/grad_flow"] = digest(gf)
                    else:
                        _lib.call("gfla_local_attn_aggregate_bwd_" + name, sd, _lib.ptr(sd), _lib.ptr(fd), _lib.ptr(attn),
                                  _lib.ptr(god), None, None, _lib.ptr(gl), B, C, H, W, H, W, k, 1)
                got[key + "/grad_logits"] = digest(gl)
    return got


def resample_digests(shape, kind, ranges_seen=None):
    """grad_in2 of resample2d, kernel_size 4, dilation 1: agg_ga_stream_kernel's EPI = 1 instantiation (a K = 3 patch)"""
    B, C, H, W = shape
    s, f, go, _ = inputs(shape, kind)
    i2 = torch.cat((f, torch.full((B, 1, H, W), 1.5)), 1).contiguous()
    got = {}
    for name in ("f32", "bf16"):
        dt = DTYPES[name]
        sd, i2d, god = s.to(dt).to(DEV), i2.to(dt).to(DEV), go.to(dt).to(DEV)
        for key5 in grad_key5(shape, "smooth"):   # no tap-by-tap branch in this epilogue: one atomic per range always
            g2 = torch.zeros((B, 3, H, W), dtype=torch.float32, device=DEV)
            key = "rs2/%s/%s/%s/ranges%d" % (shape_id(shape), kind, name, key5)
            with _Tuning(key5):
                geo = geometry(shape, 3)
                if ranges_seen is not None and geo is not None:
                    ranges_seen[key] = geo[2]
                _lib.call("gfla_resample2d_bwd_" + name, sd, _lib.ptr(sd), _lib.ptr(i2d), _lib.ptr(god), None, _lib.ptr(g2),
                          B, C, H, W, H, W, 4, 1, 0)
            got[key + "/grad_in2"] = digest(g2)
    return got


def all_digests(ranges_seen=None):
    got = {}
    for shape, kind in CASES:
        got.update(forward_digests(shape, kind))
        got.update(gradient_digests(shape, kind, ranges_seen))
        got.update(resample_digests(shape, kind, ranges_seen))
    return got
