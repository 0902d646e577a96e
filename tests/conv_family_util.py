"""Shared by tests/test_conv_family_gpu.py and tests/golden/make_conv_family_digests.py: the cases of the implicit-GEMM
convolution family (csrc/conv_igemm.h) whose outputs are pinned bit for bit, and their SHA-256 digests.  Everything goes
through the package's public functions (and, for the addend aliasing the output, the C entry point the generator tests
already call), so the same code runs on any revision of the library.  Inputs are the seeded host tensors of the per-call
tests (vgg_util.conv_inputs, gen_conv_util.conv_inputs): no NaN, parameters held in float32."""
import hashlib

import torch

import gen_conv_util as gu
import vgg_util as vu

DTYPES = gu.DTYPES
# (B, Cin, Cout, H, W): one padded chunk, TW = 8; all halo; TW = 16, two waves along the channels with a skipped tile (where
# a contiguous and an interleaved assignment of channel tiles to waves differ); TW = 32, two channel blocks, the second
# partly empty; tiles straddling both edges
VGG_SHAPES = [(1, 3, 64, 9, 7), (1, 64, 64, 1, 1), (3, 128, 96, 16, 11), (1, 8, 160, 5, 60), (2, 20, 40, 33, 17)]
VGG_CASES = [(n, s) for s in VGG_SHAPES for n in gu.ALL]
# the per-call cases of test_gen_conv_gpu.py, plus a call without a bias per geometry at odd sizes over several tiles
_NO_BIAS = {gu.S1K3: (2, 20, 40, 33, 17), gu.S2K4: (2, 20, 40, 33, 17), gu.T2K3: (2, 20, 40, 17, 9)}
GEN_CASES = [(g, n, s, o) for g, cases in ((gu.S1K3, gu.S1K3_CASES), (gu.S2K4, gu.S2K4_CASES), (gu.T2K3, gu.T2K3_CASES))
             for n, s, o in cases + [(n, _NO_BIAS[g], {"nobias": True}) for n in gu.ALL]]
_GEOMETRY_NAMES = {gu.S1K3: "S1K3", gu.S2K4: "S2K4", gu.T2K3: "T2K3"}


def shape_id(shape):
    return "x".join(map(str, shape))


def vgg_key(name, shape):
    return "conv3x3_relu/%s/%s" % (name, shape_id(shape))


def gen_key(geometry, name, shape, opts):
    return "%s/%s/%s/%s" % (_GEOMETRY_NAMES[geometry], name, shape_id(shape), gu.case_id(opts))


def vgg_run(gfla, name, shape):
    """(x, w, b, gy, y, dx) on the GPU: conv3x3_relu's inputs, its output and its data gradient"""
    x, w, b, gy = vu.conv_inputs(shape, DTYPES[name], seed=sum(shape))
    xg, w, b, gy = x.cuda().requires_grad_(), w.float().cuda(), b.float().cuda(), gy.cuda()
    y = gfla.conv3x3_relu(xg, w, b)
    y.backward(gy)
    return xg.detach(), w, b, gy, y.detach(), xg.grad


def gen_run(gfla, geometry, name, shape, opts):
    """the call of test_gen_conv_gpu.check_forward; with "nobias" the bias is None"""
    has_add = bool(opts.get("add") or opts.get("alias"))
    x, w, b, add = gu.conv_inputs(geometry, shape, DTYPES[name], seed=sum(shape) + geometry, with_add=has_add)
    b = None if opts.get("nobias") else b.float().cuda()
    with torch.no_grad():
        if opts.get("alias"):
            return gu.call_in_place(x.cuda(), w.float().cuda(), b, add.cuda())
        return gu.call(gfla, geometry, x.cuda(), w.float().cuda(), b, bool(opts.get("reflect")), opts.get("slope"),
                       None if add is None else add.cuda())


def digest(t):
    """SHA-256 of the raw bytes of t + 0 (a signed zero cannot matter)"""
    return hashlib.sha256((t + 0).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def vgg_digests(gfla, name, shape):
    _, _, _, _, y, dx = vgg_run(gfla, name, shape)
    return {vgg_key(name, shape) + "/fwd": digest(y), vgg_key(name, shape) + "/dgrad": digest(dx)}


def gen_digests(gfla, geometry, name, shape, opts):
    return {gen_key(geometry, name, shape, opts): digest(gen_run(gfla, geometry, name, shape, opts))}
