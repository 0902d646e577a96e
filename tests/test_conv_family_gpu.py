"""The implicit-GEMM convolution family (csrc/conv_igemm.h) bit for bit.

(a) Across entry points: conv3x3_relu (the VGG variants) and conv3x3 (the generator variant) are the same S1K3 kernel
with the same reduction order per output element (chunk ascending, tap ascending, then the k of the MFMA), so
    conv3x3_relu(x, w, b)              == relu(conv3x3(x, w, b))
    d conv3x3_relu / dx applied to g   == conv3x3(g [y > 0], w mirrored with Cin <-> Cout, no bias)
hold with torch.equal, in every dtype.  They held before the two kernels were one template and hold whatever wave owns
a channel tile.

(b) Against the pinned revision: SHA-256 of every output of conv_family_util's cases equals
tests/golden/conv_family_digests.json, written by tests/golden/make_conv_family_digests.py on the revision before the
merge."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import conv_family_util as cf

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_family_digests.json")) as _f:
    PINNED = json.load(_f)


def _ids(v):
    return v if isinstance(v, str) else str(v) if isinstance(v, int) else cf.shape_id(v) if isinstance(v, tuple) else cf.gu.case_id(v)


@pytest.mark.parametrize("name,shape", cf.VGG_CASES, ids=_ids)
def test_conv3x3_relu_equals_the_generator_conv3x3(gfla, monkeypatch, name, shape):
    x, w, b, gy, y, dx = cf.vgg_run(gfla, name, shape)

    def trap(*args, **kwargs):
        raise AssertionError("conv3x3 took the torch composition")

    monkeypatch.setattr(F, "conv2d", trap)
    monkeypatch.setattr(torch, "conv2d", trap)
    with torch.no_grad():
        fwd = torch.relu(gfla.conv3x3(x, w, b))
        dgrad = gfla.conv3x3(gy * (y > 0), w.flip(2, 3).transpose(0, 1).contiguous(), None)
    assert fwd.dtype == y.dtype and dgrad.dtype == dx.dtype
    assert torch.equal(y, fwd)
    assert torch.equal(dx, dgrad)


@pytest.mark.parametrize("name,shape", cf.VGG_CASES, ids=_ids)
def test_conv3x3_relu_digests(gfla, name, shape):
    got = cf.vgg_digests(gfla, name, shape)
    assert got == {k: PINNED[k] for k in got}


@pytest.mark.parametrize("geometry,name,shape,opts", cf.GEN_CASES, ids=_ids)
def test_gen_conv_digests(gfla, geometry, name, shape, opts):
    got = cf.gen_digests(gfla, geometry, name, shape, opts)
    assert got == {k: PINNED[k] for k in got}


def test_every_pinned_digest_is_checked():
    keys = {k for n, s in cf.VGG_CASES for k in (cf.vgg_key(n, s) + "/fwd", cf.vgg_key(n, s) + "/dgrad")}
    keys |= {cf.gen_key(*case) for case in cf.GEN_CASES}
    assert keys == set(PINNED) and len(keys) == 2 * len(cf.VGG_CASES) + len(cf.GEN_CASES)
