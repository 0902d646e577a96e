"""The Winograd-domain kernels of the first FC layer (csrc/fc_wino.hip, csrc/fc_wino16.hip and the skeleton they share in
csrc/fc_wino_shared.h, csrc/fc_wino_wgrad.h and the fc_wino_*.inc fragments) against the pinned revision: SHA-256 of every
output of fc_wino_family_util's cases -- forward map, grad_x and grad_w0 of each half in arithmetic modes 4 and 5 under every
staging / unit / split variant, logits and grad_target of the two-job launches -- equals tests/golden/fc_wino_digests.json,
written by tests/golden/make_fc_wino_digests.py on the revision before the four kernels were put on one skeleton.  Bit for
bit, except that digest() hashes t + 0, so a -0 and a +0 digest alike.  fc_wino_family_util's docstring says what is pinned
and what is not."""
import json
import os

import pytest

import fc_wino_family_util as wf

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fc_wino_digests.json")) as _f:
    PINNED = json.load(_f)


def _check(got, pinned_here):
    """every digest pinned for this case is recomputed and equal"""
    assert pinned_here and pinned_here <= set(got)
    wrong = sorted(k for k in pinned_here if got[k] != PINNED[k])
    assert not wrong, "%d of %d digests differ: %s" % (len(wrong), len(pinned_here), wrong[:8])


@pytest.mark.parametrize("shape,is_source,mode", wf.HALF_CASES, ids=wf.case_id)
def test_half_digests(gfla, shape, is_source, mode):
    if not wf.runs_in(shape, mode):
        pytest.skip("shape falls back from mode %d (the mode-4 row covers it)" % mode)
    got = wf.half_digests(shape, is_source, mode)
    prefix = "half/%s/half%d/mode%d/" % (wf.shape_id(shape), is_source, mode)
    assert set(got) == {k for k in PINNED if k.startswith(prefix)}     # every per-half output is pinned, and recomputed
    _check(got, set(got))


@pytest.mark.parametrize("shape,mode", wf.LAYER_CASES, ids=wf.case_id)
def test_two_job_launch_digests(gfla, shape, mode):
    if not wf.runs_in(shape, mode):
        pytest.skip("shape falls back from mode %d" % mode)
    got = wf.layer_digests(shape, mode)
    here = {k for k in got if k.split("/")[-1] in wf.LAYER_PINNED}
    assert here == {k for k in PINNED if k.startswith("layer/%s/mode%d/" % (wf.shape_id(shape), mode))}
    _check(got, here)


def test_every_pinned_digest_is_checked():
    prefixes = {"half/%s/half%d/mode%d/" % (wf.shape_id(s), h, m) for s, h, m in wf.HALF_CASES}
    prefixes |= {"layer/%s/mode%d/" % (wf.shape_id(s), m) for s, m in wf.LAYER_CASES}
    assert all(any(k.startswith(p) for p in prefixes) for k in PINNED)
    assert all(k.split("/")[-1] in wf.LAYER_PINNED for k in PINNED if k.startswith("layer/"))
    assert all(k.split("/")[-1] in ("out", "grad_x", "grad_w0") for k in PINNED if k.startswith("half/"))
    # both arithmetic modes, both kernel sizes and both halves are in the file
    for m in wf.MODES:
        for k in (3, 5):
            for h in (0, 1):
                assert any(p.startswith("half/k%d_" % k) and "/half%d/mode%d/" % (h, m) in p for p in PINNED), (m, k, h)
