"""The aggregation streaming kernels (csrc/agg_stream.h) bit for bit against the pinned revision: SHA-256 of every output of
agg_stream_family_util's cases -- forward out / attn in three storage types, d/d logits and d/d flow, resample2d's
d/d input2 -- equals tests/golden/agg_stream_digests.json, written by tests/golden/make_agg_stream_digests.py on the
revision before the kernels' shared machinery moved into one header.  agg_stream_family_util's docstring says why float
gradients published with atomics can be pinned."""
import json
import os

import pytest

import agg_stream_family_util as af

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_stream_digests.json")) as _f:
    PINNED = json.load(_f)


def _check(got):
    assert got and set(got) <= set(PINNED)
    wrong = sorted(k for k in got if got[k] != PINNED[k])
    assert not wrong, "%d of %d digests differ: %s" % (len(wrong), len(got), wrong[:8])


@pytest.mark.parametrize("shape,kind", af.CASES, ids=af.case_id)
def test_forward_digests(gfla, shape, kind):
    _check(af.forward_digests(shape, kind))


@pytest.mark.parametrize("shape,kind", af.CASES, ids=af.case_id)
def test_gradient_digests(gfla, shape, kind):
    ranges = {}
    got = af.gradient_digests(shape, kind, ranges)
    assert all(n <= 2 for n in ranges.values()), ranges
    _check(got)


@pytest.mark.parametrize("shape,kind", af.CASES, ids=af.case_id)
def test_resample2d_input2_gradient_digests(gfla, shape, kind):
    ranges = {}
    got = af.resample_digests(shape, kind, ranges)
    assert all(n <= 2 for n in ranges.values()), ranges
    _check(got)


def test_every_pinned_digest_is_checked():
    n_grad = sum(len(af.grad_key5(s, kind)) for s, kind in af.CASES)
    n_rs = sum(len(af.grad_key5(s, "smooth")) for s, kind in af.CASES)
    n_fwd = len(af.CASES) * len(af.DTYPES) * len(af.KS) * len(af.FWD_KEY5) * 2
    # per gradient run: grad_logits in three storage types at every k, f32 grad_flow at k = 3, 5
    assert len(PINNED) == n_fwd + n_grad * (3 * len(af.KS) + 2) + n_rs * 2
    assert all(k.split("/")[0] in ("fwd", "bwd", "rs2") for k in PINNED)
