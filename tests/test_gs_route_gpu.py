"""One case per route of the gather/scatter ops (csrc/gs_route.h) against the pinned revision: the returned status, the
deltas of the dispatch counters 0, 1 and 12-17, the planes-in-LDS query's answer and the SHA-256 digests of every
order-independent output equal tests/golden/gs_route_digests.json -- written by tests/golden/make_gs_route_digests.py on
the revision before the launchers were put on one route function per op.  gs_route_util's docstring says which outputs
are digested and why their bits cannot depend on the order of arrival; gradients published by atomics in free order are
checked by test_gpu_parity.py, test_plane_geometry_gpu.py, test_big_plane_gpu.py, test_default_path_gpu.py,
test_agg_stream_family_gpu.py and test_f16_gpu.py."""
import json
import os

import pytest

import gs_route_util as gr

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gs_route_digests.json")) as _f:
    PINNED = json.load(_f)


@pytest.mark.parametrize("case", gr.GPU_CASES, ids=gr.gpu_case_id)
def test_route_status_counters_and_digests(gfla, case):
    got = gr.run_gpu_case(case)
    gr.check_named_route(case, got)
    want = PINNED[gr.gpu_case_id(case)]
    assert set(got) == set(want)
    for name in got:
        assert got[name] == want[name], (name, got[name], want[name])


def test_every_pinned_case_is_checked():
    assert set(PINNED) == {gr.gpu_case_id(c) for c in gr.GPU_CASES}
    # every successful record holds exactly the digests its case names
    for case in gr.GPU_CASES:
        for name, rec in PINNED[gr.gpu_case_id(case)].items():
            assert sorted(rec.get("digests", ())) == (sorted(case["digest"]) if rec["status"] == 0 else []), (case, name)
