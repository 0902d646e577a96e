"""The routing of the gather/scatter ops (csrc/gs_route.h) as the host-side queries report it, against the pinned revision:
the sweep of gs_route_util over shapes, kernel sizes and tuning-key sets gives, per (key set, query, op), the SHA-256 and
the class counts of tests/golden/gs_route_queries.json -- written by tests/golden/make_gs_route_queries.py on the revision
before the launchers and the queries were put on one route function per op.  No GPU needed.  A differing group is found
with `make_gs_route_queries.py --dump <group>` on the two builds."""
import json
import os

import pytest

import gs_route_util as gr

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gs_route_queries.json")) as _f:
    PINNED = json.load(_f)


@pytest.fixture(scope="module")
def swept():
    return gr.sweep()[0]


def test_every_group_is_pinned(swept):
    assert set(swept) == set(PINNED)
    assert len(swept) == len(gr.KEY_SETS) * (8 + 5 + 3)


@pytest.mark.parametrize("keys", gr.KEY_SETS, ids=gr.key_set_id)
def test_answers_equal_the_pinned_revision(swept, keys):
    mine = [g for g in swept if g.startswith(gr.key_set_id(keys) + "/")]
    assert len(mine) == 8 + 5 + 3
    wrong = sorted(g for g in mine if swept[g] != PINNED[g])
    assert not wrong, "; ".join("%s: %s, pinned %s" % (g, swept[g]["classes"], PINNED[g]["classes"]) for g in wrong)


def test_every_class_of_every_op_occurs(swept):
    """Over the key sets together: each op of gfla_lds_plane_geometry is answered with whole planes, with split > 1 and with
    `not taken`, and the ops whose kernels can window (0, 5, 6, 7) with a row window; the other queries answer both ways."""
    for op in gr.LDS_OPS:
        seen = set()
        for keys in gr.KEY_SETS:
            seen |= {c for c, n in swept[gr.group_id(keys, "lds_plane_geometry", op)]["classes"].items() if n}
        want = set(gr.CLASSES) - (set() if op in gr.WINDOW_OPS else {"window"})
        assert seen == want, (op, seen)
    for op in range(5):
        seen = set()
        for keys in gr.KEY_SETS:
            seen |= set(swept[gr.group_id(keys, "big_plane_geometry", op)]["classes"])
        assert seen == {"in_regime", "outside"}, (op, seen)
    for query, want in (("unfold_supported", {"supported", "not_supported"}),
                        ("aggregate_bwd_supported", {"supported", "not_supported"}),
                        ("aggregate_fwd_geometry", {"taken", "not_taken"})):
        seen = set()
        for keys in gr.KEY_SETS:
            seen |= set(swept[gr.group_id(keys, query, 0)]["classes"])
        assert seen == want, (query, seen)


def test_default_keys_reach_every_class(swept):
    """Under the default keys alone the grid already holds every class of the planes-in-LDS query."""
    for op in gr.LDS_OPS:
        seen = {c for c, n in swept[gr.group_id({}, "lds_plane_geometry", op)]["classes"].items() if n}
        want = set(gr.CLASSES) - (set() if op in gr.WINDOW_OPS else {"window"})
        assert seen == want, (op, seen)
