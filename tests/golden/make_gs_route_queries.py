#!/usr/bin/env python3
"""Write tests/golden/gs_route_queries.json: one SHA-256 per (tuning-key set, query, op) over the ordered answers of
tests/gs_route_util.py's sweep of the host-side geometry / support queries (gfla_lds_plane_geometry, gfla_big_plane_geometry,
gfla_unfold_supported, gfla_aggregate_bwd_supported, gfla_aggregate_fwd_geometry), and per group the count of answers in each
class.  No GPU needed.  Run it on the revision whose routing is to be pinned (the parent of a change that must not move a
call to another kernel); tests/test_gs_route_cpu.py recomputes the sweep and compares.

    python tests/golden/make_gs_route_queries.py [output.json]
    python tests/golden/make_gs_route_queries.py --dump [group ...]     print the rows (all groups, or the named ones), so that
                                                                        a differing group can be diffed between two builds
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import gs_route_util as gr  # noqa: E402


def main():
    args = sys.argv[1:]
    groups, rows = gr.sweep()
    if args and args[0] == "--dump":
        for gid in (args[1:] or sorted(rows)):
            for arguments, answer in rows[gid]:
                print("%s %r -> %r" % (gid, arguments, answer))
        return
    out = args[0] if args else os.path.join(HERE, "gs_route_queries.json")
    with open(out, "w") as f:
        json.dump(groups, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d groups, %d queries -> %s" % (len(groups), sum(g["queries"] for g in groups.values()), out))


if __name__ == "__main__":
    main()
