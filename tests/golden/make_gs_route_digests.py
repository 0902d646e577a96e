#!/usr/bin/env python3
"""Write tests/golden/gs_route_digests.json: per case of tests/gs_route_util.py's GPU_CASES and storage type, the returned
status, the deltas of the dispatch counters, the answer of the planes-in-LDS query and SHA-256 digests of the outputs that
cannot depend on the order of arrival (gs_route_util's docstring), computed on the GPU by the library of the checkout this
script runs in.  Run it on the revision whose routing is to be pinned; tests/test_gs_route_gpu.py recomputes and compares.

Every case runs twice.  Nothing is written if a record differs between the two runs, or if a case did not take the route
it is named for (status, counters, query class, at most two channel ranges where a digest needs that).

    python tests/golden/make_gs_route_digests.py [output.json ...]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import gs_route_util as gr  # noqa: E402


def main():
    outs = sys.argv[1:] or [os.path.join(HERE, "gs_route_digests.json")]
    pinned, bad = {}, []
    for case in gr.GPU_CASES:
        cid = gr.gpu_case_id(case)
        first, second = gr.run_gpu_case(case), gr.run_gpu_case(case)
        print("%s: %s" % (cid, {n: (r["status"], {i: d for i, d in r["paths"].items() if d}, r.get("lds"), r.get("ranges"))
                                for n, r in first.items()}), flush=True)
        if first != second:
            bad.append("differs between two runs: %s" % cid)
        try:
            gr.check_named_route(case, first)
        except AssertionError as e:
            bad.append("not the route it is named for: %s" % (e,))
        pinned[cid] = first
    for line in bad:
        print(line)
    if bad:
        sys.exit("nothing written")
    for out in outs:
        with open(out, "w") as f:
            json.dump(pinned, f, indent=0, sort_keys=True)
            f.write("\n")
    print("%d cases, %d records, %d digests -> %s" % (len(pinned), sum(len(r) for r in pinned.values()),
                                                    sum(len(x.get("digests", ())) for r in pinned.values() for x in r.values()),
                                                    ", ".join(outs)))


if __name__ == "__main__":
    main()
