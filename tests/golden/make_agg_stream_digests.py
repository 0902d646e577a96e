#!/usr/bin/env python3
"""Write tests/golden/agg_stream_digests.json: SHA-256 of every output of tests/agg_stream_family_util.py's cases, computed
on the GPU by the library of the checkout this script runs in.  Run it on the revision whose results are to be pinned (the
parent of a change to csrc/agg_stream.h that must not change a bit); tests/test_agg_stream_family_gpu.py recomputes the
digests and compares.  The cases go through _lib.aggregate_fwd and the C entry points only, so the script runs on any
revision.

Every case runs twice.  Nothing is written if a digest differs between the two runs, or if the geometry query reports
more than two channel ranges for a gradient case (two float atomics onto a zeroed word commute; three need not).

    python tests/golden/make_agg_stream_digests.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import agg_stream_family_util as af  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "agg_stream_digests.json")
    for shape in af.SHAPES:
        for k in af.KS:
            for key5 in (0, 1, 2):
                with af._Tuning(key5):
                    print("geometry %s k=%d ranges-key=%d: %s" % (af.shape_id(shape), k, key5, af.geometry(shape, k)))
    ranges = {}
    first = af.all_digests(ranges)
    second = af.all_digests()
    unstable = sorted(k for k in first if first[k] != second[k])
    too_many = sorted(k for k, n in ranges.items() if n > 2)
    for k in unstable:
        print("differs between two runs: %s" % k)
    for k in too_many:
        print("%d channel ranges: %s" % (ranges[k], k))
    if unstable or too_many:
        sys.exit("nothing written")
    with open(out, "w") as f:
        json.dump(first, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(first), out))


if __name__ == "__main__":
    main()
