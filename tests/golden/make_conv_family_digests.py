#!/usr/bin/env python3
"""Write tests/golden/conv_family_digests.json: SHA-256 of every output of tests/conv_family_util.py's cases, computed on
the GPU by the library of the checkout this script runs in.  Run it on the revision whose results are to be pinned (the
parent of a change to csrc/conv_igemm.h that must not change a bit); tests/test_conv_family_gpu.py recomputes the digests
and compares.  The cases go through the package's public functions only, so the script runs on any revision.

    python tests/golden/make_conv_family_digests.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import global_flow_local_attention_amd as gfla  # noqa: E402
import conv_family_util as cf  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "conv_family_digests.json")
    digests = {}
    for name, shape in cf.VGG_CASES:
        digests.update(cf.vgg_digests(gfla, name, shape))
    for case in cf.GEN_CASES:
        digests.update(cf.gen_digests(gfla, *case))
    with open(out, "w") as f:
        json.dump(digests, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(digests), out))


if __name__ == "__main__":
    main()
