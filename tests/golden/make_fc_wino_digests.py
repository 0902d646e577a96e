#!/usr/bin/env python3
"""Write tests/golden/fc_wino_digests.json: SHA-256 of every output of tests/fc_wino_family_util.py's cases, computed on the
GPU by the library of the checkout this script runs in.  Run it on the revision whose results are to be pinned (the parent
of a change to the Winograd-domain kernels that must not change a bit); tests/test_fc_wino_family_gpu.py recomputes the
digests and compares.  The cases go through the C entry points only, so the script runs on any revision.

Per case it prints the geometry the kernels run with, restated here from csrc/fc_wino_shared.h (wn_geometry) and
csrc/fc_wino.hip (ww_geometry, fc_wino_wgrad_splits): tiles per group, groups, span, double or single raw buffer of the
convolutions; R, nseg, units per sample, 16-tile steps per unit and units per split of the weight gradients.
That restatement is a copy for the reader's eye only -- no test depends on it -- and must be kept in step with the C when the
geometry changes: what says that a case reaches its path (one raw buffer, R > 1, several units per split) is this print-out.

Every case runs twice.  Nothing is written if a digest differs between the two runs.  The whole layer's grad_source /
grad_flow / grad_w0 (float atomics in free order) are compared too, reported, and left out of the file either way.

    python tests/golden/make_fc_wino_digests.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import fc_wino_family_util as wf  # noqa: E402
from global_flow_local_attention_amd import fc_mfma  # noqa: E402

LDS_LIMIT, V_BYTES, THREADS = 160 * 1024, 2 * 36 * 32 * 8 * 4, 512


def wn_geometry(k, M, Wv, Wp):
    m, pitch = (2, 80) if k == 5 else (4, 72)
    TH, TW = (M // Wv + m - 1) // m, (Wv + m - 1) // m
    ntiles = TH * TW

    def span(tpg):
        worst = 0
        for grp in range((ntiles + tpg - 1) // tpg):
            t0, t1 = grp * tpg, min(grp * tpg + tpg, ntiles) - 1
            r0, r1 = t0 // TW, t1 // TW
            for r in range(max(r0, r1 - 1), r1 + 1):
                c = t1 - r1 * TW if r == r1 else TW - 1
                worst = max(worst, (m * r + 5) * Wp + m * c + 5 + 1 - m * r0 * Wp)
        return worst

    tpg, ngroups, sp = 32, (ntiles + 31) // 32, span(32)
    whole = (32 // TW) * TW if TW < 32 else 32
    if whole != 32 and whole >= 28 and (ntiles + whole - 1) // whole == ngroups and span(whole) < sp:
        tpg, sp = whole, span(whole)
    raw = (sp * pitch + 15) & ~15
    exch = {"f32": THREADS * 4 * m * m * 4, "f16": 3 * 2 * 4 * m * m * 64 * 4 * (4 if m == 2 else 1)}
    db = {n: max(V_BYTES + 2 * raw, e) <= LDS_LIMIT for n, e in exch.items()}
    return "tiles %dx%d tpg %d ngroups %d span %d raw buffers %s" % (
        TH, TW, tpg, ngroups, sp, ", ".join("%s: %s" % (n, "double" if d else "single") for n, d in db.items()))


def ww_geometry(k, B, C, Ho, Wo, key29, key12):
    m, seg = (2, 32) if k == 5 else (4, 16)
    TH, TW = (Ho + m - 1) // m, (Wo + m - 1) // m
    nseg, R = (TW + seg - 1) // seg, 1
    if nseg == 1 and key29 != 1:
        def steps(r):
            return (TH // r) * ((r * TW + 15) // 16) + (((TH % r) * TW + 15) // 16 if TH % r else 0)
        best = steps(1)
        for r in range(2, TH + 1):
            px = (m * r + 6 - m) * (m * TW + 6 - m)
            if r * TW > (16 if key29 == 2 else 1 << 20) or px * 72 > 43 * 1024 or px * 4 > (4 if k == 5 else 5) * THREADS:
                break
            if steps(r) <= best:
                R, best = r, steps(r)
    ups = (TH + R - 1) // R if R > 1 else TH * nseg
    if R > 1:
        per_unit = sorted({(TW * min(R, TH - ty) + 15) // 16 for ty in range(0, TH, R)})
    else:
        per_unit = sorted({(min(seg, TW - s * seg) + 15) // 16 for s in range(nseg)})
    units = B * ups
    nsplit = min(max(key12 if key12 > 0 else 256 // ((C + 15) // 16), 1), units)
    return "tiles %dx%d R %d nseg %d ups %d steps/unit %s units %d splits %d (%.2f units/split)" % (
        TH, TW, R, nseg, ups, per_unit, units, nsplit, units / nsplit)


def print_geometry():
    for shape in wf.SHAPES + wf.LAYER_SHAPES:
        k, B, C, H, W = shape
        print("%s: runs in mode %s" % (wf.shape_id(shape), [m for m in wf.MODES if wf.runs_in(shape, m)]))
        for h in (0, 1):
            g = fc_mfma.geometry(H, W, k, h)
            print("  half %d forward conv: %s" % (h, wn_geometry(k, g["Ho"] * g["Wo"], g["Wo"], g["Wp"])))
            print("  half %d data-gradient conv: %s" % (h, wn_geometry(k, g["Md"], g["Wp"], g["Wp"])))
            for k29, k12 in wf.WGRAD_VARIANTS:
                print("  half %d weight gradient key29=%d key12=%d: %s" % (h, k29, k12, ww_geometry(k, B, C, g["Ho"], g["Wo"], k29, k12)))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "fc_wino_digests.json")
    print_geometry()
    first = wf.all_digests()
    second = wf.all_digests()
    unstable = sorted(k for k in first if first[k] != second[k])
    for k in unstable:
        print("differs between two runs: %s" % k)
    if any(k.split("/")[0] != "layer" or k.split("/")[-1] not in wf.LAYER_UNSTABLE for k in unstable):
        sys.exit("nothing written")
    pinned = {k: v for k, v in first.items() if not (k.split("/")[0] == "layer" and k.split("/")[-1] in wf.LAYER_UNSTABLE)}
    print("left out of the pinned set: %s of the whole layer (%d of them differed between the two runs)" % (
        ", ".join(wf.LAYER_UNSTABLE), len(unstable)))
    with open(out, "w") as f:
        json.dump(pinned, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(pinned), out))


if __name__ == "__main__":
    main()
