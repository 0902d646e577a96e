"""Shared by the routing tests of the gather/scatter ops (csrc/gs_route.h): tests/test_gs_route_cpu.py with
tests/golden/make_gs_route_queries.py, and tests/test_gs_route_gpu.py with tests/golden/make_gs_route_digests.py.
Everything goes through the C entry points and the tuning keys, so the same code runs on any revision of the library.
Importing this module needs no GPU.

Part 1, host only: a sweep of the geometry / support queries over shapes, kernel sizes and tuning-key sets (`query_rows`),
one SHA-256 per (key set, query, op) over the ordered answers, and per group how many answers fall in each class.

Part 2, GPU: one case per route (`GPU_CASES`).  Per case the status, the deltas of the dispatch counters 0, 1 and 12-17, and
SHA-256 digests of the outputs whose bits cannot depend on the order in which lanes and workgroups arrive:

  every forward       no atomics: each output element is written once, by one lane, from a fixed expression.
  resample2d d/d input1, planes-in-LDS route with whole planes and split == 1 (asserted through gfla_lds_plane_geometry op 6),
  f32 / bf16 / f16    the planes are 64-bit FIXED POINT (integer adds are associative) and each plane is flushed by its sole
                      owner with plain stores or a plain read-modify-write of a zeroed buffer.  Not digested: f64 and tuning
                      key 23 = 1 (double planes, ds_add_f64 in free order), the matrix-core product with its device-side
                      switch, row windows, split > 1, the tile and the global kernels (float atomics in free order).
  resample2d d/d input2 at kernel_size 4, dilation 1, float arithmetic (the streaming kernel), tuning key 5 = 1 or 2, zeroed
  buffer              one float atomic per output element and channel range: at most two addends onto +0, and
                      a + b == b + a exactly.  The same argument as tests/agg_stream_family_util.py.
  aggregate d/d logits on the streaming kernel (k = 5, or key 8 = 2), key 5 = 1 or 2, smooth flow, zeroed buffer
                      the same: one atomic per element and range (the tap-by-tap branch of near-integer flows is avoided).

Every other gradient is published by atomics in free order (LDS double planes shared by the lanes of a workgroup, global
float atomics across channel groups) and is NOT digested; test_gpu_parity.py, test_plane_geometry_gpu.py,
test_big_plane_gpu.py, test_default_path_gpu.py, test_agg_stream_family_gpu.py and test_f16_gpu.py remain their check.  For
those cases the status and the counters are what is pinned.

What a case can show of its route: the dispatch counters exist for block_extractor's backward kernels (0, 1, 14), its
forward kernels with a compile-time kernel size (12: wave-per-row AND lane-per-pixel; 13: both big-plane versions) and
resample2d's big-plane kernels (15-17); gfla_lds_plane_geometry tells whether a planes-in-LDS kernel takes the call and with
which planes; gfla_aggregate_fwd_geometry tells whether the streaming kernels CAN take a shape (`stream` / `stream_ranges`
cases assert it).  The selection of these routes leaves no trace that the entry points expose, and a case named for one of
them pins its status and outputs only: wave-per-row against lane-per-pixel (both id 12) and tiles against their first
version (both id 13); round 1's planes-in-LDS forward against the global-gather forward (keys 0 = 2 / 0 = 1, 16-bit
storage, k outside 2-5: identical results, no counter); unfold forward / backward and source_bwd (one route each); the
aggregation's forward and backward among streaming, planes-in-LDS and global kernels beyond what the geometry query says;
the matrix-core product and whether its device-side switch took the call; FIX / TAB of resample2d's scatter.

Shapes: the smallest that reach each route through the existing tuning keys (S, R, W and the three flow widths below); the
pinned revision reached every named route with them, so no case needed a larger one."""
import ctypes
import hashlib

from global_flow_local_attention_amd import _lib
from global_flow_local_attention_amd._lib import (TUNE_AGG, TUNE_BE_BWD, TUNE_BE_FWD, TUNE_BIG_GATHER_V1, TUNE_BIG_PLANE, TUNE_G_CAP,
                                                  TUNE_LDS_KB, TUNE_NO_WINDOWS, TUNE_RS, TUNE_RS_BWD1_PLANES, TUNE_RS_BWD2_NO_STREAM,
                                                  TUNE_SPLIT)

# ------------------------------------------------------------------------------------------------------------ part 1: queries
# (B, C, Hs, Ws, H, W): from one tiny plane up to the bench shapes, a map whose planes are beyond the default budget with
# enough of them to stay out of the big-plane regime (row windows by default), and a flow grid smaller than the source
SHAPES = [(1, 1, 6, 8, 6, 8), (2, 5, 12, 10, 12, 10), (1, 3, 32, 30, 32, 30), (2, 7, 80, 60, 40, 30), (2, 7, 80, 60, 80, 60),
          (3, 40, 64, 64, 64, 64), (8, 128, 128, 96, 128, 96), (32, 128, 64, 44, 64, 44), (32, 256, 32, 22, 32, 22),
          (1, 64, 256, 176, 256, 176), (1, 3, 256, 256, 256, 256)]
KS = (1, 2, 3, 4, 5, 6)
RS_KD = ((2, 1), (4, 1), (4, 2), (5, 1))
KEY_SETS = [{}, {TUNE_LDS_KB: 16}, {TUNE_LDS_KB: 160}, {TUNE_BIG_PLANE: 1}, {TUNE_BIG_PLANE: 2}, {TUNE_BE_BWD: 1}, {TUNE_AGG: 1},
            {TUNE_RS: 1}, {TUNE_G_CAP: 1}, {TUNE_SPLIT: 3}, {TUNE_LDS_KB: 16, TUNE_SPLIT: 2}, {TUNE_LDS_KB: 16, TUNE_BIG_PLANE: 1},
            {TUNE_LDS_KB: 16, TUNE_BIG_PLANE: 2}, {TUNE_NO_WINDOWS: 1, TUNE_LDS_KB: 16}]
LDS_OPS = range(8)
WINDOW_OPS = (0, 5, 6, 7)   # the ops of gfla_lds_plane_geometry whose kernels can keep a row window
CLASSES = ("not_taken", "whole", "window", "split")   # split: whole planes shared by split > 1 workgroups


def key_set_id(keys):
    return ",".join("%d=%d" % kv for kv in sorted(keys.items())) or "default"


def _lds(op, shape, k, dil, elem, needs):
    out = (ctypes.c_int64 * 6)()
    st = _lib.lib().gfla_lds_plane_geometry(op, *shape, k, dil, elem, needs, out)
    return (st,) + tuple(out)


def lds_class(ans):
    """class of one gfla_lds_plane_geometry answer (status, G, groups, split, per, margin, lds_bytes)"""
    st, G, _, split, _, margin, _ = ans
    if st != 0 or G == 0:
        return "not_taken"
    if margin >= 0:   # (a row window is one band of flow rows per workgroup: split > 1 nearly always)
        return "window"
    return "split" if split > 1 else "whole"


def query_rows():
    """{(query, op): [(arguments, answer), ...]} under the tuning keys as they are, in a fixed order"""
    lib = _lib.lib()
    rows = {}
    for op in LDS_OPS:
        r = rows[("lds_plane_geometry", op)] = []
        for shape in SHAPES:
            for k, dil in (RS_KD if op >= 5 else [(k, 1) for k in KS]):
                for elem in (2, 4, 8):
                    for needs in (1, 2, 3):
                        r.append(((shape, k, dil, elem, needs), _lds(op, shape, k, dil, elem, needs)))
    for op in range(5):
        r = rows[("big_plane_geometry", op)] = []
        for shape in SHAPES:
            for span in sorted({k + 1 for k in KS} if op < 2 else {(k - 1) * d + 1 for k, d in RS_KD}):
                for elem in (4, 8):
                    out = (ctypes.c_int64 * 10)()
                    st = lib.gfla_big_plane_geometry(op, *shape, span, elem, out)
                    r.append(((shape, span, elem), (st,) + tuple(out)))
    r = rows[("unfold_supported", 0)] = []
    a = rows[("aggregate_bwd_supported", 0)] = []
    for shape in SHAPES:
        for elem in (2, 4, 8):
            a.append(((shape[2:4], elem), (lib.gfla_aggregate_bwd_supported(shape[2], shape[3], elem),)))
            for k in KS:
                r.append(((shape[2:4], k, elem), (lib.gfla_unfold_supported(shape[2], shape[3], k, elem),)))
    r = rows[("aggregate_fwd_geometry", 0)] = []
    for shape in SHAPES:
        for k in KS:
            out = (ctypes.c_int64 * 9)()
            st = lib.gfla_aggregate_fwd_geometry(*shape, k, out)
            r.append(((shape, k), (st,) + (tuple(out) if st == 0 else ())))
    return rows


def answer_class(query, ans):
    if query == "lds_plane_geometry":
        return lds_class(ans)
    if query == "big_plane_geometry":
        return "in_regime" if ans[1] else "outside"
    if query == "aggregate_fwd_geometry":
        return "taken" if ans[0] == 0 else "not_taken"
    return "supported" if ans[0] else "not_supported"


def group_id(keys, query, op):
    return "%s/%s/%d" % (key_set_id(keys), query, op)


def sweep():
    """{group: {"sha256": ..., "classes": {class: count}, "queries": n}} over KEY_SETS, and the rows per group"""
    groups, all_rows = {}, {}
    for keys in KEY_SETS:
        with _lib.tuned(keys):
            rows = query_rows()
        for (query, op), r in rows.items():
            classes = {}
            for _, ans in r:
                c = answer_class(query, ans)
                classes[c] = classes.get(c, 0) + 1
            text = "\n".join("%r -> %r" % row for row in r)
            gid = group_id(keys, query, op)
            groups[gid] = {"sha256": hashlib.sha256(text.encode()).hexdigest(), "classes": classes, "queries": len(r)}
            all_rows[gid] = r
    return groups, all_rows


# -------------------------------------------------------------------------------------------------------- part 2: GPU cases
DEV = "cuda:0"
PATH_IDS = (0, 1, 12, 13, 14, 15, 16, 17)
S = (2, 5, 12, 10, 12, 10)       # default planes-in-LDS routes; lane-per-pixel forward; five channels: ragged groups under {4:2}
R = (1, 3, 32, 30, 32, 30)       # output planes beyond 32 KB at k = 3: the wave-per-flow-row forward
W = (2, 7, 80, 60, 40, 30)       # planes beyond a 16 KB budget, few of them: row windows under {30:1}, tiles without
F32, F64, BF16, F16 = "f32", "f64", "bf16", "f16"
ALL, HALVES = (F32, F64, BF16, F16), (BF16, F16)
UNSUPPORTED = -3


def _w(width):
    return (2, 5, 12, width, 12, width)


def _case(op, shape, dtypes, keys=None, k=3, dil=1, status=0, paths=None, lds=None, digest=(), **extra):
    """One case: `op` on `shape` in each storage type of `dtypes` under the tuning keys `keys`.  What the generator asserts
    on the pinned revision, i.e. what the case is named for: the status, the dispatch counters that move (`paths`: id ->
    delta; every other counted id stays), `lds` = (op of gfla_lds_plane_geometry, class) and the outputs in `digest`."""
    return dict(op=op, shape=shape, dtypes=tuple(dtypes), keys=keys or {}, k=k, dil=dil, status=status, paths=paths or {}, lds=lds,
                digest=tuple(digest), **extra)


def _be_cases():
    c = []
    fwd = ("out",)
    # forward: lane-per-pixel (f32 / f64), round 1's planes-in-LDS kernel (16-bit storage); ragged last channel group
    for keys in ({}, {TUNE_G_CAP: 2}):
        c.append(_case("be_fwd", S, (F32, F64), keys, paths={12: 1}, digest=fwd))
        c.append(_case("be_fwd", S, HALVES, keys, digest=fwd))
    c.append(_case("be_fwd", R, (F32, F64), paths={12: 1}, digest=fwd))                       # wave per flow row
    for width in (10, 11, 12):                                                                # V = 2, 1, 4 outputs per lane
        c.append(_case("be_fwd", _w(width), (BF16,), digest=fwd))
        c.append(_case("be_fwd", _w(width), (F32,), {TUNE_BE_FWD: 2}, digest=fwd))   # round 1's planes in LDS
        c.append(_case("be_fwd", _w(width), (F32,), {TUNE_BE_FWD: 1}, digest=fwd))   # global gathers
    c.append(_case("be_fwd", S, (F32,), {TUNE_BE_FWD: 4}, paths={12: 1}, digest=fwd))
    c.append(_case("be_fwd", S, (F32, F64), {TUNE_BE_FWD: 2}, digest=fwd))
    c.append(_case("be_fwd", S, (F32, BF16), k=1, digest=fwd))                                # no compile-time kernel size
    c.append(_case("be_fwd", S, (F32,), k=6, digest=fwd))
    c.append(_case("be_fwd", W, (F32, BF16), {TUNE_LDS_KB: 16, TUNE_BIG_PLANE: 1}, digest=fwd))   # row windows
    c.append(_case("be_fwd", W, (F32, F64), {TUNE_LDS_KB: 16}, paths={13: 1}, digest=fwd))   # tiles
    c.append(_case("be_fwd", W, (F32,), {TUNE_LDS_KB: 16, TUNE_BIG_GATHER_V1: 1}, paths={13: 1}, digest=fwd))   # the tiles' first version
    c.append(_case("be_fwd", S, (F32,), {TUNE_BIG_PLANE: 2}, paths={13: 1}, digest=fwd))
    # backward: no gradient is digested (double LDS planes and d/d flow across >= 3 channel groups: free-order atomics)
    for keys in ({}, {TUNE_G_CAP: 2}):
        c.append(_case("be_bwd", S, ALL, keys, paths={0: 1}, lds=(0, "whole")))
    c.append(_case("be_bwd", W, (F32,), {TUNE_LDS_KB: 16, TUNE_BIG_PLANE: 1}, paths={0: 1}, lds=(0, "window")))
    c.append(_case("be_bwd", W, (F32, F64), {TUNE_LDS_KB: 16}, paths={14: 1}, lds=(0, "not_taken")))
    c.append(_case("be_bwd", S, (F32,), {TUNE_BIG_PLANE: 2}, paths={14: 1}, lds=(0, "not_taken")))
    c.append(_case("be_bwd", S, (F32, F64), {TUNE_BE_BWD: 1}, paths={1: 1}, lds=(0, "not_taken")))
    c.append(_case("be_bwd", S, HALVES, {TUNE_BE_BWD: 1}, paths={0: 1}, lds=(0, "whole")))   # 16-bit storage ignores key 2
    c.append(_case("be_bwd", S, (F32,), k=6, lds=(0, "not_taken")))                            # the per-element kernel
    c.append(_case("be_bwd", S, HALVES, k=6, status=UNSUPPORTED, lds=(0, "not_taken")))
    c.append(_case("be_bwd", W, HALVES, {TUNE_LDS_KB: 16}, status=UNSUPPORTED, lds=(0, "not_taken")))   # beyond the LDS budget
    for layout in (0, 1):
        c.append(_case("unfold_fwd", S, ALL, layout=layout, lds=(4, "whole"), digest=fwd))
        c.append(_case("unfold_bwd", S, ALL, layout=layout, lds=(2, "whole")))
    c.append(_case("unfold_fwd", S, (F32,), {TUNE_G_CAP: 2}, layout=0, lds=(4, "whole"), digest=fwd))
    c.append(_case("unfold_bwd", W, (BF16, F32), {TUNE_LDS_KB: 16}, layout=0, status=UNSUPPORTED, lds=(2, "not_taken")))
    c.append(_case("unfold_bwd", S, (BF16,), k=6, layout=0, status=UNSUPPORTED, lds=(2, "not_taken")))
    for mode, op in (("unfold", 2), ("attn", 1), ("both", 3)):
        c.append(_case("source_bwd", S, (F32, F64, BF16), mode=mode, layout=0, lds=(op, "whole")))
    c.append(_case("source_bwd", S, (F32,), mode="both", layout=1, lds=(3, "whole")))
    return c


def _rs_cases():
    c = []
    fwd, g1, g2 = ("out",), ("grad_in1",), ("grad_in2",)
    c.append(_case("rs_fwd", S, ALL, k=4, lds=(5, "whole"), digest=fwd))
    c.append(_case("rs_fwd", S, (F32,), {TUNE_G_CAP: 2}, k=4, lds=(5, "whole"), digest=fwd))
    for k, dil in ((2, 1), (4, 2), (5, 1)):
        c.append(_case("rs_fwd", S, (F32,), k=k, dil=dil, lds=(5, "whole"), digest=fwd))
    c.append(_case("rs_fwd", S, (F32, F64), {TUNE_RS: 1}, k=4, lds=(5, "not_taken"), digest=fwd))   # global kernel
    c.append(_case("rs_fwd", W, (F32, BF16), {TUNE_LDS_KB: 16, TUNE_BIG_PLANE: 1}, k=4, lds=(5, "window"), digest=fwd))
    c.append(_case("rs_fwd", W, (F32, F64), {TUNE_LDS_KB: 16}, k=4, paths={15: 1}, lds=(5, "not_taken"), digest=fwd))  # gather tiles
    c.append(_case("rs_fwd", S, (F32, BF16), {TUNE_BIG_PLANE: 2}, k=4, paths={15: 1}, lds=(5, "not_taken"), digest=fwd))  # bf16: global gathers
    c.append(_case("rs_fwd", S, (F32,), {TUNE_BIG_PLANE: 2, TUNE_BIG_GATHER_V1: 1}, k=4, paths={15: 1}, lds=(5, "not_taken"), digest=fwd))
    c.append(_case("rs_fwd", S, (F32, BF16), k=10, status=UNSUPPORTED))
    # d/d input1.  Digested: fixed-point planes flushed by their sole owner (module docstring)
    for trunc in (0, 1, 2, 3):
        c.append(_case("rs_bwd", S, (F32,), k=4, trunc=trunc, want=(1, 0), lds=(6, "whole"), digest=g1))
        c.append(_case("rs_bwd", S, (F32,), k=4, trunc=trunc, want=(1, 0), ws=True, lds=(6, "whole")))      # matrix-core product
    for trunc in (0, 2):
        c.append(_case("rs_bwd", S, (F32,), k=4, dil=2, trunc=trunc, want=(1, 0), ws=True, lds=(6, "whole"), digest=g1))  # tap records
        c.append(_case("rs_bwd", S, HALVES, k=4, trunc=trunc, want=(1, 0), lds=(6, "whole"), digest=g1))
        c.append(_case("rs_bwd", S, (F64,), k=4, trunc=trunc, want=(1, 0), lds=(6, "whole")))
        c.append(_case("rs_bwd", S, (F32,), {TUNE_RS_BWD1_PLANES: 1}, k=4, trunc=trunc, want=(1, 0), lds=(6, "whole")))   # double planes
        c.append(_case("rs_bwd", S, (F32,), {TUNE_RS_BWD1_PLANES: 2}, k=4, dil=2, trunc=trunc, want=(1, 0), ws=True, lds=(6, "whole"), digest=g1))
    c.append(_case("rs_bwd", S, (F32,), {TUNE_RS_BWD1_PLANES: 2}, k=4, trunc=2, want=(1, 0), ws=True, lds=(6, "whole")))
    c.append(_case("rs_bwd", S, (F32,), {TUNE_SPLIT: 3}, k=4, trunc=2, want=(1, 0), lds=(6, "split")))   # zero-filled first
    c.append(_case("rs_bwd", S, (F32,), {TUNE_SPLIT: 3}, k=4, trunc=2, want=(1, 0), ws=True, lds=(6, "split")))
    c.append(_case("rs_bwd", S, (F32, F64), {TUNE_RS: 1}, k=4, trunc=2, want=(1, 1), lds=(6, "not_taken")))   # global kernels
    c.append(_case("rs_bwd", S, HALVES, {TUNE_RS: 1}, k=4, trunc=2, want=(1, 1), lds=(6, "whole")))   # ignore key 6
    c.append(_case("rs_bwd", W, (F32,), {TUNE_LDS_KB: 16, TUNE_BIG_PLANE: 1}, k=4, trunc=2, want=(1, 1), lds=(6, "window")))
    c.append(_case("rs_bwd", W, (F32,), {TUNE_LDS_KB: 16, TUNE_BIG_PLANE: 1}, k=4, trunc=2, want=(1, 0), ws=True, lds=(6, "window")))
    c.append(_case("rs_bwd", W, (F32, F64), {TUNE_LDS_KB: 16}, k=4, trunc=2, want=(1, 1), paths={16: 1, 17: 1}, lds=(6, "not_taken")))
    c.append(_case("rs_bwd", W, (F32,), {TUNE_LDS_KB: 16}, k=4, trunc=2, want=(1, 1), ws=True, paths={16: 1, 17: 1}, lds=(6, "not_taken")))
    c.append(_case("rs_bwd", W, (F32,), {TUNE_LDS_KB: 16, TUNE_BIG_GATHER_V1: 1}, k=4, trunc=0, want=(0, 1), paths={17: 1}, lds=(7, "not_taken")))
    c.append(_case("rs_bwd", S, (F32,), {TUNE_BIG_PLANE: 2}, k=4, trunc=2, want=(1, 0), paths={16: 1}, lds=(6, "not_taken")))
    c.append(_case("rs_bwd", W, HALVES, {TUNE_LDS_KB: 16}, k=4, trunc=0, want=(1, 1), status=UNSUPPORTED, lds=(6, "not_taken")))
    c.append(_case("rs_bwd", S, (F32, BF16), k=10, trunc=0, want=(1, 1), status=UNSUPPORTED))
    # d/d input2 at kernel_size 4, dilation 1: the streaming kernel (digested where it has at most two channel ranges), and
    # rs_lds_kernel under key 22 = 1 and for f64 / dilation 2 (three atomics per lane and channel group: not digested)
    c.append(_case("rs_bwd", S, (F32, BF16, F16), k=4, want=(0, 1), lds=(7, "whole"), digest=g2, stream_ranges=True))
    c.append(_case("rs_bwd", S, (F32, BF16), {TUNE_RS_BWD2_NO_STREAM: 1}, k=4, want=(0, 1), lds=(7, "whole")))
    c.append(_case("rs_bwd", S, (F64,), k=4, want=(0, 1), lds=(7, "whole")))
    c.append(_case("rs_bwd", S, (F32,), k=4, dil=2, want=(0, 1), lds=(7, "whole")))
    c.append(_case("rs_bwd", S, (F32, BF16), k=4, want=(1, 1), lds=(7, "whole")))
    return c


def _agg_cases():
    c = []
    fwd = ("out", "attn")
    for k in (3, 5):
        c.append(_case("agg_fwd", S, (F32, BF16, F16), k=k, ws=True, digest=fwd, stream=k == 5))   # k = 5: table + streaming kernel
        c.append(_case("agg_fwd", S, (F32, F64, BF16), k=k, digest=fwd))
        c.append(_case("agg_fwd", S, (F32,), {TUNE_AGG: 1}, k=k, ws=True, digest=fwd))   # global kernel
        c.append(_case("agg_fwd", S, (F32,), {TUNE_G_CAP: 2}, k=k, digest=fwd))
        # backward: d/d logits is digested where it comes from the streaming kernel with at most two channel ranges
        c.append(_case("agg_bwd", S, (F32,), k=k, ws=True, digest=("grad_logits",) if k == 5 else (), stream_ranges=k == 5))
        c.append(_case("agg_bwd", S, (F32, BF16, F16), k=k, digest=("grad_logits",) if k == 5 else (), stream_ranges=k == 5))
        c.append(_case("agg_bwd", S, (F64,), k=k))
        c.append(_case("agg_bwd", S, (F32,), {TUNE_AGG: 1}, k=k, ws=True))   # global kernel
        c.append(_case("agg_bwd", S, (BF16,), {TUNE_AGG: 1}, k=k))   # 16-bit storage ignores key 3
    c.append(_case("agg_bwd", W, HALVES, {TUNE_LDS_KB: 16}, status=UNSUPPORTED))
    c.append(_case("agg_bwd", W, (F32,), {TUNE_LDS_KB: 16}))   # the global kernel behind the LDS ones
    c.append(_case("agg_bwd", W, (F32,), {TUNE_LDS_KB: 16}, ws=True))
    return c


GPU_CASES = _be_cases() + _rs_cases() + _agg_cases()


def gpu_case_id(case):
    extra = ["%s=%s" % (n, case[n]) for n in ("layout", "mode", "trunc", "want", "ws") if n in case]
    return "-".join([case["op"], "x".join(map(str, case["shape"])), "k%dd%d" % (case["k"], case["dil"]), key_set_id(case["keys"])] +
                    [e.replace(" ", "") for e in extra] + ["+".join(case["dtypes"])])


def digest(t):
    """SHA-256 of the raw bytes of t + 0 (a signed zero cannot matter)"""
    import torch
    return hashlib.sha256((t + 0).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


_INPUTS = {}


def _inputs(shape, k):
    """Seeded float32 host tensors, made once per (shape, k): source, flow, sigma map, logits, upstream gradients"""
    import torch
    from util import make_flow, randn
    if (shape, k) not in _INPUTS:
        B, C, Hs, Ws, H, Wd = shape
        seed = 100 * sum(shape) + k
        flow = make_flow("coherent", B, H, Wd, seed=seed + 1)
        _INPUTS[(shape, k)] = dict(
            src=randn((B, C, Hs, Ws), seed=seed), flow=flow,
            in2=torch.cat((flow, torch.full((B, 1, H, Wd), 1.5)), 1).contiguous(),
            logits=randn((B, k * k, H, Wd), seed=seed + 2) * 2, g_map=randn((B, C, H, Wd), seed=seed + 3),
            g_blocks=randn((B, C, k * H, k * Wd), seed=seed + 4), g_unfold=randn((B, C * k * k, H, Wd), seed=seed + 5))
    return _INPUTS[(shape, k)]


def _run(case, name):
    """(status, {output name: tensor}) of one case in storage type `name`, under the case's tuning keys"""
    import torch
    dt = {F32: torch.float32, F64: torch.float64, BF16: torch.bfloat16, F16: torch.float16}[name]
    red = torch.float32 if name in HALVES else dt   # gradients that are reductions over channels
    shape, k, dil, op = case["shape"], case["k"], case["dil"], case["op"]
    B, C, Hs, Ws, H, Wd = shape
    x = {n: t.to(dt).to(DEV) for n, t in _inputs(shape, k).items()}
    p, lib = _lib.ptr, _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    zeros = lambda *s, dtype=dt: torch.zeros(s, dtype=dtype, device=DEV)      # noqa: E731
    garbage = lambda *s: torch.full(s, float("nan"), dtype=dt, device=DEV)    # noqa: E731
    out = {}
    if op == "be_fwd":
        out["out"] = garbage(B, C, k * H, k * Wd)
        st = getattr(lib, "gfla_block_extractor_fwd_" + name)(p(x["src"]), p(x["flow"]), p(out["out"]), *shape, k, stream)
    elif op == "be_bwd":
        out["grad_source"], out["grad_flow"] = zeros(B, C, Hs, Ws), zeros(B, 2, H, Wd, dtype=red)
        st = getattr(lib, "gfla_block_extractor_bwd_" + name)(p(x["src"]), p(x["flow"]), p(x["g_blocks"]), p(out["grad_source"]),
                                                             p(out["grad_flow"]), *shape, k, stream)
    elif op == "unfold_fwd":
        out["out"] = garbage(*((C * k * k, B) if case["layout"] else (B, C * k * k)), H, Wd)
        st = getattr(lib, "gfla_block_extractor_unfold_fwd_" + name)(p(x["src"]), p(x["flow"]), p(out["out"]), *shape, k,
                                                                    case["layout"], stream)
    elif op == "unfold_bwd":
        gu = x["g_unfold"].transpose(0, 1).contiguous() if case["layout"] else x["g_unfold"]
        out["grad_source"], out["grad_flow"] = zeros(B, C, Hs, Ws), zeros(B, 2, H, Wd, dtype=red)
        st = getattr(lib, "gfla_block_extractor_unfold_bwd_" + name)(p(x["src"]), p(x["flow"]), p(gu), p(out["grad_source"]),
                                                                    p(out["grad_flow"]), *shape, k, case["layout"], stream)
    elif op == "source_bwd":
        gu = x["g_unfold"].transpose(0, 1).contiguous() if case["layout"] else x["g_unfold"]
        attn = torch.softmax(x["logits"].float(), 1).to(dt)
        use_u, use_a = case["mode"] in ("unfold", "both"), case["mode"] in ("attn", "both")
        out["grad_source"], out["grad_flow"] = zeros(B, C, Hs, Ws), zeros(B, 2, H, Wd, dtype=red)
        st = getattr(lib, "gfla_local_attn_source_bwd_" + name)(
            p(x["src"]), p(x["flow"]), p(gu) if use_u else None, p(attn) if use_a else None, p(x["g_map"]) if use_a else None,
            p(out["grad_source"]), p(out["grad_flow"]), *shape, k, case["layout"], stream)
    elif op == "rs_fwd":
        out["out"] = garbage(B, C, H, Wd)
        st = getattr(lib, "gfla_resample2d_fwd_" + name)(p(x["src"]), p(x["in2"]), p(out["out"]), *shape, k, dil, stream)
    elif op == "rs_bwd":
        want1, want2 = case["want"]
        trunc = case.get("trunc", 0)
        if want1:   # flag bit 1: grad_in1 arrives uninitialised and is to be overwritten
            out["grad_in1"] = garbage(B, C, Hs, Ws) if trunc & 2 else zeros(B, C, Hs, Ws)
        if want2:
            out["grad_in2"] = zeros(B, 3, H, Wd, dtype=red)
        args = (p(x["src"]), p(x["in2"]), p(x["g_map"]), p(out.get("grad_in1")), p(out.get("grad_in2")))
        if case.get("ws"):
            ws = _lib.scatter_workspace(x["src"], B, H, Wd, k * k)
            st = lib.gfla_resample2d_bwd_ws_f32(*args, p(ws), *shape, k, dil, trunc, stream)
        else:
            st = getattr(lib, "gfla_resample2d_bwd_" + name)(*args, *shape, k, dil, trunc, stream)
    elif op == "agg_fwd":
        out["out"], out["attn"] = garbage(B, C, H, Wd), garbage(B, k * k, H, Wd)
        args = (p(x["src"]), p(x["flow"]), p(x["logits"]), p(out["out"]), p(out["attn"]))
        if case.get("ws"):
            ws = _lib.workspace("gfla_aggregate_fwd_workspace_bytes", x["src"], B, H, Wd, k, what="local_attn_aggregate")
            st = getattr(lib, "gfla_local_attn_aggregate_fwd_ws_" + name)(*args, p(ws), *shape, k, 1, stream)
        else:
            st = getattr(lib, "gfla_local_attn_aggregate_fwd_" + name)(*args, *shape, k, 1, stream)
    elif op == "agg_bwd":
        attn = torch.softmax(x["logits"].float(), 1).to(dt)
        out["grad_source"], out["grad_flow"] = zeros(B, C, Hs, Ws), zeros(B, 2, H, Wd, dtype=red)
        out["grad_logits"] = zeros(B, k * k, H, Wd, dtype=red)
        args = (p(x["src"]), p(x["flow"]), p(attn), p(x["g_map"]), p(out["grad_source"]), p(out["grad_flow"]), p(out["grad_logits"]))
        if case.get("ws"):
            ws = _lib.scatter_workspace(x["src"], B, H, Wd, (k + 1) * (k + 1))
            st = lib.gfla_local_attn_aggregate_bwd_ws_f32(*args, p(ws), *shape, k, 1, stream)
        else:
            st = getattr(lib, "gfla_local_attn_aggregate_bwd_" + name)(*args, *shape, k, 1, stream)
    else:
        raise ValueError(op)
    torch.cuda.synchronize()
    return st, out


def run_gpu_case(case):
    """{storage type: record} of one case; record = status, dispatch-counter deltas, the planes-in-LDS query's answer, the
    channel ranges of the streaming kernel (where a digest depends on them) and the digests of the case's order-independent
    outputs (only where the call succeeded)."""
    records = {}
    with _lib.tuned(case["keys"]):
        for name in case["dtypes"]:
            elem = {F32: 4, F64: 8, BF16: 2, F16: 2}[name]
            before = [_lib.path_count(i) for i in PATH_IDS]
            st, out = _run(case, name)
            rec = {"status": st, "paths": {str(i): _lib.path_count(i) - b for i, b in zip(PATH_IDS, before)}}
            if case["lds"]:
                rec["lds"] = list(_lds(case["lds"][0], case["shape"], case["k"], case["dil"], elem, 3))
            if case.get("stream"):   # the streaming kernels take the shape (asserted here, under the case's keys; not recorded)
                assert _lib.lib().gfla_aggregate_fwd_geometry(*case["shape"], case["k"], (ctypes.c_int64 * 9)()) == 0, gpu_case_id(case)
            if case.get("stream_ranges"):
                geo = (ctypes.c_int64 * 9)()
                kk = 3 if case["op"] == "rs_bwd" else case["k"]   # resample2d at kernel_size 4 is a K = 3 patch
                ok = _lib.lib().gfla_aggregate_fwd_geometry(*case["shape"], kk, geo)
                rec["ranges"] = int(geo[2]) if ok == 0 else 0
            if st == 0:
                rec["digests"] = {n: digest(out[n]) for n in case["digest"]}
            records[name] = rec
    return records


def check_named_route(case, records):
    """What the case is named for (asserted by the generator on the pinned revision, and by the test)"""
    for name, rec in records.items():
        what = "%s %s" % (gpu_case_id(case), name)
        assert rec["status"] == case["status"], (what, rec["status"])
        want = {str(i): case["paths"].get(i, 0) if case["status"] == 0 else 0 for i in PATH_IDS}
        assert rec["paths"] == want, (what, rec["paths"])
        if case["lds"]:
            assert lds_class(rec["lds"]) == case["lds"][1], (what, rec["lds"])
        if case.get("stream_ranges"):
            assert 1 <= rec["ranges"] <= 2, (what, rec["ranges"])
