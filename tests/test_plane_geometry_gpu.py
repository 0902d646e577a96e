"""The planes-in-LDS kernels (csrc/lds_plane.h) over the launch geometries their heuristics do not pick at small shapes --
channel planes per workgroup G in {1, 2, 3} with a ragged last group, split in {1, 2, 3}, whole planes and row windows --
forced through the tuning keys 4 (cap on G), 5 (split) and 10 (LDS budget), in float32, float64, float16 and bfloat16.

Every result is compared per element with a float64 evaluation from the stored inputs under the derived bar of
tests/plane_util.py (no fitted tolerance); d/d flow entries on a kink are left out (tests/test_plane_geometry_cpu.py caps
their share on these very inputs), nothing is ever left out of a forward result or a feature-map gradient.  Before a case
compares anything it asks gfla_lds_plane_geometry whether the geometry it meant is the one in force, and the dispatch trace
whether the family ran.  Forward results must not change by a bit with G and split: the forwards have no atomics.

No case sets key 5 together with 16-bit storage.  Key 10 = 16 goes with key 30 = 1 (plane_util.WINDOWS): with key 10 alone
the few planes of these shapes would go to the tile kernels of csrc/tile_map.h instead of row windows."""
import pytest
import torch

import plane_util as pu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
NAMES = {F32: "f32", F64: "f64", F16: "f16", BF16: "bf16"}
GEOS_WIDE = [{}, {4: 2}, {4: 3}, {4: 2, 5: 2}, {4: 3, 5: 3}, dict(pu.WINDOWS), dict(list(pu.WINDOWS.items()) + [(4, 2)])]
GEOS_HALF = [{}, {4: 2}, {4: 3}, dict(pu.WINDOWS)]       # never key 5: the 16-bit backward cannot split
CASES = [(dt, g) for dt in (F32, F64) for g in range(len(GEOS_WIDE))] + [(dt, g) for dt in (F16, BF16) for g in range(len(GEOS_HALF))]
CASE_IDS = ["%s-geo%d" % (NAMES[dt], g) for dt, g in CASES]
NO_SPLIT_16 = (0, 1, 2, 3, 6)          # query ops whose 16-bit kernels own their planes


def geo_of(dtype, g):
    return dict((GEOS_HALF if dtype in (F16, BF16) else GEOS_WIDE)[g])


def kinds_of(dtype):
    return pu.KINDS16 if dtype in (F16, BF16) else pu.KINDS


def elem_of(dtype):
    return torch.empty(0, dtype=dtype).element_size()


# ---------------------------------------------------------------------------------------------- references, computed once
_REF = {}


def cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def be_case(shape, dtype, kind, k):
    def make():
        s, f, up = pu.inputs("be", shape, dtype, kind, k)
        return {"in": (s, f, up), "ref": pu.block_extractor(s, f, up, k), "P": pu.coordinate_bound(f, k),
                "keep": ~pu.be_flow_kinks(f, k, shape[2], shape[3], pu.ARITH[dtype])}
    return cached(("be", shape, dtype, kind, k), make)


def unfold_case(shape, dtype, kind, k):
    def make():
        s, f, up = pu.inputs("unfold", shape, dtype, kind, k)
        r = pu.block_extractor(s, f, pu.patches_from_unfold(up.double(), k), k)
        r["out"] = (pu.unfold_from_patches(r["out"][0], k), pu.unfold_from_patches(r["out"][1], k), 4)
        return {"in": (s, f, up), "ref": r, "P": pu.coordinate_bound(f, k),
                "keep": ~pu.be_flow_kinks(f, k, shape[2], shape[3], pu.ARITH[dtype])}
    return cached(("unfold", shape, dtype, kind, k), make)


def agg_case(shape, dtype, kind, k):
    def make():
        s, f, lg, up = pu.inputs("agg", shape, dtype, kind, k)
        return {"in": (s, f, lg, up), "ref": pu.aggregate_forward(s, f, lg, k), "P": pu.coordinate_bound(f, k),
                "keep": ~pu.be_flow_kinks(f, k, shape[2], shape[3], pu.ARITH[dtype])}
    return cached(("agg", shape, dtype, kind, k), make)


def rs_case(shape, dtype, kind, k, dil):
    def make():
        s, f, up = pu.inputs("rs", shape, dtype, kind, k)
        r = pu.resample2d(s, f, up, k, dil)
        return {"in": (s, f, up), "ref": r, "P": pu.coordinate_bound(f, (k // 2) * dil) * pu.rs_kappa(k, dil) ** 2,
                "keep": ~pu.rs_flow_kinks(f, k, dil, shape[2], shape[3], pu.ARITH[dtype])}
    return cached(("rs", shape, dtype, kind, k, dil), make)


# ------------------------------------------------------------------------------------------------------------- the harness
class Report(object):
    """Collects every comparison of one test, prints each figure, fails at the end with all of them"""

    def __init__(self, what):
        self.what, self.bad, self.worst = what, [], {}

    def compare(self, name, got, entry, P, dtype, keep=None, extra=None, tag=""):
        ref, A, n = entry
        assert got.dtype == dtype and tuple(got.shape) == tuple(ref.shape), (name, got.dtype, tuple(got.shape), tuple(ref.shape))
        ratio, beyond = pu.worst(got, ref, A, n, P, dtype, keep, extra)    # extra: resample2d's fixed-point planes
        print("  %-9s %-40s err/bar %.3f" % (name, tag, ratio))
        self.worst[name] = max(self.worst.get(name, 0.0), ratio)
        if beyond:
            self.bad.append("%s %s: %d entries beyond the bar, worst err/bar %.3f" % (name, tag, beyond, ratio))

    def same_bits(self, name, got, want, tag=""):
        if not torch.equal(got, want):
            self.bad.append("%s %s: forward differs from the default geometry's in %d entries" % (name, tag, int((got != want).sum().item())))

    def finish(self):
        print("RATIO %s %s" % (self.what, " ".join("%s=%.3f" % kv for kv in sorted(self.worst.items()))))
        assert not self.bad, "\n".join([self.what] + self.bad)


def check_geometry(_lib, qop, shape, k, dil, dtype, keys, needs=3):
    """Ask the library for the geometry of this launch and assert it is the one the keys were meant to force.  Returns the
    geometry (G == 0: the family does not take the call)."""
    B, C, Hs, Ws, Hf, Wf = shape
    elem = elem_of(dtype)
    g = pu.query(_lib, qop, shape, k, dil, elem, needs)
    half_owner = elem == 2 and qop in NO_SPLIT_16
    if g["G"] == 0:      # only under the forced budget, and only kernels that need whole planes: the factored / unfold forms
        assert 10 in keys and (qop in (1, 2, 3, 4) or elem == 2), (qop, shape, keys, g)          # and 16-bit backwards
        return g
    if g["margin"] >= 0:             # row windows: only under the forced budget, never the 16-bit owner kernels
        assert 10 in keys and not half_owner and g["lds"] <= 16 * 1024 and g["split"] > 1, (qop, shape, keys, g)
        return g
    per_channel = g["lds"] // g["G"]
    budget = (16 if 10 in keys else 64) * 1024
    assert g["lds"] <= budget
    if 4 in keys:
        want = min(keys[4], C, budget // per_channel)
        assert g["G"] == want and g["ngroups"] == -(-C // want), (qop, shape, keys, g)
        assert g["ragged"] == (C % want if C % want else 0)
    else:
        assert g["G"] == 1 and g["ngroups"] == C and g["ragged"] == 0, (qop, shape, keys, g)    # the heuristics at these sizes
    if 5 in keys:
        assert elem != 2 and g["split"] == keys[5] and g["per"] == -(-Hf * Wf // keys[5]), (qop, shape, keys, g)
    else:
        assert g["split"] == (2 if Hf * Wf >= 2048 and not half_owner else 1), (qop, shape, keys, g)
    return g


def grads(fn, inputs, up, which):
    """outputs and gradients of fn on fresh leaves; `which`: indices of the inputs that require a gradient"""
    leaves = [x.to(DEV).requires_grad_(i in which) for i, x in enumerate(inputs)]
    out = fn(*leaves)
    first = out[0] if isinstance(out, tuple) else out
    first.backward(up.to(DEV))
    return out, [leaf.grad for leaf in leaves]


def default_forward(gfla, key, run, kernel=None):
    """the forward result under the default geometry (every forcing key at 0), as a host tensor; computed once per case.
    `kernel`: keys that SELECT a kernel (key 0 / key 3), for the cases where the forced LDS budget makes the dispatch hand
    the call to another kernel of the library: bit-identity is a property of one kernel over its geometries, so the result
    is then compared with that same kernel's at the default geometry."""
    def make():
        with pu.Tuning(gfla, {4: 0, 5: 0, 10: 0, 30: 0}):
            with pu.Tuning(gfla, kernel or {}):
                out = run()
        return [o.detach().cpu() for o in (out if isinstance(out, tuple) else (out,))]
    return cached(("default", tuple(sorted((kernel or {}).items()))) + key, make)


# ------------------------------------------------------------------------------------------------------ block_extractor
@pytest.mark.parametrize("dtype,geo", CASES, ids=CASE_IDS)
def test_block_extractor_over_geometries(gfla, dtype, geo):
    from global_flow_local_attention_amd import _lib
    keys = geo_of(dtype, geo)
    rep = Report("block_extractor %s %s" % (NAMES[dtype], keys))
    with pu.Tuning(gfla, keys):
        for si, shape in enumerate(pu.SHAPES):
            for k in ((2, 3, 4, 5) if si == 0 else (3, 5)):
                for kind in kinds_of(dtype):
                    c = be_case(shape, dtype, kind, k)
                    s, f, up = c["in"]
                    tag = "%s k%d %s" % (shape, k, kind)
                    check_geometry(_lib, 0, shape, k, 1, dtype, keys, 3)
                    check_geometry(_lib, 0, shape, k, 1, dtype, keys, 1)
                    check_geometry(_lib, 0, shape, k, 1, dtype, keys, 2)
                    mod = gfla.BlockExtractor(k)
                    n_b, n_f = _lib.path_count(_lib.PATH_BE_BWD_LDS), _lib.path_count(_lib.PATH_BE_FWD_PIX)
                    out, (gs, gf) = grads(mod, (s, f), up, (0, 1))
                    assert _lib.path_count(_lib.PATH_BE_BWD_LDS) == n_b + 1, "backward left the planes-in-LDS family: " + tag
                    if elem_of(dtype) >= 4 and 10 not in keys:
                        assert _lib.path_count(_lib.PATH_BE_FWD_PIX) == n_f + 1, "forward left the planes-in-LDS family: " + tag
                    rep.compare("out", out, c["ref"]["out"], c["P"], dtype, tag=tag)
                    rep.compare("g_source", gs, c["ref"]["g_source"], c["P"], dtype, tag=tag)
                    rep.compare("g_flow", gf, c["ref"]["g_flow"], c["P"], dtype, c["keep"], tag=tag)
                    # beyond the forced budget the padded planes of the lane-per-pixel / wave-per-row kernels do not fit and
                    # round 1's kernel (key 0 = 2) takes the forward, on row windows
                    other = elem_of(dtype) >= 4 and _lib.path_count(_lib.PATH_BE_FWD_PIX) == n_f
                    assert not other or 10 in keys
                    want = default_forward(gfla, ("be", shape, dtype, kind, k), lambda: mod(s.to(DEV), f.to(DEV)), {0: 2} if other else None)
                    rep.same_bits("out", out.detach().cpu(), want[0], tag)
                    if kind == "wild":      # each gradient alone: the NEED_SRC / NEED_FLOW instantiations
                        _, (gs1, _) = grads(mod, (s, f), up, (0,))
                        _, (_, gf1) = grads(mod, (s, f), up, (1,))
                        rep.compare("g_source", gs1, c["ref"]["g_source"], c["P"], dtype, tag=tag + " alone")
                        rep.compare("g_flow", gf1, c["ref"]["g_flow"], c["P"], dtype, c["keep"], tag=tag + " alone")
                        assert _lib.path_count(_lib.PATH_BE_BWD_LDS) == n_b + 3
                    if si < 2 and kind == "wild":    # the forward kernels behind key 0
                        for variant in (2, 3, 4):
                            with pu.Tuning(gfla, {0: variant}):
                                got = mod(s.to(DEV), f.to(DEV))
                                ref0 = default_forward(gfla, ("be", shape, dtype, kind, k), lambda: mod(s.to(DEV), f.to(DEV)), {0: variant})
                            rep.compare("out", got, c["ref"]["out"], c["P"], dtype, tag=tag + " key0=%d" % variant)
                            rep.same_bits("out", got.cpu(), ref0[0], tag + " key0=%d" % variant)
    rep.finish()


# ------------------------------------------------------------------------------------------------------- unfold layout
@pytest.mark.parametrize("dtype,geo", CASES, ids=CASE_IDS)
def test_block_extractor_unfold_over_geometries(gfla, dtype, geo):
    from global_flow_local_attention_amd import _lib
    from global_flow_local_attention_amd import extractor_attn as ea
    keys = geo_of(dtype, geo)
    rep = Report("unfold %s %s" % (NAMES[dtype], keys))
    with pu.Tuning(gfla, keys):
        for shape in pu.SHAPES:
            B, C, Hs, Ws, Hf, Wf = shape
            for k in (3, 5):
                for kind in kinds_of(dtype):
                    c = unfold_case(shape, dtype, kind, k)
                    s, f, up = c["in"]
                    tag = "%s k%d %s" % (shape, k, kind)
                    fn = lambda a, b: ea.BlockExtractorUnfoldFunction.apply(a, b, k)
                    # whole planes only: beyond the forced budget the entry points refuse (float64 forward at 57 x 37; the
                    # backward, which keeps scatter + gather planes, at 48 x 32 and 57 x 37)
                    if check_geometry(_lib, 4, shape, k, 1, dtype, keys)["G"] == 0:
                        continue
                    backward = bool(_lib.lib().gfla_unfold_supported(Hs, Ws, k, elem_of(dtype)))
                    assert backward or 10 in keys
                    if backward:
                        assert check_geometry(_lib, 2, shape, k, 1, dtype, keys)["margin"] < 0
                        out, (gs, gf) = grads(fn, (s, f), up, (0, 1))
                        rep.compare("g_source", gs, c["ref"]["g_source"], c["P"], dtype, tag=tag)
                        rep.compare("g_flow", gf, c["ref"]["g_flow"], c["P"], dtype, c["keep"], tag=tag)
                        if kind == "wild":
                            _, (gs1, _) = grads(fn, (s, f), up, (0,))
                            _, (_, gf1) = grads(fn, (s, f), up, (1,))
                            rep.compare("g_source", gs1, c["ref"]["g_source"], c["P"], dtype, tag=tag + " alone")
                            rep.compare("g_flow", gf1, c["ref"]["g_flow"], c["P"], dtype, c["keep"], tag=tag + " alone")
                    else:
                        out = fn(s.to(DEV), f.to(DEV))
                    rep.compare("out", out, c["ref"]["out"], c["P"], dtype, tag=tag)
                    want = default_forward(gfla, ("unfold", shape, dtype, kind, k), lambda: fn(s.to(DEV), f.to(DEV)))
                    rep.same_bits("out", out.detach().cpu(), want[0], tag)
    rep.finish()


# ------------------------------------------------------------------------------------------------ softmax + aggregate
@pytest.mark.parametrize("dtype,geo", CASES, ids=CASE_IDS)
def test_softmax_aggregate_over_geometries(gfla, dtype, geo):
    from global_flow_local_attention_amd import _lib
    from global_flow_local_attention_amd import extractor_attn as ea
    keys = geo_of(dtype, geo)
    rep = Report("aggregate %s %s" % (NAMES[dtype], keys))
    with pu.Tuning(gfla, keys):
        for shape in pu.SHAPES:
            B, C, Hs, Ws, Hf, Wf = shape
            for k in (3, 5):
                for kind in kinds_of(dtype):
                    c = agg_case(shape, dtype, kind, k)
                    s, f, lg, up = c["in"]
                    tag = "%s k%d %s" % (shape, k, kind)
                    fn = lambda a, b, l: ea.LocalAttnAggregateFunction.apply(a, b, l, k, True)
                    # float64 planes of 57 x 37 are beyond the forced 16 KB: the global-memory kernels (key 3 = 1) take the call
                    beyond = 10 in keys and Hs * Ws * max(4, elem_of(dtype)) > 16 * 1024
                    want = default_forward(gfla, ("agg", shape, dtype, kind, k), lambda: fn(s.to(DEV), f.to(DEV), lg.to(DEV)),
                                           {3: 1} if beyond else None)
                    # the gradients are evaluated with the attention map the forward stored (the backward kernels read it)
                    bwd = cached(("agg bwd", shape, dtype, kind, k), lambda: pu.aggregate_backward(s, f, want[1], up, k))
                    g = check_geometry(_lib, 1, shape, k, 1, dtype, keys)
                    backward = g["G"] > 0 or elem_of(dtype) >= 4      # 16-bit storage beyond the forced budget: refused
                    if backward:
                        (out, attn), (gs, gf, gl) = grads(fn, (s, f, lg), up, (0, 1, 2))
                        rep.compare("g_source", gs, bwd["g_source"], c["P"], dtype, tag=tag)
                        rep.compare("g_flow", gf, bwd["g_flow"], c["P"], dtype, c["keep"], tag=tag)
                        rep.compare("g_logits", gl, bwd["g_logits"], c["P"], dtype, tag=tag)
                        if kind == "wild":
                            for i, name in enumerate(("g_source", "g_flow", "g_logits")):
                                _, got = grads(fn, (s, f, lg), up, (i,))
                                rep.compare(name, got[i], bwd[name], c["P"], dtype, c["keep"] if i == 1 else None, tag=tag + " alone")
                    else:
                        out, attn = fn(s.to(DEV), f.to(DEV), lg.to(DEV))
                    rep.compare("out", out, c["ref"]["out"], c["P"], dtype, tag=tag)
                    rep.compare("attn", attn, c["ref"]["attn"], c["P"], dtype, tag=tag)
                    rep.same_bits("out", out.detach().cpu(), want[0], tag)
                    rep.same_bits("attn", attn.detach().cpu(), want[1], tag)
    rep.finish()


# ------------------------------------------------------------------------------------------------------------ resample2d
@pytest.mark.parametrize("dtype,geo", CASES, ids=CASE_IDS)
def test_resample2d_over_geometries(gfla, dtype, geo):
    from global_flow_local_attention_amd import _lib
    keys = geo_of(dtype, geo)
    rep = Report("resample2d %s %s" % (NAMES[dtype], keys))
    with pu.Tuning(gfla, keys):
        for shape in pu.SHAPES:
            for k, dil in ((4, 1), (2, 1), (4, 2)):
                for kind in kinds_of(dtype):
                    c = rs_case(shape, dtype, kind, k, dil)
                    s, f, up = c["in"]
                    tag = "%s k%d d%d %s" % (shape, k, dil, kind)
                    mod = gfla.Resample2d(k, dil, sigma=pu.SIGMA)
                    assert check_geometry(_lib, 5, shape, k, dil, dtype, keys)["G"] > 0
                    check_geometry(_lib, 6, shape, k, dil, dtype, keys)
                    check_geometry(_lib, 7, shape, k, dil, dtype, keys)
                    out, (g1, gf) = grads(mod, (s, f), up, (0, 1))
                    rep.compare("out", out, c["ref"]["out"], c["P"], dtype, tag=tag)
                    fix = pu.rs_fixed_point_term(c["ref"]["g_input1_count"], up, dtype)
                    rep.compare("g_input1", g1, c["ref"]["g_input1"], c["P"], dtype, extra=fix, tag=tag)
                    rep.compare("g_flow", gf, c["ref"]["g_flow"], c["P"], dtype, c["keep"], tag=tag)
                    want = default_forward(gfla, ("rs", shape, dtype, kind, k, dil), lambda: mod(s.to(DEV), f.to(DEV)))
                    rep.same_bits("out", out.detach().cpu(), want[0], tag)
                    if kind == "wild":
                        _, (g1a, _) = grads(mod, (s, f), up, (0,))
                        _, (_, gfa) = grads(mod, (s, f), up, (1,))
                        rep.compare("g_input1", g1a, c["ref"]["g_input1"], c["P"], dtype, extra=fix, tag=tag + " alone")
                        rep.compare("g_flow", gfa, c["ref"]["g_flow"], c["P"], dtype, c["keep"], tag=tag + " alone")
    rep.finish()


# ------------------------------------------------------------------------------------------ float32 forward row windows
def test_float32_forwards_on_row_windows(gfla):
    """The shapes above keep every float32 GATHER plane within 16 KB, so their forwards never window in float32.  One shape
    just beyond (71 x 59 x 4 B): block_extractor's forward through round 1's kernel (key 0 = 2) and by default dispatch, and
    resample2d's forward, on row windows, against the bar and bit for bit against whole planes."""
    from global_flow_local_attention_amd import _lib
    shape, dtype = pu.WINDOW_FWD_SHAPE, F32
    rep = Report("forward windows f32")
    for kind in pu.KINDS:
        for k in (3, 5):
            c = be_case(shape, dtype, kind, k)
            s, f, _ = c["in"]
            mod = gfla.BlockExtractor(k)
            for variant in (0, 2):     # by default dispatch and forced: under this budget both are round 1's kernel (key 0 = 2)
                tag = "%s k%d %s key0=%d" % (shape, k, kind, variant)
                want = default_forward(gfla, ("be", shape, dtype, kind, k), lambda: mod(s.to(DEV), f.to(DEV)), {0: 2})
                n_f = _lib.path_count(_lib.PATH_BE_FWD_PIX)
                with pu.Tuning(gfla, dict(list(pu.WINDOWS.items()) + [(0, variant)])):
                    got = mod(s.to(DEV), f.to(DEV))
                assert _lib.path_count(_lib.PATH_BE_FWD_PIX) == n_f
                rep.compare("out", got, c["ref"]["out"], c["P"], dtype, tag=tag)
                rep.same_bits("out", got.cpu(), want[0], tag)
        for k, dil in ((4, 1), (4, 2)):
            c = rs_case(shape, dtype, kind, k, dil)
            s, f, _ = c["in"]
            mod = gfla.Resample2d(k, dil, sigma=pu.SIGMA)
            tag = "%s k%d d%d %s" % (shape, k, dil, kind)
            want = default_forward(gfla, ("rs", shape, dtype, kind, k, dil), lambda: mod(s.to(DEV), f.to(DEV)))
            with pu.Tuning(gfla, pu.WINDOWS):
                g = pu.query(_lib, 5, shape, k, dil, 4)
                assert g["G"] >= 1 and g["margin"] >= 0 and g["split"] > 1, g
                got = mod(s.to(DEV), f.to(DEV))
            rep.compare("out", got, c["ref"]["out"], c["P"], dtype, tag=tag)
            rep.same_bits("out", got.cpu(), want[0], tag)
    rep.finish()


# ----------------------------------------------------------------------------------------- what the case table reaches
def test_case_table_reaches_every_geometry(gfla):
    """The geometry assertions of the cases above (check_geometry, the same calls) collected over the whole table: every G in
    {1, 2, 3} with a ragged last group for 2 and 3, every split in {1, 2, 3}, whole planes and row windows, each by a forward
    (unfold forward, resample2d forward) and a backward kernel in float32, and the non-split ones in both 16-bit types."""
    from global_flow_local_attention_amd import _lib
    seen = set()
    for dtype, geo in CASES:
        keys = geo_of(dtype, geo)
        with pu.Tuning(gfla, keys):
            for shape in pu.SHAPES:
                for qop, k, dil, direction in ((0, 3, 1, "bwd"), (2, 3, 1, "bwd"), (1, 5, 1, "bwd"), (6, 4, 2, "bwd"), (7, 4, 2, "bwd"),
                                               (4, 3, 1, "fwd"), (5, 4, 1, "fwd")):
                    g = check_geometry(_lib, qop, shape, k, dil, dtype, keys)
                    if g["G"]:
                        seen.add((NAMES[dtype], direction, "G%d" % g["G"] if g["margin"] < 0 else "window", g["ragged"] > 0 or g["G"] == 1))
                        seen.add((NAMES[dtype], direction, "split%d" % g["split"] if g["margin"] < 0 else "window", True))
    for direction in ("fwd", "bwd"):
        for what in ("G1", "G2", "G3", "split1", "split2", "split3"):
            assert ("f32", direction, what, True) in seen, (direction, what)
        for half in ("f16", "bf16"):
            for what in ("G1", "G2", "G3", "split1"):
                assert (half, direction, what, True) in seen, (half, direction, what)
    assert ("f32", "bwd", "window", True) in seen and ("f64", "bwd", "window", True) in seen and ("f64", "fwd", "window", True) in seen
    with pu.Tuning(gfla, pu.WINDOWS):       # float32 forward windows: test_float32_forwards_on_row_windows
        assert pu.query(_lib, 5, pu.WINDOW_FWD_SHAPE, 4, 1, 4)["margin"] >= 0
