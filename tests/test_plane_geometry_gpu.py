"""The planes-in-LDS kernels (csrc/lds_plane.h) over the launch geometries their heuristics do not pick at small shapes --
channel planes per workgroup G in {1, 2, 3} with a ragged last group, split in {1, 2, 3}, whole planes and row windows --
forced through the tuning keys 4 (cap on G), 5 (split) and 10 (LDS budget), in float32, float64, float16 and bfloat16.

Every result is compared per element with a float64 evaluation from the stored inputs under the derived bar of
tests/plane_util.py (no fitted tolerance); d/d flow entries on a kink are left out (tests/test_plane_geometry_cpu.py caps
their share on these very inputs), nothing is ever left out of a forward result or a feature-map gradient.  Before a case
compares anything it asks gfla_lds_plane_geometry whether the geometry it meant is the one in force, and the dispatch trace
whether the family ran.  Forward results must not change by a bit with G and split: the forwards have no atomics.

resample2d runs twice: as the module (a constant sigma plane, d/d sigma dropped by autograd's cat), and as
Resample2dFunction with input2 = (dx, dy, sigma), one sigma per pixel (plane_util.sigma_field) and both inputs as leaves, so
a kernel that reads sigma at the wrong (b, y, x) or puts d/d sigma in the wrong place is beyond the bar.  The second form
also runs over the routes the geometry keys do not select: the coefficient table and the fixed-point scatter, double planes,
the matrix-core product off and forced, the streaming d/d input2 kernel and rs_lds_kernel in its place, the global kernels,
and the float32 widening of a refused 16-bit backward.

No case sets key 5 together with 16-bit storage.  Key 10 = 16 goes with key 30 = 1 (plane_util.WINDOWS): with key 10 alone
the few planes of these shapes would go to the tile kernels of csrc/tile_map.h instead of row windows."""
import pytest
import torch

from global_flow_local_attention_amd import (TUNE_AGG, TUNE_BE_FWD, TUNE_BIG_PLANE, TUNE_G_CAP, TUNE_LDS_KB, TUNE_PM, TUNE_RS,
                                             TUNE_RS_BWD1_PLANES, TUNE_RS_BWD2_NO_STREAM, TUNE_SPLIT)
import plane_util as pu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
NAMES = {F32: "f32", F64: "f64", F16: "f16", BF16: "bf16"}
GEOS_WIDE = [{}, {TUNE_G_CAP: 2}, {TUNE_G_CAP: 3}, {TUNE_G_CAP: 2, TUNE_SPLIT: 2}, {TUNE_G_CAP: 3, TUNE_SPLIT: 3}, dict(pu.WINDOWS),
             dict(list(pu.WINDOWS.items()) + [(TUNE_G_CAP, 2)])]
GEOS_HALF = [{}, {TUNE_G_CAP: 2}, {TUNE_G_CAP: 3}, dict(pu.WINDOWS)]       # never key 5: the 16-bit backward cannot split
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


def rs_sigma_case(shape, dtype, kind, k, dil, field):
    """resample2d with one sigma per pixel: input2 = (dx, dy, sigma) as the entry points take it.  P is a field with KAPPA
    (plane_util's docstring); the gradient of the feature map takes its largest value."""
    def of_flow(f):          # shared by the fields of one flow
        # no coordinate floors differently in the kernels' arithmetic: the forward and d/d sigma are compared everywhere
        assert torch.equal(pu.rs_coordinates(f, pu.ARITH[dtype]).floor().double(), pu.rs_coordinates(f).floor())
        return pu.coordinate_bound(f, (k // 2) * dil), ~pu.rs_flow_kinks(f, k, dil, shape[2], shape[3], pu.ARITH[dtype])

    def make():
        s, f, up = cached(("rs in", shape, dtype, kind, k), lambda: pu.inputs("rs", shape, dtype, kind, k))
        sig = pu.rs_sigma(shape, dtype, kind, k, field)
        assert sig.double().min().item() >= pu.SIGMA_MIN            # what the bar's derivation stands on
        bound, keep = cached(("rs flow", shape, dtype, kind, k, dil), lambda: of_flow(f))
        P = bound * pu.rs_kappa(k, dil, sig) ** 2
        ref = pu.resample2d(s, f, up, k, dil, sigma=sig)
        P_of = {"out": P, "g_input1": P.max().item(), "g_flow": P, "g_sigma": P}
        # the bar of each result, kept with the reference: a case compares up to three runs under every geometry
        bars = {name: pu.bar(ref[name][1], ref[name][0], ref[name][2], P_of[name], dtype) for name in P_of}
        return {"in": (s, torch.cat((f, sig), 1).contiguous(), up), "ref": ref, "P": P_of, "bar": bars, "keep": keep}
    return cached(("rs sigma", shape, dtype, kind, k, dil, field), make)


def device_leaves(c, which):
    """fresh leaves of the case's inputs on the device (copied there once per case) and its upstream gradient; `which`:
    indices of the inputs that require a gradient"""
    if "dev" not in c:
        c["dev"] = [x.to(DEV) for x in c["in"]]
    s, i2, up = c["dev"]
    return [x.detach().clone().requires_grad_(i in which) for i, x in enumerate((s, i2))], up


# ------------------------------------------------------------------------------------------------------------- the harness
class Report(object):
    """Collects every comparison of one test, prints each figure, fails at the end with all of them"""

    def __init__(self, what):
        self.what, self.bad, self.worst = what, [], {}

    def compare(self, name, got, entry, P, dtype, keep=None, extra=None, tag="", bar=None):
        ref, A, n = entry
        assert got.dtype == dtype and tuple(got.shape) == tuple(ref.shape), (name, got.dtype, tuple(got.shape), tuple(ref.shape))
        ratio, beyond = pu.worst(got, ref, A, n, P, dtype, keep, extra, bar)    # extra: resample2d's fixed-point planes
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
        assert TUNE_LDS_KB in keys and (qop in (1, 2, 3, 4) or elem == 2), (qop, shape, keys, g)          # and 16-bit backwards
        return g
    if g["margin"] >= 0:             # row windows: only under the forced budget, never the 16-bit owner kernels
        assert TUNE_LDS_KB in keys and not half_owner and g["lds"] <= 16 * 1024 and g["split"] > 1, (qop, shape, keys, g)
        return g
    per_channel = g["lds"] // g["G"]
    budget = (16 if TUNE_LDS_KB in keys else 64) * 1024
    assert g["lds"] <= budget
    if TUNE_G_CAP in keys:
        want = min(keys[TUNE_G_CAP], C, budget // per_channel)
        assert g["G"] == want and g["ngroups"] == -(-C // want), (qop, shape, keys, g)
        assert g["ragged"] == (C % want if C % want else 0)
    else:
        assert g["G"] == 1 and g["ngroups"] == C and g["ragged"] == 0, (qop, shape, keys, g)    # the heuristics at these sizes
    if TUNE_SPLIT in keys:
        assert elem != 2 and g["split"] == keys[TUNE_SPLIT] and g["per"] == -(-Hf * Wf // keys[TUNE_SPLIT]), (qop, shape, keys, g)
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
        with gfla.tuned({TUNE_G_CAP: 0, TUNE_SPLIT: 0, TUNE_LDS_KB: 0, TUNE_BIG_PLANE: 0}):
            with gfla.tuned(kernel or {}):
                out = run()
        return [o.detach().cpu() for o in (out if isinstance(out, tuple) else (out,))]
    return cached(("default", tuple(sorted((kernel or {}).items()))) + key, make)


# ------------------------------------------------------------------------------------------------------ block_extractor
@pytest.mark.parametrize("dtype,geo", CASES, ids=CASE_IDS)
def test_block_extractor_over_geometries(gfla, dtype, geo):
    from global_flow_local_attention_amd import _lib
    keys = geo_of(dtype, geo)
    rep = Report("block_extractor %s %s" % (NAMES[dtype], keys))
    with gfla.tuned(keys):
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
                    if elem_of(dtype) >= 4 and TUNE_LDS_KB not in keys:
                        assert _lib.path_count(_lib.PATH_BE_FWD_PIX) == n_f + 1, "forward left the planes-in-LDS family: " + tag
                    rep.compare("out", out, c["ref"]["out"], c["P"], dtype, tag=tag)
                    rep.compare("g_source", gs, c["ref"]["g_source"], c["P"], dtype, tag=tag)
                    rep.compare("g_flow", gf, c["ref"]["g_flow"], c["P"], dtype, c["keep"], tag=tag)
                    # beyond the forced budget the padded planes of the lane-per-pixel / wave-per-row kernels do not fit and
                    # round 1's kernel (key 0 = 2) takes the forward, on row windows
                    other = elem_of(dtype) >= 4 and _lib.path_count(_lib.PATH_BE_FWD_PIX) == n_f
                    assert not other or TUNE_LDS_KB in keys
                    want = default_forward(gfla, ("be", shape, dtype, kind, k), lambda: mod(s.to(DEV), f.to(DEV)),
                                           {TUNE_BE_FWD: 2} if other else None)
                    rep.same_bits("out", out.detach().cpu(), want[0], tag)
                    if kind == "wild":      # each gradient alone: the NEED_SRC / NEED_FLOW instantiations
                        _, (gs1, _) = grads(mod, (s, f), up, (0,))
                        _, (_, gf1) = grads(mod, (s, f), up, (1,))
                        rep.compare("g_source", gs1, c["ref"]["g_source"], c["P"], dtype, tag=tag + " alone")
                        rep.compare("g_flow", gf1, c["ref"]["g_flow"], c["P"], dtype, c["keep"], tag=tag + " alone")
                        assert _lib.path_count(_lib.PATH_BE_BWD_LDS) == n_b + 3
                    if si < 2 and kind == "wild":    # the forward kernels behind key 0
                        for variant in (2, 3, 4):
                            with gfla.tuned({TUNE_BE_FWD: variant}):
                                got = mod(s.to(DEV), f.to(DEV))
                                ref0 = default_forward(gfla, ("be", shape, dtype, kind, k), lambda: mod(s.to(DEV), f.to(DEV)),
                                                       {TUNE_BE_FWD: variant})
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
    with gfla.tuned(keys):
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
                    assert backward or TUNE_LDS_KB in keys
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
    with gfla.tuned(keys):
        for shape in pu.SHAPES:
            B, C, Hs, Ws, Hf, Wf = shape
            for k in (3, 5):
                for kind in kinds_of(dtype):
                    c = agg_case(shape, dtype, kind, k)
                    s, f, lg, up = c["in"]
                    tag = "%s k%d %s" % (shape, k, kind)
                    fn = lambda a, b, l: ea.LocalAttnAggregateFunction.apply(a, b, l, k, True)
                    # float64 planes of 57 x 37 are beyond the forced 16 KB: the global-memory kernels (key 3 = 1) take the call
                    beyond = TUNE_LDS_KB in keys and Hs * Ws * max(4, elem_of(dtype)) > 16 * 1024
                    want = default_forward(gfla, ("agg", shape, dtype, kind, k), lambda: fn(s.to(DEV), f.to(DEV), lg.to(DEV)),
                                           {TUNE_AGG: 1} if beyond else None)
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
    with gfla.tuned(keys):
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


# --------------------------------------------------------------------------------------- resample2d, one sigma per pixel
RS_FIELD_KD = ((4, 1), (2, 1), (4, 2), (6, 1))       # (6, 1): KH = 3


def rs_field_run(fn, c, which):
    """forward and backward of fn on fresh leaves of case c; (out, d/d input1, d/d input2) as host tensors, None where not
    asked for"""
    (a, b), up = device_leaves(c, which)
    out = fn(a, b)
    out.backward(up)
    return [None if t is None else t.detach().cpu() for t in (out, a.grad, b.grad)]


def rs_field_compare(rep, c, out, g1, g2, dtype, fix, tag):
    """the four results of one sigma-field run; g2 = d/d (dx, dy, sigma) in the storage type, None entries are not compared"""
    ref, P, bar = c["ref"], c["P"], c["bar"]
    if out is not None:
        rep.compare("out", out, ref["out"], P["out"], dtype, tag=tag, bar=bar["out"])
    if g1 is not None:
        rep.compare("g_input1", g1, ref["g_input1"], P["g_input1"], dtype, extra=fix, tag=tag, bar=bar["g_input1"])
    if g2 is not None:
        assert g2.dtype == dtype and g2.shape[1] == 3, (tag, g2.dtype, tuple(g2.shape))      # the storage type
        rep.compare("g_flow", g2[:, :2], ref["g_flow"], P["g_flow"], dtype, c["keep"], tag=tag, bar=bar["g_flow"])
        # everywhere: d/d sigma has no kinks of its own
        rep.compare("g_sigma", g2[:, 2:], ref["g_sigma"], P["g_sigma"], dtype, tag=tag, bar=bar["g_sigma"])


RS_FIELD_PAIRS = (("wild", "levels"), ("wild", "random"), ("smooth", "levels"), ("smooth", "random"))


def rs_field_runs(dtype, si, ki):
    """[(flow kind, sigma field, each gradient alone as well)] of shape `si` of pu.SHAPES at entry `ki` of RS_FIELD_KD.  Wild
    and smooth flows under both fields, three of the four pairs per case: the pair left out rotates with si + ki, so every
    pair runs at two or three of the first three (k, dil) of every shape, every case has both kinds and both fields, and
    each gradient is requested alone on its first wild pair.  `oob` (16-bit storage) puts every tap of a pixel on one corner
    of the map; the normalised weights then sum to 1 whatever sigma is and d/d sigma is a difference of two equal sums: one
    field.

    All four pairs at every case is beyond 1.5 x the time of the constant-sigma test of the same id: the first geometry of
    a storage type evaluates every reference on the host.  For the same reason kernel_size 6 (KH = 3), whose 36 taps cost
    the host twice the time of 16, runs in float32 and float64 only (the arithmetic of 16-bit storage is the float32 one),
    one wild and one smooth pair at the two small shapes and the wild pair at the two large ones, the fields swapped from
    shape to shape."""
    if RS_FIELD_KD[ki][0] == 6:
        if dtype in (F16, BF16):
            return []
        runs = [RS_FIELD_PAIRS[si % 2]] + ([RS_FIELD_PAIRS[3 - si % 2]] if si < 2 else [])
    else:
        runs = [pair for i, pair in enumerate(RS_FIELD_PAIRS) if i != (si + ki) % 4]
        assert {r[0] for r in runs} == {"wild", "smooth"} and {r[1] for r in runs} == set(pu.SIGMA_FIELDS)
    assert runs[0][0] == "wild"
    runs = [(kind, field, (kind, field) == runs[0]) for kind, field in runs]
    return runs + ([("oob", "random", False)] if dtype in (F16, BF16) else [])


@pytest.mark.parametrize("dtype,geo", CASES, ids=CASE_IDS)
def test_resample2d_sigma_field_over_geometries(gfla, dtype, geo):
    """Resample2dFunction with input2 = (dx, dy, sigma) and BOTH inputs as leaves: sigma varies from pixel to pixel
    (plane_util.sigma_field) and d/d sigma, which the module form drops, is compared at every pixel."""
    from global_flow_local_attention_amd import _lib
    keys = geo_of(dtype, geo)
    rep = Report("resample2d sigma field %s %s" % (NAMES[dtype], keys))
    with gfla.tuned(keys):
        for si, shape in enumerate(pu.SHAPES):
            for ki, (k, dil) in enumerate(RS_FIELD_KD):
                fn = lambda a, b: gfla.Resample2dFunction.apply(a, b, k, dil)
                runs = rs_field_runs(dtype, si, ki)
                if not runs:
                    continue
                assert check_geometry(_lib, 5, shape, k, dil, dtype, keys)["G"] > 0
                check_geometry(_lib, 6, shape, k, dil, dtype, keys)
                check_geometry(_lib, 7, shape, k, dil, dtype, keys)
                for kind, field, alone in runs:
                    c = rs_sigma_case(shape, dtype, kind, k, dil, field)
                    tag = "%s k%d d%d %s %s" % (shape, k, dil, kind, field)
                    out, g1, g2 = rs_field_run(fn, c, (0, 1))
                    fix = cached(("rs fix", shape, dtype, kind, k, dil, field),
                                 lambda: pu.rs_fixed_point_term(c["ref"]["g_input1_count"], c["in"][2], dtype))
                    rs_field_compare(rep, c, out, g1, g2, dtype, fix, tag)
                    want = default_forward(gfla, ("rs sigma", shape, dtype, kind, k, dil, field), lambda: fn(*c["dev"][:2]))
                    rep.same_bits("out", out, want[0], tag)
                    if alone:
                        _, g1a, none2 = rs_field_run(fn, c, (0,))
                        _, none1, g2a = rs_field_run(fn, c, (1,))
                        assert none1 is None and none2 is None
                        rs_field_compare(rep, c, None, g1a, g2a, dtype, fix, tag + " alone")
    rep.finish()


# the routes the geometry keys do not select (csrc/gs_route.h: rs_fwd_route / rs_bwd_route; key 14: csrc/patch_mfma.hip)
ROUTES = [({}, (F32, F64, F16, BF16)),     # coefficient table + fixed point, streaming d/d input2, the product where it pays
          ({TUNE_RS_BWD1_PLANES: 1}, (F32,)),               # double planes, no table
          ({TUNE_RS_BWD1_PLANES: 2}, (F32,)),               # fixed point without the table
          ({TUNE_RS_BWD2_NO_STREAM: 1}, (F32, F16, BF16)),  # rs_lds_kernel gathers d/d input2 instead of the streaming kernel
          ({TUNE_PM: 1}, (F32,)),                           # matrix-core product off
          ({TUNE_PM: 2}, (F32,)),                           # ... wherever the shape is supported
          ({TUNE_RS: 1}, (F32, F64))]                       # global kernels (16-bit storage ignores the key)
ROUTE_CASES = [(keys, dt) for keys, dts in ROUTES for dt in dts]
ROUTE_IDS = ["%s-%s" % (",".join("%d=%d" % kv for kv in sorted(keys.items())) or "default", NAMES[dt]) for keys, dt in ROUTE_CASES]


@pytest.mark.parametrize("keys,dtype", ROUTE_CASES, ids=ROUTE_IDS)
def test_resample2d_sigma_field_over_routes(gfla, keys, dtype):
    """The same comparison on the routes that build the per-pixel weights away from the plain kernels.  What a route
    shows of itself is asserted: the planes-in-LDS query (ops 5-7) says whole planes, or `not taken` under key 6 = 1, and
    the big-plane counters 15-17 stay put.  Every route float32-sums products or scatters into the fixed-point planes:
    plane_util.rs_input1_term."""
    import ctypes
    import gs_route_util
    from global_flow_local_attention_amd import _lib
    rep = Report("resample2d sigma field routes %s %s" % (NAMES[dtype], keys))
    is_global = keys.get(TUNE_RS) == 1 and dtype in (F32, F64)
    big = [_lib.path_count(i) for i in (15, 16, 17)]
    with gfla.tuned(keys):
        for shape in (pu.SHAPES[0], pu.SHAPES[1], gs_route_util.S):
            for k, dil in ((4, 1), (4, 2), (2, 1)):
                fn = lambda a, b: gfla.Resample2dFunction.apply(a, b, k, dil)
                for qop in (5, 6, 7):
                    g = pu.query(_lib, qop, shape, k, dil, elem_of(dtype))
                    assert (g["G"] == 0) if is_global else (g["G"] >= 1 and g["margin"] < 0 and g["split"] == 1), (qop, shape, keys, g)
                if shape == gs_route_util.S and (k, dil) == (4, 1) and dtype != F64 and not is_global:
                    # the streaming d/d input2 kernel can take the shape (a K = 3 patch)
                    assert _lib.lib().gfla_aggregate_fwd_geometry(*shape, 3, (ctypes.c_int64 * 9)()) == 0
                for field in pu.SIGMA_FIELDS:
                    c = rs_sigma_case(shape, dtype, "wild", k, dil, field)
                    tag = "%s k%d d%d wild %s" % (shape, k, dil, field)
                    out, g1, g2 = rs_field_run(fn, c, (0, 1))
                    fix = pu.rs_input1_term(c["ref"]["g_input1_count"], c["in"][2], dtype, keys)
                    rs_field_compare(rep, c, out, g1, g2, dtype, fix, tag)
    assert [_lib.path_count(i) for i in (15, 16, 17)] == big, "a big-plane kernel took a call"
    rep.finish()


def test_resample2d_sigma_field_through_the_widened_16_bit_backward(gfla):
    """bfloat16 planes beyond a forced 16 KB budget: the bfloat16 backward entry point refuses, Resample2dFunction widens
    the three inputs to float32 -- the sigma plane with them -- and rounds once at the end."""
    import gs_route_util
    from global_flow_local_attention_amd import _lib
    shape, dtype, k, dil = gs_route_util.W, BF16, 4, 1
    B, C, Hi, Wi, H, W = shape
    rep = Report("resample2d sigma field widened bf16")
    with gfla.tuned({TUNE_LDS_KB: 16}):
        for field in pu.SIGMA_FIELDS:
            c = rs_sigma_case(shape, dtype, "wild", k, dil, field)
            (a, b), g = device_leaves(c, ())
            g1, g2 = torch.zeros_like(a), torch.zeros(B, 3, H, W, dtype=F32, device=DEV)
            with pytest.raises(_lib.Unsupported):
                _lib.call("gfla_resample2d_bwd_bf16", a, _lib.ptr(a), _lib.ptr(b), _lib.ptr(g), _lib.ptr(g1), _lib.ptr(g2),
                          B, C, Hi, Wi, H, W, k, dil, 1)
            before = [_lib.path_count(i) for i in (16, 17)]
            out, g1, g2 = rs_field_run(lambda x, y: gfla.Resample2dFunction.apply(x, y, k, dil), c, (0, 1))
            assert [_lib.path_count(i) for i in (16, 17)] == [before[0] + 1, before[1] + 1]      # the float32 big-plane kernels
            fix = pu.rs_fixed_point_term(c["ref"]["g_input1_count"], c["in"][2], dtype)
            rs_field_compare(rep, c, out, g1, g2, dtype, fix, "%s k%d d%d wild %s" % (shape, k, dil, field))
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
                want = default_forward(gfla, ("be", shape, dtype, kind, k), lambda: mod(s.to(DEV), f.to(DEV)), {TUNE_BE_FWD: 2})
                n_f = _lib.path_count(_lib.PATH_BE_FWD_PIX)
                with gfla.tuned(dict(list(pu.WINDOWS.items()) + [(TUNE_BE_FWD, variant)])):
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
            with gfla.tuned(pu.WINDOWS):
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
        with gfla.tuned(keys):
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
    with gfla.tuned(pu.WINDOWS):       # float32 forward windows: test_float32_forwards_on_row_windows
        assert pu.query(_lib, 5, pu.WINDOW_FWD_SHAPE, 4, 1, 4)["margin"] >= 0
