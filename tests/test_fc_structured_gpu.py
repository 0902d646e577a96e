"""The FC layers of ExtractorAttn on STRUCTURED inputs (tests/fc_util.py): per-sample, per-channel and spatial amplitudes, post-ReLU
maps, sparse peaked upstream gradients -- the inputs on which `max err / max |want|` of the round-2 tests is blind to whatever
happens in the quiet part of a tensor (test_fc_structured_cpu.py plants such defects and shows which check sees them).

1. EXACT cases: small integers times powers of two, flows with fractions in {1/4, 1/2, 3/4}, slopes 1/4 and 1/2, chosen so that
   every term of every stage satisfies sum |terms| < 2^21 quantum (asserted on the host by test_fc_structured_cpu.py).  Any
   correct float32 summation order then returns the float64 reference BIT FOR BIT: torch.equal, zero tolerance -- for the direct
   kernels of modes 0-3, the direct legs of mode 5, the float32 glue (sampling tails, scatter, fold, d W1, biases) and the forward
   of the f16 path.  The Winograd-domain kernels multiply by 1/3 and 1/15 and cannot be exact.
2. FLOAT cases (Gaussian times the same structure): per element against float64 with derived bars -- 2 (K + 2) 2^-24 S for the
   direct kernels (S the float64 sum of absolute products; split-mode terms in fc_util.direct_bar), and for the Winograd-domain
   kernels 4 c 2^-24 S_tile with c MEASURED on the host by a float32 emulation of the same formulation on these very inputs
   (+ the lo-subnormal term of their two-term f16 form, fc_util.wn16_conv_lo / wn16_wgrad_lo: it is what a sample at 2^-16 of
   the batch maximum is entitled to under the per-tensor scale).
"""
import ctypes

import pytest
import torch

import fc_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("logits", "g_s", "g_t", "g_f", "g_w0", "g_b0", "g_w1", "g_b1")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(t, dtype=torch.float32):
    return t.to(dtype).to(DEV).contiguous()


def _layer(mode, c, f16=False):
    """gfla_fc_forward_f32 (or _f16) + gfla_fc_backward_f32 through the C ABI: logits and the seven gradients, as float64 on the host"""
    from global_flow_local_attention_amd import _lib, fc_mfma
    k, B, C, H, W, slope = c["k"], c["B"], c["C"], c["H"], c["W"], c["slope"]
    s, t = (_dev(c[n], torch.float16 if f16 else torch.float32) for n in ("s", "t"))
    f, w0, b0, w1, b1, up = (_dev(c[n]) for n in ("f", "w0", "b0", "w1", "b1", "up"))
    ws = torch.empty(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 0), dtype=torch.uint8, device=DEV)
    sc = torch.empty(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 1), dtype=torch.uint8, device=DEV)
    lg = torch.full((B, k * k, H, W), float("nan"), device=DEV)
    if f16:
        _lib.call("gfla_fc_forward_f16", s, _ptr(s), _ptr(t), _ptr(f), _ptr(w0), _ptr(b0), _ptr(w1), _ptr(b1), _ptr(ws), _ptr(lg),
                  B, C, H, W, k, slope)
    else:
        _lib.call("gfla_fc_forward_f32", s, _ptr(s), _ptr(t), _ptr(f), _ptr(w0), _ptr(b0), _ptr(w1), _ptr(b1), _ptr(ws), _ptr(lg),
                  B, C, H, W, k, slope, mode)
    gs, gt = (torch.full((B, C, H, W), float("nan"), device=DEV) for _ in range(2))
    gf = torch.full_like(f, float("nan"))
    gw0, gb0, gw1, gb1 = (torch.full_like(x, float("nan")) for x in (w0, b0, w1, b1))
    _lib.call("gfla_fc_backward_f32", f, _ptr(ws), _ptr(f), _ptr(w1), _ptr(up), _ptr(sc), _ptr(gs), _ptr(gt), _ptr(gf), _ptr(gw0),
              _ptr(gb0), _ptr(gw1), _ptr(gb1), B, C, H, W, k, slope, mode, 0)
    torch.cuda.synchronize()
    return dict(zip(NAMES, (x.double().cpu() for x in (lg, gs, gt, gf, gw0, gb0, gw1, gb1))))


def _half(mode, c, is_source):
    """gfla_fc_conv_fwd_f32 + gfla_fc_conv_bwd_f32 on one half: map, data gradient, this half's weight gradient (float64, host)"""
    from global_flow_local_attention_amd import _lib, fc_mfma
    k, B, C, H, W = c["k"], c["B"], c["C"], c["H"], c["W"]
    x, w0, dG = _dev(c["s" if is_source else "t"]), _dev(c["w0"]), _dev(c["dG%d" % is_source])
    g = fc_mfma.geometry(H, W, k, is_source)
    ws = torch.empty(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 0), dtype=torch.uint8, device=DEV)
    out = torch.full((B, g["Mg"], 128), float("nan"), device=DEV)
    _lib.call("gfla_fc_conv_fwd_f32", x, _ptr(x), _ptr(w0), is_source, _ptr(ws), _ptr(out), B, C, H, W, k, mode)
    rows = (torch.arange(g["Ho"])[:, None] * g["Wp"] + torch.arange(g["Wo"])[None, :]).reshape(-1).to(DEV)
    z = torch.zeros(B, g["Sz"], 128, device=DEV)
    z[:, g["lead"] + rows, :] = dG.permute(0, 2, 3, 1).reshape(B, -1, 128)
    sc = torch.empty(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 1), dtype=torch.uint8, device=DEV)
    gx = torch.full((B, C, H, W), float("nan"), device=DEV)
    gw = torch.full((128, 2 * C, k, k), float("nan"), device=DEV)
    _lib.call("gfla_fc_conv_bwd_f32", x, _ptr(z), is_source, _ptr(ws), _ptr(sc), _ptr(gx), _ptr(gw), B, C, H, W, k, mode)
    torch.cuda.synchronize()
    y = out[:, :g["Ho"] * g["Wo"], :].reshape(B, g["Ho"], g["Wo"], 128).permute(0, 3, 1, 2)
    other = U.half_weights(gw, C, 1 - is_source)
    assert float(other.abs().max()) == 0.0
    return dict(y=y.double().cpu(), gx=gx.double().cpu(), gw=U.half_weights(gw, C, is_source).double().cpu())


def _same(got, want, what):
    """zero tolerance, with a report that locates a finding"""
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()
    err = (got - want).abs()[bad]
    raise AssertionError("%s: %d of %d entries differ from float64, max |diff| %.3e (max |want| %.3e); first at %s: got %r want %r" % (
        what, int(bad.sum()), got.numel(), float(err.max()), float(want.abs().max()), idx[0].tolist(),
        float(got[tuple(idx[0])]), float(want[tuple(idx[0])])))


# ================================================================================= exact cases
def _exact_layer_outputs(mode, k, spread):
    names = U.EXACT_OUTPUTS[spread]
    if (mode == 5) or (mode == 1 and k == 5):   # these weight gradients run in the Winograd domain (fc_plan)
        names = tuple(n for n in names if n != "g_w0")
    return names


def _assert_mode(c, mode):
    """no silent fallback: the case runs in the mode it names"""
    from global_flow_local_attention_amd import fc_mfma
    assert fc_mfma.resolve_mode(c["C"], c["H"], c["W"], c["k"], mode) == mode


# mode 5 at k = 3: test_exact_whole_layer_mode5_k3 (its forward runs in the Winograd domain, docstring below)
EXACT_LAYER = [(m, s) for m in (0, 1, 2, 3, 5) for s in U.SHAPES + [U.COLLAPSE] if not (m == 5 and s[0] == 3)]


@pytest.mark.parametrize("spread", ["wide", "narrow"])
@pytest.mark.parametrize("mode,shape", EXACT_LAYER, ids=str)
def test_exact_whole_layer(gfla, mode, shape, spread):
    """Logits and gradients of the whole layer, bit for bit.  'wide' (samples at 2^0, 2^-11, 2^5): logits, source / target / flow
    gradients and the b1 gradient; 'narrow' (2^0, 2^-2, 2^1: the parameter gradients sum over the samples): all seven gradients.  Modes 0-3: every
    kernel is direct.  Mode 5: k = 5 only (its k = 3 forward is Winograd-domain, so hidden units that are exactly 0 -- frequent
    here, and welcome -- would come out at +-1e-7 and take the other slope), without the Winograd-domain weight gradient.  The
    mode-independent glue (tails, scatter, fold with C a multiple of 4 and not, d W1, biases) is what every one of these runs."""
    k = shape[0]
    c = U.make_case(shape, True, spread)
    _assert_mode(c, mode)
    want = U.layer_reference(c)
    got = _layer(mode, c)
    for n in _exact_layer_outputs(mode, k, spread):
        _same(got[n], want[n] if n == "logits" else want[n].reshape(got[n].shape), "mode %d %s %s %s" % (mode, shape, spread, n))


@pytest.mark.parametrize("shape", [s for s in U.SHAPES if s[0] == 3], ids=str)
def test_exact_whole_layer_mode5_k3(gfla, shape):
    """Mode 5 at k = 3 through the whole layer: everything downstream of the data-gradient convolutions, bit for bit -- the tail's
    d hidden, the two-term f16 pack of both gradient maps under ONE scale per tensor (samples of the upstream gradient at 2^0,
    2^-11, 2^5), the owner-computes scatter, both data gradients issued together, the fold; and the b1 gradient.  The forward is
    Winograd-domain and inexact, so the 'offset' case (fc_util.SPREAD) keeps every hidden unit at least 2^-7 from 0: the slopes
    are the reference's.  The flow gradient reads the inexact convolved source map and the w1 / w0 gradients the inexact
    activations / the Winograd domain: they are held to the per-element bars of the float cases instead."""
    c = U.make_case(shape, True, "offset")
    _assert_mode(c, 5)
    want = U.layer_reference(c)
    got = _layer(5, c)
    for n in U.EXACT_OUTPUTS["offset"]:
        _same(got[n], want[n].reshape(got[n].shape), "mode 5 %s offset %s" % (shape, n))


@pytest.mark.parametrize("shape", [U.COLLAPSE, (3, 3, 17, 7, 5), (3, 2, 8, 33, 65)], ids=str)
def test_exact_scatter_owner_computes_and_atomics(gfla, shape):
    """The owner-computes scatter (64-bit fixed-point cells; several list rounds on the collapsing flow) and round 2's float
    atomics (tuning key 46 = 1): on these inputs every sum is exact in any order, so both equal float64 and each other."""
    c = U.make_case(shape, True, "narrow")
    _assert_mode(c, 0)
    want = U.layer_reference(c)
    own = _layer(0, c)
    with gfla.tuned({gfla.TUNE_FC_SCATTER_ATOMICS: 1}):
        atom = _layer(0, c)
    for n in NAMES:
        _same(atom[n], own[n], "%s %s: atomics vs owner-computes" % (shape, n))
        _same(atom[n], want[n].reshape(atom[n].shape), "%s %s: atomics vs float64" % (shape, n))


@pytest.mark.parametrize("shape", U.SHAPES + [U.COLLAPSE], ids=str)
def test_exact_f16_forward(gfla, shape):
    """gfla_fc_forward_f16: a stored f16 value is one term, the records are packed unscaled -- logits bit for bit (and the mode-1
    backward on that workspace: data and flow gradients)."""
    c = U.make_case(shape, True, "wide")
    for n in ("s", "t"):
        assert torch.equal(c[n].half().double(), c[n])
    _assert_mode(c, 1)
    want = U.layer_reference(c)
    got = _layer(1, c, f16=True)
    for n in ("logits", "g_s", "g_t", "g_f"):
        _same(got[n], want[n], "f16 forward %s %s" % (shape, n))


@pytest.mark.parametrize("is_source", [0, 1])
@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 5])
def test_exact_halves(gfla, mode, shape, is_source):
    """Per-half entry points: map and data gradient on the 'wide' case, weight gradient on the 'narrow' one.  Mode 5: the legs
    fc_plan sends to the direct kernels (k = 5 forward, both data gradients)."""
    k = shape[0]
    for spread, legs in (("wide", ("y", "gx")), ("narrow", ("gw",))):
        legs = tuple(n for n in legs if not U.is_wino(mode, k, {"y": "fwd", "gx": "dgrad", "gw": "wgrad"}[n]) and
                     not (n == "gw" and mode == 1 and k == 5))
        if not legs:
            continue
        c = U.make_case(shape, True, spread)
        _assert_mode(c, mode)
        want = U.half_reference(c, is_source)
        got = _half(mode, c, is_source)
        for n in legs:
            _same(got[n], want[n], "mode %d %s half %d %s %s" % (mode, shape, is_source, spread, n))


# ================================================================================= float cases: per-element bars
FLOAT_MODES = [0, 1, 2, 3, 4, 5]  # (mode 1 -- one f16 term per operand, the bf16 / f16 feature path -- with its own derived term)
_worst = {}


def _note(mode, k, stage, ratio):
    key = (mode, k, stage)
    _worst[key] = max(_worst.get(key, 0.0), ratio)


@pytest.mark.parametrize("is_source", [0, 1])
@pytest.mark.parametrize("shape,spread", [(s, "wide") for s in U.SHAPES] + [((5, 3, 17, 7, 5), "quiet8"), ((3, 3, 17, 7, 5), "quiet8")],
                         ids=str)
@pytest.mark.parametrize("mode", FLOAT_MODES)
def test_float_halves_per_element(gfla, mode, shape, spread, is_source):
    """Map, data gradient and weight gradient of one half against float64, element by element.  'quiet8': one sample at 2^-8 of
    the batch maximum -- by fc_scale_exp both f16 terms of its values stay normal, so it stays inside the same bar."""
    from global_flow_local_attention_amd import fc_mfma
    k, B, C, H, W = shape
    assert fc_mfma.resolve_mode(C, H, W, k, mode) == mode
    hb = U.half_bars(shape, is_source, spread)
    got = _half(mode, hb["case"], is_source)
    ratios = {}
    for n, leg in (("y", "fwd"), ("gx", "dgrad"), ("gw", "wgrad")):
        ratios[n] = U.worst_ratio(got[n], hb["ref"][n], U.half_bar(hb, mode, leg))
        _note(mode, k, ("wino " if U.is_wino(mode, k, leg) else "") + leg, ratios[n])
    print("mode %d %s %s half %d: err/bar map %.3f grad_x %.3f grad_w %.3f  (Winograd c: fwd %.2f dgrad %.2f wgrad %.2f)" % (
        mode, shape, spread, is_source, ratios["y"], ratios["gx"], ratios["gw"], hb["c_y"], hb["c_gx"], hb["c_gw"]))
    assert all(r <= 1.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("shape,spread", [(s, "wide") for s in U.SHAPES] + [((5, 3, 17, 7, 5), "quiet8")], ids=str)
@pytest.mark.parametrize("mode", FLOAT_MODES)
def test_float_whole_layer_per_element(gfla, mode, shape, spread):
    """Logits and all seven gradients of the whole layer against float64, element by element, with the bars of
    fc_util.layer_bars (the stage bars propagated through the layer).  Flow gradient: entries whose sampling position is within
    FLOW_EPS of an integer coordinate are left out (the bilinear kink); at most 10 % may be."""
    from global_flow_local_attention_amd import fc_mfma
    k, B, C, H, W = shape
    assert fc_mfma.resolve_mode(C, H, W, k, mode) == mode
    lb = U.layer_bars(shape, spread, mode)
    got = _layer(mode, lb["case"])
    ratios = {}
    for n in NAMES:
        g, w, bar = got[n], lb["ref"][n].reshape(got[n].shape), lb["bar"][n].reshape(got[n].shape)
        if n == "g_f":
            keep = ~lb["flow_excluded"]
            assert float((~keep).double().mean()) <= 0.10
            g, w, bar = g[keep], w[keep], bar[keep]
        ratios[n] = U.worst_ratio(g, w, bar)
        _note(mode, k, n, ratios[n])
    print("mode %d %s %s: err/bar " % (mode, shape, spread) + " ".join("%s %.3f" % x for x in ratios.items()))
    assert all(r <= 1.0 for r in ratios.values()), ratios


def test_report_worst_ratios():
    """the largest error / bar per (mode, k, stage) of the float cases above (pytest -s)"""
    for key in sorted(_worst, key=str):
        print("mode %d k %d %-12s worst err/bar %.3f" % (key + (_worst[key],)))
    assert all(v <= 1.0 for v in _worst.values())
