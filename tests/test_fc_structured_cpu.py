"""Host side of the structured FC tests (tests/fc_util.py, tests/test_fc_structured_gpu.py): the float64 stage references
against the oracle and against F.conv2d, the exactness condition of every exact case the GPU file runs, the flow-gradient
exclusion cap, the float32 Winograd emulation, and -- the point of the exercise -- PLANTED BUGS: a host evaluation of the layer
with one defect each, confined to a quiet part of a tensor, which the round-2 rule (`max err / max |want|` <= 1e-5 for maps and
logits, 2e-5 for gradients) passes and the new checks fail.

Which check catches which planted bug ('wide' cases: samples at 2^0, 2^-11, 2^5; the bug always sits in the quiet sample):

| planted bug                                                        | round-2 rule | per-element bar (float case) | exact case (torch.equal) |
|--------------------------------------------------------------------|--------------|------------------------------|--------------------------|
| tap: one tap dropped in the last tile of the quiet sample          | passes       | FAILS                        | FAILS                    |
| chunk: the quiet, partial 16-channel chunk skipped                 | passes       | FAILS                        | FAILS                    |
| reflect: reflect for replicate padding, left edge, quiet sample    | passes       | FAILS                        | FAILS                    |
| scatter: one scatter contribution dropped                          | passes       | FAILS                        | FAILS                    |
| row: last row missing from the b1 gradient of the quiet sample     | passes       | FAILS (silent channels only) | FAILS                    |
| lo: the lo term of the f16 split dropped for the quiet sample      | passes       | FAILS (the map, K = 72)      | passes (lo = 0 there)    |

The `row` bug is invisible to a bar relative to the sum over ALL samples (the quiet sample's share is 2^-16) except for the
channels in which the sparse upstream gradient happens to be zero in the loud samples; exact arithmetic sees it in every
channel.  The same row missing from the w1 gradient is caught by NEITHER check on the wide case: that sum runs over
samples whose terms are 2^32 apart, outside any exactness budget; on the 'narrow' case (2^0, 2^-2, 2^1), where the exact
comparison covers w1, the round-2 rule is no longer blind to it either.  The `lo` bug needs a short sum: the worst-case bar
2 (K + 2) 2^-24 S grows with K while the dropped terms add up like sqrt(K); it is caught at C = 8, k = 3, not at C = 17, k = 5.
"""
import pytest
import torch
import torch.nn.functional as F

import fc_util as U

ALL = U.SHAPES + [U.COLLAPSE]
OUT = ("logits", "g_s", "g_t", "g_f", "g_w0", "g_b0", "g_w1", "g_b1")


# ---------------------------------------------------------------------------------- references
@pytest.mark.parametrize("shape", [(5, 3, 17, 7, 5), (3, 3, 17, 7, 5), (5, 2, 16, 2, 9)], ids=str)
def test_layer_reference_agrees_with_the_oracle(oracle, shape):
    """the 'sample the convolved map' reference against the reference's own composition on the oracle's literal kernels"""
    from oracle import cpu_modules
    c = U.make_case(shape, False, "narrow")
    k = c["k"]
    r = U.layer_reference(c)
    leaf = [c[n].clone().requires_grad_() for n in ("s", "t", "f", "w0", "b0", "w1", "b1")]
    s, t, f, w0, b0, w1, b1 = leaf
    bs = cpu_modules._BlockExtractorCPU.apply(s, f, k)
    bt = cpu_modules._BlockExtractorCPU.apply(t, torch.zeros_like(f), k)
    hidden = F.conv2d(torch.cat((bt, bs), 1), w0, b0, stride=k)
    logits = F.conv2d(F.leaky_relu(hidden, c["slope"]), w1.reshape(k * k, 128, 1, 1), b1)
    logits.backward(c["up"])
    assert (r["hidden"] - hidden.detach()).abs().max() <= 1e-11 * hidden.detach().abs().max()
    assert (r["logits"] - logits.detach()).abs().max() <= 1e-11 * logits.detach().abs().max()
    for n, v in zip(OUT[1:], (s, t, f, w0, b0, w1, b1)):
        assert (r[n] - v.grad).abs().max() <= 1e-10 * max(1e-30, float(v.grad.abs().max())), n


@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
def test_half_references_are_conv2d_on_replicate_padding(shape):
    """the stage functions the bars are built from (dgrad_pad + fold, wgrad) against autograd of F.conv2d(F.pad(replicate))"""
    c = U.make_case(shape, False, "wide")
    k, H, W = c["k"], c["H"], c["W"]
    for half in (0, 1):
        r = U.half_reference(c, half)
        gx = U.fold(U.dgrad_pad(r["dG"], r["w"], k), k, half, H, W)
        assert (gx - r["gx"]).abs().max() <= 1e-12 * r["gx"].abs().max()
        assert (U.wgrad(r["xp"], r["dG"], k) - r["gw"]).abs().max() <= 1e-12 * r["gw"].abs().max()
        full = U.layer_reference(c)
        want = F.conv2d(F.pad(c["s" if half else "t"], U.pads(k, half), mode="replicate"), U.half_weights(c["w0"], c["C"], half))
        assert torch.equal(full["Gs" if half else "Gt"], want)


# ---------------------------------------------------------------------------------- the exactness condition
@pytest.mark.parametrize("spread", ["wide", "narrow"])
@pytest.mark.parametrize("shape", ALL, ids=str)
def test_exactness_condition_of_the_whole_layer_cases(shape, spread):
    """sum |terms| < 2^21 quantum at every stage the GPU file compares with torch.equal, the f16 operand condition (at most 11
    significant bits, a multiple of the smallest f16 subnormal in the tensor's scale) and the fixed-point cells of the scatter"""
    c = U.make_case(shape, True, spread)
    rep = U.layer_exactness(c)
    print(shape, spread, {n: (v if isinstance(v, bool) else round(v, 4)) for n, v in rep.items()})
    assert U.exact_ok(rep, spread), rep
    for n in ("s", "t", "f", "w0", "b0", "w1", "b1", "up"):
        assert torch.equal(c[n].float().double(), c[n])
    if spread == "wide":    # gfla_fc_forward_f16 stores the maps as f16
        assert torch.equal(c["s"].half().double(), c["s"]) and torch.equal(c["t"].half().double(), c["t"])
    frac = (c["f"] - torch.floor(c["f"]))
    assert bool(((frac == 0.25) | (frac == 0.5) | (frac == 0.75)).all())
    dx = c["f"][:, 0] + torch.arange(c["W"]).double()
    assert bool((dx < -c["k"]).any() or (dx > c["W"] + c["k"]).any()), "no out-of-range position"
    assert float((U.layer_reference(c)["hidden"] == 0).double().mean()) > 0, "no hidden unit exactly on the kink"


@pytest.mark.parametrize("shape", [s for s in U.SHAPES if s[0] == 3], ids=str)
def test_exactness_condition_of_the_offset_cases(shape):
    """the whole layer of mode 5 at k = 3 (Winograd-domain forward): the backward stages it compares satisfy the condition, and
    no hidden unit is nearer to 0 than 2^-7 -- four times what a float32 Winograd forward (host emulation) moves it by at most"""
    c = U.make_case(shape, True, "offset")
    rep = U.layer_exactness(c)
    assert all(rep[n] < 1.0 for n in U.OFFSET_STAGES) and rep["fixed"] and rep["f16"], rep
    r = U.layer_reference(c)
    k, C, H, W = c["k"], c["C"], c["H"], c["W"]
    Gs32 = U.wn_conv(r["sp"], c["w0"][:, C:], H + k - 1, W + k - 1, k, torch.float32).double()
    Gt32 = U.wn_conv(r["tp"], c["w0"][:, :C], H, W, k, torch.float32).double()
    h32 = c["b0"].reshape(1, -1, 1, 1) + Gt32 + U.sample_map(Gs32, r["idx"], r["wts"], H, W)
    err = float((h32 - r["hidden"]).abs().max())
    print(shape, "min |hidden| %.4g, float32 Winograd emulation moves hidden by at most %.3g" % (float(r["hidden"].abs().min()), err))
    assert float(r["hidden"].abs().min()) >= U.OFFSET and U.WINO_MARGIN * err < U.OFFSET
    if c["B"] > 1:   # a quiet sample next to a loud one under the gradient maps' single scale
        assert float(c["up"].abs().amax((1, 2, 3)).min() / c["up"].abs().max()) <= 2.0 ** -8


@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
def test_exactness_condition_of_the_half_cases(shape):
    for half in (0, 1):
        wide, narrow = U.half_exactness(U.make_case(shape, True, "wide"), half), U.half_exactness(U.make_case(shape, True, "narrow"), half)
        assert wide["y"] < 1 and wide["gx"] < 1 and wide["f16"], wide
        assert narrow["gw"] < 1 and narrow["f16"], narrow


def test_quantum_helper():
    t = torch.tensor([0.0, 1.0, 3.0, 0.75, 6 * 2.0 ** -20, -5 * 2.0 ** 7], dtype=torch.float64)
    assert U.lsb(t).tolist() == [float("inf"), 1.0, 1.0, 0.25, 2.0 ** -19, 2.0 ** 7]
    assert U.f16_operand_ok(torch.tensor([1.0, 2047.0, 2.0 ** -10])) and not U.f16_operand_ok(torch.tensor([2049.0]))
    assert not U.f16_operand_ok(torch.tensor([1.0, 2.0 ** -40]))     # below the smallest f16 subnormal of the tensor's scale


# ---------------------------------------------------------------------------------- flow-gradient exclusion, Winograd emulation
@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
def test_flow_gradient_exclusion_cap(shape):
    for spread in ("wide", "quiet8"):
        lb = U.layer_bars(shape, spread, 0)
        share = float(lb["flow_excluded"].double().mean())
        print(shape, spread, "excluded share %.4f" % share)
        assert share <= 0.10


@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
def test_winograd_emulation(shape):
    """the transcription of fc_wino_shared.h: exact in float64; in float32 it is within its own measured c (printed: the
    constants the GPU bars use, 4 c 2^-24 S_tile)"""
    k = shape[0]
    for half in (0, 1):
        hb = U.half_bars(shape, half)
        r = hb["ref"]
        Ho, Wo = r["dG"].shape[2:]
        y64 = U.wn_conv(r["xp"], r["w"], Ho, Wo, k, torch.float64)
        assert (y64 - r["y"]).abs().max() <= 1e-12 * r["y"].abs().max()
        gp64 = U.wn_conv(U.z_lin(r["dG"], k), r["w"].flip(2, 3).transpose(0, 1), r["xp"].shape[2], r["xp"].shape[3], k, torch.float64)
        assert (gp64 - hb["emul"]["gp64"]).abs().max() <= 1e-12 * hb["emul"]["gp64"].abs().max()
        gw64 = U.wn_wgrad(r["xp"], r["dG"], k, torch.float64)
        assert (gw64 - r["gw"]).abs().max() <= 1e-12 * r["gw"].abs().max()
        print("k %d %s half %d: c fwd %.2f dgrad %.2f wgrad %.2f" % (k, shape, half, hb["c_y"], hb["c_gx"], hb["c_gw"]))
        for n, St, e32, w64 in (("c_y", hb["St_y"], hb["emul"]["y"], r["y"]), ("c_gw", hb["St_w"], hb["emul"]["gw"], r["gw"])):
            assert 0 < hb[n] < 200, (n, hb[n])
            assert bool(((e32 - w64).abs() <= hb[n] * U.U * St * (1 + 1e-12)).all())
        assert 0 < hb["c_gx"] < 200
        assert bool(((hb["emul"]["gp"] - hb["emul"]["gp64"]).abs() <= hb["c_gx"] * U.U * hb["St_x"] * (1 + 1e-12)).all())


# ---------------------------------------------------------------------------------- planted bugs
BUGS = {  # bug: (shape, mode whose bars judge the float case, outputs the bug reaches)
    "tap": ((5, 3, 17, 7, 5), 0, OUT), "chunk": ((5, 3, 17, 7, 5), 0, OUT), "reflect": ((3, 3, 17, 7, 5), 0, OUT),
    "scatter": ((3, 3, 17, 7, 5), 0, ("g_s",)), "row": ((5, 3, 17, 7, 5), 0, ("g_b1",)), "lo": ((3, 2, 8, 33, 65), 2, ("Gs",)),
}
EXPECT = {"tap": (True, True), "chunk": (True, True), "reflect": (True, True), "scatter": (True, True), "row": (True, True),
          "lo": (True, False)}   # (the per-element bar fails it, the exact case fails it): the table of the module docstring


def _bugged(c, bug):
    """the layer's outputs with the planted bug, and without"""
    ref = U.layer_reference(c)
    if bug in ("tap", "chunk", "reflect", "lo"):
        return U.layer_reference(c, bug), ref   # ('lo' is judged on the convolved source map, where the per-half GPU test judges it)
    out = {n: ref[n].clone() for n in OUT}
    q, k = U.quiet_sample(c), c["k"]
    if bug == "scatter":   # the first corner of one position of the quiet sample whose d hidden is not zero
        p = int((ref["dh"][q].abs().sum(0).reshape(-1) > 0).nonzero()[0])
        delta = torch.zeros_like(ref["dGs"])
        delta[q].reshape(128, -1)[:, int(ref["idx"][0][q, 0, p])] = ref["dh"][q].reshape(128, -1)[:, p] * ref["wts"][0][q, 0, p]
        out["g_s"] = ref["g_s"] - U.fold(U.dgrad_pad(delta, c["w0"][:, c["C"]:], k), k, 1, c["H"], c["W"])
    elif bug == "row":
        out["g_b1"] = ref["g_b1"] - c["up"][q, :, -1, :].sum(-1)
    return out, ref


@pytest.mark.parametrize("bug", list(BUGS))
def test_planted_bug(bug):
    shape, mode, outs = BUGS[bug]
    # float case: the round-2 rule and the per-element bar
    lb = U.layer_bars(shape, "wide", mode)
    got, ref = _bugged(lb["case"], bug)
    assert any(not torch.equal(got[n], ref[n]) for n in outs), "the planted bug changes nothing"
    for n in outs:
        assert U.old_rule(got[n], ref[n], 1e-5 if n in ("logits", "Gs") else 2e-5), "round-2 rule sees %s in %s (float case)" % (bug, n)
    keep = ~lb["flow_excluded"]
    bars = dict(lb["bar"])     # (layer_bars is cached and shared: nothing is written into its result)
    if "Gs" in outs:
        bars["Gs"] = U.half_bar(U.half_bars(shape, 1, "wide"), mode, "fwd")
    ratios = {n: U.worst_ratio(got[n][keep] if n == "g_f" else got[n], ref[n][keep] if n == "g_f" else ref[n],
                               bars[n].reshape(ref[n].shape)[keep] if n == "g_f" else bars[n].reshape(ref[n].shape)) for n in outs}
    bar_fails = any(v > 1.0 for v in ratios.values())
    # exact case: the round-2 rule and torch.equal on the outputs the GPU file compares
    c = U.make_case(shape, True, "wide")
    got, ref = _bugged(c, bug)
    for n in outs:
        assert U.old_rule(got[n], ref[n], 1e-5 if n in ("logits", "Gs") else 2e-5), "round-2 rule sees %s in %s (exact case)" % (bug, n)
    exact_fails = any(not torch.equal(got[n], ref[n]) for n in outs if n in U.EXACT_OUTPUTS["wide"] + ("Gs",))
    print("%-8s worst err/bar %s -> bar %s, exact case %s" % (bug, {n: "%.3g" % v for n, v in ratios.items()},
                                                              "FAILS" if bar_fails else "passes", "FAILS" if exact_fails else "passes"))
    assert (bar_fails, exact_fails) == EXPECT[bug]
    assert bar_fails or exact_fails
