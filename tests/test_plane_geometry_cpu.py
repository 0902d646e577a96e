"""What tests/test_plane_geometry_gpu.py stands on, checked without a GPU:

  1. the float64 evaluations of tests/plane_util.py against the CPU oracle (1e-12); resample2d with one sigma per pixel as
     well, all three channels of d/d input2, d/d sigma also against autograd of the forward; and a number for sigma still
     gives the bits it gave before sigma could be a field;
  2. the share of d/d flow entries left out as kinks, on the exact inputs of the GPU cases: at most 10 %, the planted lattice
     points of the `smooth` flow counted separately; and no resample2d coordinate of any case floors differently in the
     kernels' arithmetic (its forward jumps there, and nothing is ever left out of a forward result);
  3. the power of the bar: the float64 reference rounded once to the storage type passes, and three planted bugs fail it;
     with a sigma field, sigma taken from the pixel to the left, from the previous sample or from the sample's first pixel,
     and 1 / sigma^2 for 1 / sigma^3 in d/d sigma, each put more than a quarter of the entries beyond it;
  4. the host-side geometry query (gfla_lds_plane_geometry) under the tuning keys that force a geometry, with the guard that
     keeps key 5 away from the kernels that cannot split."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import plane_util as pu
from util import rand, randn

F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16


def _close(got, want, what):
    scale = max(1.0, want.abs().max().item())
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * scale, "%s: %.3e" % (what, err)


# ----------------------------------------------------------------------------------------- 1. references against the oracle
@pytest.mark.parametrize("kind", ("coherent", "wild", "smooth"))
@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_block_extractor_reference_matches_the_oracle(oracle, k, kind):
    for shape in pu.SHAPES[:2]:
        s, f, up = pu.inputs("be", shape, F64, kind, k)
        ref = pu.block_extractor(s, f, up, k)
        _close(ref["out"][0], oracle.block_extractor_fwd(s, f, k), "out")
        gs, gf = oracle.block_extractor_bwd(s, f, up, k)
        _close(ref["g_source"][0], gs, "g_source")
        _close(ref["g_flow"][0], gf, "g_flow")
        # the unfold layout is a permutation of the same numbers
        assert torch.equal(pu.patches_from_unfold(pu.unfold_from_patches(up, k), k), up)


@pytest.mark.parametrize("kind", ("coherent", "wild"))
@pytest.mark.parametrize("k", [3, 5])
def test_aggregate_reference_matches_the_oracle(oracle, k, kind):
    for shape in pu.SHAPES[:2]:
        s, f, lg, up = pu.inputs("agg", shape, F64, kind, k)
        fwd = pu.aggregate_forward(s, f, lg, k)
        bs = oracle.block_extractor_fwd(s, f, k)
        lgr = lg.clone().requires_grad_()
        attn = F.softmax(lgr, 1)
        full = oracle.local_attn_reshape_fwd(attn.detach().contiguous(), k)
        _close(fwd["attn"][0], attn.detach(), "attn")
        _close(fwd["out"][0], F.avg_pool2d(full * bs, k, k), "out")
        F.avg_pool2d(F.pixel_shuffle(attn, k) * bs, k, k).backward(up)
        bwd = pu.aggregate_backward(s, f, fwd["attn"][0], up, k)
        _close(bwd["g_logits"][0], lgr.grad, "g_logits")
        g_bs = full * up.repeat_interleave(k, 2).repeat_interleave(k, 3) / (k * k)
        gs, gf = oracle.block_extractor_bwd(s, f, g_bs.contiguous(), k)
        _close(bwd["g_source"][0], gs, "g_source")
        _close(bwd["g_flow"][0], gf, "g_flow")


@pytest.mark.parametrize("kind", ("coherent", "wild", "smooth"))
@pytest.mark.parametrize("k,dil", [(4, 1), (2, 1), (4, 2)])
def test_resample2d_reference_matches_the_oracle(oracle, k, dil, kind):
    for shape in pu.SHAPES[:2]:
        B, C, Hi, Wi, H, W = shape
        i1, f, up = pu.inputs("rs", shape, F64, kind, k)
        ref = pu.resample2d(i1, f, up, k, dil)
        i2 = torch.cat((f, torch.full((B, 1, H, W), pu.SIGMA, dtype=F64)), 1).contiguous()
        _close(ref["out"][0], oracle.resample2d_fwd(i1, i2, k, dil), "out")
        g1, g2 = oracle.resample2d_bwd(i1, i2, up, k, dil, trunc_compat=True)
        _close(ref["g_input1"][0], g1, "g_input1")
        _close(ref["g_flow"][0], g2[:, :2], "g_flow")
    # the quirk is in: on a wild flow the reference's d/d input1 differs from the forward's true gradient (kernel_size 2
    # cannot show it: for a coordinate in (-1, 0) both taps are the border pixel and the normalised weights sum to 1)
    if kind == "wild" and k == 4:
        g1_true, _ = oracle.resample2d_bwd(i1, i2, up, k, dil, trunc_compat=False)
        assert (ref["g_input1"][0] - g1_true).abs().max().item() > 1e-3


RS_FIELD_KD = [(4, 1), (2, 1), (4, 2), (6, 1)]       # the (kernel_size, dilation) of the GPU file's sigma-field cases


@pytest.mark.parametrize("field", pu.SIGMA_FIELDS)
@pytest.mark.parametrize("kind", ("coherent", "wild", "smooth"))
@pytest.mark.parametrize("k,dil", RS_FIELD_KD + [(2, 2), (6, 2)])
def test_resample2d_sigma_field_reference_matches_the_oracle(oracle, k, dil, kind, field):
    """One sigma per pixel: the forward, d/d input1 and all three channels of d/d input2 against the oracle, and d/d sigma
    against autograd of the float64 forward as well."""
    for shape in pu.SHAPES[:2]:
        i1, f, up, sig = pu.rs_sigma_inputs(shape, F64, kind, k, field)
        ref = pu.resample2d(i1, f, up, k, dil, sigma=sig)
        i2 = torch.cat((f, sig), 1).contiguous()
        _close(ref["out"][0], oracle.resample2d_fwd(i1, i2, k, dil), "out")
        g1, g2 = oracle.resample2d_bwd(i1, i2, up, k, dil, trunc_compat=True)
        _close(ref["g_input1"][0], g1, "g_input1")
        _close(ref["g_flow"][0], g2[:, :2], "g_flow")
        _close(ref["g_sigma"][0], g2[:, 2:], "g_sigma")
        leaf = sig.clone().requires_grad_()
        out = pu.resample2d(i1, f, None, k, dil, sigma=leaf)["out"][0]
        _close(ref["g_sigma"][0], torch.autograd.grad(out, leaf, up)[0], "g_sigma against autograd")
        assert ref["g_sigma"][0].abs().max().item() > 1e-3            # (not a comparison of zeros)
        assert tuple(ref["g_sigma"][0].shape) == tuple(sig.shape)


def _resample2d_before(i1, f, up, k, dil, sigma, xmax_shift=0):
    """plane_util.resample2d as it was while sigma could only be a number, kept to pin its bits: expression by expression
    the same evaluation, without d/d sigma"""
    def axis(c, n_src, frac, hi_shift=0):
        c0, taps = c.floor().long(), []
        for t in range(k // 2):
            near, far = t * dil + frac, (1 + t) * dil - frac
            w_n, w_f = torch.exp(-near * near / (2 * sigma * sigma)), torch.exp(-far * far / (2 * sigma * sigma))
            taps.append(((c0 - t * dil).clamp(0, n_src - 1 - hi_shift), w_n, -near / (sigma * sigma) * w_n))
            taps.append(((c0 + (t + 1) * dil).clamp(0, n_src - 1 - hi_shift), w_f, far / (sigma * sigma) * w_f))
        return taps

    i1, f, up = i1.double(), f.double(), up.double()
    B, C, Hi, Wi = i1.shape
    H, W = f.shape[2:]
    xf = torch.arange(W, dtype=torch.float64).view(1, 1, W) + f[:, 0]
    yf = torch.arange(H, dtype=torch.float64).view(1, H, 1) + f[:, 1]
    cols, rows = axis(xf, Wi, xf - xf.floor(), xmax_shift), axis(yf, Hi, yf - yf.floor())
    flat = i1.reshape(B, C, Hi * Wi)
    S = (sum(w for _, w, _ in rows) * sum(w for _, w, _ in cols)).unsqueeze(1)
    Dx = (sum(w for _, w, _ in rows) * sum(d for _, _, d in cols)).unsqueeze(1)
    Dy = (sum(d for _, _, d in rows) * sum(w for _, w, _ in cols)).unsqueeze(1)
    val, mag, vx, vy, term = 0, 0, 0, 0, torch.zeros(B, C, H, W, dtype=torch.float64)
    for r, wy, dwy in rows:
        for q, wx, dwx in cols:
            v = flat.gather(2, (r * Wi + q).view(B, 1, H * W).expand(B, C, H * W)).view(B, C, H, W)
            val = val + (wy * wx).unsqueeze(1) * v
            mag = mag + (wy * wx).unsqueeze(1) * v.abs()
            vx = vx + (wy * dwx).unsqueeze(1) * v
            vy = vy + (dwy * wx).unsqueeze(1) * v
            term = torch.maximum(term, ((wy * wx).unsqueeze(1) * v).abs())
    res = {"out": (val / S, mag / S, 2 * k * k), "out_term": term / S}
    gf = torch.stack([(up * (vx / S - val * Dx / (S * S))).sum(1), (up * (vy / S - val * Dy / (S * S))).sum(1)], 1)
    kappa = max(1.0, (k // 2) * dil / (sigma * sigma))
    res["g_flow"] = (gf, (2 * kappa * (up.abs() * mag / S).sum(1, keepdim=True)).expand(B, 2, H, W).contiguous(), 2 * C * k * k + 2 * k * k)
    cols1, rows1 = axis(xf, Wi, xf - xf.trunc(), xmax_shift), axis(yf, Hi, yf - yf.trunc())
    S1 = (sum(w for _, w, _ in rows1) * sum(w for _, w, _ in cols1)).unsqueeze(1)
    g1, A_g1, cnt = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros(B, 1, Hi * Wi, dtype=torch.float64)
    for r, wy, _ in rows1:
        for q, wx, _ in cols1:
            at = (r * Wi + q).view(B, 1, H * W)
            wn = (wy * wx).unsqueeze(1) / S1
            g1.scatter_add_(2, at.expand(B, C, H * W), (wn * up).reshape(B, C, H * W))
            A_g1.scatter_add_(2, at.expand(B, C, H * W), (wn * up.abs()).reshape(B, C, H * W))
            cnt.scatter_add_(2, at, torch.ones(B, 1, H * W, dtype=torch.float64))
    res["g_input1"] = (g1.view(B, C, Hi, Wi), A_g1.view(B, C, Hi, Wi), cnt.view(B, 1, Hi, Wi) + k * k)
    res["g_input1_count"] = cnt.view(B, 1, Hi, Wi)
    return res


def _same_entry(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same_entry(x, y) for x, y in zip(a, b))
    return torch.equal(a, b) if torch.is_tensor(a) else (not torch.is_tensor(b) and a == b)


@pytest.mark.parametrize("k,dil", [(4, 1), (2, 1), (4, 2)])
def test_resample2d_with_a_number_for_sigma_keeps_its_bits(k, dil):
    """The cases of before the sigma fields (a number for sigma) are evaluated to the same bits, entry by entry; and a
    constant field of that number gives those bits too."""
    for shape, kind, dtype in ((pu.SHAPES[1], "wild", F32), (pu.SHAPES[0], "smooth", BF16)):
        B, C, Hi, Wi, H, W = shape
        i1, f, up = pu.inputs("rs", shape, dtype, kind, k)
        for shift in (0, 1):
            want = _resample2d_before(i1, f, up, k, dil, pu.SIGMA, shift)
            got = pu.resample2d(i1, f, up, k, dil, xmax_shift=shift)
            as_field = pu.resample2d(i1, f, up, k, dil, torch.full((B, 1, H, W), pu.SIGMA, dtype=dtype), shift)
            assert sorted(got) == sorted(list(want) + ["g_sigma"]) == sorted(as_field)
            for name in want:
                assert _same_entry(got[name], want[name]), name
                assert _same_entry(as_field[name], want[name]), name
            assert _same_entry(as_field["g_sigma"], got["g_sigma"])
        assert pu.rs_kappa(k, dil) == max(1.0, (k // 2) * dil / 4.0) and pu.rs_kappa(4, 2, 1.0) == 4.0
        field = torch.tensor([1.0, 1.5, 2.0, 3.5], dtype=dtype).view(1, 1, 2, 2)
        assert torch.equal(pu.rs_kappa(k, dil, field), torch.tensor([pu.rs_kappa(k, dil, s) for s in (1.0, 1.5, 2.0, 3.5)], dtype=F64).view(1, 1, 2, 2))


def test_sigma_fields_are_what_the_bar_assumes():
    for dtype in (F32, F64, F16, BF16):
        for B, H, W in ((2, 14, 10), (3, 6, 7), (1, 48, 32)):
            lv = pu.sigma_field("levels", B, H, W, dtype, 1).double()
            assert sorted(lv.unique().tolist()) == [1.0, 1.5, 2.0, 2.5, 3.0, 3.5]
            assert (lv[..., 1:] != lv[..., :-1]).all() and (lv[:, :, 1:] != lv[:, :, :-1]).all() and (lv[1:] != lv[:-1]).all()
            rd = pu.sigma_field("random", B, H, W, dtype, 1)
            assert rd.dtype == dtype and tuple(rd.shape) == (B, 1, H, W) and rd.double().unique().numel() > 32       # (bfloat16 has 225 values there)
            for s in (lv, rd.double()):
                assert s.min().item() >= 1.0 and s.max().item() <= 3.5
            assert not torch.equal(rd, pu.sigma_field("random", B, H, W, dtype, 2))


# --------------------------------------------------------------------------------------------------- 2. the exclusion cap
def test_flow_gradient_exclusions_stay_under_the_cap_on_the_gpu_inputs():
    shares = {}
    for dtype in (F32, F64, F16, BF16):
        for kind in (pu.KINDS16 if dtype in (F16, BF16) else pu.KINDS):
            for shape in pu.SHAPES + [pu.WINDOW_FWD_SHAPE]:
                B, C, Hs, Ws, Hf, Wf = shape
                plant = pu.planted(B, Hf, Wf) if kind == "smooth" else torch.zeros(B, 2, Hf, Wf, dtype=torch.bool)
                masks = []
                extra = shape == pu.WINDOW_FWD_SHAPE          # float32 forwards only: k 3, 5 and Resample2d(4, 1 / 2)
                if extra and (dtype != F32 or kind == "oob"):
                    continue
                for k in ((3, 5) if extra else (2, 3, 4, 5)):
                    f = pu.inputs("be", shape, dtype, kind, k)[1]
                    masks.append(("be k%d" % k, pu.be_flow_kinks(f, k, Hs, Ws, pu.ARITH[dtype])))
                for k, dil in (((4, 1), (4, 2)) if extra else ((4, 1), (2, 1), (4, 2))):
                    f = pu.inputs("rs", shape, dtype, kind, k)[1]
                    masks.append(("rs k%d d%d" % (k, dil), pu.rs_flow_kinks(f, k, dil, Hs, Ws, pu.ARITH[dtype])))
                    # resample2d's forward jumps at an integer coordinate: the two arithmetics must agree on every floor
                    assert torch.equal(pu.rs_coordinates(f, pu.ARITH[dtype]).floor().double(), pu.rs_coordinates(f).floor())
                for name, m in masks:
                    if kind == "smooth":
                        assert m[plant].float().mean().item() > 0.5          # the planted points are kinks, as meant
                    share = (m & ~plant).float().mean().item()
                    key = (str(dtype).split(".")[1], kind)
                    shares[key] = max(shares.get(key, 0.0), share)
                    assert share <= 0.10, "%s %s %s %s: %.1f %% of the d/d flow entries are kinks" % (name, shape, dtype, kind, 100 * share)
    print("largest share of d/d flow entries left out, per storage type and flow kind:")
    for key in sorted(shares):
        print("  %-8s %-9s %.2f %%" % (key[0], key[1], 100 * shares[key]))


def test_sigma_field_cases_keep_the_flow_conditions():
    """The sigma-field cases of the GPU file use the flows of `inputs` (kernel_size 6 and the routing shape draw new ones):
    on each of them no coordinate floors differently in the kernels' arithmetic -- the forward and d/d sigma jump there and
    are compared everywhere -- and the d/d flow entries left out stay under the same 10 % cap."""
    import gs_route_util
    for dtype in (F32, F64, F16, BF16):
        for kind in ("wild", "smooth") + (("oob",) if dtype in (F16, BF16) else ()):
            for shape in pu.SHAPES + [gs_route_util.S]:
                B, C, Hs, Ws, Hf, Wf = shape
                if shape == gs_route_util.S and kind != "wild":
                    continue
                plant = pu.planted(B, Hf, Wf) if kind == "smooth" else torch.zeros(B, 2, Hf, Wf, dtype=torch.bool)
                for k, dil in RS_FIELD_KD:
                    f = pu.inputs("rs", shape, dtype, kind, k)[1]
                    assert torch.equal(pu.rs_coordinates(f, pu.ARITH[dtype]).floor().double(), pu.rs_coordinates(f).floor()), (shape, dtype, kind, k)
                    m = pu.rs_flow_kinks(f, k, dil, Hs, Ws, pu.ARITH[dtype])
                    share = (m & ~plant).float().mean().item()
                    assert share <= 0.10, "rs k%d d%d %s %s %s: %.1f %% of the d/d flow entries are kinks" % (k, dil, shape, dtype, kind, 100 * share)
    # the widened 16-bit backward's one case
    f = pu.inputs("rs", gs_route_util.W, BF16, "wild", 4)[1]
    assert torch.equal(pu.rs_coordinates(f, F32).floor().double(), pu.rs_coordinates(f).floor())
    assert pu.rs_flow_kinks(f, 4, 1, gs_route_util.W[2], gs_route_util.W[3], F32).float().mean().item() <= 0.10


# ------------------------------------------------------------------------------------------------- 3. power of the bar
def _round_to(x, dtype):
    return x.to(dtype).double()


def _beyond(got, ref, A, n, P, dtype, keep=None):
    return pu.worst(got, ref, A, n, P, dtype, keep)[1]


def _weight_bug(ref, term):
    """ref with ONE term of ONE element changed by 2^-6 relative: the element where that shows most against its own size"""
    at = (term / ref.abs().clamp_min(1e-30)).flatten().argmax()
    out = ref.clone().flatten()
    out[at] += 2.0 ** -6 * term.flatten()[at]
    return out.view_as(ref)


@pytest.mark.parametrize("dtype", [F32, F64, F16, BF16])
@pytest.mark.parametrize("op", ["be", "agg", "rs"])
def test_bar_passes_the_rounded_reference_and_fails_three_planted_bugs(op, dtype):
    shape, k, dil = pu.SHAPES[0], 3, 1       # C = 7: the last channel is the ragged group of G = 2 and of G = 3
    B, C, Hs, Ws, Hf, Wf = shape
    arith = pu.ARITH[dtype]
    if op == "be":
        s, f, up = pu.inputs("be", shape, dtype, "wild", k)
        P = pu.coordinate_bound(f, k)
        ref = pu.block_extractor(s, f, up, k)
        keep = ~pu.be_flow_kinks(f, k, Hs, Ws, arith)
        no_last = pu.block_extractor(s, f, torch.cat((up[:, :-1], torch.zeros_like(up[:, -1:])), 1), k)["g_flow"][0]
        clamp = pu.block_extractor(s, f, up, k, xmax_shift=1)
        src_name = "g_source"
    elif op == "agg":
        s, f, lg, up = pu.inputs("agg", shape, dtype, "wild", k)
        P = pu.coordinate_bound(f, k)
        ref = pu.aggregate_forward(s, f, lg, k)
        attn = _round_to(ref["attn"][0], dtype)
        ref.update(pu.aggregate_backward(s, f, attn, up, k))
        keep = ~pu.be_flow_kinks(f, k, Hs, Ws, arith)
        no_last = pu.aggregate_backward(s, f, attn, torch.cat((up[:, :-1], torch.zeros_like(up[:, -1:])), 1), k)["g_flow"][0]
        clamp = pu.aggregate_backward(s, f, attn, up, k, xmax_shift=1)
        src_name = "g_source"
    else:
        k = 4
        s, f, up = pu.inputs("rs", shape, dtype, "wild", k)
        P = pu.coordinate_bound(f, (k // 2) * dil) * pu.rs_kappa(k, dil) ** 2
        ref = pu.resample2d(s, f, up, k, dil)
        keep = ~pu.rs_flow_kinks(f, k, dil, Hs, Ws, arith)
        no_last = pu.resample2d(s, f, torch.cat((up[:, :-1], torch.zeros_like(up[:, -1:])), 1), k, dil)["g_flow"][0]
        clamp = pu.resample2d(s, f, up, k, dil, xmax_shift=1)
        src_name = "g_input1"
    assert keep.float().mean().item() >= 0.9
    # the reference, rounded once to the storage type, passes everywhere
    for name in ("out", src_name, "g_flow") + (("attn", "g_logits") if op == "agg" else ()):
        r, A, n = ref[name]
        assert _beyond(_round_to(r, dtype), r, A, n, P, dtype, keep if name == "g_flow" else None) == 0, name
    # (a) one tap weight of one pixel off by 2^-6
    r, A, n = ref["out"]
    assert _beyond(_round_to(_weight_bug(r, ref["out_term"]), dtype), r, A, n, P, dtype) >= 1
    # (b) the last channel of a ragged group dropped from d/d flow
    r, A, n = ref["g_flow"]
    assert _beyond(_round_to(no_last, dtype), r, A, n, P, dtype, keep) >= 1
    # (c) one border column's clamp moved by one: seen by the gradient of the feature map (and by d/d flow)
    r, A, n = ref[src_name]
    assert _beyond(_round_to(clamp[src_name][0], dtype), r, A, n, P, dtype) >= 1
    r, A, n = ref["g_flow"]
    assert _beyond(_round_to(clamp["g_flow"][0], dtype), r, A, n, P, dtype, keep) >= 1


def _share_beyond(got, entry, P, dtype, keep=None):
    ref, A, n = entry
    total = ref.numel() if keep is None else int(keep.expand_as(ref).sum().item())
    return _beyond(_round_to(got, dtype), ref, A, n, P, dtype, keep) / float(total)


@pytest.mark.parametrize("field", pu.SIGMA_FIELDS)
@pytest.mark.parametrize("dtype", [F32, F64, F16, BF16])
def test_bar_sees_a_sigma_read_at_the_wrong_pixel(dtype, field):
    """With one sigma per pixel the float64 reference rounded once to the storage type passes all four outputs, and a result
    computed from sigma one pixel to the left, one sample back, or from the first pixel of the sample is beyond the bar in
    more than a quarter of the entries of the forward, of d/d flow and of d/d sigma; so is d/d sigma with 1 / sigma^2 for
    1 / sigma^3."""
    shape, k, dil = pu.SHAPES[0], 4, 1
    B, C, Hs, Ws, Hf, Wf = shape
    s, f, up, sig = pu.rs_sigma_inputs(shape, dtype, "wild", k, field)
    kappa2 = pu.rs_kappa(k, dil, sig) ** 2
    P = pu.coordinate_bound(f, (k // 2) * dil) * kappa2
    ref = pu.resample2d(s, f, up, k, dil, sigma=sig)
    keep = ~pu.rs_flow_kinks(f, k, dil, Hs, Ws, pu.ARITH[dtype])
    assert keep.float().mean().item() >= 0.9
    for name in ("out", "g_input1", "g_flow", "g_sigma"):
        share = _share_beyond(ref[name][0], ref[name], P.max().item() if name == "g_input1" else P, dtype, keep if name == "g_flow" else None)
        assert share == 0, (name, share)
    wrong = {"left": sig.roll(1, 3), "sample": sig.roll(1, 0), "first": sig[:, :, :1, :1].expand_as(sig).contiguous()}
    for what, other in wrong.items():
        bug = pu.resample2d(s, f, up, k, dil, sigma=other)
        for name in ("out", "g_flow", "g_sigma"):
            share = _share_beyond(bug[name][0], ref[name], P, dtype, keep if name == "g_flow" else None)
            print("sigma from %-6s %-8s %.1f %% beyond the bar" % (what, name, 100 * share))
            assert share > 0.25, (what, name, share)
    bug = pu.resample2d(s, f, up, k, dil, sigma=sig, sigma_power=2)
    share = _share_beyond(bug["g_sigma"][0], ref["g_sigma"], P, dtype)
    print("1 / sigma^2 for 1 / sigma^3: g_sigma %.1f %% beyond the bar" % (100 * share))
    assert share > 0.25, share


# ---------------------------------------------------------------------------------------------------------- 4. the query
OPS_BWD16_NO_SPLIT = (0, 1, 2, 3, 6)      # kernels that flush each plane from one owner in 16-bit storage


def test_query_reports_the_forced_geometries_and_key_5_respects_allow_split(gfla):
    from global_flow_local_attention_amd import _lib
    assert "gfla_lds_plane_geometry" in _lib.extension_symbols() and _lib.ABI_VERSION == 8
    q = lambda *a, **kw: pu.query(_lib, *a, **kw)
    # keys at 0: every small shape of the older suites runs with one plane per workgroup -- the gap this file's GPU twin closes
    for op in range(8):
        g = q(op, (2, 8, 16, 12, 16, 12), 4 if op >= 5 else 3)
        assert g["G"] == 1 and g["ngroups"] == 8 and g["split"] == 1 and g["margin"] < 0, (op, g)
    g = q(0, (32, 256, 32, 22, 32, 22), 3)                          # a bench shape: the heuristic's own G, ragged
    assert g["G"] > 1 and 256 % g["G"] != 0 and g["ngroups"] == -(-256 // g["G"])
    with gfla.tuned({gfla.TUNE_G_CAP: 3}):
        for op in range(8):
            for elem in (2, 4, 8):
                g = q(op, pu.SHAPES[0], 4 if op >= 5 else 3, elem=elem)
                assert (g["G"], g["ngroups"]) == (3, 3), (op, elem, g)           # C = 7: groups of 3, 3, 1
    with gfla.tuned({gfla.TUNE_SPLIT: 3}):
        for op in range(8):
            for elem in (2, 4, 8):
                g = q(op, pu.SHAPES[0], 4 if op >= 5 else 3, elem=elem)
                want = 1 if (elem == 2 and op in OPS_BWD16_NO_SPLIT) else 3
                assert g["split"] == want and g["per"] == -(-140 // want), (op, elem, g)
    # the two callers the issue names, once more by name: 16-bit block_extractor backward and resample2d d/d input1
    with gfla.tuned({gfla.TUNE_SPLIT: 3}):
        assert q(0, pu.SHAPES[3], 3, elem=2)["split"] == 1 and q(0, pu.SHAPES[3], 3, elem=4)["split"] == 3
        assert q(6, pu.SHAPES[3], 4, elem=2)["split"] == 1 and q(6, pu.SHAPES[3], 4, elem=4)["split"] == 3
        assert q(0, pu.SHAPES[3], 3, elem=4)["per"] == 703            # 2109 = 3 x 703 = 19 rows of 37: ends inside a flow row
    # key 10 = 16: 48 x 32 x 12 B > 16 KB.  With only 8 such planes the tile kernels of csrc/tile_map.h take the call first
    # (B C < 4 workgroups per CU: gfla_big_plane_geometry's regime), so the family reports G = 0; key 30 = 1 switches those
    # off and the same planes run as ROW WINDOWS
    with gfla.tuned({gfla.TUNE_LDS_KB: 16}):
        assert q(0, pu.SHAPES[2], 3, elem=4)["G"] == 0
    with gfla.tuned(pu.WINDOWS):
        # block_extractor backward (12 B per element) at 48 x 32, resample2d d/d input1 (8 B) at 57 x 37; resample2d's gather
        # planes (4 B) fit 16 KB at every shape of the GPU file and stay whole
        for op, k, shape in ((0, 3, pu.SHAPES[2]), (0, 5, pu.SHAPES[2]), (0, 3, pu.SHAPES[3]), (6, 4, pu.SHAPES[3])):
            g = q(op, shape, k, elem=4)
            assert g["G"] >= 1 and g["margin"] >= 0 and g["lds"] <= 16 * 1024 and g["split"] > 1, (op, g)
        assert q(5, pu.SHAPES[3], 4, elem=4)["margin"] < 0 and q(7, pu.SHAPES[3], 4, elem=4)["margin"] < 0
        assert q(0, pu.SHAPES[2], 3, elem=2)["G"] == 0                # 16-bit backward: whole planes or nothing
        assert q(6, pu.SHAPES[3], 4, elem=2)["G"] == 0                # 57 x 37 x 8 B > 16 KB
        assert q(0, pu.SHAPES[0], 3, elem=4)["margin"] < 0            # 14 x 10 planes fit whatever the budget
    g = q(0, pu.SHAPES[2], 3, elem=4)
    assert g["margin"] < 0 and g["lds"] <= 64 * 1024                   # default budget: whole planes
    assert q(0, pu.SHAPES[3], 3, elem=4)["split"] == 2                 # 2109 pixels: the heuristic splits in two
    # arguments
    L = _lib.lib()
    out = (ctypes.c_int64 * 6)()
    po = ctypes.cast(out, ctypes.c_void_p)
    assert L.gfla_lds_plane_geometry(0, 1, 1, 4, 4, 4, 4, 3, 1, 4, 3, None) == -1
    assert L.gfla_lds_plane_geometry(8, 1, 1, 4, 4, 4, 4, 3, 1, 4, 3, po) == -2
    assert L.gfla_lds_plane_geometry(0, 1, 1, 4, 4, 4, 4, 3, 1, 3, 3, po) == -2
    assert L.gfla_lds_plane_geometry(0, 1, 1, 4, 4, 4, 4, 3, 1, 4, 0, po) == -2
    assert L.gfla_lds_plane_geometry(5, 1, 1, 4, 4, 4, 4, 1, 1, 4, 0, po) == -2
    assert L.gfla_lds_plane_geometry(0, 1, 64, 256, 176, 256, 176, 3, 1, 4, 3, po) == 0 and out[0] == 0    # the tile kernels' regime


def test_tuning_context_restores_keys_on_every_exit_path(gfla):
    keys = (gfla.TUNE_G_CAP, gfla.TUNE_SPLIT, gfla.TUNE_LDS_KB)
    before = [gfla.set_tuning(key, 0) for key in keys]
    assert before == [0, 0, 0]
    with pytest.raises(RuntimeError):
        with gfla.tuned(dict(zip(keys, (2, 3, 16)))):
            raise RuntimeError("a failing case")
    assert [gfla.set_tuning(key, 0) for key in keys] == [0, 0, 0]
