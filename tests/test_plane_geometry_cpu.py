"""What tests/test_plane_geometry_gpu.py stands on, checked without a GPU:

  1. the float64 evaluations of tests/plane_util.py against the CPU oracle (1e-12);
  2. the share of d/d flow entries left out as kinks, on the exact inputs of the GPU cases: at most 10 %, the planted lattice
     points of the `smooth` flow counted separately; and no resample2d coordinate of any case floors differently in the
     kernels' arithmetic (its forward jumps there, and nothing is ever left out of a forward result);
  3. the power of the bar: the float64 reference rounded once to the storage type passes, and three planted bugs fail it;
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
    with pu.Tuning(gfla, {4: 3}):
        for op in range(8):
            for elem in (2, 4, 8):
                g = q(op, pu.SHAPES[0], 4 if op >= 5 else 3, elem=elem)
                assert (g["G"], g["ngroups"]) == (3, 3), (op, elem, g)           # C = 7: groups of 3, 3, 1
    with pu.Tuning(gfla, {5: 3}):
        for op in range(8):
            for elem in (2, 4, 8):
                g = q(op, pu.SHAPES[0], 4 if op >= 5 else 3, elem=elem)
                want = 1 if (elem == 2 and op in OPS_BWD16_NO_SPLIT) else 3
                assert g["split"] == want and g["per"] == -(-140 // want), (op, elem, g)
    # the two callers the issue names, once more by name: 16-bit block_extractor backward and resample2d d/d input1
    with pu.Tuning(gfla, {5: 3}):
        assert q(0, pu.SHAPES[3], 3, elem=2)["split"] == 1 and q(0, pu.SHAPES[3], 3, elem=4)["split"] == 3
        assert q(6, pu.SHAPES[3], 4, elem=2)["split"] == 1 and q(6, pu.SHAPES[3], 4, elem=4)["split"] == 3
        assert q(0, pu.SHAPES[3], 3, elem=4)["per"] == 703            # 2109 = 3 x 703 = 19 rows of 37: ends inside a flow row
    # key 10 = 16: 48 x 32 x 12 B > 16 KB.  With only 8 such planes the tile kernels of csrc/tile_map.h take the call first
    # (B C < 4 workgroups per CU: gfla_big_plane_geometry's regime), so the family reports G = 0; key 30 = 1 switches those
    # off and the same planes run as ROW WINDOWS
    with pu.Tuning(gfla, {10: 16}):
        assert q(0, pu.SHAPES[2], 3, elem=4)["G"] == 0
    with pu.Tuning(gfla, pu.WINDOWS):
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
    before = [gfla.set_tuning(key, 0) for key in (4, 5, 10)]
    assert before == [0, 0, 0]
    with pytest.raises(RuntimeError):
        with pu.Tuning(gfla, {4: 2, 5: 3, 10: 16}):
            raise RuntimeError("a failing case")
    assert [gfla.set_tuning(key, 0) for key in (4, 5, 10)] == [0, 0, 0]
