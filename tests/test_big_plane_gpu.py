"""BASELINE configs[1] -- block_extractor + resample2d forward/backward on a (1, 64, 256, 176) fp32 feature map -- and the
kernel family that serves it (round 5: few planes, each far beyond the LDS budget; csrc/tile_map.h, be_tile.h, the
*_big / *_tile kernels of resample2d.hip).

  1. the configuration itself, DEFAULT dispatch, on every flow kind of tests/test_default_path_gpu.py (smooth, wild, integer,
     near-integer, out of bounds) against the REAL reference kernels (oracle/_ref), forward and every gradient, with the
     dispatch trace asserting that the big-plane kernels ran;
  2. the kernels forced on (tuning key 30 = 2) at small, ragged shapes (Hs != Hf, odd sizes, batch > 1, kernel sizes 2-5,
     resample kernel sizes 2-6 and dilation 2) in float32 and float64 against the CPU oracle, over launch geometries the
     heuristics do not pick: tile shapes, channels per workgroup / per thread, an LDS budget small enough that a tile's
     bounding box needs several channel rounds, and one small enough that tiles fall to global atomics;
  3. resample2d's int() quirk (resample2d_kernel.cu:137-138) both ways through the tile scatter.
"""
import pytest
import torch

import global_flow_local_attention_amd as T
from test_bench_shapes_gpu import _ref
from test_default_path_gpu import KINDS, flow_of, rel_err
from util import assert_close, make_flow, rand, randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5
CFG2 = (1, 64, 256, 176)


def _flow(kind, B, H, W, seed):
    return flow_of(kind, B, H, W, seed) if kind in KINDS else make_flow(kind, B, H, W, seed=seed)


def floor_mismatch(f, k):
    """(B,H,W) mask of the flow pixels where a float32 and a float64 evaluation of (flow + offset) + index
    (block_extractor_kernel.cu:62-67) floor DIFFERENTLY: the float32 sum rounds onto an integer the exact value lies just
    below.  The forward value is continuous there, d/dflow is one-sided -- a float32 kernel and the float64 reference take
    different sides, legitimately (measured on the smooth flow of this file: 2 of 45 056 pixels, a flow component within
    2^-22 of -2.0 and of -1.0; every kernel of this library, round 1's included, agrees with the others there)."""
    B, _, H, W = f.shape
    ys, xs = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    bad = torch.zeros(B, H, W, dtype=torch.bool)
    for t in range(k):
        o = float(t - k // 2)
        for ch, idx in ((0, xs), (1, ys)):
            c32 = (f[:, ch].float() + o) + idx.float()
            c64 = (f[:, ch].double() + o) + idx.double()
            bad |= torch.floor(c32).double() != torch.floor(c64)
    return bad


# ------------------------------------------------------------------------------------------ 1. the configuration itself
@pytest.mark.parametrize("kind", ("smooth", "zero") + KINDS)
@pytest.mark.parametrize("k", [3, 5])
def test_config2_block_extractor_all_flows_vs_reference_kernels(gfla, k, kind):
    ref = _ref()
    from global_flow_local_attention_amd import _lib
    B, C, H, W = CFG2
    s, f = randn((B, C, H, W), seed=1210), _flow(kind, B, H, W, 1211)
    sd, fd = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
    n_f, n_b = _lib.path_count(_lib.PATH_BE_FWD_GPIX), _lib.path_count(_lib.PATH_BE_BWD_TILE)
    out = gfla.BlockExtractor(k)(sd, fd)
    up = randn((B, C, k * H, k * W), seed=1212).to(DEV)
    out.backward(up)
    assert _lib.path_count(_lib.PATH_BE_FWD_GPIX) == n_f + 1, "forward did not take the big-plane kernel"
    assert _lib.path_count(_lib.PATH_BE_BWD_TILE) == n_b + 1, "backward did not take the tile kernel"
    dt = torch.float32 if kind == "near_integer" else torch.float64
    sr, fr = s.to(dt).to(DEV), f.to(dt).to(DEV)
    want = ref.block_extractor_fwd(sr, fr, k)
    gs, gf = ref.block_extractor_bwd(sr, fr, up.to(dt), k)
    got_gf = fd.grad.detach().clone()
    if dt == torch.float64:   # pixels whose coordinate floors differently in float32: one-sided derivative, other side
        bad = floor_mismatch(f, k)
        assert bad.sum().item() <= 0.002 * bad.numel(), "too many float32 / float64 floor mismatches to call them exceptions"
        keep = (~bad).unsqueeze(1).to(DEV)
        got_gf, gf = got_gf * keep, gf * keep
    errs = (("out", rel_err(out, want)), ("grad source", rel_err(sd.grad, gs)), ("grad flow", rel_err(got_gf, gf)))
    print("config2 block_extractor k%d %s: " % (k, kind) + " ".join("%s %.2e" % e for e in errs))
    assert (out.detach().double() - want.double()).abs().max().item() <= 1e-4        # the north star's own bar, absolute
    for n, e in errs:
        assert e <= (1e-4 if dt == torch.float32 and n != "out" else TOL), "k%d %s %s: rel err %.3e" % (k, kind, n, e)
    if kind == "zero":   # the reference's own KAT (test_block_extractor.py:46-55): centre tap = identity
        assert torch.equal(out[:, :, k // 2::k, k // 2::k], sd.detach())


@pytest.mark.parametrize("kind", ("smooth", "zero") + KINDS)
def test_config2_resample2d_all_flows_vs_reference_kernels(gfla, kind):
    ref = _ref()
    from global_flow_local_attention_amd import _lib
    B, C, H, W = CFG2
    i1, fl, up = randn((B, C, H, W), seed=1220), _flow(kind, B, H, W, 1221), randn((B, C, H, W), seed=1222)
    i1d, fld = i1.to(DEV).requires_grad_(), fl.to(DEV).requires_grad_()
    ids = (_lib.PATH_RS_FWD_BIG, _lib.PATH_RS_BWD1_TILE, _lib.PATH_RS_BWD2_BIG)
    before = [_lib.path_count(i) for i in ids]
    out = gfla.Resample2d(4, 1, 2)(i1d, fld)
    out.backward(up.to(DEV))
    assert [_lib.path_count(i) for i in ids] == [b + 1 for b in before], "default dispatch did not take the big-plane kernels"
    dt = torch.float32 if kind == "near_integer" else torch.float64
    i2 = torch.cat((fl, torch.full((B, 1, H, W), 2.0)), 1).to(dt).to(DEV).contiguous()
    i1r = i1.to(dt).to(DEV)
    want = ref.resample2d_fwd(i1r, i2, 4, 1)
    g1, g2 = ref.resample2d_bwd(i1r, i2, up.to(dt).to(DEV), 4, 1)
    errs = (("out", rel_err(out, want)), ("grad input1", rel_err(i1d.grad, g1)),
            ("grad flow", rel_err(fld.grad, g2[:, :2], 1.0 if kind == "oob" else 0.0)))
    print("config2 resample2d %s: " % kind + " ".join("%s %.2e" % e for e in errs))
    assert (out.detach().double() - want.double()).abs().max().item() <= 1e-4
    for n, e in errs:
        assert e <= (1e-4 if dt == torch.float32 and n != "out" else TOL), "resample2d %s %s: rel err %.3e" % (kind, n, e)


# ------------------------------------------------------------------------------------------ 2. forced, small shapes
# T.TUNE_BIG_PLANE = 2 forces the family; the geometries: tile sizes, channels per workgroup, 16 KB of LDS (several channel
# rounds, tiles on global memory), the first version of the gathers (the bodies every window kernel falls back to per tile),
# block_extractor's source scatter without the cross-lane fold (include/gfla_hip.h: enum gfla_tuning_key)
GEOS = [{},
        {T.TUNE_TILE_ROWS: 3, T.TUNE_TILE_COLS: 5, T.TUNE_SCATTER_TILE_CHANNELS: 1, T.TUNE_BIG_GATHER_CPW: 1,
         T.TUNE_BE_FWD_TILE_ROWS: 3, T.TUNE_BE_FWD_TILE_COLS: 5, T.TUNE_GATHER_TILE_CHANNELS: 1},
        {T.TUNE_TILE_ROWS: 16, T.TUNE_TILE_COLS: 32, T.TUNE_SCATTER_TILE_CHANNELS: 7, T.TUNE_BIG_GATHER_CPW: 3,
         T.TUNE_BE_FWD_TILE_ROWS: 2, T.TUNE_BE_FWD_TILE_COLS: 48, T.TUNE_GATHER_TILE_CHANNELS: 7, T.TUNE_BE_FWD_TILE_CHUNK: 1,
         T.TUNE_BE_BWD_TILE_NO_FOLD: 1},
        {T.TUNE_TILE_ROWS: 4, T.TUNE_TILE_COLS: 64, T.TUNE_SCATTER_TILE_CHANNELS: 3, T.TUNE_LDS_KB: 16, T.TUNE_BIG_GATHER_CPW: 2,
         T.TUNE_BE_FWD_TILE_ROWS: 16, T.TUNE_BE_FWD_TILE_COLS: 32, T.TUNE_GATHER_TILE_CHANNELS: 5},
        {T.TUNE_TILE_ROWS: 32, T.TUNE_TILE_COLS: 16, T.TUNE_SCATTER_TILE_CHANNELS: 5, T.TUNE_LDS_KB: 16, T.TUNE_BIG_GATHER_V1: 1,
         T.TUNE_BE_BWD_TILE_NO_FOLD: 1},
        {T.TUNE_TILE_ROWS: 1, T.TUNE_TILE_COLS: 512, T.TUNE_SCATTER_TILE_CHANNELS: 2, T.TUNE_BE_FWD_TILE_ROWS: 1,
         T.TUNE_BE_FWD_TILE_COLS: 512, T.TUNE_GATHER_TILE_CHANNELS: 2, T.TUNE_BE_FWD_TILE_CHUNK: 2},
        {T.TUNE_BIG_GATHER_V1: 1, T.TUNE_BIG_GATHER_CPW: 2}]
SHAPES = [  # B, C, Hs, Ws, Hf, Wf
    (2, 5, 21, 17, 21, 17), (1, 9, 40, 60, 40, 60), (2, 3, 12, 20, 9, 14), (1, 6, 7, 5, 11, 3), (1, 4, 64, 48, 64, 48)]


@pytest.mark.parametrize("geo", range(len(GEOS)))
@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_block_extractor_big_plane_kernels_forced(gfla, oracle, k, geo):
    from global_flow_local_attention_amd import _lib
    keys = dict(GEOS[geo])
    keys[T.TUNE_BIG_PLANE] = 2
    with gfla.tuned(keys):
        for (B, C, Hs, Ws, Hf, Wf) in SHAPES:
            for dtype, tf, tg in ((torch.float32, 2e-6, 2e-5), (torch.float64, 1e-12, 1e-11)):
                for kind, scale in (("wild", 0.6), ("wild", 3.0), ("smooth", 1.0)):
                    s = randn((B, C, Hs, Ws), dtype, seed=3)
                    f = (make_flow(kind, B, Hf, Wf, seed=4) * scale).to(dtype)
                    if kind == "smooth":   # a few lattice points and near-lattice points: the tap-by-tap branches
                        f[:, :, ::3, ::2] = torch.round(f[:, :, ::3, ::2])
                        f[:, :, 1::4, 1::3] = torch.round(f[:, :, 1::4, 1::3]) + (2.0 ** -22 if dtype == torch.float32 else 2.0 ** -50)
                    up = randn((B, C, k * Hf, k * Wf), dtype, seed=5)
                    want = oracle.block_extractor_fwd(s, f, k)
                    gs_w, gf_w = oracle.block_extractor_bwd(s, f, up, k)
                    sd, fd = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
                    n_f, n_b = _lib.path_count(_lib.PATH_BE_FWD_GPIX), _lib.path_count(_lib.PATH_BE_BWD_TILE)
                    out = gfla.BlockExtractorFunction.apply(sd, fd, k)
                    out.backward(up.to(DEV))
                    assert _lib.path_count(_lib.PATH_BE_FWD_GPIX) == n_f + 1 and _lib.path_count(_lib.PATH_BE_BWD_TILE) == n_b + 1
                    what = "k%d %s x%.1f %s %s keys %s" % (k, kind, scale, (B, C, Hs, Ws, Hf, Wf), dtype, keys)
                    assert_close(out.detach().cpu(), want, tf, "fwd " + what)
                    assert_close(sd.grad.cpu(), gs_w, tg, "grad source " + what)
                    assert_close(fd.grad.cpu(), gf_w, tg, "grad flow " + what)
            # one gradient at a time (the NEED_SRC / NEED_FLOW instantiations)
            s, f = randn((B, C, Hs, Ws), seed=6), make_flow("coherent", B, Hf, Wf, seed=7)
            up = randn((B, C, k * Hf, k * Wf), seed=8)
            gs_w, gf_w = oracle.block_extractor_bwd(s, f, up, k)
            sd, fd, upd = s.to(DEV), f.to(DEV), up.to(DEV)
            gs, gf = torch.zeros_like(sd), torch.zeros_like(fd)
            _lib.call("gfla_block_extractor_bwd_f32", sd, _lib.ptr(sd), _lib.ptr(fd), _lib.ptr(upd), _lib.ptr(gs), None, B, C, Hs, Ws, Hf, Wf, k)
            _lib.call("gfla_block_extractor_bwd_f32", sd, _lib.ptr(sd), _lib.ptr(fd), _lib.ptr(upd), None, _lib.ptr(gf), B, C, Hs, Ws, Hf, Wf, k)
            assert_close(gs.cpu(), gs_w, 2e-5, "grad source alone")
            assert_close(gf.cpu(), gf_w, 2e-5, "grad flow alone")


@pytest.mark.parametrize("geo", range(len(GEOS)))
@pytest.mark.parametrize("k,dil", [(4, 1), (2, 1), (6, 1), (4, 2), (5, 1)])
def test_resample2d_big_plane_kernels_forced(gfla, oracle, k, dil, geo):
    from global_flow_local_attention_amd import _lib
    keys = dict(GEOS[geo])
    keys[T.TUNE_BIG_PLANE] = 2
    ids = (_lib.PATH_RS_FWD_BIG, _lib.PATH_RS_BWD1_TILE, _lib.PATH_RS_BWD2_BIG)
    with gfla.tuned(keys):
        for (B, C, Hi, Wi, H, W) in SHAPES:
            for dtype, tf, tg in ((torch.float32, 4e-6, 3e-5), (torch.float64, 1e-12, 1e-10)):
                for kind, scale in (("wild", 0.6), ("wild", 3.0), ("smooth", 1.0)):
                    i1 = randn((B, C, Hi, Wi), dtype, seed=13)
                    i2 = torch.cat(((make_flow(kind, B, H, W, seed=14) * scale).to(dtype),
                                    rand((B, 1, H, W), dtype, seed=15) * 3 + 0.3), 1).contiguous()
                    up = randn((B, C, H, W), dtype, seed=16)
                    want = oracle.resample2d_fwd(i1, i2, k, dil)
                    g1_w, g2_w = oracle.resample2d_bwd(i1, i2, up, k, dil, trunc_compat=True)
                    i1d, i2d = i1.to(DEV).requires_grad_(), i2.to(DEV).requires_grad_()
                    before = [_lib.path_count(i) for i in ids]
                    out = gfla.Resample2dFunction.apply(i1d, i2d, k, dil)
                    out.backward(up.to(DEV))
                    assert [_lib.path_count(i) for i in ids] == [b + 1 for b in before]
                    what = "k%d d%d %s x%.1f %s %s keys %s" % (k, dil, kind, scale, (B, C, Hi, Wi, H, W), dtype, keys)
                    assert_close(out.detach().cpu(), want, tf, "fwd " + what)
                    assert_close(i1d.grad.cpu(), g1_w, tg, "grad input1 " + what)
                    assert_close(i2d.grad.cpu(), g2_w, tg, "grad (dx, dy, sigma) " + what)


@pytest.mark.parametrize("geo", (0, len(GEOS) - 1))
def test_resample2d_big_plane_forward_bf16_forced(gfla, oracle, geo):
    """bf16 storage through the big-plane forward kernel (rs_fwd_big_kernel<bf16>, the dispatch a bf16 map beyond the LDS budget
    takes; forced here by tuning key 30 = 2 -- advisor finding, round 5: no test reached it): bf16-rounded inputs through the
    float32 oracle, 2^-7 of the largest entry (the bf16 bar of tests/test_gpu_parity.py)."""
    from global_flow_local_attention_amd import _lib
    keys = dict(GEOS[geo])
    keys[T.TUNE_BIG_PLANE] = 2
    with gfla.tuned(keys):
        for (B, C, Hi, Wi, H, W) in SHAPES:
            for kind, scale in (("wild", 3.0), ("smooth", 1.0)):
                i1 = randn((B, C, Hi, Wi), seed=13).bfloat16()
                i2 = torch.cat((make_flow(kind, B, H, W, seed=14) * scale, rand((B, 1, H, W), seed=15) * 3 + 0.3), 1).bfloat16().contiguous()
                want = oracle.resample2d_fwd(i1.float(), i2.float(), 4, 1)
                before = _lib.path_count(_lib.PATH_RS_FWD_BIG)
                out = gfla.Resample2dFunction.apply(i1.to(DEV), i2.to(DEV), 4, 1)
                assert _lib.path_count(_lib.PATH_RS_FWD_BIG) == before + 1
                assert out.dtype == torch.bfloat16
                err = (out.float().cpu() - want).abs().max().item()
                assert err <= 2 ** -7 * max(1.0, want.abs().max().item()), "bf16 fwd %s x%.1f %s: %.3e" % (kind, scale, (B, C, Hi, Wi, H, W), err)


def test_bf16_storage_backward_beyond_the_lds_budget(gfla, oracle):
    """bf16 feature maps too large for the planes-in-LDS kernels (BASELINE configs[1]'s (1,64,256,176) in bf16 storage): the bf16
    backward entry points return GFLA_ERR_UNSUPPORTED there (their kernels keep whole planes in LDS); round 6: the operator
    surface then widens storage for the call and runs the float32 tile kernels, so a bf16 model trains on such maps.  Against the
    float32 oracle on the bf16-rounded inputs: 2^-7 of the largest entry (the bf16 bar of tests/test_gpu_parity.py)."""
    from global_flow_local_attention_amd import _lib
    B, C, H, W, k = 1, 8, 256, 176, 3
    s = randn((B, C, H, W), seed=31).bfloat16()
    f = make_flow("smooth", B, H, W, seed=32).bfloat16()
    up = randn((B, C, k * H, k * W), seed=33).bfloat16()
    sd, fd = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
    with pytest.raises(_lib.Unsupported):     # the C entry point itself still refuses (nothing launched)
        gs = torch.zeros_like(sd.detach())
        _lib.call("gfla_block_extractor_bwd_bf16", gs, _lib.ptr(sd.detach()), _lib.ptr(fd.detach()), _lib.ptr(up.to(DEV)), _lib.ptr(gs), None,
                  B, C, H, W, H, W, k)
    out = gfla.BlockExtractor(k)(sd, fd)
    out.backward(up.to(DEV))
    gs_w, gf_w = oracle.block_extractor_bwd(s.float(), f.float(), up.float(), k)
    assert sd.grad.dtype == torch.bfloat16 and fd.grad.dtype == torch.bfloat16
    for name, got, want in (("grad source", sd.grad, gs_w), ("grad flow", fd.grad, gf_w)):
        err = (got.float().cpu() - want).abs().max().item()
        assert err <= 2 ** -7 * max(1.0, want.abs().max().item()), "bf16 block_extractor %s: %.3e" % (name, err)
    # resample2d, same regime
    i1 = randn((B, C, H, W), seed=34).bfloat16()
    fl = make_flow("smooth", B, H, W, seed=35).bfloat16()
    upr = randn((B, C, H, W), seed=36).bfloat16()
    i1d, fld = i1.to(DEV).requires_grad_(), fl.to(DEV).requires_grad_()
    warped = gfla.Resample2d(4, 1, 2)(i1d, fld)
    warped.backward(upr.to(DEV))
    i2 = torch.cat((fl.float(), torch.full((B, 1, H, W), 2.0)), 1).contiguous()
    g1_w, g2_w = oracle.resample2d_bwd(i1.float(), i2, upr.float(), 4, 1, trunc_compat=True)
    for name, got, want in (("grad input1", i1d.grad, g1_w), ("grad flow", fld.grad, g2_w[:, :2])):
        err = (got.float().cpu() - want).abs().max().item()
        assert err <= 2 ** -7 * max(1.0, want.abs().max().item()), "bf16 resample2d %s: %.3e" % (name, err)


def test_resample2d_tile_scatter_trunc_compat_both_ways(gfla, oracle):
    """resample2d_kernel.cu:137-138 -- int() instead of floor() in d/d input1 -- matters where x + dx < 0: wild flows near the
    left / top border.  The tile scatter reproduces it by default and gives the forward's true gradient with it off."""
    from global_flow_local_attention_amd import resample2d as rs
    B, C, H, W = 2, 6, 24, 36
    with gfla.tuned({T.TUNE_BIG_PLANE: 2}):
        for dtype, tol in ((torch.float64, 1e-11), (torch.float32, 2e-5)):
            i1 = randn((B, C, H, W), dtype, seed=19)
            i2 = torch.cat((make_flow("wild", B, H, W, dtype, seed=20), rand((B, 1, H, W), dtype, seed=21) * 3 + 0.3), 1).contiguous()
            g = randn((B, C, H, W), dtype, seed=22)
            g1_t, _ = oracle.resample2d_bwd(i1, i2, g, 4, 1, trunc_compat=True)
            g1_f, _ = oracle.resample2d_bwd(i1, i2, g, 4, 1, trunc_compat=False)
            assert (g1_t - g1_f).abs().max().item() > 1e-3        # the quirk is visible on this input
            for compat, want in ((True, g1_t), (False, g1_f)):
                rs.TRUNC_COMPAT = compat
                try:
                    i1d = i1.to(DEV).requires_grad_()
                    gfla.Resample2dFunction.apply(i1d, i2.to(DEV), 4, 1).backward(g.to(DEV))
                    assert_close(i1d.grad.cpu(), want, tol, "trunc_compat=%s %s" % (compat, dtype))
                finally:
                    rs.TRUNC_COMPAT = True


def test_tile_scatter_is_reproducible_and_handles_nonfinite_gradients(gfla):
    """The float tile scatter accumulates 64-bit fixed point in LDS (order-independent); what leaves the window are float
    atomics, one per element and tile -- elements reached from several tiles may differ in the last bit run to run, which
    is the reference's own behaviour (float atomics everywhere).  A non-finite upstream gradient poisons what its tile
    reaches and nothing crashes."""
    B, C, H, W = CFG2
    i1, fl = randn((B, C, H, W), seed=31).to(DEV), make_flow("smooth", B, H, W, seed=32).to(DEV)
    up = randn((B, C, H, W), seed=33).to(DEV)
    mod = gfla.Resample2d(4, 1, 2)
    grads = []
    for _ in range(3):
        x = i1.clone().requires_grad_()
        mod(x, fl).backward(up)
        grads.append(x.grad)
    for g in grads[1:]:
        assert (g - grads[0]).abs().max().item() <= 1e-5 * grads[0].abs().max().item()
    up2 = up.clone()
    up2[0, 3, 100, 77] = float("inf")
    x = i1.clone().requires_grad_()
    mod(x, fl).backward(up2)
    torch.cuda.synchronize()
    assert not torch.isfinite(x.grad[0, 3]).all() and torch.isfinite(x.grad[0, 4]).all()


@pytest.mark.parametrize("k", [3, 5])
def test_config2_round1_row_window_kernels_still_agree(gfla, oracle, k):
    """tuning key 30 = 1: the configuration on round 1's row-window kernels (what serves planes beyond the LDS budget when
    there are MANY of them, B*C >= 1024) -- kept under test now that the default dispatch at this shape has moved on."""
    from global_flow_local_attention_amd import _lib
    with gfla.tuned({T.TUNE_BIG_PLANE: 1}):
        s, f = randn((1, 16, 256, 176), seed=34), make_flow("smooth", 1, 256, 176, seed=35)
        sd, fd = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
        n_f, n_b = _lib.path_count(_lib.PATH_BE_FWD_GPIX), _lib.path_count(_lib.PATH_BE_BWD_TILE)
        out = gfla.BlockExtractor(k)(sd, fd)
        assert_close(out.detach().cpu(), oracle.block_extractor_fwd(s, f, k), 2e-6, "windowed fwd")
        g = randn(tuple(out.shape), seed=36)
        out.backward(g.to(DEV))
        assert _lib.path_count(_lib.PATH_BE_FWD_GPIX) == n_f and _lib.path_count(_lib.PATH_BE_BWD_TILE) == n_b
        gs, gf = oracle.block_extractor_bwd(s, f, g, k)
        assert_close(sd.grad.cpu(), gs, 2e-5, "windowed grad_source")
        assert_close(fd.grad.cpu(), gf, 2e-5, "windowed grad_flow")
        if k == 3:
            i1d, fld = s.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
            o = gfla.Resample2d(4, 1, 2)(i1d, fld)
            i2 = torch.cat((f, torch.full((1, 1, 256, 176), 2.0)), 1).contiguous()
            assert_close(o.detach().cpu(), oracle.resample2d_fwd(s, i2, 4, 1), 4e-6, "windowed resample fwd")
            g = randn(tuple(o.shape), seed=39)
            o.backward(g.to(DEV))
            g1, g2 = oracle.resample2d_bwd(s, i2, g, 4, 1)
            assert_close(i1d.grad.cpu(), g1, 2e-5)
            assert_close(fld.grad.cpu(), g2[:, :2], 2e-5)
