"""The matrix-core scatter (csrc/patch_mfma.hip) with its tile prefetch in flight: same bits at every band height.

patch_scatter_mfma_kernel requests the next tile's gradient values and patch-table entries unconditionally, with clamped
addresses, and masks them where they are used (channel beyond C, pixel beyond H W, entry beyond E); the old values of the
accumulate path and the per-tile row ranges are requested the same way.  Every output element is summed over the tiles in
ascending order and over a tile's pixels in K order whatever the band height R, and a skipped all-zero slice adds exact
zeros, so for finite inputs the product's output is the same bits

  (a) at TUNE_PM_BAND_ROWS 1, 2, 3, 4 and the library's choice, between two runs, and with the gradient read through the
      scalar path (a G that starts one element into its storage: not 16-byte aligned);

and it agrees, at the bars of tests/test_default_path_gpu.py::test_aggregate_source_gradient_scatter_paths and
::test_resample2d_input1_gradient_scatter_paths (2e-5 of max(1, max |want|)),

  (b) with the CPU oracle (float64 autograd through the gather formulation / the literal resample2d restatement), and
  (c) with the LDS-atomic kernels (TUNE_PM 1).

The product is forced on (TUNE_PM 2, TUNE_PM_LIMIT_ROWS 100000) and seen to have run: it fills the patch table at the
head of the workspace.  Planes: 3x5 (one partial tile, H W % 4 != 0: scalar loads), 8x8 (two full tiles), 9x7 (tail tile),
12x22 (nine tiles, the last one a quarter full, 16-byte loads clamped at the end of the plane).  C = 5 is less than one
wave of channels, C = 130 a ragged second 128-channel slice.  Flows: zero; smooth; constant +H in y (every patch clamps
onto the last row: most bands have an empty tile list, one band takes every tile); far out of range.
"""
import pytest
import torch
import torch.nn.functional as F

from util import assert_close, make_flow, randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 2e-5          # test_default_path_gpu.py: grad_source / grad_input1 of the scatter-path tests
B = 2
CHANNELS = (5, 130)
PLANES = ((3, 5), (8, 8), (9, 7), (12, 22))
FLOWS = ("zero", "smooth", "last_row", "oob")
BAND_ROWS = (1, 2, 3, 4)
FILL = 0x7f


def flow_of(kind, H, W, seed):
    if kind == "last_row":
        f = torch.zeros(B, 2, H, W)
        f[:, 1] = float(H)
        return f
    if kind == "oob":
        f = make_flow("coherent", B, H, W, seed=seed)
        f[:, 0] += 1000.0
        f[:, 1] -= 1000.0
        f[1:, 0] -= 2000.0      # the second sample leaves through the other two sides
        f[1:, 1] += 2000.0
        return f.contiguous()
    return make_flow(kind, B, H, W, seed=seed)


def one_past_alignment(t):
    """t's values in a storage view that starts one element into its allocation: never 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0
    return view


def check_all(gfla, run, want, what):
    """run(go_misaligned=False) -> (gradient, workspace) under the tuning keys in force."""
    forced = {gfla.TUNE_PM: 2, gfla.TUNE_PM_LIMIT_ROWS: 100000}
    with gfla.tuned(forced):
        got, ws = run()
        assert not bool((ws[:8] == FILL).all()), "the matrix-core path did not run: " + what
        again, _ = run()
        assert torch.equal(got, again), "two runs differ: " + what
        for rows in BAND_ROWS:
            with gfla.tuned({gfla.TUNE_PM_BAND_ROWS: rows}):
                banded, _ = run()
            assert torch.equal(got, banded), "band height %d differs from the default: %s" % (rows, what)
        scalar, _ = run(True)
        assert torch.equal(got, scalar), "misaligned G differs: " + what
    with gfla.tuned({gfla.TUNE_PM: 1}):
        atomics, _ = run()
    assert torch.isfinite(got).all(), what
    assert_close(got.cpu(), want, BAR, "vs oracle " + what)
    assert_close(got.cpu(), atomics.cpu(), BAR, "vs LDS-atomic kernels " + what)


@pytest.mark.parametrize("plane", PLANES, ids=lambda p: "%dx%d" % p)
@pytest.mark.parametrize("k", (3, 5))
def test_aggregate_source_gradient_same_bits_at_every_band_height(gfla, oracle, k, plane):
    """d/d source of the aggregation through gfla_local_attn_aggregate_bwd_ws_f32, which accumulates: into a non-zero
    gradient here."""
    from global_flow_local_attention_amd import _lib
    H, W = plane
    for C in CHANNELS:
        s = randn((B, C, H, W), seed=41)
        lg = randn((B, k * k, H, W), seed=42) * 2
        go = randn((B, C, H, W), seed=43)
        base = randn((B, C, H, W), seed=44)
        for kind in FLOWS:
            f = flow_of(kind, H, W, 45)
            s64 = s.double().requires_grad_()
            a = torch.softmax(lg.double(), 1)
            ref = F.avg_pool2d(F.pixel_shuffle(a, k) * oracle.block_extractor_gather(s64, f.double(), k), k, k)
            ref.backward(go.double())
            want = (base.double() + s64.grad).float()
            sd, fd, ad, god, based = s.to(DEV), f.to(DEV), a.float().to(DEV).contiguous(), go.to(DEV), base.to(DEV)
            god1 = one_past_alignment(god)

            def run(misaligned=False):
                gs = based.clone()
                ws = _lib.scatter_workspace(sd, B, H, W, (k + 1) ** 2).fill_(FILL)
                _lib.call("gfla_local_attn_aggregate_bwd_ws_f32", sd, _lib.ptr(sd), _lib.ptr(fd), _lib.ptr(ad),
                          _lib.ptr(god1 if misaligned else god), _lib.ptr(gs), None, None, _lib.ptr(ws), B, C, H, W, H, W, k, 1)
                torch.cuda.synchronize()
                return gs, ws
            check_all(gfla, run, want, "aggregate k%d C%d %dx%d %s" % (k, C, H, W, kind))


@pytest.mark.parametrize("plane", PLANES, ids=lambda p: "%dx%d" % p)
@pytest.mark.parametrize("k", (4, 2))
def test_resample2d_input1_gradient_same_bits_at_every_band_height(gfla, oracle, k, plane):
    """d/d input1 of Resample2d(k, 1) through gfla_resample2d_bwd_ws_f32 (reference int() quirk on): accumulated into a
    non-zero gradient (trunc_compat 1) and written over a NaN-filled one (trunc_compat 3)."""
    from global_flow_local_attention_amd import _lib
    H, W = plane
    for C in CHANNELS:
        i1 = randn((B, C, H, W), seed=51)
        go = randn((B, C, H, W), seed=52)
        base = randn((B, C, H, W), seed=53)
        for kind in FLOWS:
            i2 = torch.cat((flow_of(kind, H, W, 54), torch.full((B, 1, H, W), 2.0)), 1).contiguous()
            grad, _ = oracle.resample2d_bwd(i1.double(), i2.double(), go.double(), k, 1, True)
            i1d, i2d, god, based = i1.to(DEV), i2.to(DEV), go.to(DEV), base.to(DEV)
            god1 = one_past_alignment(god)
            for overwrite in (False, True):
                want = grad.float() if overwrite else (base.double() + grad).float()

                def run(misaligned=False):
                    g1 = torch.full_like(i1d, float("nan")) if overwrite else based.clone()
                    ws = _lib.scatter_workspace(i1d, B, H, W, k * k).fill_(FILL)
                    _lib.call("gfla_resample2d_bwd_ws_f32", i1d, _lib.ptr(i1d), _lib.ptr(i2d),
                              _lib.ptr(god1 if misaligned else god), _lib.ptr(g1), None, _lib.ptr(ws), B, C, H, W, H, W, k, 1,
                              3 if overwrite else 1)
                    torch.cuda.synchronize()
                    return g1, ws
                check_all(gfla, run, want, "resample2d k%d C%d %dx%d %s %s" % (
                    k, C, H, W, kind, "overwrite" if overwrite else "accumulate"))
