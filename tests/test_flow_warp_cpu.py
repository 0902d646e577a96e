"""Bilinear flow warp (flow_warp, FlowWarp, BilinearSamplingBlock, PerceptualCorrectness.bilinear_warp) without a GPU: the
ABI surface and its argument checks, the three conventions on host tensors against tests/golden/flow_warp_golden.npz (the
reference's own warps in float64, tests/golden/make_flow_warp_golden.py), and the formula the kernels of
csrc/flow_warp.hip implement (tests/flow_warp_util.py: emulate) against the goldens and against autograd through the torch
composition.  Bar: 1e-12 of the largest reference entry, float64 throughout."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_warp_util as fu  # noqa: E402

ROOT = fu.ROOT
NEW_SYMBOLS = ["gfla_flow_warp_%s_%s" % (d, s) for d in ("fwd", "bwd") for s in ("f32", "f64", "f16", "bf16")]
BAR = 1e-12


def _close(got, want, what):
    err = (got.double() - want.double()).abs().max().item()
    assert err <= BAR * max(want.abs().max().item(), 1e-300), "%s: %.3e" % (what, err)


def _scalars(convention, src):
    from global_flow_local_attention_amd.flow_warp import convention_scalars
    return convention_scalars(convention, src.size(2), src.size(3))


def test_symbols_exported_and_declared(gfla):
    from global_flow_local_attention_amd import _lib
    names = gfla.exported_symbols()
    header = open(os.path.join(ROOT, "include", "gfla_hip.h")).read()
    handle = _lib.lib()
    for sym in NEW_SYMBOLS:
        assert sym in names, sym
        assert re.search(r"\b%s\(" % sym, header), sym
        assert hasattr(handle, sym), sym
    assert "#define GFLA_ABI_VERSION 8" in header
    assert handle.gfla_abi_version() == _lib.ABI_VERSION == 8
    for name in ("FlowWarpFunction", "flow_warp", "FlowWarp", "BilinearSamplingBlock"):
        assert hasattr(gfla, name), name


def test_argument_validation_without_gpu(gfla):
    """NULL -> -1, non-positive sizes -> -2, planes beyond 32-bit offsets -> -3: all decided on the host, nothing is
    launched"""
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    n = None
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    one = (1.0, 1.0, 1.0, 1.0)
    for sfx in ("f32", "f64", "f16", "bf16"):
        fwd, bwd = getattr(L, "gfla_flow_warp_fwd_" + sfx), getattr(L, "gfla_flow_warp_bwd_" + sfx)
        for args in ((n, p, p), (p, n, p), (p, p, n)):
            assert fwd(*args, 1, 1, 4, 4, 4, 4, *one, n) == -1
        for args in ((n, p, p), (p, n, p), (p, p, n)):                  # source, flow, grad_out are required ...
            assert bwd(*args, p, p, 1, 1, 4, 4, 4, 4, *one, n) == -1
        for at in range(6):
            sizes = [1, 1, 4, 4, 4, 4]
            sizes[at] = 0
            assert fwd(p, p, p, *sizes, *one, n) == -2
            sizes[at] = -3
            assert bwd(p, p, p, p, p, *sizes, *one, n) == -2            # ... (and sizes are checked before the outputs)
        assert fwd(p, p, p, 1, 1, 65536, 65536, 4, 4, *one, n) == -3
        assert bwd(p, p, p, p, p, 1, 1, 4, 4, 65536, 65536, *one, n) == -3


def test_golden_file_is_small_and_data_only():
    assert os.path.getsize(fu.GOLDEN_PATH) < 100 * 1024
    g = np.load(fu.GOLDEN_PATH)
    assert all(g[k].dtype.kind == "f" for k in g.files)
    cases = fu.golden_cases()
    assert {c for _, c in cases} == set(fu.CONVENTIONS)
    assert any(g[n + "/src"].shape[2:] != g[n + "/flow"].shape[2:] for n, c in cases if c == "pixel")   # Hs x Ws != H x W
    assert any(g[n + "/src"].shape[2] != g[n + "/src"].shape[3] for n, _ in cases)                      # h != w


@pytest.mark.parametrize("case,convention", fu.golden_cases())
def test_goldens_leave_the_map_on_every_side_and_avoid_kinks(case, convention):
    g = fu.golden(case, convention)
    hs, ws = g["src"].shape[2:]
    ix, iy = fu.positions(g["flow"], _scalars(convention, g["src"]))
    assert (ix < -1).any() and (ix > ws).any() and (iy < -1).any() and (iy > hs).any()
    assert ((ix > 0) & (ix < ws - 1) & (iy > 0) & (iy < hs - 1)).any()
    assert not fu.near_kink(g["flow"], _scalars(convention, g["src"])).any()


@pytest.mark.parametrize("impl", ["auto", "torch"])
@pytest.mark.parametrize("case,convention", fu.golden_cases())
def test_host_tensors_reproduce_the_reference(gfla, case, convention, impl):
    g = fu.golden(case, convention)

    def run(fn):
        s, f = g["src"].clone().requires_grad_(), g["flow"].clone().requires_grad_()
        out = fn(s, f)
        (out.reshape(g["up"].shape) * g["up"]).sum().backward()
        return out.detach().reshape(g["up"].shape), s.grad, f.grad

    routes = [("flow_warp", lambda s, f: gfla.flow_warp(s, f, convention, impl)),
              ("FlowWarp", gfla.FlowWarp(convention, impl))]
    if convention == "block" and impl == "auto":
        routes.append(("BilinearSamplingBlock", gfla.BilinearSamplingBlock()))
    if convention == "correctness":
        mod = gfla.PerceptualCorrectness()
        assert mod.warp_impl == "auto"
        mod.warp_impl = impl
        routes.append(("bilinear_warp", mod.bilinear_warp))
        assert mod.bilinear_warp(g["src"], g["flow"]).shape == g["src"].shape[:2] + (g["src"][0, 0].numel(),)
    for name, fn in routes:
        out, gs, gf = run(fn)
        assert out.dtype == torch.float64
        _close(out, g["out"], name + " forward")
        _close(gs, g["g_source"], name + " grad source")
        _close(gf, g["g_flow"], name + " grad flow")


@pytest.mark.parametrize("case,convention", fu.golden_cases())
def test_kernel_formula_matches_the_goldens(case, convention):
    g = fu.golden(case, convention)
    out, gs, gf = fu.emulate(g["src"], g["flow"], _scalars(convention, g["src"]), g["up"])
    _close(out, g["out"], "forward")
    _close(gs, g["g_source"], "grad source")
    _close(gf, g["g_flow"], "grad flow")


# a source axis of one element exists for "pixel" only: the other two conventions divide by w - 1 or h - 1
FORMULA_SHAPES = [(c, 2, 5, 7, 6, 7, 6) for c in fu.CONVENTIONS] + [(c, 1, 3, 4, 9, 6, 5) for c in fu.CONVENTIONS] + \
    [(c, 1, 70, 6, 6, 1, 11) for c in fu.CONVENTIONS] + [("pixel", 2, 2, 5, 1, 5, 1), ("pixel", 1, 4, 1, 8, 3, 8)]


@pytest.mark.parametrize("convention,B,C,Hs,Ws,H,W", FORMULA_SHAPES)
def test_kernel_formula_matches_autograd(gfla, convention, B, C, Hs, Ws, H, W):
    """the emulation against autograd through the composition on random shapes the goldens do not have (a source of one
    column or one row, a flow of one row, more channels than a wavefront), flows near and far"""
    gen = torch.Generator().manual_seed(B * 100 + C + Hs + W)
    src = torch.randn(B, C, Hs, Ws, generator=gen, dtype=torch.float64)
    up = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64)
    flow = torch.randn(B, 2, H, W, generator=gen, dtype=torch.float64) * 1.5
    flow = torch.where(torch.rand(B, 1, H, W, generator=gen) < 0.3, flow * 2 * max(Hs, Ws), flow)
    scalars = _scalars(convention, src)
    flow = fu.clear_of_kinks(flow, [scalars])
    assert not fu.near_kink(flow, scalars).any()
    want = fu.truth(src, flow, scalars, up)
    for got, ref, what in zip(fu.emulate(src, flow, scalars, up), want, ("forward", "grad source", "grad flow")):
        _close(got, ref, what)
    s, f = src.clone().requires_grad_(), flow.clone().requires_grad_()
    (gfla.flow_warp(s, f, convention) * up).sum().backward()
    _close(f.grad, want[2], "flow_warp grad flow")


def test_sixteen_bit_inputs_on_the_host(gfla):
    """16-bit sources give a float32 map, a 16-bit flow is up-cast and gets its gradient back in its own dtype"""
    for dtype in (torch.float16, torch.bfloat16):
        src = torch.randn(1, 3, 5, 5).to(dtype)
        flow = torch.randn(1, 2, 5, 5).to(dtype).requires_grad_()
        out = gfla.flow_warp(src, flow, "pixel")
        assert out.dtype == torch.float32
        out.sum().backward()
        assert flow.grad.dtype == dtype
        want = gfla.flow_warp(src.float(), flow.detach().float(), "pixel")
        assert torch.equal(out.detach(), want)


def test_argument_errors(gfla):
    src, flow = torch.zeros(1, 4, 3, 3), torch.zeros(1, 2, 3, 3)
    with pytest.raises(ValueError):
        gfla.flow_warp(src, flow, impl="hip")
    with pytest.raises(ValueError):
        gfla.flow_warp(src, flow, convention="normalised")
    with pytest.raises(ValueError):
        gfla.FlowWarp(impl="fast")
    with pytest.raises(ValueError):
        gfla.FlowWarp(convention="visi")
    mod = gfla.PerceptualCorrectness()
    mod.warp_impl = "fast"
    with pytest.raises(ValueError):
        mod.bilinear_warp(src, flow)
    with pytest.raises(NotImplementedError):
        gfla.FlowWarpFunction.apply(src, flow, 1.0, 1.0, 1.0, 1.0)       # host tensors: the kernels run on the GPU only
    assert gfla.FlowWarp().convention == "pixel" and gfla.FlowWarp().impl == "auto"
    assert len(list(gfla.BilinearSamplingBlock().parameters())) == 0


def test_install_leaves_the_reference_class_alone_by_default(gfla):
    assert inspect.signature(gfla.install).parameters["bilinear_sampling_block"].default is False
