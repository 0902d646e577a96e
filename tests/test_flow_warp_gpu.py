"""Bilinear flow warp on the GPU (csrc/flow_warp.hip): goldens, a sweep over convention x dtype x shape, bit identity of
d/d flow, 16-bit sources under autocast, and the sampling-correctness loss with `use_bilinear_sampling=True`.

The truth of every comparison is the float64 HOST evaluation of the torch composition on the same, already rounded,
inputs (flow_warp_util.truth).  Bars are not fixed numbers: for each case the torch composition is evaluated on the GPU
in the same run (for 16-bit sources under torch.autocast, which is how it is used), its error against the truth is the
bar, and the kernel may not exceed it -- with a floor of 4 units in the last place of the output's type, taken at
max |source| for the forward, at max |d/d flow| for d/d flow and at max |d/d source| for d/d source, because the kernel
and grid_sample order the four products differently and neither is the truth.  float64: 1e-12 relative.

d/d flow is piecewise constant in the sampling position and jumps where a coordinate is an integer; every flow here is
nudged on the host until no coordinate is within 1e-3 px of one (flow_warp_util.clear_of_kinks), the case asserts that
none is left, and no element is excluded from any comparison."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_warp_util as fu  # noqa: E402
from util import make_flow, randn  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALF = (torch.float16, torch.bfloat16)
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]


def _scalars(convention, hs, ws):
    from global_flow_local_attention_amd.flow_warp import convention_scalars
    return convention_scalars(convention, hs, ws)


def _ulp(dtype, at):
    """spacing of `dtype` at magnitude `at`"""
    if at == 0:
        return 0.0
    return math.ldexp(torch.finfo(dtype).eps, math.frexp(at)[1] - 1)


def _composition(src, flow, scalars, up):
    """the torch composition on the GPU, for 16-bit sources as autocast evaluates it: (out, g_source, g_flow)"""
    from global_flow_local_attention_amd.flow_warp import torch_flow_warp
    s, f = src.detach().clone().requires_grad_(), flow.detach().clone().requires_grad_()
    with torch.autocast("cuda", dtype=src.dtype, enabled=src.dtype in HALF):
        out = torch_flow_warp(s, f, *scalars)
    (out * up).sum().backward()
    return out.detach(), s.grad, f.grad


def _kernel(gfla, src, flow, scalars, up):
    s, f = src.detach().clone().requires_grad_(), flow.detach().clone().requires_grad_()
    out = gfla.FlowWarpFunction.apply(s, f, *scalars)
    (out * up).sum().backward()
    return out.detach(), s.grad, f.grad


def check(gfla, src, flow, scalars, up, label):
    """src / flow / up on the host in their storage types.  Prints every figure, then asserts."""
    assert not fu.near_kink(flow, scalars).any(), "a sampling position is within %.0e px of a kink" % fu.CLEAR
    want = fu.truth(src, flow, scalars, up)
    dev = [t.to(DEV) for t in (src, flow, up)]
    got = _kernel(gfla, dev[0], dev[1], scalars, dev[2])
    comp = _composition(dev[0], dev[1], scalars, dev[2])
    out_dtype = flow.dtype
    assert got[0].dtype == out_dtype and got[1].dtype == src.dtype and got[2].dtype == flow.dtype
    scales = (src.double().abs().max().item(), want[1].abs().max().item(), want[2].abs().max().item())
    types = (out_dtype, src.dtype, flow.dtype)
    failures = []
    for what, g, c, w, scale, t in zip(("forward", "d/d source", "d/d flow"), got, comp, want, scales, types):
        err_k = (g.double().cpu() - w).abs().max().item()
        err_c = (c.double().cpu() - w).abs().max().item()
        if src.dtype == torch.float64:
            bar, floor = 1e-12 * scale, 1e-12 * scale
        else:
            floor = 4 * _ulp(t, scale)
            bar = max(err_c, floor)
        print("%s %s: kernel %.3e, composition %.3e, floor %.3e (scale %.3e), excluded 0" % (label, what, err_k, err_c, floor, scale))
        assert torch.isfinite(g).all()
        if not err_k <= bar:
            failures.append((what, err_k, bar))
    assert not failures, failures


@pytest.mark.parametrize("case,convention", fu.golden_cases())
def test_goldens_float64(gfla, case, convention):
    """forward and both gradients against the reference's own outputs, 1e-12 of the largest entry"""
    g = fu.golden(case, convention, device=DEV)
    s, f = g["src"].clone().requires_grad_(), g["flow"].clone().requires_grad_()
    out = gfla.flow_warp(s, f, convention)
    assert isinstance(out.grad_fn, gfla.FlowWarpFunction._backward_cls)
    (out * g["up"]).sum().backward()
    for what, got, want in (("forward", out.detach(), g["out"]), ("d/d source", s.grad, g["g_source"]),
                            ("d/d flow", f.grad, g["g_flow"])):
        err = (got - want).abs().max().item()
        print("golden %s %s float64 %s: %.3e of %.3e" % (case, convention, what, err, want.abs().max().item()))
        assert err <= 1e-12 * want.abs().max().item(), (what, err)


@pytest.mark.parametrize("case,convention", fu.golden_cases())
def test_goldens_float32(gfla, case, convention):
    """the goldens' inputs rounded to float32.  Rounding a flow of 25 px moves the sample by 1e-6 px, which is in the
    golden's outputs but is not the kernel's error, so the truth is the float64 host composition on the ROUNDED inputs --
    the function tests/test_flow_warp_cpu.py pins to the goldens at 1e-12 -- and the bar is the sweep's."""
    g = fu.golden(case, convention, torch.float32)
    scalars = _scalars(convention, *g["src"].shape[2:])
    flow = fu.clear_of_kinks(g["flow"], [scalars])
    check(gfla, g["src"], flow, scalars, g["up"], "golden %s %s float32" % (case, convention))


# B, C, Hs, Ws, H, W, flow kind
SWEEP = [
    (2, 16, 12, 10, 12, 10, "coherent"),
    (1, 70, 9, 17, 9, 17, "wild"),          # C not a multiple of the wave width (64) nor of the channel group (32)
    (2, 33, 16, 8, 16, 8, "far"),           # flows of +-2 W: every sample outside, zero padding only
    (3, 5, 6, 7, 1, 13, "wild"),            # a flow of one row, other size than the source
    (2, 3, 7, 5, 9, 1, "coherent"),         # a flow of one column
    (1, 130, 32, 32, 32, 32, "smooth"),     # a correctness-loss layer shape, C over two wave passes
]


def _inputs(B, C, Hs, Ws, H, W, kind, dtype, scalars, seed):
    flow_dtype = torch.float64 if dtype == torch.float64 else torch.float32
    src = randn((B, C, Hs, Ws), seed=seed).to(dtype)
    up = randn((B, C, H, W), seed=seed + 1).to(flow_dtype)
    if kind == "far":
        sign = torch.where(randn((B, 2, H, W), seed=seed + 2) > 0, 1.0, -1.0)
        flow = (sign * 2 * W + randn((B, 2, H, W), seed=seed + 3) * 0.3).to(flow_dtype)
    else:
        flow = make_flow(kind, B, H, W, seed=seed + 2).to(flow_dtype)
    return src, fu.clear_of_kinks(flow, [scalars]), up


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("convention", fu.CONVENTIONS)
@pytest.mark.parametrize("B,C,Hs,Ws,H,W,kind", SWEEP)
def test_sweep(gfla, B, C, Hs, Ws, H, W, kind, convention, dtype):
    scalars = _scalars(convention, Hs, Ws)
    src, flow, up = _inputs(B, C, Hs, Ws, H, W, kind, dtype, scalars, seed=B * 1000 + C)
    if kind == "far":
        ix, iy = fu.positions(flow, scalars)
        assert ((ix < -1) | (ix > Ws)).all()
    check(gfla, src, flow, scalars, up, "%s %s %s" % ((B, C, Hs, Ws, H, W, kind), convention, str(dtype)[6:]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_flow_gradient_is_bit_identical_and_partial_requests(gfla, dtype):
    scalars = _scalars("correctness", 20, 24)
    src, flow, up = _inputs(2, 48, 20, 24, 20, 24, "wild", dtype, scalars, seed=7)
    dev = [t.to(DEV) for t in (src, flow, up)]
    first = _kernel(gfla, *dev[:2], scalars, dev[2])
    again = _kernel(gfla, *dev[:2], scalars, dev[2])
    assert torch.equal(first[2], again[2]) and torch.equal(first[0], again[0])
    # the flow's gradient alone (what the loss asks for): the same bits, and the source gets none
    s, f = dev[0].clone(), dev[1].clone().requires_grad_()
    (gfla.FlowWarpFunction.apply(s, f, *scalars) * dev[2]).sum().backward()
    assert torch.equal(f.grad, first[2])
    s, f = dev[0].clone().requires_grad_(), dev[1].clone()
    (gfla.FlowWarpFunction.apply(s, f, *scalars) * dev[2]).sum().backward()
    assert s.grad is not None and s.grad.dtype == dtype


@pytest.mark.parametrize("dtype", HALF)
def test_sixteen_bit_source_is_read_as_stored(gfla, dtype):
    """float32 map from a 16-bit source; under autocast the op saves the 16-bit tensor and allocates no float32 copy of the
    source, which the composition does"""
    B, C, H, W = 4, 64, 32, 32
    scalars = _scalars("correctness", H, W)
    src, flow, _ = _inputs(B, C, H, W, H, W, "coherent", dtype, scalars, seed=11)
    src, flow = src.to(DEV), flow.to(DEV).requires_grad_()
    peaks = {}
    with torch.autocast("cuda", dtype=dtype):
        for impl in ("auto", "torch"):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            out = gfla.flow_warp(src, flow, "correctness", impl)
            torch.cuda.synchronize()
            peaks[impl] = torch.cuda.max_memory_allocated() - before
            assert out.dtype == torch.float32
            if impl == "auto":
                saved = out.grad_fn.saved_tensors
                assert saved[0].dtype == dtype and saved[0].data_ptr() == src.data_ptr()
            del out
    out_bytes, copy_bytes = B * C * H * W * 4, src.numel() * 4
    print("peak bytes above the inputs: kernel %d, composition %d (output %d, float32 source %d)"
          % (peaks["auto"], peaks["torch"], out_bytes, copy_bytes))
    assert peaks["auto"] < out_bytes + copy_bytes // 2 and peaks["auto"] < peaks["torch"]
    # a 16-bit flow is up-cast, its gradient comes back in its own dtype
    f16 = flow.detach().to(dtype).requires_grad_()
    out = gfla.flow_warp(src, f16, "correctness")
    out.sum().backward()
    assert out.dtype == torch.float32 and f16.grad.dtype == dtype


def test_modules_route_gpu_tensors_through_the_kernels(gfla):
    scalars = _scalars("block", 12, 9)
    src, flow, _ = _inputs(2, 6, 12, 9, 12, 9, "coherent", torch.float32, scalars, seed=21)
    src, flow = src.to(DEV), flow.to(DEV)
    want = gfla.FlowWarpFunction.apply(src, flow, *scalars)
    assert torch.equal(gfla.BilinearSamplingBlock()(src, flow), want)
    assert torch.equal(gfla.FlowWarp("block")(src, flow), want)
    assert want.abs().max().item() > 0.1
    assert (gfla.FlowWarp("block", "torch")(src, flow) - want).abs().max().item() <= 1e-4
    with pytest.raises(TypeError):
        gfla.FlowWarpFunction.apply(src, flow.double(), *scalars)
    with pytest.raises(ValueError):
        gfla.FlowWarpFunction.apply(src, flow[:, :1], *scalars)


def _layers(dtype):
    from test_correctness_half_gpu import features
    out = {}
    for name, shape, seed in (("relu3_1", (2, 40, 12, 10), 31), ("relu4_1", (2, 72, 6, 5), 41)):
        out[name] = (features(shape, seed, dtype), features(shape, seed + 2, dtype))
    return out


class _Warp(torch.nn.Module):
    """the composition in the place of the CPU oracle's Resample2d"""

    def __init__(self, scalars):
        super().__init__()
        self.scalars = scalars

    def forward(self, source, flow):
        from global_flow_local_attention_amd.flow_warp import torch_flow_warp
        return torch_flow_warp(source, flow, *self.scalars)


def _clear_flow(h, w, seed):
    scalars = _scalars("correctness", h, w)
    flow = fu.clear_of_kinks(make_flow("coherent", 2, h, w, seed=seed), [scalars])
    assert not fu.near_kink(flow, scalars).any()
    return flow


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype", HALF)
def test_loss_native_bilinear_equals_the_float32_route(gfla, dtype, masked):
    """PerceptualCorrectness(half_features="native")(use_bilinear_sampling=True) on 16-bit features against the "float32"
    route (features up-cast, float32 kernels), at the bar tests/test_correctness_half_gpu.py holds the Resample2d route to:
    loss within 2e-6, flow gradient within 1e-5 under assert_close"""
    from util import assert_close
    feats = _layers(dtype)
    native, plain = gfla.PerceptualCorrectness(half_features="native"), gfla.PerceptualCorrectness()
    for mod in (native, plain):
        mod.source_vgg = {k: v[0].to(DEV) for k, v in feats.items()}
        mod.target_vgg = {k: v[1].to(DEV) for k, v in feats.items()}
    mask = (randn((2, 1, 24, 20), seed=51) > -0.3).float().to(DEV) if masked else None
    for layer, (h, w), seed in (("relu3_1", (12, 10), 61), ("relu4_1", (6, 5), 62)):
        flow = _clear_flow(h, w, seed)
        f1, f2 = flow.to(DEV).requires_grad_(), flow.to(DEV).requires_grad_()
        a = native.calculate_loss(f1, layer, mask, use_bilinear_sampling=True)
        b = plain.calculate_loss(f2, layer, mask, use_bilinear_sampling=True)
        a.backward()
        b.backward()
        err = abs(a.item() - b.item())
        print("native bilinear %s %s masked=%s: loss %.9g / %.9g, |err| %.3e" % (layer, dtype, masked, a.item(), b.item(), err))
        assert a.dtype == torch.float32 and f1.grad.dtype == torch.float32
        assert err <= 2e-6
        assert_close(f1.grad, f2.grad, 1e-5, "grad flow")


def test_loss_bilinear_float32_and_the_torch_route(gfla):
    """float32 features, use_bilinear_sampling=True: warp_impl="torch" gives exactly the values of the normalised grid and
    grid_sample written out here as the loss has had them; the kernel route matches the host evaluation (the CPU oracle's
    loss with the composition as its warp) within the 2e-6 of tests/test_correctness_gpu.py."""
    import torch.nn.functional as F
    from oracle.cpu_modules import PerceptualCorrectnessCPU
    from util import assert_close
    feats = _layers(torch.float32)

    def written_out(source, flow):
        b, c, h, w = source.shape
        xs = torch.arange(w, device=source.device).view(1, -1).expand(h, -1).type_as(source) / (w - 1)
        ys = torch.arange(h, device=source.device).view(-1, 1).expand(-1, w).type_as(source) / (h - 1)
        grid = 2 * torch.stack([xs, ys], dim=0).unsqueeze(0).expand(b, -1, -1, -1) - 1
        scale = torch.tensor([w, h], device=flow.device).view(1, 2, 1, 1).type_as(flow)
        grid = (grid + 2 * flow / scale).permute(0, 2, 3, 1)
        return F.grid_sample(source, grid, align_corners=True).view(b, c, -1)

    mod = gfla.PerceptualCorrectness()
    mod.source_vgg = {k: v[0].to(DEV) for k, v in feats.items()}
    mod.target_vgg = {k: v[1].to(DEV) for k, v in feats.items()}
    ref = PerceptualCorrectnessCPU()
    ref.source_vgg = {k: v[0].double() for k, v in feats.items()}
    ref.target_vgg = {k: v[1].double() for k, v in feats.items()}
    for layer, (h, w), seed in (("relu3_1", (12, 10), 61), ("relu4_1", (6, 5), 62)):
        flow = _clear_flow(h, w, seed)
        scalars = _scalars("correctness", h, w)
        src = mod.source_vgg[layer]
        mod.warp_impl = "torch"
        assert torch.equal(mod.bilinear_warp(src, flow.to(DEV)), written_out(src, flow.to(DEV)))
        f_t = flow.to(DEV).requires_grad_()
        loss_t = mod.calculate_loss(f_t, layer, None, use_bilinear_sampling=True)
        mod.warp_impl = "auto"
        f_k = flow.to(DEV).requires_grad_()
        loss_k = mod.calculate_loss(f_k, layer, None, use_bilinear_sampling=True)
        ref.resample = _Warp(scalars)
        f_r = flow.double().requires_grad_()
        want = ref.calculate_loss(f_r, layer)
        loss_k.backward()
        want.backward()
        print("bilinear loss %s: kernel %.9g, torch %.9g, host %.9g" % (layer, loss_k.item(), loss_t.item(), want.item()))
        assert abs(loss_k.item() - want.item()) <= 2e-6 and abs(loss_t.item() - want.item()) <= 2e-6
        assert_close(f_k.grad.cpu(), f_r.grad, 1e-5, "grad flow")
