"""Affine regularisation loss on the kernels of csrc/affine_reg.hip (AffineRegFunction, AffineRegularizationLoss on GPU
tensors).  Reference everywhere: today's torch composition (u^T M u on flow + grid) evaluated on the host in float64 on the
same stored values -- the reference class's arithmetic, pinned by tests/golden/affine_golden.npz.

Bars: loss within 2e-6 relative in float32 and for 16-bit flows, 1e-12 in float64; d/d flow within
1e-5 of the largest reference entry in float32 (1e-12 in float64), plus half an ulp of the storage type per entry for
16-bit gradients.

The float64 composition is not exact either: it cancels the pixel coordinates (up to the map size, squared) numerically,
where the kernels never form them.  Its own error is measured without the code under test, at the zero flow, where the
exact loss and gradient are 0 (M annihilates the grid) and whatever the composition returns is its rounding: 1e-14 ..
1e-12 for the loss at these shapes.  The same cancellation on a non-zero flow adds cross terms of the order |flow| /
map size of that, so 4 x the zero-flow value is allowed on top of every bar (`_reference_error`).  It only matters in
float64 and on smooth fields, where the loss is 1e-4 .. 1e-2 and 1e-12 of it is below the reference's rounding."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_util as au  # noqa: E402
from util import FLOW_KINDS, make_flow  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_BAR = {torch.float32: 2e-6, torch.float64: 1e-12, torch.float16: 2e-6, torch.bfloat16: 2e-6}
GRAD_BAR = {torch.float32: 1e-5, torch.float64: 1e-12, torch.float16: 1e-5, torch.bfloat16: 1e-5}
HALF_ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SHAPES = [(3, 32, 22, 3), (2, 64, 44, 5), (2, 64, 64, 5), (2, 32, 32, 3), (1, 7, 9, 4), (2, 5, 5, 5), (1, 9, 31, 2),
          (1, 16, 12, 7), (1, 200, 300, 5)]
_ref_err = {}


def _reference_error(B, H, W, kz):
    """(loss, largest gradient entry) the float64 reference returns at the zero flow, where both are exactly 0."""
    key = (B, H, W, kz)
    if key not in _ref_err:
        loss, grad = au.reference(torch.zeros(B, 2, H, W, dtype=torch.float64), kz)
        _ref_err[key] = (abs(loss), grad.abs().max().item())
    return _ref_err[key]


def _field(kind, B, H, W, dtype, seed):
    if kind == "smooth0.5":
        return au.smooth_flow(B, H, W, 0.5, dtype, seed)
    if kind == "smooth4":
        return au.smooth_flow(B, H, W, 4.0, dtype, seed)
    return make_flow(kind, B, H, W, dtype, seed)


def _check(what, got_loss, got_grad, flow, kz, grad_scale=1.0):
    """Loss and gradient of the kernel path against the float64 host reference on flow's stored values, at flow's dtype's
    bars.  grad_scale: what the loss was multiplied by before backward."""
    dt = flow.dtype
    want, want_g = au.reference(flow, kz)
    e_loss, e_grad = _reference_error(*flow.shape[:1], *flow.shape[2:], kz)
    assert got_loss.dtype == (torch.float64 if dt == torch.float64 else torch.float32) and got_loss.dim() == 0
    err = abs(got_loss.item() - want)
    print("%s %s %s k%d: loss %.6e, err %.2e relative (reference's own %.1e)"
          % (what, str(dt)[6:], tuple(flow.shape), kz, want, err / max(abs(want), 1e-300), e_loss / max(abs(want), 1e-300)))
    assert err <= LOSS_BAR[dt] * abs(want) + 4 * e_loss, (what, got_loss.item(), want)
    if got_grad is None:
        return
    assert got_grad.dtype == dt and got_grad.shape == flow.shape
    want_g = want_g * grad_scale
    top = want_g.abs().max().item()
    diff = (got_grad.detach().cpu().double() - want_g).abs()
    tol = GRAD_BAR[dt] * top + 4 * e_grad * grad_scale + HALF_ULP.get(dt, 0.0) * want_g.abs()
    print("%s %s %s k%d: d/dflow err %.2e of the largest entry" % (what, str(dt)[6:], tuple(flow.shape), kz,
                                                                  diff.max().item() / max(top, 1e-300)))
    assert bool((diff <= tol).all()), (what, (diff - tol).max().item(), top)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", FLOW_KINDS + ("smooth0.5",))
@pytest.mark.parametrize("B,H,W,kz", SHAPES)
def test_parity_with_float64_composition(gfla, B, H, W, kz, kind, dtype):
    flow = _field(kind, B, H, W, dtype, seed=100 + kz)
    f = flow.to(DEV).requires_grad_()
    loss = gfla.AffineRegularizationLoss(kz)(f)
    loss.backward()
    _check(kind, loss, f.grad, flow, kz)


@pytest.mark.parametrize("kz", [3, 4])
def test_gradcheck_float64(gfla, kz):
    f = make_flow("coherent", 2, 9, 8, torch.float64, seed=kz).to(DEV).requires_grad_()
    assert torch.autograd.gradcheck(lambda x: gfla.AffineRegFunction.apply(x, kz), (f,), nondet_tol=0.0)


@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("amplitude", [0.5, 4.0])
@pytest.mark.parametrize("B,H,W,kz", [(2, 64, 64, 5), (2, 32, 32, 3)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16bit_flows(gfla, dtype, B, H, W, kz, amplitude, autocast):
    """The flow is read as stored and nothing is rounded to 16 bits on the way to the loss, called directly or under
    torch.autocast.  (The torch composition under autocast rounds flow + grid and M to 16 bits before the matmul: 0.5x to
    250x off on these inputs.)  Gradients as the GradScaler asks for them: backward of loss * 2^16."""
    flow = au.smooth_flow(B, H, W, amplitude, dtype, seed=7)
    f = flow.to(DEV).requires_grad_()
    with torch.autocast("cuda", dtype=dtype, enabled=autocast):
        loss = gfla.AffineRegularizationLoss(kz)(f)
    (loss * 2.0 ** 16).backward()
    _check("autocast" if autocast else "direct", loss, f.grad, flow, kz, grad_scale=2.0 ** 16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16])
def test_reproducible_and_call_forms(gfla, dtype):
    mod = gfla.AffineRegularizationLoss(5)
    flow = au.smooth_flow(2, 64, 44, 4.0, dtype, seed=3).to(DEV)
    runs = []
    for _ in range(2):
        f = flow.clone().requires_grad_()
        loss = mod(f)
        loss.backward()
        runs.append((loss.detach().clone(), f.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    with torch.no_grad():
        assert torch.equal(mod(flow), runs[0][0])
    plain = mod(flow)
    assert not plain.requires_grad and torch.equal(plain, runs[0][0])
    # a non-contiguous view: the channels of a wider tensor, every other column
    wide = torch.zeros(2, 3, 64, 88, dtype=dtype, device=DEV)
    wide[:, :2, :, ::2] = flow
    view = wide[:, :2, :, ::2]
    assert not view.is_contiguous()
    v = view.detach().requires_grad_()
    loss = mod(v)
    loss.backward()
    assert torch.equal(loss.detach(), runs[0][0]) and torch.equal(v.grad, runs[0][1])
    with pytest.raises(ValueError):
        mod(torch.zeros(1, 2, 4, 9, dtype=dtype, device=DEV))
    with pytest.raises(ValueError):
        mod(torch.zeros(1, 2, 9, 4, dtype=dtype, device=DEV))


def test_multi_layer_loss_and_torch_impl(gfla):
    flows = [au.smooth_flow(2, 32, 22, 0.5, seed=11), au.smooth_flow(2, 64, 44, 0.5, seed=12)]
    multi = gfla.MultiAffineRegularizationLoss({'2': 5, '3': 3})
    fs = [f.to(DEV).requires_grad_() for f in flows]
    loss = multi(fs)
    loss.backward()
    refs = [au.reference(flows[0], 3), au.reference(flows[1], 5)]
    want = refs[0][0] + refs[1][0]
    assert loss.dtype == torch.float32 and abs(loss.item() - want) <= 2e-6 * abs(want), (loss.item(), want)
    for f, (_, want_g) in zip(fs, refs):
        assert (f.grad.cpu().double() - want_g).abs().max().item() <= 1e-5 * want_g.abs().max().item()
    multi.impl = "torch"
    composed = multi([f.to(DEV) for f in flows])
    assert all(m.impl == "torch" for m in multi.method_dic.values())
    assert torch.isfinite(composed)
    print("multi: kernels %.9e, torch composition %.9e, float64 host %.9e" % (loss.item(), composed.item(), want))


def test_amp_trainer_step_reports_the_reference_value(gfla):
    """One TrainerShell(amp="bf16") step: the reported regularisation term is lambda x the float64 reference on the very
    bfloat16 flow fields the network produced."""
    import trainer_util as tu
    from global_flow_local_attention_amd.trainer import TrainerShell
    base, net = tu.build_shell(DEV, ngf=16, lr=1e-3)
    base.reducer.remove()
    shell = TrainerShell(net, lr=1e-3, correctness=base.correctness, regularization=base.regularization, attn_layer=(2, 3),
                         amp="bf16")
    seen = []
    hook = net.register_forward_hook(lambda mod, inp, out: seen.append([f.detach().clone() for f in out[1]]))
    try:
        losses = tu.run_step(shell, net, tu.make_batch(2, 64, 48), DEV)[0]
    finally:
        hook.remove()
    (flow3, flow2), = seen
    assert flow3.dtype == flow2.dtype == torch.bfloat16
    want = shell.lambdas["regularization"] * (au.reference(flow3, 3)[0] + au.reference(flow2, 5)[0])
    rel = abs(losses["regularization"] - want) / abs(want)
    print("amp bf16 step: regularization %.9e, reference %.9e, relative difference %.2e" % (losses["regularization"], want, rel))
    assert rel <= 1e-5, (losses["regularization"], want)
