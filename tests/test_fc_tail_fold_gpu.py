"""The sampling tails and the replicate-pad fold of the FC path (csrc/fc_sample.hip: fc_tail_fwd_kernel, fc_tail_bwd_kernel,
fc_dw1_kernel, fc_fold_kernel / fc_fold_rows_kernel) through gfla_fc_forward_f32 / gfla_fc_backward_f32, against the
float64 host composition of the reference formulation (test_fc_mfma_gpu._logits_f64) on the same inputs.

Bars: logits <= 2e-6 of the largest entry, every gradient <= 1e-5 of the largest entry.  FC biases are
+-8 so that no hidden activation sits near LeakyReLU's kink.

Shapes are the smallest at which these kernels change path:
  * the tails work on tiles of 64 positions, a wave on 16 consecutive ones: H W = 64, 65, 99, 63 (a last tile of 1, of 35, a
    wave with nothing to do);
  * the fold owns R rows x 32 channels per workgroup, R from W (whole 128-byte lines where they fit): one row group (8 x 8),
    a short last group (W 44: 8 + 3, W 22: 16 + 4, W 12: 8 + 3), planes that are no multiple of 16 bytes (5 x 13, 11 x 9, 9 x 7:
    the element-wise store), more than one channel group with a short last one (C 40), and C % 4 != 0 (the one-row kernel).
"""
import functools

import pytest
import torch

from test_fc_mfma_gpu import _collapse_flow, _logits_f64, _ptr, rel_err
from util import make_flow, randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL, GRAD_TOL = 2e-6, 1e-5
ACC_SOURCE, ACC_FLOW = 1, 2
NAMES = ("source", "target", "flow", "w0", "b0", "w1", "b1")

SHAPES = [(2, 16, 8, 8), (2, 16, 5, 13), (3, 8, 11, 9), (1, 16, 20, 22), (1, 16, 11, 44), (1, 16, 9, 7), (1, 40, 11, 12),
          (2, 6, 7, 10)]
FLOWS = ("zero", "integer", "near_integer_below", "near_integer_above", "smooth", "far_left", "far_right", "far_up", "far_down",
         "collapse")


@pytest.fixture(scope="module")
def lib(gfla, oracle):
    from global_flow_local_attention_amd import _lib
    return _lib


def _flow(kind, B, H, W):
    if kind == "collapse":
        return _collapse_flow(B, H, W)
    if kind.startswith("near_integer"):
        return make_flow("integer", B, H, W, seed=73) + (1e-4 if kind.endswith("above") else -1e-4)
    if kind.startswith("far_"):
        f = make_flow("coherent", B, H, W, seed=73)
        dx, dy = {"left": (-1, 0), "right": (1, 0), "up": (0, -1), "down": (0, 1)}[kind[4:]]
        f[:, 0] += dx * (W + 50.0)
        f[:, 1] += dy * (H + 50.0)
        return f.contiguous()
    return make_flow(kind, B, H, W, seed=73)


@functools.lru_cache(maxsize=None)
def _case(shape, k, kind):
    """Inputs (host, float32), the upstream gradient, and the float64 logits and gradients: computed once, never written to."""
    B, C, H, W = shape
    s, t = randn((B, C, H, W), seed=71), randn((B, C, H, W), seed=72)
    f = _flow(kind, B, H, W)
    w0 = randn((128, 2 * C, k, k), seed=74) / (2 * C * k * k) ** 0.5
    b0 = torch.where(randn((128,), seed=75) > 0, 8.0, -8.0)
    w1 = randn((k * k, 128, 1, 1), seed=76) / 128 ** 0.5
    b1 = randn((k * k,), seed=77) * 0.1
    up = randn((B, k * k, H, W), seed=78)
    a64 = [x.double().clone().requires_grad_() for x in (s, t, f, w0, b0, w1, b1)]
    want, hidden = _logits_f64(*a64, k, 0.1)
    assert hidden.abs().min().item() > 1e-2, "a hidden activation near the LeakyReLU kink"
    want.backward(up.double())
    return (s, t, f, w0, b0, w1, b1), up, want.detach(), tuple(a.grad for a in a64)


def _run(lib, mode, inputs, up, k, flags=0, outputs=NAMES, prior=None):
    """forward + backward through the C ABI; gradients not in `outputs` are passed as NULL; `prior`: initial content of an
    accumulated gradient (the others start as NaN: every element has to be written)."""
    from global_flow_local_attention_amd import fc_mfma
    s, t, f, w0, b0, w1, b1 = (x.to(DEV) for x in inputs)
    up = up.to(DEV)
    B, C, H, W = s.shape
    assert fc_mfma.resolve_mode(C, H, W, k, mode) == mode
    ws = torch.empty(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 0), dtype=torch.uint8, device=DEV)
    sc = torch.empty(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 1), dtype=torch.uint8, device=DEV)
    lg = torch.full((B, k * k, H, W), float("nan"), device=DEV)
    w1r = w1.reshape(k * k, 128).contiguous()
    lib.call("gfla_fc_forward_f32", s, _ptr(s), _ptr(t), _ptr(f), _ptr(w0), _ptr(b0), _ptr(w1r), _ptr(b1), _ptr(ws), _ptr(lg),
             B, C, H, W, k, 0.1, mode)
    g = {}
    for n_, x in zip(NAMES, (s, t, f, w0, b0, w1r, b1)):
        if n_ in outputs:
            g[n_] = prior[n_].to(DEV).clone() if prior and n_ in prior else torch.full_like(x, float("nan"))
    p = [_ptr(g.get(n_)) for n_ in NAMES]
    lib.call("gfla_fc_backward_f32", s, _ptr(ws), _ptr(f), _ptr(w1r), _ptr(up), _ptr(sc), *p, B, C, H, W, k, 0.1, mode, flags)
    torch.cuda.synchronize()
    return lg, g


def _check(lg, g, want, grads, what):
    errs = [("logits", rel_err(lg.cpu(), want), FWD_TOL)]
    for n_, r in zip(NAMES, grads):
        if n_ in g:
            errs.append((n_, rel_err(g[n_].cpu().reshape(r.shape), r), GRAD_TOL))
    print(what + ": " + " ".join("%s %.2e" % e[:2] for e in errs))
    for n_, e, tol in errs:
        assert e <= tol, "%s, %s: %.3e of the largest entry (bar %.0e)" % (what, n_, e, tol)


@pytest.mark.parametrize("mode", (5, 4))
@pytest.mark.parametrize("k", (3, 5))
@pytest.mark.parametrize("shape", SHAPES)
def test_tile_and_row_group_edges(lib, shape, k, mode):
    inputs, up, want, grads = _case(shape, k, "smooth")
    lg, g = _run(lib, mode, inputs, up, k)
    _check(lg, g, want, grads, "%s k %d mode %d" % (shape, k, mode))


@pytest.mark.parametrize("k", (3, 5))
@pytest.mark.parametrize("kind", FLOWS)
def test_flow_kinds(lib, kind, k):
    """Zero, integer and near-integer flows (weights 0 / 1 and 1e-4 away from them), flows that send every position far out
    of range on each side (all four corners clamp: ring-only folds, a flow gradient of exactly zero along the clamped axis),
    and one that collapses a sample onto one corner."""
    shape = (2, 16, 5, 13)
    inputs, up, want, grads = _case(shape, k, kind)
    lg, g = _run(lib, 5, inputs, up, k)
    _check(lg, g, want, grads, "%s k %d" % (kind, k))


@pytest.mark.parametrize("k", (3, 5))
@pytest.mark.parametrize("shape", [(2, 16, 5, 13), (1, 16, 11, 44), (1, 16, 20, 22)])
def test_accumulate_flags(lib, shape, k):
    """GFLA_FC_ACCUMULATE_SOURCE / _FLOW: prior content + the gradient, to the gradients' bar (the scale is that of the sum)."""
    inputs, up, want, grads = _case(shape, k, "smooth")
    ref = dict(zip(NAMES, grads))
    prior = {"source": randn(inputs[0].shape, seed=81) * 3, "flow": randn(inputs[2].shape, seed=82) * 3}
    _, plain = _run(lib, 5, inputs, up, k)
    for flags in (ACC_SOURCE, ACC_FLOW, ACC_SOURCE | ACC_FLOW):
        _, acc = _run(lib, 5, inputs, up, k, flags=flags, prior=prior)
        for n_, bit in (("source", ACC_SOURCE), ("flow", ACC_FLOW)):
            if flags & bit:
                e = rel_err(acc[n_].cpu(), prior[n_].double() + ref[n_])
                e2 = rel_err(acc[n_].cpu(), prior[n_].double() + plain[n_].cpu().double())
                print("flags %d %s: vs float64 %.2e, vs prior + plain %.2e" % (flags, n_, e, e2))
                assert e <= GRAD_TOL and e2 <= GRAD_TOL, (n_, flags, e, e2)
            else:   # (prior content of a gradient that is not accumulated is overwritten)
                assert torch.equal(acc[n_], plain[n_]), (n_, flags)
        for n_ in ("target", "w0", "b0", "w1", "b1"):
            assert torch.equal(acc[n_], plain[n_]), (n_, flags)


@pytest.mark.parametrize("k", (3, 5))
@pytest.mark.parametrize("outputs", [("source",), ("target",), ("source", "target", "flow", "w0", "b0"), ("flow",),
                                     ("w1", "b1"), ("source", "flow", "b1")])
def test_one_sided_calls(lib, outputs, k):
    """Any subset of the gradients: the others are NULL pointers, and the ones asked for are those of the full call."""
    shape = (2, 16, 5, 13)
    inputs, up, want, grads = _case(shape, k, "smooth")
    lg, g = _run(lib, 5, inputs, up, k, outputs=outputs)
    assert set(g) == set(outputs)
    _check(lg, g, want, grads, "outputs %s k %d" % (",".join(outputs), k))


@pytest.mark.parametrize("k", (3, 5))
@pytest.mark.parametrize("shape,kind", [((3, 8, 11, 9), "smooth"), ((1, 16, 11, 44), "collapse"), ((1, 40, 11, 12), "smooth")])
def test_run_to_run_equality(lib, shape, kind, k):
    """No float atomics anywhere: two calls on the same inputs give the same bits."""
    inputs, up, _, _ = _case(shape, k, kind)
    prior = {"source": randn(inputs[0].shape, seed=81), "flow": randn(inputs[2].shape, seed=82)}
    for flags in (0, ACC_SOURCE | ACC_FLOW):
        lg1, g1 = _run(lib, 5, inputs, up, k, flags=flags, prior=prior if flags else None)
        lg2, g2 = _run(lib, 5, inputs, up, k, flags=flags, prior=prior if flags else None)
        assert torch.equal(lg1, lg2)
        for n_ in NAMES:
            assert torch.isfinite(g1[n_]).all(), n_
            assert torch.equal(g1[n_], g2[n_]), "%s differs from run to run (flags %d)" % (n_, flags)
