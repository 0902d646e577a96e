"""Affine regularisation loss, the parts that need no GPU: the identities the kernels of csrc/affine_reg.hip rest on
(M = I - P, M A = 0), the residual form in float32 torch ops against the float64 composition, the host-side argument checks
of the gfla_affine_reg_* entry points, and that CPU tensors still take the torch composition."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_util as au  # noqa: E402

# float32 results within 2e-6 (values) / 1e-5 of the largest entry (gradients) of float64
F32_LOSS, F32_GRAD = 2e-6, 1e-5
SHAPES = [(64, 64, 5), (32, 32, 3), (64, 44, 5), (32, 22, 3), (12, 10, 4), (9, 31, 2), (14, 15, 6), (16, 12, 7)]
FIELDS = {"smooth4": lambda B, H, W, dt: au.smooth_flow(B, H, W, 4.0, dt, seed=1),
          "smooth0.5": lambda B, H, W, dt: au.smooth_flow(B, H, W, 0.5, dt, seed=2),
          "noise2": lambda B, H, W, dt: au.noise_flow(B, H, W, 2.0, dt, seed=3),
          "noise30": lambda B, H, W, dt: au.noise_flow(B, H, W, 30.0, dt, seed=4)}


@pytest.mark.parametrize("kz", [2, 3, 4, 5, 6, 7])
def test_projector_identities(kz):
    """The reference's K is P - I, so M = K^T K = I - P, and M annihilates [row, col, 1] -- hence the sampling grid."""
    from global_flow_local_attention_amd.losses import affine_projector
    M = affine_projector(kz).numpy()
    rows, cols = np.arange(kz).repeat(kz).astype(np.float64), np.tile(np.arange(kz), kz).astype(np.float64)
    A = np.stack([rows, cols, np.ones(kz * kz)], 1)
    P = A @ np.linalg.inv(A.T @ A) @ A.T
    assert np.abs(M - (np.eye(kz * kz) - P)).max() <= 1e-12
    assert np.abs(M @ A).max() <= 1e-12
    # P f is the plane the kernels fit: a = mean, slopes = sum(d f) / s, s = k^2 (k^2 - 1) / 12
    f = np.random.RandomState(kz).randn(kz * kz)
    c, s = (kz - 1) / 2.0, kz ** 2 * (kz ** 2 - 1) / 12.0
    plane = f.mean() + (rows - c) * ((rows - c) @ f / s) + (cols - c) * ((cols - c) @ f / s)
    assert np.abs(P @ f - plane).max() <= 1e-12


@pytest.mark.parametrize("H,W,kz", SHAPES)
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_residual_form_in_float32_matches_float64_composition(H, W, kz, field):
    """The residual form the kernels evaluate, here in float32 torch ops (the kernels fit in float64),
    against today's composition in float64 on the same stored values: float32, float16 and bfloat16 flows (widened
    exactly to float32, as the kernels' loads do)."""
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        flow = FIELDS[field](2, H, W, dt)
        want, want_g = au.reference(flow, kz)
        f = flow.float().requires_grad_()
        got = au.residual_form(f, kz)
        rel = abs(got.item() - want) / abs(want)
        assert got.dtype == torch.float32 and rel <= F32_LOSS, (dt, rel)
        if dt == torch.float32:
            got.backward()
            err = (f.grad.double() - want_g).abs().max().item() / want_g.abs().max().item()
            assert err <= F32_GRAD, err


def test_argument_validation_without_gpu(gfla):
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    p, n = ctypes.cast(buf, ctypes.c_void_p), None
    for sfx in ("f32", "f64", "f16", "bf16"):
        fwd, bwd = getattr(L, "gfla_affine_reg_fwd_" + sfx), getattr(L, "gfla_affine_reg_bwd_" + sfx)
        assert fwd(n, p, p, 1, 8, 8, 3, n) == -1 and fwd(p, n, p, 1, 8, 8, 3, n) == -1 and fwd(p, p, n, 1, 8, 8, 3, n) == -1
        assert bwd(n, p, p, p, 1, 8, 8, 3, n) == -1 and bwd(p, n, p, p, 1, 8, 8, 3, n) == -1
        assert bwd(p, p, p, n, 1, 8, 8, 3, n) == -1
        for B, H, W, k in ((0, 8, 8, 3), (1, 0, 8, 3), (1, 8, -1, 3), (1, 2, 8, 3), (1, 8, 4, 5)):
            assert fwd(p, p, p, B, H, W, k, n) == -2 and bwd(p, p, p, p, B, H, W, k, n) == -2, (B, H, W, k)
        for k in (1, 8, 0):
            assert fwd(p, p, p, 1, 8, 8, k, n) == -3 and bwd(p, p, p, p, 1, 8, 8, k, n) == -3, k
    ws = L.gfla_affine_reg_workspace_bytes
    assert ws(0, 8, 8, 3) == -2 and ws(1, 2, 8, 3) == -2 and ws(1, 8, 8, 1) == -3 and ws(1, 8, 8, 8) == -3
    for k in range(2, 8):
        last = 0
        for B, H, W in ((1, 7, 7), (1, 7, 9), (1, 16, 32), (1, 17, 32), (1, 17, 33), (2, 17, 33), (32, 64, 64),
                        (32, 200, 300), (32, 2048, 2048)):
            got = ws(B, H, W, k)
            assert got > 0 and got >= last, (B, H, W, k, got)
            last = got


@pytest.mark.parametrize("kz", [3, 5])
def test_cpu_tensors_take_the_torch_composition(gfla, kz):
    from util import make_flow
    mod = gfla.AffineRegularizationLoss(kz)
    assert mod.impl == "auto"
    for dt in (torch.float32, torch.float64):
        flow = make_flow("coherent", 2, 12, 10, dt, seed=7)
        f1, f2 = flow.clone().requires_grad_(), flow.clone().requires_grad_()
        got = mod(f1)
        grid, weights = mod.flow2grid(f2), mod.kernel.type_as(f2)
        want = mod.calculate_loss(grid[:, 0:1], weights) + mod.calculate_loss(grid[:, 1:2], weights)
        got.backward()
        want.backward()
        assert torch.equal(got, want) and torch.equal(f1.grad, f2.grad)
    multi = gfla.MultiAffineRegularizationLoss({"2": 5, "3": 3}, impl="torch")
    flows = [make_flow("coherent", 1, 8, 6, seed=8), make_flow("coherent", 1, 16, 12, seed=9)]
    assert torch.equal(multi(flows), gfla.AffineRegularizationLoss(3)(flows[0]) + gfla.AffineRegularizationLoss(5)(flows[1]))
    assert all(m.impl == "torch" for m in multi.method_dic.values())
    with pytest.raises(ValueError):
        gfla.AffineRegularizationLoss(3, impl="triton")
