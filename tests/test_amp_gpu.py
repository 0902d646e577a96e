"""Mixed-precision training end to end: the generator-shaped network (tools/warp_generator.py) with the sampling-correctness
and affine-regularisation losses through TrainerShell(amp="fp16") and amp="bf16", three steps each, in strict mode (no
vendor fallback).  Both attention blocks must receive 16-bit source / target / flow (conv -> InstanceNorm -> LeakyReLU
stays in the autocast dtype) and take the 16-bit path; the losses stay finite, the parameters move, the first step's loss
is within 2e-2 of the float32 step from the same weights and batch, and a forced overflow makes the GradScaler skip."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _amp_shell(state, amp):
    import trainer_util as tu
    from global_flow_local_attention_amd.trainer import TrainerShell
    base, net = tu.build_shell(DEV, ngf=16, lr=1e-3, state=state)
    base.reducer.remove()
    shell = TrainerShell(net, lr=1e-3, correctness=base.correctness, regularization=base.regularization, attn_layer=(2, 3),
                         amp=amp)
    return shell, net


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
def test_amp_training_steps(gfla, amp):
    import trainer_util as tu
    from global_flow_local_attention_amd import _lib
    from global_flow_local_attention_amd import extractor_attn as ea
    dt = DTYPES[amp]
    batch = tu.make_batch(2, 64, 48)        # L3 (64 channels, 8x6) k3, L2 (32 channels, 16x12) k5
    ref_shell, ref_net = tu.build_shell(DEV, ngf=16, lr=1e-3)
    state = {k: v.clone() for k, v in ref_net.state_dict().items()}
    want = sum(tu.run_step(ref_shell, ref_net, batch, DEV)[0].values())      # the float32 step from the same weights
    shell, net = _amp_shell(state, amp)
    seen = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: seen.append(tuple(x.dtype for x in inp) + (out.dtype,)))
             for m in (net.attn3, net.attn2)]
    old = ea.VENDOR_FALLBACK
    ea.VENDOR_FALLBACK = "error"
    try:
        n_vendor = ea.vendor_fallback_calls
        pack0, fwd1 = _lib.path_count(_lib.PATH_FC_PACK_F16), _lib.path_count(_lib.fc_path(1))
        totals, first = [], None
        for step in range(3):
            losses, grads, before, after = tu.run_step(shell, net, batch, DEV)
            if first is None:
                first = before
            totals.append(sum(losses.values()))
            assert all(torch.isfinite(torch.tensor(v)) for v in losses.values()), losses
        assert ea.vendor_fallback_calls == n_vendor
        # both blocks, three steps, all on the 16-bit path (FC forward in arithmetic mode 1)
        assert _lib.path_count(_lib.fc_path(1)) - fwd1 == 6
        assert _lib.path_count(_lib.PATH_FC_PACK_F16) - pack0 == (6 if dt == torch.float16 else 0)
    finally:
        ea.VENDOR_FALLBACK = old
        for h in hooks:
            h.remove()
    assert len(seen) == 6 and all(d == (dt,) * 4 for d in seen), seen
    moved = sum(int(not torch.equal(first[n], p.detach())) for n, p in net.named_parameters())
    assert moved > 0.5 * len(first), "parameters did not move (%d of %d)" % (moved, len(first))
    if amp == "fp16":
        assert shell.skipped_steps < 3
    rel = abs(totals[0] - want) / abs(want)
    print("amp %s: step-0 loss %.6f, float32 %.6f, relative difference %.3e; losses %s" % (amp, totals[0], want, rel, totals))
    assert rel <= 2e-2, (totals[0], want)


def test_fp16_overflow_skips_the_step(gfla):
    import trainer_util as tu
    batch = tu.make_batch(2, 64, 48)
    shell, net = _amp_shell(None, "fp16")
    tu.run_step(shell, net, batch, DEV)
    shell.scaler.update(new_scale=2.0 ** 100)     # the scaled loss overflows float16 and float32 gradients alike
    skipped = shell.skipped_steps
    _, _, before, after = tu.run_step(shell, net, batch, DEV)
    assert shell.skipped_steps == skipped + 1
    assert shell.scaler.get_scale() < 2.0 ** 100
    for n in before:
        assert torch.equal(before[n], after[n]), n
