"""float16 storage without a GPU: every _f16 entry point and gfla_fc_forward_f16 resolve, the dtype maps to its suffix,
the host-side argument checks answer as the f32 ones do, and TrainerShell builds a GradScaler for amp="fp16" only."""
import ctypes

import pytest
import torch


def test_every_f16_symbol_resolves(gfla):
    from global_flow_local_attention_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    bases = ("gfla_block_extractor_fwd", "gfla_block_extractor_bwd", "gfla_block_extractor_unfold_fwd",
             "gfla_block_extractor_unfold_bwd", "gfla_local_attn_reshape_fwd", "gfla_local_attn_reshape_bwd",
             "gfla_resample2d_fwd", "gfla_resample2d_bwd", "gfla_local_attn_aggregate_fwd", "gfla_local_attn_aggregate_bwd",
             "gfla_local_attn_source_bwd", "gfla_flow_warp_fwd", "gfla_flow_warp_bwd", "gfla_instance_norm_fwd",
             "gfla_instance_norm_bwd")
    names = ["%s_f16" % base for base in bases]
    names += ["gfla_fc_forward_f16", "gfla_mask_blend_fwd_f16", "gfla_mask_blend_bwd_f16",
              "gfla_local_attn_aggregate_fwd_ws_f16"]
    for name in names:
        assert hasattr(handle, name), name
        assert name in gfla.exported_symbols(), name
    _lib.lib()   # argtypes set for every one of them


def test_suffix_of_float16(gfla):
    from global_flow_local_attention_amd import _lib
    assert _lib.suffix(torch.zeros(1, dtype=torch.float16), "x") == "f16"
    assert _lib.suffix(torch.zeros(1, dtype=torch.bfloat16), "x") == "bf16"
    with pytest.raises(TypeError, match="float16"):
        _lib.suffix(torch.zeros(1, dtype=torch.int32), "x")
    assert _lib.reduction_like(torch.zeros(2, dtype=torch.float16)).dtype == torch.float32


def test_f16_entry_points_validate_arguments(gfla):
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    n = None
    buf = (ctypes.c_uint16 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f32 = (ctypes.c_float * 64)()
    q = ctypes.cast(f32, ctypes.c_void_p)
    # NULL pointers: -1
    assert L.gfla_block_extractor_fwd_f16(n, n, n, 1, 1, 4, 4, 4, 4, 3, n) == -1
    assert L.gfla_block_extractor_bwd_f16(n, n, n, n, n, 1, 1, 4, 4, 4, 4, 3, n) == -1
    assert L.gfla_local_attn_reshape_fwd_f16(n, n, 1, 4, 4, 3, n) == -1
    assert L.gfla_resample2d_fwd_f16(n, n, n, 1, 1, 4, 4, 4, 4, 4, 1, n) == -1
    assert L.gfla_fc_forward_f16(n, n, n, n, n, n, n, n, n, 1, 16, 8, 8, 3, 0.1, n) == -1
    # bad shapes: -2, as for float32
    assert L.gfla_block_extractor_fwd_f16(p, p, p, 0, 1, 4, 4, 4, 4, 3, n) == -2
    assert L.gfla_resample2d_fwd_f16(p, p, p, 1, 1, 4, 4, 4, 4, 1, 1, n) == -2          # kernel_size < 2
    assert L.gfla_block_extractor_fwd_f32(q, q, q, 0, 1, 4, 4, 4, 4, 3, n) == -2
    # k > 5: -3 (GFLA_ERR_UNSUPPORTED)
    assert L.gfla_local_attn_aggregate_fwd_f16(p, p, p, p, n, 1, 1, 4, 4, 4, 4, 9, 1, n) == -3
    assert L.gfla_block_extractor_bwd_f16(p, p, p, p, q, 1, 1, 4, 4, 4, 4, 7, n) == -3
    # gfla_convert_multi: nothing to do is fine, NULL with n > 0 is not
    assert L.gfla_convert_multi(n, n, 0, n, n, 0, n, n, 0, n, n, 0, 3, n) == 0
    assert L.gfla_convert_multi(n, n, 4, n, n, 0, n, n, 0, n, n, 0, 2, n) == -1


def test_path_ids(gfla):
    from global_flow_local_attention_amd import _lib
    assert _lib.PATH_FC_PACK_F16 == 21 and _lib.PATH_COUNT == 22
    assert _lib.path_count(_lib.PATH_FC_PACK_F16) >= 0
    assert _lib.path_count(_lib.PATH_COUNT) == -1


def test_trainer_amp_builds_a_scaler_for_fp16_only(gfla):
    from global_flow_local_attention_amd.trainer import TrainerShell
    net = torch.nn.Linear(4, 4)
    assert TrainerShell(net).scaler is None
    assert TrainerShell(net, amp=None).amp is None
    shell = TrainerShell(net, amp="fp16")
    assert isinstance(shell.scaler, torch.amp.GradScaler)
    assert TrainerShell(net, amp="bf16").scaler is None
    with pytest.raises(ValueError):
        TrainerShell(net, amp="fp8")
