"""16-bit path of the sampling-correctness loss, host side: the new entry points are declared, exported and resolvable;
16-bit host tensors are rejected like float32 ones; mixed source / target dtypes raise TypeError before anything runs."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gfla_max_cosine_fwd_f16", "gfla_max_cosine_fwd_bf16", "gfla_correctness_map_fwd_f16", "gfla_correctness_map_fwd_bf16",
       "gfla_correctness_map_bwd_f16", "gfla_correctness_map_bwd_bf16"]


def test_half_entry_points_are_declared_and_exported(gfla):
    header = open(os.path.join(ROOT, "include", "gfla_hip.h")).read()
    handle = gfla._lib.lib()
    for name in NEW:
        assert name in gfla.exported_symbols(), name
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert hasattr(handle, name), name
    assert handle.gfla_abi_version() == 8


def test_half_entry_points_validate_arguments(gfla):
    L = gfla._lib.lib()
    n = None
    assert L.gfla_max_cosine_fwd_f16(n, n, n, n, n, 1, 8, 16, 16, 1e-8, n) == -1       # NULL pointer
    assert L.gfla_max_cosine_fwd_bf16(n, n, n, n, n, 1, 8, 16, 16, 1e-8, n) == -1
    assert L.gfla_correctness_map_fwd_f16(n, n, n, n, n, 1, 8, 16, 1e-8, 1e-8, n) == -1
    assert L.gfla_correctness_map_bwd_bf16(n, n, n, n, n, n, n, n, n, 1, 8, 16, 1e-8, 1e-8, n) == -1


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_host_tensors_are_rejected(gfla, dtype):
    x = torch.zeros(1, 4, 3, 3, dtype=dtype)
    with pytest.raises(NotImplementedError):
        gfla.max_cosine_similarity(x, x)
    with pytest.raises(NotImplementedError):
        gfla.CorrectnessMapFunction.apply(torch.zeros(1, 4, 9), x.view(1, 4, 9), torch.ones(1, 9), 1e-8)


def test_mixed_feature_dtypes_raise_type_error(gfla, monkeypatch):
    """the dtype check sits behind the device check; with that one out of the way it must fire before any library call"""
    from global_flow_local_attention_amd import _lib
    monkeypatch.setattr(_lib, "require_gpu", lambda *tensors: None)
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("the library was called"))
    a = torch.zeros(1, 4, 9)
    for da, db in ((torch.float16, torch.float32), (torch.float16, torch.bfloat16), (torch.float32, torch.bfloat16)):
        with pytest.raises(TypeError):
            gfla.max_cosine_similarity(a.to(da), a.to(db))
    with pytest.raises(TypeError):
        gfla.CorrectnessMapFunction.apply(a.half(), a.half(), torch.ones(1, 9), 1e-8)
    with pytest.raises(TypeError):
        gfla.max_cosine_similarity(a.double(), a.double())


def test_half_features_argument(gfla):
    assert gfla.PerceptualCorrectness().half_features == "float32"
    assert gfla.PerceptualCorrectness(half_features="native").half_features == "native"
    with pytest.raises(ValueError):
        gfla.PerceptualCorrectness(half_features="half")
