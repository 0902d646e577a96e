"""The loss-side matrix-core ops and the face blend on inputs on which their float32 arithmetic is exact
(tests/loss_exact_util.py: how the inputs are built, the rounding counts read from the kernels, the planted-bug table;
tests/test_loss_exact_cpu.py: the premises).  The oracle is float64 on the host.  No element is left out anywhere:

* `max_cosine_similarity`: best == the rational cosine, index == the first maximal row, for tuning key 5 in {0, 1, 2, 3} and
  identical in float32 / float16 / bfloat16; the gradients within the existing bars of float64 autograd at that index.
* `gram_l1`: the saved D is 0 exactly where the integer sums agree, has the oracle's sign everywhere else, is symmetric bit
  for bit and within 3 float32 roundings of max(|Gx|, |Gy|) at each entry (torch.equal where N C is a power of two); each
  gradient element within 2 float32 roundings of itself plus the storage half-ulp, and exactly 0 where the oracle is.
* `MaskBlendFunction`: the forward and all five gradients equal the float64 result rounded once to the storage type."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_exact_util as L  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPE_IDS = list(L.DTYPES)
COSINE_CASES = [(s, d) for s in L.COSINE_SHAPES for d in DTYPE_IDS] + [(s, d) for s in L.COSINE_SHAPES_16 for d in ("f16", "bf16")]


def _cosine(gfla, case, dtype, split):
    src, tgt = case["src"].to(dtype).to(DEV), case["tgt"].to(dtype).to(DEV)
    with gfla.tuned({gfla.TUNE_SPLIT: split}):
        best, index = gfla.max_cosine_similarity(src, tgt, return_index=True)
        torch.cuda.synchronize()
    assert index.dtype == torch.int32
    return best.cpu(), index.cpu()


@pytest.mark.parametrize("flavour", [0, 1], ids=["zeros-first", "negative-first"])
@pytest.mark.parametrize("shape,dname", COSINE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_max_cosine_values_and_first_maximal_rows(gfla, shape, dname, flavour):
    case = L.cosine_case(shape, flavour)
    for split in L.COSINE_SPLITS:
        best, index = _cosine(gfla, case, L.DTYPES[dname], split)
        try:
            L.cosine_new_rule(best, index, case)
        except AssertionError as err:
            raise AssertionError("tuning key 5 = %d: %s" % (split, err))


@pytest.mark.parametrize("shape", L.COSINE_SHAPES, ids=str)
def test_max_cosine_is_identical_across_storage_types_and_splits(gfla, shape):
    case = L.cosine_case(shape, 0)
    got = [_cosine(gfla, case, dt, split) for dt in L.DTYPES.values() for split in L.COSINE_SPLITS]
    for best, index in got[1:]:
        assert torch.equal(best, got[0][0]) and torch.equal(index, got[0][1])


@pytest.mark.parametrize("flavour", [0, 1], ids=["zeros-first", "negative-first"])
@pytest.mark.parametrize("shape,dname", COSINE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_max_cosine_gradients_at_the_first_maximal_rows(gfla, shape, dname, flavour):
    """the existing bars (tests/test_correctness_gpu.py, tests/test_correctness_half_gpu.py) against float64 autograd through
    the host oracle's expression, the maximum taken at want_index.  (A column whose best is 1 has no gradient: the
    second-codebook and the all-negative columns carry it.)"""
    dtype = L.DTYPES[dname]
    case = L.cosine_case(shape, flavour)
    want_s, want_t = L.cosine_grads64(case["src"], case["tgt"], case["want_index"], case["up"])
    s, t = case["src"].to(dtype).to(DEV).requires_grad_(), case["tgt"].to(dtype).to(DEV).requires_grad_()
    best, index = gfla.max_cosine_similarity(s, t, return_index=True)
    (best * case["up"].float().to(DEV)).sum().backward()
    L.cosine_new_rule(best.detach().cpu(), index.cpu(), case)
    assert s.grad.dtype == dtype and t.grad.dtype == dtype
    if dtype != torch.float32:
        want_s, want_t = want_s.to(dtype), want_t.to(dtype)
    e_s = L.assert_close(s.grad.cpu(), want_s, L.COSINE_GRAD_BAR[dtype], "grad source")
    e_t = L.assert_close(t.grad.cpu(), want_t, L.COSINE_GRAD_BAR[dtype], "grad target")
    print("%s %s: gradient errors %.3e (source, top %.3e), %.3e (target, top %.3e)" % (
        shape, dname, e_s, float(want_s.double().abs().max()), e_t, float(want_t.double().abs().max())))


# ------------------------------------------------------------------------------------------------------------- Gram
@pytest.mark.parametrize("dname", DTYPE_IDS)
@pytest.mark.parametrize("shape", L.GRAM_SHAPES, ids=str)
def test_gram_l1_exact(gfla, shape, dname):
    dtype = L.DTYPES[dname]
    case = L.gram_case(shape)
    B, C, H, W = shape
    if shape == L.GRAM_CHUNKED:     # the chunk rule read from csrc/gram_l1.hip, asserted through the workspace size
        assert L.gram_chunks(B, C, H * W)[1] >= 2
    assert gfla._lib.lib().gfla_gram_l1_workspace_bytes(B, C, H * W) == L.gram_workspace_bytes(B, C, H * W)
    scale = 1.0 if dtype == torch.float32 else 2.0 ** 16
    x, y = case["x"].to(dtype).to(DEV).requires_grad_(), case["y"].to(dtype).to(DEV).requires_grad_()
    loss = gfla.gram_l1(x, y)
    diff = loss.grad_fn.saved_tensors[2]
    (loss * scale).backward()
    assert loss.dtype == torch.float32 and loss.dim() == 0
    o = L.gram_oracle(case)
    print("%s %s: loss %.9e (oracle %.9e); worst |D - D64| / max(|Gx|, |Gy|) at the entry: %.3g roundings" % (
        shape, dname, loss.item(), o["loss"],
        float(((diff.cpu().double() - o["d"]).abs() / torch.maximum(o["gx"], o["gy"]).clamp_min(1e-300)).max()) / L.U32))
    L.gram_new_rule(case, loss.item(), diff, x.grad, dtype, "x", scale)
    L.gram_new_rule(case, loss.item(), diff, y.grad, dtype, "y", scale)


# ------------------------------------------------------------------------------------------------------- mask blend
@pytest.mark.parametrize("dname", DTYPE_IDS)
@pytest.mark.parametrize("shape", L.BLEND_SHAPES, ids=str)
def test_mask_blend_exact(gfla, shape, dname):
    dtype = L.DTYPES[dname]
    case = L.blend_case(shape)
    leaves = [t.to(dtype).to(DEV).requires_grad_() for t in case["leaves"]]
    y = gfla.MaskBlendFunction.apply(*leaves)
    y.backward(case["up"].to(dtype).to(DEV))
    L.blend_new_rule(case, y, [t.grad for t in leaves], dtype)
