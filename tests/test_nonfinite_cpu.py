"""The case list of tests/nonfinite_util.py on the host alone, before anything goes to the GPU: every case discriminates (its
oracle has non-finite elements, the other samples have none, the planted element is where its name says), the check itself
rejects a laundering and an over-poisoning stand-in, and torch's own semantics that the cases lean on are pinned."""
import pytest
import torch
import torch.nn.functional as F

import nonfinite_util as nu

CASES = nu.all_cases()
NAN = float("nan")


@pytest.fixture(scope="module")
def oracles():
    """every case's planted inputs and oracle, computed once; read-only"""
    memo = {}

    def get(case):
        if case.name not in memo:
            inputs = case.make()
            memo[case.name] = (inputs, case.oracle(inputs))
        return memo[case.name]
    return get


def test_case_names_are_unique_and_every_op_is_there():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert {c.op for c in CASES} >= set(nu.OPS)
    for op in nu.PER_SAMPLE_OPS:                      # one case per op plants in the LAST sample
        assert any(c.op == op and c.sample not in (None, 0) for c in CASES), op


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_discriminates_on_the_oracle_alone(case, oracles):
    inputs, want = oracles(case)
    nu.self_check(case, inputs, want)
    # the oracle passes its own check
    nu.check(case, {name: q.want for name, q in want.items()}, want)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_stand_ins_are_rejected(case, oracles):
    _, want = oracles(case)
    with pytest.raises(AssertionError, match="laundered [1-9]"):
        nu.check(case, nu.laundering_stand_in(want), want)
    if case.sample is not None and next(iter(want.values())).batched:
        with pytest.raises(AssertionError, match="over-poisoned [1-9]"):
            nu.check(case, nu.over_poisoning_stand_in(case, want), want)


def test_an_allowance_outside_the_planted_sample_is_refused(oracles):
    case = next(c for c in CASES if c.sample == 0)
    _, want = oracles(case)
    name, q = next(iter(want.items()))
    everywhere = nu.Quantity(q.want, q.bar, allow=torch.ones_like(q.want, dtype=torch.bool), floor=q.floor)
    with pytest.raises(AssertionError, match="outside the planted sample"):
        nu.check(case, {name: q.want}, {name: everywhere})


# ---- torch's own semantics that the cases lean on -----------------------------------------------------------------------------
def test_torch_relu_keeps_nan_and_passes_its_gradient():
    x = torch.tensor([NAN, -1.0, 2.0, float("inf"), float("-inf")], dtype=torch.float64, requires_grad=True)
    y = F.relu(x)
    assert torch.isnan(y[0]) and y[1:].tolist() == [0.0, 2.0, float("inf"), 0.0]
    y.backward(torch.ones_like(y))
    # threshold_backward: the gradient is zeroed where the result <= 0, and NaN <= 0 is false
    assert x.grad.tolist() == [1.0, 0.0, 1.0, 1.0, 0.0]


def test_torch_leaky_relu():
    x = torch.tensor([NAN, -2.0, 3.0, float("-inf")], dtype=torch.float64, requires_grad=True)
    y = F.leaky_relu(x, 0.1)
    assert torch.isnan(y[0]) and y[1:].tolist() == [-0.2, 3.0, float("-inf")]
    y.backward(torch.ones_like(y))
    assert x.grad.tolist() == [0.1, 0.1, 1.0, 0.1]             # x > 0 ? 1 : slope, also for a NaN


@pytest.mark.parametrize("slot", range(4))
def test_torch_max_pool2d_returns_and_routes_to_a_nan_in_any_slot(slot):
    x = torch.tensor([[1.0, 4.0], [3.0, 2.0]], dtype=torch.float64).view(1, 1, 2, 2).clone()
    x[0, 0, slot // 2, slot % 2] = NAN
    x.requires_grad_()
    y = F.max_pool2d(x, 2, 2)
    assert torch.isnan(y).all()
    y.backward(torch.full_like(y, 7.0))
    want = torch.zeros(4, dtype=torch.float64)
    want[slot] = 7.0
    assert torch.equal(x.grad.view(-1), want)


def test_torch_max_pool2d_two_nans_the_last_one_in_scan_order_gets_the_gradient():
    x = torch.tensor([[NAN, 4.0], [NAN, 2.0]], dtype=torch.float64).view(1, 1, 2, 2).requires_grad_()
    F.max_pool2d(x, 2, 2).backward(torch.ones(1, 1, 1, 1, dtype=torch.float64))
    assert x.grad.view(-1).tolist() == [0.0, 0.0, 1.0, 0.0]


def test_torch_max_dim_returns_nan_at_the_first_nan():
    x = torch.tensor([[1.0, 5.0], [NAN, 2.0], [7.0, 9.0], [NAN, 3.0]], dtype=torch.float64)
    value, index = torch.max(x, dim=0)
    assert torch.isnan(value[0]) and index[0].item() == 1
    assert value[1].item() == 9.0 and index[1].item() == 2


def test_torch_l1_loss_backward_is_sign_with_nan_to_zero_or_nan():
    """gram_l1.hip's sign_of maps NaN to 0 on purpose; what torch does is recorded here, whichever it is, so that a change
    of torch's shows: the GPU cases compare with the float64 composition, not with this"""
    d = torch.tensor([NAN, -2.0, 0.0, 3.0], dtype=torch.float64, requires_grad=True)
    F.l1_loss(d, torch.zeros_like(d), reduction="sum").backward()
    assert d.grad[1:].tolist() == [-1.0, 0.0, 1.0]
    assert torch.isnan(d.grad[0]) or d.grad[0].item() == 0.0
    assert torch.isnan(torch.sign(torch.tensor(NAN))) or torch.sign(torch.tensor(NAN)).item() == 0.0


def test_torch_softmax_with_one_nan_logit_is_all_nan():
    z = torch.tensor([0.5, NAN, -1.0], dtype=torch.float64)
    assert torch.isnan(torch.softmax(z, dim=0)).all()
    assert torch.sigmoid(torch.tensor(float("-inf"), dtype=torch.float64)).item() == 0.0     # finite: the oracle decides


def test_torch_normalize_keeps_a_nan_norm():
    v = torch.tensor([1.0, NAN, 2.0], dtype=torch.float64)
    assert torch.isnan(F.normalize(v, dim=0, eps=1e-12)).all()
