"""tests/placement_util.py on the host alone: the placing mode does what it says on host tensors, torch stand-ins for the
mistakes a kernel can make at an odd pointer are each rejected by exactly the intended assertion, the finite case list has one
case per (op, row, dtype) with finite oracles, and the package calls no factory the mode does not intercept."""
import os
import re

import pytest
import torch

import nonfinite_util as nu
import placement_util as pu

NAN = float("nan")
ROWS = pu.all_rows()


def _mode(placement):
    return pu.Placing(placement, "cpu")


# ---- the mode on host tensors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int32])
def test_uniform_placements_put_every_allocation_at_the_phase(dtype):
    esize = dtype.itemsize
    assert [p.name for p in pu.placements(dtype)] == ["uniform%d" % p for p in pu.PHASES[esize]] + ["mixed"]
    for placement, phase in zip(pu.placements(dtype), pu.PHASES[esize]):
        with _mode(placement) as mode:
            made = [torch.empty(5, 3, dtype=dtype), torch.zeros(7, dtype=dtype), torch.empty(4, dtype=dtype).new_empty((2, 2)),
                    torch.empty_like(torch.empty(3, dtype=dtype)), torch.full((3,), 2, dtype=dtype), torch.ones(2, dtype=dtype)]
        for t in made:
            rec = pu.covering(mode.records, t)
            assert rec is not None and rec.view.data_ptr() == t.data_ptr() and rec.phase == phase
            assert t.storage_offset() == pu.ZONE_BYTES // esize + phase and t.is_contiguous()
            assert (t.data_ptr() - rec.buffer.data_ptr()) % 16 == (phase * esize) % 16
            assert rec.buffer.numel() - rec.hi == pu.ZONE_BYTES // esize and rec.lo - phase == pu.ZONE_BYTES // esize
        assert len(mode.records) == 8                    # the two throw-away tensors included: every factory call is recorded
        pu.check_zones(mode.records)


def test_phases_cover_the_byte_offsets_the_issue_names():
    assert [p * 4 for p in pu.PHASES[4]] == [4, 8, 12] and [p * 2 for p in pu.PHASES[2]] == [2, 6, 8, 14] and pu.PHASES[8] == (1,)
    assert pu.ZONE_BYTES >= 256 and pu.ZONE_BYTES % 256 == 0


def test_mixed_placement_cycles_through_the_phases_in_allocation_order():
    mixed = pu.placements(torch.float32)[-1]
    with _mode(mixed) as mode:
        made = [torch.empty(4) for _ in range(6)] + [torch.empty(4, dtype=torch.bfloat16) for _ in range(2)]
    assert [r.phase for r in mode.records] == [1, 2, 3, 1, 2, 3, 4, 7]
    assert mixed.input_phase(torch.float32) == 1 and mixed.input_phase(torch.float16) == 1
    assert len({(t.data_ptr() - r.buffer.data_ptr()) % 16 for t, r in zip(made[:3], mode.records)}) == 3


def test_empty_strided_keeps_the_strides_it_asked_for():
    with _mode(pu.placements(torch.float32)[1]) as mode:
        t = torch.empty_strided((3, 4), (1, 5))
        like = torch.empty_like(t)
    assert t.stride() == (1, 5) and t.shape == (3, 4) and like.stride() == torch.empty_like(torch.empty_strided((3, 4), (1, 5))).stride()
    rec = mode.records[0]
    assert rec.hi - rec.lo == 1 + 2 * 1 + 3 * 5 and t.storage_offset() == rec.lo
    pu.check_zones(mode.records)


def test_interiors_nan_for_empty_zero_for_zeros_value_for_full():
    with _mode(pu.placements(torch.float16)[2]) as mode:
        e, z, f = torch.empty(9, dtype=torch.float16), torch.zeros(9, dtype=torch.float16), torch.full((9,), 3.0, dtype=torch.float16)
        zl, nz = torch.zeros_like(e), e.new_zeros((2, 3))
        i = torch.empty(5, dtype=torch.int32)
    assert torch.isnan(e).all() and (z == 0).all() and (f == 3).all() and (zl == 0).all() and (nz == 0).all()
    assert (i.view(torch.uint8) == pu.INT_FILL).all()
    for rec in mode.records:                             # the zones hold the NaN / byte pattern
        zone = torch.cat((rec.buffer[:rec.lo], rec.buffer[rec.hi:]))
        assert torch.isnan(zone).all() if zone.dtype.is_floating_point else (zone.view(torch.uint8) == pu.INT_FILL).all()


def test_uint8_keeps_the_base_alignment_and_still_has_zones():
    for placement in pu.placements(torch.float32):
        with _mode(placement) as mode:
            ws = torch.empty(100, dtype=torch.uint8)
            idx = torch.empty(6, dtype=torch.int64)
        for t, rec in zip((ws, idx), mode.records):
            assert rec.phase == 0 and (t.data_ptr() - rec.buffer.data_ptr()) % 256 == 0
            assert rec.lo * t.element_size() == pu.ZONE_BYTES and (rec.buffer.numel() - rec.hi) * t.element_size() == pu.ZONE_BYTES


def test_other_devices_and_other_ops_are_left_alone():
    with pu.Placing(pu.placements(torch.float32)[0], "cuda") as mode:        # acts on device tensors only
        t = torch.empty(4)
        c = torch.ones(3).clone()
    assert t.storage_offset() == 0 and c.storage_offset() == 0 and not mode.records
    with _mode(pu.placements(torch.float32)[0]) as mode:
        x = torch.empty(4)
        made = [x.clone(), x.to(torch.float64), torch.cat((x, x))]           # clone, _to_copy and cat: not intercepted
    assert len(mode.records) == 1 and all(m.storage_offset() == 0 for m in made)


class _Toy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = torch.empty_like(x)
        y.copy_(x * 2)
        return y

    @staticmethod
    def backward(ctx, g):
        ctx_seen.append((g.storage_offset(), g.data_ptr()))
        dx = torch.empty_like(g)
        dx.copy_(g * 2)
        return dx


ctx_seen = []


def test_the_mode_is_seen_in_forward_and_backward_and_grad_keeps_its_offset():
    del ctx_seen[:]
    x_host, up_host = torch.arange(6.0), torch.ones(6)

    def run(dev):
        x = dev(x_host).requires_grad_()
        y = _Toy.apply(x)
        up = dev(up_host)
        y.backward(up)
        return {"y": y, "gx": x.grad, "up": up}
    placement = pu.placements(torch.float32)[2]
    got, records, refused, _ = pu.run_placed(run, placement, "cpu", [_Toy])
    assert refused is None
    zone = pu.ZONE_BYTES // 4
    assert got["y"].storage_offset() == zone + 3 and got["gx"].storage_offset() == zone + 3
    assert ctx_seen == [(zone + 3, got["up"].data_ptr())]          # the upstream gradient reached backward as the placed tensor
    ry, rg = pu.covering(records, got["y"]), pu.covering(records, got["gx"])
    assert ry is not None and not ry.in_backward and rg is not None and rg.in_backward
    assert torch.equal(got["gx"], torch.full((6,), 2.0)) and torch.equal(got["y"], x_host * 2)
    assert _Toy.__dict__["backward"].__func__.__name__ == "backward" and _Toy.backward(None, torch.ones(2)).storage_offset() == 0
    pu.check_zones(records)


# ---- stand-in kernels: each mistake is reported by exactly the intended assertion ---------------------------------------------
N = 11                                                   # n % 4 == 3: a tail the vector body does not reach
TOY = nu.Case("toy-doubling", "toy", None, None, None, None, None)


def _raw(t, start, count):
    """`count` elements of t's buffer from `start` elements after t's first one: a kernel's pointer arithmetic"""
    return t.as_strided((count,), (1,), t.storage_offset() + start)


def _good(x, y, ws):
    y.copy_(x * 2)


def _one_past_the_end(x, y, ws):
    _good(x, y, ws)
    _raw(y, N, 1).fill_(0.0)


def _one_before_the_start(x, y, ws):
    _good(x, y, ws)
    _raw(y, -1, 1).fill_(0.0)


def _skips_the_tail(x, y, ws):
    body = N - N % 4
    _raw(y, 0, body).copy_(_raw(x, 0, body) * 2)


def _rounds_its_start_down(x, y, ws):
    back = (x.data_ptr() % 16) // x.element_size()       # to the 16-byte boundary below x: its first `back` reads are the red zone
    y.copy_(_raw(x, -back, N) * 2)


def _modifies_its_input(x, y, ws):
    _good(x, y, ws)
    x[N // 2] += 1


def _overruns_its_workspace(x, y, ws):
    _good(x, y, ws)
    _raw(ws, 0, ws.numel() + 1).fill_(1)


def _outcome(kernel, placement):
    """which of the harness's assertions the stand-in trips: the messages"""
    x_host = torch.arange(1.0, N + 1)
    want = {"y": nu.Quantity(x_host * 2, 0.0, batched=False)}

    def run(dev):
        x = dev(x_host)
        y, ws = torch.empty_like(x), torch.empty(24, dtype=torch.uint8)
        kernel(x, y, ws)
        return {"y": y}
    got, records, _, _ = pu.run_placed(run, placement, "cpu")
    found = []
    for step in (lambda: nu.check(TOY, got, want), lambda: pu.check_zones(records)):
        try:
            step()
        except AssertionError as e:
            found += str(e).split("\n")
    return found


STAND_INS = [(_one_past_the_end, r"red zone past the end of buffer 1 \(empty .*empty_like.*first at offsets \[11\]"),
             (_one_before_the_start, r"red zone before the start of buffer 1 \(empty .*first at offsets \[-1\]"),
             (_skips_the_tail, r"toy-doubling y: .* over-poisoned 3 "),
             (_rounds_its_start_down, r"toy-doubling y: .* over-poisoned [1-3] "),
             (_modifies_its_input, r"input modified: buffer 0 \(input .* 1 elements, first at \[5\]"),
             (_overruns_its_workspace, r"red zone past the end of buffer 2 \(empty .*\(24,\).* 1 elements, first at offsets \[24\]")]


@pytest.mark.parametrize("placement", pu.placements(torch.float32), ids=repr)
def test_a_correct_stand_in_passes(placement):
    assert _outcome(_good, placement) == []


@pytest.mark.parametrize("placement", pu.placements(torch.float32), ids=repr)
@pytest.mark.parametrize("kernel,message", STAND_INS, ids=[k.__name__.strip("_") for k, _ in STAND_INS])
def test_stand_in_is_rejected_by_exactly_the_intended_assertion(kernel, message, placement):
    found = _outcome(kernel, placement)
    assert len(found) == 1 and re.search(message, found[0]), found


def test_a_tensor_declared_in_place_may_change_but_its_zones_may_not():
    host = torch.arange(1.0, N + 1)

    def run(dev):
        u = dev.inout(host)
        u.mul_(2)
        return {"u": u}
    got, records, _, _ = pu.run_placed(run, pu.placements(torch.float32)[0], "cpu")
    assert records[0].kind == "inout" and torch.equal(got["u"], host * 2)
    pu.check_zones(records)
    _raw(got["u"], N, 1).fill_(0.0)
    with pytest.raises(AssertionError, match="red zone past the end of buffer 0"):
        pu.check_zones(records)


def test_the_aligned_allocator_hides_every_one_of_them():
    """what the rest of the suite sees: the same stand-ins on aligned tensors with slack behind them, judged by the values
    alone, pass"""
    x = torch.arange(1.0, N + 1)
    for kernel in (_one_past_the_end, _modifies_its_input, _rounds_its_start_down):
        buf = torch.zeros(N + 16)
        y = buf[:N]
        xin = x.clone()
        kernel(xin, y, torch.empty(32, dtype=torch.uint8)[:24])
        nu.check(TOY, {"y": y}, {"y": nu.Quantity(x * 2, 0.0, batched=False)})


# ---- the rows ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracles():
    memo = {}

    def get(row):
        if row.name not in memo:
            memo[row.name] = row.case.oracle(row.inputs())
        return memo[row.name]
    return get


def test_one_row_per_op_row_and_dtype_and_every_op_is_there():
    cases = nu.all_cases()
    assert len(cases) == 258
    keys = {(c.op,) + pu.row_key(c) for c in cases}
    ragged = pu.ragged_rows()
    assert len(ragged) == len(keys) and len({r.name for r in ROWS}) == len(ROWS)
    assert {r.op for r in ragged} == set(nu.OPS)
    for op in nu.OPS:                                    # every dtype the op has cases for
        assert {r.dtype for r in ragged if r.op == op} == {nu.DTYPES[pu.row_key(c)[1]] for c in cases if c.op == op}, op
    assert {r.op for r in ROWS} >= set(nu.OPS) | set(pu.ADDED_OPS)


def test_cases_that_collapse_into_one_row_have_the_same_finite_inputs():
    first = {}
    for case in nu.all_cases():
        if case.op == "VGG19Features":
            continue
        key = (case.op,) + pu.row_key(case)
        inputs = pu.finite_inputs(case)
        if key not in first:
            first[key] = inputs
            continue
        assert inputs.keys() == first[key].keys(), case.name
        for name, t in inputs.items():
            if isinstance(t, torch.Tensor):
                assert t.dtype == first[key][name].dtype and torch.equal(t, first[key][name]), (case.name, name)
            else:
                assert t == first[key][name], (case.name, name)


@pytest.mark.parametrize("row", ROWS, ids=repr)
def test_row_is_finite_and_its_oracle_passes_its_own_check(row, oracles):
    inputs, want = row.inputs(), oracles(row)
    for name, t in inputs.items():
        if isinstance(t, torch.Tensor) and t.is_floating_point():
            assert torch.isfinite(t).all(), name
    for name, q in want.items():
        assert torch.isfinite(q.want).all(), name
    nu.check(row.case, {name: q.want for name, q in want.items()}, want)


@pytest.mark.parametrize("row", [r for r in ROWS if r.friendly], ids=repr)
def test_vector_friendly_row_satisfies_the_shape_condition_it_cites(row):
    assert re.fullmatch(r"csrc/[\w.]+:\d+(, csrc/[\w.]+:\d+)*", row.guard), row.guard
    assert row.holds(row.inputs())
    for cite in row.guard.split(", "):
        path, line = cite.split(":")
        source = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "global_flow_local_attention_amd", path)
        with open(source) as f:
            text = f.readlines()[int(line) - 1]
        # the cited line is the guard: a test of a pointer or of the shape
        assert re.search(r"uintptr_t|& 15|% 16|% 4|& 3\)|% px", text), (cite, text)


def test_every_op_with_a_friendly_row_keeps_its_ragged_one():
    ragged = {r.op for r in ROWS if not r.friendly}
    assert {r.op for r in ROWS if r.friendly} <= ragged


def test_exemptions_and_refusals_name_rows_and_give_reasons():
    ops, names = {r.op for r in ROWS}, {r.name for r in ROWS}
    for (op, quantity), reason in pu.EXEMPT.items():
        assert op in ops and re.search(r"\w+\.(hip|h|py):\d+", reason), (op, quantity)
    for name, sentence in pu.REFUSES.items():
        assert name in names and sentence
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gfla_hip.h")) as f:
            assert " ".join(sentence.split()) in " ".join(re.sub(r"^\s*\*?\s?", "", l) for l in f.read().splitlines()), name


# ---- hygiene -------------------------------------------------------------------------------------------------------------------
def test_every_factory_the_package_calls_is_intercepted():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "global_flow_local_attention_amd")
    called = {}
    for name in sorted(os.listdir(root)):
        if name.endswith(".py"):
            with open(os.path.join(root, name)) as f:
                for m in re.finditer(r"(torch\.(?:empty|zeros|ones|full)\w*|\.new_\w+)\(", f.read()):
                    called.setdefault(m.group(1), name)
    assert len(called) >= 7                              # the scan sees the package
    stray = {k: v for k, v in called.items() if k not in pu.FACTORY_NAMES}
    assert not stray, "factory calls the placing mode does not intercept: %s" % stray
    assert len(pu.FACTORY_NAMES) == len(pu.INTERCEPTED)
    for name in pu.FACTORY_NAMES:                        # every spelling is an intercepted overload
        op = name.split(".")[1]
        assert any(str(f).split(".")[1] == op for f in pu.INTERCEPTED), name
