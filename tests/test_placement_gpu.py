"""Every op at every 16-byte phase, inside red zones (tests/placement_util.py has the harness and the rows,
tests/test_placement_cpu.py proves on the host that it discriminates; DESIGN.md, "Pointer placement").

A row runs once on fresh aligned tensors, then with its inputs, its upstream gradients and everything its wrappers allocate
placed `phase` elements into NaN-filled, red-zoned buffers.  The placed run must
    1  be within the op's existing bar of the float64 host oracle, element by element (nonfinite_util.check: a NaN left in
       an output is an element the kernel never wrote, or a read of the red zone),
    2  leave every red zone and every input as it was (placement_util.check_zones: workspaces included),
    3  be bit-equal to the aligned run, but for the quantities of placement_util.EXEMPT and those whose two ALIGNED runs
       differ,
    4  have produced every checked result in a recorded buffer at the requested phase, some of them during the backward,
    5  end in _lib.Unsupported only under the mixed placement and only for the rows of placement_util.REFUSES."""
import pytest
import torch

import nonfinite_util as nu
import placement_util as pu

pytestmark = pytest.mark.gpu
ROWS = pu.all_rows()
PARAMS = [(row, placement) for row in ROWS for placement in pu.placements(row.dtype)]


@pytest.fixture(scope="module")
def aligned():
    """per row, computed once and left unchanged: the float64 host oracle, the torch composition on the GPU where the op's
    bar is that error, and two runs on fresh aligned tensors"""
    memo = {}

    def get(gfla, row):
        if row.name not in memo:
            inputs = row.inputs()
            want = row.case.oracle(inputs)
            comp = row.case.composition(gfla, inputs) if row.case.composition is not None else None
            runs = []
            for _ in range(2):
                got = pu.run_row(gfla, row)[0]
                nu.check(row.case, got, want, comp)
                runs.append({name: got[name].detach().clone() for name in want})
            memo[row.name] = (want, comp, runs)
        return memo[row.name]
    return get


def _paths(lib):
    return [lib.path_count(p) for p in range(lib.PATH_COUNT)]


@pytest.mark.parametrize("row,placement", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_placed_run(gfla, aligned, row, placement):
    from global_flow_local_attention_amd import _lib
    want, comp, (first, second) = aligned(gfla, row)
    names = {v: k for k, v in vars(_lib).items() if k.startswith("PATH_") and k != "PATH_COUNT"}
    before = _paths(_lib)
    got, records, refused, mode = pu.run_row(gfla, row, placement)
    torch.cuda.synchronize()
    taken = [names.get(p, str(p)) for p, (a, b) in enumerate(zip(before, _paths(_lib))) if b > a]
    head = "%s %s (input phase %d): paths %s" % (row.name, placement, placement.input_phase(row.dtype), ",".join(taken) or "-")
    if refused is not None:                                                              # 5
        print("%s: refused, %s" % (head, refused))
        pu.check_zones(records)
        assert placement.name == "mixed" and row.name in pu.REFUSES, "%s: refused outside the REFUSES table: %s" % (head, refused)
        return
    print("%s; the mode %s" % (head, "was entered by reaching_backward %d times" % mode.entered_for_backward
                               if mode.entered_for_backward else "reached every backward by itself"))
    failures = []
    for step in (lambda: nu.check(row.case, got, want, comp), lambda: pu.check_zones(records)):     # 1, 2
        try:
            step()
        except AssertionError as e:
            failures.append(str(e))
    made_in_backward = sum(1 for r in records if r.kind != "input" and r.in_backward)
    for name in want:                                                                    # 3, 4
        equal, settled = pu.bit_equal(got[name], first[name]), pu.bit_equal(first[name], second[name])
        exempt = pu.EXEMPT.get((row.op, name))
        rec = pu.covering(records, got[name])
        where = "not in a recorded buffer" if rec is None else "%s buffer, %d bytes past a 16-byte boundary" % (
            rec.kind, got[name].data_ptr() % 16)
        print("%s %s %s: %s; %s" % (row.name, placement, name, "bit-equal to the aligned run" if equal else
                                    "NOT bit-equal (%s)" % ("exempt: " + exempt if exempt else "the aligned runs differ too: exempt by "
                                                            "measurement" if not settled else "NOT exempt"), where))
        if not equal and settled and not exempt:
            failures.append("%s %s: differs bitwise from the aligned run" % (row.name, name))
        made_by = pu.TORCH_MADE.get((row.op, name, pu.dtype_name(row.dtype)))
        if rec is None and made_by is None:
            failures.append("%s %s: the result is no view of a recorded buffer (the placing mode did not see its allocation)"
                            % (row.name, name))
        if rec is not None and rec.kind not in ("input", "inout") and got[name].numel() == rec.view.numel() and rec.view.numel():
            want_phase = placement.alloc_phase(got[name].dtype, records.index(rec))
            if got[name].storage_offset() != rec.lo or rec.phase != want_phase:
                failures.append("%s %s: at offset %d of its buffer, phase %d asked for" % (row.name, name, got[name].storage_offset()
                                                                                         - rec.lo + rec.phase, want_phase))
    if row.autograd and not made_in_backward:
        failures.append("%s: no recorded allocation was made during the backward" % row.name)
    for path in row.path or ():
        if path not in taken:
            failures.append("%s: path %s did not run (ran: %s)" % (row.name, path, taken))
    assert not failures, "\n".join(failures)


def test_every_op_dtype_and_placement_is_covered():
    assert {r.op for r in ROWS} >= set(nu.OPS) | set(pu.ADDED_OPS)
    for row in ROWS:
        names = [p.name for r, p in PARAMS if r is row]
        assert names == ["uniform%d" % p for p in pu.PHASES[row.dtype.itemsize]] + ["mixed"]
