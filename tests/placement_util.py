"""Pointer placement: every op at every 16-byte phase, inside red zones ("Pointer placement").

Every tensor the rest of the suite hands a kernel comes straight from the caching allocator: its base sits on a 256-byte
boundary and what lies behind its end is the allocator's slack.  Here the inputs, the upstream gradients and everything the
wrappers allocate sit `phase` elements into a buffer of their own whose first and last ZONE_BYTES hold a NaN bit pattern (a
fixed byte pattern for integer types):

    place(t, phase, device)   an input, with its record
    Placing(placement)        a TorchDispatchMode that gives every factory call of the package such a buffer
    check_zones(records)      no red zone touched, no input modified

The rows are the cases of tests/nonfinite_util.py with nothing planted -- one per distinct (op, row, dtype) -- next to a
vector-friendly shape per op and the ops that list lacks; oracles, bars and check() are nonfinite_util's, no tolerance is
this file's.  tests/test_placement_cpu.py proves on the host that the harness discriminates, tests/test_placement_gpu.py
runs the rows."""
import contextlib
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode, _get_current_dispatch_mode_stack

import nonfinite_util as nu

ZONE_BYTES = 512                     # before and after every placed tensor; a multiple of 256, so phase 0 keeps the base's alignment
INT_FILL = 0xA5                      # every byte of an integer buffer
# phases in ELEMENTS by element size: 4, 8, 12 bytes; 2, 6, 8 ("8 but not 16") and 14 bytes; 8 bytes
PHASES = {4: (1, 2, 3), 2: (1, 3, 4, 7), 8: (1,)}
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}

aten = torch.ops.aten
# the factory calls the package makes (tests/test_placement_cpu.py scans its sources for others) -> what the interior holds
INTERCEPTED = {
    aten.empty.memory_format: "empty", aten.empty_strided.default: "empty", aten.empty_like.default: "empty",
    aten.new_empty.default: "empty", aten.new_empty_strided.default: "empty",
    aten.zeros.default: "value", aten.zeros_like.default: "value", aten.new_zeros.default: "value",
    aten.full.default: "value", aten.full_like.default: "value", aten.new_full.default: "value",
    aten.ones.default: "value", aten.ones_like.default: "value", aten.new_ones.default: "value",
}
# the spelling in Python source of every intercepted overload, for the hygiene scan
FACTORY_NAMES = {"torch.empty", "torch.empty_strided", "torch.empty_like", ".new_empty", ".new_empty_strided", "torch.zeros",
                 "torch.zeros_like", ".new_zeros", "torch.full", "torch.full_like", ".new_full", "torch.ones", "torch.ones_like",
                 ".new_ones"}
_bypass = [False]                    # place() allocates its own buffer while a Placing mode may be active


def shifted(dtype):
    """floating and int32 tensors move off the 16-byte boundary; uint8 (the workspaces) and everything else keep the base's
    alignment and only get the red zones"""
    return dtype.is_floating_point or dtype == torch.int32


def bits(t):
    """t through an integer view of its element size: NaN payloads and signed zeros compare as stored"""
    return t if not t.dtype.is_floating_point and t.dtype != torch.bool else t.view(_BITS[t.element_size()])


class Record(object):
    """buffer: the whole allocation.  view: the placed tensor.  saved: a copy of the whole buffer, taken when the tensor was
    placed (an input: with its values; an allocation: the fill).  [lo, hi): the elements of `buffer` the view may touch.
    kind: "input", "empty" or "value".  in_backward: made while the autograd engine was running a node."""

    def __init__(self, buffer, view, lo, hi, kind, phase, what, in_backward=False):
        self.buffer, self.view, self.lo, self.hi, self.kind, self.phase, self.what = buffer, view, lo, hi, kind, phase, what
        self.in_backward = in_backward
        self.saved = buffer.clone()

    def __iter__(self):                                   # (buffer, view, saved copy of the whole buffer)
        return iter((self.buffer, self.view, self.saved))


def _buffer(size, stride, dtype, device, phase, kind, what, in_backward=False):
    esize = dtype.itemsize
    zone = ZONE_BYTES // esize
    span = 0 if any(n == 0 for n in size) else 1 + sum((n - 1) * s for n, s in zip(size, stride))
    old, _bypass[0] = _bypass[0], True
    try:
        buffer = torch.empty(2 * zone + phase + span, dtype=dtype, device=device)
        if dtype.is_floating_point:
            buffer.fill_(float("nan"))
        else:
            buffer.view(torch.uint8).fill_(INT_FILL)
        view = buffer.as_strided(tuple(size), tuple(stride), zone + phase)
        return Record(buffer, view, zone + phase, zone + phase + span, kind, phase, what, in_backward)
    finally:
        _bypass[0] = old


def place(t, phase, device):
    """(a contiguous tensor of t's shape and values that starts `phase` elements into a fresh red-zoned buffer on `device`,
    its Record)"""
    t = t.detach()
    stride = torch.empty(t.shape, dtype=t.dtype, device="meta").stride()
    rec = _buffer(t.shape, stride, t.dtype, device, phase, "input", "input")
    old, _bypass[0] = _bypass[0], True
    try:
        rec.view.copy_(t)
        rec.saved = rec.buffer.clone()
    finally:
        _bypass[0] = old
    return rec.view, rec


class Placement(object):
    """Which phase an input and the n-th allocation get.  uniform(i): the i-th phase of the element size, for the inputs,
    the upstream gradients and every allocation (an allocation of another element size than the row's takes the i-th phase
    of its own list, cyclically: bfloat16 at 7 elements goes with float32 at 1).  mixed: the inputs at the first phase, the
    allocations cycling through their lists in allocation order, which breaks every `agree modulo 16` deterministically."""

    def __init__(self, name, index=None):
        self.name, self.index = name, index

    def __repr__(self):
        return self.name

    def _nth(self, dtype, n):
        if not shifted(dtype):
            return 0
        row = PHASES[dtype.itemsize]
        return row[n % len(row)]

    def input_phase(self, dtype):
        return self._nth(dtype, 0 if self.index is None else self.index)

    def alloc_phase(self, dtype, n):
        return self._nth(dtype, n if self.index is None else self.index)


def placements(dtype):
    """uniform(p) for every phase p of the row's storage type, and the mixed one"""
    row = PHASES[dtype.itemsize]
    return [Placement("uniform%d" % p, i) for i, p in enumerate(row)] + [Placement("mixed")]


class Placing(TorchDispatchMode):
    """Gives every factory call of INTERCEPTED that makes a tensor on `device_type` a view into a red-zoned buffer: at the
    placement's phase, with the strides the call asked for, the interior of an empty* NaN (the byte pattern for integers) and
    that of a zeros* / full* / ones* its value.  clone, _to_copy and cat are not intercepted: a wrapper that
    realigns a tensor (instance_norm._aligned) does it with one of them.  Every buffer is in self.records."""

    def __init__(self, placement, device_type="cuda"):
        super(Placing, self).__init__()
        self.placement, self.device_type, self.records = placement, device_type, []
        self.entered_for_backward = 0                     # times reaching_backward had to enter the mode itself

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        kind = INTERCEPTED.get(func)
        if kind is None or _bypass[0] or not isinstance(out, torch.Tensor) or out.device.type != self.device_type \
                or out.layout != torch.strided:
            return out
        phase = self.placement.alloc_phase(out.dtype, len(self.records))
        rec = _buffer(out.shape, out.stride(), out.dtype, out.device, phase, kind, str(func),
                      torch._C._current_graph_task_id() != -1)
        if kind == "value":
            rec.view.copy_(out)
        self.records.append(rec)
        return rec.view.requires_grad_(out.requires_grad)


def package_functions():
    """every autograd.Function of the package's modules imported so far"""
    import global_flow_local_attention_amd as pkg
    found = []
    for name, mod in sorted(sys.modules.items()):
        if mod is None or not name.startswith(pkg.__name__ + "."):
            continue
        for obj in list(vars(mod).values()):
            if isinstance(obj, type) and issubclass(obj, torch.autograd.Function) and obj.__module__ == mod.__name__ \
                    and obj not in found:
                found.append(obj)
    return found


@contextlib.contextmanager
def reaching_backward(mode, functions):
    """The engine runs a device's nodes on a thread of its own.  Where `mode` is not on that thread's stack when a backward
    of `functions` starts, enter it there for the call; where it is, change nothing."""
    saved = []

    def wrap(inner):
        def backward(ctx, *grads):
            if any(m is mode for m in _get_current_dispatch_mode_stack()):
                return inner(ctx, *grads)
            mode.entered_for_backward += 1
            with mode:
                return inner(ctx, *grads)
        return backward
    for fn in functions:
        inner = fn.__dict__.get("backward")
        if inner is not None:
            saved.append((fn, inner))
            fn.backward = staticmethod(wrap(inner.__func__ if isinstance(inner, staticmethod) else inner))
    try:
        yield
    finally:
        for fn, inner in saved:
            fn.backward = inner


def check_zones(records):
    """Every red zone is bit-identical to its fill, every INPUT buffer bit-identical to its saved copy throughout; raises
    AssertionError naming every buffer that is not."""
    bad = []
    for i, rec in enumerate(records):
        now, then = bits(rec.buffer).cpu(), bits(rec.saved).cpu()
        who = "buffer %d (%s %s%s at phase %d)" % (i, rec.kind, rec.what, tuple(rec.view.shape), rec.phase)
        for name, lo, hi in (("before the start", 0, rec.lo), ("past the end", rec.hi, now.numel())):
            hit = (now[lo:hi] != then[lo:hi]).nonzero().view(-1)
            if hit.numel():
                at = [int(h) + lo - rec.lo for h in hit[:4]]
                bad.append("red zone %s of %s written: %d elements, first at offsets %s from its first element"
                           % (name, who, hit.numel(), at))
        if rec.kind == "input":
            hit = (now[rec.lo:rec.hi] != then[rec.lo:rec.hi]).nonzero().view(-1)
            if hit.numel():
                bad.append("input modified: %s, %d elements, first at %s" % (who, hit.numel(), hit[:4].tolist()))
    assert not bad, "\n".join(bad)


def covering(records, t):
    """the record whose interior holds every element of t (None: t is no view of a recorded buffer)"""
    for rec in records:
        if t.untyped_storage().data_ptr() == rec.buffer.untyped_storage().data_ptr() and t.dtype == rec.buffer.dtype:
            span = 0 if t.numel() == 0 else 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
            if rec.lo <= t.storage_offset() and t.storage_offset() + span <= rec.hi:
                return rec
    return None


def run_placed(run, placement, device, functions=(), refusal=()):
    """run(dev) -> {name: tensor} with dev(host tensor) placing an input and every factory call placed as well.  Returns
    (results or None, records, the `refusal` exception that ended it or None, the mode)."""
    mode = Placing(placement, torch.device(device).type)

    def dev(t, kind="input"):
        view, rec = place(t, placement.input_phase(t.dtype), device)
        rec.kind = kind
        mode.records.append(rec)
        return view
    dev.inout = lambda t: dev(t, "inout")      # a tensor the op updates in place: zones checked, contents free
    got, refused = None, None
    with mode, reaching_backward(mode, functions):
        try:
            got = run(dev)
        except refusal as e:
            refused = e
    return got, mode.records, refused, mode


def run_row(gfla, row, placement=None):
    """the row's kernels on its finite inputs: aligned (placement None) or placed"""
    if placement is None:
        return row.case.run(gfla, row.inputs()), [], None, None
    from global_flow_local_attention_amd import _lib

    def run(dev):
        saved, nu.to_dev = nu.to_dev, dev
        try:
            return row.case.run(gfla, row.inputs())
        finally:
            nu.to_dev = saved
    return run_placed(run, placement, nu.DEV, package_functions(), _lib.Unsupported)


def bit_equal(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bits(a).cpu(), bits(b).cpu()))


# ---- the rows ---------------------------------------------------------------------------------------------------------------
class Row(object):
    """name: the test id.  case: a nonfinite_util.Case whose make() is called with nothing planted.  dtype: the storage type
    whose phases the row runs at.  friendly: the vector-friendly shape of its op -- guard: the file:line of the shape
    condition consulted, holds(inputs): that condition.  path: (the _lib.PATH_* names that must all have been enqueued, or
    None).  autograd: the op's backward runs on the engine (False: the C ABI is called directly, or forward only)."""

    def __init__(self, name, case, dtype, friendly=False, guard=None, holds=None, path=None, autograd=True):
        self.name, self.case, self.op, self.dtype = name, case, case.op, dtype
        self.friendly, self.guard, self.holds, self.path, self.autograd = friendly, guard, holds, path, autograd
        self._inputs = None

    def __repr__(self):
        return self.name

    def inputs(self):
        """the case's finite host inputs, made once; read-only"""
        if self._inputs is None:
            self._inputs = finite_inputs(self.case)
        return self._inputs


def finite_inputs(case):
    """case.make() with `plant` a no-op (a module global of nonfinite_util, looked up when make() calls it)"""
    saved, nu.plant = nu.plant, lambda t, index, value: t
    try:
        return case.make()
    finally:
        nu.plant = saved


_DTYPE_TOKENS = ("f32", "f16", "bf16")


def row_key(case):
    """(row, dtype name) of a non-finite case: its name up to the dtype token; the FC layer's cases (float32 only) have
    none and are told apart by k and mode, their first three tokens"""
    tokens = case.name.split("-")
    at = [i for i, tok in enumerate(tokens) if tok in _DTYPE_TOKENS]
    if not at:
        return "-".join(tokens[:3]), "f32"
    return "-".join(tokens[:at[0]]), tokens[at[0]]


def collapse(cases):
    """one case per distinct (op, row, dtype), the first of each"""
    seen, out = set(), []
    for case in cases:
        key = (case.op,) + row_key(case)
        if key not in seen:
            seen.add(key)
            out.append((key, case))
    return out


NO_BACKWARD = ("VGG19Features", "fc_layer")      # forward only / both halves called through the C ABI, not the engine

# rows of the non-finite list that already are the vector-friendly shape of their op: name prefix -> (guard, condition)
_COSINE_FAST = ("csrc/max_cosine.hip:340, csrc/max_cosine.hip:641",
                lambda inp: inp["source"].size(1) % 32 == 0 and inp["source"].size(2) % 8 == 0 and inp["target"].size(2) % 8 == 0)


def _rows_of(cases, friendly=False, guard=None, holds=None):
    rows = []
    for (op, row, dname), case in collapse(cases):
        name = "%s-%s%s" % (row, dname, "-friendly" if friendly else "")
        # the FC layer's arithmetic mode has a dispatch-trace id of its own: the row asserts that it ran
        path = ("PATH_FC_FWD_MODE" + row[-1], "PATH_FC_BWD_MODE" + row[-1]) if op == "fc_layer" else None
        rows.append(Row(name, case, nu.DTYPES[dname], friendly, guard, holds, path, autograd=op not in NO_BACKWARD))
        if not friendly and row == "max_cosine-fast":
            rows[-1].friendly, (rows[-1].guard, rows[-1].holds) = True, _COSINE_FAST
    return rows


def ragged_rows():
    """the shapes of the non-finite list: odd sizes, ragged tiles (and max cosine's FAST shape, which it has already)"""
    return _rows_of(nu.all_cases())


def _plane4(key):
    """W and H W multiples of 4 elements of 4 bytes, of 8 of 2 bytes: the rows and planes of an aligned tensor start on 16"""
    def holds(inp):
        t = inp[key]
        per = 16 // t.element_size()
        return t.size(-1) % per == 0 and (t.size(-1) * t.size(-2)) % per == 0
    return holds


def fold_rows(H, W, positions=352):
    """fc_fold_rows of csrc/fc_sample.hip (kFoldPos = 352): the rows R a workgroup of the streaming fold takes"""
    import math
    maxr = max(1, min(H, positions // W))
    for m in (32, 4):
        step = m // math.gcd(W, m)
        if step <= maxr:
            return maxr // step * step
    return maxr


def _fold_vectors(c):
    return c["C"] % 4 == 0 and (c["H"] * c["W"]) % 4 == 0 and (fold_rows(c["H"], c["W"]) * c["W"]) % 4 == 0


def friendly_rows():
    """The smallest shapes at which the ALIGNED call satisfies the shape half of the op's guard (the file:line beside each),
    so that the pointer's phase decides the path.  Ops whose kernels test no pointer (the implicit-GEMM convolutions, the 1x1
    convolution, the max pool, the affine loss, the correctness map, the flow warp) have no such shape."""
    rows = []
    # planes staged and flushed as float4 (csrc/lds_plane.h:162, :190); BlockExtractor's forward reads rows as float4 when
    # Ws % 4 == 0 (csrc/be_fwd_wrow.h:52, csrc/be_fwd_pix.h:99) and stores V outputs when Wo % V == 0 (block_extractor.hip:237)
    rows += _rows_of(nu.scatter_cases((2, 8, 20, 16)), True, "csrc/lds_plane.h:162, csrc/lds_plane.h:190, csrc/be_fwd_wrow.h:52, "
                     "csrc/be_fwd_pix.h:99, csrc/block_extractor.hip:237", _plane4("src"))
    # whole strips of 4 (2) pixels: W % px == 0 (csrc/head_conv3x3.hip:532, called with px 4 and 2 at :559, :591, :595)
    heads = [("head_conv3x3-heads", ((2, 20, 8, 16), 6, (None,) * 4 + ("sigmoid",) * 2, 4), "zeros", None),
             ("head_conv3x3-output", ((2, 3, 4, 8), 3, "tanh", None), "reflect", 0.1)]
    rows += _rows_of(nu.head_conv_cases(heads), True, "csrc/head_conv3x3.hip:532", lambda inp: inp["x"].size(3) % 4 == 0)
    # no head and no tail: N a multiple of the 16-byte vector (csrc/instance_norm.hip:76)
    rows += _rows_of(nu.instance_norm_cases(((2, 5, 4, 8),)), True, "csrc/instance_norm.hip:76", _plane4("x"))
    # whole 16-byte segments per row: N % seg_elems == 0 (csrc/gram_l1.hip:429); rows of D read as float4 when C % 4 == 0 (:310)
    rows += _rows_of(nu.gram_cases((2, 40, 8, 8)), True, "csrc/gram_l1.hip:429, csrc/gram_l1.hip:310",
                     lambda inp: (inp["x"].size(2) * inp["x"].size(3)) % 8 == 0 and inp["x"].size(1) % 4 == 0)
    # the FC layer's fold of the padded data gradients: 16-byte streams when C % 4 == 0, float4 stores of the gradient when H W
    # and R W are multiples of 4 and the gradient is on 16 (csrc/fc_sample.hip:1114, :1117, :1122); max |x| reads float4 where
    # the map is on 16 (csrc/fc_gemm.hip:111)
    fc = [(shape, mode) for shape in ((5, 3, 16, 8, 6), (3, 3, 16, 8, 6)) for mode in (5, 4)]
    rows += _rows_of(nu.fc_layer_cases(fc), True, "csrc/fc_sample.hip:1114, csrc/fc_sample.hip:1117, csrc/fc_sample.hip:1122, "
                     "csrc/fc_gemm.hip:111", _fold_vectors)
    # the transposed convolution's pair stores (csrc/conv_igemm.h:318): Wout = 2 W is even for every W, the ragged row is it
    return rows


# ---- the ops the non-finite list lacks -------------------------------------------------------------------------------------------
ADDED_OPS = ("LocalAttnAggregateFunction", "LocalAttnReshape", "MaskBlendFunction", "spectral_normalize", "ExtractorAttn",
             "instance_norm_abi")
AGGREGATE_SHAPES = [(3, (2, 16, 12, 10)), (5, (2, 8, 11, 9))]       # H W = 120: patch_mfma.hip:472's g_vec holds; 99: it does not
RESHAPE_SHAPE = (3, (3, 17, 9))                                    # tests/test_f16_gpu.py's


def aggregate_rows():
    """softmax + aggregate, forward and backward, against the float64 composition avg_pool(pixel_shuffle(softmax(logits)) x
    block_extractor(source, flow)); the bars of tests/test_gpu_parity.py (float32: 2e-6 / 1e-5 of max(1, top); bfloat16:
    2^-8 / 2^-7 of the top) and tests/test_f16_gpu.py (float16: 2^-8 of the top)"""
    import torch.nn.functional as F
    from oracle import cpu_modules
    from util import make_flow, randn
    rows = []
    for k, shape in AGGREGATE_SHAPES:
        B, C, H, W = shape
        for dname in ("f32", "f16", "bf16"):
            dtype = nu.DTYPES[dname]

            def make(k=k, shape=shape, dtype=dtype):
                B, C, H, W = shape
                return {"s": randn(shape, seed=1).to(dtype), "f": make_flow("coherent", B, H, W, seed=3).to(dtype),
                        "lg": randn((B, k * k, H, W), seed=5).to(dtype), "up": randn(shape, seed=4).to(dtype)}

            def oracle(inp, k=k, dtype=dtype):
                s, f, lg = (inp[n].double().requires_grad_() for n in ("s", "f", "lg"))
                attn = torch.softmax(lg, 1)
                out = F.avg_pool2d(F.pixel_shuffle(attn, k) * cpu_modules._BlockExtractorCPU.apply(s, f, k), k, k)
                gs, gf, gl = torch.autograd.grad(out, (s, f, lg), inp["up"].double())
                fwd, bwd = (2e-6, 1e-5) if dtype == torch.float32 else (2.0 ** -8, 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -8)
                size = nu._scale if dtype == torch.float32 else nu._top
                return {"y": nu.Quantity(out, fwd * size(out.detach())), "y_attn": nu.Quantity(attn, fwd * size(attn.detach())),
                        "gs": nu.Quantity(gs, bwd * size(gs)), "gf": nu.Quantity(gf, bwd * size(gf)),
                        "gl": nu.Quantity(gl, bwd * size(gl))}

            def run(gfla, inp, k=k):
                from global_flow_local_attention_amd.extractor_attn import LocalAttnAggregateFunction
                s, f, lg = nu._leaf(inp["s"]), nu._leaf(inp["f"]), nu._leaf(inp["lg"])
                out, attn = LocalAttnAggregateFunction.apply(s, f, lg, k, True)
                out.backward(nu.to_dev(inp["up"]))
                return {"y": out, "y_attn": attn, "gs": s.grad, "gf": f.grad, "gl": lg.grad}
            case = nu.Case("aggregate-k%d-%s" % (k, dname), "LocalAttnAggregateFunction", None, make, oracle, run, None)
            vec = (H * W) % 4 == 0 and dname == "f32"
            rows.append(Row(case.name + ("-friendly" if vec else ""), case, dtype, vec, "csrc/patch_mfma.hip:472" if vec else None,
                            (lambda inp: (inp["s"].size(2) * inp["s"].size(3)) % 4 == 0) if vec else None))
    return rows


def reshape_rows():
    """LocalAttnReshape, bit-exact against pixel_shuffle, and its backward against pixel_unshuffle"""
    import torch.nn.functional as F
    from util import randn
    k, (B, H, W) = RESHAPE_SHAPE
    rows = []
    for dname in ("f32", "f16"):
        dtype = nu.DTYPES[dname]

        def make(dtype=dtype):
            return {"x": (randn((B, k * k, H, W), seed=60) * 100).to(dtype), "up": (randn((B, 1, k * H, k * W), seed=61) * 100).to(dtype)}

        def oracle(inp):
            return {"y": nu.Quantity(F.pixel_shuffle(inp["x"].double(), k)), "gx": nu.Quantity(F.pixel_unshuffle(inp["up"].double(), k))}

        def run(gfla, inp):
            x = nu._leaf(inp["x"])
            out = gfla.LocalAttnReshape()(x, k)
            out.backward(nu.to_dev(inp["up"]))
            return {"y": out, "gx": x.grad}
        case = nu.Case("local_attn_reshape-%s" % dname, "LocalAttnReshape", None, make, oracle, run, None)
        rows.append(Row(case.name, case, dtype))
    return rows


BLEND_SHAPE = (2, 20, 9, 7)                                        # tests/test_face_step_gpu.py's first
_BLEND_LEAVES = ("out", "attn_p", "attn_r", "mask_p", "mask_r")


def mask_blend_rows():
    """The mask blend of face_step.py: out (1 - m_p) + attn_p m_p + out (1 - m_r) + attn_r m_r.  The bars of
    tests/test_face_step_gpu.py: the forward as exact as the op-by-op torch expression in the same dtype (bar 0 under the
    floor that check() raises to that expression's own error on the GPU), the five gradients 1e-5 (16-bit: 2^-6) of the
    largest entry"""
    from util import rand, randn
    B, C, H, W = BLEND_SHAPE

    def expression(out, a_p, a_r, m_p, m_r):
        return (out * (1 - m_p) + a_p * m_p) + (out * (1 - m_r) + a_r * m_r)
    rows = []
    for dname in ("f32", "bf16"):
        dtype = nu.DTYPES[dname]

        def make(dtype=dtype):
            inp = {n: randn(BLEND_SHAPE, seed=i + 1).to(dtype) for i, n in enumerate(_BLEND_LEAVES[:3])}
            inp.update({"mask_p": rand((B, 1, H, W), seed=4).to(dtype), "mask_r": rand((B, 1, H, W), seed=5).to(dtype),
                        "up": randn(BLEND_SHAPE, seed=6).to(dtype)})
            return inp

        def oracle(inp, dtype=dtype):
            leaves = [inp[n].double().requires_grad_() for n in _BLEND_LEAVES]
            want = expression(*leaves)
            grads = torch.autograd.grad(want, leaves, inp["up"].double())
            tol = 1e-5 if dtype == torch.float32 else 2.0 ** -6
            out = {"y": nu.Quantity(want, 0.0, floor=dtype)}
            out.update({"g_" + n: nu.Quantity(g, tol * nu._top(g)) for n, g in zip(_BLEND_LEAVES, grads)})
            return out

        def evaluate(fn, inp):
            leaves = [nu._leaf(inp[n]) for n in _BLEND_LEAVES]
            y = fn(*leaves)
            y.backward(nu.to_dev(inp["up"]))
            got = {"y": y}
            got.update({"g_" + n: t.grad for n, t in zip(_BLEND_LEAVES, leaves)})
            return got

        def run(gfla, inp, evaluate=evaluate):
            return evaluate(gfla.MaskBlendFunction.apply, inp)

        def composition(gfla, inp, evaluate=evaluate):
            return evaluate(expression, inp)
        case = nu.Case("mask_blend-%s" % dname, "MaskBlendFunction", None, make, oracle, run, None, composition)
        rows.append(Row(case.name, case, dtype))
    return rows


def spectral_norm_rows():
    """The batched spectral norm: three matrices in one call, one power iteration, forward and backward.  u and v are updated
    in place.  The bar of tests/test_spectral_norm_gpu.py: 4 x the distance of torch's own float32 hook from the float64
    truth on the same inputs and device, relative to the quantity's largest entry.  Every matrix has a multiple of four
    elements, so the aligned call takes the float4 branches (csrc/spectral_norm.hip:161, :186, :243); the ragged row has a
    matrix of 15 elements in front, so that the next one starts off a 16-byte boundary in the batch's flat buffers and the
    scalar loads and the n < 4 tails run under red zones as well."""
    import discriminator_util as du
    return [_spectral_row(du, "spectral_normalize-f32-friendly", du.MATRICES[1:4], True),
            _spectral_row(du, "spectral_normalize-f32", ((3, 5),) + du.MATRICES[2:4], False)]


def _spectral_row(du, name, shapes, friendly):
    def make():
        inp = {}
        for i, (R, K) in enumerate(shapes):
            inp["w%d" % i], inp["u%d" % i], inp["v%d" % i], inp["g%d" % i] = du.matrix_inputs(R, K, seed=R + K)
        return inp

    def oracle(inp):
        device = nu.DEV if torch.cuda.is_available() else "cpu"
        out = {}
        for i in range(len(shapes)):
            args = [inp[n + str(i)] for n in "wuvg"]
            want, base = du.truth64(*args, 1), du.hook_float32(*args, 1, device)
            for q in ("w_sn", "u", "v", "sigma", "grad_w"):
                measured = du.distance(base[q], want[q])
                assert 0 < measured < 1e-4, (q, measured)             # a broken baseline cannot widen the bar
                out["%s%d" % (q, i)] = nu.Quantity(want[q], 4 * measured * want[q].abs().max().item(), batched=False)
        return out

    def run(gfla, inp):
        n = len(shapes)
        inout = getattr(nu.to_dev, "inout", nu.to_dev)
        ws = [nu._leaf(inp["w%d" % i]) for i in range(n)]
        us, vs = [inout(inp["u%d" % i].clone()) for i in range(n)], [inout(inp["v%d" % i].clone()) for i in range(n)]
        outs = gfla.spectral_normalize(ws, us, vs, power_iterations=1)
        sigma = outs[0].grad_fn.sigma
        torch.autograd.backward(list(outs), [nu.to_dev(inp["g%d" % i]) for i in range(n)])
        got = {}
        for i in range(n):
            got.update({"w_sn%d" % i: outs[i], "u%d" % i: us[i], "v%d" % i: vs[i], "sigma%d" % i: sigma[i:i + 1], "grad_w%d" % i: ws[i].grad})
        return got
    case = nu.Case(name, "spectral_normalize", None, make, oracle, run, None)
    if not friendly:
        return Row(name, case, torch.float32)
    return Row(name, case, torch.float32, True, "csrc/spectral_norm.hip:161, csrc/spectral_norm.hip:186, csrc/spectral_norm.hip:243",
               lambda inp: all(inp["w%d" % i].numel() % 4 == 0 for i in range(len(shapes))))


# ---- the whole fused float32 ExtractorAttn, the op the benchmark runs -----------------------------------------------------------
# (k, (B, C, H, W), FC arithmetic modes: None = the library's own).  C = 16, H W = 120: the fold's vector forms
# (csrc/fc_sample.hip:1114) and patch_mfma.hip:472's g_vec hold for the aligned call; C = 8, H W = 99: they do not
EXTRACTOR_SHAPES = [(3, (2, 16, 12, 10), (None, 4)), (5, (2, 8, 11, 9), (None,))]


def extractor_attn_rows():
    """ExtractorAttn (FC layers, softmax, aggregation), forward and backward, float32, against the float64 host module
    (oracle.cpu_modules.ExtractorAttnCPU); the bar of smoke() and of the module tests: 1e-4 of max(1, the largest entry).
    The gradients of source, flow and logits are views of ONE float32 allocation of the wrapper (extractor_attn._zeros_f32),
    which the mode shifts like any other: the kernels accumulate into gradients at a phase.  Inputs: the first seed whose
    hidden activations all stay clear of LeakyReLU's kink, as smoke() picks it."""
    from oracle import cpu_modules
    from util import make_flow, randn

    def host_module(k, C, state=None, seed=None):
        if seed is not None:
            torch.manual_seed(seed)
        ref = cpu_modules.ExtractorAttnCPU(C, k, torch.nn.LeakyReLU(0.1), softmax=True)
        if state is not None:
            ref.load_state_dict(state)
        return ref
    rows = []
    for k, shape, modes in EXTRACTOR_SHAPES:
        B, C, H, W = shape

        def make(k=k, shape=shape):
            B, C, H, W = shape
            for seed in range(20):
                ref = host_module(k, C, seed=seed)
                inp = {"s": randn(shape, seed=10 * seed + 1), "t": randn(shape, seed=10 * seed + 2),
                       "f": make_flow("coherent", B, H, W, seed=10 * seed + 3), "up": randn(shape, seed=10 * seed + 4)}
                hidden = []
                hook = ref.fully_connect_layer[0].register_forward_hook(lambda m, i, o: hidden.append(o.detach()))
                with torch.no_grad():
                    ref(inp["s"], inp["t"], inp["f"])
                hook.remove()
                if hidden[0].abs().min().item() > 1e-4:
                    break
            inp.update({"param/" + n: p.detach().clone() for n, p in ref.state_dict().items()})
            return inp

        def state_of(inp, dtype):
            return {n[len("param/"):]: t.to(dtype) for n, t in inp.items() if n.startswith("param/")}

        def oracle(inp, k=k, C=C, state_of=state_of):
            ref = host_module(k, C, state_of(inp, torch.float64)).double()
            leaves = [inp[n].double().requires_grad_() for n in ("s", "t", "f")]
            out = ref(*leaves)
            out.backward(inp["up"].double())
            want = {"y": out.detach(), "g_s": leaves[0].grad, "g_t": leaves[1].grad, "g_f": leaves[2].grad}
            want.update({"g_" + n: p.grad for n, p in ref.named_parameters()})
            return {n: nu.Quantity(v, 1e-4 * nu._scale(v), batched=not n.startswith("g_fully")) for n, v in want.items()}
        for mode in modes:
            def run(gfla, inp, k=k, C=C, mode=mode, state_of=state_of):
                mod = gfla.ExtractorAttn(C, k, torch.nn.LeakyReLU(0.1), softmax=True)
                mod.load_state_dict(state_of(inp, torch.float32))
                mod = mod.to(nu.DEV)
                if mode is not None:
                    mod.fc_mode = mode
                leaves = [nu._leaf(inp[n]) for n in ("s", "t", "f")]
                out = mod(*leaves)
                out.backward(nu.to_dev(inp["up"]))
                got = {"y": out, "g_s": leaves[0].grad, "g_t": leaves[1].grad, "g_f": leaves[2].grad}
                got.update({"g_" + n: p.grad for n, p in mod.named_parameters()})
                return got
            name = "extractor_attn-k%d-%s-f32" % (k, "mode%d" % mode if mode is not None else "default")
            case = nu.Case(name, "ExtractorAttn", None, make, oracle, run, None)
            vec = C % 4 == 0 and (H * W) % 4 == 0
            rows.append(Row(name + ("-friendly" if vec else ""), case, torch.float32, vec,
                            "csrc/fc_sample.hip:1114, csrc/patch_mfma.hip:472" if vec else None,
                            (lambda inp: inp["s"].size(1) % 4 == 0 and (inp["s"].size(2) * inp["s"].size(3)) % 4 == 0) if vec else None,
                            # (k 3 at this shape resolves to mode 5, as smoke() asserts of it)
                            tuple("PATH_FC_%s_MODE%d" % (d, mode or 5) for d in ("FWD", "BWD")) if k == 3 else None))
    return rows


# ---- instance norm through the C ABI: x itself at a phase -----------------------------------------------------------------------
def instance_norm_abi_rows():
    """gfla_instance_norm_fwd / _bwd called as a C caller would, with x, dy, y and dx wherever the placement puts them: the
    Python wrapper copies an offset x onto a 16-byte boundary (instance_norm._aligned), so only here does a span have a head
    (csrc/instance_norm.hip:76).  Cases, oracle and bars are nonfinite_util.instance_norm_cases'."""
    import instance_norm_util as iu
    rows = []
    for label, friendly in (("small", False), ((2, 5, 4, 8), True)):
        for (op, row, dname), case in collapse(nu.instance_norm_cases((label,))):
            def run(gfla, inp):
                from global_flow_local_attention_amd import _lib
                x, up = nu.to_dev(inp["x"]), nu.to_dev(inp["up"].to(inp["x"].dtype))
                w, b = nu.to_dev(inp["w"].float()), nu.to_dev(inp["b"].float())
                B, C, H, W = x.shape
                sfx, p = _lib.suffix(x, "instance_norm"), _lib.ptr
                y, dx = torch.empty_like(x), torch.empty_like(x)
                mean, rstd, dw, db = (torch.empty(n, dtype=torch.float32, device=x.device) for n in (B * C, B * C, C, C))
                ws = _lib.workspace("gfla_instance_norm_workspace_bytes", x, B, C, H, W, x.element_size(), what="instance_norm")
                _lib.call("gfla_instance_norm_fwd_" + sfx, x, p(x), p(w), p(b), p(y), p(mean), p(rstd), p(ws), B, C, H, W,
                          float(iu.EPS), 0.1, 1)
                _lib.call("gfla_instance_norm_bwd_" + sfx, x, p(x), p(up), p(w), p(b), p(mean), p(rstd), p(dx), p(dw), p(db),
                          p(ws), B, C, H, W, 0.1, 1)
                torch.cuda.synchronize()
                return {"y": y, "gx": dx, "gw": dw, "gb": db}
            abi = nu.Case(case.name.replace("instance_norm_act", "instance_norm_abi"), "instance_norm_abi", None, case.make,
                          case.oracle, run, None, case.composition)
            name = "%s-%s%s" % (row.replace("instance_norm_act", "instance_norm_abi"), dname, "-friendly" if friendly else "")
            rows.append(Row(name, abi, nu.DTYPES[dname], friendly, "csrc/instance_norm.hip:76" if friendly else None,
                            _plane4("x") if friendly else None, autograd=False))
    return rows


# ---- what may differ from the aligned run, what is made by torch, and what may be refused ---------------------------------------
_ATOMICS = "float atomics whose order is not fixed: "
_COSINE_BWD = ("correctness.py:66 the backward is a torch composition (gather, norm, sum, scatter_add_): torch's reductions vectorise "
               "by the pointer's phase and its scatter_add_ uses atomics")
# (op, quantity) -> the reason, read from the code, why the placed result need not be BIT-equal to the aligned one.  Such a
# quantity is still held to its bar against the float64 oracle, and its zones are checked.  Only what was MEASURED unequal on
# an MI355X stands here; nondeterminism that shows between two aligned runs is exempt by that measurement alone.
_NORM_SPAN = ("instance_norm.hip:76 the head / vectors / tail split of a span follows x's address, so the elements a thread sums "
              "regroup with x's phase, and the sums feed every output")
EXEMPT = {
    ("instance_norm_abi", "y"): _NORM_SPAN, ("instance_norm_abi", "gx"): _NORM_SPAN, ("instance_norm_abi", "gw"): _NORM_SPAN,
    ("instance_norm_abi", "gb"): _NORM_SPAN,
    ("max_cosine_similarity", "gs"): _COSINE_BWD, ("max_cosine_similarity", "gt"): _COSINE_BWD,
    ("LocalAttnAggregateFunction", "gf"): _ATOMICS + "local_attn_aggregate.hip:241, local_attn_aggregate.hip:811",
}

# (op, quantity, dtype name) -> why the checked result is made by a torch op (a cast of what the kernel wrote into a recorded
# buffer), not by a factory call the mode sees
_CAST = "a float32 sum the kernels wrote, rounded once to the storage type by torch: "
TORCH_MADE = {}
for _d in ("f32", "f16", "bf16"):
    TORCH_MADE[("max_cosine_similarity", "gs", _d)] = TORCH_MADE[("max_cosine_similarity", "gt", _d)] = _COSINE_BWD
for _d in ("f16", "bf16"):
    TORCH_MADE[("head_conv3x3", "gw", _d)] = TORCH_MADE[("head_conv3x3", "gb", _d)] = _CAST + "_conv_common.py:67"
    TORCH_MADE[("instance_norm_act", "gw", _d)] = TORCH_MADE[("instance_norm_act", "gb", _d)] = _CAST + "_conv_common.py:67"
    TORCH_MADE[("flow_warp", "gs", _d)] = _CAST + "flow_warp.py:89"
    TORCH_MADE[("BlockExtractor", "gf", _d)] = _CAST + "block_extractor.py:81"
    TORCH_MADE[("MaskBlendFunction", "g_mask_p", _d)] = TORCH_MADE[("MaskBlendFunction", "g_mask_r", _d)] = _CAST + "face_step.py:73"
    TORCH_MADE[("LocalAttnAggregateFunction", "gf", _d)] = _CAST + "extractor_attn.py:124"
    TORCH_MADE[("LocalAttnAggregateFunction", "gl", _d)] = _CAST + "extractor_attn.py:126"

# row name -> the sentence of include/gfla_hip.h that lets the MIXED placement end in _lib.Unsupported.  Empty: since the
# instance norm and the transposed convolution take any element-aligned pointer, no entry point states such a requirement
REFUSES = {}


def all_rows():
    return ragged_rows() + friendly_rows() + aggregate_rows() + reshape_rows() + mask_blend_rows() + spectral_norm_rows() + extractor_attn_rows() + \
        instance_norm_abi_rows()


def dtype_name(dtype):
    return next(name for name, d in nu.DTYPES.items() if d == dtype)
