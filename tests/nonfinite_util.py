"""Non-finite inputs: one check for every op ("Non-finite values").

A case names an op, its small seeded finite inputs (the input makers of the op's own *_util.py), one planted value (NaN,
+inf, -inf) and the tensor and element it goes into.  The oracle is the op's own torch composition evaluated on the HOST
in float64 on the same planted inputs; for every output and every gradient it gives the set P of non-finite elements.

    no laundering   every element of P is non-finite in the kernel's result
    containment     every element outside P is finite and within the op's EXISTING bar of the float64 oracle (the bar
                    functions of gen_conv_util, conv1x1_util, vgg_util, head_conv_util, ...: no tolerance of this file's)
    over-poisoning  allowed only where a Quantity says so (`allow`), and never outside the planted sample -- but for the
                    one documented deviation, which says so too (`batch_wide`: the FC layer's grad_source)
    bit equality    a Quantity without a bar (max pool) is compared exactly: equal values where finite, equal NaN masks

The case list is checked on the host alone by tests/test_nonfinite_cpu.py (every case discriminates, the planted element
is where the case says, two stand-ins that launder / over-poison are rejected) and run on the GPU by
tests/test_nonfinite_gpu.py."""
import math

import torch
import torch.nn.functional as F

import conv1x1_util as cu
import gen_conv_train_util as tu
import gen_conv_util as gu
import head_conv_util as hu
import instance_norm_util as iu
import vgg_util as vu

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
VALUE_NAMES = {"nan": NAN, "+inf": PINF, "-inf": NINF}
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DEV = "cuda:0"


class Quantity(object):
    """One output or gradient of the oracle.  want: float64 host tensor.  bar: elementwise tolerance (tensor or number;
    None: exact).  batched: dim 0 is the batch.  allow: bool mask of elements that may be non-finite although the
    oracle's are not (a documented over-poisoning), None: none.  floor: dtype of the `4 units in the last place of the
    largest entry` floor that the op's own test puts under its bar (None: the op's test has none); such a bar is also
    raised to the error of the torch composition in the same dtype on the GPU, where the case evaluates it.  scale: the
    magnitude the floor is taken at (None: the largest finite entry of `want`)."""

    def __init__(self, want, bar=None, batched=True, allow=None, floor=None, scale=None):
        self.want, self.bar, self.batched, self.allow, self.floor = want.detach().double().cpu(), bar, batched, allow, floor
        self.scale = scale
        self.batch_wide = False      # True: a documented DEVIATION whose allowance reaches the other samples


class Case(object):
    """name: the test id.  sample: the batch index the value is planted in (None: a parameter, or an op without a
    batch).  make() -> dict of host tensors in their storage types, the value planted.  oracle(inputs) -> {name:
    Quantity}, the first one the forward output.  run(gfla, inputs) -> {name: tensor} from the kernels.  composition
    (gfla, inputs) -> the same from the torch composition on the GPU (only for ops whose bar is that error), or None.
    where(inputs) -> bool: the planted element is where the name says."""

    def __init__(self, name, op, sample, make, oracle, run, where, composition=None):
        self.name, self.op, self.sample = name, op, sample
        self.make, self.oracle, self.run, self.where, self.composition = make, oracle, run, where, composition

    def __repr__(self):
        return self.name


def plant(t, index, value):
    t = t.clone()
    t[index] = value
    return t


def ulp(dtype, at):
    return 0.0 if at == 0 or not math.isfinite(at) else math.ldexp(torch.finfo(dtype).eps, math.frexp(at)[1] - 1)


def _others(q, sample):
    keep = torch.ones(q.want.size(0), dtype=torch.bool)
    keep[sample] = False
    return keep


def check(case, got, want, comp=None):
    """The four conditions of the module docstring for every Quantity; returns the printed report, raises AssertionError
    naming every quantity that breaks one."""
    lines, bad = [], []
    for name, q in want.items():
        assert got.get(name) is not None, "%s: no result for %s" % (case.name, name)
        g, w = got[name].detach().double().cpu(), q.want
        assert g.shape == w.shape, (case.name, name, tuple(g.shape), tuple(w.shape))
        P, nf = ~torch.isfinite(w), ~torch.isfinite(g)
        allow = torch.zeros_like(P) if q.allow is None else q.allow
        if q.allow is not None and q.batched and case.sample is not None and not q.batch_wide:
            assert not allow[_others(q, case.sample)].any(), "%s %s: an allowance outside the planted sample" % (case.name, name)
        laundered, over, ok = P & ~nf, nf & ~P & ~allow, ~P & ~nf
        if q.bar is None:
            wrong = (ok & (g != w)) | (P & (torch.isnan(g) != torch.isnan(w))) | (P & torch.isinf(w) & (g != w))
            worst = float(wrong.any())
        else:
            bar = torch.as_tensor(q.bar, dtype=torch.float64).expand_as(w).clone()
            if q.floor is not None:
                low = 4 * ulp(q.floor, q.scale if q.scale is not None else w[~P].abs().max().item() if (~P).any() else 0.0)
                if comp is not None and comp.get(name) is not None:
                    c = comp[name].detach().double().cpu()
                    held = ~P & torch.isfinite(c)
                    if held.any():
                        low = max(low, (c - w).abs()[held].max().item())
                bar = bar.clamp_min(low)
            err = (g - w).abs()
            wrong = ok & ~(err <= bar)
            ratio = (err / bar.clamp_min(1e-300))[ok]
            worst = ratio.max().item() if ratio.numel() else 0.0
        if q.batch_wide and q.batched and case.sample is not None:
            # the documented deviation reaches the other samples WHOLE: each of them is NaN throughout or finite and within
            # the bar throughout, never finite garbage next to NaN
            for b in range(w.size(0)):
                if b != case.sample and not (bool(nf[b].all()) or not bool(nf[b].any())):
                    wrong[b] = wrong[b] | ~nf[b]
        lines.append("%s %s: |P| %d of %d, laundered %d, over-poisoned %d (allowed %d), outside the bar %d, worst err/bar %.3f"
                     % (case.name, name, int(P.sum()), P.numel(), int(laundered.sum()), int(over.sum()),
                        int((nf & ~P & allow).sum()), int(wrong.sum()), worst))
        if laundered.any() or over.any() or wrong.any():
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, "\n".join(bad)
    return lines


def self_check(case, inputs, want):
    """What must hold of a case on the oracle alone, so that it can discriminate"""
    assert case.where(inputs), "%s: the planted element is not where the case says" % case.name
    # the forward outputs are the quantities named y...; a value planted in the upstream gradient shows in the gradients only
    upstream = "-upstream-" in case.name
    hit = [bool((~torch.isfinite(q.want)).any()) for name, q in want.items() if name.startswith("y") != upstream]
    assert any(hit), "%s: the %s of the oracle are finite everywhere" % (case.name, "gradients" if upstream else "forward outputs")
    if case.sample is not None:
        for name, q in want.items():
            if q.batched:
                assert torch.isfinite(q.want[_others(q, case.sample)]).all(), \
                    "%s %s: another sample is not finite in the oracle" % (case.name, name)
            elif q.bar is not None:
                assert torch.as_tensor(q.bar).numel() == 1 or torch.as_tensor(q.bar).shape == q.want.shape


def laundering_stand_in(want):
    return {name: torch.nan_to_num(q.want, nan=0.0, posinf=1.0, neginf=-1.0) for name, q in want.items()}


def over_poisoning_stand_in(case, want):
    """the oracle's values with one more sample set to NaN in the forward output"""
    out = {name: q.want.clone() for name, q in want.items()}
    name, q = next(iter(want.items()))
    other = (case.sample + 1) % q.want.size(0)
    out[name][other] = NAN
    return out


def to_dev(t):
    """Every host -> device move of the `run` functions goes through here (looked up at call time), so that
    tests/placement_util.py can put the device tensor where it wants it"""
    return t.to(DEV)


def _leaf(t, need=True, dtype=None):
    if t is None:
        return None
    t = t.detach().clone()
    if dtype is not None:
        t = t.to(dtype)
    return to_dev(t).requires_grad_(need)


def _grad(t):
    return None if t is None else t.grad


# ---- conv3x3_relu (csrc/conv3x3.hip on conv_igemm.h, kCvVggFwd / kCvVggBwd) -------------------------------------------------
RELU_SHAPE = (2, 5, 7, 6, 9)     # (B, Cin, Cout, H, W): tests/test_vgg19_gpu.py's smallest; one padded chunk, one ragged tile


def _relu_conv_oracle(dtype, shape):
    B, Cin, Cout, H, W = shape

    def oracle(inp):
        x, w, b, gy = (inp[k].double() for k in ("x", "w", "b", "gy"))
        xs = x.clone().requires_grad_()
        y = F.relu(F.conv2d(xs, w, b, padding=1))
        gx, = torch.autograd.grad(y, xs, gy)
        pre = F.conv2d(x, w, b, padding=1)
        S = F.conv2d(x.abs(), w.abs(), b.abs(), padding=1)
        bar_y = vu.conv_bar(S, y.detach(), 9 * Cin, dtype)
        # the data gradient's bar of tests/test_vgg19_gpu.py, S from |g| [y > 0] and |w|.  That test takes the mask from
        # the kernel's own y; here the oracle is the host's alone, so an output within the forward's bar of 0, whose mask
        # the kernel may set the other way, adds what it can move: |g| |w| through the same transposed convolution
        live = ((pre > 0) | torch.isnan(pre)).double()
        flip = (pre.abs() <= bar_y).double()
        Sg = F.conv_transpose2d(gy.abs() * live, w.abs(), padding=1)
        extra = F.conv_transpose2d(torch.nan_to_num(gy.abs() * flip, nan=0.0, posinf=0.0), w.abs().nan_to_num(0.0, 0.0, 0.0),
                                   padding=1)
        return {"y": Quantity(y, bar_y), "gx": Quantity(gx, vu.conv_bar(Sg, gx, 9 * Cout, dtype) + extra)}
    return oracle


def _relu_conv_run(gfla, inp):
    x = _leaf(inp["x"])
    y = gfla.conv3x3_relu(x, to_dev(inp["w"].float()), to_dev(inp["b"].float()))
    assert type(y.grad_fn).__name__ == "Conv3x3ReluFunctionBackward"
    y.backward(to_dev(inp["gy"]))
    return {"y": y, "gx": x.grad}


def relu_conv_cases(shape=RELU_SHAPE):
    B, Cin, Cout, H, W = shape
    spots = [("x", "interior", (0, 2, 3, 4), ("nan", "+inf", "-inf"), 0), ("x", "corner", (0, 1, 0, 0), ("nan", "+inf"), 0),
             ("x", "last-sample", (1, 4, 5, 8), ("nan",), 1), ("w", "weight", (3, 2, 1, 1), ("nan", "+inf"), None),
             ("b", "bias", (4,), ("nan", "+inf"), None)]      # (-inf in a bias: relu makes it 0, nothing is non-finite)
    cases = []
    for dname in ("f32", "f16", "bf16"):
        dtype = DTYPES[dname]
        for tensor, label, index, values, sample in spots:
            for vname in values if dname == "f32" else values[:1]:
                def make(tensor=tensor, index=index, vname=vname, dtype=dtype):
                    x, w, b, gy = vu.conv_inputs(shape, dtype, seed=sum(shape))
                    inp = {"x": x, "w": w, "b": b, "gy": gy}
                    inp[tensor] = plant(inp[tensor], index, VALUE_NAMES[vname])
                    return inp

                cases.append(Case("conv3x3_relu-%s-%s-%s" % (dname, label, vname), "conv3x3_relu", sample, make,
                                  _relu_conv_oracle(dtype, shape), _relu_conv_run,
                                  _spot_where(shape, tensor, label, index)))
    return cases


# ---- maxpool2x2 (csrc/maxpool2x2.hip): bit equality ------------------------------------------------------------------------
POOL_SHAPE = (2, 5, 7, 9)        # odd both ways: the last row and column are dropped, their gradient is zero
POOL_WINDOW = (2, 3)             # the window (output row, output column) the value goes into, in plane (sample, 3)


def pool_input(dtype, slot, sample=0, value=NAN, shape=POOL_SHAPE):
    """tests/test_vgg19_gpu.py's `odd` map with `value` in slot 0..3 (scan order) of one window"""
    x = torch.randn(shape, generator=torch.Generator().manual_seed(11)).to(dtype)
    oy, ox = POOL_WINDOW
    return plant(x, (sample, 3, 2 * oy + slot // 2, 2 * ox + slot % 2), value)


def _pool_oracle(inp):
    xs = inp["x"].double().requires_grad_()            # widening is exact
    y = F.max_pool2d(xs, kernel_size=2, stride=2)
    gx, = torch.autograd.grad(y, xs, inp["gy"].double())
    return {"y": Quantity(y), "gx": Quantity(gx)}


def _pool_run(gfla, inp):
    x = _leaf(inp["x"])
    y = gfla.maxpool2x2(x)
    assert type(y.grad_fn).__name__ == "MaxPool2x2FunctionBackward"
    y.backward(to_dev(inp["gy"]))
    return {"y": y, "gx": x.grad}


def pool_cases(shape=POOL_SHAPE):
    cases = []
    for dname in ("f32", "f16", "bf16"):
        dtype = DTYPES[dname]
        # (-inf never wins a window: nothing would be non-finite, so there is no such case)
        for slot, sample, vname in [(s, 0, "nan") for s in range(4)] + [(2, 1, "nan"), (1, 0, "+inf")]:
            if dname != "f32" and vname != "nan":
                continue

            def make(dtype=dtype, slot=slot, sample=sample, vname=vname):
                g = torch.randn((shape[0], shape[1], shape[2] // 2, shape[3] // 2),
                                generator=torch.Generator().manual_seed(5)).to(dtype)
                return {"x": pool_input(dtype, slot, sample, VALUE_NAMES[vname], shape), "gy": g + (g == 0).to(dtype)}

            def where(inp, slot=slot, sample=sample):
                hit = (~torch.isfinite(inp["x"])).nonzero()
                oy, ox = POOL_WINDOW
                return hit.shape[0] == 1 and tuple(hit[0].tolist()) == (sample, 3, 2 * oy + slot // 2, 2 * ox + slot % 2) \
                    and 2 * oy + 1 < shape[2] - 1 and 2 * ox + 1 < shape[3] - 1
            cases.append(Case("maxpool2x2-%s-slot%d-sample%d-%s" % (dname, slot, sample, vname), "maxpool2x2", sample, make,
                              _pool_oracle, _pool_run, where))
    return cases


# ---- conv3x3 / conv4x4_down / conv_transpose3x3_up with their gradients (csrc/gen_conv*.hip on conv_igemm.h) ---------------
GEN_ROWS = [  # (label, geometry, (B, Cin, Cout, H, W), options): Cin = 20 leaves a ragged last chunk of 4 channels
    ("conv3x3-zeros", gu.S1K3, (2, 20, 40, 9, 7), {}),
    ("conv3x3-reflect", gu.S1K3, (2, 20, 40, 9, 7), {"reflect": True, "slope": 0.1, "add": True}),
    ("conv4x4_down", gu.S2K4, (2, 20, 40, 9, 7), {"slope": 0.1, "add": True}),
    ("conv_transpose3x3_up", gu.T2K3, (2, 20, 40, 5, 4), {"add": True}),
]


def _gen_call(gfla, geometry, x, w, b, reflect, slope, add):
    if geometry == gu.S1K3:
        return gfla.conv3x3(x, w, b, padding="reflect" if reflect else "zeros", pre_slope=slope, add=add, grad="kernels")
    if geometry == gu.S2K4:
        return gfla.conv4x4_down(x, w, b, pre_slope=slope, add=add, grad="kernels")
    return gfla.conv_transpose3x3_up(x, w, b, add=add, pre_slope=slope, grad="kernels")


def halo_ring(shape4, channel):
    """The documented over-poisoning of a non-finite WEIGHT tap in a padded convolution's data gradient (DESIGN.md,
    "Non-finite values"): the kernels multiply the halo's zeros like any pixel, and 0 x NaN = NaN, so the border pixels of
    the tap's input channel whose tap lies in the padding come out NaN as well (torch's own forward does the same with
    its padding; its backward happens not to).  Every sample has them: the value sits in a parameter."""
    allow = torch.zeros(shape4, dtype=torch.bool)
    allow[:, channel, 0], allow[:, channel, -1], allow[:, channel, :, 0], allow[:, channel, :, -1] = True, True, True, True
    return allow


def _gen_oracle(geometry, shape, opts, dtype, weight_at=None):
    B, Cin, Cout, H, W = shape
    reflect, slope = bool(opts.get("reflect")), opts.get("slope")

    def oracle(inp):
        x, w, b, add, g = (inp.get(k) for k in ("x", "w", "b", "add", "gy"))
        y, S = gu.ref64(geometry, x, w, b, reflect, slope, add)
        (gx, gw, gb), (Sx, Sw, Sb) = tu.grads64(geometry, x, w, b, g, reflect, slope)
        Kw = tu.weight_reduction_length(geometry, shape)
        out = {"y": Quantity(y, gu.bar(S, y, gu.reduction_length(geometry, Cin), dtype, add is not None)),
               "gx": Quantity(gx, gu.bar(Sx, gx, tu.data_reduction_length(geometry, Cout), dtype, False)),
               "gw": Quantity(gw, gu.bar(Sw, gw, Kw, torch.float32, False), batched=False),
               "gb": Quantity(gb, gu.bar(Sb, gb, Kw, torch.float32, False), batched=False)}
        if add is not None:
            out["gadd"] = Quantity(g.double())          # the addend's gradient is grad_y itself
        if weight_at is not None and geometry != gu.T2K3:     # (the transposed convolution's gradient has no halo)
            out["gx"].allow = halo_ring((B, Cin, H, W), weight_at[1])
        return out
    return oracle


def _gen_run(geometry, opts):
    reflect, slope = bool(opts.get("reflect")), opts.get("slope")

    def run(gfla, inp):
        x, w, b, add = _leaf(inp["x"]), _leaf(inp["w"], dtype=torch.float32), _leaf(inp["b"], dtype=torch.float32), \
            _leaf(inp.get("add"))
        y = _gen_call(gfla, geometry, x, w, b, reflect, slope, add)
        assert type(y.grad_fn).__name__ == "GenConvFunctionBackward"
        y.backward(to_dev(inp["gy"]))
        out = {"y": y, "gx": x.grad, "gw": w.grad, "gb": b.grad}
        if add is not None:
            out["gadd"] = add.grad
        return out
    return run


def _conv_spots(shape, out_hw, border):
    """(tensor, label, index, values, sample) of the convolution families: an interior pixel, a border pixel (row 0:
    reflect-padded where the op pads by reflection), the last channel of the ragged last chunk, the last sample, one weight,
    one bias and one upstream-gradient element"""
    B, Cin, Cout, H, W = shape
    return [("x", "interior", (0, 3, H // 2, W // 2), ("nan", "+inf", "-inf"), 0), ("x", border, (0, 3, 0, W // 2), ("nan", "+inf", "-inf"), 0),
            ("x", "last-chunk", (0, Cin - 1, H // 2, W // 2), ("nan", "+inf", "-inf"), 0), ("x", "last-sample", (B - 1, 3, H // 2, W // 2), ("nan",), B - 1),
            ("w", "weight", (5, 7, 1, 2) if Cout > 7 else (0, 1, 1, 2), ("nan", "+inf"), None), ("b", "bias", (min(6, Cout - 1),), ("nan",), None),
            ("gy", "upstream", (0, min(5, Cout - 1), out_hw[0] // 2, out_hw[1] // 2), ("nan", "+inf"), 0)]


def _spot_where(shape, tensor, label, index):
    B, Cin, Cout, H, W = shape

    def where(inp):
        hit = ~torch.isfinite(inp[tensor])
        if label == "interior":
            at = 0 < index[-2] < H - 1 and 0 < index[-1] < W - 1
        elif label in ("border", "reflect-border"):
            at = index[-2] == 0
        elif label == "corner":
            at = index[-2:] == (0, 0)
        elif label == "last-chunk":                     # chunks of 8 (float32) or 16 (16-bit) channels: the last one is ragged
            at = index[1] == Cin - 1 and Cin % 8 != 0 and Cin % 16 != 0
        elif label == "last-sample":
            at = index[0] == B - 1 and B > 1
        else:
            at = True
        return int(hit.sum()) == 1 and bool(hit[index]) and at
    return where


def gen_conv_cases(rows=GEN_ROWS):
    cases = []
    for label, geometry, shape, opts in rows:
        out_hw = gu.out_size(geometry, shape[3], shape[4])
        for dname in ("f32", "bf16") if geometry != gu.S2K4 else ("f32", "f16"):
            dtype = DTYPES[dname]
            for tensor, spot, index, values, sample in _conv_spots(shape, out_hw, "reflect-border" if opts.get("reflect") else "border"):
                if dname != "f32" and spot not in ("interior", "weight", "upstream"):
                    continue
                for vname in values if dname == "f32" else values[:1]:
                    def make(geometry=geometry, shape=shape, opts=opts, dtype=dtype, tensor=tensor, index=index, vname=vname):
                        x, w, b, add = gu.conv_inputs(geometry, shape, dtype, seed=sum(shape) + geometry, with_add=bool(opts.get("add")))
                        inp = {"x": x, "w": w, "b": b, "gy": tu.upstream(geometry, shape, dtype, seed=sum(shape))}
                        if add is not None:
                            inp["add"] = add
                        inp[tensor] = plant(inp[tensor], index, VALUE_NAMES[vname])
                        return inp
                    cases.append(Case("%s-%s-%s-%s" % (label, dname, spot, vname), label.split("-")[0], sample, make,
                                      _gen_oracle(geometry, shape, opts, dtype, index if tensor == "w" else None),
                                      _gen_run(geometry, opts),
                                      _spot_where(shape, tensor, spot, index)))
    return cases


# ---- conv1x1, pool 1 and pool 2 (csrc/conv1x1.hip) -------------------------------------------------------------------------
C11_ROWS = [("conv1x1-pool1", (2, 20, 40, 9, 7), {"slope": 0.1}), ("conv1x1-pool2", (2, 20, 40, 7, 5), {"pool": 2})]


def conv1x1_cases(rows=C11_ROWS):
    cases = []
    for label, shape, opts in rows:
        pool, slope = opts.get("pool", 1), opts.get("slope")
        B, Cin, Cout, H, W = shape
        out_hw = cu.out_size(H, W, pool)
        for dname in ("f32", "f16"):
            dtype = DTYPES[dname]
            for tensor, spot, index, values, sample in _conv_spots(shape, out_hw, "border"):
                if tensor == "w":
                    index = index[:2] + (0, 0)
                if dname != "f32" and spot not in ("interior", "weight", "upstream"):
                    continue
                for vname in values if dname == "f32" else values[:1]:
                    def make(shape=shape, opts=opts, dname=dname, tensor=tensor, index=index, vname=vname):
                        x, w, b, g = cu.inputs(dname, shape, cu.key(opts))
                        inp = {"x": x, "w": w, "b": b, "gy": g}
                        inp[tensor] = plant(inp[tensor], index, VALUE_NAMES[vname])
                        return inp

                    def oracle(inp, shape=shape, pool=pool, slope=slope, dtype=dtype):
                        t = cu.truth_of(inp["x"], inp["w"], inp["b"], inp["gy"], pool, slope)
                        bars = cu.bars_of(t, dtype, shape, pool)
                        return {"y": Quantity(t["y"], bars["y"]), "gx": Quantity(t["gx"], bars["gx"]),
                                "gw": Quantity(t["gw"], bars["gw"], batched=False), "gb": Quantity(t["gb"], bars["gb"], batched=False)}

                    def run(gfla, inp, pool=pool, slope=slope):
                        x, w, b = _leaf(inp["x"]), _leaf(inp["w"]), _leaf(inp["b"])
                        y = gfla.conv1x1(x, w, b, pre_slope=slope, pool=pool, grad="kernels")
                        assert type(y.grad_fn).__name__ == "Conv1x1FunctionBackward"
                        y.backward(to_dev(inp["gy"]))
                        return {"y": y, "gx": x.grad, "gw": w.grad, "gb": b.grad}
                    cases.append(Case("%s-%s-%s-%s" % (label, dname, spot, vname), "conv1x1", sample, make, oracle, run,
                                      _spot_where(shape, tensor, spot, index)))
    return cases


# ---- head_conv3x3: identity, tanh and sigmoid channels (csrc/head_conv3x3.hip) -------------------------------------------------
HEAD_ROWS = [  # (label, (shape, Cout, post, split), padding, pre_slope): the face heads and the image output of the goldens
    ("head_conv3x3-heads", ((2, 20, 9, 13), 6, (None,) * 4 + ("sigmoid",) * 2, 4), "zeros", None),
    ("head_conv3x3-output", ((2, 3, 3, 5), 3, "tanh", None), "reflect", 0.1),
]


def head_conv_cases(rows=HEAD_ROWS):
    cases = []
    for label, (shape4, cout, post, split), padding, slope in rows:
        B, Cin, H, W = shape4
        shape = (B, Cin, cout, H, W)
        spots = [("x", "interior", (0, Cin - 1, H // 2, W // 2), ("nan", "+inf", "-inf"), 0),
                 ("x", "reflect-border" if padding == "reflect" else "border", (0, 0, 0, W // 2), ("nan",), 0),
                 ("x", "last-sample", (B - 1, 0, H // 2, W // 2), ("nan",), B - 1),
                 # channel 1 is an identity channel of the heads and a tanh channel of the output; the last one is a
                 # sigmoid / tanh channel.  tanh and sigmoid saturate: +-inf gives the finite +-1, 0 or 1 (torch does the
                 # same, the oracle decides), so only an identity channel has +-inf cases of its own; -inf in x reaches every
                 # channel, the sigmoid ones included
                 ("w", "weight", (1, Cin - 1, 1, 2), ("nan", "+inf", "-inf") if post != "tanh" else ("nan",), None),
                 ("w", "weight-last", (cout - 1, Cin - 1, 1, 2), ("nan",), None), ("b", "bias", (cout - 1,), ("nan",), None),
                 ("up", "upstream", (0, cout - 1, H // 2, W // 2), ("nan",), 0)]
        for dname in ("f32", "bf16"):
            dtype = DTYPES[dname]
            for tensor, spot, index, values, sample in spots:
                if dname != "f32" and spot not in ("interior", "weight"):
                    continue
                for vname in values if dname == "f32" else values[:1]:
                    def make(shape4=shape4, cout=cout, dtype=dtype, tensor=tensor, index=index, vname=vname):
                        x, w, b, up = hu.make_case(shape4, cout, dtype, seed=3)
                        inp = {"x": x, "w": w, "b": b, "up": up}
                        inp[tensor] = plant(inp[tensor], index, VALUE_NAMES[vname])
                        return inp

                    def oracle(inp, shape4=shape4, cout=cout, post=post, split=split, padding=padding, slope=slope, dtype=dtype,
                               tensor=tensor, index=index):
                        t = hu.truth(inp["x"], inp["w"], inp["b"], inp["up"], padding, slope, post, split)
                        n = hu.term_counts(shape4, cout)
                        out = {}
                        for j, (y, S) in enumerate(zip(t["y"], t["S"]["y"])):
                            out["y%d" % j] = Quantity(y, hu.summation_bound(n["y"], S, y, dtype), floor=dtype)
                        out["gx"] = Quantity(t["gx"], hu.summation_bound(n["gx"], t["S"]["gx"], t["gx"], dtype), floor=dtype,
                                             allow=halo_ring(shape4, index[1]) if tensor == "w" and padding == "zeros" else None)
                        out["gw"] = Quantity(t["gw"], hu.summation_bound(n["gw"], t["S"]["gw"], t["gw"], dtype), batched=False, floor=dtype)
                        out["gb"] = Quantity(t["gb"], hu.summation_bound(n["gb"], t["S"]["gb"], t["gb"], dtype), batched=False, floor=dtype)
                        return out

                    def evaluate(fn, inp, split=split):
                        x, w, b = _leaf(inp["x"]), _leaf(inp["w"]), _leaf(inp["b"])
                        ys = fn(x, w, b)
                        ys = ys if isinstance(ys, tuple) else (ys,)
                        # each output's upstream gradient reaches the backward as the tensor made here (the same value as
                        # the gradient of sum(y * u))
                        up = inp["up"]
                        parts = (up,) if split is None else (up[:, :split].contiguous(), up[:, split:].contiguous())
                        torch.autograd.backward(list(ys), [to_dev(u.to(y.dtype)) for y, u in zip(ys, parts)])
                        out = {"y%d" % j: y for j, y in enumerate(ys)}
                        out.update({"gx": x.grad, "gw": w.grad, "gb": b.grad})
                        return out

                    def run(gfla, inp, evaluate=evaluate, post=post, split=split, padding=padding, slope=slope):
                        return evaluate(lambda x, w, b: gfla.HeadConv3x3Function.apply(
                            x, w, b, padding, slope, hu.posts_of(post, w.size(0)), split), inp)

                    def composition(gfla, inp, evaluate=evaluate, post=post, split=split, padding=padding, slope=slope):
                        return evaluate(lambda x, w, b: hu.composition(x, w, b, padding, slope, post, split), inp)
                    cases.append(Case("%s-%s-%s-%s" % (label, dname, spot, vname), "head_conv3x3", sample, make, oracle, run,
                                      _spot_where(shape, tensor, spot, index), composition))
    return cases


# ---- instance_norm_act: the single-workgroup and the split-plane route (csrc/instance_norm.hip) ---------------------------------
_SPLIT_SHAPE = {}


def instance_norm_shape(label, elem_size):
    """regime 0 from the sweep; "split": the smallest two-plane shape the library itself splits for this element size (B = 2,
    C = 1: the planes are the samples).  Asked of the library when a case runs, so that building the case list needs none.
    A label that is a shape stands for itself."""
    if isinstance(label, tuple):
        return label
    if label == "small":
        return (2, 5, 3, 7)
    if elem_size not in _SPLIT_SHAPE:
        _SPLIT_SHAPE[elem_size] = next((2, 1, H, 64) for H in range(1, 4097) if iu.geometry(2, 1, H, 64, elem_size)["regime"] == 2)
    return _SPLIT_SHAPE[elem_size]


def instance_norm_cases(labels=("small", "split")):
    cases = []
    for dname in ("f32", "bf16"):
        dtype = DTYPES[dname]
        esize = torch.empty((), dtype=dtype).element_size()
        for label in labels:
            for last, first_plane, vname in [(False, False, "nan"), (False, False, "+inf"), (True, True, "nan")]:
                if dname != "f32" and (vname != "nan" or last):
                    continue

                def index_of(shape, last=last, first_plane=first_plane):
                    B, C, H, W = shape
                    return (B - 1 if last else 0, 0 if first_plane else C - 1, H // 2, W // 2)

                def make(label=label, esize=esize, dtype=dtype, index_of=index_of, vname=vname):
                    shape = instance_norm_shape(label, esize)
                    x, w, b, up, slope = iu.make_case(shape, dtype, "affine_leaky", seed=iu.sweep_seed(shape))
                    return {"x": plant(x, index_of(shape), VALUE_NAMES[vname]), "w": w, "b": b, "up": up}

                def oracle(inp, dtype=dtype):
                    y, gx, gw, gb = iu.truth(inp["x"], inp["w"], inp["b"], inp["up"], iu.EPS, 0.1)
                    return {"y": Quantity(y, 0.0, floor=dtype), "gx": Quantity(gx, 0.0, floor=dtype),
                            "gw": Quantity(gw, 0.0, batched=False, floor=dtype), "gb": Quantity(gb, 0.0, batched=False, floor=dtype)}

                def evaluate(fn, inp):
                    x, w, b = _leaf(inp["x"]), _leaf(inp["w"]), _leaf(inp["b"])
                    y = fn(x, w, b)
                    y.backward(to_dev(inp["up"].to(y.dtype)))
                    return {"y": y, "gx": x.grad, "gw": w.grad, "gb": b.grad}

                def run(gfla, inp, evaluate=evaluate):
                    return evaluate(lambda x, w, b: gfla.InstanceNormActFunction.apply(x, w, b, iu.EPS, 0.1), inp)

                def composition(gfla, inp, evaluate=evaluate, dtype=dtype):
                    def fn(x, w, b):
                        with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
                            return iu.composition(x, w, b, iu.EPS, 0.1)
                    return evaluate(fn, inp)

                def where(inp, index_of=index_of, label=label):
                    hit = ~torch.isfinite(inp["x"])
                    regime = iu.geometry(*inp["x"].shape, inp["x"].element_size())["regime"]
                    return int(hit.sum()) == 1 and bool(hit[index_of(tuple(inp["x"].shape))]) and (regime == 2) == (label == "split")
                cases.append(Case("instance_norm_act-%s-%s-sample%s-%s" % ("x".join(map(str, label)) if isinstance(label, tuple) else label,
                                                                           dname, "last" if last else "0", vname),
                                  "instance_norm_act", 1 if last else 0, make, oracle, run, where, composition))
    return cases


# ---- max_cosine_similarity (csrc/max_cosine.hip) -------------------------------------------------------------------------------
# (B, C, Ns, Nt), forced source-range split (tuning key 5; 0: the library's own): the FAST staging path (C % 32 == 0, Ns and
# Nt multiples of 4 -- and of 8 for the 16-bit kernels), and a ragged shape with Ns > 128, so that the value crosses the
# merge of two source tiles, and with the split forced the merge of two workgroups' keys
COSINE_ROWS = [("fast", (2, 32, 264, 136), 0), ("ragged", (2, 20, 300, 257), 0), ("ragged-split2", (2, 20, 300, 257), 2)]
COSINE_ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}


def cosine_features(shape, seed, dtype):
    """tests/test_correctness_gpu.py's post-ReLU-like features, rounded to `dtype`"""
    from util import randn
    x = randn(shape, seed=seed).relu() * (1 + randn(shape[:1] + (1,) + shape[2:], seed=seed + 1).abs())
    return x.to(dtype).contiguous()


def max_cosine_cases(rows=COSINE_ROWS):
    from oracle.cpu_modules import max_cosine_cpu
    from util import randn
    cases = []
    for label, shape, split in rows:
        B, C, Ns, Nt = shape
        # a source position in the SECOND tile (row 200), a target position, one +inf feature; the last sample once
        spots = [("source", "source-position", (0, 3, 200), "nan", 0), ("target", "target-position", (0, C - 1, Nt - 1), "nan", 0),
                 ("source", "source-feature", (0, 5, 130), "+inf", 0), ("target", "target-feature", (0, 2, 7), "+inf", 0),
                 ("source", "last-sample", (B - 1, 0, 0), "nan", B - 1)]
        for dname in ("f32", "f16", "bf16"):
            dtype = DTYPES[dname]
            for tensor, spot, index, vname, sample in spots:
                if dname != "f32" and spot in ("target-feature", "last-sample"):
                    continue

                def make(shape=shape, dtype=dtype, tensor=tensor, index=index, vname=vname):
                    B, C, Ns, Nt = shape
                    inp = {"source": cosine_features((B, C, Ns), 1, dtype), "target": cosine_features((B, C, Nt), 2, dtype),
                           "up": randn((B, Nt), seed=9)}
                    inp[tensor] = plant(inp[tensor], index, VALUE_NAMES[vname])
                    return inp

                def oracle(inp, dtype=dtype):
                    s, t = inp["source"].double().requires_grad_(), inp["target"].double().requires_grad_()
                    best, index = max_cosine_cpu(s, t)
                    gs, gt = torch.autograd.grad(best, (s, t), inp["up"].double())
                    # the bars of tests/test_correctness_gpu.py and tests/test_correctness_half_gpu.py (util.assert_close:
                    # tol x max(1, max |want|) over the finite entries; 16-bit gradients: one unit of the storage type)
                    def scale(t):
                        f = t[torch.isfinite(t)]
                        return max(1.0, f.abs().max().item() if f.numel() else 0.0)
                    gtol = 1e-5 if dtype == torch.float32 else COSINE_ULP[dtype]
                    out = {"y": Quantity(best, 2e-6 * scale(best.detach())), "gs": Quantity(gs, gtol * scale(gs)),
                           "gt": Quantity(gt, gtol * scale(gt))}
                    out["y"].index = index            # torch.max: the row of the first NaN of a column that has one
                    return out

                def run(gfla, inp, shape=shape, split=split):
                    s, t = _leaf(inp["source"]), _leaf(inp["target"])
                    with gfla.tuned({gfla.TUNE_SPLIT: split}):
                        best, index = gfla.max_cosine_similarity(s, t, return_index=True)
                    # ORDER MATTERS: the backward gathers and scatters at `index` on the device.  It runs only behind this
                    # assertion, made on the host
                    host = index.cpu()
                    assert host.dtype == torch.int32 and int(host.min()) >= 0 and int(host.max()) < shape[2], \
                        "max_cosine_similarity returned an index outside [0, Ns): %d .. %d" % (int(host.min()), int(host.max()))
                    best.backward(to_dev(inp["up"].to(best.dtype)))
                    return {"y": best, "gs": s.grad, "gt": t.grad, "index": host}

                def where(inp, shape=shape, tensor=tensor, index=index, spot=spot, label=label, dtype=dtype):
                    B, C, Ns, Nt = shape
                    hit = ~torch.isfinite(inp[tensor])
                    fast = C % 32 == 0 and Ns % 8 == 0 and Nt % 8 == 0
                    return int(hit.sum()) == 1 and bool(hit[index]) and fast == (label == "fast") and Ns > 128 and \
                        (spot not in ("source-position", "source-feature") or index[2] >= 128)
                cases.append(Case("max_cosine-%s-%s-%s" % (label, dname, spot), "max_cosine_similarity", sample, make, oracle, run,
                                  where))
    return cases


# ---- VGG19Features at the golden widths, and VGGLoss of it ---------------------------------------------------------------------
def vgg_case():
    """One NaN pixel in sample 0 of golden image `a` (2, 3, 32, 24): every returned map against vgg_util.TorchVGG in
    float64 on the host; the bar is that of test_golden_network_float32 (4 x the largest relative error of the host's own
    float32 composition, of each map's largest entry)."""
    index = (0, 1, 13, 9)

    def make():
        gold = vu.load_golden()
        inp = {"image": plant(gold["a/image"].float(), index, NAN), "other": gold["b/image"].float()}
        inp.update({"param/" + k: gold["param/" + k] for k in vu.STATE_KEYS})
        return inp

    def state(inp, dtype):
        return {k: inp["param/" + k].to(dtype) for k in vu.STATE_KEYS}

    def oracle(inp):
        want = vu.TorchVGG(state(inp, torch.float64))(inp["image"].double())
        host = vu.TorchVGG(state(inp, torch.float32))(inp["image"])
        out, measured = {}, 0.0
        for layer in vu.LAYERS:
            ok = torch.isfinite(want[layer])
            measured = max(measured, ((host[layer].double() - want[layer]).abs()[ok].max() / want[layer][ok].abs().max()).item())
        for layer in vu.LAYERS:
            ok = torch.isfinite(want[layer])
            out["y_" + layer] = Quantity(want[layer], 4 * measured * want[layer][ok].abs().max().item())
        return out

    def module(gfla, inp):
        m = gfla.VGG19Features(widths=vu.GOLDEN_WIDTHS)
        m.load_state_dict(state(inp, torch.float32), strict=True)
        return m.to(DEV)

    def run(gfla, inp):
        out = module(gfla, inp)(to_dev(inp["image"]))
        return {"y_" + layer: out[layer] for layer in vu.LAYERS}

    def where(inp):
        hit = ~torch.isfinite(inp["image"])
        return int(hit.sum()) == 1 and bool(hit[index])
    case = Case("VGG19Features-f32-one-nan-pixel", "VGG19Features", 0, make, oracle, run, where)
    case.module = module
    return case


def _scale(t):
    """util.assert_close's scale, over the finite entries: max(1, max |want|)"""
    f = t[torch.isfinite(t)]
    return max(1.0, f.abs().max().item() if f.numel() else 0.0)


def _top(t):
    f = t[torch.isfinite(t)]
    return f.abs().max().item() if f.numel() else 0.0


# ---- flow_warp (csrc/flow_warp.hip) ----------------------------------------------------------------------------------------------
WARP_SHAPE = (2, 16, 12, 10)      # tests/test_flow_warp_gpu.py's first sweep row, the flow of the source's size, "pixel"


def flow_warp_cases(shape=WARP_SHAPE):
    import flow_warp_util as fu
    from global_flow_local_attention_amd.flow_warp import convention_scalars, torch_flow_warp
    from util import make_flow, randn
    B, C, H, W = shape
    scalars = convention_scalars("pixel", H, W)
    spots = [("src", "source", (0, 3, 5, 4), ("nan", "+inf"), 0), ("flow", "flow-x", (0, 0, 6, 5), ("nan", "+inf"), 0),
             ("flow", "flow-y", (0, 1, 6, 5), ("nan", "-inf"), 0), ("src", "last-sample", (B - 1, C - 1, 6, 5), ("nan",), B - 1),
             ("up", "upstream", (0, 2, 3, 3), ("nan",), 0)]
    cases = []
    for dname in ("f32", "f16"):
        dtype = DTYPES[dname]
        for tensor, spot, index, values, sample in spots:
            for vname in values if dname == "f32" else values[:1]:
                def make(dtype=dtype, tensor=tensor, index=index, vname=vname):
                    flow = fu.clear_of_kinks(make_flow("coherent", B, H, W, seed=4), [scalars])
                    inp = {"src": randn(shape, seed=3).to(dtype), "flow": flow, "up": randn(shape, seed=5)}
                    inp[tensor] = plant(inp[tensor], index, VALUE_NAMES[vname])
                    return inp

                def oracle(inp, dtype=dtype, tensor=tensor, index=index):
                    out, gs, gf = fu.truth(inp["src"], inp["flow"], scalars, inp["up"])
                    return {"y": Quantity(out, 0.0, floor=torch.float32, scale=_top(inp["src"].double())),
                            "gs": Quantity(gs, 0.0, floor=dtype), "gf": Quantity(gf, 0.0, floor=torch.float32)}

                def evaluate(fn, inp):
                    s, f = _leaf(inp["src"]), _leaf(inp["flow"])
                    out = fn(s, f)
                    out.backward(to_dev(inp["up"].to(out.dtype)))
                    return {"y": out, "gs": s.grad, "gf": f.grad}

                def run(gfla, inp, evaluate=evaluate):
                    return evaluate(lambda s, f: gfla.FlowWarpFunction.apply(s, f, *scalars), inp)

                def composition(gfla, inp, evaluate=evaluate, dtype=dtype):
                    def fn(s, f):
                        with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
                            return torch_flow_warp(s, f, *scalars)
                    return evaluate(fn, inp)

                def where(inp, tensor=tensor, index=index):
                    hit = ~torch.isfinite(inp[tensor])
                    return int(hit.sum()) == 1 and bool(hit[index]) and bool((inp["up"][index[0], :, index[2], index[3]] != 0).all())
                cases.append(Case("flow_warp-%s-%s-%s" % (dname, spot, vname), "flow_warp", sample, make, oracle, run, where,
                                  composition))
    return cases


# ---- AffineRegularizationLoss (csrc/affine_reg.hip) -------------------------------------------------------------------------------
AFFINE_SHAPE, AFFINE_KZ = (2, 9, 8), 3


def affine_cases(shape=AFFINE_SHAPE):
    import affine_util as au
    from util import make_flow
    B, H, W = shape
    half_ulp = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
    cases = []
    for dname in ("f32", "bf16"):
        dtype = DTYPES[dname]
        for spot, index, vname, sample in [("interior", (0, 0, 4, 3), "nan", 0), ("interior", (0, 1, 4, 3), "+inf", 0),
                                           ("corner", (B - 1, 1, H - 1, W - 1), "nan", B - 1)]:
            if dname != "f32" and vname != "nan":
                continue

            def make(dtype=dtype, index=index, vname=vname):
                return {"flow": plant(make_flow("coherent", B, H, W, dtype, seed=103), index, VALUE_NAMES[vname])}

            def oracle(inp, dtype=dtype):
                # the bars of tests/test_affine_reg_gpu.py (_check): its float64 reference's own rounding, measured at the
                # zero flow, is allowed on top
                want, want_g = au.reference(inp["flow"], AFFINE_KZ)
                _, e_grad = au.reference(torch.zeros(B, 2, H, W, dtype=torch.float64), AFFINE_KZ)
                tol = 1e-5 * _top(want_g) + 4 * e_grad.abs().max().item() + half_ulp.get(dtype, 0.0) * want_g.abs().nan_to_num(0.0, 0.0, 0.0)
                return {"y": Quantity(torch.tensor(want, dtype=torch.float64), 2e-6 * abs(want), batched=False),
                        "gf": Quantity(want_g, tol)}

            def run(gfla, inp):
                f = _leaf(inp["flow"])
                loss = gfla.AffineRegularizationLoss(AFFINE_KZ)(f)
                assert type(loss.grad_fn).__name__ == "AffineRegFunctionBackward"
                loss.backward()
                return {"y": loss, "gf": f.grad}

            def where(inp, index=index, spot=spot):
                hit = ~torch.isfinite(inp["flow"])
                corner = index[2:] == (H - 1, W - 1)
                return int(hit.sum()) == 1 and bool(hit[index]) and corner == (spot == "corner")
            cases.append(Case("affine_reg-%s-%s-sample%d-%s" % (dname, spot, sample, vname), "AffineRegularizationLoss", sample,
                              make, oracle, run, where))
    return cases


# ---- CorrectnessMapFunction (csrc/correctness_map.hip) ------------------------------------------------------------------------------
CMAP_SHAPE = (2, 12, 70)


def correctness_map_cases(shape=CMAP_SHAPE):
    from util import randn
    B, C, N = shape
    spots = [("warped", "warped", (0, 3, 20), ("nan", "+inf"), 0), ("target", "target", (0, 4, 33), ("nan", "-inf"), 0),
             ("best", "best", (0, 41), ("nan",), 0), ("warped", "last-sample", (B - 1, 0, 69), ("nan",), B - 1),
             ("up", "upstream", (0, 7), ("nan",), 0)]
    cases = []
    for dname in ("f32", "bf16"):
        dtype = DTYPES[dname]
        for tensor, spot, index, values, sample in spots:
            if dname != "f32" and spot not in ("warped", "target"):
                continue
            for vname in values if dname == "f32" else values[:1]:
                def make(dtype=dtype, tensor=tensor, index=index, vname=vname):
                    inp = {"warped": cosine_features(shape, 21, torch.float32), "target": cosine_features(shape, 22, dtype),
                           "best": (randn((B, N), seed=23).abs() * 0.5 + 0.2).contiguous(), "up": randn((B, N), seed=24)}
                    inp[tensor] = plant(inp[tensor], index, VALUE_NAMES[vname])
                    return inp

                def oracle(inp, dtype=dtype):
                    x, t, best = (inp[k].double().requires_grad_() for k in ("warped", "target", "best"))
                    want = torch.exp(-F.cosine_similarity(x, t) / (best + 1e-8))
                    gx, gt, gb = torch.autograd.grad(want, (x, t, best), inp["up"].double())
                    # tests/test_correctness_gpu.py: 2e-6 / 1e-5 under util.assert_close; a 16-bit target's gradient at one
                    # unit of its type (tests/test_correctness_half_gpu.py)
                    ttol = 1e-5 if dtype == torch.float32 else COSINE_ULP[dtype]
                    return {"y": Quantity(want, 2e-6 * _scale(want.detach())), "gx": Quantity(gx, 1e-5 * _scale(gx)),
                            "gt": Quantity(gt, ttol * _scale(gt)), "gb": Quantity(gb, 1e-5 * _scale(gb))}

                def run(gfla, inp):
                    x, t, best = _leaf(inp["warped"]), _leaf(inp["target"]), _leaf(inp["best"])
                    out = gfla.CorrectnessMapFunction.apply(x, t, best, 1e-8)
                    out.backward(to_dev(inp["up"].to(out.dtype)))
                    return {"y": out, "gx": x.grad, "gt": t.grad, "gb": best.grad}
                cases.append(Case("correctness_map-%s-%s-%s" % (dname, spot, vname), "CorrectnessMapFunction", sample, make, oracle,
                                  run, _one_hit(tensor, index)))
    return cases


def _one_hit(tensor, index):
    def where(inp):
        hit = ~torch.isfinite(inp[tensor])
        return int(hit.sum()) == 1 and bool(hit[index])
    return where


# ---- gram_l1, the style term of VGGLoss / StyleLoss (csrc/gram_l1.hip) ---------------------------------------------------------
GRAM_SHAPE = (2, 40, 9, 7)


def gram_cases(shape=GRAM_SHAPE):
    import style_util as su
    from global_flow_local_attention_amd.losses import compute_gram
    B, C, H, W = shape
    half_ulp = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
    cases = []
    for dname in ("f32", "f16"):
        dtype = DTYPES[dname]
        for tensor, spot, index, vname, sample in [("x", "generated", (0, 7, 4, 3), "nan", 0), ("x", "generated", (0, 7, 4, 3), "+inf", 0),
                                                   ("y", "target", (0, 11, 2, 2), "nan", 0), ("x", "last-sample", (B - 1, C - 1, 8, 6), "nan", B - 1)]:
            if dname != "f32" and vname != "nan":
                continue

            def make(dtype=dtype, tensor=tensor, index=index, vname=vname):
                x, y = su.make_features(B, C, H, W, dtype, seed=C + H + W, near=False)
                inp = {"x": x, "y": y}
                inp[tensor] = plant(inp[tensor], index, VALUE_NAMES[vname])
                return inp

            def oracle(inp, dtype=dtype):
                x, y = inp["x"].double().requires_grad_(), inp["y"].double().requires_grad_()
                loss = F.l1_loss(compute_gram(x), compute_gram(y))
                gx, gy = torch.autograd.grad(loss, (x, y))
                # tests/test_style_loss_gpu.py: 1e-5 of the largest entry, half a unit of a 16-bit type per entry
                tol = [1e-5 * _top(g) + (half_ulp.get(dtype, 0.0) * g.abs().nan_to_num(0.0, 0.0, 0.0)).clamp_min(
                    2.0 ** -25 if dtype == torch.float16 else 0.0) for g in (gx, gy)]
                q = {"y": Quantity(loss, 2e-6 * abs(loss.item()), batched=False), "gx": Quantity(gx, tol[0]), "gy": Quantity(gy, tol[1])}
                q["y"].diff = compute_gram(x).detach() - compute_gram(y).detach()
                return q

            def run(gfla, inp):
                x, y = _leaf(inp["x"]), _leaf(inp["y"])
                loss = gfla.gram_l1(x, y)
                assert type(loss.grad_fn).__name__ == "GramL1FunctionBackward"
                loss.backward()
                return {"y": loss, "gx": x.grad, "gy": y.grad}

            def where(inp, tensor=tensor, index=index):
                # and no entry of D so small that float32 may resolve its sign the other way (tests/test_style_loss_gpu.py's
                # mask): every sign of the finite part is decided
                hit = ~torch.isfinite(inp[tensor])
                _, d, gx = su.reference(inp["x"], inp["y"])
                ok = torch.isfinite(d)
                clear = bool((d[ok].abs() > 2e-6 * gx[torch.isfinite(gx)].abs().max()).all())
                return int(hit.sum()) == 1 and bool(hit[index]) and clear
            cases.append(Case("gram_l1-%s-%s-%s" % (dname, spot, vname), "gram_l1", sample, make, oracle, run, where))
    return cases


# ---- the fully connected layer of ExtractorAttn (csrc/fc_block.hip, fc_sample.hip): a non-finite FLOW entry ------------------
FC_NAMES = ("logits", "g_s", "g_t", "g_f", "g_w0", "g_b0", "g_w1", "g_b1")
FC_BATCHED = ("logits", "g_s", "g_t", "g_f")
FC_ROWS = [((5, 3, 17, 7, 5), 5), ((5, 3, 17, 7, 5), 4), ((3, 3, 17, 7, 5), 5), ((3, 3, 17, 7, 5), 4)]   # (k, B, C, H, W), mode


def fc_layer_run(c, mode):
    """gfla_fc_forward_f32 + gfla_fc_backward_f32 through the C ABI, as tests/test_fc_structured_gpu.py runs them"""
    from global_flow_local_attention_amd import _lib, fc_mfma
    k, B, C, H, W, slope = c["k"], c["B"], c["C"], c["H"], c["W"], c["slope"]
    assert fc_mfma.resolve_mode(C, H, W, k, mode) == mode
    s, t, f, w0, b0, w1, b1, up = (to_dev(c[n].float().contiguous()) for n in ("s", "t", "f", "w0", "b0", "w1", "b1", "up"))
    ws = torch.empty(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 0), dtype=torch.uint8, device=DEV)
    sc = torch.empty(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 1), dtype=torch.uint8, device=DEV)
    lg = torch.full((B, k * k, H, W), NAN, device=DEV)
    p = _lib.ptr
    _lib.call("gfla_fc_forward_f32", s, p(s), p(t), p(f), p(w0), p(b0), p(w1), p(b1), p(ws), p(lg), B, C, H, W, k, slope, mode)
    gs, gt = (torch.full((B, C, H, W), NAN, device=DEV) for _ in range(2))
    gf = torch.full_like(f, NAN)
    gw0, gb0, gw1, gb1 = (torch.full_like(x, NAN) for x in (w0, b0, w1, b1))
    _lib.call("gfla_fc_backward_f32", f, p(ws), p(f), p(w1), p(up), p(sc), p(gs), p(gt), p(gf), p(gw0), p(gb0), p(gw1), p(gb1),
              B, C, H, W, k, slope, mode, 0)
    torch.cuda.synchronize()
    return dict(zip(FC_NAMES, (lg, gs, gt, gf, gw0, gb0, gw1, gb1)))


def fc_layer_cases(rows=FC_ROWS):
    import fc_util as fu
    cases = []
    for shape, mode in rows:
        k, B, C, H, W = shape
        live = fu.make_case(shape, False, "narrow")["up"].abs().sum(1) > 0      # the case's upstream gradient is sparse

        def pixel(sample):
            """the first interior position of `sample` with a non-zero upstream gradient"""
            at = live[sample, 1:-1, 1:-1].nonzero()[0].tolist()
            return at[0] + 1, at[1] + 1
        for spot, index, vname, sample in [("flow-x", (0, 0) + pixel(0), "nan", 0), ("flow-y", (0, 1) + pixel(0), "+inf", 0),
                                           ("last-sample", (B - 1, 0) + pixel(B - 1), "nan", B - 1)]:
            if mode == 4 and spot != "flow-x":
                continue

            def make(shape=shape, index=index, vname=vname):
                c = dict(fu.make_case(shape, False, "narrow"))
                c["f"] = plant(c["f"], index, VALUE_NAMES[vname])
                return c

            def oracle(c, shape=shape, mode=mode, sample=sample):
                # the float64 layer on the planted flow; the bars of fc_util.layer_bars, worked out on the case without the
                # value: outside P nothing depends on the poisoned position, so both the reference and its bar are the same
                r = fu.layer_reference(c)
                lb = fu.layer_bars(shape, "narrow", mode)
                out = {}
                for n in FC_NAMES:
                    want = r[n]
                    bar = lb["bar"][n].reshape(want.shape).clone()
                    if n == "g_f":
                        bar[lb["flow_excluded"]] = PINF          # the bilinear kink, left out as in test_fc_structured_gpu.py
                    out["y_logits" if n == "logits" else n] = Quantity(want, bar, batched=n in FC_BATCHED)
                # DESIGN.md, "Non-finite values": the scale of the owner-computes scatter's fixed-point cells is ONE maximum over
                # the batch, so a non-finite d hidden or flow makes every workgroup write NaN to the rows it owns: the gradient
                # of the source map is NaN in every sample.  The one documented deviation from batch isolation; the logits and
                # every other gradient are held to the rule
                out["g_s"].allow = torch.ones(out["g_s"].want.shape, dtype=torch.bool)
                out["g_s"].batch_wide = True
                return out

            def run(gfla, c, mode=mode):
                got = fc_layer_run(c, mode)
                got["y_logits"] = got.pop("logits")
                return got

            def where(c, index=index):
                hit = ~torch.isfinite(c["f"])
                return int(hit.sum()) == 1 and bool(hit[index]) and bool((c["up"][index[0], :, index[2], index[3]] != 0).any())
            cases.append(Case("fc_layer-k%d-mode%d-%s-%s" % (k, mode, spot, vname), "fc_layer", sample, make, oracle, run, where))
    return cases


# ---- Resample2d and BlockExtractor: a NaN flow entry under a NON-ZERO upstream gradient ----------------------------------------
# (tests/test_gpu_parity.py::test_non_finite_flows_stay_in_bounds gives the poisoned pixels a zero gradient.)  Only NaN is
# planted: the host oracle is C, and its float -> int conversion of an inf is not the GPU's (INT_MIN against a saturated
# INT_MAX), so the clamped taps -- hence the cells the NaN weights reach -- would differ for a reason that is the host's.
SCATTER_SHAPE = (2, 8, 20, 14)


def scatter_cases(shape=SCATTER_SHAPE):
    from oracle import cpu_modules
    from util import make_flow, randn
    B, C, H, W = shape
    cases = []
    for op, k in (("Resample2d", 4), ("BlockExtractor", 3)):
        for dname in ("f32", "bf16"):
            dtype = DTYPES[dname]
            for sample in (0, B - 1):
                if dname != "f32" and sample != 0:
                    continue
                index = (sample, 0, 7, 5)

                def make(dtype=dtype, index=index, op=op, k=k):
                    up_shape = shape if op == "Resample2d" else (B, C, H * k, W * k)
                    up = randn(up_shape, seed=82).to(dtype)
                    return {"src": randn(shape, seed=80).to(dtype), "up": up + (up == 0).to(dtype),
                            "flow": plant(make_flow("coherent", B, H, W, seed=81).to(dtype), index, NAN)}

                def forward(op=op, k=k):
                    return (lambda g, s, f: g.Resample2d(4, 1, 2)(s, f)) if op == "Resample2d" else \
                        (lambda g, s, f: g.BlockExtractor(k)(s, f))

                def oracle(inp, op=op, k=k, index=index, dtype=dtype):
                    s, f = inp["src"].double().requires_grad_(), inp["flow"].double().requires_grad_()
                    out = cpu_modules.Resample2dCPU(4, 1, 2)(s, f) if op == "Resample2d" else cpu_modules._BlockExtractorCPU.apply(s, f, k)
                    gs, gf = torch.autograd.grad(out, (s, f), inp["up"].double())
                    # tests/test_gpu_parity.py's bars: float32 2e-6 forward and 1e-5 for the gradients under util.assert_close
                    # (of max(1, the largest entry)); bfloat16 storage 2^-8 forward and 2^-7 for the gradients, of the largest
                    # entry (test_bf16_forward_ops, test_bf16_backward_ops)
                    if dtype == torch.float32:
                        bars = (2e-6 * _scale(out.detach()), 1e-5 * _scale(gs), 1e-5 * _scale(gf))
                    else:
                        bars = (2.0 ** -8 * _top(out.detach()), 2.0 ** -7 * _top(gs), 2.0 ** -7 * _top(gf))
                    q = {"y": Quantity(out, bars[0]), "gs": Quantity(gs, bars[1]), "gf": Quantity(gf, bars[2])}
                    # lds_plane.h: a workgroup whose fixed-point cells meet a contribution they cannot hold writes NaN to the
                    # planes it owns -- channels of the planted sample, never another sample
                    # (Resample2d's scatter; BlockExtractor's planes are floating point and need no allowance)
                    if op == "Resample2d":
                        q["gs"].allow = torch.zeros(gs.shape, dtype=torch.bool)
                        q["gs"].allow[index[0]] = True
                    return q

                def run(gfla, inp, forward=forward):
                    s, f = _leaf(inp["src"]), _leaf(inp["flow"])
                    out = forward()(gfla, s, f)
                    out.backward(to_dev(inp["up"]))
                    return {"y": out, "gs": s.grad, "gf": f.grad}
                cases.append(Case("%s-%s-flow-nan-sample%d" % (op, dname, sample), op, sample, make, oracle, run,
                                  _one_hit("flow", index)))
    return cases


PER_SAMPLE_OPS = ("Resample2d", "BlockExtractor", "conv3x3_relu", "maxpool2x2", "conv3x3", "conv4x4_down", "conv_transpose3x3_up", "conv1x1", "head_conv3x3",
                  "instance_norm_act", "max_cosine_similarity", "flow_warp", "AffineRegularizationLoss", "CorrectnessMapFunction",
                  "gram_l1", "fc_layer")
OPS = PER_SAMPLE_OPS + ("VGG19Features",)


def all_cases():
    return relu_conv_cases() + pool_cases() + [vgg_case()] + max_cosine_cases() + gen_conv_cases() + conv1x1_cases() + \
        head_conv_cases() + instance_norm_cases() + flow_warp_cases() + affine_cases() + correctness_map_cases() + gram_cases() + \
        fc_layer_cases() + scatter_cases()
