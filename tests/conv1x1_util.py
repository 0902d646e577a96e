"""Shared by the tests of the 1x1 convolutions (gen_conv.conv1x1; csrc/conv1x1.hip, csrc/gen_conv_wgrad.hip): the cases,
their seeded host inputs, the float64 host truth with the derived bars, and a generator-shaped residual block with a
learnable 1x1 shortcut.

The truth is float64 on the host from the stored values all the way through: the pooling in float64 as well, the
activation as torch hands it on (gen_conv_util.activated: computed by torch in x's dtype, rounded once).  The bars, with K
products per element, S the same expression on absolute values and u = gen_conv_util.UNIT[dtype]:

    forward   |y - y64|   <= 2 (K + 2 + 3 [pool 2]) 2^-24 S + u |y64| (+ u S for pool 2 in a 16-bit dtype),    K = Cin
              K products and a bias summed in float32 in an order of the kernel's own; with pool 2 every product's
              operand is itself a float32 sum of four values and a scaling (three more roundings); then the one rounding
              of a 16-bit result.  A pooled value of a 16-bit map is rounded to the dtype once before it is multiplied:
              a relative error u of every product, u S in all.
    grad_x    |gx - gx64| <= 2 (K + 2) 2^-24 S_x + u |gx64|,                                                 K = Cout
              the 0.25 of pool 2 is a power of two, exact; nothing is added.
    grad_w    |gw - gw64| <= 2 (K + 2) 2^-24 S_w (+ u S_w for pool 2 in a 16-bit dtype),            K = B Hout Wout
              float32 result; the pooled operand carries its one rounding as in the forward.
    grad_b    |gb - gb64| <= 2 (K + 2) 2^-24 sum |g|,                                                K = B Hout Wout
              as tests/test_gen_conv_train_gpu.py.
"""
import functools

import torch
import torch.nn.functional as F
from torch import nn

import gen_conv_util as gu

# (B, Cin, Cout, H, W) and options, every row in all three dtypes: one output pixel in one row of a 32-row tile with a
# chunk 3/8 or 3/16 full; odd both ways (10 x 9) with a ragged chunk and a ragged channel tile; several workgroups along
# the pixels and two channel blocks, Cout > 64 and no multiple of 32; the activation and its derivative on a small odd
# map; the final convolution's form without a bias.  Then the longest reduction in float32 and bfloat16.
ROWS = [((1, 3, 1, 2, 2), {"pool": 2}), ((2, 20, 40, 21, 19), {"pool": 2}), ((1, 8, 72, 70, 80), {"pool": 2}),
        ((2, 20, 40, 9, 7), {"slope": 0.1}), ((1, 33, 1, 5, 5), {"slope": 0.1, "nobias": True})]
DEEP = (1, 512, 4, 4, 4)
CASES = [(n, s, o) for s, o in ROWS for n in gu.ALL] + [(n, DEEP, {}) for n in ("f32", "bf16")]
ODD = ((2, 20, 40, 21, 19), {"pool": 2})


def key(opts):
    return tuple(sorted(opts.items()))


def out_size(H, W, pool):
    return H // pool, W // pool


@functools.lru_cache(maxsize=None)
def inputs(name, shape, opts_key):
    """(x, w, b | None, g) on the host: x and g in the case's dtype, the parameters float32 and representable in it; with
    a slope, a few entries of x are exactly 0 (act'(0) = slope)"""
    opts = dict(opts_key)
    dtype = gu.DTYPES[name]
    B, Cin, Cout, H, W = shape
    gen = torch.Generator().manual_seed(sum(shape) + 7 * opts.get("pool", 1))
    x = torch.randn(B, Cin, H, W, generator=gen).to(dtype)
    if opts.get("slope") is not None:
        x.view(-1)[::7] = 0
    w = (torch.randn(Cout, Cin, 1, 1, generator=gen) * (2.0 / Cin) ** 0.5).to(dtype).float()
    b = None if opts.get("nobias") else (torch.randn(Cout, generator=gen) * 0.2).to(dtype).float()
    g = torch.randn((B, Cout) + out_size(H, W, opts.get("pool", 1)), generator=gen).to(dtype)
    return x, w, b, g


@functools.lru_cache(maxsize=None)
def truth(name, shape, opts_key):
    """dict of y, gx, gw, gb (None without a bias) in float64 and of Sy, Sx, Sw, Sb, the same from absolute values;
    computed once per case and shared: treat it as read-only"""
    opts = dict(opts_key)
    return truth_of(*inputs(name, shape, opts_key), pool=opts.get("pool", 1), slope=opts.get("slope"))


def truth_of(x, w, b, g, pool=1, slope=None):
    """truth() of host tensors given as they are stored (tests/nonfinite_util.py plants a NaN in one first)"""
    dact = torch.ones(x.shape, dtype=torch.float64) if slope is None else \
        torch.where(x.float() > 0, 1.0, float(torch.tensor(slope, dtype=torch.float32))).double()

    def run(x64, a64, w64, b64, g64):
        # pool 2: differentiate through the float64 pooling from x; pool 1: from the activated map, then act'(x)
        leaf = (x64 if pool == 2 else a64).clone().requires_grad_()
        w64 = w64.clone().requires_grad_()
        b64 = None if b64 is None else b64.clone().requires_grad_()
        y = F.conv2d(F.avg_pool2d(leaf, 2, 2) if pool == 2 else leaf, w64, b64)
        grads = torch.autograd.grad(y, (leaf, w64) + (() if b64 is None else (b64,)), g64)
        return y.detach(), grads[0] * dact, grads[1], None if b64 is None else grads[2]
    x64, g64, w64 = x.double(), g.double(), w.double()
    a64 = gu.activated(x, slope).double()
    b64 = None if b is None else b.double()
    y, gx, gw, gb = run(x64, a64, w64, b64, g64)
    Sy, Sx, Sw, Sb = run(x64.abs(), a64.abs(), w64.abs(), None if b64 is None else b64.abs(), g64.abs())
    return {"y": y, "gx": gx, "gw": gw, "gb": gb, "Sy": Sy, "Sx": Sx, "Sw": Sw, "Sb": Sb}


def bars(name, shape, opts_key):
    """the four bars of a case (see the module docstring), each of its quantity's shape"""
    return bars_of(truth(name, shape, opts_key), gu.DTYPES[name], shape, dict(opts_key).get("pool", 1))


def bars_of(t, dtype, shape, pool=1):
    """bars() from a truth dict"""
    B, Cin, Cout, H, W = shape
    ho, wo = out_size(H, W, pool)
    u, eps = gu.UNIT[dtype], 2.0 ** -24
    staged = u if pool == 2 else 0.0                     # the one rounding of each pooled value
    out = {"y": 2.0 * (Cin + 2 + (3 if pool == 2 else 0)) * eps * t["Sy"] + u * t["y"].abs() + staged * t["Sy"],
           "gx": 2.0 * (Cout + 2) * eps * t["Sx"] + u * t["gx"].abs(),
           "gw": 2.0 * (B * ho * wo + 2) * eps * t["Sw"] + staged * t["Sw"]}
    if t["gb"] is not None:
        out["gb"] = gu.bar(t["Sb"], t["gb"], B * ho * wo, torch.float32, False)
    return out


def leaves(name, shape, opts_key, device="cuda", needs=(True, True, True)):
    """fresh leaf tensors (x, w, b | None) of a case on `device`, and the upstream gradient"""
    x, w, b, g = inputs(name, shape, opts_key)
    made = [None if t is None else t.detach().clone().to(device).requires_grad_(n) for t, n in zip((x, w, b), needs)]
    return made, g.to(device)


class WideningResBlock(nn.Module):
    """(act -> conv3x3 -> act -> conv3x3)(x) + conv1x1(x): the structure of the reference's ResBlock with a learnable
    shortcut, nn.Sequential-built, without norms"""

    def __init__(self, cin=12, cout=20):
        super(WideningResBlock, self).__init__()
        self.model = nn.Sequential(nn.LeakyReLU(0.1), nn.Conv2d(cin, cout, 3, 1, 1), nn.LeakyReLU(0.1),
                                   nn.Conv2d(cout, cout, 3, 1, 1))
        self.shortcut = nn.Sequential(nn.Conv2d(cin, cout, 1))

    def forward(self, x):
        return self.model(x) + self.shortcut(x)


def widening_blocks(device, copies=2, seed=41):
    """(`copies` float32 blocks on `device` with equal parameters, an input (2, 12, 11, 9))"""
    torch.manual_seed(seed)
    first = WideningResBlock()
    nets = []
    for _ in range(copies):
        net = WideningResBlock()
        net.load_state_dict(first.state_dict())
        nets.append(net.to(device).train())
    g = torch.Generator().manual_seed(seed + 1)
    return nets, torch.randn(2, 12, 11, 9, generator=g).to(device)
