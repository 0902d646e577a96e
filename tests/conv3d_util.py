"""Shared by the tests of the frames-major 3-D convolutions (conv3d.py, spectral_norm.SpectralConv3d; csrc/conv3d.hip,
csrc/gen_conv_wgrad.hip, csrc/avg_pool_frames.hip): the cases, their seeded host inputs, the float64 host truth with the
derived bars, a pure-Python emulation of the window rule, and stand-in networks written from the documented structure of the
reference's ResBlock3DEncoder and TemporalDiscriminator (none of the reference's code).

Truth is float64 F.conv3d / F.avg_pool3d on the host from the stored values (the activation as torch hands it on,
gen_conv_util.activated).  Bars, with gen_conv_util.bar(S, y64, K, dtype, add) = 2 (K + 2 + add) 2^-24 S + u |y64|, S the
same expression from absolute values:

    forward   K = 27 C (k333), 48 C (k344): the three temporal taps are part of the one float32 sum
    grad_x    K = 27 Cout (k333: 3 frames x 9 taps), 12 Cout (k344: 3 frames x one phase of 2 x 2 taps)
    grad_w    K = B Lout Hout Wout, float32 result;  grad_b  the same K, S = sum |g|
    pool      u |p64| + 14 2^-24 S, S = avg_pool3d(|x|): eleven float32 additions, the rounded constant 1/12 and the
              product are thirteen roundings, each relative to at most the absolute-value sum (scaled by 1/12 as the result
              is); fourteen leaves one to spare.  Its gradient likewise with S from |g| (two additions at most).
              u |p64| is the rounding of a NORMAL 16-bit number; a float16 result below 2^-14 is rounded to a multiple of
              2^-24, an absolute error of up to 2^-25 that no relative term covers (measured on standard-normal inputs: 36
              of 179,200 gradient elements, every one a correctly rounded subnormal, e.g. -2^-24 for -7.45e-8).  The pool's
              inputs therefore have magnitudes of at least 0.25 (pool_inputs): a single-term result is then normal, and any
              other has S >= 2 x 0.25 / 12, so that 14 2^-24 S >= 3.4e-8 covers the 2^-25 = 2.98e-8 of a subnormal one.
"""
import functools

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils import spectral_norm as sn

import discriminator_util as du
import gen_conv_util as gu

K = {"k333": 3, "k344": 4}
STRIDE = {"k333": (1, 1, 1), "k344": (1, 2, 2)}
PADDING = {"k333": (1, 1, 1), "k344": (0, 1, 1)}

# (geometry, (B, L, C, Cout, H, W), options): the table of the issue
ROWS = [("k333", (1, 1, 3, 64, 9, 7), {}),             # window clipped on both sides; a chunk spanning all frames
        ("k333", (2, 4, 20, 40, 17, 9), {}),           # both strides of the two-level batch; chunks straddle frames
        ("k333", (1, 2, 16, 32, 1, 40), {}),           # C equal to or half a chunk; one-row map
        ("k333", (1, 3, 5, 130, 5, 5), {}),            # three channel blocks, the last ragged
        ("k344", (1, 3, 3, 64, 10, 8), {}),            # Lout = 1
        ("k344", (2, 4, 20, 40, 33, 17), {"slope": 0.1, "add": True}),    # odd sizes; tiles over both edges
        ("k344", (1, 6, 21, 32, 2, 2), {}),            # all halo
        ("k344", (1, 5, 16, 72, 19, 21), {"add": True})]                  # today's addend shape
DEEP = ("k344", (1, 3, 512, 32, 4, 4), {})             # the longest reduction
CASES = [(n, g, s, o) for g, s, o in ROWS for n in gu.ALL] + [(n,) + DEEP for n in ("f32", "bf16")]
POOL_SHAPES = [(1, 3, 1, 2, 2), (2, 5, 20, 21, 19), (1, 4, 8, 70, 80)]     # (B, L, C, H, W)
POOL_CASES = [(n, s) for s in POOL_SHAPES for n in gu.ALL]


def case_id(v):
    return gu.case_id(v)


def key(opts):
    return tuple(sorted(opts.items()))


def out_size(geometry, L, H, W):
    return (L, H, W) if geometry == "k333" else (L - 2, (H - 2) // 2 + 1, (W - 2) // 2 + 1)


def torch_layout(t):
    """frames-major (B,L,C,H,W) <-> torch's (B,C,L,H,W): the permutation is its own inverse"""
    return t.permute(0, 2, 1, 3, 4)


@functools.lru_cache(maxsize=None)
def inputs(name, geometry, shape, opts_key):
    """(x, w, b, add | None, g) on the host: x, add and g frames-major in the case's dtype, the parameters float32 and
    representable in it; with a slope a few entries of x are exactly 0"""
    opts = dict(opts_key)
    dtype = gu.DTYPES[name]
    B, L, C, Cout, H, W = shape
    k = K[geometry]
    gen = torch.Generator().manual_seed(sum(shape) + k)
    x = torch.randn(B, L, C, H, W, generator=gen).to(dtype)
    if opts.get("slope") is not None:
        x.view(-1)[::7] = 0
    w = (torch.randn(Cout, C, 3, k, k, generator=gen) * (2.0 / (3 * k * k * C)) ** 0.5).to(dtype).float()
    b = (torch.randn(Cout, generator=gen) * 0.2).to(dtype).float()
    oshape = (B, out_size(geometry, L, H, W)[0], Cout) + out_size(geometry, L, H, W)[1:]
    add = torch.randn(oshape, generator=gen).to(dtype) if opts.get("add") else None
    g = torch.randn(oshape, generator=gen).to(dtype)
    return x, w, b, add, g


def truth_of(geometry, x, w, b, add, g, slope=None):
    """dict of y, gx, gw, gb in float64 (frames-major) and Sy, Sx, Sw, Sb, the same from absolute values"""
    dact = torch.ones(x.shape, dtype=torch.float64) if slope is None else \
        torch.where(x.float() > 0, 1.0, float(torch.tensor(slope, dtype=torch.float32))).double()

    def run(a64, w64, b64, add64, g64):
        a64, w64, b64 = a64.clone().requires_grad_(), w64.clone().requires_grad_(), b64.clone().requires_grad_()
        y = torch_layout(F.conv3d(torch_layout(a64), w64, b64, stride=STRIDE[geometry], padding=PADDING[geometry]))
        ga, gw, gb = torch.autograd.grad(y, (a64, w64, b64), g64)
        y = y.detach() if add64 is None else y.detach() + add64
        return y, ga * dact, gw, gb
    a64 = gu.activated(x, slope).double()
    w64, b64, g64 = w.double(), b.double(), g.double()
    add64 = None if add is None else add.double()
    y, gx, gw, gb = run(a64, w64, b64, add64, g64)
    Sy, Sx, Sw, Sb = run(a64.abs(), w64.abs(), b64.abs(), None if add64 is None else add64.abs(), g64.abs())
    return {"y": y, "gx": gx, "gw": gw, "gb": gb, "Sy": Sy, "Sx": Sx, "Sw": Sw, "Sb": Sb}


@functools.lru_cache(maxsize=None)
def truth(name, geometry, shape, opts_key):
    """computed once per case and shared: treat it as read-only"""
    return truth_of(geometry, *inputs(name, geometry, shape, opts_key), slope=dict(opts_key).get("slope"))


def bars_of(t, geometry, dtype, shape, has_add):
    B, L, C, Cout, H, W = shape
    lo, ho, wo = out_size(geometry, L, H, W)
    kk = K[geometry] ** 2
    kx = 3 * (9 if geometry == "k333" else 4) * Cout
    kw = B * lo * ho * wo
    return {"y": gu.bar(t["Sy"], t["y"], 3 * kk * C, dtype, has_add), "gx": gu.bar(t["Sx"], t["gx"], kx, dtype, False),
            "gw": gu.bar(t["Sw"], t["gw"], kw, torch.float32, False), "gb": gu.bar(t["Sb"], t["gb"], kw, torch.float32, False)}


def bars(name, geometry, shape, opts_key):
    return bars_of(truth(name, geometry, shape, opts_key), geometry, gu.DTYPES[name], shape, bool(dict(opts_key).get("add")))


def leaves(name, geometry, shape, opts_key, device="cuda", needs=(True, True, True, True)):
    """fresh leaf tensors (x, w, b, add | None) of a case on `device`, and the upstream gradient"""
    x, w, b, add, g = inputs(name, geometry, shape, opts_key)
    made = [None if t is None else t.detach().clone().to(device).requires_grad_(n) for t, n in zip((x, w, b, add), needs)]
    return made, g.to(device)


# ---- the pool ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_inputs(name, shape):
    B, L, C, H, W = shape
    gen = torch.Generator().manual_seed(sum(shape))
    def away_from_zero(t):                             # magnitudes >= 0.25, either sign (the module docstring, "pool")
        return (torch.where(t < 0, -0.25, 0.25) + t).to(gu.DTYPES[name])
    x = away_from_zero(torch.randn(shape, generator=gen))
    g = away_from_zero(torch.randn(B, L - 2, C, H // 2, W // 2, generator=gen))
    return x, g


def pool_truth_of(x, g):
    def run(x64, g64):
        x64 = x64.clone().requires_grad_()
        p = torch_layout(F.avg_pool3d(torch_layout(x64), (3, 2, 2), (1, 2, 2)))
        return p.detach(), torch.autograd.grad(p, x64, g64)[0]
    p, gx = run(x.double(), g.double())
    Sp, Sx = run(x.double().abs(), g.double().abs())
    return {"p": p, "gx": gx, "Sp": Sp, "Sx": Sx}


@functools.lru_cache(maxsize=None)
def pool_truth(name, shape):
    return pool_truth_of(*pool_inputs(name, shape))


def pool_bars_of(t, dtype):
    u = gu.UNIT[dtype]
    return {"p": u * t["p"].abs() + 14 * 2.0 ** -24 * t["Sp"], "gx": u * t["gx"].abs() + 14 * 2.0 ** -24 * t["Sx"]}


# ---- the window rule, emulated on the host (the twin of csrc/conv_igemm.h's WIN variant) --------------------------------------
def window_forward(x, w, b, geometry):
    """y (B,Lout,Cout,Ho,Wo) from frames-major x by the window rule: sample (b, lo) is F.conv2d of the channels [clo, chi)
    of the 3 C channel window that starts at frame lo - pt, with the weight w.permute(0,2,1,3,4) as (Cout, 3 C, k, k)"""
    B, L, C, H, W = x.shape
    k, pt = K[geometry], PADDING[geometry][0]
    lout = out_size(geometry, L, H, W)[0]
    wf = w.permute(0, 2, 1, 3, 4).reshape(w.size(0), 3 * C, k, k)
    flat = x.reshape(B, L * C, H, W)
    out = []
    for lo in range(lout):
        f0 = lo - pt
        clo, chi = max(0, -f0) * C, min(3, L - f0) * C
        start = f0 * C                                   # may be negative: channels below clo are never addressed
        part = flat[:, start + clo:start + chi]
        out.append(F.conv2d(part, wf[:, clo:chi], b, stride=STRIDE[geometry][1], padding=1))
    return torch.stack(out, 1)


def window_grad_x(g, w, geometry, L, H, W):
    """grad_x (B,L,C,H,W) from frames-major g (B,Lout,Cout,Ho,Wo): sample (b, l) is the adjoint 2-D convolution over the
    window of 3 frames of g that starts at frame l - (2 - pt), clipped to [0, Lout), with the temporal taps reversed:
    row j Cout + co of the gradient weight is w[co][.][2 - j]"""
    B, lout, cout = g.shape[:3]
    C, k, pt = w.size(1), K[geometry], PADDING[geometry][0]
    wg = w.flip(2).permute(2, 0, 1, 3, 4).reshape(3 * cout, C, k, k)
    flat = g.reshape(B, lout * cout, g.size(3), g.size(4))
    s = STRIDE[geometry][1]
    out = []
    for l in range(L):
        f0 = l - (2 - pt)
        clo, chi = max(0, -f0) * cout, min(3, lout - f0) * cout
        start = f0 * cout
        part = flat[:, start + clo:start + chi]
        out.append(torch.nn.grad.conv2d_input((B, C, H, W), wg[clo:chi], part, stride=s, padding=1))
    return torch.stack(out, 1)


# ---- stand-in networks -------------------------------------------------------------------------------------------------
def standin_classes():
    """Fresh (Block3D, TemporalDiscriminator) classes, so that a test can wrap their methods without touching another's.
    Block3D: model = Sequential(act, sn(Conv3d k333), act, sn(Conv3d k344)), shortcut = Sequential(AvgPool3d((3,2,2),
    (1,2,2)), sn(Conv3d 1x1x1)), forward model(x) + shortcut(x) on torch's (B,C,L,H,W).  TemporalDiscriminator: block0,
    block1, the frames folded into the channels, `layers - 2` 2-D encoder blocks (discriminator_util.Block), act, final
    sn(Conv2d 1x1)."""

    class Block3D(nn.Module):
        def __init__(self, cin, cout, hidden, norm=None, pool=(3, 2, 2)):
            super(Block3D, self).__init__()
            conv1 = sn(nn.Conv3d(cin, hidden, (3, 3, 3), (1, 1, 1), (1, 1, 1)))
            conv2 = sn(nn.Conv3d(hidden, cout, (3, 4, 4), (1, 2, 2), (0, 1, 1)))
            if norm is None:
                self.model = nn.Sequential(nn.LeakyReLU(0.1), conv1, nn.LeakyReLU(0.1), conv2)
            else:
                self.model = nn.Sequential(norm(cin), nn.LeakyReLU(0.1), conv1, norm(hidden), nn.LeakyReLU(0.1), conv2)
            self.shortcut = nn.Sequential(nn.AvgPool3d(pool, (1, 2, 2)), sn(nn.Conv3d(cin, cout, 1)))

        def forward(self, x):
            return self.model(x) + self.shortcut(x)

    class TemporalDiscriminator(nn.Module):
        def __init__(self, input_nc=3, input_length=6, ndf=8, layers=3):
            super(TemporalDiscriminator, self).__init__()
            self.layers = layers
            self.nonlinearity = nn.LeakyReLU(0.1)
            self.block0 = Block3D(input_nc, ndf, ndf)
            self.block1 = Block3D(ndf, 2 * ndf, ndf)
            width = 2 * ndf * (input_length - 4)
            for i in range(layers - 2):
                setattr(self, "encoder" + str(i), du.Block(width, width))
            self.conv = sn(nn.Conv2d(width, 1, 1))

        def forward(self, x):
            out = self.block1(self.block0(x))
            b, c, l, h, w = out.shape
            out = out.view(b, -1, h, w)
            for i in range(self.layers - 2):
                out = getattr(self, "encoder" + str(i))(out)
            return self.conv(self.nonlinearity(out))

    return Block3D, TemporalDiscriminator


Block3D, TemporalDiscriminator = standin_classes()
VIDEO = (1, 3, 6, 32, 32)                              # torch's (B, C, L, H, W)


def temporal_discriminators(device, copies=2, seed=31, cls=None):
    """(`copies` float32 networks on `device` with equal parameters and buffers, float64 host network, two videos), all in
    train() mode"""
    cls = cls or TemporalDiscriminator
    torch.manual_seed(seed)
    host = TemporalDiscriminator()
    state = host.state_dict()
    nets = []
    for _ in range(copies):
        net = cls()
        net.load_state_dict(state)
        nets.append(net.to(device).train())
    g = torch.Generator().manual_seed(seed + 1)
    videos = [torch.rand(VIDEO, generator=g) * 2 - 1 for _ in range(2)]
    return nets, host.double().train(), videos


def hooked_convs(net):
    return [m for m in net.modules() if type(m) in (nn.Conv2d, nn.Conv3d) and "weight_orig" in m._parameters]
