"""Shared by the VGG19 tests: the golden file, float64 host references with the derived error bars of the issue, an
emulation of the packed-weight index maps of csrc/conv_igemm.h, and torchvision's configuration-E `features` stack."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vgg_golden.npz")
GOLDEN_WIDTHS = (4, 4, 8, 8, 8)
GOLDEN_IMAGES = ("a", "b")          # (2, 3, 32, 24) and (1, 3, 19, 21)
LAYERS = ("relu1_1", "relu1_2", "relu2_1", "relu2_2", "relu3_1", "relu3_2", "relu3_3", "relu3_4",
          "relu4_1", "relu4_2", "relu4_3", "relu4_4", "relu5_1", "relu5_2", "relu5_3", "relu5_4")
# the reference's state-dict keys (external_function.py:348-394), without .weight / .bias
PARAM_PREFIXES = ("relu1_1.0", "relu1_2.2", "relu2_1.5", "relu2_2.7", "relu3_1.10", "relu3_2.12", "relu3_2.14", "relu3_4.16",
                  "relu4_1.19", "relu4_2.21", "relu4_3.23", "relu4_4.25", "relu5_1.28", "relu5_2.30", "relu5_3.32",
                  "relu5_4.34")
STATE_KEYS = tuple("%s.%s" % (p, w) for p in PARAM_PREFIXES for w in ("weight", "bias"))
CFG_E = (1, 1, "M", 2, 2, "M", 3, 3, 3, 3, "M", 4, 4, 4, 4, "M", 5, 5, 5, 5, "M")   # stage of every convolution
UNIT = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def torchvision_features(widths, seed, gain=1.0, bias_scale=0.1):
    """The 37-module `features` Sequential of torchvision's vgg19 at the given stage widths: He-scaled random weights
    (times gain), small random biases, seeded."""
    gen = torch.Generator().manual_seed(seed)
    mods, cin = [], 3
    for v in CFG_E:
        if v == "M":
            mods.append(torch.nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        conv = torch.nn.Conv2d(cin, widths[v - 1], kernel_size=3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * gain * (2.0 / (9 * cin)) ** 0.5)
            conv.bias.copy_(torch.randn(conv.bias.shape, generator=gen) * bias_scale)
        mods += [conv, torch.nn.ReLU(inplace=True)]
        cin = widths[v - 1]
    assert len(mods) == 37
    return torch.nn.Sequential(*mods)


def load_golden():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def golden_state_dict(gold, dtype=torch.float64):
    return {k: gold["param/" + k].to(dtype) for k in STATE_KEYS}


def conv_ref64(x, w, b):
    """(relu(conv(x, w) + b), S = conv(|x|, |w|) + |b|) in float64 on the host, from the stored values"""
    x, w, b = (t.detach().cpu().double() for t in (x, w, b))
    y = F.relu(F.conv2d(x, w, b, padding=1))
    return y, F.conv2d(x.abs(), w.abs(), b.abs(), padding=1)


def conv_bar(S, y64, K, dtype):
    """the issue's forward bar: 2 (K + 2) 2^-24 S + u |y64|"""
    return 2.0 * (K + 2) * 2.0 ** -24 * S + UNIT[dtype] * y64.abs()


def dgrad_ref64(g, y_kernel, w):
    """(dX, S) of the data gradient in float64: conv_transpose of g [y_kernel > 0], the mask from the kernel's own
    saved output"""
    g, w = g.detach().cpu().double(), w.detach().cpu().double()
    gm = g * (y_kernel.detach().cpu().double() > 0)
    return F.conv_transpose2d(gm, w, padding=1), F.conv_transpose2d(gm.abs(), w.abs(), padding=1)


def conv_inputs(shape, dtype, seed):
    B, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g).to(dtype)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5).to(dtype)   # rounded as the packing does
    b = (torch.randn(Cout, generator=g) * 0.2).to(dtype)
    gy = torch.randn(B, Cout, H, W, generator=g).to(dtype)
    return x, w, b, gy


# ---- emulation of the packed layouts (csrc/conv_igemm.h: conv_igemm_pack_kernel) -------------------------------------
def packed_dims(cout, cin, layout, ck):
    """(NCH, MP): chunks of the reduction axis and padded result channels"""
    m, k = (cin, cout) if layout else (cout, cin)
    return -(-k // ck), -(-m // 32) * 32


def pack_emulated(w, layout, ck):
    """packed[tap][chunk][m][j] exactly as the kernel indexes it, as a float64 array"""
    cout, cin = w.shape[:2]
    nch, mp = packed_dims(cout, cin, layout, ck)
    m_n, k_n = (cin, cout) if layout else (cout, cin)
    out = torch.zeros(9, nch, mp, ck, dtype=torch.float64)
    flat = w.double().reshape(cout, cin, 9)
    for tap in range(9):
        for k in range(k_n):
            for m in range(m_n):
                co, ci, tp = (k, m, 8 - tap) if layout else (m, k, tap)
                out[tap, k // ck, m, k % ck] = flat[co, ci, tp]
    return out


def conv_from_packed(x, packed, m_n, ck):
    """What the kernel computes from a packed array: out[b, m, p] = sum over tap, chunk, j of
    packed[tap, chunk, m, j] * x[b, chunk ck + j, p + tap], x zero-padded in space and in channels."""
    b, k_n, h, w = x.shape
    nch = packed.shape[1]
    xp = torch.zeros(b, nch * ck, h + 2, w + 2, dtype=torch.float64)
    xp[:, :k_n, 1:-1, 1:-1] = x.double()
    xp = xp.reshape(b, nch, ck, h + 2, w + 2)
    out = torch.zeros(b, packed.shape[2], h, w, dtype=torch.float64)
    for tap in range(9):
        ty, tx = divmod(tap, 3)
        out += torch.einsum("cmj,bcjyx->bmyx", packed[tap], xp[:, :, :, ty:ty + h, tx:tx + w])
    return out[:, :m_n]


class TorchVGG(object):
    """The network as a plain torch composition (F.conv2d / F.max_pool2d) from a state dict with the reference's keys:
    the yardstick the float32 bar of the golden test is measured with.  Shares no code with the package."""

    # output name(s) of the sixteen convolutions in order; the second of stage 3 (features[12]) has none (:363-370)
    NAMES = (("relu1_1",), ("relu1_2",), ("relu2_1",), ("relu2_2",), ("relu3_1",), (), ("relu3_2", "relu3_3"),
             ("relu3_4",), ("relu4_1",), ("relu4_2",), ("relu4_3",), ("relu4_4",), ("relu5_1",), ("relu5_2",),
             ("relu5_3",), ("relu5_4",))
    POOL_BEFORE = (2, 4, 8, 12)

    def __init__(self, state):
        self.state = state

    def __call__(self, x):
        out = {}
        for k, prefix in enumerate(PARAM_PREFIXES):
            if k in self.POOL_BEFORE:
                x = F.max_pool2d(x, kernel_size=2, stride=2)
            x = F.relu(F.conv2d(x, self.state[prefix + ".weight"], self.state[prefix + ".bias"], padding=1))
            for name in self.NAMES[k]:
                out[name] = x
        return {name: out[name] for name in LAYERS}
