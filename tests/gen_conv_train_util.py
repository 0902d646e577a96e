"""Shared by the tests of the generator convolutions' gradients (gen_conv.GenConvFunction; csrc/gen_conv_bwd.hip,
csrc/gen_conv_wgrad.hip): the float64 host gradients with their derived bars, a pure-Python emulation of the three adjoint
packings and of what the data-gradient kernels compute from a packed array, and a convolution-only generator-shaped
network built from gen_conv_util's blocks."""
import torch
import torch.nn.functional as F
from torch import nn

import gen_conv_util as gu
from gen_conv_util import S1K3, S2K4, T2K3

ADJ_TAPS = {S1K3: 9, S2K4: 16, T2K3: 9}


def _cases(rows, deep):
    return [(n, s, o) for s, o in rows for n in gu.ALL] + [(n, deep, {}) for n in ("f32", "bf16")]


# (B, Cin, Cout, H, W): the forward's shapes -- one padded chunk, tiles straddling both edges, all halo, two rows that fold
# onto each other, several chunks and channel blocks with activation and addend, the longest reduction
S1K3_CASES = _cases([((1, 3, 64, 9, 7), {}), ((2, 20, 40, 33, 17), {}), ((2, 20, 40, 33, 17), {"reflect": True}),
                     ((1, 64, 64, 1, 1), {}), ((1, 16, 32, 2, 40), {"reflect": True}),
                     ((3, 128, 96, 16, 11), {"slope": 0.1, "add": True}),
                     ((3, 128, 96, 16, 11), {"reflect": True, "slope": 0.1, "add": True})], (1, 512, 512, 4, 3))
S2K4_CASES = _cases([((1, 3, 64, 10, 8), {}), ((2, 20, 40, 33, 17), {"slope": 0.1}), ((1, 21, 32, 2, 2), {}),
                     ((1, 64, 64, 3, 70), {}), ((3, 128, 96, 16, 22), {})], (1, 512, 512, 8, 6))
T2K3_CASES = _cases([((1, 5, 7, 1, 1), {}), ((2, 20, 40, 17, 9), {"add": True}), ((1, 16, 32, 1, 40), {}),
                     ((3, 128, 96, 8, 11), {"slope": 0.1})], (1, 512, 512, 4, 3))


def data_reduction_length(geometry, cout):
    """K of grad_x's bar: products per element (S2K4: one phase of 2 x 2 taps)"""
    return {S1K3: 9, S2K4: 4, T2K3: 9}[geometry] * cout


def weight_reduction_length(geometry, shape):
    B, _, _, H, W = shape
    ho, wo = gu.out_size(geometry, H, W)
    return B * ho * wo if geometry == S2K4 else B * H * W


def upstream(geometry, shape, dtype, seed):
    """grad_y in the map's dtype"""
    B, _, Cout, H, W = shape
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn((B, Cout) + gu.out_size(geometry, H, W), generator=g).to(dtype)


def grads64(geometry, x, w, b, g, reflect=False, slope=None):
    """((grad_x64, grad_w64, grad_b64), (S_x, S_w, S_b)): torch.autograd.grad of the float64 composition at (act(x), w, b)
    with upstream g, grad_x64 = grad_a64 act'(x) with act'(x) = x > 0 ? 1 : float32(slope); S: the same from |g|, |a|, |w|"""
    a = gu.activated(x, slope).double()
    w, b, g = w.detach().cpu().double(), b.detach().cpu().double(), g.detach().cpu().double()
    dact = torch.ones_like(a) if slope is None else \
        torch.where(x.detach().cpu().float() > 0, 1.0, float(torch.tensor(slope, dtype=torch.float32))).double()

    def run(a, w, b, g):
        a, w, b = a.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        ga, gw, gb = torch.autograd.grad(gu._conv64(a, w, b, geometry, reflect), (a, w, b), g)
        return ga * dact, gw, gb
    return run(a, w, b, g), run(a.abs(), w.abs(), b.abs(), g.abs())


# ---- emulation of the adjoint packings and of the data-gradient kernels (csrc/gen_conv_bwd.hip) ----------------------
def pack_grad_emulated(w, geometry, ck):
    """packed[tap][chunk of Cout][ci padded to 32][j] exactly as gfla_gen_conv_pack_grad_weights indexes torch's weight:
    S1K3 transposed with the taps mirrored, S2K4 transposed with the taps as stored, T2K3 as stored"""
    taps = ADJ_TAPS[geometry]
    cout, cin = (w.shape[1], w.shape[0]) if geometry == T2K3 else (w.shape[0], w.shape[1])
    nch, mp = -(-cout // ck), -(-cin // 32) * 32
    out = torch.zeros(taps, nch, mp, ck, dtype=torch.float64)
    flat = w.double().reshape(-1)
    for tap in range(taps):
        src = taps - 1 - tap if geometry == S1K3 else tap
        for k in range(cout):
            for m in range(cin):
                at = ((m * cout + k) if geometry == T2K3 else (k * cin + m)) * taps + src
                out[tap, k // ck, m, k % ck] = flat[at]
    return out


def u2k4_tap(tap):
    """(phase, oy, ox) of a tap of the S2K4 adjoint: the phase 2 [row odd] + [column odd] of x it feeds and the pixel
    (i + oy, j + ox) of g it reads"""
    ky, kx = divmod(tap, 4)
    off = {0: 1, 1: 0, 2: 0, 3: -1}
    return 2 * int(ky % 2 == 0) + int(kx % 2 == 0), off[ky], off[kx]


def fold_reflect(gp):
    """(B,C,H+2,W+2) on the padded domain -> (B,C,H,W): padded row -1 onto row 1, padded row H onto row H - 2, columns
    likewise"""
    H, W = gp.shape[2] - 2, gp.shape[3] - 2
    rows = gp[:, :, 1:H + 1].clone()
    rows[:, :, 1] += gp[:, :, 0]
    rows[:, :, H - 2] += gp[:, :, H + 1]
    out = rows[:, :, :, 1:W + 1].clone()
    out[:, :, :, 1] += rows[:, :, :, 0]
    out[:, :, :, W - 2] += rows[:, :, :, W + 1]
    return out


def grad_a_from_packed(g, packed, geometry, cin, ck, H, W, reflect=False):
    """What the data-gradient kernels compute from a packed array, before act'(x): g is zero outside its map and beyond
    Cout; every tap multiplies its [ci][chunk] slice with g at the tap's offset."""
    b, cout, hg, wg = g.shape
    nch = packed.shape[1]
    gc = torch.zeros(b, nch * ck, hg, wg, dtype=torch.float64)
    gc[:, :cout] = g.double()
    if geometry == S1K3:
        p = 2 if reflect else 1                     # reflect: the output is the padded domain, one pixel further out
        oh, ow = H + 2 * (p - 1), W + 2 * (p - 1)
        gp = F.pad(gc, (p, p, p, p)).reshape(b, nch, ck, H + 2 * p, W + 2 * p)
        out = torch.zeros(b, packed.shape[2], oh, ow, dtype=torch.float64)
        for tap in range(9):
            ky, kx = divmod(tap, 3)
            out += torch.einsum("cmj,bcjyx->bmyx", packed[tap], gp[:, :, :, ky:ky + oh, kx:kx + ow])
        out = fold_reflect(out) if reflect else out
    elif geometry == S2K4:
        th, tw = (H + 1) // 2, (W + 1) // 2         # the half-resolution grid
        gp = F.pad(gc, (1, tw + 1 - wg, 1, th + 1 - hg)).reshape(b, nch, ck, th + 2, tw + 2)
        out = torch.zeros(b, packed.shape[2], 2 * th, 2 * tw, dtype=torch.float64)
        for tap in range(16):
            phase, oy, ox = u2k4_tap(tap)
            out[:, :, phase // 2::2, phase % 2::2] += torch.einsum(
                "cmj,bcjyx->bmyx", packed[tap], gp[:, :, :, 1 + oy:1 + oy + th, 1 + ox:1 + ox + tw])
        out = out[:, :, :H, :W]
    else:
        gp = F.pad(gc, (1, 0, 1, 0)).reshape(b, nch, ck, 2 * H + 1, 2 * W + 1)
        out = torch.zeros(b, packed.shape[2], H, W, dtype=torch.float64)
        for tap in range(9):
            ky, kx = divmod(tap, 3)
            out += torch.einsum("cmj,bcjyx->bmyx", packed[tap], gp[:, :, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2])
    return out[:, :cin]


# ---- a convolution-only generator-shaped network ---------------------------------------------------------------------
class ConvGenerator(nn.Module):
    """Three encoder blocks, a residual block, three decoder blocks with a jump connection and an image head: every
    convolution geometry of the generators' bodies, and nothing but convolutions, norms and activations"""

    def __init__(self, widths=(8, 16, 32)):
        super(ConvGenerator, self).__init__()
        act = nn.LeakyReLU(0.1)
        w0, w1, w2 = widths
        self.enc0, self.enc1, self.enc2 = gu.EncoderBlock(3, w0, act), gu.EncoderBlock(w0, w1, act), gu.EncoderBlock(w1, w2, act)
        self.res = gu.ResBlock(w2, act)
        self.dec0, self.dec1, self.dec2 = gu.DecoderBlock(w2, w1, act), gu.DecoderBlock(w1, w0, act), gu.DecoderBlock(w0, w0, act)
        self.jump = gu.Jump(w1, act)
        self.out = gu.Output(w0, act)

    def forward(self, image):
        e1 = self.enc1(self.enc0(image))
        t = self.res(self.enc2(e1))
        return self.out(self.dec2(self.dec1(self.dec0(t) + self.jump(e1))))


def conv_generators(device, copies=2):
    """(GPU float32 networks with the same parameters, float64 host network, input (2, 3, 32, 24)), all in train() mode"""
    torch.manual_seed(11)
    host = ConvGenerator()
    state = host.state_dict()
    nets = []
    for _ in range(copies):
        net = ConvGenerator()
        net.load_state_dict(state)
        nets.append(net.to(device).train())
    g = torch.Generator().manual_seed(12)
    return nets, host.double().train(), torch.rand(2, 3, 32, 24, generator=g) * 2 - 1


def rewrite(gfla, net):
    """the three rewrites of the generator, the convolutions with their gradients on the kernels"""
    return (gfla.fuse_instance_norm_act(net), gfla.fuse_output_heads(net), gfla.fuse_inference_convs(net, grad="kernels"))
