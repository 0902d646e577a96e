"""Shared by the generator-convolution tests: float64 host references built from the very tensors the kernels read, the
derived error bar, a pure-Python emulation of the three packed index maps of csrc/conv_igemm.h and of what the kernel
computes from a packed array, and generator-shaped blocks (the documented structures of the reference's EncoderBlock,
ResBlock, ResBlockDecoder, Jump and Output, written here: none of the reference's code)."""
import torch
import torch.nn.functional as F
from torch import nn

S1K3, S2K4, T2K3 = 0, 1, 2
TAPS = {S1K3: 9, S2K4: 16, T2K3: 9}
UNIT = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def out_size(geometry, H, W):
    return (H, W) if geometry == S1K3 else ((H - 2) // 2 + 1, (W - 2) // 2 + 1) if geometry == S2K4 else (2 * H, 2 * W)


def reduction_length(geometry, cin):
    """K of the bar: products per output element (T2K3: the deepest phase, four taps)"""
    return {S1K3: 9, S2K4: 16, T2K3: 4}[geometry] * cin


def activated(x, pre_slope):
    """act(x) as the torch composition hands it to its convolution: computed by torch in x's dtype on the host"""
    x = x.detach().cpu()
    return x if pre_slope is None else F.leaky_relu(x, pre_slope)


def _conv64(a, w, b, geometry, reflect):
    if geometry == S1K3 and reflect:
        return F.conv2d(F.pad(a, (1, 1, 1, 1), mode="reflect"), w, b)
    if geometry == S1K3:
        return F.conv2d(a, w, b, padding=1)
    if geometry == S2K4:
        return F.conv2d(a, w, b, stride=2, padding=1)
    return F.conv_transpose2d(a, w, b, stride=2, padding=1, output_padding=1)


def ref64(geometry, x, w, b=None, reflect=False, pre_slope=None, add=None):
    """(y64, S): y = bias + conv(act(x), w) (+ add) in float64 from the stored values, and S = the same convolution of
    |act(x)| with |w|, plus |b| and |add|"""
    a = activated(x, pre_slope).double()
    w = w.detach().cpu().double()
    b = None if b is None else b.detach().cpu().double()
    y = _conv64(a, w, b, geometry, reflect)
    S = _conv64(a.abs(), w.abs(), None if b is None else b.abs(), geometry, reflect)
    if add is not None:
        add = add.detach().cpu().double()
        y, S = y + add, S + add.abs()
    return y, S


def bar(S, y64, K, dtype, has_add):
    """|y - y64| <= 2 (K + 2 + a) 2^-24 S + u |y64|: K products, a bias and (a = 1) an addend summed in float32 in an order
    of the kernel's own, then the one rounding of a 16-bit result"""
    return 2.0 * (K + 2 + (1 if has_add else 0)) * 2.0 ** -24 * S + UNIT[dtype] * y64.abs()


# ---- the per-call cases and their seeded host inputs (test_gen_conv_gpu.py, conv_family_util.py) ----------------------
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
ALL = ("f32", "f16", "bf16")


def _cases(rows, deep):
    """(dtype name, shape, options) for every row in every dtype, plus the longest reduction in float32 and bfloat16"""
    return [(n, s, o) for s, o in rows for n in ALL] + [(n, deep, {}) for n in ("f32", "bf16")]


def case_id(v):
    if isinstance(v, str):
        return v
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    return "-".join(sorted(k if v[k] is True else "%s%s" % (k, v[k]) for k in v)) or "plain"


# (B, Cin, Cout, H, W): first layer with one padded chunk; nothing a multiple of anything, tiles straddle both edges; all
# halo; a map of two rows; several channel chunks and channel blocks with activation and addend
S1K3_CASES = _cases([((1, 3, 64, 9, 7), {}), ((2, 20, 40, 33, 17), {}), ((2, 20, 40, 33, 17), {"reflect": True}),
                     ((1, 64, 64, 1, 1), {}), ((1, 16, 32, 2, 40), {"reflect": True}),
                     ((3, 128, 96, 16, 11), {"reflect": True, "slope": 0.1, "add": True})], (1, 512, 512, 4, 3))
# odd both ways; the smallest map (one output pixel); three rows (the last one dropped) and more than two tiles across
S2K4_CASES = _cases([((1, 3, 64, 10, 8), {}), ((2, 20, 40, 33, 17), {"slope": 0.1}), ((1, 21, 32, 2, 2), {}),
                     ((1, 64, 64, 3, 70), {}), ((3, 128, 96, 16, 22), {})], (1, 512, 512, 8, 6))
# one input pixel; odd sizes over several tiles with an addend; one row; the addend aliasing the output
T2K3_CASES = _cases([((1, 5, 7, 1, 1), {}), ((2, 20, 40, 17, 9), {"add": True}), ((1, 16, 32, 1, 40), {}),
                     ((3, 128, 96, 8, 11), {"alias": True})], (1, 512, 512, 4, 3))


def conv_inputs(geometry, shape, dtype, seed, with_add):
    B, Cin, Cout, H, W = shape
    k = 4 if geometry == S2K4 else 3
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g).to(dtype)
    wshape = (Cin, Cout, k, k) if geometry == T2K3 else (Cout, Cin, k, k)
    fan = (4 if geometry == T2K3 else k * k) * Cin
    w = (torch.randn(wshape, generator=g) * (2.0 / fan) ** 0.5).to(dtype)      # rounded as the packing does
    b = (torch.randn(Cout, generator=g) * 0.2).to(dtype)
    add = torch.randn((B, Cout) + out_size(geometry, H, W), generator=g).to(dtype) if with_add else None
    return x, w, b, add


def call(gfla, geometry, x, w, b, reflect=False, slope=None, add=None):
    if geometry == S1K3:
        return gfla.conv3x3(x, w, b, padding="reflect" if reflect else "zeros", pre_slope=slope, add=add)
    if geometry == S2K4:
        return gfla.conv4x4_down(x, w, b, pre_slope=slope)
    return gfla.conv_transpose3x3_up(x, w, b, add=add, pre_slope=slope)


def call_in_place(x, w, b, add):
    """T2K3 through the C entry point with the addend's buffer as the output"""
    from global_flow_local_attention_amd import _lib, gen_conv
    x = x.contiguous()
    B, Cin, H, W = x.shape
    y = add.clone()
    wp = gen_conv.packed_weights(w, x.dtype, T2K3)
    _lib.call("gfla_gen_conv_fwd_" + _lib.SUFFIX[x.dtype], x, _lib.ptr(x), _lib.ptr(wp), _lib.ptr(b.float().contiguous()),
              _lib.ptr(y), _lib.ptr(y), B, Cin, w.size(1), H, W, T2K3, 0, 0, 0.0)
    return y


# ---- emulation of the packed layouts (csrc/conv_igemm.h: conv_igemm_pack_kernel, conv_igemm_kernel) ------------------
def packed_dims(cout, cin, ck):
    """(NCH, MP): chunks of the input channels and padded output channels"""
    return -(-cin // ck), -(-cout // 32) * 32


def pack_emulated(w, geometry, ck):
    """packed[tap][chunk][co][j] exactly as the pack kernel indexes torch's weight ((Cout,Cin,k,k); T2K3: (Cin,Cout,3,3)),
    as a float64 array"""
    taps = TAPS[geometry]
    cout, cin = (w.shape[1], w.shape[0]) if geometry == T2K3 else (w.shape[0], w.shape[1])
    nch, mp = packed_dims(cout, cin, ck)
    out = torch.zeros(taps, nch, mp, ck, dtype=torch.float64)
    flat = w.double().reshape(-1)
    for tap in range(taps):
        for k in range(cin):
            for m in range(cout):
                at = ((k * cout + m) if geometry == T2K3 else (m * cin + k)) * taps + tap
                out[tap, k // ck, m, k % ck] = flat[at]
    return out


def t2k3_tap(tap):
    """(phase, dy, dx) of a tap of T2K3: the output phase 2 [oy odd] + [ox odd] it feeds, and the input neighbour
    (i + dy, j + dx) it reads"""
    ky, kx = divmod(tap, 3)
    return 2 * int(ky != 1) + int(kx != 1), int(ky == 0), int(kx == 0)


def conv_from_packed(x, packed, geometry, cout, ck, reflect=False):
    """What the kernel computes from a packed array: the halo tile is x, zero (or mirrored) outside the image and zero
    beyond Cin; every tap multiplies its [co][chunk] slice with the tile at the tap's offset (S2K4: at stride 2; T2K3: into
    the tap's output phase)."""
    b, cin, h, w = x.shape
    nch = packed.shape[1]
    ho, wo = out_size(geometry, h, w)
    xc = torch.zeros(b, nch * ck, h, w, dtype=torch.float64)
    xc[:, :cin] = x.double()
    out = torch.zeros(b, packed.shape[2], ho, wo, dtype=torch.float64)
    if geometry == S1K3:
        xp = F.pad(xc, (1, 1, 1, 1), mode="reflect") if reflect else F.pad(xc, (1, 1, 1, 1))
        xp = xp.reshape(b, nch, ck, h + 2, w + 2)
        for tap in range(9):
            ky, kx = divmod(tap, 3)
            out += torch.einsum("cmj,bcjyx->bmyx", packed[tap], xp[:, :, :, ky:ky + h, kx:kx + w])
    elif geometry == S2K4:
        xp = F.pad(xc, (1, 2 * wo + 2 - w - 1, 1, 2 * ho + 2 - h - 1)).reshape(b, nch, ck, 2 * ho + 2, 2 * wo + 2)
        for tap in range(16):
            ky, kx = divmod(tap, 4)
            out += torch.einsum("cmj,bcjyx->bmyx", packed[tap], xp[:, :, :, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2])
    else:
        xp = F.pad(xc, (0, 1, 0, 1)).reshape(b, nch, ck, h + 1, w + 1)
        for tap in range(9):
            phase, dy, dx = t2k3_tap(tap)
            out[:, :, phase // 2::2, phase % 2::2] += torch.einsum("cmj,bcjyx->bmyx", packed[tap],
                                                                   xp[:, :, :, dy:dy + h, dx:dx + w])
    return out[:, :cout]


# ---- generator-shaped blocks ---------------------------------------------------------------------------------------------
def _norm(c):
    return nn.InstanceNorm2d(c)


class EncoderBlock(nn.Module):
    """norm -> act -> conv4x4/2 -> norm -> act -> conv3x3"""

    def __init__(self, cin, cout, act):
        super(EncoderBlock, self).__init__()
        self.model = nn.Sequential(_norm(cin), act, nn.Conv2d(cin, cout, 4, 2, 1), _norm(cout), act, nn.Conv2d(cout, cout, 3, 1, 1))

    def forward(self, x):
        return self.model(x)


class ResBlock(nn.Module):
    """x + (norm -> act -> conv3x3 -> norm -> act -> conv3x3)(x)"""

    def __init__(self, c, act):
        super(ResBlock, self).__init__()
        self.model = nn.Sequential(_norm(c), act, nn.Conv2d(c, c, 3, 1, 1), _norm(c), act, nn.Conv2d(c, c, 3, 1, 1))

    def forward(self, x):
        last = self.model[5]
        if hasattr(last, "geometry"):                 # an InferenceConv: the residual goes into its epilogue
            return last(self.model[:5](x), x)
        return self.model(x) + x


class DecoderBlock(nn.Module):
    """(norm -> act -> conv3x3 -> norm -> act -> transposed conv) + transposed shortcut"""

    def __init__(self, cin, cout, act):
        super(DecoderBlock, self).__init__()
        self.model = nn.Sequential(_norm(cin), act, nn.Conv2d(cin, cin, 3, 1, 1), _norm(cin), act,
                                   nn.ConvTranspose2d(cin, cout, 3, 2, 1, output_padding=1))
        self.shortcut = nn.Sequential(nn.ConvTranspose2d(cin, cout, 3, 2, 1, output_padding=1))

    def forward(self, x):
        last = self.model[5]
        if hasattr(last, "geometry"):
            return last(self.model[:5](x), self.shortcut(x))
        return self.model(x) + self.shortcut(x)


class Jump(nn.Module):
    """act -> reflect pad -> conv3x3, the convolution also registered as `conv1`"""

    def __init__(self, c, act):
        super(Jump, self).__init__()
        self.conv1 = nn.Conv2d(c, c, 3, padding=0)
        self.model = nn.Sequential(act, nn.ReflectionPad2d(1), self.conv1)

    def forward(self, x):
        return self.model(x)


class Output(nn.Module):
    """act -> reflect pad -> conv3x3 to 3 channels -> tanh"""

    def __init__(self, c, act):
        super(Output, self).__init__()
        self.model = nn.Sequential(act, nn.ReflectionPad2d(1), nn.Conv2d(c, 3, 3, padding=0), nn.Tanh())

    def forward(self, x):
        return self.model(x)


class StandInGenerator(nn.Module):
    """A generator-shaped network around one attention layer: a source encoder, a target encoder, attention at the
    coarsest level, a residual block, two decoder blocks with a jump connection, an image head.  attn_cls(channels,
    kernel_size, activation, softmax=True) -> module(source, target, flow)."""

    def __init__(self, attn_cls, widths=(8, 16, 32), structure_nc=6):
        super(StandInGenerator, self).__init__()
        act = nn.LeakyReLU(0.1)
        w0, w1, w2 = widths
        self.source = nn.Sequential(EncoderBlock(3, w0, act), EncoderBlock(w0, w1, act), EncoderBlock(w1, w2, act))
        self.enc0, self.enc1, self.enc2 = EncoderBlock(structure_nc, w0, act), EncoderBlock(w0, w1, act), EncoderBlock(w1, w2, act)
        self.attn = attn_cls(w2, 3, act, softmax=True)
        self.res = ResBlock(w2, act)
        self.dec0, self.dec1, self.dec2 = DecoderBlock(w2, w1, act), DecoderBlock(w1, w0, act), DecoderBlock(w0, w0, act)
        self.jump = Jump(w1, act)
        self.out = Output(w0, act)

    def forward(self, image, pose, flow):
        f = self.source(image)
        e1 = self.enc1(self.enc0(pose))
        t = self.enc2(e1)
        t = self.res(t + self.attn(f, t, flow))
        return self.out(self.dec2(self.dec1(self.dec0(t) + self.jump(e1))))
