"""Shared by the tests of spectrally normalised generators (spectral_norm.py: dim-1 matrices in the batched op,
SpectralConvTranspose, the reflect-padded SpectralConv, SpectralHead, fuse_spectral_norm(generator=True)): dim-1 weights
with the float64 truth and torch's own hook as the float32 baseline, and a generator-shaped network of plain torch modules
under torch.nn.utils.spectral_norm -- the documented structure of the reference's blocks, none of its code."""
import torch
from torch import nn
from torch.nn.utils import spectral_norm as sn

import discriminator_util as du

# (Cin, Cout, k) of a transposed convolution's weight (Cin, Cout, k, k), normalised along dim 1: a matrix of one row; tails
# in both directions; fewer rows than a wave; a middle layer; the largest of the pose generator; inner 16; inner 1
DIM1 = ((3, 1, 3), (5, 7, 3), (8, 3, 3), (64, 32, 3), (256, 128, 3), (6, 10, 4), (12, 5, 1))
IMAGE = (2, 3, 20, 12)       # the bottleneck is 5 x 3, odd both ways
WIDTHS = (8, 16)


# ---- a dim-1 weight --------------------------------------------------------------------------------------------------------
def to_matrix(w):
    """the hook's reshape_weight_to_matrix for dim 1: (Cin, Cout, kh, kw) -> (Cout, Cin kh kw)"""
    return w.permute(1, 0, 2, 3).reshape(w.size(1), -1)


def to_storage(m, shape):
    """a (Cout, Cin kh kw) matrix back in the weight's layout (Cin, Cout, kh, kw)"""
    cin, cout, kh, kw = shape
    return m.reshape(cout, cin, kh, kw).permute(1, 0, 2, 3).contiguous()


def dim1_inputs(cin, cout, k, seed, scale=None):
    """(W (Cin,Cout,k,k), u (Cout,), v (Cin k k,), G like W) float32 on the host, unit start vectors as the hook draws them"""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(cin, cout, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    if scale is not None:
        W = W * (scale / W.abs().max())
    u = torch.nn.functional.normalize(torch.randn(cout, generator=g), dim=0)
    v = torch.nn.functional.normalize(torch.randn(cin * k * k, generator=g), dim=0)
    return W, u, v, torch.randn(cin, cout, k, k, generator=g)


def all_dim1():
    return [dim1_inputs(cin, cout, k, seed=100 + cin + cout) for cin, cout, k in DIM1]


def truth64(W, u, v, G, iters, eps=1e-12):
    """The op's formulas in float64 on the permuted matrix, W_sn and grad_w mapped back to the weight's storage"""
    out = du.truth64(to_matrix(W), u, v, to_matrix(G), iters, eps)
    out["w_sn"], out["grad_w"] = to_storage(out["w_sn"], W.shape), to_storage(out["grad_w"], W.shape)
    return out


def hooked_transpose(W, u, v, iters, eps=1e-12, device="cpu"):
    """an nn.ConvTranspose2d under torch's hook (dim 1) holding W, u, v; and the hook object"""
    cin, cout, k, _ = W.shape
    conv = sn(nn.ConvTranspose2d(cin, cout, k, bias=False), n_power_iterations=max(iters, 1), eps=eps).to(device)
    hook = next(iter(conv._forward_pre_hooks.values()))
    assert hook.dim == 1
    with torch.no_grad():
        conv.weight_orig.copy_(W)
        conv.weight_u.copy_(u)
        conv.weight_v.copy_(v)
    return conv, hook


def hook_float32(W, u, v, G, iters, device, eps=1e-12):
    """torch's own hook on `device` in float32 on the same inputs: dict of u, v, sigma, w_sn, grad_w"""
    conv, hook = hooked_transpose(W, u, v, iters, eps, device)
    w_sn = hook.compute_weight(conv, do_power_iteration=iters > 0)
    grad_w, = torch.autograd.grad(w_sn, conv.weight_orig, G.to(device))
    with torch.no_grad():
        sigma = torch.dot(conv.weight_u, torch.mv(to_matrix(conv.weight_orig), conv.weight_v)).reshape(1)
    return {"u": conv.weight_u.detach(), "v": conv.weight_v.detach(), "sigma": sigma, "w_sn": w_sn.detach(), "grad_w": grad_w}


# ---- a generator-shaped network under spectral norm ------------------------------------------------------------------------
def _act():
    return nn.LeakyReLU(0.1)


class EncoderBlock(nn.Module):
    """norm -> act -> sn(conv4x4/2) -> norm -> act -> sn(conv3x3)"""

    def __init__(self, cin, cout):
        super(EncoderBlock, self).__init__()
        self.model = nn.Sequential(nn.InstanceNorm2d(cin), _act(), sn(nn.Conv2d(cin, cout, 4, 2, 1)),
                                   nn.InstanceNorm2d(cout), _act(), sn(nn.Conv2d(cout, cout, 3, 1, 1)))

    def forward(self, x):
        return self.model(x)


class ResBlock(nn.Module):
    """(act -> sn(conv3x3) -> act -> sn(conv3x3))(x) + sn(conv1x1)(x): a learnable shortcut"""

    def __init__(self, c):
        super(ResBlock, self).__init__()
        self.learnable_shortcut = True
        self.model = nn.Sequential(_act(), sn(nn.Conv2d(c, c, 3, 1, 1)), _act(), sn(nn.Conv2d(c, c, 3, 1, 1)))
        self.shortcut = nn.Sequential(sn(nn.Conv2d(c, c, 1, 1, 0)))

    def forward(self, x):
        return self.model(x) + self.shortcut(x)


class ResBlockDecoder(nn.Module):
    """(act -> sn(conv3x3) -> act -> sn(transposed conv)) + sn(transposed conv) shortcut"""

    def __init__(self, cin, cout):
        super(ResBlockDecoder, self).__init__()
        self.model = nn.Sequential(_act(), sn(nn.Conv2d(cin, cin, 3, 1, 1)), _act(),
                                   sn(nn.ConvTranspose2d(cin, cout, 3, 2, 1, output_padding=1)))
        self.shortcut = nn.Sequential(sn(nn.ConvTranspose2d(cin, cout, 3, 2, 1, output_padding=1)))

    def forward(self, x):
        return self.model(x) + self.shortcut(x)


class Jump(nn.Module):
    """act -> reflect pad -> sn(conv3x3, p 0), the convolution registered twice: `conv1` and `model.2`"""

    def __init__(self, c):
        super(Jump, self).__init__()
        self.conv1 = sn(nn.Conv2d(c, c, 3, 1, 0))
        self.model = nn.Sequential(_act(), nn.ReflectionPad2d(1), self.conv1)

    def forward(self, x):
        return self.model(x)


class Output(nn.Module):
    """act -> reflect pad -> sn(conv3x3 to 3 channels) -> tanh, the convolution registered twice"""

    def __init__(self, c):
        super(Output, self).__init__()
        self.conv1 = sn(nn.Conv2d(c, 3, 3))
        self.model = nn.Sequential(_act(), nn.ReflectionPad2d(1), self.conv1, nn.Tanh())

    def forward(self, x):
        return self.model(x)


class Generator(nn.Module):
    """two encoder blocks, a residual block with a learnable shortcut and a jump around it, `decoders` decoder blocks (two:
    back to the image's size), an image head"""

    def __init__(self, widths=WIDTHS, decoders=2):
        super(Generator, self).__init__()
        w0, w1 = widths
        self.enc0, self.enc1 = EncoderBlock(3, w0), EncoderBlock(w0, w1)
        self.res = ResBlock(w1)
        self.jump = Jump(w1)
        self.decs = nn.ModuleList(ResBlockDecoder(w1 if i == 0 else w0, w0) for i in range(decoders))
        self.out = Output(w0)

    def forward(self, image):
        e = self.enc1(self.enc0(image))
        t = self.res(e) + self.jump(e)
        for dec in self.decs:
            t = dec(t)
        return self.out(t)


def hooked(net):
    """every module of `net` that still carries torch's spectral-norm hook"""
    return [m for m in net.modules() if "weight_orig" in m._parameters and m._forward_pre_hooks]


def hooked_count(decoders=2):
    return 4 + 3 + 1 + 3 * decoders + 1


def generators(device, copies=2, decoders=2, seed=41):
    """(`copies` float32 networks on `device` with equal parameters and buffers, float64 host network, two images), all
    in train() mode"""
    torch.manual_seed(seed)
    host = Generator(decoders=decoders)
    state = host.state_dict()
    nets = []
    for _ in range(copies):
        net = Generator(decoders=decoders)
        net.load_state_dict(state)
        nets.append(net.to(device).train())
    g = torch.Generator().manual_seed(seed + 1)
    images = [torch.rand(IMAGE, generator=g) * 2 - 1 for _ in range(2)]
    return nets, host.double().train(), images
