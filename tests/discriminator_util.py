"""Shared by the tests of the batched spectral norm (spectral_norm.py; csrc/spectral_norm.hip): a discriminator-shaped
network under torch's spectral_norm hooks, the float64 host evaluation of the op's formulas, and the torch hook itself as
the float32 baseline of a single matrix."""
import torch
from torch import nn
from torch.nn.utils import spectral_norm as sn

# (R, K): the final convolution (R = 1); K no multiple of 4; small and odd; a middle layer; the largest matrix of the
# reference's discriminator; tails in both directions
MATRICES = ((1, 128), (32, 27), (7, 80), (64, 512), (128, 2048), (130, 2051))
IMAGE = (2, 3, 21, 19)      # odd both ways: the 4x4 stride-2 output and the pooled shortcut must agree at 10 x 9 and below


class Block(nn.Module):
    """act -> sn(conv3x3) -> act -> sn(conv4x4/2), plus the pooled 1x1 shortcut"""

    def __init__(self, cin, cout, iters=1):
        super(Block, self).__init__()
        self.model = nn.Sequential(nn.LeakyReLU(0.1), sn(nn.Conv2d(cin, cin, 3, 1, 1), n_power_iterations=iters),
                                   nn.LeakyReLU(0.1), sn(nn.Conv2d(cin, cout, 4, 2, 1), n_power_iterations=iters))
        self.shortcut = nn.Sequential(nn.AvgPool2d(2, 2), sn(nn.Conv2d(cin, cout, 1), n_power_iterations=iters))

    def forward(self, x):
        return self.model(x) + self.shortcut(x)


class Discriminator(nn.Module):
    def __init__(self, widths=(8, 16, 32), iters=1):
        super(Discriminator, self).__init__()
        chans = (3,) + tuple(widths)
        self.blocks = nn.ModuleList(Block(a, b, iters) for a, b in zip(chans[:-1], chans[1:]))
        self.act = nn.LeakyReLU(0.1)
        self.conv = sn(nn.Conv2d(chans[-1], 1, 1), n_power_iterations=iters)

    def forward(self, x):
        for block in self.blocks:
            x = block(x)
        return self.conv(self.act(x))


def hooked_convs(net):
    return [m for m in net.modules() if type(m) is nn.Conv2d and "weight_orig" in m._parameters]


def discriminators(device, copies=2, widths=(8, 16, 32), iters=1, seed=21):
    """(`copies` float32 networks on `device` with equal parameters and buffers, float64 host network, two images), all
    in train() mode"""
    torch.manual_seed(seed)
    host = Discriminator(widths, iters)
    state = host.state_dict()
    nets = []
    for _ in range(copies):
        net = Discriminator(widths, iters)
        net.load_state_dict(state)
        nets.append(net.to(device).train())
    g = torch.Generator().manual_seed(seed + 1)
    images = [torch.rand(IMAGE, generator=g) * 2 - 1 for _ in range(2)]
    return nets, host.double().train(), images


def matrix_inputs(R, K, seed, scale=None):
    """(W, u, v, G) float32 on the host: a weight, unit start vectors as torch's hook draws them, an upstream gradient"""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(R, K, generator=g) * (2.0 / K) ** 0.5
    if scale is not None:
        W = W * (scale / W.abs().max())
    u = torch.nn.functional.normalize(torch.randn(R, generator=g), dim=0)
    v = torch.nn.functional.normalize(torch.randn(K, generator=g), dim=0)
    return W, u, v, torch.randn(R, K, generator=g)


def truth64(W, u, v, G, iters, eps=1e-12):
    """The op's formulas in float64 from the float32 inputs: dict of u, v, sigma, w_sn, grad_w"""
    W, u, v, G = W.double(), u.double(), v.double(), G.double()
    for _ in range(iters):
        t = W.t() @ u
        v = t / max(t.norm().item(), eps)
        s = W @ v
        u = s / max(s.norm().item(), eps)
    sigma = u @ (W @ v)
    c = (G * W).sum() / sigma
    return {"u": u, "v": v, "sigma": sigma.reshape(1), "w_sn": W / sigma, "grad_w": (G - c * torch.outer(u, v)) / sigma}


def hook_float32(W, u, v, G, iters, device, eps=1e-12):
    """torch's own hook on `device` in float32 on the same inputs: the same dict.  The hook object of a spectrally
    normalised nn.Linear (weight (R, K), dim 0) computes the weight; autograd gives the gradient."""
    R, K = W.shape
    lin = sn(nn.Linear(K, R, bias=False), n_power_iterations=max(iters, 1), eps=eps).to(device)
    with torch.no_grad():
        lin.weight_orig.copy_(W)
        lin.weight_u.copy_(u)
        lin.weight_v.copy_(v)
    hook = next(iter(lin._forward_pre_hooks.values()))
    w_sn = hook.compute_weight(lin, do_power_iteration=iters > 0)
    grad_w, = torch.autograd.grad(w_sn, lin.weight_orig, G.to(device))
    with torch.no_grad():
        sigma = torch.dot(lin.weight_u, torch.mv(lin.weight_orig, lin.weight_v)).reshape(1)
    return {"u": lin.weight_u.detach(), "v": lin.weight_v.detach(), "sigma": sigma, "w_sn": w_sn.detach(), "grad_w": grad_w}


def distance(got, want64):
    """largest error relative to the quantity's largest float64 entry"""
    return ((got.detach().cpu().double() - want64).abs().max() / want64.abs().max()).item()
