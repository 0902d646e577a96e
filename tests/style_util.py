"""Shared by the style-loss tests: the stub feature extractor, the feature generators of the issue's cases and the
float64 host reference (the reference's compute_gram + L1Loss on the stored values)."""
import torch

STYLE_LAYERS = ("relu2_2", "relu3_4", "relu4_4", "relu5_2")
CONTENT_LAYERS = ("relu1_1", "relu2_1", "relu3_1", "relu4_1", "relu5_1")


class TableVGG(torch.nn.Module):
    """image = a 0-dim tag -> the feature maps stored under it (the losses are functions of the features alone)"""

    def __init__(self, table):
        super().__init__()
        self.table = table

    def forward(self, tag):
        return self.table[int(tag)]


def make_features(B, C, H, W, dtype, seed, near):
    """x = relu(1.5 randn + 0.2); y drawn separately ("independent") or relu(x + 0.01 noise - 0.01) ("near"), both
    rounded to `dtype`."""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(1.5 * torch.randn(B, C, H, W, generator=g) + 0.2)
    if near:
        y = torch.relu(x + 0.01 * torch.randn(B, C, H, W, generator=g) - 0.01)
    else:
        y = torch.relu(1.5 * torch.randn(B, C, H, W, generator=g) + 0.2)
    return x.to(dtype), y.to(dtype)


def gram64(x):
    """compute_gram (external_function.py:134-139) in float64 on the host, on x's stored values"""
    b, ch, h, w = x.shape
    f = x.detach().cpu().double().reshape(b, ch, h * w)
    return f.bmm(f.transpose(1, 2)) / (h * w * ch)


def reference(x, y):
    """(loss, D, G(x)) in float64 on the host"""
    gx, gy = gram64(x), gram64(y)
    d = gx - gy
    return d.abs().mean().item(), d, gx


def reference_grad(x, sign, negate=False):
    """(+-) 2 / (B C^3 N) S F in float64 for a given sign matrix S (B,C,C)"""
    b, ch, h, w = x.shape
    f = x.detach().cpu().double().reshape(b, ch, h * w)
    g = 2.0 / (b * ch ** 3 * h * w) * sign.double().bmm(f)
    return (-g if negate else g).reshape(x.shape)


class ConvStubVGG(torch.nn.Module):
    """Frozen random stand-in for VGG19 that yields all nine layers VGGLoss reads: five strided stages, each giving its
    relu*_1 map and (stages 2-5) the style map from one more convolution."""

    def __init__(self, widths=(8, 24, 40, 64, 64), seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.stages, self.heads = torch.nn.ModuleList(), torch.nn.ModuleList()
        cin = 3
        for i, c in enumerate(widths):
            self.stages.append(torch.nn.Conv2d(cin, c, 3, 1 if i == 0 else 2, 1))
            self.heads.append(torch.nn.Conv2d(c, c, 3, 1, 1))
            cin = c
        with torch.no_grad():
            for conv in list(self.stages) + list(self.heads):
                fan = 9 * conv.in_channels
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (2.0 / fan) ** 0.5)
                conv.bias.copy_(torch.randn(conv.bias.shape, generator=gen) * 0.1)
        for p in self.parameters():
            p.requires_grad_(False)

    def forward(self, x):
        out = {}
        for i, (stage, head) in enumerate(zip(self.stages, self.heads)):
            x = torch.relu(stage(x))
            out[CONTENT_LAYERS[i]] = x
            if i >= 1:
                out[STYLE_LAYERS[i - 1]] = torch.relu(head(x))
        return out
