#!/usr/bin/env python3
"""Golden vectors for VGGLoss / StyleLoss / PerceptualLoss, produced by the REFERENCE's own classes
(model/networks/external_function.py:121-220): their __init__ / compute_gram / __call__ run unchanged on the host in
float64.  `external_function.VGG19` (torchvision + downloaded weights) is replaced, before construction, by a stub
extractor that hands out stored feature maps: the losses are functions of the features alone.  Stored per case: the
feature maps of both images, (content, style) as VGGLoss returns them, and d(content + style)/d features of both images;
the features are float32-representable so that the float32 tests read the very same numbers.  Includes channel counts
and map sizes that are no multiple of anything.  Needs a checkout of the reference:
    python tests/golden/make_style_golden.py REFERENCE_ROOT
"""
import os, sys, types
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import global_flow_local_attention_amd as gfla  # noqa: E402

sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
sys.modules.setdefault("torchvision.models", types.ModuleType("torchvision.models"))
sys.modules["torchvision"].models = sys.modules["torchvision.models"]
if len(sys.argv) != 2:
    sys.exit(__doc__)
gfla.install(sys.argv[1], fuse_extractor_attn=False)
import model.networks.external_function as ef  # noqa: E402

LAYERS = ("relu1_1", "relu2_1", "relu3_1", "relu4_1", "relu5_1", "relu2_2", "relu3_4", "relu4_4", "relu5_2")
# name, B, {layer: (C, H, W)}, content weights
CASES = [
    ("small", 2, dict(relu1_1=(4, 8, 6), relu2_1=(6, 4, 3), relu3_1=(8, 2, 2), relu4_1=(8, 1, 1), relu5_1=(8, 1, 1),
                      relu2_2=(8, 6, 5), relu3_4=(12, 4, 3), relu4_4=(16, 2, 2), relu5_2=(6, 1, 1)), [1.0] * 5),
    ("ragged", 1, dict(relu1_1=(3, 5, 7), relu2_1=(5, 3, 4), relu3_1=(7, 2, 3), relu4_1=(9, 1, 2), relu5_1=(9, 1, 1),
                       relu2_2=(24, 7, 5), relu3_4=(10, 5, 3), relu4_4=(7, 3, 3), relu5_2=(5, 2, 1)),
     [1.0, 0.5, 0.25, 2.0, 1.5]),
    ("near", 3, dict(relu1_1=(2, 4, 4), relu2_1=(2, 2, 2), relu3_1=(2, 2, 2), relu4_1=(2, 1, 1), relu5_1=(2, 1, 1),
                     relu2_2=(9, 4, 5), relu3_4=(6, 3, 3), relu4_4=(5, 2, 2), relu5_2=(4, 1, 2)), [1.0] * 5),
]


class StubVGG(torch.nn.Module):
    """image = a 0-dim tag (0: generated, 1: target) -> the stored feature maps of that image"""

    def __init__(self):
        super().__init__()
        self.table = {}

    def forward(self, tag):
        return self.table[int(tag)]


def features(gen, B, shapes, near_of=None):
    out = {}
    for layer in LAYERS:
        C, H, W = shapes[layer]
        if near_of is None:
            f = torch.relu(1.5 * torch.randn(B, C, H, W, generator=gen) + 0.2)
        else:
            f = torch.relu(near_of[layer].float() + 0.01 * torch.randn(B, C, H, W, generator=gen) - 0.01)
        out[layer] = f.double().requires_grad_()
    return out


def main():
    ef.VGG19 = StubVGG
    out = {}
    for i, (name, B, shapes, weights) in enumerate(CASES):
        gen = torch.Generator().manual_seed(500 + i)
        x = features(gen, B, shapes)
        y = features(gen, B, shapes, near_of={k: v.detach() for k, v in x.items()} if name == "near" else None)
        ref = ef.VGGLoss(weights)                     # the reference's constructor, around the stub
        ref.vgg.table = {0: x, 1: y}
        content, style = ref(torch.tensor(0), torch.tensor(1))     # the reference's __call__ / compute_gram
        assert ef.StyleLoss.__call__(ref, torch.tensor(0), torch.tensor(1)).item() == style.item()
        assert ef.PerceptualLoss.__call__(ref, torch.tensor(0), torch.tensor(1)).item() == content.item()
        (content + style).backward()
        out[name + "/weights"] = np.asarray(weights)
        out[name + "/content"] = content.detach().numpy()
        out[name + "/style"] = style.detach().numpy()
        for layer in LAYERS:
            out["%s/x/%s" % (name, layer)] = x[layer].detach().numpy()
            out["%s/y/%s" % (name, layer)] = y[layer].detach().numpy()
            out["%s/gx/%s" % (name, layer)] = x[layer].grad.numpy()
            out["%s/gy/%s" % (name, layer)] = y[layer].grad.numpy()
        print(name, content.item(), style.item())
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "style_golden.npz"), **out)


if __name__ == "__main__":
    main()
