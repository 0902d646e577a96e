#!/usr/bin/env python3
"""Golden vectors for VGG19Features, produced by the REFERENCE's own `VGG19` class
(model/networks/external_function.py:323-444): its __init__ (the slicing of `features`, the freeze) and its forward run
unchanged on the host in float64.  `torchvision.models.vgg19` (torchvision + downloaded weights) is replaced, before
construction, by a function that returns a seeded configuration-E `features` stack at widths (4, 4, 8, 8, 8)
(tests/vgg_util.py: torchvision_features).  Stored: two float32-representable images, (2, 3, 32, 24) and (1, 3, 19, 21);
the parameters under the reference's state-dict keys; all sixteen outputs per image; random r_layer per output and
d(sum over layers of sum(out * r_layer)) / d image.  Data only.  Needs a checkout of the reference:
    python tests/golden/make_vgg_golden.py REFERENCE_ROOT
"""
import importlib.util
import os, sys, types
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import global_flow_local_attention_amd as gfla  # noqa: E402

# tests/vgg_util.py by path: tests/ on sys.path would shadow the reference's own `util` package
_spec = importlib.util.spec_from_file_location("vgg_util", os.path.join(ROOT, "tests", "vgg_util.py"))
vgg_util = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(vgg_util)

SEED, GAIN, BIAS = 19, 1.4, 0.2
SHAPES = {"a": (2, 3, 32, 24), "b": (1, 3, 19, 21)}

sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
sys.modules.setdefault("torchvision.models", types.ModuleType("torchvision.models"))
sys.modules["torchvision"].models = sys.modules["torchvision.models"]
if len(sys.argv) != 2:
    sys.exit(__doc__)
gfla.install(sys.argv[1], fuse_extractor_attn=False)
import model.networks.external_function as ef  # noqa: E402


class _StubTorchvisionVGG19(object):
    def __init__(self, features):
        self.features = features


def main():
    ef.models.vgg19 = lambda pretrained=True: _StubTorchvisionVGG19(
        vgg_util.torchvision_features(vgg_util.GOLDEN_WIDTHS, SEED, GAIN, BIAS))
    ref = ef.VGG19().double()                        # the reference's constructor around the stub
    state = ref.state_dict()
    assert tuple(state.keys()) == vgg_util.STATE_KEYS, list(state.keys())
    assert not any(p.requires_grad for p in ref.parameters())
    out = {"param/" + k: v.numpy() for k, v in state.items()}
    gen = torch.Generator().manual_seed(SEED + 1)
    for tag, shape in SHAPES.items():
        image = torch.randn(shape, generator=gen).double().requires_grad_()     # float32-representable
        maps = ref(image)                            # the reference's forward
        assert tuple(maps.keys()) == vgg_util.LAYERS and maps["relu3_3"] is maps["relu3_2"]
        total = 0
        for layer in vgg_util.LAYERS:
            r = torch.randn(maps[layer].shape, generator=gen).double()
            total = total + (maps[layer] * r).sum()
            out["%s/out/%s" % (tag, layer)] = maps[layer].detach().numpy()
            out["%s/r/%s" % (tag, layer)] = r.numpy()
            alive = (maps[layer] > 0).double().mean().item()
            print(tag, layer, tuple(maps[layer].shape), "positive: %.2f" % alive)
            assert alive >= 0.1, "a stage of the narrow network has died: choose another seed / gain"
        total.backward()
        out[tag + "/image"] = image.detach().numpy()
        out[tag + "/grad_image"] = image.grad.numpy()
    path = os.path.join(ROOT, "tests", "golden", "vgg_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
