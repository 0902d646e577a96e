#!/usr/bin/env python3
"""Write tests/golden/head_conv_golden.npz: float64 inputs, parameters, upstream gradients, outputs and all gradients of
the reference's OWN classes on the host -- base_function.Output (norm_layer=None, LeakyReLU(0.1)) and the attn_output
methods of generator.PoseFlowNet / generator.FaceFlowNet -- at the shapes tests/head_conv_util.GOLDENS lists.  Data only.

usage: python tests/golden/make_head_conv_golden.py /path/to/reference/checkout"""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import head_conv_util as hu  # noqa: E402


def flow_net(cls, cin, nflow, nmask):
    """an instance of the reference's flow network class with nothing but the two heads of layer 0: attn_output reads
    `output0` and `mask0` only"""
    net = cls.__new__(cls)
    nn.Module.__init__(net)
    net.output0 = nn.Conv2d(cin, nflow, kernel_size=3, stride=1, padding=1, bias=True)
    net.mask0 = nn.Sequential(nn.Conv2d(cin, nmask, kernel_size=3, stride=1, padding=1, bias=True), nn.Sigmoid())
    return net.double()


def main():
    import global_flow_local_attention_amd as gfla
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
    base_function = gfla.install(sys.argv[1])
    import model.networks.generator as generator
    out = {}
    for i, (name, (shape, cout, post, split, padding, slope)) in enumerate(sorted(hu.GOLDENS.items())):
        torch.manual_seed(100 + i)
        B, Cin, H, W = shape
        x = torch.randn(shape, dtype=torch.float64, requires_grad=True)
        up = torch.randn(B, cout, H, W, dtype=torch.float64)
        if name == "output":
            net = base_function.Output(Cin, cout, 3, None, nn.LeakyReLU(slope), False, False).double()
            ys = (net(x),)
            weight, bias = net.conv1.weight, net.conv1.bias
            (ys[0] * up).sum().backward()
            gw, gb = weight.grad, bias.grad
        else:
            cls = generator.PoseFlowNet if name == "pose_heads" else generator.FaceFlowNet
            net = flow_net(cls, Cin, split, cout - split)
            ys = net.attn_output(x, 0)
            ((ys[0] * up[:, :split]).sum() + (ys[1] * up[:, split:]).sum()).backward()
            weight = torch.cat((net.output0.weight, net.mask0[0].weight), 0)
            bias = torch.cat((net.output0.bias, net.mask0[0].bias), 0)
            gw = torch.cat((net.output0.weight.grad, net.mask0[0].weight.grad), 0)
            gb = torch.cat((net.output0.bias.grad, net.mask0[0].bias.grad), 0)
        rec = {"x": x, "weight": weight, "bias": bias, "up": up, "g_x": x.grad, "g_weight": gw, "g_bias": gb}
        for j, y in enumerate(ys):
            rec["y%d" % j] = y
        for k, v in rec.items():
            out["%s/%s" % (name, k)] = v.detach().numpy().copy()
    np.savez_compressed(hu.GOLDEN_PATH, **out)
    print("wrote %s: %d arrays, %d bytes" % (hu.GOLDEN_PATH, len(out), os.path.getsize(hu.GOLDEN_PATH)))


if __name__ == "__main__":
    main()
