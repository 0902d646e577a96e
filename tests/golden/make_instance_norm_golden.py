#!/usr/bin/env python3
"""Record tests/golden/instance_norm_golden.npz: float64 input, parameters, upstream gradient, output and the three
gradients of nn.InstanceNorm2d -> LeakyReLU / ReLU / nothing, from torch on the CPU, for three small cases (affine +
LeakyReLU 0.1, non-affine + ReLU, affine without activation).  Inputs are kept clear of the activation's kink
(tests/instance_norm_util.clear_of_kinks), so that lower-precision evaluations of the same inputs pick the same slopes.

usage: python tests/golden/make_instance_norm_golden.py"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import instance_norm_util as iu  # noqa: E402


def main():
    out = {}
    for seed, (config, shape) in enumerate(sorted(iu.GOLDEN_SHAPES.items())):
        x, weight, bias, up, slope = iu.make_case(shape, torch.float64, config, seed=100 + seed)
        affine = weight is not None
        norm = nn.InstanceNorm2d(shape[1], eps=iu.EPS, affine=affine).double()
        if affine:
            with torch.no_grad():
                norm.weight.copy_(weight)
                norm.bias.copy_(bias)
        act = nn.Identity() if slope is None else (nn.ReLU() if slope == 0 else nn.LeakyReLU(slope))
        xs = x.clone().requires_grad_()
        y = act(norm(xs))
        (y * up).sum().backward()
        rec = {"x": x, "up": up, "y": y.detach(), "g_x": xs.grad}
        if affine:
            rec.update({"weight": weight, "bias": bias, "g_weight": norm.weight.grad, "g_bias": norm.bias.grad})
        for k, v in rec.items():
            out["%s/%s" % (config, k)] = v.numpy()
    path = os.path.join(HERE, "instance_norm_golden.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
