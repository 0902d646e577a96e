#!/usr/bin/env python3
"""Time VGG19Features on the library's kernels (impl = "auto": csrc/conv3x3.hip, csrc/maxpool2x2.hip) next to the torch
composition (impl = "torch": F.conv2d / F.max_pool2d, MIOpen) in the same process, with the same random He-scaled weights:
the whole network forward and forward + backward with respect to the image, and every convolution on its own (forward,
fed with the map the network produces there), for an (8, 3, 256, 176) image in float32 / float16 / bfloat16.

usage: python tools/bench_vgg19.py [--iters N] [--batch B] [--out profiles/vgg19_bench.jsonl]
Every shape is warmed up on both routes first; the two routes alternate inside each round; one HIP event pair around
each call; medians and quartiles are reported (us).  TF/s = 2 * 9 * Cin * Cout * B * H * W (the convolution's own
operations) over the median time of the call: a rate of the whole call, not a kernel's share of peak."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import global_flow_local_attention_amd as gfla  # noqa: E402

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
IMPLS = (("kernels", "auto"), ("torch", "torch"))


def timed_pair(fns, iters, warmup=3):
    """(median, first quartile, third quartile) in us of each callable; the callables alternate inside every round"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3)
    out = []
    for t in times:
        q = statistics.quantiles(t, n=4)
        out.append((statistics.median(t), round(q[0], 1), round(q[2], 1)))
    return out


def he_init(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / (9 * m.in_channels)) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=176)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgg19_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_vgg19: no GPU visible")
    rows = []
    image32 = torch.randn(a.batch, 3, a.height, a.width, generator=torch.Generator().manual_seed(0))
    for name, dt in DTYPES.items():
        nets = {}
        for key, impl in IMPLS:
            net = gfla.VGG19Features(impl=impl)
            he_init(net, seed=1)
            nets[key] = net.cuda().to(dt)
        image = image32.to(dt).cuda()

        def forward(net):
            def run():
                with torch.no_grad():
                    return net(image)
            return run

        def forward_backward(net):
            leaf = image.clone().requires_grad_()

            def run():
                leaf.grad = None
                out = net(leaf)
                total = 0
                for layer in ("relu1_1", "relu2_1", "relu3_1", "relu4_1", "relu5_1", "relu2_2", "relu3_4", "relu4_4", "relu5_2"):
                    total = total + out[layer].float().mean()
                total.backward()
            return run

        # the two routes must compute the same thing before their times are compared
        with torch.no_grad():
            ya, yb = nets["kernels"](image)["relu5_4"].float(), nets["torch"](image)["relu5_4"].float()
        row = {"what": "network", "dtype": name, "B": a.batch, "H": a.height, "W": a.width,
               "relu5_4_rel_diff": ((ya - yb).abs().max() / yb.abs().max()).item()}
        for what, make in (("fwd", forward), ("fwd_bwd", forward_backward)):
            res = timed_pair([make(nets["kernels"]), make(nets["torch"])], a.iters)
            for (key, _), (med, q1, q3) in zip(IMPLS, res):
                row["%s_%s_us" % (key, what)], row["%s_%s_q1_q3_us" % (key, what)] = med, [q1, q3]
        row["fwd_speedup"] = round(row["torch_fwd_us"] / row["kernels_fwd_us"], 3)
        row["fwd_bwd_speedup"] = round(row["torch_fwd_bwd_us"] / row["kernels_fwd_bwd_us"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)

        # every convolution on its own, on the map the network feeds it
        inputs = {}
        hooks = [m.register_forward_hook(lambda mod, inp, out, n=n: inputs.__setitem__(n, inp[0].detach()))
                 for n, m in nets["kernels"].named_modules() if isinstance(m, torch.nn.Conv2d)]
        with torch.no_grad():
            nets["kernels"](image)
        for h in hooks:
            h.remove()
        convs = {key: dict((n, m) for n, m in nets[key].named_modules() if isinstance(m, torch.nn.Conv2d)) for key in nets}
        for n, x in inputs.items():
            def layer(key):
                conv = convs[key][n]

                def run():
                    with torch.no_grad():
                        return conv(x)
                return run
            (tk, k1, k3), (tt, _, _) = timed_pair([layer("kernels"), layer("torch")], a.iters)
            B, Cin, H, W = x.shape
            flop = 2.0 * 9 * Cin * convs["kernels"][n].out_channels * B * H * W
            row = {"what": "conv", "layer": n, "dtype": name, "Cin": Cin, "Cout": convs["kernels"][n].out_channels, "H": H,
                   "W": W, "kernels_us": round(tk, 1), "kernels_q1_q3_us": [k1, k3], "torch_us": round(tt, 1),
                   "kernels_tflops": round(flop / tk * 1e-6, 1), "torch_tflops": round(flop / tt * 1e-6, 1)}
            print(json.dumps(row), flush=True)
            rows.append(row)
        del nets, convs, inputs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
