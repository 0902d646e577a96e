#!/usr/bin/env python3
"""Time the generator inference convolutions (gen_conv.py impl = "auto", csrc/gen_conv.hip) next to the torch composition
(impl = "torch": F.leaky_relu + F.conv2d / F.conv_transpose2d, MIOpen) in the same process, under torch.no_grad(), for
float32 / float16 / bfloat16 at the generator's own shapes (B = 8, ngf = 64, 256 x 176 input):

    S1K3  conv3x3              64 -> 64 at 128 x 88, 128 -> 128 at 64 x 44, 256 -> 256 at 32 x 22
    S2K4  conv4x4_down         21 -> 64 from 256 x 176, 64 -> 128 from 128 x 88, 128 -> 256 from 64 x 44
    T2K3  conv_transpose3x3_up 256 -> 128 from 32 x 22, 128 -> 64 from 64 x 44, 64 -> 64 from 128 x 88

each with the LeakyReLU(0.1) in front of it folded in, as the rewritten blocks call them.  The S1K3 rows also time
conv3x3_relu (csrc/conv3x3.hip, the same launch geometry) and conv3x3 without the pre-activation on the same tensors.
Then a generator-shaped stand-in (three encoder blocks, two residual blocks, three decoder blocks, an image head) in
eval() / no_grad(): rewritten by fuse_instance_norm_act + fuse_output_heads + fuse_inference_convs next to the
unrewritten copy with the same parameters.

usage: python tools/bench_gen_conv.py [--iters N] [--out profiles/gen_conv_bench.jsonl]
The parent process does not touch the GPU: every dtype is measured by a child of its own under `timeout -k 10`, and the
first child that fails ends the run.  Every shape is warmed up on all routes; the routes alternate inside each round; one
HIP event pair per call; medians and quartiles (us).  TF/s = 2 * taps * Cin * Cout * B * (pixels the taps are applied at)
over the median time of the call: a rate of the whole call, not a kernel's share of peak."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# geometry, (B, Cin, H, W) of the input, Cout
CASES = [("S1K3", (8, 64, 128, 88), 64), ("S1K3", (8, 128, 64, 44), 128), ("S1K3", (8, 256, 32, 22), 256),
         ("S2K4", (8, 21, 256, 176), 64), ("S2K4", (8, 64, 128, 88), 128), ("S2K4", (8, 128, 64, 44), 256),
         ("T2K3", (8, 256, 32, 22), 128), ("T2K3", (8, 128, 64, 44), 64), ("T2K3", (8, 64, 128, 88), 64)]
DTYPES = ("f32", "f16", "bf16")
SLOPE = 0.1


def timed(fns, iters, warmup=5):
    """(median, first quartile, third quartile) in us of each of `fns`, measured alternately"""
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(iters):
        for t, fn in zip(times, fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) * 1e3)
    out = []
    for t in times:
        q = statistics.quantiles(t, n=4)
        out.append((round(statistics.median(t), 1), round(q[0], 1), round(q[2], 1)))
    return out


def standin(ngf, structure_nc):
    """a generator-shaped body: the block structures of the reference at its widths, without the attention layers"""
    from torch import nn
    act = nn.LeakyReLU(SLOPE)

    def enc(cin, cout):
        return nn.Sequential(nn.InstanceNorm2d(cin), act, nn.Conv2d(cin, cout, 4, 2, 1), nn.InstanceNorm2d(cout), act,
                             nn.Conv2d(cout, cout, 3, 1, 1))

    class Res(nn.Module):
        def __init__(self, c):
            super(Res, self).__init__()
            self.model = nn.Sequential(nn.InstanceNorm2d(c), act, nn.Conv2d(c, c, 3, 1, 1), nn.InstanceNorm2d(c), act,
                                       nn.Conv2d(c, c, 3, 1, 1))

        def forward(self, x):
            last = self.model[5]
            return last(self.model[:5](x), x) if hasattr(last, "geometry") else self.model(x) + x

    class Dec(nn.Module):
        def __init__(self, cin, cout):
            super(Dec, self).__init__()
            self.model = nn.Sequential(nn.InstanceNorm2d(cin), act, nn.Conv2d(cin, cin, 3, 1, 1), nn.InstanceNorm2d(cin), act,
                                       nn.ConvTranspose2d(cin, cout, 3, 2, 1, output_padding=1))
            self.shortcut = nn.Sequential(nn.ConvTranspose2d(cin, cout, 3, 2, 1, output_padding=1))

        def forward(self, x):
            last = self.model[5]
            if hasattr(last, "geometry"):
                return last(self.model[:5](x), self.shortcut(x))
            return self.model(x) + self.shortcut(x)

    c1, c2, c3 = ngf, 2 * ngf, 4 * ngf
    return nn.Sequential(enc(structure_nc, c1), enc(c1, c2), enc(c2, c3), Res(c3), Res(c3), Dec(c3, c2), Dec(c2, c1), Dec(c1, c1),
                         nn.Sequential(act, nn.ReflectionPad2d(1), nn.Conv2d(c1, 3, 3), nn.Tanh()))


def worker(a):
    import copy
    import torch
    import global_flow_local_attention_amd as gfla
    dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[a.worker]
    calls = {"S1K3": lambda x, w, b, impl: gfla.conv3x3(x, w, b, pre_slope=SLOPE, impl=impl),
             "S2K4": lambda x, w, b, impl: gfla.conv4x4_down(x, w, b, pre_slope=SLOPE, impl=impl),
             "T2K3": lambda x, w, b, impl: gfla.conv_transpose3x3_up(x, w, b, pre_slope=SLOPE, impl=impl)}
    with torch.no_grad():
        for geometry, shape, cout in CASES:
            B, Cin, H, W = shape
            k = 4 if geometry == "S2K4" else 3
            g = torch.Generator().manual_seed(Cin + H + cout)
            x = torch.randn(shape, generator=g).to(dt).cuda()
            wshape = (Cin, cout, k, k) if geometry == "T2K3" else (cout, Cin, k, k)
            w = (torch.randn(wshape, generator=g) * (2.0 / (k * k * Cin)) ** 0.5).to(dt).cuda()
            b = (0.1 * torch.randn(cout, generator=g)).to(dt).cuda()
            call = calls[geometry]
            fns = [lambda: call(x, w, b, "auto"), lambda: call(x, w, b, "torch")]
            if geometry == "S1K3":
                fns.append(lambda: gfla.conv3x3_relu(x, w, b))
                fns.append(lambda: gfla.conv3x3(x, w, b))
            res = timed(fns, a.iters)
            ya, yt = call(x, w, b, "auto").float(), call(x, w, b, "torch").float()
            # multiply-adds actually needed: S2K4 16 taps per output pixel, T2K3 9 taps per input pixel
            px = {"S1K3": H * W, "S2K4": ((H - 2) // 2 + 1) * ((W - 2) // 2 + 1), "T2K3": H * W}[geometry]
            flop = 2.0 * (16 if geometry == "S2K4" else 9) * Cin * cout * B * px
            row = {"what": "conv", "geometry": geometry, "dtype": a.worker, "B": B, "Cin": Cin, "Cout": cout, "H": H, "W": W,
                   "kernels_us": res[0][0], "kernels_q1_q3_us": res[0][1:], "torch_us": res[1][0], "torch_q1_q3_us": res[1][1:],
                   "speedup": round(res[1][0] / res[0][0], 2), "kernels_tflops": round(flop / res[0][0] * 1e-6, 1),
                   "torch_tflops": round(flop / res[1][0] * 1e-6, 1),
                   "routes_rel_diff": ((ya - yt).abs().max() / yt.abs().max()).item()}
            if geometry == "S1K3":
                row["conv3x3_relu_us"], row["conv3x3_relu_q1_q3_us"] = res[2][0], res[2][1:]
                row["kernels_no_act_us"], row["kernels_no_act_q1_q3_us"] = res[3][0], res[3][1:]
            print(json.dumps(row), flush=True)
            del x, w, b, ya, yt
        torch.manual_seed(3)
        plain = standin(64, 18).cuda().to(dt).eval()
        fused = copy.deepcopy(plain)
        counts = (gfla.fuse_instance_norm_act(fused), gfla.fuse_output_heads(fused), gfla.fuse_inference_convs(fused))
        # the torch route of the same rewritten modules: what the rewrite costs or saves outside the convolutions
        pose = torch.rand(8, 18, 256, 176, generator=torch.Generator().manual_seed(4)).to(dt).cuda()
        res = timed([lambda: fused(pose), lambda: plain(pose)], a.iters)
        ya, yt = fused(pose).float(), plain(pose).float()
        row = {"what": "network", "dtype": a.worker, "B": 8, "H": 256, "W": 176, "ngf": 64, "rewritten": list(counts),
               "rewritten_us": res[0][0], "rewritten_q1_q3_us": res[0][1:], "plain_us": res[1][0], "plain_q1_q3_us": res[1][1:],
               "speedup": round(res[1][0] / res[0][0], 2), "routes_rel_diff": ((ya - yt).abs().max() / yt.abs().max()).item()}
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=int, default=150, help="seconds a dtype's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_conv_bench.jsonl"))
    ap.add_argument("--worker", choices=DTYPES, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    rows = []
    for name in DTYPES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", name,
               "--iters", str(a.iters)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(done.stdout)
        sys.stdout.flush()
        if done.returncode != 0:
            sys.exit("the %s child ended with status %d: nothing more is started" % (name, done.returncode))
        rows += [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(json.dumps(r) for r in rows) + "\n")
    convs = [r for r in rows if r["what"] == "conv"]
    summary = {"tool": "bench_gen_conv", "rows": len(rows), "detail": os.path.relpath(a.out, ROOT),
               "conv_speedup_min_max": [min(r["speedup"] for r in convs), max(r["speedup"] for r in convs)],
               "network_speedup": {r["dtype"]: r["speedup"] for r in rows if r["what"] == "network"}}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
