#!/usr/bin/env python3
"""Time a forward + backward of the generator convolutions on the library's own kernels (gen_conv.py grad = "kernels":
GenConvFunction, csrc/gen_conv.hip + csrc/gen_conv_bwd.hip + csrc/gen_conv_wgrad.hip) next to the torch composition
(grad = "torch": F.leaky_relu + F.conv2d / F.conv_transpose2d and their MIOpen gradients) in the same process, for float32
/ float16 / bfloat16 at the shapes of tools/bench_gen_conv.py (B = 8, ngf = 64, 256 x 176 input), x, the weight and the
bias all requiring a gradient.  Then that tool's generator-shaped stand-in in train() mode, forward + backward of
net(pose).square().mean(): rewritten by fuse_instance_norm_act + fuse_output_heads + fuse_inference_convs(grad="kernels")
next to the same rewrite with grad="torch" (so the difference is the convolutions alone) and to the unrewritten copy.

usage: python tools/bench_gen_conv_train.py [--iters N] [--out profiles/gen_conv_train_bench.jsonl]
Method as tools/bench_gen_conv.py: the parent process does not touch the GPU, every dtype is measured by a child of its
own under `timeout -k 10`, the first child that fails ends the run; every shape is warmed up on all routes; the routes
alternate inside each round; one HIP event pair per call; medians and quartiles (us).  No pass bar."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_gen_conv import CASES, DTYPES, SLOPE, standin, timed  # noqa: E402


def worker(a):
    import copy
    import torch
    import global_flow_local_attention_amd as gfla
    dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[a.worker]
    calls = {"S1K3": lambda x, w, b, grad: gfla.conv3x3(x, w, b, pre_slope=SLOPE, grad=grad),
             "S2K4": lambda x, w, b, grad: gfla.conv4x4_down(x, w, b, pre_slope=SLOPE, grad=grad),
             "T2K3": lambda x, w, b, grad: gfla.conv_transpose3x3_up(x, w, b, pre_slope=SLOPE, grad=grad)}
    for geometry, shape, cout in CASES:
        B, Cin, H, W = shape
        k = 4 if geometry == "S2K4" else 3
        g = torch.Generator().manual_seed(Cin + H + cout)
        x = torch.randn(shape, generator=g).to(dt).cuda().requires_grad_()
        wshape = (Cin, cout, k, k) if geometry == "T2K3" else (cout, Cin, k, k)
        w = (torch.randn(wshape, generator=g) * (2.0 / (k * k * Cin)) ** 0.5).to(dt).cuda().requires_grad_()
        b = (0.1 * torch.randn(cout, generator=g)).to(dt).cuda().requires_grad_()
        call = calls[geometry]
        gy = torch.randn_like(call(x, w, b, "torch").detach())

        def step(grad):
            x.grad = w.grad = b.grad = None
            call(x, w, b, grad).backward(gy)

        def forward(grad):
            with torch.no_grad():
                call(x, w, b, grad)

        res = timed([lambda: step("kernels"), lambda: step("torch"), lambda: forward("kernels")], a.iters)
        step("kernels")
        ours = [t.grad.float().clone() for t in (x, w, b)]
        step("torch")
        diff = max(((o - t.grad.float()).abs().max() / t.grad.float().abs().max()).item() for o, t in zip(ours, (x, w, b)))
        row = {"what": "conv", "geometry": geometry, "dtype": a.worker, "B": B, "Cin": Cin, "Cout": cout, "H": H, "W": W,
               "kernels_us": res[0][0], "kernels_q1_q3_us": res[0][1:], "torch_us": res[1][0], "torch_q1_q3_us": res[1][1:],
               "kernels_forward_us": res[2][0], "speedup": round(res[1][0] / res[0][0], 2), "routes_rel_diff": diff}
        print(json.dumps(row), flush=True)
        del x, w, b, gy, ours
    torch.manual_seed(3)
    plain = standin(64, 18).cuda().to(dt).train()
    nets, counts = [], None
    for grad in ("kernels", "torch"):
        net = copy.deepcopy(plain)
        counts = (gfla.fuse_instance_norm_act(net), gfla.fuse_output_heads(net), gfla.fuse_inference_convs(net, grad=grad))
        nets.append(net)
    pose = torch.rand(8, 18, 256, 176, generator=torch.Generator().manual_seed(4)).to(dt).cuda()

    def train_step(net):
        net.zero_grad(set_to_none=True)
        net(pose).float().square().mean().backward()

    res = timed([lambda: train_step(nets[0]), lambda: train_step(nets[1]), lambda: train_step(plain)], a.iters)
    row = {"what": "network", "dtype": a.worker, "B": 8, "H": 256, "W": 176, "ngf": 64, "rewritten": list(counts),
           "kernels_us": res[0][0], "kernels_q1_q3_us": res[0][1:], "torch_us": res[1][0], "torch_q1_q3_us": res[1][1:],
           "plain_us": res[2][0], "plain_q1_q3_us": res[2][1:], "speedup": round(res[1][0] / res[0][0], 2)}
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=int, default=150, help="seconds a dtype's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_conv_train_bench.jsonl"))
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
    summary = {"tool": "bench_gen_conv_train", "rows": len(rows), "detail": os.path.relpath(a.out, ROOT),
               "conv_speedup_min_max": [min(r["speedup"] for r in convs), max(r["speedup"] for r in convs)],
               "network_speedup": {r["dtype"]: r["speedup"] for r in rows if r["what"] == "network"}}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
