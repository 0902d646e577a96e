#!/usr/bin/env python3
"""Time the fused InstanceNorm2d + LeakyReLU(0.1) (instance_norm_act impl = "auto", csrc/instance_norm.hip) next to the
torch composition (impl = "torch": F.instance_norm + F.leaky_relu) in the same process: forward, and forward + backward
(d x, d weight, d bias), with the affine terms, for float32 / float16 / bfloat16 maps (float32 parameters, as under
autocast) at the generator's plane sizes (C,H,W) = (64,256,176) (64,128,88) (128,64,44) (256,32,22) (512,8,6), each at
B = 1 and B = 32.

Per row: the median time of both routes (us), their ratio, the launch regime, and the kernel's effective GB/s from the
byte model -- forward N B C (elem in + elem out), backward N B C (2 in + 1 out) -- next to the 6.3 TB/s the chip
sustains.  The backward's time is (forward + backward) - forward of the same route.

usage: python tools/bench_instance_norm.py [--iters N] [--out profiles/instance_norm_bench.jsonl]
The parent process does not touch the GPU: every dtype is measured by a child of its own under `timeout -k 10`, and the
first child that fails ends the run.  Warm-up, then one HIP event pair per iteration, the two routes alternating; the
last line printed is one JSON summary, the rows go to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64, 256, 176), (64, 128, 88), (128, 64, 44), (256, 32, 22), (512, 8, 6)]   # C, H, W
BATCHES = (1, 32)
DTYPES = ("f32", "f16", "bf16")
PEAK_GBS = 6300.0
SLOPE = 0.1


def timed_pair(fns, iters, warmup=10):
    """median us of each of `fns`, measured alternately"""
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
    return [statistics.median(t) for t in times]


def worker(a):
    import ctypes
    import torch
    import global_flow_local_attention_amd as gfla
    from global_flow_local_attention_amd import _lib
    dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[a.worker]
    esize = torch.empty((), dtype=dt).element_size()
    geo = (ctypes.c_int64 * 7)()
    for C, H, W in SHAPES:
        for B in BATCHES:
            g = torch.Generator().manual_seed(C + H + B)
            x = torch.randn(B, C, H, W, generator=g).to(dt).cuda().requires_grad_()
            up = torch.randn(B, C, H, W, generator=g).to(dt).cuda()
            w = (1 + 0.5 * torch.randn(C, generator=g)).cuda().requires_grad_()
            b = (0.3 * torch.randn(C, generator=g)).cuda().requires_grad_()
            assert _lib.lib().gfla_instance_norm_geometry(B, C, H, W, esize, 0, ctypes.cast(geo, ctypes.c_void_p)) == 0

            def forward(impl):
                def fn():
                    with torch.no_grad():
                        return gfla.instance_norm_act(x, w, b, 1e-5, SLOPE, impl)
                return fn

            def step(impl):
                def fn():
                    x.grad = w.grad = b.grad = None
                    gfla.instance_norm_act(x, w, b, 1e-5, SLOPE, impl).backward(up)
                return fn
            k_fwd, t_fwd = timed_pair([forward("auto"), forward("torch")], a.iters)
            k_all, t_all = timed_pair([step("auto"), step("torch")], a.iters)
            err = (forward("auto")().float() - forward("torch")().float()).abs().max().item()
            n = B * C * H * W
            k_bwd = max(k_all - k_fwd, 1e-3)
            row = {"C": C, "H": H, "W": W, "B": B, "dtype": a.worker, "regime": int(geo[0]), "threads": int(geo[1]),
                   "workgroups": int(geo[6]),
                   "kernels_fwd_us": round(k_fwd, 1), "torch_fwd_us": round(t_fwd, 1), "speedup_fwd": round(t_fwd / k_fwd, 2),
                   "kernels_fwd_bwd_us": round(k_all, 1), "torch_fwd_bwd_us": round(t_all, 1),
                   "speedup_fwd_bwd": round(t_all / k_all, 2),
                   "kernels_fwd_gbs": round(n * 2 * esize / k_fwd * 1e-3, 1),
                   "kernels_bwd_gbs": round(n * 3 * esize / k_bwd * 1e-3, 1),
                   "routes_max_abs_diff": err}
            row["kernels_fwd_share_of_6300_gbs"] = round(row["kernels_fwd_gbs"] / PEAK_GBS, 3)
            row["kernels_bwd_share_of_6300_gbs"] = round(row["kernels_bwd_gbs"] / PEAK_GBS, 3)
            print(json.dumps(row), flush=True)
            del x, up


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--limit", type=int, default=240, help="seconds a dtype's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance_norm_bench.jsonl"))
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
    by = {}
    for r in rows:
        by.setdefault(r["regime"], []).append(r)
    summary = {"tool": "bench_instance_norm", "rows": len(rows), "detail": os.path.relpath(a.out, ROOT)}
    for regime, rs in sorted(by.items()):
        summary["regime%d_speedup_fwd_min_max" % regime] = [min(r["speedup_fwd"] for r in rs), max(r["speedup_fwd"] for r in rs)]
        summary["regime%d_speedup_fwd_bwd_min_max" % regime] = [min(r["speedup_fwd_bwd"] for r in rs),
                                                               max(r["speedup_fwd_bwd"] for r in rs)]
        summary["regime%d_best_fwd_gbs" % regime] = max(r["kernels_fwd_gbs"] for r in rs)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
