#!/usr/bin/env python3
"""Time the narrow 3x3 heads (head_conv3x3 impl = "auto", csrc/head_conv3x3.hip) next to the torch composition (impl =
"torch": leaky_relu, reflection pad, conv2d, tanh / sigmoid) in the same process: forward, and forward + backward (d x,
d weight, d bias), for float32 / float16 / bfloat16 maps at
    Output      (32,64,256,176) -> 3 and (1,64,256,176) -> 3     LeakyReLU(0.1), reflect, tanh
    pose heads  (32,64,64,44) -> 2+1 and (32,128,32,22) -> 2+1   zeros, identity + sigmoid, two outputs
    face heads  (8,64,64,64) -> 4+2

Per row: the median time of both routes (us), their ratio, and the op's effective GB/s from the byte model -- forward x
once plus the outputs; backward x, grad_y, y and grad_x once each -- next to the 6.3 TB/s the chip sustains.  The
backward's time is (forward + backward) - forward of the same route.  16-bit maps run the composition with 16-bit
parameters, as under autocast; the op takes float32 parameters.

usage: python tools/bench_head_conv.py [--iters N] [--out profiles/head_conv_bench.jsonl]
The parent process does not touch the GPU: every dtype is measured by a child of its own under `timeout -k 10`, and the
first child that fails ends the run.  Warm-up, then one HIP event pair per iteration, the two routes alternating; the
last line printed is one JSON summary, the rows go to --out."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, (B, Cin, H, W), Cout, split, padding, pre_slope, post
CASES = [
    ("output", (32, 64, 256, 176), 3, None, "reflect", 0.1, "tanh"),
    ("output", (1, 64, 256, 176), 3, None, "reflect", 0.1, "tanh"),
    ("pose_heads", (32, 64, 64, 44), 3, 2, "zeros", None, (None, None, "sigmoid")),
    ("pose_heads", (32, 128, 32, 22), 3, 2, "zeros", None, (None, None, "sigmoid")),
    ("face_heads", (8, 64, 64, 64), 6, 4, "zeros", None, (None,) * 4 + ("sigmoid",) * 2),
]
DTYPES = ("f32", "f16", "bf16")
PEAK_GBS = 6300.0


def timed_pair(fns, iters, warmup=5):
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
    import torch
    import global_flow_local_attention_amd as gfla
    dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[a.worker]
    esize = torch.empty((), dtype=dt).element_size()
    for name, shape, cout, split, padding, slope, post in CASES:
        B, Cin, H, W = shape
        g = torch.Generator().manual_seed(Cin + H + B)
        x = torch.randn(shape, generator=g).to(dt).cuda().requires_grad_()
        w = (torch.randn(cout, Cin, 3, 3, generator=g) * (1.5 / math.sqrt(9 * Cin))).cuda().requires_grad_()
        b = (0.3 * torch.randn(cout, generator=g)).cuda().requires_grad_()
        w_t = w.detach().to(dt).requires_grad_()      # what the composition multiplies with
        b_t = b.detach().to(dt).requires_grad_()
        up = torch.randn(B, cout, H, W, generator=g).to(dt).cuda()
        ups = (up,) if split is None else (up[:, :split].contiguous(), up[:, split:].contiguous())

        def run(impl):
            ww, bb = (w, b) if impl == "auto" else (w_t, b_t)
            y = gfla.head_conv3x3(x, ww, bb, padding, slope, post, split, impl)
            return y if isinstance(y, tuple) else (y,)

        def forward(impl):
            def fn():
                with torch.no_grad():
                    return run(impl)
            return fn

        def step(impl):
            def fn():
                x.grad = w.grad = b.grad = w_t.grad = b_t.grad = None
                torch.autograd.backward(run(impl), ups)
            return fn
        k_fwd, t_fwd = timed_pair([forward("auto"), forward("torch")], a.iters)
        k_all, t_all = timed_pair([step("auto"), step("torch")], a.iters)
        err = max((p.float() - q.float()).abs().max().item() for p, q in zip(forward("auto")(), forward("torch")()))
        px = B * H * W
        k_bwd = max(k_all - k_fwd, 1e-3)
        fwd_bytes = px * (Cin + cout) * esize
        bwd_bytes = px * (2 * Cin + 2 * cout) * esize
        row = {"case": name, "B": B, "Cin": Cin, "H": H, "W": W, "Cout": cout, "dtype": a.worker,
               "kernels_fwd_us": round(k_fwd, 1), "torch_fwd_us": round(t_fwd, 1), "speedup_fwd": round(t_fwd / k_fwd, 2),
               "kernels_fwd_bwd_us": round(k_all, 1), "torch_fwd_bwd_us": round(t_all, 1),
               "speedup_fwd_bwd": round(t_all / k_all, 2),
               "kernels_fwd_gbs": round(fwd_bytes / k_fwd * 1e-3, 1), "kernels_bwd_gbs": round(bwd_bytes / k_bwd * 1e-3, 1),
               "routes_max_abs_diff": err}
        row["kernels_fwd_share_of_6300_gbs"] = round(row["kernels_fwd_gbs"] / PEAK_GBS, 3)
        row["kernels_bwd_share_of_6300_gbs"] = round(row["kernels_bwd_gbs"] / PEAK_GBS, 3)
        print(json.dumps(row), flush=True)
        del x, up, ups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--limit", type=int, default=240, help="seconds a dtype's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_conv_bench.jsonl"))
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
    summary = {"tool": "bench_head_conv", "rows": len(rows), "detail": os.path.relpath(a.out, ROOT),
               "speedup_fwd_min_max": [min(r["speedup_fwd"] for r in rows), max(r["speedup_fwd"] for r in rows)],
               "speedup_fwd_bwd_min_max": [min(r["speedup_fwd_bwd"] for r in rows), max(r["speedup_fwd_bwd"] for r in rows)],
               "best_fwd_gbs": max(r["kernels_fwd_gbs"] for r in rows)}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
