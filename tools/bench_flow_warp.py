#!/usr/bin/env python3
"""Time the bilinear flow warp on the library's kernels (flow_warp impl = "auto", csrc/flow_warp.hip) next to the torch
composition (impl = "torch": normalised grid + F.grid_sample) in the same process: forward, and forward + backward to the
flow (what the sampling-correctness loss asks for; the source needs no gradient there), in the "correctness" convention
at the loss's layer shapes (C = 128 at 64 x 64, C = 256 at 32 x 32, B = 32) for float32 / float16 / bfloat16 sources
with a float32 flow.  16-bit rows run both routes under torch.autocast("cuda", dtype), and every row reports the largest
warp error of both routes against the float64 host evaluation on the same stored inputs (first --truth-batch samples).

usage: python tools/bench_flow_warp.py [--iters N] [--out profiles/flow_warp_bench.jsonl]
The parent process does not touch the GPU: every dtype is measured by a child of its own under `timeout -k 10`, and the
first child that fails ends the run.  Warm-up, then one HIP event pair per iteration; the median is reported (us)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(128, 64, 64), (256, 32, 32)]   # C, H, W
DTYPES = ("f32", "f16", "bf16")


def timed(fn, iters, warmup=10):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times)


def worker(a):
    import torch
    import global_flow_local_attention_amd as gfla
    dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[a.worker]
    half = dt != torch.float32
    for C, H, W in SHAPES:
        g = torch.Generator().manual_seed(C + H)
        stored = torch.randn(a.batch, C, H, W, generator=g).relu().to(dt)
        flow_host = torch.randn(a.batch, 2, H, W, generator=g) * a.flow_std
        up_host = torch.randn(a.batch, C, H, W, generator=g)
        n = min(a.truth_batch, a.batch)
        truth = gfla.flow_warp(stored[:n].double(), flow_host[:n].double(), "correctness")       # host tensors, float64
        src, up = stored.cuda(), up_host.cuda()
        flow = flow_host.cuda().requires_grad_()
        row = {"C": C, "H": H, "W": W, "B": a.batch, "dtype": a.worker, "autocast": half, "flow_std_px": a.flow_std}
        for impl in ("auto", "torch"):
            def forward():
                with torch.autocast("cuda", dtype=dt, enabled=half):
                    return gfla.flow_warp(src, flow.detach(), "correctness", impl)

            def step():
                flow.grad = None
                with torch.autocast("cuda", dtype=dt, enabled=half):
                    out = gfla.flow_warp(src, flow, "correctness", impl)
                out.backward(up)
            key = "kernels" if impl == "auto" else "torch"
            row[key + "_fwd_us"] = round(timed(forward, a.iters), 1)
            row[key + "_fwd_bwd_flow_us"] = round(timed(step, a.iters), 1)
            row[key + "_warp_max_err"] = (forward()[:n].double().cpu() - truth).abs().max().item()
        row["speedup_fwd"] = round(row["torch_fwd_us"] / row["kernels_fwd_us"], 2)
        row["speedup_fwd_bwd_flow"] = round(row["torch_fwd_bwd_flow_us"] / row["kernels_fwd_bwd_flow_us"], 2)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--flow-std", type=float, default=3.0, help="standard deviation of the flow in pixels")
    ap.add_argument("--truth-batch", type=int, default=4, help="samples of the batch evaluated in float64 on the host")
    ap.add_argument("--limit", type=int, default=180, help="seconds a dtype's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_warp_bench.jsonl"))
    ap.add_argument("--worker", choices=DTYPES, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    rows = []
    for name in DTYPES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", name,
               "--iters", str(a.iters), "--batch", str(a.batch), "--flow-std", str(a.flow_std),
               "--truth-batch", str(a.truth_batch)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(done.stdout)
        sys.stdout.flush()
        if done.returncode != 0:
            sys.exit("the %s child ended with status %d: nothing more is started" % (name, done.returncode))
        rows += [line for line in done.stdout.splitlines() if line.startswith("{")]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
