#!/usr/bin/env python3
"""Time AffineRegularizationLoss forward + backward on the library's kernels (impl = "auto", csrc/affine_reg.hip) next to
the torch composition (impl = "torch") in the same process, at the attention-layer flow shapes of a 256x176 / 256x256
image, B = 32, for float32 / float16 / bfloat16 flows.  16-bit rows run both paths under torch.autocast("cuda", dtype), as
the trainer does, and also report the loss error of both against the host float64 value on the same stored flow.

usage: python tools/bench_affine_reg.py [--iters N] [--out profiles/affine_reg_bench.jsonl]
Warm-up, then one HIP event pair per iteration; the median is reported (us)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import global_flow_local_attention_amd as gfla  # noqa: E402

SHAPES = [(32, 22, 3), (64, 44, 5), (32, 32, 3), (64, 64, 5)]   # H, W, kz
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def smooth_flow(B, H, W, amplitude, seed=0):
    """Three plane waves of at most 1.5 periods across the map per (b, axis), peak `amplitude` px (float64, host)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1) / H
    x = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W) / W
    f = torch.zeros(B, 2, H, W, dtype=torch.float64)
    for _ in range(3):
        fy, fx = (torch.rand(B, 2, 1, 1, generator=g, dtype=torch.float64) * 3 - 1.5 for _ in range(2))
        phase = torch.rand(B, 2, 1, 1, generator=g, dtype=torch.float64) * 2 * math.pi
        f = f + torch.sin(2 * math.pi * (fy * y + fx * x) + phase)
    return f * (amplitude / f.abs().amax(dim=(2, 3), keepdim=True))


def timed(fn, iters, warmup=10):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--amplitude", type=float, default=0.5, help="peak of the smooth flow field in pixels")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_reg_bench.jsonl"))
    a = ap.parse_args()
    rows = []
    for H, W, kz in SHAPES:
        for name, dt in DTYPES.items():
            stored = smooth_flow(a.batch, H, W, a.amplitude).to(dt)
            flow = stored.cuda().requires_grad_()
            host = gfla.AffineRegularizationLoss(kz)(stored.double()).item()     # CPU tensors: the composition, float64
            half = dt != torch.float32
            row = {"H": H, "W": W, "kz": kz, "B": a.batch, "dtype": name, "autocast": half, "amplitude_px": a.amplitude,
                   "host_float64_loss": host}
            for impl in ("auto", "torch"):
                mod = gfla.AffineRegularizationLoss(kz, impl=impl)

                def step():
                    flow.grad = None
                    with torch.autocast("cuda", dtype=dt, enabled=half):
                        loss = mod(flow)
                    loss.backward()
                    return loss
                key = "kernels" if impl == "auto" else "torch"
                row[key + "_us"] = round(timed(step, a.iters), 1)
                row[key + "_loss_rel_err"] = abs(step().item() - host) / abs(host)
            row["speedup"] = round(row["torch_us"] / row["kernels_us"], 2)
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
