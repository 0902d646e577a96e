#!/usr/bin/env python3
"""Time the Gram-difference L1 of VGGLoss's style term, forward + backward (d/d generated features only, as in training),
on the library's kernels (gram_l1 impl = "auto", csrc/gram_l1.hip) next to the torch composition (impl = "torch":
compute_gram + l1_loss, the reference's arithmetic) in the same process, at the four style layers of a 256x256 and of a
256x176 image, B = 32, for float32 features and for float16 / bfloat16 features under torch.autocast("cuda", dtype), as the
trainer runs them.  Also reports the loss error of both against the host float64 value on the same stored features.
Features: relu(1.5 randn + 0.2), the target drawn separately.

usage: python tools/bench_style_loss.py [--iters N] [--batch B] [--out profiles/style_loss_bench.jsonl]
Warm-up, then one HIP event pair per iteration; the median is reported (us)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import global_flow_local_attention_amd as gfla  # noqa: E402

SHAPES = [  # layer, C, H, W
    ("relu2_2", 128, 128, 128), ("relu3_4", 256, 64, 64), ("relu4_4", 512, 32, 32), ("relu5_2", 512, 16, 16),
    ("relu2_2", 128, 128, 88), ("relu3_4", 256, 64, 44), ("relu4_4", 512, 32, 22), ("relu5_2", 512, 16, 11),
]
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def timed(fn, iters, warmup=5):
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "style_loss_bench.jsonl"))
    a = ap.parse_args()
    rows = []
    for i, (layer, C, H, W) in enumerate(SHAPES):
        g = torch.Generator().manual_seed(i)
        x32, y32 = (torch.relu(1.5 * torch.randn(a.batch, C, H, W, generator=g) + 0.2) for _ in range(2))
        for name, dt in DTYPES.items():
            xs, ys = x32.to(dt), y32.to(dt)
            host = gfla.gram_l1(xs.double(), ys.double()).item()       # CPU tensors: the composition, float64
            x, y = xs.cuda().requires_grad_(), ys.cuda()
            half = dt != torch.float32
            row = {"layer": layer, "C": C, "H": H, "W": W, "B": a.batch, "dtype": name, "autocast": half,
                   "host_float64_loss": host}
            for impl in ("auto", "torch"):
                def step():
                    x.grad = None
                    with torch.autocast("cuda", dtype=dt, enabled=half):
                        loss = gfla.gram_l1(x, y, impl=impl)
                    loss.backward()
                    return loss
                key = "kernels" if impl == "auto" else "torch"
                row[key + "_us"] = round(timed(step, a.iters), 1)
                row[key + "_loss_rel_err"] = abs(step().item() - host) / abs(host)
            row["speedup"] = round(row["torch_us"] / row["kernels_us"], 2)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del x, y
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
