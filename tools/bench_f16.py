"""ExtractorAttn forward + backward with float16, bfloat16 and float32 features (float32: arithmetic mode 5, the default) at
the face shapes and the bench shapes, and Resample2d(4, 1, sigma=2) forward + backward at the same maps.  HIP events, warm-up,
median of the timed repetitions; one JSON line per row.  Runs well under two minutes.

    python tools/bench_f16.py [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [  # (name, B, C, H, W, k)
    ("face_k3", 8, 256, 32, 32, 3),
    ("face_k5", 8, 128, 64, 64, 5),
    ("bench_k5", 32, 128, 64, 44, 5),
    ("bench_k3", 32, 256, 32, 22, 3),
]
DTYPES = (("f16", torch.float16), ("bf16", torch.bfloat16), ("f32", torch.float32))


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import global_flow_local_attention_amd as gfla
    dev = "cuda:0"
    torch.manual_seed(0)
    for name, B, C, H, W, k in SHAPES:
        m = gfla.ExtractorAttn(C, k, torch.nn.LeakyReLU(0.1), softmax=True).to(dev)
        with torch.no_grad():
            m.fully_connect_layer[0].bias.copy_(torch.where(torch.arange(128, device=dev) % 2 == 0, 8.0, -8.0))
        rs = gfla.Resample2d(4, 1, sigma=2)
        s32, t32 = torch.randn(B, C, H, W, device=dev), torch.randn(B, C, H, W, device=dev)
        f32 = torch.randn(B, 2, H, W, device=dev) * 2
        for dname, dt in DTYPES:
            s, t, f = (x.to(dt).requires_grad_() for x in (s32, t32, f32))
            up = torch.randn(B, C, H, W, device=dev).to(dt)

            def attn_step():
                m.zero_grad(set_to_none=True)
                for x in (s, t, f):
                    x.grad = None
                m(s, t, f).backward(up)

            def rs_step():
                s.grad = f.grad = None
                rs(s, f).backward(up)

            for op, fn in (("ExtractorAttn", attn_step), ("Resample2d", rs_step)):
                med, best = _time(fn, args.reps, args.warmup)
                print(json.dumps({"op": op, "shape": name, "B": B, "C": C, "H": H, "W": W, "k": k, "dtype": dname,
                                  "fwd_bwd_ms_median": round(med, 4), "fwd_bwd_ms_min": round(best, 4)}), flush=True)


if __name__ == "__main__":
    main()
