#!/usr/bin/env python3
"""float64 ExtractorAttn forward + backward: the FP64 matrix-core path (fc_f64.py, csrc/gemm_f64.hip) against
fc_impl = "library" (torch.mm / F.conv2d: rocBLAS / MIOpen), and gfla_gemm_f64 against torch.mm in float64 at the
three GEMM shapes of the first FC layer.  One JSON line per row; the variants alternate inside every step, after warm-up,
each timed between device synchronisations.

    python tools/bench_f64_attn.py [--steps 5] [--warmup 2] [--shapes attn2_256x176,attn3_256x176] [--out file.jsonl]

FLOP counts come from the shapes: the first FC layer is 2*128*(C*k*k)*(B*H*W) per half and product; a block forward
+ backward does it 6 times (two halves x forward, weight gradient, data gradient).  No share of an FP64 peak is given.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import global_flow_local_attention_amd as gfla  # noqa: E402
from global_flow_local_attention_amd import fc_f64  # noqa: E402

SHAPES = {"attn2_256x176": (32, 128, 64, 44, 5), "attn3_256x176": (32, 256, 32, 22, 3)}
DEV = "cuda:0"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def block_step(mod, inputs, up):
    def run():
        for x in inputs:
            x.grad = None
        mod.zero_grad(set_to_none=True)
        mod(*inputs).backward(up)
    return run


def gemm_pair(M, N, K):
    """(ours, torch.mm) closures for C (M x N) = A (M x K) . B (K x N), all row-major float64."""
    a = torch.randn(M, K, dtype=torch.float64, device=DEV)
    b = torch.randn(K, N, dtype=torch.float64, device=DEV)
    c = torch.empty(M, N, dtype=torch.float64, device=DEV)
    av = fc_f64.view(fc_f64.axis((M, K)), fc_f64.axis((K, 1)))
    bv = fc_f64.view(fc_f64.axis((K, N)), fc_f64.axis((N, 1)))
    cv = fc_f64.view(fc_f64.axis((M, N)), fc_f64.axis((N, 1)))
    ours = lambda: fc_f64.gemm(c, cv, a, av, b, bv, M, N, K)
    ref = lambda: torch.mm(a, b, out=c)
    ours()
    want = torch.mm(a, b)
    err = (c - want).abs().max().item() / want.abs().max().item()
    return ours, ref, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_f64_attn: needs a GPU (no CPU timing is reported)")
    rows = []
    for name in a.shapes.split(","):
        B, C, H, W, k = SHAPES[name]
        ckk, n = C * k * k, B * H * W
        torch.manual_seed(0)
        mod = gfla.ExtractorAttn(C, k, torch.nn.LeakyReLU(0.2), softmax=True).double().to(DEV)
        mod.vendor_fallback = "allow"
        inputs = [torch.randn(B, C, H, W, dtype=torch.float64, device=DEV).requires_grad_(),
                  torch.randn(B, C, H, W, dtype=torch.float64, device=DEV).requires_grad_(),
                  (torch.randn(B, 2, H, W, dtype=torch.float64, device=DEV) * 3).requires_grad_()]
        up = torch.randn(B, C, H, W, dtype=torch.float64, device=DEV)
        step = block_step(mod, inputs, up)

        def with_impl(impl):
            def run():
                mod.fc_impl = impl
                step()
            return run

        variants = {"fp64_mfma": with_impl("mfma"), "library": with_impl("library")}
        gemms = {"fwd": (128, n, ckk), "wgrad": (128, ckk, n), "dgrad": (ckk, n, 128)}
        gemm_err = {}
        for g, (M, N, K) in gemms.items():
            ours, ref, gemm_err[g] = gemm_pair(M, N, K)
            variants["gemm_%s_ours" % g], variants["gemm_%s_torch_mm" % g] = ours, ref
        times = {v: [] for v in variants}
        for it in range(a.warmup + a.steps):
            for v, fn in variants.items():
                dt = timed(fn)
                if it >= a.warmup:
                    times[v].append(dt)
        med = {v: statistics.median(ts) for v, ts in times.items()}
        fc_flop = 6 * 2 * 128 * ckk * n
        row = {"shape": name, "B": B, "C": C, "H": H, "W": W, "k": k, "steps": a.steps, "warmup": a.warmup,
               "block_ms": {"fp64_mfma": med["fp64_mfma"] * 1e3, "library": med["library"] * 1e3},
               "block_speedup_vs_library": med["library"] / med["fp64_mfma"],
               "block_fc_gemm_flop": fc_flop,
               "block_fc_tflops_fp64_mfma_end_to_end": fc_flop / med["fp64_mfma"] / 1e12,
               "block_spread_ms": {v: [min(times[v]) * 1e3, max(times[v]) * 1e3] for v in ("fp64_mfma", "library")},
               "gemm": {}}
        for g, (M, N, K) in gemms.items():
            flop = 2 * M * N * K
            to, tr = med["gemm_%s_ours" % g], med["gemm_%s_torch_mm" % g]
            row["gemm"][g] = {"M": M, "N": N, "K": K, "flop": flop, "ours_ms": to * 1e3, "torch_mm_ms": tr * 1e3,
                              "ours_tflops": flop / to / 1e12, "torch_mm_tflops": flop / tr / 1e12,
                              "rate_vs_torch_mm": tr / to, "max_rel_err_vs_torch_mm": gemm_err[g]}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del mod, inputs, up, variants
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
