#!/usr/bin/env python3
"""Time the reconstruction metrics (global_flow_local_attention_amd/recon_metrics.py, csrc/recon_metrics.hip) at B = 32,
256 x 176 x 3, window 51, in one child process:

    metrics_all        reconstruction_metrics of two uint8 batches, all five numbers: four launches
    metrics_ssim       ... ssim alone (the uniform 51 x 51 window and the finishing launch)
    metrics_ssim_256   ... ssim_256 alone (pixel sums for the range, the Gaussian window, the finishing launch)
    metrics_pixels     ... psnr, l1 and mae alone
    to_uint8_f32       images_to_uint8 of a float32 (32, 3, 256, 176) batch, into one of three output buffers in turn
    to_uint8_f16       the same of a float16 batch
    metrics_torch_gpu  torch_reconstruction_metrics on the device: the float64 composition the tests compare with
    host_scipy         the same batch image by image through numpy + scipy.ndimage on the HOST, the reference's pipeline
                       (uniform_filter / gaussian_filter in float64); only where scipy is importable
    host_torch         torch_reconstruction_metrics on the HOST, where scipy is not importable
                       -- the two host rows are CPU figures of whatever machine the tool runs on, a host clock

Per row: us per call (a batch of 32) -- the median of --repeats windows of --steps calls between two device events, the
routes alternating window by window, with the smallest and largest window beside it.  The host routes take --host-steps
calls per window and --host-repeats windows, without a warm-up call.  Before anything is timed the kernels' numbers are
compared with the composition's at the timed shape (two images), and the largest distance is printed.

usage: python tools/bench_recon_metrics.py [--steps 40] [--repeats 5] [--out profiles/recon_metrics_bench.jsonl]
The parent process does not touch the GPU: the child runs under `timeout -k 10`; without a GPU it fails and nothing is
measured.  The last line printed is one JSON summary, the rows go to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W, C, WIN = 32, 256, 176, 3, 51


def host_scipy(pred, gt):
    """script/metrics.py:322-344 for one batch, image by image, with the two scipy.ndimage filters skimage calls"""
    import numpy as np
    from scipy.ndimage import gaussian_filter, uniform_filter

    def ssim(X, Y, filt, cov_norm, pad, R):
        C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
        means = []
        for c in range(X.shape[2]):
            x, y = X[..., c].astype(np.float64), Y[..., c].astype(np.float64)
            ux, uy, uxx, uyy, uxy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
            vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
            S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
            means.append(S[pad:-pad, pad:-pad].mean())
        return np.mean(means)
    out = []
    N = WIN * WIN
    for b in range(pred.shape[0]):
        a, p = gt[b].astype(np.float32) / 255.0, pred[b].astype(np.float32) / 255.0
        d = a.astype(np.float64) - p.astype(np.float64)
        a256, p256 = a * 255.0, p * 255.0
        out.append((ssim(a, p, lambda v: uniform_filter(v, size=WIN), N / (N - 1.0), WIN // 2, 1.0),
                    ssim(a256, p256, lambda v: gaussian_filter(v, sigma=1.5, truncate=3.5), 1.0, 5, float(p256.max() - p256.min())),
                    10 * np.log10(1.0 / np.mean(d * d)), np.mean(np.abs(d)), np.sum(np.abs(d)) / np.sum(a.astype(np.float64) + p)))
    return out


def worker(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_recon_metrics: no GPU; nothing is measured without one")
    import global_flow_local_attention_amd as gfla
    try:
        import scipy.ndimage  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    g = torch.Generator().manual_seed(1)
    # a smooth picture and a noisy copy: random bytes would be the one input without structure
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([128 + 80 * torch.sin(0.05 * xs + c) * torch.cos(0.04 * ys) for c in range(C)], -1)
    gt_host = (base[None] + 12 * torch.randn(B, H, W, C, generator=g)).clamp(0, 255).to(torch.uint8)
    pred_host = (gt_host.float() * 0.9 + 20 * torch.randn(B, H, W, C, generator=g) + 8).clamp(0, 255).to(torch.uint8)
    pred, gt = pred_host.cuda(), gt_host.cuda()
    maps = {"f32": torch.rand(B, C, H, W, generator=g).mul(2).sub(1).cuda()}
    maps["f16"] = maps["f32"].half()
    outs = [torch.empty((B, H, W, C), dtype=torch.uint8, device="cuda") for _ in range(3)]
    turn = [0]
    got = gfla.reconstruction_metrics(pred[:2], gt[:2], WIN)
    want = gfla.torch_reconstruction_metrics(pred_host[:2], gt_host[:2], WIN)
    distance = max((got[k].cpu() - want[k]).abs().max().item() for k in want)
    assert distance <= 5e-7, distance
    for name, x in maps.items():
        assert torch.equal(gfla.images_to_uint8(x[:2]).cpu(), gfla.torch_images_to_uint8(x[:2].cpu())), name
    print(json.dumps({"check": "kernels against the composition at the timed shape", "largest_distance": distance}), flush=True)

    def to_uint8(name):
        turn[0] = (turn[0] + 1) % 3
        gfla.images_to_uint8(maps[name], out=outs[turn[0]])
    pred_np, gt_np = pred_host.numpy(), gt_host.numpy()
    fns = {"metrics_all": lambda: gfla.reconstruction_metrics(pred, gt, WIN),
           "metrics_ssim": lambda: gfla.reconstruction_metrics(pred, gt, WIN, ("ssim",)),
           "metrics_ssim_256": lambda: gfla.reconstruction_metrics(pred, gt, WIN, ("ssim_256",)),
           "metrics_pixels": lambda: gfla.reconstruction_metrics(pred, gt, WIN, ("psnr", "l1", "mae")),
           "to_uint8_f32": lambda: to_uint8("f32"), "to_uint8_f16": lambda: to_uint8("f16"),
           "metrics_torch_gpu": lambda: gfla.torch_reconstruction_metrics(pred, gt, WIN),
           "host_scipy": lambda: host_scipy(pred_np, gt_np),
           "host_torch": lambda: gfla.torch_reconstruction_metrics(pred_host, gt_host, WIN)}
    host_routes = ("host_scipy",) if have_scipy else ("host_torch",)
    slow = ("metrics_torch_gpu",)
    routes = [r for r in fns if not r.startswith("host_")] + list(host_routes)
    for route in routes:
        for _ in range(0 if route in host_routes else 1 if route in slow else 10):
            fns[route]()
    torch.cuda.synchronize()
    windows = {r: [] for r in routes}
    for window in range(a.repeats):
        for route in routes:
            if route in host_routes:
                if window >= a.host_repeats:
                    continue
                t0 = time.perf_counter()
                for _ in range(a.host_steps):
                    fns[route]()
                windows[route].append((time.perf_counter() - t0) * 1e6 / a.host_steps)
                continue
            steps = max(a.steps // 10, 1) if route in slow else a.steps
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                fns[route]()
            t1.record()
            t1.synchronize()
            windows[route].append(t0.elapsed_time(t1) * 1e3 / steps)
    for route in routes:
        w = windows[route]
        row = {"route": route, "B": B, "shape": [H, W, C], "win_size": WIN, "us_per_call": round(statistics.median(w), 1),
               "us_min_max": [round(min(w), 1), round(max(w), 1)],
               "calls_timed": a.host_steps * min(a.host_repeats, a.repeats) if route in host_routes
               else (max(a.steps // 10, 1) if route in slow else a.steps) * a.repeats}
        if route in host_routes:
            row["where"] = "host CPU of this machine, %d torch threads, a host clock" % torch.get_num_threads()
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="calls per timed window of a device route")
    ap.add_argument("--host-steps", type=int, default=1, help="calls per timed window of a host route")
    ap.add_argument("--repeats", type=int, default=5, help="windows per route; steps x repeats >= 200 per figure")
    ap.add_argument("--host-repeats", type=int, default=2, help="windows of a host route (seconds each)")
    ap.add_argument("--limit", type=int, default=420, help="seconds the child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_metrics_bench.jsonl"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.steps * a.repeats < 200:
        sys.exit("bench_recon_metrics: at least 200 calls per figure (got %d x %d)" % (a.steps, a.repeats))
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(a.steps),
           "--host-steps", str(a.host_steps), "--repeats", str(a.repeats), "--host-repeats", str(a.host_repeats)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(done.stdout)
    sys.stdout.flush()
    if done.returncode != 0:
        sys.exit("the child ended with status %d" % done.returncode)
    rows = [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{") and "route" in line]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(json.dumps(r) for r in rows) + "\n")
    by = {r["route"]: r["us_per_call"] for r in rows}
    summary = {"tool": "bench_recon_metrics", "rows": len(rows), "detail": os.path.relpath(a.out, ROOT)}
    summary.update({k + "_us": v for k, v in by.items()})
    host = by.get("host_scipy", by.get("host_torch"))
    summary["host_over_kernels"] = round(host / by["metrics_all"], 1)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
