#!/usr/bin/env python3
"""Time the pose-input ops (global_flow_local_attention_amd/pose_inputs.py, csrc/pose_inputs.hip) at B = 32, J = 18, at
256 x 176 and 128 x 64 (key points given in a 256 x 176 frame), for float32 and float16 outputs, in the same process:

    maps_kernel      pose_maps on the kernel, into one of three output buffers in turn (312 MB at 256 x 176 float32: more
                     than the 256 MB of the last-level cache), with the bytes it stores per second
    maps_torch       the torch composition of the same expressions on the same device
    maps_host        the composition on CPU tensors plus the copy of its float32 result from pinned memory to the device:
                     what a loader that builds the maps itself delivers; a host clock around work that ends in a
                     device synchronise, the host being whatever CPU the tool runs on
    images_kernel    normalize_images on the kernel
    images_torch     u8.permute(0, 3, 1, 2).float().div(255).sub(.5).div(.5) on the device

Per row: us per call -- the median of --repeats windows of --steps calls between two device events, the routes alternating
window by window, with the smallest and largest window beside it.  The host route takes --host-steps calls per window.

usage: python tools/bench_pose_inputs.py [--steps 40] [--repeats 5] [--out profiles/pose_inputs_bench.jsonl]
The parent process does not touch the GPU: every (size, dtype) is measured by a child of its own under `timeout -k 10`,
and the first child that fails ends the run -- without a GPU that is the first one.  The last line printed is one JSON
summary, the rows go to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, J, OLD = 32, 18, (256, 176)
SIZES = ((256, 176), (128, 64))
DTYPES = ("f32", "f16")
ROUTES = ("maps_kernel", "maps_torch", "maps_host", "images_kernel", "images_torch")


def worker(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pose_inputs: no GPU; nothing is measured without one")
    import global_flow_local_attention_amd as gfla
    size_name, name = a.worker.split(":")
    H, W = (int(s) for s in size_name.split("x"))
    dt = {"f32": torch.float32, "f16": torch.float16}[name]
    g = torch.Generator().manual_seed(1)
    cords_host = torch.stack([torch.randint(0, OLD[0], (B, J), generator=g), torch.randint(0, OLD[1], (B, J), generator=g)], dim=2)
    cords_host[:, 5] = -1                                                   # a missing joint per sample, as in the data
    cords = cords_host.cuda()
    u8 = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    outs = [torch.empty((B, J, H, W), dtype=dt, device="cuda") for _ in range(3)]
    imgs = [torch.empty((B, 3, H, W), dtype=dt, device="cuda") for _ in range(3)]
    pinned = torch.empty((B, J, H, W), dtype=torch.float32, pin_memory=True)
    landing = torch.empty((B, J, H, W), dtype=torch.float32, device="cuda")
    turn = [0]

    def maps_kernel():
        turn[0] = (turn[0] + 1) % 3
        gfla.pose_maps(cords, (H, W), old_size=OLD, dtype=dt, out=outs[turn[0]])

    def maps_torch():
        gfla.pose_maps(cords, (H, W), old_size=OLD, dtype=dt, impl="torch")

    def maps_host():
        pinned.copy_(gfla.pose_maps(cords_host, (H, W), old_size=OLD))
        landing.copy_(pinned, non_blocking=True)

    def images_kernel():
        turn[0] = (turn[0] + 1) % 3
        gfla.normalize_images(u8, dtype=dt, out=imgs[turn[0]])

    def images_torch():
        u8.permute(0, 3, 1, 2).float().div(255).sub(.5).div(.5).to(dt)

    fns = dict(maps_kernel=maps_kernel, maps_torch=maps_torch, maps_host=maps_host, images_kernel=images_kernel,
               images_torch=images_torch)
    assert int((gfla.pose_maps(cords, (H, W), old_size=OLD).view(torch.int32)
                - gfla.pose_maps(cords, (H, W), old_size=OLD, impl="torch").view(torch.int32)).abs().max()) <= 1
    for route in ROUTES:
        for _ in range(1 if route == "maps_host" else 10):
            fns[route]()
    torch.cuda.synchronize()
    windows = {r: [] for r in ROUTES}
    for _ in range(a.repeats):
        for route in ROUTES:
            if route == "maps_host":
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.host_steps):
                    maps_host()
                torch.cuda.synchronize()
                windows[route].append((time.perf_counter() - t0) * 1e6 / a.host_steps)
                continue
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                fns[route]()
            t1.record()
            t1.synchronize()
            windows[route].append(t0.elapsed_time(t1) * 1e3 / a.steps)
    esize = 4 if name == "f32" else 2
    for route in ROUTES:
        w = windows[route]
        us = statistics.median(w)
        row = {"size": size_name, "dtype": name, "B": B, "J": J, "route": route, "us_per_call": round(us, 1),
               "us_min_max": [round(min(w), 1), round(max(w), 1)],
               "calls_timed": (a.host_steps if route == "maps_host" else a.steps) * a.repeats}
        if route == "maps_kernel":
            stored = B * J * H * W * esize
            row.update(bytes_stored=stored, stored_gbs=round(stored / us * 1e-3, 1))
        if route == "images_kernel":
            moved = B * 3 * H * W * (1 + esize)
            row.update(bytes_moved=moved, moved_gbs=round(moved / us * 1e-3, 1))
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="calls per timed window of a device route")
    ap.add_argument("--host-steps", type=int, default=2, help="calls per timed window of the host route")
    ap.add_argument("--repeats", type=int, default=5, help="windows per route; steps x repeats >= 200 per figure")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_inputs_bench.jsonl"))
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.steps * a.repeats < 200:
        sys.exit("bench_pose_inputs: at least 200 calls per figure (got %d x %d)" % (a.steps, a.repeats))
    rows = []
    for H, W in SIZES:
        for name in DTYPES:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker",
                   "%dx%d:%s" % (H, W, name), "--steps", str(a.steps), "--host-steps", str(a.host_steps), "--repeats", str(a.repeats)]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(done.stdout)
            sys.stdout.flush()
            if done.returncode != 0:
                sys.exit("the %dx%d:%s child ended with status %d: nothing more is started" % (H, W, name, done.returncode))
            rows += [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(json.dumps(r) for r in rows) + "\n")
    summary = {"tool": "bench_pose_inputs", "rows": len(rows), "detail": os.path.relpath(a.out, ROOT)}
    for r in rows:
        if r["route"] != "maps_kernel":
            continue
        same = {o["route"]: o for o in rows if (o["size"], o["dtype"]) == (r["size"], r["dtype"])}
        summary["%s_%s" % (r["size"], r["dtype"])] = {
            "maps_kernel_us": r["us_per_call"], "stored_gbs": r["stored_gbs"],
            "maps_torch_over_kernel": round(same["maps_torch"]["us_per_call"] / r["us_per_call"], 1),
            "maps_host_over_kernel": round(same["maps_host"]["us_per_call"] / r["us_per_call"], 1),
            "images_kernel_us": same["images_kernel"]["us_per_call"],
            "images_torch_over_kernel": round(same["images_torch"]["us_per_call"] / same["images_kernel"]["us_per_call"], 1)}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
