#!/usr/bin/env python3
"""Time the image-input ops (global_flow_local_attention_amd/image_inputs.py, csrc/image_inputs.hip) at B = 32, in the
same process per child:

    affine_rotated     affine_images at 256 x 176 x 3 with rotations (the fixed-point branch), both of its launches, into
                       one of three output buffers in turn
    affine_scaled      the same with angle 0 (the scale branch: two table reads per pixel)
    normalize          normalize_images at the same shape and dtype: the same bytes read and written without the gather
    resize_bilinear    resize_images 1101 x 750 -> 256 x 176, both passes
    resize_bicubic
    pil_affine_host    Image.transform(AFFINE, NEAREST) + ToTensor/Normalize arithmetic in numpy, image by image, on the HOST:
    pil_resize_host    Image.resize(BICUBIC), image by image, on the HOST -- CPU figures of whatever machine the tool runs
                       on, one core, a host clock; only where Pillow is importable

Per row: us per call (a batch of 32) -- the median of --repeats windows of --steps calls between two device events, the
routes alternating window by window, with the smallest and largest window beside it.  The host routes take --host-steps
calls per window.

usage: python tools/bench_image_inputs.py [--steps 40] [--repeats 5] [--out profiles/image_inputs_bench.jsonl]
The parent process does not touch the GPU: every child (affine:f32, affine:f16, resize:u8) runs under `timeout -k 10`, and
the first child that fails ends the run -- without a GPU that is the first one.  The last line printed is one JSON
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

B, SIZE, RAW = 32, (256, 176), (1101, 750)
CHILDREN = ("affine:f32", "affine:f16", "resize:u8")


def timed(fns, routes, host_routes, a):
    import torch
    for route in routes:
        for _ in range(1 if route in host_routes else 10):
            fns[route]()
    torch.cuda.synchronize()
    windows = {r: [] for r in routes}
    for _ in range(a.repeats):
        for route in routes:
            if route in host_routes:
                t0 = time.perf_counter()
                for _ in range(a.host_steps):
                    fns[route]()
                windows[route].append((time.perf_counter() - t0) * 1e6 / a.host_steps)
                continue
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                fns[route]()
            t1.record()
            t1.synchronize()
            windows[route].append(t0.elapsed_time(t1) * 1e3 / a.steps)
    return windows


def worker(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_image_inputs: no GPU; nothing is measured without one")
    import global_flow_local_attention_amd as gfla
    try:
        from PIL import Image
    except ImportError:
        Image = None
    import numpy as np
    what, name = a.worker.split(":")
    g = torch.Generator().manual_seed(1)
    H, W = SIZE
    turn = [0]
    if what == "affine":
        dt = {"f32": torch.float32, "f16": torch.float16}[name]
        host = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
        u8 = host.cuda()
        angles = (torch.rand(B, generator=g) * 60 - 30).tolist()
        shifts = (torch.rand(B, 2, generator=g) * 40 - 20).tolist()
        scales = (torch.rand(B, generator=g) * 0.5 + 0.8).tolist()
        rotated, _ = gfla.augmentation_matrices(angles, shifts, scales, SIZE)
        scaled, _ = gfla.augmentation_matrices([0.0] * B, shifts, scales, SIZE)
        outs = [torch.empty((B, 3, H, W), dtype=dt, device="cuda") for _ in range(3)]
        for m in (rotated, scaled):
            assert torch.equal(gfla.affine_images(u8[:2], m[:2].cuda(), dtype=dt).cpu(), gfla.affine_images(host[:2], m[:2], dtype=dt))
        rotated_dev, scaled_dev = rotated.cuda(), scaled.cuda()

        def affine(m):
            turn[0] = (turn[0] + 1) % 3
            gfla.affine_images(u8, m, 128, dtype=dt, out=outs[turn[0]])

        def normalize():
            turn[0] = (turn[0] + 1) % 3
            gfla.normalize_images(u8, dtype=dt, out=outs[turn[0]])

        def pil_affine_host():
            for b in range(B):
                warped = Image.fromarray(host[b].numpy(), "RGB").transform((W, H), Image.AFFINE, rotated[b].reshape(-1).tolist(),
                                                                             Image.NEAREST, fillcolor=(128, 128, 128))
                ((np.asarray(warped).transpose(2, 0, 1).astype(np.float32) / np.float32(255)) - np.float32(0.5)) / np.float32(0.5)
        fns = dict(affine_rotated=lambda: affine(rotated_dev), affine_scaled=lambda: affine(scaled_dev), normalize=normalize,
                   pil_affine_host=pil_affine_host)
        host_routes = ("pil_affine_host",)
        routes = ("affine_rotated", "affine_scaled", "normalize") + (host_routes if Image is not None and name == "f32" else ())
        moved = B * 3 * H * W * (1 + dt.itemsize)
    else:
        host = torch.randint(0, 256, (B,) + RAW + (3,), dtype=torch.uint8, generator=g)
        u8 = host.cuda()
        outs = [torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(3)]
        for f in ("bilinear", "bicubic"):
            assert torch.equal(gfla.resize_images(u8[:1], SIZE, f).cpu(), gfla.resize_images(host[:1], SIZE, f))

        def resize(f):
            turn[0] = (turn[0] + 1) % 3
            gfla.resize_images(u8, SIZE, f, out=outs[turn[0]])

        def pil_resize_host():
            for b in range(B):
                Image.fromarray(host[b].numpy(), "RGB").resize((W, H), Image.BICUBIC)
        fns = dict(resize_bilinear=lambda: resize("bilinear"), resize_bicubic=lambda: resize("bicubic"), pil_resize_host=pil_resize_host)
        host_routes = ("pil_resize_host",)
        routes = ("resize_bilinear", "resize_bicubic") + (host_routes if Image is not None else ())
        moved = B * 3 * (RAW[0] * RAW[1] + 2 * RAW[0] * W + H * W)       # the source, the intermediate twice, the result
    windows = timed(fns, routes, host_routes, a)
    for route in routes:
        w = windows[route]
        us = statistics.median(w)
        row = {"op": what, "dtype": name, "B": B, "route": route, "us_per_call": round(us, 1),
               "us_min_max": [round(min(w), 1), round(max(w), 1)],
               "calls_timed": (a.host_steps if route in host_routes else a.steps) * a.repeats}
        if route in host_routes:
            row["where"] = "host CPU of this machine, one core, Pillow %s" % __import__("PIL").__version__
        else:
            row.update(bytes_moved=moved, moved_gbs=round(moved / us * 1e-3, 1))
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="calls per timed window of a device route")
    ap.add_argument("--host-steps", type=int, default=1, help="calls per timed window of a host route")
    ap.add_argument("--repeats", type=int, default=5, help="windows per route; steps x repeats >= 200 per figure")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_inputs_bench.jsonl"))
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.steps * a.repeats < 200:
        sys.exit("bench_image_inputs: at least 200 calls per figure (got %d x %d)" % (a.steps, a.repeats))
    rows = []
    for child in CHILDREN:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", child,
               "--steps", str(a.steps), "--host-steps", str(a.host_steps), "--repeats", str(a.repeats)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(done.stdout)
        sys.stdout.flush()
        if done.returncode != 0:
            sys.exit("the %s child ended with status %d: nothing more is started" % (child, done.returncode))
        rows += [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(json.dumps(r) for r in rows) + "\n")
    by = {(r["op"], r["dtype"], r["route"]): r["us_per_call"] for r in rows}
    summary = {"tool": "bench_image_inputs", "rows": len(rows), "detail": os.path.relpath(a.out, ROOT)}
    for name in ("f32", "f16"):
        base = by[("affine", name, "normalize")]
        summary["affine_" + name] = {"rotated_us": by[("affine", name, "affine_rotated")], "scaled_us": by[("affine", name, "affine_scaled")],
                                     "normalize_us": base, "rotated_over_normalize": round(by[("affine", name, "affine_rotated")] / base, 2),
                                     "scaled_over_normalize": round(by[("affine", name, "affine_scaled")] / base, 2)}
    summary["resize"] = {"bilinear_us": by[("resize", "u8", "resize_bilinear")], "bicubic_us": by[("resize", "u8", "resize_bicubic")]}
    for key, route in (("pil_affine_host_us", ("affine", "f32", "pil_affine_host")), ("pil_resize_host_us", ("resize", "u8", "pil_resize_host"))):
        if route in by:
            summary[key] = by[route]
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
