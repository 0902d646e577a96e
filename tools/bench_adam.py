#!/usr/bin/env python3
"""Time one optimizer step of FusedAdam (global_flow_local_attention_amd/adam.py, csrc/adam.hip) next to torch.optim.Adam
in three forms -- foreach=False, the default (foreach), fused=True -- in the same process, for float32 parameters and for
bfloat16 parameters (FusedAdam: float32 masters and moments; torch: bfloat16 moments, no masters -- another arithmetic,
timed for its traffic only); float32 also through a torch.amp.GradScaler (`scaler.step(opt); scaler.update()`), which
refuses bfloat16 gradients on every route (its inf check has no bfloat16 kernel).

Parameter sets: "warp" -- the parameters of tools/warp_generator.py's network at ngf = 64 --, and "synthetic" -- 270 tensors,
about 14 M elements, in the size mix of the reference's PoseGenerator: a few dozen 3x3 and 1x1 convolution weights at 64 to
256 channels that hold nearly all elements, and two hundred bias and norm vectors.  The tool sets the gradients itself
(0.01 randn, scaled by the scaler's scale where there is one); betas = (0, 0.999), the reference's.

Per row: us per step -- the median of --repeats windows of --steps steps between two device events, the routes
alternating window by window, with the smallest and largest window beside it --, kernel launches per step (counted by
torch.profiler over two steps, null where the profiler gives nothing), and for FusedAdam the bytes per step of the byte
model -- float32: p 4 + 4, g 4, v 4 + 4, m 4 (+ 4 when beta1 != 0) per element; bfloat16: p 2, g 2, master 4 + 4, the same
moments -- over the time, as a share of the 6.29 TB/s the chip sustains (MI355X_MICROARCH.md, HBM3E, float4 copy).

usage: python tools/bench_adam.py [--steps 40] [--repeats 5] [--out profiles/adam_bench.jsonl]
The parent process does not touch the GPU: every (dtype, parameter set) is measured by a child of its own under
`timeout -k 10`, and the first child that fails ends the run -- without a GPU that is the first one.  The last line printed
is one JSON summary, the rows go to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DTYPES = ("f32", "bf16")
SETS = ("warp", "synthetic")
ROUTES = ("kernels", "torch_foreach_false", "torch_default", "torch_fused")
PEAK_GBS = 6290.0
BETAS = (0.0, 0.999)
LR = 1e-4


def synthetic_shapes():
    shapes = [(256, 256, 3, 3)] * 17 + [(128, 128, 3, 3)] * 20 + [(64, 64, 3, 3)] * 20 + [(256, 128, 1, 1)] * 10
    shapes += [(256,)] * 68 + [(128,)] * 68 + [(64,)] * 67
    assert len(shapes) == 270
    return shapes


def warp_shapes():
    import warp_generator
    net = warp_generator.WarpGenerator(3, 18, 3, 64)
    return [tuple(p.shape) for p in net.parameters() if p.requires_grad]


def bytes_per_step(numel, dtype_name, beta1):
    moments = 4 + 4 + 4 + (4 if beta1 != 0 else 0)
    return numel * ((4 + 4 + 4 if dtype_name == "f32" else 2 + 2 + 4 + 4) + moments)


def make_route(route, shapes, dt, scaled):
    """step(): one optimizer step of `route` on its own copy of the parameters, through a GradScaler when `scaled`"""
    import torch
    from global_flow_local_attention_amd import FusedAdam
    g = torch.Generator().manual_seed(1)
    scale = 2.0 ** 10 if scaled else 1.0
    ps = [torch.nn.Parameter((0.1 * torch.randn(s, generator=g)).to(dt).cuda()) for s in shapes]
    for p in ps:
        p.grad = (0.01 * scale * torch.randn(p.shape, generator=g)).to(dt).cuda()
    if route == "kernels":
        opt = FusedAdam(ps, lr=LR, betas=BETAS)
    else:
        kw = {"torch_foreach_false": dict(foreach=False), "torch_default": {}, "torch_fused": dict(fused=True)}[route]
        opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, **kw)
    if not scaled:
        return opt.step
    scaler = torch.amp.GradScaler("cuda", init_scale=scale, growth_interval=10 ** 9)
    scaler.scale(torch.zeros(1, device="cuda"))

    def step():
        scaler.step(opt)
        scaler.update()
    return step


def launches_per_step(step):
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            step()
            torch.cuda.synchronize()
        count = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                    and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return count / 2.0 if count else None
    except Exception:
        return None


def worker(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_adam: no GPU; nothing is measured without one")
    name, which = a.worker.split(":")
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[name]
    shapes = warp_shapes() if which == "warp" else synthetic_shapes()
    numel = sum(int(torch.Size(s).numel()) for s in shapes)
    for scaled in ((False, True) if name == "f32" else (False,)):     # the scaler's inf check has no bfloat16 kernel in torch
        steps = [make_route(r, shapes, dt, scaled) for r in ROUTES]
        for fn in steps:
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        windows = [[] for _ in ROUTES]
        for _ in range(a.repeats):
            for w, fn in zip(windows, steps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.steps):
                    fn()
                t1.record()
                t1.synchronize()
                w.append(t0.elapsed_time(t1) * 1e3 / a.steps)
        for route, w, fn in zip(ROUTES, windows, steps):
            us = statistics.median(w)
            row = {"dtype": name, "set": which, "tensors": len(shapes), "numel": numel, "route": route, "grad_scaler": scaled,
                   "us_per_step": round(us, 1), "us_min_max": [round(min(w), 1), round(max(w), 1)],
                   "steps_timed": a.steps * a.repeats, "launches_per_step": launches_per_step(fn)}
            if route == "kernels":
                gbs = bytes_per_step(numel, name, BETAS[0]) / us * 1e-3
                row.update(bytes_per_step=bytes_per_step(numel, name, BETAS[0]), gbs=round(gbs, 1),
                           share_of_6290_gbs=round(gbs / PEAK_GBS, 3))
            print(json.dumps(row), flush=True)
        del steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="steps per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per route; steps x repeats >= 200 per figure")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_bench.jsonl"))
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.steps * a.repeats < 200:
        sys.exit("bench_adam: at least 200 steps per figure (got %d x %d)" % (a.steps, a.repeats))
    rows = []
    for name in DTYPES:
        for which in SETS:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker",
                   "%s:%s" % (name, which), "--steps", str(a.steps), "--repeats", str(a.repeats)]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(done.stdout)
            sys.stdout.flush()
            if done.returncode != 0:
                sys.exit("the %s:%s child ended with status %d: nothing more is started" % (name, which, done.returncode))
            rows += [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(json.dumps(r) for r in rows) + "\n")
    summary = {"tool": "bench_adam", "rows": len(rows), "detail": os.path.relpath(a.out, ROOT)}
    for r in rows:
        if r["route"] != "kernels":
            continue
        key = "%s_%s_%s" % (r["dtype"], r["set"], "scaler" if r["grad_scaler"] else "plain")
        others = {o["route"]: o for o in rows if (o["dtype"], o["set"], o["grad_scaler"]) == (r["dtype"], r["set"], r["grad_scaler"])}
        summary[key] = {"kernels_us": r["us_per_step"], "share_of_6290_gbs": r["share_of_6290_gbs"],
                        "torch_default_over_kernels": round(others["torch_default"]["us_per_step"] / r["us_per_step"], 2),
                        "torch_fused_over_kernels": round(others["torch_fused"]["us_per_step"] / r["us_per_step"], 2)}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
