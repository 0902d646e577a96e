#!/usr/bin/env python3
"""Time the 1x1 convolutions of the stand-in discriminator (tools/bench_discriminator.py: ndf 32, img_f 128, 4 blocks, B = 8,
256 x 256) on the library's kernels (gen_conv.conv1x1, csrc/conv1x1.hip) next to F.avg_pool2d + F.conv2d through MIOpen,
in one process:

    per layer               forward (no gradient), and forward + backward with all three gradients, float32 and bfloat16:
                            3 -> 32 at 256 x 256 pooled, 32 -> 64 at 128 x 128 pooled, 64 -> 128 at 64 x 64 pooled,
                            128 -> 1 at 16 x 16; the forward's compulsory bytes (x read once, y written once) per second
                            next to the 8 TB/s HBM peak
    whole step              forward + backward of the stand-in, float32: torch hooks + MIOpen | fuse_spectral_norm(grad="torch")
                            | grad="kernels" | grad="kernels", pointwise="kernels"

usage: python tools/bench_conv1x1.py [--iters N] [--out profiles/conv1x1_bench.jsonl]
Method as tools/bench_discriminator.py: the parent process does not touch the GPU, the measurement runs in a child under
`timeout -k 10`; every route is warmed up; the routes alternate inside each round; one HIP event pair per call, medians and
quartiles (us).  No pass bar."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_discriminator import BATCH, standin  # noqa: E402
from bench_gen_conv import timed  # noqa: E402

HBM_PEAK = 8.0e12
# (Cin, Cout, H, W, pool) at B = BATCH
LAYERS = ((3, 32, 256, 256, 2), (32, 64, 128, 128, 2), (64, 128, 64, 64, 2), (128, 1, 16, 16, 1))


def layer_rows(a):
    import torch
    import torch.nn.functional as F
    import global_flow_local_attention_amd as gfla
    for dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        for cin, cout, H, W, pool in LAYERS:
            g = torch.Generator().manual_seed(cin + cout)
            x = torch.randn(BATCH, cin, H, W, generator=g).to(dtype).cuda()
            w = (torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5).cuda()
            b = (torch.randn(cout, generator=g) * 0.2).cuda()
            wt, bt = w.to(dtype), b.to(dtype)                       # the vendor route gets its parameters in x's dtype
            up = torch.randn(BATCH, cout, H // pool, W // pool, generator=g).to(dtype).cuda()

            def vendor(x, w, b):
                return F.conv2d(F.avg_pool2d(x, 2, 2) if pool == 2 else x, w, b)

            def fwd_kernels():
                with torch.no_grad():
                    return gfla.conv1x1(x, w, b, pool=pool)

            def fwd_vendor():
                with torch.no_grad():
                    return vendor(x, wt, bt)

            def step(fn, params):
                leaves = [t.detach().requires_grad_() for t in params]
                fn(*leaves).backward(up)

            def train_kernels():
                step(lambda x, w, b: gfla.conv1x1(x, w, b, pool=pool, grad="kernels"), (x, w, b))

            def train_vendor():
                step(vendor, (x, wt, bt))

            res = timed([fwd_vendor, fwd_kernels, train_vendor, train_kernels], a.iters)
            moved = (x.numel() + up.numel()) * x.element_size()
            row = {"what": "layer", "dtype": name, "B": BATCH, "Cin": cin, "Cout": cout, "H": H, "W": W, "pool": pool,
                   "fwd_vendor_us": res[0][0], "fwd_vendor_q1_q3_us": res[0][1:], "fwd_kernels_us": res[1][0],
                   "fwd_kernels_q1_q3_us": res[1][1:], "train_vendor_us": res[2][0], "train_vendor_q1_q3_us": res[2][1:],
                   "train_kernels_us": res[3][0], "train_kernels_q1_q3_us": res[3][1:], "fwd_bytes": moved,
                   "fwd_kernels_tb_per_s": round(moved / res[1][0] / 1e6, 3),
                   "fwd_kernels_of_hbm_peak": round(moved / res[1][0] * 1e6 / HBM_PEAK, 3),
                   "fwd_speedup": round(res[0][0] / res[1][0], 2), "train_speedup": round(res[2][0] / res[3][0], 2)}
            print(json.dumps(row), flush=True)


def network_row(a):
    import copy
    import torch
    import global_flow_local_attention_amd as gfla
    torch.manual_seed(5)
    plain = standin().cuda().train()
    nets = [copy.deepcopy(plain) for _ in range(3)]
    counts = [gfla.fuse_spectral_norm(nets[0], grad="torch"), gfla.fuse_spectral_norm(nets[1], grad="kernels"),
              gfla.fuse_spectral_norm(nets[2], grad="kernels", pointwise="kernels")]
    image = (torch.rand(BATCH, 3, 256, 256, generator=torch.Generator().manual_seed(6)) * 2 - 1).cuda()

    def train_step(net):
        net.zero_grad(set_to_none=True)
        net(image).square().mean().backward()

    res = timed([lambda: train_step(plain)] + [lambda net=net: train_step(net) for net in nets], a.iters)
    row = {"what": "network", "dtype": "f32", "B": BATCH, "H": 256, "W": 256, "rewritten": counts,
           "hooks_us": res[0][0], "hooks_q1_q3_us": res[0][1:], "rewritten_torch_us": res[1][0],
           "rewritten_torch_q1_q3_us": res[1][1:], "rewritten_kernels_us": res[2][0], "rewritten_kernels_q1_q3_us": res[2][1:],
           "pointwise_kernels_us": res[3][0], "pointwise_kernels_q1_q3_us": res[3][1:],
           "pointwise_over_kernels": round(res[3][0] / res[2][0], 3), "speedup_pointwise": round(res[0][0] / res[3][0], 2)}
    print(json.dumps(row), flush=True)


def worker(a):
    layer_rows(a)
    network_row(a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--limit", type=int, default=300, help="seconds the child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv1x1_bench.jsonl"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", "--iters", str(a.iters)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(done.stdout)
    sys.stdout.flush()
    if done.returncode != 0:
        sys.exit("the child ended with status %d" % done.returncode)
    rows = [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(json.dumps(r) for r in rows) + "\n")
    print(json.dumps({"tool": "bench_conv1x1", "rows": len(rows), "detail": os.path.relpath(a.out, ROOT),
                      "network_pointwise_over_kernels": rows[-1]["pointwise_over_kernels"]}), flush=True)


if __name__ == "__main__":
    main()
