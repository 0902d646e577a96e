#!/usr/bin/env python3
"""Time the spectral normalisation and a forward + backward of a discriminator-shaped stand-in (the block structure of the
reference's ResDiscriminator at ndf = 32, img_f = 128, layers = 4: 13 convolutions under torch's spectral_norm hook,
0.66 M weights, the largest matrix 128 x 2048) at B = 8, 256 x 256, float32, in one process:

    normalisation alone     the 13 hooks' compute_weight, one after the other (3 gemv, 2 normalisations, a dot and a
                            division each)  |  one batched call (spectral_norm.spectral_normalize, csrc/spectral_norm.hip)
    forward + backward      torch hooks + MIOpen  |  fuse_spectral_norm(grad="torch")  |  fuse_spectral_norm(grad="kernels")

usage: python tools/bench_discriminator.py [--iters N] [--out profiles/discriminator_bench.jsonl]
Method as tools/bench_gen_conv.py: the parent process does not touch the GPU, the measurement runs in a child under
`timeout -k 10`; every route is warmed up; the routes alternate inside each round; one HIP event pair per call, medians
and quartiles (us).  The normalisation is launch-bound, so next to the event time the host's wall clock per call (a
window of calls that ends in a synchronise) is reported as well.  --profile-only ROUTE runs one route's normalisation a
few times and nothing else, for a kernel trace of its own.  No pass bar."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_gen_conv import timed  # noqa: E402

NDF, IMG_F, LAYERS, BATCH, SIZE, SLOPE = 32, 128, 4, 8, 256, 0.1


def standin():
    """the reference's ResDiscriminator in shape: ResBlockEncoder blocks without norm layers and a final 1x1"""
    from torch import nn
    from torch.nn.utils import spectral_norm as sn

    class Block(nn.Module):
        def __init__(self, cin, cout, hidden):
            super(Block, self).__init__()
            self.model = nn.Sequential(nn.LeakyReLU(SLOPE), sn(nn.Conv2d(cin, hidden, 3, 1, 1)), nn.LeakyReLU(SLOPE),
                                       sn(nn.Conv2d(hidden, cout, 4, 2, 1)))
            self.shortcut = nn.Sequential(nn.AvgPool2d(2, 2), sn(nn.Conv2d(cin, cout, 1)))

        def forward(self, x):
            return self.model(x) + self.shortcut(x)

    class Net(nn.Module):
        def __init__(self):
            super(Net, self).__init__()
            blocks, mult = [Block(3, NDF, NDF)], 1
            for i in range(LAYERS - 1):
                prev, mult = mult, min(2 ** (i + 1), IMG_F // NDF)
                blocks.append(Block(NDF * prev, NDF * mult, NDF * prev))
            self.blocks = nn.ModuleList(blocks)
            self.act = nn.LeakyReLU(SLOPE)
            self.conv = sn(nn.Conv2d(NDF * mult, 1, 1))

        def forward(self, x):
            for block in self.blocks:
                x = block(x)
            return self.conv(self.act(x))
    return Net()


def wall_us(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / calls * 1e6, 1)


def worker(a):
    import copy
    import torch
    from torch import nn
    import global_flow_local_attention_amd as gfla
    torch.manual_seed(5)
    plain = standin().cuda().train()
    hooked = [m for m in plain.modules() if type(m) is nn.Conv2d and "weight_orig" in m._parameters]
    hooks = [next(iter(m._forward_pre_hooks.values())) for m in hooked]
    batch_net = copy.deepcopy(plain)
    gfla.fuse_spectral_norm(batch_net)
    convs = [m for m in batch_net.modules() if type(m) is gfla.SpectralConv]
    ws, us, vs = [c.weight_orig for c in convs], [c.weight_u for c in convs], [c.weight_v for c in convs]

    def norm_hooks():
        return [h.compute_weight(m, True) for h, m in zip(hooks, hooked)]

    def norm_batched():
        return gfla.spectral_normalize(ws, us, vs, 1)

    if a.profile_only:
        fn = {"hooks": norm_hooks, "batched": norm_batched}[a.profile_only]
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        return
    diff = max(((x - y).abs().max() / y.abs().max()).item() for x, y in zip(norm_batched(), norm_hooks()))
    res = timed([norm_hooks, norm_batched], a.iters)
    row = {"what": "normalisation", "matrices": len(convs), "floats": sum(w.numel() for w in ws),
           "hooks_us": res[0][0], "hooks_q1_q3_us": res[0][1:], "batched_us": res[1][0], "batched_q1_q3_us": res[1][1:],
           "hooks_wall_us": wall_us(norm_hooks, 50), "batched_wall_us": wall_us(norm_batched, 50),
           "speedup": round(res[0][0] / res[1][0], 2), "routes_rel_diff": diff}
    print(json.dumps(row), flush=True)
    nets = [copy.deepcopy(plain) for _ in range(2)]
    counts = [gfla.fuse_spectral_norm(nets[0], grad="torch"), gfla.fuse_spectral_norm(nets[1], grad="kernels")]
    image = (torch.rand(BATCH, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(6)) * 2 - 1).cuda()

    def train_step(net):
        net.zero_grad(set_to_none=True)
        net(image).square().mean().backward()

    res = timed([lambda: train_step(plain), lambda: train_step(nets[0]), lambda: train_step(nets[1])], a.iters)
    row = {"what": "network", "dtype": "f32", "B": BATCH, "H": SIZE, "W": SIZE, "ndf": NDF, "img_f": IMG_F, "layers": LAYERS,
           "rewritten": counts, "hooks_us": res[0][0], "hooks_q1_q3_us": res[0][1:], "rewritten_torch_us": res[1][0],
           "rewritten_torch_q1_q3_us": res[1][1:], "rewritten_kernels_us": res[2][0], "rewritten_kernels_q1_q3_us": res[2][1:],
           "speedup_kernels": round(res[0][0] / res[2][0], 2), "speedup_torch": round(res[0][0] / res[1][0], 2)}
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--limit", type=int, default=200, help="seconds the child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "discriminator_bench.jsonl"))
    ap.add_argument("--profile-only", choices=("hooks", "batched"), help="run that route's normalisation ten times, no timing")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker or a.profile_only:
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
    print(json.dumps({"tool": "bench_discriminator", "rows": len(rows), "detail": os.path.relpath(a.out, ROOT),
                      "normalisation_speedup": rows[0]["speedup"], "network_speedup_kernels": rows[1]["speedup_kernels"]}),
          flush=True)


if __name__ == "__main__":
    main()
