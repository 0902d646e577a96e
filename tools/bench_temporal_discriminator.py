#!/usr/bin/env python3
"""Time a forward + backward of a stand-in of the reference's TemporalDiscriminator(input_length=6, ndf=32, img_f=128,
layers=4) -- two ResBlock3DEncoder, two ResBlockEncoder, a final 1x1, sixteen convolutions under torch's spectral_norm hook --
at B = 2, 256 x 256, in float32 and under bfloat16 autocast, in one process, on three routes:

    hooks + MIOpen          the network as built: torch's hooks, F.conv3d, F.avg_pool3d, F.conv2d
    rewritten, grad torch   patch_reference_discriminators(grad="torch", pointwise="kernels", temporal="kernels"): the batched
                            normalisation, frames-major blocks, but every convolution that needs a gradient on its torch
                            composition (a permuted view into F.conv3d)
    rewritten, kernels      the same with grad="kernels": csrc/conv3d.hip, csrc/avg_pool_frames.hip, csrc/conv1x1.hip and the
                            2-D kernels, no vendor convolution or pool

usage: python tools/bench_temporal_discriminator.py [--iters N] [--out profiles/temporal_discriminator_bench.jsonl]
Method as tools/bench_discriminator.py: the parent process does not touch the GPU, the measurement runs in a child under
`timeout -k 10`; every route is warmed up; the routes alternate inside each round; one HIP event pair per call, medians and
quartiles (us).  No pass bar: the acceptance of this route is the vendor fence and the parity tests, not a speed-up."""
import argparse
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_gen_conv import timed  # noqa: E402

LENGTH, NDF, IMG_F, LAYERS, BATCH, SIZE, SLOPE = 6, 32, 128, 4, 2, 256, 0.1


def standin():
    """fresh classes (Block3D, Block2D, Net) in the reference's shape, without norm layers"""
    from torch import nn
    from torch.nn.utils import spectral_norm as sn

    class Block3D(nn.Module):
        def __init__(self, cin, cout, hidden):
            super(Block3D, self).__init__()
            self.model = nn.Sequential(nn.LeakyReLU(SLOPE), sn(nn.Conv3d(cin, hidden, (3, 3, 3), 1, (1, 1, 1))),
                                       nn.LeakyReLU(SLOPE), sn(nn.Conv3d(hidden, cout, (3, 4, 4), (1, 2, 2), (0, 1, 1))))
            self.shortcut = nn.Sequential(nn.AvgPool3d((3, 2, 2), (1, 2, 2)), sn(nn.Conv3d(cin, cout, 1)))

        def forward(self, x):
            return self.model(x) + self.shortcut(x)

    class Block2D(nn.Module):
        def __init__(self, cin, cout, hidden):
            super(Block2D, self).__init__()
            self.model = nn.Sequential(nn.LeakyReLU(SLOPE), sn(nn.Conv2d(cin, hidden, 3, 1, 1)), nn.LeakyReLU(SLOPE),
                                       sn(nn.Conv2d(hidden, cout, 4, 2, 1)))
            self.shortcut = nn.Sequential(nn.AvgPool2d(2, 2), sn(nn.Conv2d(cin, cout, 1)))

        def forward(self, x):
            return self.model(x) + self.shortcut(x)

    class Net(nn.Module):
        def __init__(self):
            super(Net, self).__init__()
            self.layers = LAYERS
            self.nonlinearity = nn.LeakyReLU(SLOPE)
            self.block0 = Block3D(3, NDF, NDF)
            self.block1 = Block3D(NDF, 2 * NDF, NDF)
            mult = 2 * (LENGTH - 4)
            for i in range(LAYERS - 2):
                prev, mult = mult, min(2 ** (i + 2), IMG_F // NDF)
                setattr(self, "encoder" + str(i), Block2D(NDF * prev, NDF * mult, NDF * prev))
            self.conv = sn(nn.Conv2d(NDF * mult, 1, 1))

        def forward(self, x):
            out = self.block1(self.block0(x))
            b, c, l, h, w = out.shape
            out = out.view(b, -1, h, w)
            for i in range(self.layers - 2):
                out = getattr(self, "encoder" + str(i))(out)
            return self.conv(self.nonlinearity(out))
    return Block3D, Block2D, Net


def worker(a):
    import torch
    import global_flow_local_attention_amd as gfla
    torch.manual_seed(5)
    plain = standin()[2]().cuda().train()
    nets = [plain]
    for grad in ("torch", "kernels"):
        block3d, block2d, net_cls = standin()
        gfla.patch_reference_discriminators(types.SimpleNamespace(TemporalDiscriminator=net_cls),
                                            types.SimpleNamespace(ResBlock3DEncoder=block3d, ResBlockEncoder=block2d),
                                            grad=grad, pointwise="kernels", temporal="kernels")
        net = net_cls()
        net.load_state_dict(plain.state_dict())
        nets.append(net.cuda().train())
    video = (torch.rand(BATCH, 3, LENGTH, SIZE, SIZE, generator=torch.Generator().manual_seed(6)) * 2 - 1).cuda()
    for name in ("f32", "bf16"):
        def train_step(net):
            net.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=name == "bf16"):
                out = net(video)
            out.float().square().mean().backward()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=name == "bf16"):
            outs = [net.eval()(video).float() for net in nets]
        for net in nets:
            net.train()
        diff = [((o - outs[0]).abs().max() / outs[0].abs().max()).item() for o in outs[1:]]
        res = timed([lambda n=n: train_step(n) for n in nets], a.iters)
        row = {"what": "temporal discriminator", "dtype": name, "B": BATCH, "L": LENGTH, "H": SIZE, "W": SIZE, "ndf": NDF,
               "img_f": IMG_F, "layers": LAYERS, "hooks_us": res[0][0], "hooks_q1_q3_us": res[0][1:],
               "rewritten_torch_us": res[1][0], "rewritten_torch_q1_q3_us": res[1][1:], "rewritten_kernels_us": res[2][0],
               "rewritten_kernels_q1_q3_us": res[2][1:], "speedup_torch": round(res[0][0] / res[1][0], 2),
               "speedup_kernels": round(res[0][0] / res[2][0], 2), "routes_rel_diff": diff}
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds the child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_discriminator_bench.jsonl"))
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
    print(json.dumps({"tool": "bench_temporal_discriminator", "rows": len(rows), "detail": os.path.relpath(a.out, ROOT),
                      "speedup_kernels": {r["dtype"]: r["speedup_kernels"] for r in rows}}), flush=True)


if __name__ == "__main__":
    main()
