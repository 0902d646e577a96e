#!/usr/bin/env python3
"""Time a generator-shaped stand-in under spectral norm (the block structure of the reference's pose generator at ngf = 64,
img_f = 512, 3 layers: encoder blocks, a residual block, three ResBlockDecoder with transposed convolutions -- the largest
matrix normalised along dim 1 is (256,128,3,3) --, a jump and an image head; 20 convolutions under torch's spectral_norm
hook) at B = 2, 128 x 128, float32, in one process:

    forward                 eval mode, no gradient:  torch hooks + MIOpen  |  fuse_spectral_norm(generator=True)
    forward + backward      torch hooks + MIOpen  |  rewritten, grad="torch"  |  rewritten, grad="kernels", pointwise="kernels"
    normalisation passes    the network's dim-1 weights in one batched call  |  the same numbers stored transposed
                            ((Cout,Cin,3,3), dim 0) in one batched call; and the largest matrix alone, both ways

usage: python tools/bench_spectral_generator.py [--iters N] [--out profiles/spectral_generator_bench.jsonl]
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

from bench_gen_conv import timed  # noqa: E402

NGF, IMG_F, LAYERS, BATCH, SIZE, SLOPE = 64, 512, 3, 2, 128, 0.1


def standin():
    """the reference's pose target net in shape, without the attention: every convolution under torch's hook"""
    from torch import nn
    from torch.nn.utils import spectral_norm as sn

    def act():
        return nn.LeakyReLU(SLOPE)

    class Encoder(nn.Module):
        def __init__(self, cin, cout):
            super(Encoder, self).__init__()
            self.model = nn.Sequential(nn.InstanceNorm2d(cin), act(), sn(nn.Conv2d(cin, cout, 4, 2, 1)),
                                       nn.InstanceNorm2d(cout), act(), sn(nn.Conv2d(cout, cout, 3, 1, 1)))

        def forward(self, x):
            return self.model(x)

    class Res(nn.Module):
        def __init__(self, c):
            super(Res, self).__init__()
            self.model = nn.Sequential(nn.InstanceNorm2d(c), act(), sn(nn.Conv2d(c, c, 3, 1, 1)),
                                       nn.InstanceNorm2d(c), act(), sn(nn.Conv2d(c, c, 3, 1, 1)))
            self.shortcut = nn.Sequential(sn(nn.Conv2d(c, c, 1)))

        def forward(self, x):
            return self.model(x) + self.shortcut(x)

    class Decoder(nn.Module):
        def __init__(self, cin, cout):
            super(Decoder, self).__init__()
            self.model = nn.Sequential(nn.InstanceNorm2d(cin), act(), sn(nn.Conv2d(cin, cin, 3, 1, 1)), nn.InstanceNorm2d(cin),
                                       act(), sn(nn.ConvTranspose2d(cin, cout, 3, 2, 1, output_padding=1)))
            self.shortcut = nn.Sequential(sn(nn.ConvTranspose2d(cin, cout, 3, 2, 1, output_padding=1)))

        def forward(self, x):
            return self.model(x) + self.shortcut(x)

    class Net(nn.Module):
        def __init__(self):
            super(Net, self).__init__()
            chans = [NGF * min(2 ** i, IMG_F // NGF) for i in range(LAYERS)]                 # 64, 128, 256
            self.encoders = nn.Sequential(*[Encoder(a, b) for a, b in zip([3] + chans[:-1], chans)])
            self.res = Res(chans[-1])
            down = chans[::-1] + [NGF]                                                       # 256, 128, 64, 64
            self.decoders = nn.ModuleList(Decoder(a, b) for a, b in zip(down[:-1], down[1:]))
            self.jump = nn.Sequential(act(), nn.ReflectionPad2d(1), sn(nn.Conv2d(chans[-1], chans[-1], 3)))
            self.out = nn.Sequential(act(), nn.ReflectionPad2d(1), sn(nn.Conv2d(NGF, 3, 3)), nn.Tanh())

        def forward(self, x):
            e = self.encoders(x)
            t = self.res(e) + self.jump(e)
            for dec in self.decoders:
                t = dec(t)
            return self.out(t)
    return Net()


def worker(a):
    import copy
    import torch
    import global_flow_local_attention_amd as gfla
    torch.manual_seed(5)
    plain = standin().cuda().train()
    nets = [copy.deepcopy(plain) for _ in range(2)]
    counts = [gfla.fuse_spectral_norm(nets[0], grad="torch", generator=True),
              gfla.fuse_spectral_norm(nets[1], grad="kernels", pointwise="kernels", generator=True)]
    image = (torch.rand(BATCH, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(6)) * 2 - 1).cuda()
    shape = {"dtype": "f32", "B": BATCH, "H": SIZE, "W": SIZE, "ngf": NGF, "img_f": IMG_F, "layers": LAYERS, "rewritten": counts}

    def infer(net):
        with torch.no_grad():
            return net(image)

    for net in [plain] + nets:
        net.eval()
    res = timed([lambda: infer(plain), lambda: infer(nets[1])], a.iters)
    print(json.dumps(dict(shape, what="forward", hooks_us=res[0][0], hooks_q1_q3_us=res[0][1:], rewritten_us=res[1][0],
                          rewritten_q1_q3_us=res[1][1:], speedup=round(res[0][0] / res[1][0], 2))), flush=True)
    for net in [plain] + nets:
        net.train()

    def train_step(net):
        net.zero_grad(set_to_none=True)
        net(image).square().mean().backward()

    res = timed([lambda: train_step(plain), lambda: train_step(nets[0]), lambda: train_step(nets[1])], a.iters)
    print(json.dumps(dict(shape, what="forward + backward", hooks_us=res[0][0], hooks_q1_q3_us=res[0][1:],
                          rewritten_torch_us=res[1][0], rewritten_torch_q1_q3_us=res[1][1:], rewritten_kernels_us=res[2][0],
                          rewritten_kernels_q1_q3_us=res[2][1:], speedup_kernels=round(res[0][0] / res[2][0], 2),
                          speedup_torch=round(res[0][0] / res[1][0], 2))), flush=True)
    # the passes: the dim-1 weights where they lie, against the same numbers stored as their matrices (dim 0)
    ups = [m for m in nets[1].modules() if type(m) is gfla.SpectralConvTranspose]
    ups.sort(key=lambda m: -m.weight_orig.numel())
    for label, members in (("all transposed convolutions", ups), ("the largest alone", ups[:1])):
        w1 = [m.weight_orig.detach().clone() for m in members]
        w0 = [w.permute(1, 0, 2, 3).contiguous() for w in w1]
        bufs = [[m.weight_u.clone() for m in members], [m.weight_v.clone() for m in members]]
        bufs0 = [[u.clone() for u in bufs[0]], [v.clone() for v in bufs[1]]]
        for iters in (1, 0):
            def dim1():
                return gfla.spectral_normalize(w1, bufs[0], bufs[1], iters, dims=[1] * len(w1))

            def dim0():
                return gfla.spectral_normalize(w0, bufs0[0], bufs0[1], iters)
            res = timed([dim1, dim0], a.iters)
            print(json.dumps({"what": "normalisation passes", "batch": label, "matrices": len(w1), "power_iterations": iters,
                              "shapes_cin_cout": [tuple(w.shape[:2]) for w in w1], "floats": sum(w.numel() for w in w1),
                              "dim1_us": res[0][0], "dim1_q1_q3_us": res[0][1:], "dim0_us": res[1][0],
                              "dim0_q1_q3_us": res[1][1:], "dim1_over_dim0": round(res[0][0] / res[1][0], 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--limit", type=int, default=240, help="seconds the child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_generator_bench.jsonl"))
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
    print(json.dumps({"tool": "bench_spectral_generator", "rows": len(rows), "detail": os.path.relpath(a.out, ROOT),
                      "forward_speedup": rows[0]["speedup"], "training_speedup_kernels": rows[1]["speedup_kernels"]}),
          flush=True)


if __name__ == "__main__":
    main()
