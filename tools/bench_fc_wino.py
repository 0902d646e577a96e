#!/usr/bin/env python3
"""HIP-event times of the first FC layer's kernels, one at a time (gfla_fc_kernel_f32, as bench.py's fc_kernel_probes times
them), at the two bench layers with B = 32 in arithmetic modes 4 and 5: one JSON row per (layer, mode, which).  which = 0 / 1
forward convolution of the source / target half, 2 / 3 data gradient, 4 / 5 weight gradient, 6 / 7 both convolutions in one
launch, 8 both weight gradients in one launch.  In mode 5 the k = 5 convolutions and every data gradient run on the direct
kernels: controls for a change to the Winograd-domain kernels.

    GFLA_HIP_LIBRARY=/path/to/other/libgfla_hip.so python tools/bench_fc_wino.py --label parent --round 1

compares two builds: alternate the two libraries process by process (P P N P N P N) and judge every row of the new one
against the range of the old one's, widened by the difference of its first two rounds."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from global_flow_local_attention_amd import _lib, fc_mfma  # noqa: E402

LAYERS = ((5, 128, 64, 44), (3, 256, 32, 22))   # (k, C, H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="tree")
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev, B, p = "cuda:0", a.batch, _lib.ptr
    for k, C, H, W in LAYERS:
        g = torch.Generator().manual_seed(k)
        s, t = (torch.randn(B, C, H, W, generator=g).to(dev) for _ in range(2))
        f = (torch.randn(B, 2, H, W, generator=g) * 1.5).to(dev)
        w0 = (torch.randn(128, 2 * C, k, k, generator=g) / (2 * C * k * k) ** 0.5).to(dev)
        w1 = (torch.randn(k * k, 128, generator=g) * 0.1).to(dev)
        gl = (torch.randn(B, k * k, H, W, generator=g) * 1e-3).to(dev)
        for mode in (4, 5):
            if fc_mfma.resolve_mode(C, H, W, k, mode) != mode:
                continue
            ws = torch.empty(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 0), dtype=torch.uint8, device=dev)
            sc = torch.empty(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 1), dtype=torch.uint8, device=dev)
            logits = torch.empty(B, k * k, H, W, device=dev)
            gs, gt, gf, gw0 = torch.zeros_like(s), torch.empty_like(t), torch.zeros_like(f), torch.empty_like(w0)
            _lib.call("gfla_fc_forward_f32", s, p(s), p(t), p(f), p(w0), None, p(w1), None, p(ws), p(logits), B, C, H, W, k, 0.1, mode)
            _lib.call("gfla_fc_backward_f32", s, p(ws), p(f), p(w1), p(gl), p(sc), p(gs), p(gt), p(gf), p(gw0), None, None, None,
                      B, C, H, W, k, 0.1, mode, 0)
            stream = torch.cuda.current_stream(dev)
            for which in range(9):
                for _ in range(3):
                    _lib.call("gfla_fc_kernel_f32", s, which, p(ws), p(sc), B, C, H, W, k, mode)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.iters):
                    _lib.call("gfla_fc_kernel_f32", s, which, p(ws), p(sc), B, C, H, W, k, mode)
                e1.record(stream)
                torch.cuda.synchronize()
                print(json.dumps({"lib": a.label, "round": a.round, "dims": [B, C, H, W, k], "mode": mode, "which": which,
                                  "avg_us": round(e0.elapsed_time(e1) / a.iters * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
