"""Shared by tests/test_fc_wino_family_gpu.py and tests/golden/make_fc_wino_digests.py: the cases of the Winograd-domain
kernels of the first FC layer (csrc/fc_wino.hip, csrc/fc_wino16.hip on csrc/fc_wino_shared.h / fc_wino_wgrad.h: fc_wino_conv_kernel,
fc_wino16_conv_kernel, fc_wino_wgrad_kernel, fc_wino16_wgrad_kernel) whose outputs are pinned bit for bit, and their
SHA-256 digests.  Everything goes through the C entry points gfla_fc_conv_fwd_f32 / gfla_fc_conv_bwd_f32 (one half of the
layer, called the way test_fc_wino_gpu.py's _run_half does) and gfla_fc_forward_f32 / gfla_fc_backward_f32 (both halves:
the two-job launches), so the same code runs on any revision of the library.

Every output buffer is filled with a finite sentinel before the call and digested WHOLE -- out (B, Mg, 128), grad_x,
grad_w0 -- so a stray or a missing write shows as well as a changed value.

Pinned: every per-half output (forward map, grad_x, grad_w0) in arithmetic modes 4 and 5 under every tuning variant below,
and of the whole layer logits and grad_target.  NOT pinned: the whole layer's grad_source, grad_flow and grad_w0 -- they
sit behind the splat of the sampled map's gradient into the source map (csrc/fc_sample.hip: float atomics in free order;
test_fc_wino_gpu.py's two-job test has seen their last bits move from run to run).  At these small shapes the recorder's
runs agreed on them, which is no promise: the recorder reports them and leaves them out."""
import hashlib

import torch

from global_flow_local_attention_amd import _lib, fc_mfma
from util import randn

DEV = "cuda:0"
SENTINEL = -7.25
MODES = (4, 5)
# (k, B, C, H, W), by the path they reach (tests/golden/make_fc_wino_digests.py prints the geometry of each):
RAGGED = [(5, 1, 5, 3, 3), (3, 1, 5, 3, 3), (5, 3, 17, 7, 5), (3, 3, 17, 7, 5)]   # partial tiles both ways, < one tile group, C < one chunk
CHUNKS = [(5, 1, 33, 13, 31), (3, 1, 40, 13, 31)]     # several input chunks: the stage_next branch of the step loop
# one raw buffer (DB = false), two input chunks so that the forward commits between its two barriers as well ((3, 1, 16, 10, 200)
# is too wide for any Winograd mode: it falls back to the direct kernels)
SINGLE_RAW = [(5, 1, 24, 9, 120), (3, 1, 24, 10, 100)]
ROWS = [(3, 4, 32, 32, 22), (3, 2, 24, 12, 30), (5, 2, 16, 20, 26)]   # whole-tile-row groups (tpg != 32), multi-row units (R > 1)
SEGMENTS = [(5, 2, 8, 40, 66), (3, 2, 8, 33, 65)]     # single-row units, nseg > 1, units of one and of two 16-tile steps
SHAPES = RAGGED + CHUNKS + SINGLE_RAW + ROWS + SEGMENTS
HALF_CASES = [(s, h, m) for s in SHAPES for h in (0, 1) for m in MODES]
# weight-gradient variants: tuning key 29 (0 whole-row units, 1 single-row units, 2 at most 16 tiles) x key 12 (0: the
# launcher's splits -- one unit per split at these sizes; 3: three splits, so that one workgroup walks several units and
# crosses samples: the has_next half of the unit pipeline)
WGRAD_VARIANTS = [(k29, k12) for k29 in (0, 1, 2) for k12 in (0, 3)]
# the whole layer (two jobs in one launch; tuning key 21 = 2: one launch per job)
LAYER_SHAPES = [(5, 3, 24, 11, 9), (3, 2, 40, 9, 14)]
LAYER_CASES = [(s, m) for s in LAYER_SHAPES for m in MODES]
LAYER_KEY21 = (0, 2)
LAYER_PINNED = ("logits", "grad_target")
LAYER_UNSTABLE = ("grad_source", "grad_flow", "grad_w0")   # never pinned (module docstring)


def shape_id(shape):
    return "k%d_%s" % (shape[0], "x".join(map(str, shape[1:])))


def case_id(v):
    return shape_id(v) if isinstance(v, tuple) else str(v)


def digest(t):
    """SHA-256 of the raw bytes of t + 0 (a signed zero cannot matter)"""
    return hashlib.sha256((t + 0).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


_INPUTS = {}


def inputs(shape):
    """Seeded float32 host tensors of a shape, made once: x of either half, w0, w1, flow, grad_logits, {half: dG}"""
    if shape not in _INPUTS:
        k, B, C, H, W = shape
        seed = 100 * sum(shape)
        dG = {}
        for h in (0, 1):
            g = fc_mfma.geometry(H, W, k, h)
            dG[h] = randn((B, 128, g["Ho"], g["Wo"]), seed=seed + 5 + h) * 1e-3
        _INPUTS[shape] = {"x": {h: randn((B, C, H, W), seed=seed + h) * 1.7 for h in (0, 1)},
                          "w0": randn((128, 2 * C, k, k), seed=seed + 2) * 0.05, "w1": randn((k * k, 128), seed=seed + 3) * 0.1,
                          "flow": randn((B, 2, H, W), seed=seed + 4) * 1.5, "gl": randn((B, k * k, H, W), seed=seed + 7) * 1e-2,
                          "dG": dG}
    return _INPUTS[shape]


def _full(shape):
    return torch.full(shape, SENTINEL, device=DEV)


def run_half(shape, is_source, mode):
    """forward map, grad_x, grad_w0 of one half: whole buffers"""
    k, B, C, H, W = shape
    inp = inputs(shape)
    x, w0, dG = inp["x"][is_source].to(DEV), inp["w0"].to(DEV), inp["dG"][is_source].to(DEV)
    g = fc_mfma.geometry(H, W, k, is_source)
    ws = torch.zeros(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 0), dtype=torch.uint8, device=DEV)
    out = _full((B, g["Mg"], 128))
    _lib.call("gfla_fc_conv_fwd_f32", x, _lib.ptr(x), _lib.ptr(w0), is_source, _lib.ptr(ws), _lib.ptr(out), B, C, H, W, k, mode)
    rows = (torch.arange(g["Ho"])[:, None] * g["Wp"] + torch.arange(g["Wo"])[None, :]).reshape(-1).to(DEV)
    z = torch.zeros(B, g["Sz"], 128, device=DEV)
    z[:, g["lead"] + rows, :] = dG.permute(0, 2, 3, 1).reshape(B, -1, 128)
    sc = torch.zeros(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 1), dtype=torch.uint8, device=DEV)
    gx, gw = _full((B, C, H, W)), _full((128, 2 * C, k, k))
    _lib.call("gfla_fc_conv_bwd_f32", x, _lib.ptr(z), is_source, _lib.ptr(ws), _lib.ptr(sc), _lib.ptr(gx), _lib.ptr(gw), B, C, H, W,
              k, mode)
    torch.cuda.synchronize()
    return out, gx, gw


def runs_in(shape, mode):
    k, B, C, H, W = shape
    return fc_mfma.resolve_mode(C, H, W, k, mode) == mode


def half_digests(shape, is_source, mode):
    """{} where the shape falls back from `mode` (resolve_mode)"""
    if not runs_in(shape, mode):
        return {}
    key = "half/%s/half%d/mode%d" % (shape_id(shape), is_source, mode)
    got = {}
    out, gx, gw = run_half(shape, is_source, mode)
    got[key + "/out"], got[key + "/grad_x"] = digest(out), digest(gx)
    if shape in RAGGED:   # the single-raw-buffer staging forced on
        with _lib.tuned({_lib.TUNE_WINO_LAUNCH: 1}):
            out, gx, _ = run_half(shape, is_source, mode)
        got[key + "/key21_1/out"], got[key + "/key21_1/grad_x"] = digest(out), digest(gx)
    for k29, k12 in WGRAD_VARIANTS:
        if (k29, k12) != (0, 0):
            with _lib.tuned({_lib.TUNE_WINO_WGRAD_UNITS: k29, _lib.TUNE_FC_WGRAD_SPLITS: k12}):
                _, _, gw = run_half(shape, is_source, mode)
        got[key + "/key29_%d/key12_%d/grad_w0" % (k29, k12)] = digest(gw)
    return got


def run_layer(shape, mode):
    k, B, C, H, W = shape
    inp = inputs(shape)
    s, t, f = inp["x"][1].to(DEV), inp["x"][0].to(DEV), inp["flow"].to(DEV)
    w0, w1, gl = inp["w0"].to(DEV), inp["w1"].to(DEV), inp["gl"].to(DEV)
    p = _lib.ptr
    ws = torch.zeros(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 0), dtype=torch.uint8, device=DEV)
    sc = torch.zeros(fc_mfma.workspace_bytes(B, C, H, W, k, mode, 1), dtype=torch.uint8, device=DEV)
    logits = _full((B, k * k, H, W))
    gs, gt, gf, gw0 = torch.zeros_like(s), _full(t.shape), torch.zeros_like(f), _full(w0.shape)
    _lib.call("gfla_fc_forward_f32", s, p(s), p(t), p(f), p(w0), None, p(w1), None, p(ws), p(logits), B, C, H, W, k, 0.1, mode)
    _lib.call("gfla_fc_backward_f32", s, p(ws), p(f), p(w1), p(gl), p(sc), p(gs), p(gt), p(gf), p(gw0), None, None, None,
              B, C, H, W, k, 0.1, mode, 0)
    torch.cuda.synchronize()
    return {"logits": logits, "grad_source": gs, "grad_target": gt, "grad_flow": gf, "grad_w0": gw0}


def layer_digests(shape, mode):
    if not runs_in(shape, mode):
        return {}
    got = {}
    for k21 in LAYER_KEY21:
        with _lib.tuned({_lib.TUNE_WINO_LAUNCH: k21}):
            for name, t in run_layer(shape, mode).items():
                got["layer/%s/mode%d/key21_%d/%s" % (shape_id(shape), mode, k21, name)] = digest(t)
    return got


def all_digests():
    got = {}
    for shape, h, mode in HALF_CASES:
        got.update(half_digests(shape, h, mode))
    for shape, mode in LAYER_CASES:
        got.update(layer_digests(shape, mode))
    return got
