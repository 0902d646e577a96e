"""Shared by the planes-in-LDS geometry tests (test_plane_geometry_cpu.py / test_plane_geometry_gpu.py): float64 evaluations
of block_extractor, the softmax + aggregate composition and resample2d, forward and every gradient, written as plain gathers
and scatters in torch; the per-element error bar; the d/d flow entries that sit on a kink; and the inputs of the GPU cases,
so the CPU tests can state conditions on exactly those inputs.

Every evaluation starts from the stored values (16-bit inputs are widened exactly) and returns, next to each result, A: the
same sum with every term replaced by its magnitude and every bilinear weight by 1 (|upstream| x |corner value|), and the
number n of products the kernels sum into one element.

The bar, per element (after gen_conv_util.bar):

    |got - ref| <= e + u (|ref| + e) + t,     e = 2 (n + 2 P) eps A

  eps  2^-24 (the kernels' arithmetic is float32 for float32 and 16-bit storage), 2^-53 for float64 storage.
  n    products summed into the element in the arithmetic type, per operator (see each function).  A sum of n products
       carries at most (n - 1 + m) eps of sum |terms| with m roundings inside a product (two or three weights, 1 - a); the
       factor 2 and the 2 P >= 2 below leave room for m.
  P    largest |sampling coordinate| + 1 of the case.  The kernels form (flow + tap) + index in the arithmetic type: two
       roundings, each at most eps |coordinate|, move the fraction a = x - floor(x) and with it a weight by 2 eps P; what a
       weight multiplies is bounded by the corner magnitudes in A.
  u    the ONE rounding of the stored result: 0 for float32 / float64, 2^-11 float16, 2^-8 bfloat16.  It applies to what
       the kernel rounds, ref + (its float32 error), hence u (|ref| + e).
  t    half the smallest subnormal of the storage type (2^-25 for float16): the absolute rounding error below the normal
       range.  0 for the other types at the magnitudes of these tests.

resample2d: the weights are Gaussian, exp(-d^2 / (2 sigma^2)) / sum, evaluated in double by the kernels and rounded once.  A
keeps them (they are positive and sum to 1); a coordinate error delta moves a weight w by at most w d / sigma^2 delta and a
weight derivative w d / sigma^2 by at most w (d^2 / sigma^4 + 1 / sigma^2) delta.  With d <= (k / 2) dilation =: D the factor
KAPPA = max(1, D / sigma^2) bounds the first and (KAPPA^2 + 1 / sigma^2) <= 2 KAPPA^2 the second (sigma >= 1), so resample2d
uses P KAPPA^2 for P, and its d/d flow replaces each |dw / dx| by KAPPA w in A.  sigma is per pixel (input2 = dx, dy, sigma):
given as a (B,1,H,W) field, KAPPA(b, y, x) = max(1, D / sigma^2) and with it P are fields too, and the gradient of the
feature map, whose elements collect pixels of any sigma, takes the largest P of the case.

resample2d, d/d sigma.  dw / dsigma = w d^2 / sigma^3 on each axis, so with c = (yd^2 + xd^2) / sigma^3 per tap (yd, xd its
two distances), Vs = sum w c v and Ds = sum w c,

    g_sigma = sum_c up (Vs / S - val Ds / S^2).

Every distance is at most D, so 0 <= c <= 2 D^2 / sigma^3 =: c_max, |Vs| <= c_max sum w |v| and |val Ds / S^2| <= c_max
sum w |v| / S: A = 2 c_max sum_c |up| (sum w |v|) / S, the quotient rule's two sums as for d/d flow, and the same
n = 2 C k^2 + 2 k^2.  A coordinate error delta moves a term w c by |dw / dx| c + w |dc / dx| <= (KAPPA + 2 d / (sigma^3
c_max)) w c_max delta = (KAPPA + d / D^2) w c_max delta <= 2 KAPPA w c_max delta (d <= D, D >= 1, KAPPA >= 1), which is
below the 2 KAPPA^2 that d/d flow's P KAPPA^2 already pays for: P as for d/d flow.  sigma itself is an input, read exactly;
sigma^3, its reciprocal and the squared distances are roundings inside a product (m).  All of this needs sigma >= 1
(1 / sigma^2 <= KAPPA^2 above); `sigma_field` produces and asserts [1, 3.5].  d/d sigma is continuous in the flow wherever the
forward is: it has no kinks of its own and is compared at every pixel.

d/d flow has a jump wherever a sampling coordinate is an integer inside the range where the clamped taps still differ.
`flow_kinks` marks those entries (within CLEAR px, or where the float32 and float64 floors differ); they are left out of the d/d
flow comparison only.  Forward results and feature-map gradients are compared everywhere."""
import torch
import torch.nn.functional as F

from global_flow_local_attention_amd import TUNE_BIG_PLANE, TUNE_LDS_KB, TUNE_RS, TUNE_RS_BWD1_PLANES
from util import make_flow, rand, randn

CLEAR = 1e-3
EPS = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -24, torch.float64: 2.0 ** -53}
UNIT = {torch.float32: 0.0, torch.float64: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float32: 0.0, torch.float64: 0.0, torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}
SIGMA = 2.0


def bar(A, ref, n, P, dtype):
    """The per-element bound of the module docstring; n a number or a tensor that broadcasts against A."""
    e = 2.0 * (n + 2.0 * P) * EPS[dtype] * A
    return e + UNIT[dtype] * (ref.abs() + e) + TINY[dtype]


def worst(got, ref, A, n, P, dtype, keep=None, extra=None, b=None):
    """(max err / bar over the kept entries, number of entries beyond the bar); got in any dtype, anywhere.  `extra`: an
    absolute term on top of the bar (rs_fixed_point_term).  `b`: bar(A, ref, n, P, dtype) where the caller keeps it with
    its reference."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if b is None:
        b = bar(A, ref, n, P, dtype)
    if extra is not None:
        b = b + extra
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))      # finite where the reference is
    ratio = err / b.clamp_min(1e-300)
    ratio = torch.where((err == 0) & (b == 0), torch.zeros_like(ratio), ratio)
    if keep is not None:
        ratio = torch.where(keep.expand_as(ratio), ratio, torch.zeros_like(ratio))
    return ratio.max().item(), int((ratio > 1).sum().item())


# ------------------------------------------------------------------------------------------------------ block_extractor
def _be_setup(f, k, Hs, Ws, xmax_shift=0):
    """coordinates of every output position (B, kHf, kWf): block_extractor_kernel.cu:62-67, dx = (flow + offset) + index"""
    B, _, Hf, Wf = f.shape
    y, x = torch.arange(k * Hf), torch.arange(k * Wf)
    yf, xf = y // k, x // k
    oy, ox = (y % k - k // 2).double(), (x % k - k // 2).double()
    dx = (f[:, 0][:, yf][:, :, xf] + ox.view(1, 1, -1)) + xf.double().view(1, 1, -1)
    dy = (f[:, 1][:, yf][:, :, xf] + oy.view(1, -1, 1)) + yf.double().view(1, -1, 1)
    x0, y0 = dx.floor(), dy.floor()
    ax, ay = (dx - x0).unsqueeze(1), (dy - y0).unsqueeze(1)
    xhi = Ws - 1 - xmax_shift            # xmax_shift != 0: the planted bug of the power test (a clamp moved by one)
    xL, xR = x0.long().clamp(0, xhi), (x0.long() + 1).clamp(0, xhi)
    yT, yB = y0.long().clamp(0, Hs - 1), (y0.long() + 1).clamp(0, Hs - 1)
    idx = [yT * Ws + xL, yT * Ws + xR, yB * Ws + xL, yB * Ws + xR]
    w = [(1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay]
    return idx, w, ax, ay


def block_extractor(s, f, up, k, xmax_shift=0):
    """block_extractor in float64.  s (B,C,Hs,Ws), f (B,2,Hf,Wf), up (B,C,kHf,kWf) or None.  Returns a dict of
    name -> (ref, A, n): out (n = 4: four corners), g_source (n = the number of (position, corner) pairs that land on the
    element, a tensor), g_flow (n = 4 C k^2: four corners of k^2 taps of C channels); and out_term, the largest single
    |weight x value| of each output element."""
    s, f = s.double(), f.double()
    B, C, Hs, Ws = s.shape
    Hf, Wf = f.shape[2:]
    idx, w, ax, ay = _be_setup(f, k, Hs, Ws, xmax_shift)
    flat = s.reshape(B, C, Hs * Ws)
    n_out = k * Hf * k * Wf

    def tap(i):
        return flat.gather(2, i.view(B, 1, n_out).expand(B, C, n_out)).view(B, C, k * Hf, k * Wf)

    v = [tap(i) for i in idx]
    out = sum(wi * vi for wi, vi in zip(w, v))
    A_out = sum(vi.abs() for vi in v)
    res = {"out": (out, A_out, 4), "out_term": torch.stack([(wi * vi).abs() for wi, vi in zip(w, v)]).max(0)[0]}
    if up is None:
        return res
    up = up.double()
    gs, A_gs, cnt = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros(B, 1, Hs * Ws, dtype=torch.float64)
    for wi, i in zip(w, idx):
        at = i.view(B, 1, n_out)
        gs.scatter_add_(2, at.expand(B, C, n_out), (wi * up).reshape(B, C, n_out))
        A_gs.scatter_add_(2, at.expand(B, C, n_out), up.abs().reshape(B, C, n_out))
        cnt.scatter_add_(2, at, torch.ones(B, 1, n_out, dtype=torch.float64))
    res["g_source"] = (gs.view(B, C, Hs, Ws), A_gs.view(B, C, Hs, Ws), cnt.view(B, 1, Hs, Ws))
    vTL, vTR, vBL, vBR = v
    d_x = (1 - ay) * (vTR - vTL) + ay * (vBR - vBL)
    d_y = (1 - ax) * (vBL - vTL) + ax * (vBR - vTR)

    def pixel(t):     # sum over the channels and the k x k taps of a flow pixel
        return t.sum(1).view(B, Hf, k, Wf, k).sum((2, 4))

    gf = torch.stack([pixel(up * d_x), pixel(up * d_y)], 1)
    A_gf = pixel(up.abs() * A_out).unsqueeze(1).expand(B, 2, Hf, Wf).contiguous()
    res["g_flow"] = (gf, A_gf, 4 * C * k * k)
    return res


def be_coordinates(f, k, dtype=torch.float64):
    """(B, 2, k, Hf, Wf): the k sampling coordinates per axis of every flow entry, (flow + offset) + index evaluated in dtype"""
    f = f.to(dtype)
    B, _, Hf, Wf = f.shape
    xs, ys = torch.arange(Wf).to(dtype).view(1, 1, Wf), torch.arange(Hf).to(dtype).view(1, Hf, 1)
    cx = torch.stack([(f[:, 0] + float(t - k // 2)) + xs for t in range(k)], 1)
    cy = torch.stack([(f[:, 1] + float(t - k // 2)) + ys for t in range(k)], 1)
    return torch.stack([cx, cy], 1)


def _kinks(c64, c_arith, lo, hi):
    """any over the taps (dim 2) of: coordinate within CLEAR of an integer in [lo, hi] (both (2,)-shaped per axis), or the
    floors of the two evaluations differ"""
    lo, hi = lo.view(1, 2, 1, 1, 1), hi.view(1, 2, 1, 1, 1)
    near = ((c64 - c64.round()).abs() < CLEAR) & (c64.round() >= lo) & (c64.round() <= hi)
    return (near | (c_arith.floor().double() != c64.floor())).any(2)


def be_flow_kinks(f, k, Hs, Ws, arith):
    """(B,2,Hf,Wf) bool: d/d flow of block_extractor is one-sided here.  The clamped taps xL, xR differ only for a coordinate
    in (0, Ws - 1): integers 0 .. Ws - 1 are the kinks (beyond, both corners are the border pixel and the slope is 0 on
    either side)."""
    hi = torch.tensor([Ws - 1.0, Hs - 1.0], dtype=torch.float64)
    return _kinks(be_coordinates(f, k), be_coordinates(f, k, arith), torch.zeros(2, dtype=torch.float64), hi)


# ---------------------------------------------------------------------------------------------- softmax + aggregate
def aggregate_forward(s, f, lg, k):
    """out = avg_pool(pixel_shuffle(softmax(logits)) * block_extractor(s, f), k) in float64.  name -> (ref, A, n):
    attn (A = attn; n = k^2 + 8 + 2 L: the k^2 terms of the normaliser, the exponential and the division, and the rounding
    of logit - max, at most eps L relative in the exponential with L = max |logit - max logit|);
    out (A = mean over the taps of attn x sum |corner|; n = 4 k^2 products + n of attn)."""
    s, f, lg = s.double(), f.double(), lg.double()
    be = block_extractor(s, f, None, k)
    bs, A_bs, _ = be["out"]
    attn = F.softmax(lg, 1)
    L = (lg - lg.max(1, keepdim=True)[0]).abs().max().item()
    n_attn = k * k + 8 + 2 * L
    full = F.pixel_shuffle(attn, k)
    out = F.avg_pool2d(full * bs, k, k)
    A_out = F.avg_pool2d(full * A_bs, k, k)
    return {"attn": (attn, attn, n_attn), "out": (out, A_out, 4 * k * k + n_attn),
            "out_term": F.max_pool2d(full * be["out_term"], k, k) / (k * k)}


def aggregate_backward(s, f, attn, up, k, xmax_shift=0):
    """The gradients of that composition for upstream `up` (B,C,H,W), evaluated with the attention map the forward STORED
    (`attn`, widened exactly: the backward kernels read it, so its rounding to the storage type is an input here, not an
    error).  g_source (n = contributions per element), g_flow (n = 4 C k^2), g_logits (the softmax Jacobian of d/d attn;
    n = 4 C products per tap + the k^2 terms of the Jacobian's inner product)."""
    s, f, attn, up = s.double(), f.double(), attn.double(), up.double()
    B, C = s.shape[:2]
    up_rep = up.repeat_interleave(k, 2).repeat_interleave(k, 3)
    full = F.pixel_shuffle(attn, k)
    be = block_extractor(s, f, full * up_rep / (k * k), k, xmax_shift)
    bs, A_bs, _ = be["out"]
    g_attn = F.pixel_unshuffle((bs * up_rep).sum(1, keepdim=True), k) / (k * k)
    A_ga = F.pixel_unshuffle((A_bs * up_rep.abs()).sum(1, keepdim=True), k) / (k * k)
    gl = attn * (g_attn - (attn * g_attn).sum(1, keepdim=True))
    A_gl = attn * (A_ga + (attn * A_ga).sum(1, keepdim=True))
    return {"g_source": be["g_source"], "g_flow": be["g_flow"], "g_logits": (gl, A_gl, 4 * C + k * k)}


# ------------------------------------------------------------------------------------------------------------ resample2d
def rs_kappa(k, dil, sigma=SIGMA):
    """KAPPA of the module docstring: a number for a number, a float64 field for a (B,1,H,W) field of stored sigmas"""
    if torch.is_tensor(sigma):
        sigma = sigma.double()
        return ((k // 2) * dil / (sigma * sigma)).clamp_min(1.0)
    return max(1.0, (k // 2) * dil / (sigma * sigma))


def _rs_axis(c, n_src, KH, dil, sigma, frac, hi_shift=0):
    """The 2 KH taps of one axis: [(clamped index, weight, d weight / d coordinate, distance)].  `frac` = the fraction the
    weights use (coordinate - floor, or coordinate - trunc for the reference's d/d input1); indices always come from the
    floor.  sigma: a number, or a float64 tensor shaped like c."""
    c0 = c.floor().long()
    taps = []
    for t in range(KH):
        near, far = t * dil + frac, (1 + t) * dil - frac
        w_n, w_f = torch.exp(-near * near / (2 * sigma * sigma)), torch.exp(-far * far / (2 * sigma * sigma))
        taps.append(((c0 - t * dil).clamp(0, n_src - 1 - hi_shift), w_n, -near / (sigma * sigma) * w_n, near))
        taps.append(((c0 + (t + 1) * dil).clamp(0, n_src - 1 - hi_shift), w_f, far / (sigma * sigma) * w_f, far))
    return taps


def resample2d(i1, f, up, k, dil, sigma=SIGMA, xmax_shift=0, sigma_power=3):
    """Resample2d(k, dil, sigma) in float64 (resample2d_kernel.cu:20-95, :98-202 with its int() quirk as
    oracle.resample2d_bwd(trunc_compat=True) has it, :204-330 for dx, dy, sigma).  i1 (B,C,Hi,Wi), f (B,2,H,W), up (B,C,H,W)
    or None; sigma a number, or a (B,1,H,W) tensor of stored values (widened exactly): one sigma per pixel, the third channel
    of input2.  With a number every entry but g_sigma is what it was before sigma could be a field, bit for bit.
    name -> (ref, A, n): out (n = 2 k^2: k^2 products and the k^2 terms of the normaliser); g_input1 (n = contributions per
    element + k^2 for the normaliser every contribution shares); g_flow (n = 2 C k^2 + 2 k^2: the two sums of the quotient
    rule over C channels and k^2 taps, and the normaliser twice; A = 2 KAPPA sum |up| sum w |v| / S); g_sigma ((B,1,H,W), no
    reference quirk, fractions from the floor; the same n; A = 2 (2 D^2 / sigma^3) sum |up| sum w |v| / S, module docstring).
    xmax_shift, sigma_power: the planted bugs of the power tests (a clamp moved by one; 1 / sigma^2 for 1 / sigma^3 in c)."""
    i1, f = i1.double(), f.double()
    B, C, Hi, Wi = i1.shape
    H, W = f.shape[2:]
    KH = k // 2
    field = sigma
    if torch.is_tensor(sigma):
        assert tuple(sigma.shape) == (B, 1, H, W), (tuple(sigma.shape), (B, 1, H, W))
        field = sigma.double()
        sigma = field[:, 0]
    xf = torch.arange(W, dtype=torch.float64).view(1, 1, W) + f[:, 0]
    yf = torch.arange(H, dtype=torch.float64).view(1, H, 1) + f[:, 1]
    cols = _rs_axis(xf, Wi, KH, dil, sigma, xf - xf.floor(), xmax_shift)
    rows = _rs_axis(yf, Hi, KH, dil, sigma, yf - yf.floor())
    flat = i1.reshape(B, C, Hi * Wi)

    def tap(r_off, q):
        return flat.gather(2, (r_off + q).view(B, 1, H * W).expand(B, C, H * W)).view(B, C, H, W)

    S = (sum(w for _, w, _, _ in rows) * sum(w for _, w, _, _ in cols)).unsqueeze(1)
    Dx = (sum(w for _, w, _, _ in rows) * sum(d for _, _, d, _ in cols)).unsqueeze(1)
    Dy = (sum(d for _, _, d, _ in rows) * sum(w for _, w, _, _ in cols)).unsqueeze(1)
    val, mag, vx, vy, vs, term = 0, 0, 0, 0, 0, torch.zeros(B, C, H, W, dtype=torch.float64)
    yd2, xd2 = [d * d for _, _, _, d in rows], [d * d for _, _, _, d in cols]
    for (r, wy, dwy, _), y2 in zip(rows, yd2):
        r_off = r * Wi
        for (q, wx, dwx, _), x2 in zip(cols, xd2):
            v = tap(r_off, q)
            w = (wy * wx).unsqueeze(1)
            wv = w * v
            wv_abs = wv.abs()              # = w |v| to the bit: w >= 0
            val = val + wv
            mag = mag + wv_abs
            vx = vx + (wy * dwx).unsqueeze(1) * v
            vy = vy + (dwy * wx).unsqueeze(1) * v
            vs = vs + (y2 + x2).unsqueeze(1) * wv            # c without its 1 / sigma^3, a factor of the pixel
            term = torch.maximum(term, wv_abs)
    res = {"out": (val / S, mag / S, 2 * k * k), "out_term": term / S}
    if up is None:
        return res
    up = up.double()
    up_abs = up.abs()
    gf = torch.stack([(up * (vx / S - val * Dx / (S * S))).sum(1), (up * (vy / S - val * Dy / (S * S))).sum(1)], 1)
    A_gf = (2 * rs_kappa(k, dil, field) * (up_abs * mag / S).sum(1, keepdim=True)).expand(B, 2, H, W).contiguous()
    res["g_flow"] = (gf, A_gf, 2 * C * k * k + 2 * k * k)
    # d/d sigma: Vs / S - val Ds / S^2 with c = (yd^2 + xd^2) / sigma^3 (:273-328)
    sg = (sigma if torch.is_tensor(sigma) else torch.full((B, H, W), float(sigma), dtype=torch.float64)).unsqueeze(1)
    s3 = sg ** sigma_power
    Ds = (sum(w * d * d for _, w, _, d in rows) * sum(w for _, w, _, _ in cols) +
          sum(w for _, w, _, _ in rows) * sum(w * d * d for _, w, _, d in cols)).unsqueeze(1) / s3
    gsig = (up * (vs / s3 / S - val * Ds / (S * S))).sum(1, keepdim=True)
    D = float(KH * dil)
    A_gs = 2 * (2 * D * D / sg ** 3) * (up_abs * mag / S).sum(1, keepdim=True)
    res["g_sigma"] = (gsig, A_gs, 2 * C * k * k + 2 * k * k)
    # d/d input1: weights from coordinate - int(coordinate) (:137-138), indices from the floor
    cols1 = _rs_axis(xf, Wi, KH, dil, sigma, xf - xf.trunc(), xmax_shift)
    rows1 = _rs_axis(yf, Hi, KH, dil, sigma, yf - yf.trunc())
    S1 = (sum(w for _, w, _, _ in rows1) * sum(w for _, w, _, _ in cols1)).unsqueeze(1)
    g1, A_g1, cnt = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros(B, 1, Hi * Wi, dtype=torch.float64)
    one = torch.ones(B, 1, H * W, dtype=torch.float64)
    for r, wy, _, _ in rows1:
        r_off = r * Wi
        for q, wx, _, _ in cols1:
            at = (r_off + q).view(B, 1, H * W)
            at_c = at.expand(B, C, H * W)
            wn = (wy * wx).unsqueeze(1) / S1
            g1.scatter_add_(2, at_c, (wn * up).reshape(B, C, H * W))
            A_g1.scatter_add_(2, at_c, (wn * up_abs).reshape(B, C, H * W))
            cnt.scatter_add_(2, at, one)
    res["g_input1"] = (g1.view(B, C, Hi, Wi), A_g1.view(B, C, Hi, Wi), cnt.view(B, 1, Hi, Wi) + k * k)
    res["g_input1_count"] = cnt.view(B, 1, Hi, Wi)
    return res


def rs_coordinates(f, dtype=torch.float64):
    """(B, 2, 1, H, W): index + flow evaluated in dtype (resample2d_kernel.cu:47-55)"""
    f = f.to(dtype)
    H, W = f.shape[2:]
    return torch.stack([torch.arange(W).to(dtype).view(1, 1, W) + f[:, 0], torch.arange(H).to(dtype).view(1, H, 1) + f[:, 1]], 1).unsqueeze(2)


def rs_flow_kinks(f, k, dil, Hi, Wi, arith):
    """(B,2,H,W) bool.  The taps floor - t d .. floor + (t + 1) d, clamped, all name the same border pixel once the floor is
    below -(k/2) d or at least n - 1 + (k/2 - 1) d: integers outside that range are no kinks."""
    KH = k // 2
    lo = torch.full((2,), -float(KH * dil), dtype=torch.float64)
    hi = torch.tensor([Wi - 1.0, Hi - 1.0], dtype=torch.float64) + (KH - 1) * dil
    return _kinks(rs_coordinates(f), rs_coordinates(f, arith), lo, hi)


def rs_fixed_point_term(cnt, up, dtype):
    """float32 arithmetic scatters d/d input1 into 64-bit fixed-point planes whose scale puts the largest |upstream| of a
    workgroup at 2^40 (csrc/lds_plane.h: fix_scale): every contribution is rounded to 2^-41 of a power of two below
    2 max |up|, an absolute error of at most 2^-40 max |up| each, whatever its own size."""
    if dtype == torch.float64:
        return torch.zeros_like(cnt)
    return cnt * 2.0 ** -40 * up.double().abs().max().item()


# The other routes of d/d input1 have no term of their own.  The matrix-core product (csrc/patch_mfma.hip, tuning key 14 = 2)
# float32-sums products: rs_patch_table_kernel pre-sums, in float32, the weights wy[r] / S * wx[s] of the taps that clamp onto
# one border position, and v_mfma_f32_32x32x2_f32 multiplies and accumulates in float32 without intermediate rounding to a
# narrower type -- the same n products in another association, which the (n - 1 + m) eps sum |terms| of the bar does not
# depend on.  Double planes (key 23 = 1) and the global kernels (key 6 = 1) add the float32 products with float64 / float32
# atomics: at most the float32 sum the bar allows.  Since the product decides on the device whether the fixed-point scatter
# behind it runs instead, the float32 cases keep rs_fixed_point_term under every key set but 23 = 1 and 6 = 1.
def rs_input1_term(cnt, up, dtype, keys):
    # (16-bit storage ignores both keys)
    if dtype == torch.float32 and (keys.get(TUNE_RS_BWD1_PLANES) == 1 or keys.get(TUNE_RS) == 1):
        return torch.zeros_like(cnt)
    return rs_fixed_point_term(cnt, up, dtype)


# ------------------------------------------------------------------------------------------------ the GPU cases' inputs
SHAPES = [(2, 7, 14, 10, 14, 10),      # prime C: every G > 1 leaves a ragged last group
          (3, 5, 9, 13, 6, 7),         # source and flow sizes differ, odd everywhere
          (1, 8, 48, 32, 48, 32),      # whole planes at 64 KB, row windows at key 10 = 16
          (2, 6, 57, 37, 57, 37)]      # 2109 pixels: split = 2 by default, `per` ends inside a flow row
WINDOW_FWD_SHAPE = (1, 3, 71, 59, 71, 59)    # 4189 float32 elements > 16 KB: the forward kernels' row windows at key 10 = 16
KINDS = ("coherent", "wild", "smooth")
KINDS16 = KINDS + ("oob",)
ARITH = {torch.float32: torch.float32, torch.float16: torch.float32, torch.bfloat16: torch.float32, torch.float64: torch.float64}


def planted(B, Hf, Wf):
    """(B,2,Hf,Wf) bool: the lattice and near-lattice points planted into the `smooth` flow"""
    m = torch.zeros(B, 2, Hf, Wf, dtype=torch.bool)
    m[:, :, ::3, ::2] = True
    m[:, :, 1::4, 1::3] = True
    return m


def flow_of(kind, B, Hf, Wf, dtype, seed):
    """The flow of a case, rounded to its storage type.  smooth: lattice points at [::3, ::2] and, for float32 / float64,
    points 2^-22 / 2^-50 above a lattice point at [1::4, 1::3] (the tap-by-tap branch of the kernels; 16-bit types cannot
    represent such an offset: there these are lattice points too).  oob: every tap beyond the map, on all four sides."""
    if kind == "oob":
        f = make_flow("coherent", B, Hf, Wf, seed=seed)
        f[:, 0] += 1000.0
        f[:, 1] -= 1000.0
        f[::2, 0] -= 2000.0
        f[::2, 1] += 2000.0
        return f.to(dtype)
    f = make_flow(kind, B, Hf, Wf, torch.float64, seed=seed)
    if kind == "smooth":
        f[:, :, ::3, ::2] = torch.round(f[:, :, ::3, ::2])
        off = {torch.float32: 2.0 ** -22, torch.float64: 2.0 ** -50}.get(dtype, 0.0)
        f[:, :, 1::4, 1::3] = torch.round(f[:, :, 1::4, 1::3]) + off
    return f.to(dtype).contiguous()


def inputs(op, shape, dtype, kind, k):
    """The stored inputs of one GPU case, on the host: op 'be' / 'unfold' -> (source, flow, upstream), 'agg' -> (source,
    flow, logits, upstream), 'rs' -> (input1, flow, upstream)."""
    B, C, Hs, Ws, Hf, Wf = shape
    seed = 7000 + 100 * (SHAPES.index(shape) if shape in SHAPES else len(SHAPES)) + 10 * KINDS16.index(kind) + k
    s = randn((B, C, Hs, Ws), seed=seed).to(dtype)
    f = flow_of(kind, B, Hf, Wf, dtype, seed + 1)
    if op == "be":
        return s, f, randn((B, C, k * Hf, k * Wf), seed=seed + 2).to(dtype)
    if op == "unfold":
        return s, f, randn((B, C * k * k, Hf, Wf), seed=seed + 2).to(dtype)
    if op == "agg":
        return s, f, (randn((B, k * k, Hf, Wf), seed=seed + 3) * 2).to(dtype), randn((B, C, Hf, Wf), seed=seed + 2).to(dtype)
    return s, f, randn((B, C, Hf, Wf), seed=seed + 2).to(dtype)


SIGMA_FIELDS = ("random", "levels")
SIGMA_MIN, SIGMA_MAX = 1.0, 3.5


def sigma_field(kind, B, H, W, dtype, seed):
    """(B,1,H,W) sigma per pixel, rounded to the storage type, every value in [1, 3.5] (the module docstring's bar for
    resample2d assumes sigma >= 1).  random: 1 + 2.5 rand.  levels: 1 + 0.5 ((x + 2 y + 3 b) % 6) -- six values, exact in
    float16 and bfloat16, and different from the left, the upper and the previous sample's neighbour of every pixel: a
    kernel that reads sigma one pixel, one row or one sample off sees another value everywhere."""
    if kind == "random":
        s = 1.0 + 2.5 * rand((B, 1, H, W), torch.float64, seed=seed)
    elif kind == "levels":
        b, y, x = torch.arange(B).view(B, 1, 1, 1), torch.arange(H).view(1, 1, H, 1), torch.arange(W).view(1, 1, 1, W)
        s = 1.0 + 0.5 * ((x + 2 * y + 3 * b) % 6).double()
    else:
        raise ValueError(kind)
    s = s.to(dtype).contiguous()
    assert s.double().min().item() >= SIGMA_MIN and s.double().max().item() <= SIGMA_MAX, (kind, dtype)
    return s


def rs_sigma(shape, dtype, kind, k, field):
    """the sigma field of one sigma-field case of resample2d (seeded by the case, like its `inputs`)"""
    B, C, Hs, Ws, Hf, Wf = shape
    seed = 9000 + 100 * (SHAPES.index(shape) if shape in SHAPES else len(SHAPES)) + 10 * KINDS16.index(kind) + k
    return sigma_field(field, B, Hf, Wf, dtype, seed)


def rs_sigma_inputs(shape, dtype, kind, k, field):
    """The stored inputs of one sigma-field case of resample2d: (input1, flow, upstream) of `inputs` and the sigma field"""
    return inputs("rs", shape, dtype, kind, k) + (rs_sigma(shape, dtype, kind, k, field),)


def coordinate_bound(f, span):
    """P: the largest |sampling coordinate| + 1 -- |flow| + the largest index + the tap span"""
    return f.double().abs().max().item() + max(f.shape[2], f.shape[3]) + span + 1.0


def unfold_from_patches(t, k):
    """(B,C,kH,kW) -> (B, C k^2, H, W) with channel c k^2 + i k + j = tap (i, j) of channel c"""
    B, C, Hk, Wk = t.shape
    return t.view(B, C, Hk // k, k, Wk // k, k).permute(0, 1, 3, 5, 2, 4).reshape(B, C * k * k, Hk // k, Wk // k)


def patches_from_unfold(t, k):
    B, Ck, H, W = t.shape
    C = Ck // (k * k)
    return t.view(B, C, k, k, H, W).permute(0, 1, 4, 2, 5, 3).reshape(B, C, k * H, k * W)


# ------------------------------------------------------------------------------------------------- tuning keys, the query
# key 10 = 16 (KB of LDS) alone hands few large planes to the tile kernels of csrc/tile_map.h; key 30 = 1 keeps them out, so
# planes beyond 16 KB run as row windows of this family
WINDOWS = {TUNE_LDS_KB: 16, TUNE_BIG_PLANE: 1}
QUERY_OPS = {"be_bwd": 0, "agg_bwd": 1, "unfold_bwd": 2, "unfold_attn_bwd": 3, "unfold_fwd": 4, "rs_fwd": 5, "rs_bwd1": 6, "rs_bwd2": 7}


def query(_lib, op, shape, k, dil=1, elem=4, needs=3):
    """gfla_lds_plane_geometry (include/gfla_lds_plane.h) as a dict: G, ngroups, split, per, margin, lds; ragged = channels
    of the last group when it is narrower than G, else 0"""
    import ctypes
    B, C, Hs, Ws, Hf, Wf = shape
    out = (ctypes.c_int64 * 6)()
    rc = _lib.lib().gfla_lds_plane_geometry(int(op), B, C, Hs, Ws, Hf, Wf, int(k), int(dil), int(elem), int(needs),
                                            ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0, rc
    g = dict(zip(("G", "ngroups", "split", "per", "margin", "lds"), list(out)))
    g["ragged"] = C - (g["ngroups"] - 1) * g["G"] if g["G"] and C % g["G"] else 0
    return g
