"""Structured inputs, float64 stage references, exactness conditions and per-element error bars for the FC layers of
ExtractorAttn (csrc/fc_block.hip, fc_conv*.hip, fc_wino*.hip, fc_sample.hip, fc_tail.hip, fc_gemm.hip).  Shared by
test_fc_structured_cpu.py and test_fc_structured_gpu.py; everything here runs on the host in float64 / int64.

The layer, for source s, target t, flow f, conv0 (w0, b0), conv1 (w1, b1), kernel size k:
    Gs = conv_kxk(replicate_pad(s, k-1), w0[:, C:])        (B, 128, H+k-1, W+k-1)
    Gt = conv_kxk(replicate_pad(t, lo|hi), w0[:, :C])      (B, 128, H, W)
    hidden = b0 + Gt + bilinear_sample(Gs, p + f(p))       clamped corner indices, unclamped weights
    logits = b1 + w1 . leaky_relu(hidden)                  the slope at exactly 0 is the negative slope
"""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of float32
HID = 128
EXACT_BITS = 21         # sum |terms| < 2^21 quantum: exact even on an accumulator that aligns to the largest addend at 24 bits
F16_BITS = 11           # significant bits of one f16 term

# (k, B, C, H, W): the geometries the existing sweeps found necessary (test_fc_wino_gpu.py SWEEP, the collapse flow of
# test_fc_mfma_gpu.py): C below / equal to / straddling a 16-channel chunk, > 32 tiles per sample, maps smaller than a tile
# group, ragged tiles both ways
SHAPES = [(5, 3, 17, 7, 5), (5, 2, 16, 2, 9), (5, 1, 33, 13, 31), (3, 3, 17, 7, 5), (3, 1, 40, 13, 31), (3, 2, 8, 33, 65)]
COLLAPSE = (5, 3, 16, 40, 28)


# ================================================================================= 1. structure
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def sample_amp(B, exps):
    """powers of two spread over the batch (sample b gets 2^exps[b mod len])"""
    return torch.tensor([2.0 ** exps[b % len(exps)] for b in range(B)], dtype=torch.float64).reshape(B, 1, 1, 1)


def channel_amp(C, tail, emax):
    """powers of two within 2^0 .. 2^emax over the channels; the last (for C % 16 != 0: partially filled) 16-channel chunk is
    the quiet one (tail = 'quiet': 2^0, every other channel >= 2^1) or the loud one ('loud': 2^emax, the others below)"""
    e = (torch.arange(C) * 3) % (emax + 1)
    c0 = 16 * ((C - 1) // 16)
    last = torch.arange(C) >= (c0 if c0 > 0 else C // 2)   # a single chunk: its second half plays the tail
    if tail == "quiet":
        e = torch.where(last, torch.zeros_like(e), e.clamp(min=1))
    else:
        e = torch.where(last, torch.full_like(e, emax), e.clamp(max=max(emax - 1, 0)))
    return (2.0 ** e.double()).reshape(1, C, 1, 1)


def spatial_amp(H, W, kind, e, n_outliers=0, seed=0):
    """'loud_frame': a one-pixel frame at 2^e around an interior at 1;  'quiet_frame': the reverse;  plus isolated outliers at 2^e"""
    a = torch.ones(H, W, dtype=torch.float64)
    frame = torch.ones(H, W, dtype=torch.bool)
    if H > 2 and W > 2:
        frame[1:-1, 1:-1] = False
    if kind == "loud_frame":
        a[frame] = 2.0 ** e
    elif kind == "quiet_frame":
        a[~frame] = 2.0 ** e
    if n_outliers:
        idx = torch.randperm(H * W, generator=_gen(seed))[:n_outliers]
        a.view(-1)[idx] = 2.0 ** e
    return a.reshape(1, 1, H, W)


def amplitude(B, C, H, W, sample=None, channel=None, spatial=None, outliers=0, seed=0):
    """the product of the structures that are switched on (None = off): sample = exponents, channel = (tail, emax),
    spatial = (kind, exponent)"""
    a = torch.ones(B, C, H, W, dtype=torch.float64)
    if sample is not None:
        a = a * sample_amp(B, sample)
    if channel is not None:
        a = a * channel_amp(C, *channel)
    if spatial is not None or outliers:
        kind, e = spatial if spatial is not None else ("none", 3)
        a = a * spatial_amp(H, W, kind, e, outliers, seed)
    return a


def values(shape, kind, seed, r=2, density=1.0):
    """'int': integers in [-r, r];  'pos': post-ReLU-like integers (exact zeros, positive mean);  'gauss' / 'gauss_pos': the
    float counterparts.  density < 1 zeroes entries at random."""
    g = _gen(seed)
    if kind in ("int", "pos"):
        v = torch.randint(-r, r + 1, shape, generator=g).double()
    else:
        v = torch.randn(shape, generator=g, dtype=torch.float64)
    if kind in ("pos", "gauss_pos"):
        v = v.clamp(min=0)
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g, dtype=torch.float64) < density)
    return v


def peaked(shape, exact, seed, density=0.04, amp=None):
    """sparse, peaked upstream gradients: most entries exactly zero, a few large ones, as a softmax gives"""
    g = _gen(seed)
    keep = torch.rand(shape, generator=g, dtype=torch.float64) < density
    if exact:
        v = torch.randint(1, 4, shape, generator=g).double() * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)
        v = v * 2.0 ** torch.randint(0, 2, shape, generator=g).double()
    else:
        v = torch.randn(shape, generator=g, dtype=torch.float64) * 2.0 ** (3 * torch.rand(shape, generator=g, dtype=torch.float64))
    v = v * keep
    return v if amp is None else v * amp


def exact_flow(B, H, W, seed, reach=3, far=4):
    """fractional parts in {1/4, 1/2, 3/4}: bilinear weights are multiples of 1/16 and no position sits on the bilinear kink;
    `far` positions per sample leave the map by more than its size (every corner clamps)"""
    g = _gen(seed)
    f = torch.randint(-reach, reach + 1, (B, 2, H, W), generator=g).double()
    f = f + torch.randint(1, 4, (B, 2, H, W), generator=g).double() / 4
    for b in range(B):
        idx = torch.randperm(H * W, generator=g)[:far]
        sign = torch.randint(0, 2, (far,), generator=g).double() * 2 - 1
        f[b, 0].view(-1)[idx] += sign * (W + 6)
        f[b, 1].view(-1)[idx[: far // 2]] -= (H + 6)
    return f


def float_flow(B, H, W, seed):
    """smooth flow + noise (positions land at generic fractions), a few far out-of-range positions"""
    g = _gen(seed)
    n = torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
    f = F.avg_pool2d(F.pad(n * 6, (2, 2, 2, 2), mode="replicate"), 5, 1) + 0.3 * torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
    for b in range(B):
        idx = torch.randperm(H * W, generator=g)[:3]
        f[b, 0].view(-1)[idx] += W + 6.5
    return f


def collapse_flow(B, H, W):
    """every position of sample 0 lands in one corner cell of the map (several list rounds of the owner-computes scatter); the
    other samples far outside.  Fractions 1/4 and 3/4."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    f = torch.stack((0.25 - xs, 0.75 - ys))[None].repeat(B, 1, 1, 1)
    f[1:] = f[1:] + 100.0
    return f.contiguous()


# ---- the cases -------------------------------------------------------------------------------------------------------
# structure per shape: channel = (which 16-channel chunk is the tail, largest exponent of the exact case), spatial = (frame kind,
# exponent); every structure meets a k = 5 and a k = 3 shape
_STRUCT = {
    (5, 3, 17, 7, 5): dict(channel=("quiet", 3), spatial=("loud_frame", 2), positive=False),
    (5, 2, 16, 2, 9): dict(channel=("loud", 3), spatial=None, positive=True),
    (5, 1, 33, 13, 31): dict(channel=("loud", 2), spatial=("quiet_frame", 3), positive=False, outliers=3),
    (3, 3, 17, 7, 5): dict(channel=("loud", 3), spatial=("quiet_frame", 3), positive=True),
    # tests/placement_util.py's vector-friendly FC shapes: C, H W and the fold's R W multiples of 4
    (5, 3, 16, 8, 6): dict(channel=("quiet", 3), spatial=("loud_frame", 2), positive=False),
    (3, 3, 16, 8, 6): dict(channel=("loud", 3), spatial=("quiet_frame", 3), positive=True),
    (3, 1, 40, 13, 31): dict(channel=("quiet", 2), spatial=("loud_frame", 3), positive=False, outliers=3),
    (3, 2, 8, 33, 65): dict(channel=("quiet", 4), spatial=("loud_frame", 2), positive=True, up_density=0.005),
    COLLAPSE: dict(channel=("loud", 3), spatial=("loud_frame", 2), positive=False, up_density=0.001),
}
# per-sample exponents: 'wide' for the forward and the data / flow gradients, 'narrow' where sums run over the samples
# (weight and bias gradients): the spread of the samples' quanta is spent from the same 2^21
SPREAD = {"wide": (0, -11, 5), "narrow": (0, -2, 1), "quiet8": (0, -8, 0), "offset": (0, -2, 1)}
# 'offset' (exact cases, for the whole layer of mode 5 at k = 3, whose forward runs in the Winograd domain): the maps narrow, the
# upstream gradient wide, and conv0.bias + 2^-7 on every unit.  Every other term of a hidden unit is a multiple of 2^-6 (the
# quietest sample's quantum 2^-2 times the bilinear 1/16), so no unit is exactly 0 and |hidden| >= 2^-7, far above the error of a
# float32 Winograd forward at these magnitudes (asserted on the host with the emulation): the slopes, hence d hidden and all that
# is downstream of the data-gradient convolutions, are exact although the forward is not.
OFFSET = 2.0 ** -7


@functools.lru_cache(maxsize=None)
def make_case(shape, exact, spread="wide", seed=0):
    """All tensors of one layer call in float64 (every value float32-representable; for f16 cases float16-representable), with
    the structure of _STRUCT[shape] and the per-sample amplitudes SPREAD[spread]."""
    k, B, C, H, W = shape
    st = _STRUCT[shape]
    sexp = SPREAD[spread]
    vk = ("pos" if st["positive"] else "int") if exact else ("gauss_pos" if st["positive"] else "gauss")
    # (the exact cases spend the channel spread from their 2^21: 2^0 .. 2^2-4; the float cases use the full 2^0 .. 2^6)
    channel = st["channel"] if exact else (st["channel"][0], 6)
    amp = lambda sd: amplitude(B, C, H, W, sample=sexp, channel=channel, spatial=st["spatial"], outliers=st.get("outliers", 0), seed=sd)
    c = dict(k=k, B=B, C=C, H=H, W=W, exact=exact, spread=spread, shape=shape, slope=0.25 if k == 3 else 0.5)
    c["s"] = values((B, C, H, W), vk, seed + 1, r=1) * amp(seed + 11)
    c["t"] = values((B, C, H, W), vk, seed + 2, r=1) * amp(seed + 12)   # (the same sample is the quiet one: hidden adds both halves)
    ho, wo = H + k - 1, W + k - 1
    up_amp = sample_amp(B, SPREAD["wide"] if spread == "offset" else sexp if spread != "narrow" else (0,))
    if exact:
        c["f"] = collapse_flow(B, H, W) if shape == COLLAPSE else exact_flow(B, H, W, seed + 3)
        c["w0"] = values((HID, 2 * C, k, k), "int", seed + 4, r=1, density=0.3)
        c["b0"] = values((HID,), "int", seed + 5, r=1, density=0.25) + (OFFSET if spread == "offset" else 0.0)
        c["w1"] = values((k * k, HID), "int", seed + 6, r=1, density=0.4)
        c["b1"] = values((k * k,), "int", seed + 7, r=3)
    else:
        c["f"] = float_flow(B, H, W, seed + 3)
        c["w0"] = values((HID, 2 * C, k, k), "gauss", seed + 4) / (2 * C * k * k) ** 0.5
        c["b0"] = values((HID,), "gauss", seed + 5) * 0.1
        c["w1"] = values((k * k, HID), "gauss", seed + 6) / HID ** 0.5
        c["b1"] = values((k * k,), "gauss", seed + 7) * 0.1
    c["up"] = peaked((B, k * k, H, W), exact, seed + 8, density=st.get("up_density", 0.04), amp=up_amp)
    # gradient maps for the per-half entry points (what the tail hands to the convolutions: sparse, peaked, per sample)
    c["dG1"] = peaked((B, HID, ho, wo), exact, seed + 9, density=0.03, amp=up_amp)
    c["dG0"] = peaked((B, HID, H, W), exact, seed + 10, density=0.03, amp=up_amp)
    for n in ("s", "t", "f", "w0", "b0", "w1", "b1", "up", "dG0", "dG1"):
        c[n] = c[n].float().double().contiguous()
    return c


def pads(k, is_source):
    lo, hi = k // 2, k - 1 - k // 2
    return (k - 1, k - 1, k - 1, k - 1) if is_source else (lo, hi, lo, hi)


def half_weights(w0, C, is_source):
    return w0[:, C:] if is_source else w0[:, :C]


# ================================================================================= float64 stage references
def corners(f, H, W, k):
    """csrc/fc_sample.hip: corners() in float64: flat indices into the (Ho, Wo) convolved source map and the four weights
    (clamped indices, unclamped weights: block_extractor_kernel.cu:58-76); weights differentiable in the flow"""
    lo, hi = k // 2, k - 1 - k // 2
    wo = W + k - 1
    ys, xs = torch.meshgrid(torch.arange(H, dtype=f.dtype), torch.arange(W, dtype=f.dtype), indexing="ij")
    dx, dy = f[:, 0] + xs, f[:, 1] + ys
    fdx, fdy = torch.floor(dx.detach()), torch.floor(dy.detach())
    xr, yb = dx - fdx, dy - fdy
    xl, yt = 1 - xr, 1 - yb
    qx, qy = fdx.long(), fdy.long()
    gx0, gx1 = qx.clamp(-hi, W - 1 + lo) + hi, (qx + 1).clamp(-hi, W - 1 + lo) + hi
    gy0, gy1 = qy.clamp(-hi, H - 1 + lo) + hi, (qy + 1).clamp(-hi, H - 1 + lo) + hi
    B = f.shape[0]
    idx = [(gy0 * wo + gx0), (gy0 * wo + gx1), (gy1 * wo + gx0), (gy1 * wo + gx1)]
    wts = [xl * yt, xr * yt, xl * yb, xr * yb]
    return [i.reshape(B, 1, -1) for i in idx], [w.reshape(B, 1, -1) for w in wts]


def sample_map(G, idx, wts, H, W):
    """sum of the four weighted corner rows of G (B, N, Ho, Wo) -> (B, N, H, W)"""
    B, N = G.shape[:2]
    flat = G.reshape(B, N, -1)
    out = sum(w * torch.gather(flat, 2, i.expand(B, N, -1)) for i, w in zip(idx, wts))
    return out.reshape(B, N, H, W)


def scatter_map(d, idx, wts, Ho, Wo):
    """the adjoint of sample_map in its map argument: d (B, N, H, W) -> (B, N, Ho, Wo)"""
    B, N = d.shape[:2]
    out = torch.zeros(B, N, Ho * Wo, dtype=d.dtype)
    for i, w in zip(idx, wts):
        out.scatter_add_(2, i.expand(B, N, -1), d.reshape(B, N, -1) * w)
    return out.reshape(B, N, Ho, Wo)


def leaky(h, slope):
    return torch.where(h > 0, h, h * slope)


def layer_reference(c, bug=None):
    """The whole layer in float64, stage by stage, with every intermediate, and all seven gradients for the upstream gradient
    c['up'].  `bug`: a planted defect (test_fc_structured_cpu.py), see plant()."""
    k, B, C, H, W, slope = c["k"], c["B"], c["C"], c["H"], c["W"], c["slope"]
    leaf = {n: c[n].clone().requires_grad_() for n in ("s", "t", "f", "w0", "b0", "w1", "b1")}
    sp, tp = F.pad(leaf["s"], pads(k, 1), mode="replicate"), F.pad(leaf["t"], pads(k, 0), mode="replicate")
    if bug == "reflect":   # reflect where replicate belongs, on the left edge of the quiet sample's target map
        lo, q = k // 2, quiet_sample(c)
        tq = leaf["t"][q]
        rows = torch.cat((tq[:, :1].expand(-1, lo, -1), tq, tq[:, -1:].expand(-1, k - 1 - lo, -1)), 1)   # rows padded: (C, Hp, W)
        tp = tp.clone()
        tp[q, :, :, :lo] = rows[:, :, 1:lo + 1].flip(-1)
    ws, wt_ = leaf["w0"][:, C:], leaf["w0"][:, :C]
    Gs, Gt = F.conv2d(sp, ws), F.conv2d(tp, wt_)
    if bug in ("chunk", "lo"):
        Gs = Gs + plant(c, bug, sp.detach(), ws.detach())
    if bug == "tap":
        Gt = Gt + plant(c, bug, tp.detach(), wt_.detach())
    Gs.retain_grad(), Gt.retain_grad()
    idx, wts = corners(leaf["f"], H, W, k)
    hidden = leaf["b0"].reshape(1, -1, 1, 1) + Gt + sample_map(Gs, idx, wts, H, W)
    hidden.retain_grad()
    act = leaky(hidden, slope)
    logits = torch.einsum("qo,bohw->bqhw", leaf["w1"], act) + leaf["b1"].reshape(1, -1, 1, 1)
    logits.backward(c["up"])
    r = dict(Gs=Gs.detach(), Gt=Gt.detach(), hidden=hidden.detach(), act=act.detach(), logits=logits.detach(),
             dh=hidden.grad, dGs=Gs.grad, idx=idx, wts=[w.detach() for w in wts], sp=sp.detach(), tp=tp.detach())
    for n, v in leaf.items():
        r["g_" + n] = v.grad
    return r


def plant(c, bug, sp, ws):
    """the additive change of a convolved map (padded input sp, weights ws) a planted forward bug makes (see the table in
    test_fc_structured_cpu.py)"""
    k, B, C = c["k"], c["B"], c["C"]
    q = quiet_sample(c)
    d = torch.zeros(B, HID, sp.shape[2] - k + 1, sp.shape[3] - k + 1, dtype=torch.float64)
    if bug == "tap":      # tap (k-1, k-2) dropped in the last m x m tile of the quiet sample's target map
        m = 2 if k == 5 else 4
        ho, wo = d.shape[2:]
        y0, x0 = (ho - 1) // m * m, (wo - 1) // m * m
        i, j = k - 1, k - 2
        win = sp[q, :, y0 + i:ho + i, x0 + j:wo + j]
        d[q, :, y0:, x0:] = -torch.einsum("chw,nc->nhw", win, ws[:, :, i, j])
    elif bug == "chunk":  # the last (partial) 16-channel chunk skipped in the quiet sample
        c0 = 16 * ((C - 1) // 16)
        d[q] = -F.conv2d(sp[q:q + 1, c0:], ws[:, c0:])[0]
    elif bug == "lo":     # the lo term of the two-term f16 split dropped for the quiet sample (activations only)
        e = torch.floor(torch.log2(sp.abs().max()))
        scale = 2.0 ** (14 - e)
        hi = (sp[q:q + 1] * scale).half().double() / scale
        d[q] = F.conv2d(hi - sp[q:q + 1], ws)[0]
    return d


def quiet_sample(c):
    """the sample of the source map with the smallest amplitude"""
    return int(torch.argmin(c["s"].abs().amax((1, 2, 3))))


def half_reference(c, is_source):
    """one half through the per-half entry points: map, data gradient, weight gradient for the gradient map c['dG<half>']"""
    k, C = c["k"], c["C"]
    x = (c["s"] if is_source else c["t"]).clone().requires_grad_()
    w = half_weights(c["w0"], C, is_source).clone().requires_grad_()
    xp = F.pad(x, pads(k, is_source), mode="replicate")
    y = F.conv2d(xp, w)
    dG = c["dG%d" % is_source]
    y.backward(dG)
    return dict(y=y.detach(), gx=x.grad, gw=w.grad, xp=xp.detach(), w=w.detach(), dG=dG)


def fold(gpad, k, is_source, H, W):
    """the adjoint of the replicate padding (linear: also folds bounds)"""
    x0 = torch.zeros(gpad.shape[0], gpad.shape[1], H, W, dtype=gpad.dtype, requires_grad=True)
    return torch.autograd.grad(F.pad(x0, pads(k, is_source), mode="replicate"), x0, gpad)[0]


def dgrad_pad(dG, w, k):
    """the data gradient on the padded domain: full correlation of the gradient map with the flipped taps"""
    return F.conv2d(F.pad(dG, (k - 1,) * 4), w.flip(2, 3).transpose(0, 1))


def wgrad(xp, dG, k):
    return torch.nn.grad.conv2d_weight(xp, (dG.shape[1], xp.shape[1], k, k), dG)


# ================================================================================= 2. exactness condition
def lsb(t):
    """the value of the lowest set bit of every element (its quantum); inf for zeros"""
    m, e = torch.frexp(t.abs())
    mi = (m * 2.0 ** 53).long()
    low = (mi & -mi).double()
    return torch.where(t == 0, torch.full_like(t, float("inf")), low * 2.0 ** (e.double() - 53))


def qmin(t, per_sample=False):
    """the smallest quantum among the entries of t (of every sample)"""
    q = lsb(t)
    return q.reshape(q.shape[0], -1).amin(1) if per_sample else q.amin()


def _bshape(q, like):
    return q.reshape(-1, *([1] * (like.dim() - 1)))


def _ratio(S, q):
    """max over the elements of sum|terms| / (2^21 q): the condition holds below 1.  q: scalar, or one value per sample."""
    q = _bshape(q, S) if q.dim() else q
    r = S / (2.0 ** EXACT_BITS * q)
    return float(torch.nan_to_num(r, nan=0.0).amax())     # (0 / inf: no terms)


def f16_operand_ok(t):
    """an operand tensor of the f16-term kernels: at most 11 significant bits per element, and, scaled by the tensor's power of
    two (fc_scale_exp: 2^(14 - e), e the exponent of max |x|), a multiple of the smallest f16 subnormal 2^-24: hi carries the
    value alone, lo = 0"""
    nz = t[t != 0]
    if nz.numel() == 0:
        return True
    q = lsb(nz)
    e = torch.floor(torch.log2(nz.abs().max()))
    return bool(((nz.abs() / q) < 2.0 ** F16_BITS).all()) and bool((q * 2.0 ** (14 - e) >= 2.0 ** -24).all())


def half_exactness(c, is_source):
    """{stage: ratio} for the per-half entry points: ratio < 1 <=> sum |terms| < 2^21 q for every output element, with q a lower
    bound of the smallest quantum among the element's terms (product of the factors' smallest quanta; per sample where the
    sum stays inside a sample, over all samples where it runs over them)"""
    k = c["k"]
    r = half_reference(c, is_source)
    qx, qw, qg = qmin(r["xp"], True), qmin(r["w"]), qmin(r["dG"], True)
    out = {"y": _ratio(F.conv2d(r["xp"].abs(), r["w"].abs()), qx * qw)}
    Sx = fold(dgrad_pad(r["dG"].abs(), r["w"].abs(), k), k, is_source, c["H"], c["W"])
    out["gx"] = _ratio(Sx, qg * qw)
    out["gw"] = _ratio(wgrad(r["xp"].abs(), r["dG"].abs(), k), (qx * qg).amin())
    out["f16"] = all(f16_operand_ok(t) for t in (r["xp"], r["w"], r["dG"]))
    return out


def layer_exactness(c):
    """{stage: ratio} for every stage of the whole layer and its backward (the products of a stage are its terms), 'f16': the
    operand condition of the f16-term modes on every tensor a convolution or weight gradient reads, 'fixed': the 64-bit
    fixed-point cells of the owner-computes scatter hold every contribution exactly (scale 2^40 / max |d hidden|)."""
    k, B, C, H, W, slope = c["k"], c["B"], c["C"], c["H"], c["W"], c["slope"]
    r = layer_reference(c)
    a = lambda t: t.abs()
    ws, wt_ = c["w0"][:, C:], c["w0"][:, :C]
    q_s, q_t, q_w0 = qmin(r["sp"], True), qmin(r["tp"], True), qmin(c["w0"])
    q_b0, q_w1, q_b1, q_up = qmin(c["b0"]), qmin(c["w1"]), qmin(c["b1"]), qmin(c["up"], True)
    out = {}
    S_Gs, S_Gt = F.conv2d(a(r["sp"]), a(ws)), F.conv2d(a(r["tp"]), a(wt_))
    out["Gs"], out["Gt"] = _ratio(S_Gs, q_s * q_w0), _ratio(S_Gt, q_t * q_w0)
    wa = [a(w) for w in r["wts"]]
    q_h = torch.minimum(torch.minimum(q_s * q_w0 / 16, q_t * q_w0), q_b0.expand(B))
    S_h = a(c["b0"]).reshape(1, -1, 1, 1) + a(r["Gt"]) + sample_map(a(r["Gs"]), r["idx"], wa, H, W)
    out["hidden"] = _ratio(S_h, q_h)
    q_act = q_h * slope
    S_l = torch.einsum("qo,bohw->bqhw", a(c["w1"]), a(r["act"])) + a(c["b1"]).reshape(1, -1, 1, 1)
    out["logits"] = _ratio(S_l, torch.minimum(q_act * q_w1, q_b1.expand(B)))
    # backward
    S_ga = torch.einsum("qo,bqhw->bohw", a(c["w1"]), a(c["up"]))
    q_dh = q_w1 * q_up * slope
    out["dh"] = _ratio(S_ga, q_w1 * q_up)
    out["g_b1"] = _ratio(a(c["up"]).sum((0, 2, 3)), q_up.amin())
    out["g_w1"] = _ratio(torch.einsum("bohw,bqhw->qo", a(r["act"]), a(c["up"])), (q_act * q_up).amin())
    out["g_b0"] = _ratio(a(r["dh"]).sum((0, 2, 3)), q_dh.amin())
    ho, wo = H + k - 1, W + k - 1
    S_dGs = scatter_map(a(r["dh"]), r["idx"], wa, ho, wo)
    q_dGs = q_dh / 16
    out["dGs"] = _ratio(S_dGs, q_dGs)
    amax = r["dh"].abs().max()
    cell = 2.0 ** (torch.floor(torch.log2(amax)) - 40) if amax > 0 else torch.tensor(0.0, dtype=torch.float64)
    out["fixed"] = bool((q_dGs >= cell).all()) and bool((S_dGs < cell * 2.0 ** 62).all())
    # flow gradient: d hidden x corner value x one-dimensional weight (multiples of 1/4), four corners, 128 channels
    S_f = (a(r["dh"]) * sample_map(a(r["Gs"]), r["idx"], [torch.ones_like(w) for w in wa], H, W)).sum(1)
    out["g_f"] = _ratio(S_f, q_dh * q_s * q_w0 / 4)
    out["g_s"] = _ratio(fold(dgrad_pad(S_dGs, a(ws), k), k, 1, H, W), q_dGs * q_w0)
    out["g_t"] = _ratio(fold(dgrad_pad(a(r["dh"]), a(wt_), k), k, 0, H, W), q_dh * q_w0)
    out["g_w0"] = max(_ratio(wgrad(a(r["sp"]), S_dGs, k), (q_s * q_dGs).amin()),
                      _ratio(wgrad(a(r["tp"]), a(r["dh"]), k), (q_t * q_dh).amin()))
    out["f16"] = all(f16_operand_ok(t) for t in (r["sp"], r["tp"], c["w0"], r["dGs"], r["dh"]))
    out["f16_fwd"] = all(f16_operand_ok(t) for t in (r["sp"], r["tp"], c["w0"]))
    return out


FWD_STAGES = ("Gs", "Gt", "hidden", "logits")
DATA_STAGES = FWD_STAGES + ("dh", "dGs", "g_f", "g_s", "g_t", "g_b1")
PARAM_STAGES = DATA_STAGES + ("g_w1", "g_b0", "g_w0")
# what the exact GPU cases compare, per spread: outputs -> the stages that must satisfy the condition
OFFSET_STAGES = ("dh", "dGs", "g_s", "g_t", "g_b1")
EXACT_OUTPUTS = {"offset": ("g_s", "g_t", "g_b1"), "wide": ("logits", "g_s", "g_t", "g_f", "g_b1"), "narrow": ("logits", "g_s", "g_t", "g_f", "g_w0", "g_b0", "g_w1", "g_b1")}


def exact_ok(report, spread):
    stages = DATA_STAGES if spread == "wide" else PARAM_STAGES
    return all(report[s] < 1.0 for s in stages) and report["fixed"] and report["f16"]


# ================================================================================= 3. per-element bars
def pow2_ceil(v):
    v = float(v)
    return 0.0 if v == 0 else 2.0 ** torch.ceil(torch.log2(torch.tensor(v, dtype=torch.float64))).item()


def direct_bar(S, K, mode=0, x=None, w=None, conv=None):
    """|y - y64| <= 2 (K + 2) 2^-24 S for a sum of K float32 products accumulated in float32 in any order (each product and each
    partial sum rounds once, |partial| <= S; the factor 2 covers the second-order terms and the conversion of the result), S
    the float64 sum of the absolute products.
    Split modes (2, 5: two f16 terms per operand, hi.hi + hi.lo + lo.hi; 3: three terms): every operand is hi + lo to 2^-24 of
    its own magnitude and the dropped lo.lo is below 2^-22 of the product: 2^-21 per product -> + 2^-21 S
    (mode 3 keeps every term above 2^-32: + 2^-30 S).  The lo term is an f16 in the tensor's scale 2^(14 - e) (fc_scale_exp), so
    it is rounded to the f16 subnormal quantum 2^-24 there: an ABSOLUTE error of at most 2^(e - 39) per operand value, which in
    the products is 2^-39 (2^ex sum|w| + 2^ew sum|x|): `conv(ones, |w|)` and `conv(|x|, ones)` scaled by the tensors' powers
    of two.  It matters only for entries below ~2^-15 of the tensor's largest.
    Mode 1 (ONE f16 term per operand: the arithmetic of the bf16 / f16 feature path): every operand is rounded to 11 significant
    bits, x^ = x (1 + d), |d| <= 2^-11, so a product is off by at most (2 . 2^-11 + 2^-22) |x w| -> + (2^-10 + 2^-22) S; the one
    term meets the same subnormal quantum, so the absolute term is the same."""
    bar = 2.0 * (K + 2) * U * S
    if mode == 1:
        bar = bar + (2.0 ** -10 + 2.0 ** -22) * S
    if mode in (2, 5):
        bar = bar + 2.0 ** -21 * S
    elif mode == 3:
        bar = bar + 2.0 ** -30 * S
    if mode in (1, 2, 3, 5) and conv is not None:
        ex, ew = pow2_ceil(x.abs().max()), pow2_ceil(w.abs().max())
        bar = bar + 2.0 ** -39 * (ex * conv(torch.ones_like(x), w.abs()) + ew * conv(x.abs(), torch.ones_like(w)))
    return bar


# ---- float32 emulation of the Winograd-domain formulation (csrc/fc_wino_shared.h, points {0, 1, -1, 2, -1/2, inf}) -------------
WN_BT = [[1, 1.5, -2, -1.5, 1, 0], [0, -1, -2.5, -0.5, 1, 0], [0, 1, 0.5, -2.5, 1, 0], [0, -0.5, -1, 0.5, 1, 0],
         [0, 2, -1, -2, 1, 0], [0, 1, 1.5, -2, -1.5, 1]]
WN_AT = {2: [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -0.5, 1]],
         4: [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -0.5, 0], [0, 1, 1, 4, 0.25, 0], [0, 1, -1, 8, -0.125, 1]]}


def wn_mats(k, dt):
    m = 2 if k == 5 else 4
    G = torch.zeros(6, k, dtype=torch.float64)
    G[0, 0] = 1
    G[5, k - 1] = 1
    j = torch.arange(k, dtype=torch.float64)
    G[1] = -torch.ones(k, dtype=torch.float64) / 3
    G[2] = (-1.0) ** j / 3
    G[3] = 2.0 ** j / 15
    G[4] = -16 * (-0.5) ** j / 15
    return (torch.tensor(WN_BT, dtype=torch.float64).to(dt), G.to(dt), torch.tensor(WN_AT[m], dtype=torch.float64).to(dt), m)


def wn_extend(lin, rows, cols):
    """A linearised map (B, C, R, Wp; row pitch Wp) as the tiles read it: column x >= Wp of row y is pixel (y + 1, x - Wp) -- the
    ragged tiles of the last tile column see the beginning of the next row --, zeros behind the map"""
    B, C, R, Wp = lin.shape
    flat = torch.cat((lin.reshape(B, C, -1), torch.zeros(B, C, (rows + 2) * Wp + cols, dtype=lin.dtype)), 2)
    ys, xs = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    return flat[:, :, (ys * Wp + xs).reshape(-1)].reshape(B, C, rows, cols)


def wn_tiles(lin, Hv, Wv, k):
    m = 2 if k == 5 else 4
    TH, TW = -(-Hv // m), -(-Wv // m)
    return wn_extend(lin, TH * m + 6 + k, TW * m + 6 + k), TH, TW, m


def wn_conv(lin, w, Hv, Wv, k, dt):
    """out[y, x] = sum lin[y + i, x + j] w[i, j] on the (Hv, Wv) domain, in the Winograd domain with every step in `dt`"""
    ext, TH, TW, m = wn_tiles(lin, Hv, Wv, k)
    BT, G, AT, _ = wn_mats(k, dt)
    tiles = ext[:, :, :TH * m + 6 - m, :TW * m + 6 - m].to(dt).unfold(2, 6, m).unfold(3, 6, m)
    Uw = torch.einsum("ai,ncij,ej->aenc", G, w.to(dt), G)
    V = torch.einsum("ai,bcyxij,ej->aebyxc", BT, tiles, BT)
    M = torch.einsum("aebyxc,aenc->aebyxn", V, Uw)
    Y = torch.einsum("ia,aebyxn,je->bnyixj", AT, M, AT)
    return Y.reshape(lin.shape[0], w.shape[0], TH * m, TW * m)[:, :, :Hv, :Wv]


def wn_conv_stile(lin, w, Hv, Wv, k):
    """S_tile: the float64 sum of absolute products, maximised over the 6 x 6 input window of the element's tile, i.e. over every
    output position whose own k x k window meets it (tile origin - (k - 1) ... origin + 5 both ways, clipped to the map): the
    products of a Winograd tile pair every input of the window with every tap"""
    ext, TH, TW, m = wn_tiles(lin, Hv, Wv, k)
    S = F.conv2d(ext.abs(), w.abs())[:, :, :TH * m + 6 - m, :TW * m + 6 - m]
    St = F.max_pool2d(F.pad(S, (k - 1, 0, k - 1, 0)), 6 + k - 1, m)          # (B, N, TH, TW)
    return St.repeat_interleave(m, 2).repeat_interleave(m, 3)[:, :, :Hv, :Wv]


def wn_wgrad(lin, dG, k, dt):
    """dW[n, c, i, j] = sum lin[y + i, x + j] dG[n, y, x] in the Winograd domain (G^T (sum_tiles V . A dY A^T) G), steps in `dt`"""
    Hv, Wv = dG.shape[2:]
    ext, TH, TW, m = wn_tiles(lin, Hv, Wv, k)
    BT, G, AT, _ = wn_mats(k, dt)
    tiles = ext[:, :, :TH * m + 6 - m, :TW * m + 6 - m].to(dt).unfold(2, 6, m).unfold(3, 6, m)
    dyt = F.pad(dG, (0, TW * m - Wv, 0, TH * m - Hv)).to(dt).unfold(2, m, m).unfold(3, m, m)
    V = torch.einsum("ai,bcyxij,ej->aebyxc", BT, tiles, BT)
    Zh = torch.einsum("ia,bnyxij,je->aebyxn", AT, dyt, AT)
    dU = torch.einsum("aebyxc,aebyxn->aenc", V, Zh)
    return torch.einsum("ai,aenc,ej->ncij", G, dU, G)


def wn_wgrad_stile(lin, dG, k):
    """the weight gradient's S_tile: sum |x| |dY| at every offset a 6 x 6 window puts between an input and a gradient entry of
    its m x m tile (-(m - 1) ... 5 both ways), maximised over the offsets"""
    Hv, Wv = dG.shape[2:]
    ext, TH, TW, m = wn_tiles(lin, Hv, Wv, k)
    xa = F.pad(ext[:, :, :Hv + 5, :Wv + 5].abs(), (m - 1, 0, m - 1, 0))
    S6 = torch.nn.grad.conv2d_weight(xa, (dG.shape[1], lin.shape[1], 5 + m, 5 + m), dG.abs())
    return S6.amax((2, 3), keepdim=True).expand(-1, -1, k, k)


def _pow2_floor_exp(t):
    return float(torch.floor(torch.log2(t.abs().max()))) if float(t.abs().max()) > 0 else -200.0


WN16_HEAD_X, WN16_HEAD_W, WN16_HEAD_Z = 6, 3, 4   # bits of headroom below fc_scale_exp for B^T d B, G w G^T, A dY A^T


def wn16_conv_lo(lin, w, Hv, Wv, k, x_max, w_max):
    """The lo-subnormal term of the Winograd-domain two-term f16 convolution (fc_wino16.hip).  A transformed value is split in the
    scale 2^(14 - e - headroom), e the exponent of the RAW tensor's max |x| (fc_scale_exp, wn16_scale_exp); its lo term is rounded
    to the f16 subnormal quantum 2^-24 there: an absolute error of at most 2^(e + headroom - 39) per transformed value --
    dV for the inputs (6 bits), dU for the weights (3 bits).  Through the products and the output transform:
    |dY| <= |A^T| (sum_c dV |U| + |V| dU) |A|, evaluated here in float64."""
    ext, TH, TW, m = wn_tiles(lin, Hv, Wv, k)
    BT, G, AT, _ = wn_mats(k, torch.float64)
    tiles = ext[:, :, :TH * m + 6 - m, :TW * m + 6 - m].unfold(2, 6, m).unfold(3, 6, m)
    Uw = torch.einsum("ai,ncij,ej->aenc", G, w, G).abs()
    V = torch.einsum("ai,bcyxij,ej->aebyxc", BT, tiles, BT).abs()
    dV = 2.0 ** (_pow2_floor_exp(x_max) + WN16_HEAD_X - 39)
    dU = 2.0 ** (_pow2_floor_exp(w_max) + WN16_HEAD_W - 39)
    dM = dV * Uw.sum(3)[:, :, None, None, None, :] + dU * V.sum(5)[..., None]          # (a, e, b, y, x, n)
    Y = torch.einsum("ia,aebyxn,je->bnyixj", AT.abs(), dM, AT.abs())
    return Y.reshape(lin.shape[0], w.shape[0], TH * m, TW * m)[:, :, :Hv, :Wv]


def wn16_wgrad_lo(lin, dG, k, x_max, z_max):
    """the same for the two-term f16 weight gradient (fc_wino16.hip: fc_wino16_wgrad_kernel): dV as above, dZ = 2^(ez + 4 - 39) for
    the lifted gradient tiles A dY A^T; |d dW| <= |G^T| (sum_tiles dV |Zh| + |V| dZ) |G|"""
    Hv, Wv = dG.shape[2:]
    ext, TH, TW, m = wn_tiles(lin, Hv, Wv, k)
    BT, G, AT, _ = wn_mats(k, torch.float64)
    tiles = ext[:, :, :TH * m + 6 - m, :TW * m + 6 - m].unfold(2, 6, m).unfold(3, 6, m)
    dyt = F.pad(dG, (0, TW * m - Wv, 0, TH * m - Hv)).unfold(2, m, m).unfold(3, m, m)
    V = torch.einsum("ai,bcyxij,ej->aebyxc", BT, tiles, BT).abs()
    Zh = torch.einsum("ia,bnyxij,je->aebyxn", AT, dyt, AT).abs()
    dV = 2.0 ** (_pow2_floor_exp(x_max) + WN16_HEAD_X - 39)
    dZ = 2.0 ** (_pow2_floor_exp(z_max) + WN16_HEAD_Z - 39)
    dU = dV * Zh.sum((2, 3, 4))[:, :, :, None] + dZ * V.sum((2, 3, 4))[:, :, None, :]    # (a, e, n, c)
    return torch.einsum("ai,aenc,ej->ncij", G.abs(), dU, G.abs())


def z_lin(dG, k):
    """a gradient map in "Z layout" as a linearised map of row pitch Wp = Wo + k - 1: k - 1 zero rows / columns ahead"""
    return F.pad(dG, (k - 1, 0, k - 1, k - 1))


def measure_c(err, S_tile):
    """c = max err_host / (2^-24 S_tile): the amplification of the float32 Winograd emulation on these very inputs"""
    ok = S_tile > 0
    return float((err[ok] / (U * S_tile[ok])).max()) if bool(ok.any()) else 0.0


WINO_MARGIN = 4.0   # another valid float32 order of the same sums (the margin of test_golden_network_float32)


def is_wino(mode, k, leg):
    """fc_plan: which legs run in the Winograd domain"""
    if mode == 4:
        return True
    if mode == 5:
        return (leg == "fwd" and k == 3) or leg == "wgrad"
    if mode == 1:     # wgrad_x32: the f16 records are unpacked to float32 and the k = 5 weight gradient runs in the Winograd domain
        return leg == "wgrad" and k == 5
    return False


@functools.lru_cache(maxsize=None)
def half_bars(shape, is_source, spread="wide", seed=0):
    """float case of one half: reference, direct-kernel bars per mode, and for the Winograd-domain legs S_tile and the measured
    constants c (host emulation in float32 against float64 on these inputs)."""
    c = make_case(shape, False, spread, seed)
    k, C, H, W = c["k"], c["C"], c["H"], c["W"]
    r = half_reference(c, is_source)
    xp, w, dG = r["xp"], r["w"], r["dG"]
    Hp, Wp = xp.shape[2:]
    Ho, Wo = dG.shape[2:]
    wf = w.flip(2, 3).transpose(0, 1)
    out = dict(ref=r, case=c)
    conv = lambda a, b: F.conv2d(a, b)
    out["S_y"] = conv(xp.abs(), w.abs())
    out["split_y"] = lambda mode: direct_bar(out["S_y"], C * k * k, mode, xp, w, conv)
    zp = F.pad(dG, (k - 1,) * 4)
    S_xp = conv(zp.abs(), wf.abs())
    fo = lambda g: fold(g, k, is_source, H, W)
    # the fold adds up to (pad + 1)^2 <= k^2 padded entries per element: K + k^2
    out["bar_gx"] = lambda mode: fo(direct_bar(S_xp, HID * k * k + k * k, mode, zp, wf, conv))
    S_w = out["S_w"] = wgrad(xp.abs(), dG.abs(), k)
    nterm = dG.shape[0] * Ho * Wo
    out["bar_gw"] = lambda mode: direct_bar(S_w, nterm, mode) + (2.0 ** -39 * (
        pow2_ceil(xp.abs().max()) * dG.abs().sum((0, 2, 3)).reshape(-1, 1, 1, 1) + pow2_ceil(dG.abs().max()) * wgrad(xp.abs(), torch.ones_like(dG), k))
        if mode in (1, 2, 3, 5) else 0.0)
    # Winograd-domain legs
    y32 = wn_conv(xp, w, Ho, Wo, k, torch.float32).double()
    out["St_y"] = wn_conv_stile(xp, w, Ho, Wo, k)
    out["c_y"] = measure_c((y32 - r["y"]).abs(), out["St_y"])
    zl = z_lin(dG, k)
    gp64 = conv(zp, wf)
    gp32 = wn_conv(zl, wf, Hp, Wp, k, torch.float32).double()
    St_x = out["St_x"] = wn_conv_stile(zl, wf, Hp, Wp, k)
    out["c_gx"] = measure_c((gp32 - gp64).abs(), St_x)
    out["wbar_gx"] = lambda: fo(WINO_MARGIN * out["c_gx"] * U * St_x + 2.0 * (k * k + 2) * U * S_xp)
    gw32 = wn_wgrad(xp, dG, k, torch.float32).double()
    out["St_w"] = wn_wgrad_stile(xp, dG, k)
    out["c_gw"] = measure_c((gw32 - r["gw"]).abs(), out["St_w"])
    out["emul"] = dict(y=y32, gp=gp32, gp64=gp64, gw=gw32)
    return out


def is_wino16(mode, k, leg, both=False):
    """... and of those, which run on two-term f16 operands: mode 5, the k = 3 forward and the k = 5 weight gradient; mode 1, the
    k = 5 weight gradient when both halves run as one grid (`both`: the whole layer; fc_plan: wgrad_both), float32 operands on
    the per-half entry points"""
    if mode == 1:
        return both and leg == "wgrad" and k == 5
    return mode == 5 and ((leg == "fwd" and k == 3) or (leg == "wgrad" and k == 5))


def x_rounding(mode, S):
    """mode 1's Winograd-domain weight gradient reads the activations as they were packed -- one f16 term, |d| <= 2^-11 --, the
    gradient map in float32: + 2^-11 S"""
    return 2.0 ** -11 * S if mode == 1 else 0.0


def half_bar(hb, mode, leg):
    """the bar of one output of the per-half entry points in `mode`: leg = 'fwd' | 'dgrad' | 'wgrad'"""
    c, r = hb["case"], hb["ref"]
    k = c["k"]
    if is_wino(mode, k, leg):
        if leg == "fwd":
            lo = wn16_conv_lo(r["xp"], r["w"], r["dG"].shape[2], r["dG"].shape[3], k, r["xp"], c["w0"]) if is_wino16(mode, k, leg) else 0.0
            return WINO_MARGIN * hb["c_y"] * U * hb["St_y"] + lo
        if leg == "dgrad":
            return hb["wbar_gx"]()
        lo = wn16_wgrad_lo(r["xp"], r["dG"], k, r["xp"], r["dG"]) if is_wino16(mode, k, leg) else 0.0
        return WINO_MARGIN * hb["c_gw"] * U * hb["St_w"] + lo + x_rounding(mode, hb["S_w"])
    return {"fwd": hb["split_y"], "dgrad": hb["bar_gx"], "wgrad": hb["bar_gw"]}[leg](mode)


def worst_ratio(got, want, bar):
    """max |got - want| / bar over the elements (elements whose bar is 0 must be equal)"""
    err = (got.double() - want).abs()
    zero = bar <= 0
    if bool((err[zero] > 0).any()):
        return float("inf")
    return float((err[~zero] / bar[~zero]).max()) if bool((~zero).any()) else 0.0


def old_rule(got, want, tol):
    """the rule of the round-2 tests: max |got - want| / max |want| <= tol"""
    return float((got.double() - want).abs().max() / want.abs().max().clamp(min=1e-30)) <= tol


# ---- the whole layer: the stage bars propagated ------------------------------------------------------------------------
FLOW_EPS = 2.0 ** -10   # flow-gradient entries whose sampling coordinate is this close to an integer are left out (the kink)


@functools.lru_cache(maxsize=None)
def _wino_legs(shape, spread, seed=0):
    """the six Winograd-domain legs of the whole layer emulated in float32 on the case's own tensors (gradient maps from the
    float64 reference): {leg: (c, S_tile)}"""
    c = make_case(shape, False, spread, seed)
    k, C, H, W = c["k"], c["C"], c["H"], c["W"]
    r = layer_reference(c)
    out = {}
    for half, xp, w, dG in ((1, r["sp"], c["w0"][:, C:], r["dGs"]), (0, r["tp"], c["w0"][:, :C], r["dh"])):
        Ho, Wo = dG.shape[2:]
        Hp, Wp = xp.shape[2:]
        wf = w.flip(2, 3).transpose(0, 1)
        St = wn_conv_stile(xp, w, Ho, Wo, k)
        out["fwd", half] = (measure_c((wn_conv(xp, w, Ho, Wo, k, torch.float32).double() - F.conv2d(xp, w)).abs(), St), St)
        zl = z_lin(dG, k)
        St = wn_conv_stile(zl, wf, Hp, Wp, k)
        out["dgrad", half] = (measure_c((wn_conv(zl, wf, Hp, Wp, k, torch.float32).double() - dgrad_pad(dG, w, k)).abs(), St), St)
        St = wn_wgrad_stile(xp, dG, k)
        out["wgrad", half] = (measure_c((wn_wgrad(xp, dG, k, torch.float32).double() - wgrad(xp, dG, k)).abs(), St), St)
    return out


@functools.lru_cache(maxsize=None)
def layer_bars(shape, spread, mode, seed=0):
    """Reference and per-element bars of the whole layer's eight outputs in `mode`.  Every stage adds its own bar -- direct_bar
    for a float32 sum of K products, 4 c 2^-24 S_tile for a Winograd-domain leg -- to the bars of its inputs carried through
    the stage's absolute values (E(sum a_i b_i) <= sum |a_i| E(b_i) + |b_i| E(a_i) + own bar).  Also carried: the bilinear weights
    are formed in float32 from x + flow (absolute error 2 u (|x + flow| + 2) per weight); a hidden unit closer to 0 than its own
    bar may take the other slope in float32 ((1 - slope) |d act| on that entry's gradient); the fixed-point cells of the
    owner-computes scatter (2^-39 of max |d hidden| per contribution)."""
    c = make_case(shape, False, spread, seed)
    k, B, C, H, W, slope = c["k"], c["B"], c["C"], c["H"], c["W"], c["slope"]
    r = layer_reference(c)
    a, conv, KK, n = torch.abs, F.conv2d, k * k, B * H * W
    ws, wt_ = c["w0"][:, C:], c["w0"][:, :C]
    wino = _wino_legs(shape, spread, seed) if mode in (4, 5) or (mode == 1 and k == 5) else {}
    cs = {}

    def leg_bar(leg, half, S, K, x=None, w=None, cv=None, dG=None):
        if is_wino(mode, k, leg):
            cc, St = wino[leg, half]
            cs[leg, half] = cc
            lo = 0.0
            if is_wino16(mode, k, leg, both=True):
                lo = (wn16_conv_lo(x, w, S.shape[2], S.shape[3], k, x, c["w0"]) if leg == "fwd" else wn16_wgrad_lo(x, dG, k, x, dG))
            if leg == "wgrad":
                lo = lo + x_rounding(mode, S)
            return WINO_MARGIN * cc * U * St + lo + (2.0 * (KK + 2) * U * S if leg == "dgrad" else 0.0)
        return direct_bar(S, K, mode, x, w, cv)

    S_Gs, S_Gt = conv(a(r["sp"]), a(ws)), conv(a(r["tp"]), a(wt_))
    E_Gs = leg_bar("fwd", 1, S_Gs, C * KK, r["sp"], ws, conv)
    E_Gt = leg_bar("fwd", 0, S_Gt, C * KK, r["tp"], wt_, conv)
    idx, wa = r["idx"], [a(w) for w in r["wts"]]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    dx, dy = c["f"][:, 0] + xs, c["f"][:, 1] + ys
    w_err = (2.0 * U * (a(dx) + a(dy) + 2.0)).reshape(B, 1, -1)
    ones = [torch.ones_like(w) for w in wa]
    corner_sum = lambda X: sample_map(X, idx, ones, H, W)
    A_Gs = corner_sum(a(r["Gs"]))
    S_h = a(c["b0"]).reshape(1, -1, 1, 1) + S_Gt + sample_map(S_Gs, idx, wa, H, W)
    E_h = E_Gt + sample_map(E_Gs, idx, wa, H, W) + w_err.reshape(B, 1, H, W) * A_Gs + 16.0 * U * S_h
    E_act = E_h + U * S_h
    S_l = torch.einsum("qo,bohw->bqhw", a(c["w1"]), S_h) + a(c["b1"]).reshape(1, -1, 1, 1)
    bar = {"logits": torch.einsum("qo,bohw->bqhw", a(c["w1"]), E_act) + 2.0 * (HID + 3) * U * S_l}
    # backward
    S_ga = torch.einsum("qo,bqhw->bohw", a(c["w1"]), a(c["up"]))
    flip = (a(r["hidden"]) <= E_h).double()
    E_dh = 2.0 * (KK + 3) * U * S_ga + flip * (1.0 - slope) * S_ga
    bar["g_b1"] = 2.0 * (n + 2) * U * a(c["up"]).sum((0, 2, 3))
    bar["g_w1"] = torch.einsum("bohw,bqhw->qo", E_act, a(c["up"])) + 2.0 * (n + 2) * U * torch.einsum("bohw,bqhw->qo", S_h, a(c["up"]))
    bar["g_b0"] = E_dh.sum((0, 2, 3)) + 2.0 * (n + 2) * U * a(r["dh"]).sum((0, 2, 3))
    ho, wo = H + k - 1, W + k - 1
    S_dGs = scatter_map(a(r["dh"]), idx, wa, ho, wo)
    n_cell = scatter_map(torch.ones(B, 1, H, W, dtype=torch.float64), idx, ones, ho, wo)
    amax = float(a(r["dh"]).max())
    cell = 2.0 ** (torch.floor(torch.log2(torch.tensor(amax, dtype=torch.float64))).item() - 39) if amax > 0 else 0.0
    E_dGs = (scatter_map(E_dh, idx, wa, ho, wo) + scatter_map(a(r["dh"]), idx, [w_err.expand_as(w) for w in wa], ho, wo) +
             2.0 * (n_cell + 2) * U * S_dGs + n_cell * cell)
    S_f = (a(r["dh"]) * A_Gs).sum(1)
    E_f = ((E_dh * A_Gs).sum(1) + (a(r["dh"]) * corner_sum(E_Gs)).sum(1) + 2.0 * (6 * HID + 4) * U * S_f +
           w_err.reshape(B, H, W) * S_f)
    bar["g_f"] = torch.stack((E_f, E_f), 1)
    near = lambda v: (v - torch.round(v)).abs() < FLOW_EPS
    excl = (near(dx) | near(dy))[:, None].expand(B, 2, H, W)
    g = {}
    for half, xp, w, dG, E_dG, key in ((1, r["sp"], ws, r["dGs"], E_dGs, "g_s"), (0, r["tp"], wt_, r["dh"], E_dh, "g_t")):
        wf = w.flip(2, 3).transpose(0, 1)
        zp = F.pad(dG, (k - 1,) * 4)
        S_xp = conv(a(zp), a(wf))
        E = conv(F.pad(E_dG, (k - 1,) * 4), a(wf)) + leg_bar("dgrad", half, S_xp, HID * KK + KK, zp, wf, conv)
        bar[key] = fold(E, k, half, H, W)
        S_w = wgrad(a(xp), a(dG), k)
        nt = B * dG.shape[2] * dG.shape[3]
        E = wgrad(a(xp), E_dG, k) + leg_bar("wgrad", half, S_w, nt, x=xp, dG=dG)
        if mode in (1, 2, 3, 5) and not is_wino(mode, k, "wgrad"):
            E = E + 2.0 ** -39 * (pow2_ceil(a(xp).max()) * a(dG).sum((0, 2, 3)).reshape(-1, 1, 1, 1) +
                                  pow2_ceil(a(dG).max()) * wgrad(a(xp), torch.ones_like(dG), k))
        g[half] = E
    bar["g_w0"] = torch.cat((g[0], g[1]), 1)
    ref = {n_: r[n_] for n_ in ("logits", "g_s", "g_t", "g_f", "g_w0", "g_b0", "g_w1", "g_b1")}
    return dict(case=c, ref=ref, bar=bar, flow_excluded=excl, c=cs, full=r, flips=int(flip.sum()))
