"""Spectrally normalised generators on the GPU (spectral_norm.py; csrc/spectral_norm.hip, csrc/spectral_norm_dim1.h): the
batched op on matrices normalised along dim 1, alone and mixed with dim-0 ones, and the modules built on it.

Op parity follows tests/test_spectral_norm_gpu.py: truth is the float64 host evaluation of the op's formulas on the
permuted matrix, mapped back to the weight's storage (spectral_generator_util.truth64); the baseline is torch's own float32
hook on the GPU, on an nn.ConvTranspose2d with the same weight, u and v; the library must be within 4x the hook's distance
from the truth, that distance must be < 1e-4 and > 0, and where it is exactly 0 (u of a matrix of one row: s / |s| = +-1)
the library must be exact as well.  Then determinism and batch invariance, the launch count, NaN containment, the three new
modules against float64 within gen_conv_util.bar, the whole network against its unrewritten float32 and float64 copies, the
vendor fence and autocast."""
import pytest
import torch
import torch.nn.functional as F

import discriminator_util as du
import gen_conv_train_util as tu
import gen_conv_util as gu
import spectral_generator_util as sg

pytestmark = pytest.mark.gpu
QUANTITIES = ("u", "v", "sigma", "w_sn", "grad_w")
_DIM1 = {}


def dim1_mats():
    """the dim-1 inputs, made once and never changed"""
    if not _DIM1:
        _DIM1["mats"] = sg.all_dim1()
    return _DIM1["mats"]


def dim0_mats():
    if "dim0" not in _DIM1:
        _DIM1["dim0"] = [du.matrix_inputs(R, K, seed=R + K) for R, K in du.MATRICES]
    return _DIM1["dim0"]


def lib_run(gfla, mats, dims, iters, eps=1e-12):
    """the library on a batch of (W, u, v, G) with one dim each: one dict per matrix"""
    Ws = [W.cuda().requires_grad_() for W, _, _, _ in mats]
    us, vs = [u.cuda() for _, u, _, _ in mats], [v.cuda() for _, _, v, _ in mats]
    outs = gfla.spectral_normalize(Ws, us, vs, iters, eps, dims=dims)
    assert type(outs[0].grad_fn).__name__ == "SpectralNormFunctionBackward"
    assert all(o.dtype == torch.float32 and o.shape == W.shape and o.is_contiguous() for o, W in zip(outs, Ws))
    sigma = outs[0].grad_fn.sigma
    torch.autograd.backward(outs, [G.cuda() for _, _, _, G in mats])
    return [{"u": us[i], "v": vs[i], "sigma": sigma[i:i + 1], "w_sn": outs[i].detach(), "grad_w": Ws[i].grad}
            for i in range(len(mats))]


def check_against_hook(got, mats, dims, iters, eps=1e-12, label=""):
    for (W, u, v, G), d, mine in zip(mats, dims, got):
        want = (sg.truth64 if d else du.truth64)(W, u, v, G, iters, eps)
        base = (sg.hook_float32 if d else du.hook_float32)(W, u, v, G, iters, "cuda", eps)
        rows = W.size(d)
        for q in QUANTITIES:
            assert torch.isfinite(mine[q]).all() and torch.isfinite(want[q]).all(), q
            if iters == 0 and q in ("u", "v"):                     # eval mode: untouched
                assert torch.equal(mine[q].cpu(), (u, v)[q == "v"])
                continue
            measured, own = du.distance(base[q], want[q]), du.distance(mine[q], want[q])
            print("%s%s dim %d iterations %d %s: torch hook %.3e from float64, bar %.3e, library %.3e"
                  % (label, tuple(W.shape), d, iters, q, measured, 4 * measured, own))
            assert measured < 1e-4 and (measured > 0 or (q == "u" and rows == 1)), (q, measured)
            assert own <= 4 * measured, (tuple(W.shape), d, iters, q, own, measured)


# ---- 1. op parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 1, 2])
@pytest.mark.parametrize("which", list(range(len(sg.DIM1))) + ["mixed"],
                         ids=lambda w: w if w == "mixed" else "x".join(map(str, sg.DIM1[w])))
def test_op_parity(gfla, which, iters):
    if which == "mixed":                     # every dim-1 shape and every dim-0 matrix of the discriminator tests, interleaved
        pairs = [(m, 1) for m in dim1_mats()] + [(m, 0) for m in dim0_mats()]
        pairs = pairs[::2] + pairs[1::2]
    else:
        pairs = [(dim1_mats()[which], 1)]
    mats, dims = [m for m, _ in pairs], [d for _, d in pairs]
    check_against_hook(lib_run(gfla, mats, dims, iters), mats, dims, iters)


@pytest.mark.parametrize("iters", [1, 2])
def test_eps_clamp(gfla, iters):
    """a weight so small that both norms fall below eps = 1e-12: v = t / eps, u = s / eps, finite everywhere"""
    m = sg.dim1_inputs(5, 7, 3, seed=5, scale=1e-14)
    assert (sg.to_matrix(m[0]).double().t() @ m[1].double()).norm() < 1e-12
    check_against_hook(lib_run(gfla, [m], [1], iters), [m], [1], iters, label="eps clamp ")


# ---- 2. determinism and batch invariance ---------------------------------------------------------------------------------------
def test_determinism_and_batch_invariance(gfla):
    mats, zeros = dim1_mats(), dim0_mats()
    ragged = du.matrix_inputs(3, 5, seed=8)                       # 15 elements: what follows starts off a 16-byte boundary
    for iters in (0, 1, 2):
        first, second = lib_run(gfla, mats, [1] * len(mats), iters), lib_run(gfla, mats, [1] * len(mats), iters)
        for i, m in enumerate(mats):
            alone = lib_run(gfla, [m], [1], iters)[0]
            behind = lib_run(gfla, [ragged, m], [0, 1], iters)[1]
            for q in QUANTITIES:
                assert torch.equal(first[i][q], second[i][q]), (iters, i, q)
                assert torch.equal(first[i][q], alone[q]), (iters, i, q, "batched against alone")
                assert torch.equal(behind[q], alone[q]), (iters, i, q, "behind a ragged dim-0 neighbour")
        # a dim-0 matrix: in a mixed batch the bits of today's call (dims=None: the dim-0 entry points)
        today = lib_run(gfla, zeros, None, iters)
        mixed = lib_run(gfla, [mats[1]] + zeros + [mats[4]], [1] + [0] * len(zeros) + [1], iters)[1:-1]
        for a, b in zip(today, mixed):
            for q in QUANTITIES:
                assert torch.equal(a[q], b[q]), (iters, q, "dim 0: mixed against today's call")


# ---- 3. launch count -------------------------------------------------------------------------------------------------------------
def _normalisation_launches(gfla, decoders):
    from torch.profiler import ProfilerActivity, profile
    from global_flow_local_attention_amd import spectral_norm
    (net,), _, _ = sg.generators("cuda", copies=1, decoders=decoders)
    count = gfla.fuse_spectral_norm(net, generator=True)
    convs = [m for m in net.modules() if isinstance(m, spectral_norm._Normalized)]
    assert {c.dim for c in convs} == {0, 1}

    def forward():
        spectral_norm._normalize_all(convs, "auto")
        outs = [c.normalized_weight() for c in convs]
        assert all(o.grad_fn is not None for o in outs)
        return outs
    for _ in range(2):                                             # steady state: the table exists
        torch.autograd.backward(forward(), [torch.ones_like(c.weight_orig) for c in convs])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        outs = forward()
        torch.cuda.synchronize()
    fwd = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    grads = [torch.ones_like(c.weight_orig) for c in convs]
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        torch.autograd.backward(outs, grads)
        torch.cuda.synchronize()
    bwd = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "sn_" in e.name]
    return count, fwd, bwd


def test_launch_count_does_not_grow_with_the_network(gfla):
    n1, fwd1, bwd1 = _normalisation_launches(gfla, 1)
    n3, fwd3, bwd3 = _normalisation_launches(gfla, 3)
    print("normalisation of %d / %d convolutions: forward %s / %s, backward %s / %s" % (n1, n3, fwd1, fwd3, bwd1, bwd3))
    assert (n1, n3) == (sg.hooked_count(1), sg.hooked_count(3)) == (12, 18)
    assert all("sn_" in name for name in fwd1 + fwd3)
    # include/gfla_spectral_norm.h: 2 power_iterations + 1 forward (the hooks' one iteration), 2 backward, whatever the batch
    assert len(fwd1) == len(fwd3) == 3 and len(bwd1) == len(bwd3) == 2


# ---- 4. non-finite values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 1])
def test_a_nan_stays_in_its_matrix(gfla, iters):
    clean = [dim1_mats()[1], dim0_mats()[2], dim1_mats()[3], dim1_mats()[5]]
    dims = [1, 0, 1, 1]
    want = lib_run(gfla, clean, dims, iters)
    W, u, v, G = clean[2]
    bad = W.clone()
    bad[17, 5, 1, 2] = float("nan")
    got = lib_run(gfla, clean[:2] + [(bad, u, v, G)] + clean[3:], dims, iters)
    for i in (0, 1, 3):
        for q in QUANTITIES:
            assert torch.equal(got[i][q], want[i][q]), (i, q)
    for q in ("sigma", "w_sn", "grad_w") + (("u", "v") if iters else ()):
        assert torch.isnan(got[2][q]).all(), q


# ---- 5. the modules ----------------------------------------------------------------------------------------------------------------
def _module_case(gfla, make, geometry, shape, dtype, reflect, seed):
    """A hooked convolution holding gen_conv_util's seeded weights, rewritten by `make`; the forward with the normalised
    weight handed in (so that its gradient can be read) against the float64 composition on the weight the kernel reads:
    W_sn rounded to the map's dtype, as the packing rounds it."""
    B, Cin, Cout, H, W = shape
    slope = 0.1
    x, w, b, add = gu.conv_inputs(geometry, shape, dtype, seed=seed, with_add=True)
    g = tu.upstream(geometry, shape, dtype, seed=seed)
    mod = make(w.float(), b.float()).cuda().train()
    u0, v0 = mod.weight_u.clone(), mod.weight_v.clone()
    w_sn, = gfla.spectral_normalize([mod.weight_orig], [mod.weight_u], [mod.weight_v], 1, mod.eps, dims=[mod.dim])
    w_sn.retain_grad()
    mod.hand(w_sn)
    xg, ag = x.clone().cuda().requires_grad_(), add.clone().cuda().requires_grad_()
    return mod, (x, b, add, g, slope), (xg, ag, w_sn, u0, v0)


def _check_module(name, y, mod, host, dev, geometry, shape, dtype, reflect, with_add, packs=True):
    """packs: the kernel reads the weight packed in the map's dtype and the activated map rounded to it, as the torch
    composition hands it on (gen_conv.py); the head kernel reads the weight in float32 and keeps act(x) unrounded
    (head_conv_util.truth), so its reference activates in float64"""
    B, Cin, Cout, H, W = shape
    x, b, add, g, slope = host
    xg, ag, w_sn, u0, v0 = dev
    w_read = w_sn.detach().to(dtype) if packs else w_sn.detach()
    x = x if packs else x.double()
    y64, S = gu.ref64(geometry, x, w_read, b, reflect, slope, add if with_add else None)
    err = (y.detach().cpu().double() - y64).abs()
    limit = gu.bar(S, y64, gu.reduction_length(geometry, Cin), dtype, with_add)
    print("%s forward: max err %.3e err/bar %.3f" % (name, err.max(), (err / limit.clamp_min(1e-300)).max()))
    assert y.dtype == dtype and (err <= limit).all()
    y.backward(g.cuda())
    assert xg.grad.dtype == dtype and w_sn.grad.dtype == mod.bias.grad.dtype == mod.weight_orig.grad.dtype == torch.float32
    (gx64, gw64, gb64), (Sx, Sw, Sb) = tu.grads64(geometry, x, w_read, b, g, reflect, slope)
    for what, got, want, Sq, K, u in (
            ("grad_x", xg.grad, gx64, Sx, tu.data_reduction_length(geometry, Cout), dtype),
            ("grad_w_sn", w_sn.grad, gw64, Sw, tu.weight_reduction_length(geometry, shape), torch.float32),
            ("grad_b", mod.bias.grad, gb64, Sb, tu.weight_reduction_length(geometry, shape), torch.float32)):
        e = (got.cpu().double() - want).abs()
        limit = gu.bar(Sq, want, K, u, False)
        print("%s %s: max err %.3e err/bar %.3f" % (name, what, e.max(), (e / limit.clamp_min(1e-300)).max()))
        assert got.shape == want.shape and (e <= limit).all(), what
    if with_add:
        assert ag.grad.dtype == dtype and torch.equal(ag.grad.cpu(), g)
    # weight_orig's gradient: the normalisation's backward of the gradient that arrived, by the op-parity rule
    W0, G0 = mod.weight_orig.detach().cpu(), w_sn.grad.cpu()
    truth, hook = (sg.truth64, sg.hook_float32) if mod.dim else (du.truth64, du.hook_float32)
    if not mod.dim:
        W0, G0 = W0.reshape(W0.size(0), -1), G0.reshape(G0.size(0), -1)
    want = truth(W0, u0.cpu(), v0.cpu(), G0, 1, mod.eps)["grad_w"]
    base = hook(W0, u0.cpu(), v0.cpu(), G0, 1, "cuda", mod.eps)["grad_w"]
    measured, own = du.distance(base, want), du.distance(mod.weight_orig.grad.reshape(want.shape), want)
    print("%s grad weight_orig: torch hook %.3e from float64, bar %.3e, library %.3e" % (name, measured, 4 * measured, own))
    assert 0 < measured < 1e-4 and own <= 4 * measured


@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_transposed_conv_with_addend(gfla, name):
    """SpectralConvTranspose(x, add): the forward and all gradients against the float64 composition"""
    dtype, shape = gu.DTYPES[name], (2, 40, 24, 9, 11)

    def make(w, b):
        conv = torch.nn.utils.spectral_norm(torch.nn.ConvTranspose2d(shape[1], shape[2], 3, 2, 1, output_padding=1))
        with torch.no_grad():
            conv.weight_orig.copy_(w), conv.bias.copy_(b)
        return gfla.SpectralConvTranspose(conv, pre_slope=0.1, grad="kernels")
    mod, host, dev = _module_case(gfla, make, gu.T2K3, shape, dtype, False, seed=23)
    y = mod(dev[0], dev[1])
    assert type(y.grad_fn).__name__ == "GenConvFunctionBackward" and mod.__dict__["_handed"] is None
    _check_module("SpectralConvTranspose + add " + name, y, mod, host, dev, gu.T2K3, shape, dtype, False, True)


@pytest.mark.parametrize("name", ["f32", "bf16"])
@pytest.mark.parametrize("cout", [16, 3])
def test_reflect_padded_conv_and_narrow_head(gfla, cout, name):
    """Conv2d(k 3, p 0) behind the reflection pad: Cout 16 is a SpectralConv(padding="reflect"), Cout 3 a SpectralHead"""
    dtype, shape = gu.DTYPES[name], (2, 20, cout, 13, 7)

    def make(w, b):
        conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(shape[1], cout, 3))
        with torch.no_grad():
            conv.weight_orig.copy_(w), conv.bias.copy_(b)
        seq = torch.nn.Sequential(torch.nn.LeakyReLU(0.1), torch.nn.ReflectionPad2d(1), conv)
        assert gfla.fuse_spectral_norm(seq, grad="kernels", generator=True) == 1
        assert type(seq[2]) is (gfla.SpectralHead if cout <= 8 else gfla.SpectralConv) and seq[2].pre_slope == 0.1
        return seq[2]
    mod, host, dev = _module_case(gfla, make, gu.S1K3, shape, dtype, True, seed=29)
    if cout <= 8:
        y = mod(dev[0])
        assert type(y.grad_fn).__name__ == "HeadConv3x3FunctionBackward"
    else:
        y = mod(dev[0], dev[1])
        assert type(y.grad_fn).__name__ == "GenConvFunctionBackward"
    _check_module("reflect Cout %d %s" % (cout, name), y, mod, host, dev, gu.S1K3, shape, dtype, True, cout > 8, cout > 8)


# ---- 6. the whole network ----------------------------------------------------------------------------------------------------------
def _loss(net, images):
    return (net(images[0]) + net(images[1])).square().mean()


def test_whole_network_parity(gfla):
    """G(a), G(b), one backward, an optimizer step, and again: outputs and every parameter's gradient of the rewritten network
    (generator=True, grad="kernels", pointwise="kernels") within 4x the distance of the unrewritten float32 GPU network from
    the float64 host network."""
    (fused, plain), host, images = sg.generators("cuda")
    assert gfla.fuse_spectral_norm(fused, grad="kernels", pointwise="kernels", generator=True) == 15 and not sg.hooked(fused)
    nets = {"host": (host, [i.double() for i in images]), "plain": (plain, [i.cuda() for i in images]),
            "fused": (fused, [i.cuda() for i in images])}
    opts = {k: torch.optim.SGD(n.parameters(), lr=0.05) for k, (n, _) in nets.items()}
    for step in range(2):
        outs = {}
        for k, (net, ims) in nets.items():
            opts[k].zero_grad(set_to_none=True)
            _loss(net, ims).backward()
            outs[k] = net.eval()(ims[0]).detach().cpu().double()
            net.train()
        want = {k: p.grad for k, p in host.named_parameters()}
        base = {k: p.grad.cpu().double() for k, p in plain.named_parameters()}
        got = {k: p.grad.cpu().double() for k, p in fused.named_parameters()}
        assert set(want) == set(base) == set(got) and all(p.grad.dtype == torch.float32 for p in fused.parameters())
        top = max(w.abs().max().item() for w in want.values())
        scale = {k: w.abs().max().item() if w.abs().max().item() >= 1e-10 * top else top for k, w in want.items()}
        measured = max(((base[k] - want[k]).abs().max() / scale[k]).item() for k in want)
        own = max(((got[k] - want[k]).abs().max() / scale[k]).item() for k in want)
        out_measured, out_own = du.distance(outs["plain"], outs["host"]), du.distance(outs["fused"], outs["host"])
        print("generator step %d: gradients, unrewritten float32 network %.3e from float64, bar %.3e, rewritten %.3e; "
              "outputs %.3e, bar %.3e, rewritten %.3e" % (step, measured, 4 * measured, own, out_measured, 4 * out_measured, out_own))
        assert 0 < measured < 1e-4 and 0 < out_measured < 1e-4
        assert out_own <= 4 * out_measured
        for k in want:
            assert ((got[k] - want[k]).abs().max() / scale[k]).item() <= 4 * measured, (step, k)
        for (k, b), (_, c) in zip(fused.named_buffers(), host.named_buffers()):
            assert du.distance(b, c) < 1e-4, (step, k)
        for opt in opts.values():
            opt.step()


# ---- 7. the vendor fence -----------------------------------------------------------------------------------------------------------
def test_training_step_behind_the_vendor_fence(gfla, monkeypatch):
    """No gemv, dot, matmul, convolution or transposed convolution of a vendor library in a training step of the rewritten
    network (reflection padding itself is no vendor call); the unrewritten network trips the same trap."""
    (fused, plain), _, images = sg.generators("cuda")
    assert gfla.fuse_spectral_norm(fused, grad="kernels", pointwise="kernels", generator=True) == 15

    def trap(*args, **kwargs):
        raise AssertionError("vendor library call in the generator's training step")

    for mod, name in ((torch, "mv"), (torch, "dot"), (torch, "bmm"), (torch, "matmul"), (F, "conv2d"), (torch, "conv2d"),
                      (F, "conv_transpose2d"), (torch, "conv_transpose2d"), (torch.nn.grad, "conv2d_input"),
                      (torch.nn.grad, "conv2d_weight")):
        monkeypatch.setattr(mod, name, trap)
    ims = [i.cuda() for i in images]
    _loss(fused, ims).backward()
    for key, p in fused.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, key
    with pytest.raises(AssertionError, match="vendor library call"):
        _loss(plain, ims).backward()


# ---- 8. autocast -------------------------------------------------------------------------------------------------------------------
def test_autocast(gfla):
    """Under torch.autocast(bfloat16) parameters and their gradients stay float32, and the output is within the 16-bit bar of
    the float64 network: 30 u, u = 2^-8 -- each of the 15 convolutions rounds the weight it reads and the map it writes
    once, the errors taken as adding up, relative to the largest output of a tanh head whose slope is at most 1.  The
    unrewritten network under the same autocast is printed beside it (its hooks run their gemv in bfloat16)."""
    (fused, plain), host, images = sg.generators("cuda")
    gfla.fuse_spectral_norm(fused, grad="kernels", pointwise="kernels", generator=True)
    outs = {}
    for k, net in (("fused", fused), ("plain", plain)):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            outs[k] = net(images[0].cuda())
        outs[k].float().square().mean().backward()
    want = host(images[0].double()).detach()
    for key, p in fused.named_parameters():
        assert p.dtype == torch.float32 and p.grad is not None and p.grad.dtype == torch.float32, key
        assert torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, key
    measured, own = du.distance(outs["plain"].float(), want), du.distance(outs["fused"].float(), want)
    print("generator under autocast(bfloat16): output %s; rewritten %.3e from float64, bar %.3e; unrewritten %.3e"
          % (outs["fused"].dtype, own, 30 * 2.0 ** -8, measured))
    assert outs["fused"].dtype == torch.bfloat16 and own <= 30 * 2.0 ** -8
