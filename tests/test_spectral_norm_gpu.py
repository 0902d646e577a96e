"""The batched spectral norm on the GPU (spectral_norm.py; csrc/spectral_norm.hip) and the discriminator convolutions that
run on it.

Op parity: truth is a float64 host evaluation of the op's formulas (discriminator_util.truth64).  The bar of a quantity
(u, v, sigma, W_sn, grad W) is 4x the distance of torch's own float32 GPU hook from that truth on the same inputs, relative
to the quantity's largest float64 entry -- the rule of test_whole_network_gradient_parity; the library must be within the
bar OF THE TRUTH.  The hook's distance must be > 0 and < 1e-4, so a broken baseline cannot widen the bar; the one quantity
that float32 computes exactly, u of a matrix of one row (s / |s| = +-1), has distance 0 and the library must be exact there
too.  Then the eps clamp, determinism, the buffers, the launch count, the 4x4 stride-2 convolution with an addend, the
whole network against its unrewritten float32 and float64 copies, the vendor fence and autocast.  The figures measured on
an MI355X are in DESIGN.md, "Spectral norm"."""
import copy

import pytest
import torch
import torch.nn.functional as F

import discriminator_util as du
import gen_conv_train_util as tu
import gen_conv_util as gu

pytestmark = pytest.mark.gpu
QUANTITIES = ("u", "v", "sigma", "w_sn", "grad_w")


def lib_run(gfla, mats, iters, eps=1e-12):
    """the library on a batch of (W, u, v, G): one dict per matrix, and the batch's tensors"""
    Ws = [W.cuda().requires_grad_() for W, _, _, _ in mats]
    us, vs = [u.cuda() for _, u, _, _ in mats], [v.cuda() for _, _, v, _ in mats]
    outs = gfla.spectral_normalize(Ws, us, vs, iters, eps)
    assert type(outs[0].grad_fn).__name__ == "SpectralNormFunctionBackward"
    assert all(o.dtype == torch.float32 and o.shape == W.shape for o, W in zip(outs, Ws))
    sigma = outs[0].grad_fn.sigma
    torch.autograd.backward(outs, [G.cuda() for _, _, _, G in mats])
    return [{"u": us[i], "v": vs[i], "sigma": sigma[i:i + 1], "w_sn": outs[i].detach(), "grad_w": Ws[i].grad}
            for i in range(len(mats))]


def check_against_hook(gfla, mats, iters, eps=1e-12, label=""):
    got = lib_run(gfla, mats, iters, eps)
    for (W, u, v, G), mine in zip(mats, got):
        want = du.truth64(W, u, v, G, iters, eps)
        base = du.hook_float32(W, u, v, G, iters, "cuda", eps)
        for q in QUANTITIES:
            assert torch.isfinite(mine[q]).all() and torch.isfinite(want[q]).all(), q
            if iters == 0 and q in ("u", "v"):                     # eval mode: untouched
                assert torch.equal(mine[q].cpu(), (u, v)[q == "v"])
                continue
            measured, own = du.distance(base[q], want[q]), du.distance(mine[q], want[q])
            print("%s%s iterations %d %s: torch hook %.3e from float64, bar %.3e, library %.3e"
                  % (label, tuple(W.shape), iters, q, measured, 4 * measured, own))
            assert measured < 1e-4 and (measured > 0 or (q == "u" and W.size(0) == 1)), (q, measured)
            assert own <= 4 * measured, (tuple(W.shape), iters, q, own, measured)


def _mats():
    return [du.matrix_inputs(R, K, seed=R + K) for R, K in du.MATRICES]


@pytest.mark.parametrize("iters", [0, 1, 2])
@pytest.mark.parametrize("which", list(range(len(du.MATRICES))) + ["all"], ids=lambda w: "all" if w == "all" else "%dx%d" % du.MATRICES[w])
def test_op_parity(gfla, which, iters):
    mats = _mats()
    check_against_hook(gfla, mats if which == "all" else [mats[which]], iters)


@pytest.mark.parametrize("iters", [1, 2])
def test_eps_clamp(gfla, iters):
    """a weight so small that both norms fall below eps = 1e-12: v = t / eps, u = s / eps, finite everywhere"""
    W, u, v, G = du.matrix_inputs(7, 45, seed=5, scale=1e-14)
    want = du.truth64(W, u, v, G, 1)
    assert (W.double().t() @ u.double()).norm() < 1e-12 and want["u"].norm() < 1e-2 and want["v"].norm() < 0.5
    check_against_hook(gfla, [(W, u, v, G)], iters, label="eps clamp ")


def test_determinism_and_batch_invariance(gfla):
    mats = _mats()
    for iters in (0, 1, 2):
        first, second = lib_run(gfla, mats, iters), lib_run(gfla, mats, iters)
        singles = [lib_run(gfla, [m], iters)[0] for m in mats]
        for a, b, c in zip(first, second, singles):
            for q in QUANTITIES:
                assert torch.equal(a[q], b[q]), (iters, q)
                assert torch.equal(a[q], c[q]), (iters, q, "batched against alone")


def test_a_matrix_behind_a_ragged_one_equals_itself_alone(gfla):
    """The batch layout does not pad: behind a matrix whose R K is no multiple of 4 the next one's slice of the upstream
    gradient starts off a 16-byte boundary, and the backward's dot takes its scalar loads.  It must add as the float4 loads do
    (du.MATRICES has its only ragged matrix last, so the test above never puts one in front)."""
    ragged, whole = du.matrix_inputs(3, 5, seed=8), du.matrix_inputs(64, 512, seed=576)
    assert ragged[0].numel() % 4 != 0 and whole[0].numel() % 4 == 0
    behind, alone = lib_run(gfla, [ragged, whole], 1)[1], lib_run(gfla, [whole], 1)[0]
    for q in QUANTITIES:
        assert torch.equal(behind[q], alone[q]), q


def test_buffers_in_place_and_eval_untouched(gfla):
    W, u, v, _ = du.matrix_inputs(32, 27, seed=9)
    W, u, v = W.cuda(), u.cuda(), v.cuda()
    u0, v0, pu, pv = u.clone(), v.clone(), u.data_ptr(), v.data_ptr()
    gfla.spectral_normalize([W], [u], [v], 0)
    assert torch.equal(u, u0) and torch.equal(v, v0)
    gfla.spectral_normalize([W], [u], [v], 1)
    assert (u.data_ptr(), v.data_ptr()) == (pu, pv) and not torch.equal(u, u0) and not torch.equal(v, v0)
    (net,), _, images = du.discriminators("cuda", copies=1)
    assert gfla.fuse_spectral_norm(net) == 10
    before = {k: (b.data_ptr(), b.clone()) for k, b in net.named_buffers()}
    net.eval()
    with torch.no_grad():
        net(images[0].cuda())
    assert all(torch.equal(b, before[k][1]) for k, b in net.named_buffers())
    net.train()
    net(images[0].cuda())
    for k, b in net.named_buffers():                 # (u of the one-row final convolution is +-1 before and after)
        assert b.data_ptr() == before[k][0] and (b.numel() == 1 or not torch.equal(b, before[k][1])), k


def _normalisation_launches(gfla, widths):
    from torch.profiler import ProfilerActivity, profile
    from global_flow_local_attention_amd import spectral_norm
    (net,), _, _ = du.discriminators("cuda", copies=1, widths=widths)
    count = gfla.fuse_spectral_norm(net)
    convs = [m for m in net.modules() if type(m) is gfla.SpectralConv]
    for _ in range(2):                                             # steady state: the table exists
        spectral_norm._normalize_all(convs, "auto")
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        spectral_norm._normalize_all(convs, "auto")
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return count, names


def test_launch_count_does_not_grow_with_the_network(gfla):
    n3, small = _normalisation_launches(gfla, (8, 16, 32))
    n4, large = _normalisation_launches(gfla, (8, 16, 32, 32))
    print("normalisation of %d / %d convolutions: device events %s / %s" % (n3, n4, small, large))
    assert (n3, n4) == (10, 13)
    assert 0 < len(small) == len(large) <= 3 and all("sn_" in name for name in small + large)


@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_s2k4_with_addend(gfla, name):
    """conv4x4_down(..., add=...): the forward and all four gradients against the float64 composition"""
    dtype, shape, slope = gu.DTYPES[name], (2, 40, 72, 19, 21), 0.1
    B, Cin, Cout, H, W = shape
    x, w, b, add = gu.conv_inputs(gu.S2K4, shape, dtype, seed=17, with_add=True)
    g = tu.upstream(gu.S2K4, shape, dtype, seed=17)
    xg, wg, bg, ag = [t.detach().clone().cuda().requires_grad_() for t in (x, w.float(), b.float(), add)]
    y = gfla.conv4x4_down(xg, wg, bg, pre_slope=slope, grad="kernels", add=ag)
    assert y.dtype == dtype and type(y.grad_fn).__name__ == "GenConvFunctionBackward"
    with torch.no_grad():
        assert torch.equal(y, gfla.conv4x4_down(xg, wg, bg, pre_slope=slope, add=ag))
    y64, S = gu.ref64(gu.S2K4, x, w, b, False, slope, add)
    err = (y.detach().cpu().double() - y64).abs()
    limit = gu.bar(S, y64, gu.reduction_length(gu.S2K4, Cin), dtype, True)
    print("conv4x4_down + add %s forward: max err %.3e err/bar %.3f" % (name, err.max(), (err / limit.clamp_min(1e-300)).max()))
    assert (err <= limit).all()
    y.backward(g.cuda())
    assert xg.grad.dtype == dtype and wg.grad.dtype == bg.grad.dtype == torch.float32
    assert ag.grad.dtype == dtype and torch.equal(ag.grad.cpu(), g)
    (gx64, gw64, gb64), (Sx, Sw, Sb) = tu.grads64(gu.S2K4, x, w, b, g, False, slope)
    for what, got, want, Sq, K, u in (
            ("grad_x", xg.grad, gx64, Sx, tu.data_reduction_length(gu.S2K4, Cout), dtype),
            ("grad_w", wg.grad, gw64, Sw, tu.weight_reduction_length(gu.S2K4, shape), torch.float32),
            ("grad_b", bg.grad, gb64, Sb, tu.weight_reduction_length(gu.S2K4, shape), torch.float32)):
        err = (got.cpu().double() - want).abs()
        limit = gu.bar(Sq, want, K, u, False)
        print("conv4x4_down + add %s %s: max err %.3e err/bar %.3f" % (name, what, err.max(), (err / limit.clamp_min(1e-300)).max()))
        assert got.shape == want.shape and (err <= limit).all(), what


def _loss(net, images):
    return (net(images[0]) + net(images[1])).square().mean()


def test_whole_network_parity(gfla):
    """D(a), D(b), one backward, an optimizer step, and again: outputs and every parameter's gradient of the rewritten
    network (grad="kernels") within 4x the distance of the unrewritten float32 GPU network from the float64 host network,
    as test_whole_network_gradient_parity measures it.  The second iteration runs on stepped weights (repacked) and on
    the u / v the first one left."""
    (fused, plain), host, images = du.discriminators("cuda")
    assert gfla.fuse_spectral_norm(fused, grad="kernels") == 10 and not du.hooked_convs(fused)
    nets = {"host": (host, [i.double() for i in images]), "plain": (plain, [i.cuda() for i in images]),
            "fused": (fused, [i.cuda() for i in images])}
    opts = {k: torch.optim.SGD(n.parameters(), lr=0.05) for k, (n, _) in nets.items()}
    for step in range(2):
        outs = {}
        for k, (net, ims) in nets.items():
            opts[k].zero_grad(set_to_none=True)
            loss = _loss(net, ims)
            loss.backward()
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
        print("discriminator step %d: gradients, unrewritten float32 network %.3e from float64, bar %.3e, rewritten %.3e; "
              "outputs %.3e, bar %.3e, rewritten %.3e" % (step, measured, 4 * measured, own, out_measured, 4 * out_measured, out_own))
        assert 0 < measured < 1e-4 and 0 < out_measured < 1e-4
        assert (outs["fused"] - outs["plain"]).abs().max().item() / outs["host"].abs().max().item() <= 4 * out_measured
        for k in want:
            assert ((got[k] - base[k]).abs().max() / scale[k]).item() <= 4 * measured, (step, k)
        for (k, b), (_, c) in zip(fused.named_buffers(), host.named_buffers()):
            assert du.distance(b, c) < 1e-4, (step, k)
        for opt in opts.values():
            opt.step()


def test_training_step_behind_the_vendor_fence(gfla, monkeypatch):
    """No gemv, dot, matmul or vendor convolution other than the 1x1 ones in a training step of the rewritten network; the
    unrewritten network trips the same trap (torch's hook calls torch.mv)."""
    (fused, plain), _, images = du.discriminators("cuda")
    assert gfla.fuse_spectral_norm(fused, grad="kernels") == 10
    real_conv2d = F.conv2d

    def trap(*args, **kwargs):
        raise AssertionError("vendor library call in the discriminator's training step")

    def conv2d_1x1_only(x, weight, *args, **kwargs):
        if tuple(weight.shape[2:]) != (1, 1):
            trap()
        return real_conv2d(x, weight, *args, **kwargs)

    for mod, name in ((torch, "mv"), (torch, "dot"), (torch, "bmm"), (torch, "matmul"), (F, "conv_transpose2d"),
                      (torch, "conv_transpose2d"), (torch.nn.grad, "conv2d_input"), (torch.nn.grad, "conv2d_weight")):
        monkeypatch.setattr(mod, name, trap)
    monkeypatch.setattr(F, "conv2d", conv2d_1x1_only)
    monkeypatch.setattr(torch, "conv2d", conv2d_1x1_only)
    ims = [i.cuda() for i in images]
    _loss(fused, ims).backward()
    for key, p in fused.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, key
    with pytest.raises(AssertionError, match="vendor library call"):
        _loss(plain, ims).backward()


@pytest.mark.parametrize("kernel", [3, 4])
def test_autocast(gfla, kernel):
    """Under autocast the normalised weight and weight_orig.grad stay float32, the convolution runs in bfloat16, and the
    results are those of an explicit bfloat16 input outside autocast."""
    torch.manual_seed(31)
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(12, 20, kernel, kernel - 2, 1)).cuda()
    a = gfla.SpectralConv(conv, pre_slope=0.1, grad="kernels")
    b = copy.deepcopy(a)
    g = torch.Generator().manual_seed(32)
    x = torch.randn(2, 12, 10, 7, generator=g).cuda()
    xa, xb = x.clone().requires_grad_(), x.bfloat16().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        w_sn, = gfla.spectral_normalize([a.weight_orig], [a.weight_u.clone()], [a.weight_v.clone()], 1)
        ya = a(xa)
    yb = b(xb)
    assert w_sn.dtype == torch.float32 and ya.dtype == yb.dtype == torch.bfloat16
    assert type(ya.grad_fn).__name__ == "GenConvFunctionBackward"
    up = torch.randn(ya.shape, generator=g).to(torch.bfloat16).cuda()
    ya.backward(up)
    yb.backward(up)
    assert a.weight_orig.grad.dtype == a.bias.grad.dtype == torch.float32 and xa.grad.dtype == torch.float32
    assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad.float())
    assert torch.equal(a.weight_orig.grad, b.weight_orig.grad) and torch.equal(a.bias.grad, b.bias.grad)
    assert torch.equal(a.weight_u, b.weight_u) and torch.equal(a.weight_v, b.weight_v)
