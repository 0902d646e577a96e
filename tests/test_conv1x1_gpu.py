"""The 1x1 convolutions on the GPU (gen_conv.conv1x1, Conv1x1Function; csrc/conv1x1.hip and the KW = 1 instantiation of
csrc/gen_conv_wgrad.hip): the forward and all three gradients of every case against the float64 host truth with the bars
derived in conv1x1_util, every element checked; then reproducibility, the uninitialised grad_x, the untouched default,
autocast, the whole discriminator against its unrewritten float32 and float64 copies, and a training step of the
discriminator and of a widening generator block with no vendor convolution and no vendor pooling."""
import pytest
import torch
import torch.nn.functional as F

import conv1x1_util as cu
import discriminator_util as du
import gen_conv_util as gu

pytestmark = pytest.mark.gpu


def _run(gfla, name, shape, opts, needs=(True, True, True)):
    """conv1x1(..., grad="kernels") forward and backward on fresh leaves: (y, grad_x, grad_w, grad_b)"""
    (x, w, b), g = cu.leaves(name, shape, cu.key(opts), needs=needs)
    y = gfla.conv1x1(x, w, b, pre_slope=opts.get("slope"), pool=opts.get("pool", 1), grad="kernels")
    assert type(y.grad_fn).__name__ == "Conv1x1FunctionBackward"
    y.backward(g)
    return y.detach(), x.grad, w.grad, None if b is None else b.grad


def _check(name, shape, opts, got, label=""):
    want, limits = cu.truth(name, shape, cu.key(opts)), cu.bars(name, shape, cu.key(opts))
    worst = []
    for q, mine in zip(("y", "gx", "gw", "gb"), got):
        if want[q] is None:
            assert mine is None
            continue
        assert mine.shape == want[q].shape and torch.isfinite(mine).all(), q
        err = (mine.cpu().double() - want[q]).abs()
        worst.append((q, err.max().item(), (err / limits[q].clamp_min(1e-300)).max().item(), bool((err <= limits[q]).all())))
    print("conv1x1 %s%s %s %s: " % (label, name, shape, opts) + ", ".join("%s max err %.3e err/bar %.3f" % w3[:3] for w3 in worst))
    assert all(w3[3] for w3 in worst), worst


@pytest.mark.parametrize("name,shape,opts", cu.CASES, ids=gu.case_id)
def test_forward_and_gradients(gfla, name, shape, opts):
    dtype = gu.DTYPES[name]
    got = _run(gfla, name, shape, opts)
    assert got[0].dtype == got[1].dtype == dtype and got[2].dtype == torch.float32
    assert got[0].shape == (shape[0], shape[2]) + cu.out_size(shape[3], shape[4], opts.get("pool", 1))
    _check(name, shape, opts, got)
    (x, w, b), _ = cu.leaves(name, shape, cu.key(opts))
    with torch.no_grad():                             # the forward is the inference launch, bit for bit
        assert torch.equal(got[0], gfla.conv1x1(x, w, b, pre_slope=opts.get("slope"), pool=opts.get("pool", 1)))
    if shape[3] % 2 and opts.get("pool") == 2:        # the dropped row and column get no gradient: exactly zero
        assert not got[1][:, :, shape[3] - 1, :].any() and not got[1][:, :, :, shape[4] - 1].any()
    if opts.get("slope") is not None:                 # act'(0) = slope at the planted zeros, 1 at positive entries
        assert (x == 0).any()


@pytest.mark.parametrize("name,shape,opts", [(n,) + cu.ODD for n in gu.ALL] + [("f32", (2, 20, 40, 9, 7), {"slope": 0.1})],
                         ids=gu.case_id)
def test_reproducible_and_only_what_is_asked_for(gfla, name, shape, opts):
    first, second = _run(gfla, name, shape, opts), _run(gfla, name, shape, opts)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    only_x = _run(gfla, name, shape, opts, needs=(True, False, False))
    assert only_x[2] is None and only_x[3] is None and torch.equal(only_x[1], first[1])
    only_p = _run(gfla, name, shape, opts, needs=(False, True, True))
    assert only_p[1] is None and torch.equal(only_p[2], first[2]) and torch.equal(only_p[3], first[3])
    only_b = _run(gfla, name, shape, opts, needs=(False, False, True))
    assert only_b[1] is None and only_b[2] is None and torch.equal(only_b[3], first[3])


@pytest.mark.parametrize("name", gu.ALL)
def test_grad_x_is_written_everywhere(gfla, name):
    """grad_x comes from torch.empty: with the allocator's free blocks full of NaN, the zero row and column of an odd map
    (and everything else) must be the kernel's own writes"""
    shape, opts = cu.ODD
    (x, _, _), _ = cu.leaves(name, shape, cu.key(opts))
    junk = [torch.full_like(x, float("nan")) for _ in range(16)] + [torch.full((1 << 20,), float("nan"), device="cuda")]
    torch.cuda.synchronize()
    del junk
    got = _run(gfla, name, shape, opts)
    assert torch.isfinite(got[1]).all()
    assert not got[1][:, :, shape[3] - 1, :].any() and not got[1][:, :, :, shape[4] - 1].any()
    _check(name, shape, opts, got, "after a NaN fill ")


@pytest.mark.parametrize("opts", [{"pool": 2}, {"slope": 0.1}], ids=gu.case_id)
def test_the_default_is_the_torch_composition(gfla, opts):
    shape = (2, 20, 40, 21, 19)
    pool, slope = opts.get("pool", 1), opts.get("slope")
    (x, w, b), g = cu.leaves("f32", shape, cu.key(opts))
    (x2, w2, b2), _ = cu.leaves("f32", shape, cu.key(opts))
    y = gfla.conv1x1(x, w, b, pre_slope=slope, pool=pool)
    want = F.conv2d(F.avg_pool2d(x2, 2, 2) if pool == 2 else F.leaky_relu(x2, slope), w2, b2)
    # the vendor library's own gradients are not bit-reproducible from call to call (its weight gradient differed in the
    # last bit between two identical compositions), so what is compared is the graph: torch's own nodes, nothing of ours
    chain = [type(y.grad_fn).__name__, type(y.grad_fn.next_functions[0][0]).__name__]
    assert chain == [type(want.grad_fn).__name__, type(want.grad_fn.next_functions[0][0]).__name__]
    assert chain[0] == "ConvolutionBackward0" and torch.equal(y, want)
    y.backward(g)
    assert x.grad.shape == x.shape and w.grad.shape == w.shape and b.grad.shape == b.shape
    y = gfla.conv1x1(x, w, b, pre_slope=slope, pool=pool, impl="torch", grad="kernels")
    assert type(y.grad_fn).__name__ == "ConvolutionBackward0" and torch.equal(y, want)


@pytest.mark.parametrize("opts", [{"pool": 2}, {"slope": 0.1}], ids=gu.case_id)
def test_autocast(gfla, opts):
    """float32 x and parameters under autocast: float32 gradients, and the bits of an explicit bfloat16 x outside it"""
    shape = (2, 12, 20, 11, 7)
    pool, slope = opts.get("pool", 1), opts.get("slope")
    (xa, wa, ba), _ = cu.leaves("f32", shape, cu.key(opts))
    (xd, wd, bd), _ = cu.leaves("f32", shape, cu.key(opts))
    xd = xd.detach().bfloat16().requires_grad_()
    g = cu.inputs("bf16", shape, cu.key(opts))[3].cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ya = gfla.conv1x1(xa, wa, ba, pre_slope=slope, pool=pool, grad="kernels")
    yd = gfla.conv1x1(xd, wd, bd, pre_slope=slope, pool=pool, grad="kernels")
    assert ya.dtype == yd.dtype == torch.bfloat16 and type(ya.grad_fn).__name__ == "Conv1x1FunctionBackward"
    ya.backward(g)
    yd.backward(g)
    assert xa.grad.dtype == wa.grad.dtype == ba.grad.dtype == torch.float32
    assert torch.equal(ya, yd) and torch.equal(xa.grad, xd.grad.float())
    assert torch.equal(wa.grad, wd.grad) and torch.equal(ba.grad, bd.grad)


# ---- the whole network -------------------------------------------------------------------------------------------------
def _loss(net, images):
    return (net(images[0]) + net(images[1])).square().mean()


def _pointwise_discriminator(gfla, fused):
    assert gfla.fuse_spectral_norm(fused, grad="kernels", pointwise="kernels") == 10 and not du.hooked_convs(fused)
    assert all(type(b.shortcut[0]) is torch.nn.Identity and b.shortcut[1].pool == 2 for b in fused.blocks)
    assert not any(type(m) in (torch.nn.Conv2d, torch.nn.AvgPool2d) for m in fused.modules())


def test_whole_network_parity(gfla):
    """The rule of test_spectral_norm_gpu.test_whole_network_parity with the 1x1 convolutions on the kernels as well: two
    steps of D(a), D(b), backward, SGD; outputs and every parameter's gradient of the rewritten network within 4x the
    distance of the unrewritten float32 GPU network from the float64 host network, measured here."""
    (fused, plain), host, images = du.discriminators("cuda")
    _pointwise_discriminator(gfla, fused)
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
        print("pointwise discriminator step %d: gradients, unrewritten float32 network %.3e from float64, bar %.3e, "
              "rewritten %.3e; outputs %.3e, bar %.3e, rewritten %.3e"
              % (step, measured, 4 * measured, own, out_measured, 4 * out_measured, out_own))
        assert 0 < measured < 1e-4 and 0 < out_measured < 1e-4
        assert (outs["fused"] - outs["plain"]).abs().max().item() / outs["host"].abs().max().item() <= 4 * out_measured
        for k in want:
            assert ((got[k] - base[k]).abs().max() / scale[k]).item() <= 4 * measured, (step, k)
        for (k, b), (_, c) in zip(fused.named_buffers(), host.named_buffers()):
            assert du.distance(b, c) < 1e-4, (step, k)
        for opt in opts.values():
            opt.step()


def _trap(*args, **kwargs):
    raise AssertionError("vendor library call in the training step")


_CONV_TRAPS = ((F, "conv2d"), (torch, "conv2d"), (F, "conv_transpose2d"), (torch, "conv_transpose2d"), (torch, "bmm"),
               (torch.nn.grad, "conv2d_input"), (torch.nn.grad, "conv2d_weight"))


def test_discriminator_step_behind_the_vendor_fence(gfla, monkeypatch):
    """The traps of test_spectral_norm_gpu's fence without its exemption for (1, 1) weights, and avg_pool2d trapped as
    well: a training step of the rewritten discriminator calls none of them; the network rewritten with the defaults
    trips the pooling trap."""
    (fused, default), _, images = du.discriminators("cuda")
    _pointwise_discriminator(gfla, fused)
    assert gfla.fuse_spectral_norm(default, grad="kernels") == 10
    for mod, name in _CONV_TRAPS + ((torch, "mv"), (torch, "dot"), (torch, "matmul")):
        monkeypatch.setattr(mod, name, _trap)

    def pool_trap(*args, **kwargs):
        raise AssertionError("vendor pooling call in the training step")
    # F.avg_pool2d is what nn.AvgPool2d and the torch composition call; the builtin behind it is trapped under its own name
    # as well, and under torch.avg_pool2d where a torch version has that name
    monkeypatch.setattr(F, "avg_pool2d", pool_trap)
    monkeypatch.setattr(torch._C._nn, "avg_pool2d", pool_trap)
    monkeypatch.setattr(torch, "avg_pool2d", pool_trap, raising=False)
    ims = [i.cuda() for i in images]
    _loss(fused, ims).backward()
    for key, p in fused.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, key
    with pytest.raises(AssertionError, match="vendor pooling call"):
        _loss(default, ims).backward()


def test_generator_block_behind_the_vendor_fence(gfla, monkeypatch):
    """a residual block with a learnable 1x1 shortcut: with pointwise=True a training step calls no vendor convolution;
    rewritten without it, the shortcut stays on F.conv2d and the same trap fires"""
    (fused, partly), x = cu.widening_blocks("cuda")
    assert gfla.fuse_inference_convs(fused, grad="kernels", pointwise=True) == 3
    assert gfla.fuse_inference_convs(partly, grad="kernels") == 2
    assert not any(type(m) is torch.nn.Conv2d for m in fused.modules())
    for mod, name in _CONV_TRAPS:
        monkeypatch.setattr(mod, name, _trap)
    fused(x).square().mean().backward()
    for key, p in fused.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, key
    with pytest.raises(AssertionError, match="vendor library call"):
        partly(x).square().mean().backward()
