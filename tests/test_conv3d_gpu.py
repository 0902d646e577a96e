"""The frames-major 3-D convolutions on the GPU (conv3d.conv3d_frames, Conv3dFramesFunction, avg_pool_frames; csrc/conv3d.hip,
the windowed instantiations of csrc/conv_igemm.h and csrc/gen_conv_wgrad.hip, csrc/avg_pool_frames.hip): the forward and all
gradients of every case against the float64 host F.conv3d / F.avg_pool3d with the bars derived in conv3d_util, every element
checked; then bit reproducibility and the addend aliasing the output, non-finite values, every 16-byte pointer phase inside
red zones, the whole stand-in TemporalDiscriminator against its unrewritten float32 and float64 copies, a training step
behind the vendor fence, and the one batched normalisation per forward."""
import pytest
import torch
import torch.nn.functional as F

import conv3d_util as c3
import discriminator_util as du
import gen_conv_util as gu
import placement_util as pu

pytestmark = pytest.mark.gpu


def _run(gfla, name, geometry, shape, opts, needs=(True, True, True, True)):
    """conv3d_frames(..., grad="kernels") forward and backward on fresh leaves: (y, grad_x, grad_w, grad_b, grad_add)"""
    (x, w, b, add), g = c3.leaves(name, geometry, shape, c3.key(opts), needs=needs)
    y = gfla.conv3d_frames(x, w, b, geometry=geometry, pre_slope=opts.get("slope"), add=add, grad="kernels")
    assert type(y.grad_fn).__name__ == "Conv3dFramesFunctionBackward"
    y.backward(g)
    return y.detach(), x.grad, w.grad, b.grad, None if add is None else add.grad


def _check(want, limits, got, head, names=("y", "gx", "gw", "gb")):
    worst = []
    for q, mine in zip(names, got):
        assert mine.shape == want[q].shape and torch.isfinite(mine).all(), q
        err = (mine.cpu().double() - want[q]).abs()
        worst.append((q, err.max().item(), (err / limits[q].clamp_min(1e-300)).max().item(), bool((err <= limits[q]).all())))
        if not worst[-1][3]:                              # the worst offenders: (got, truth, bar)
            at = (err / limits[q].clamp_min(1e-300)).flatten().topk(min(5, err.numel())).indices
            print("%s %s: %d of %d elements over the bar, worst %s" % (head, q, int((err > limits[q]).sum()), err.numel(), [
                (mine.cpu().double().flatten()[i].item(), want[q].flatten()[i].item(), limits[q].flatten()[i].item()) for i in at]))
    print(head + ": " + ", ".join("%s max err %.3e err/bar %.3f" % w3[:3] for w3 in worst))
    assert all(w3[3] for w3 in worst), worst


@pytest.mark.parametrize("name,geometry,shape,opts", c3.CASES, ids=c3.case_id)
def test_forward_and_gradients(gfla, name, geometry, shape, opts):
    dtype = gu.DTYPES[name]
    B, L, C, Cout, H, W = shape
    got = _run(gfla, name, geometry, shape, opts)
    lo, ho, wo = c3.out_size(geometry, L, H, W)
    assert got[0].shape == (B, lo, Cout, ho, wo) and got[0].is_contiguous()
    assert got[0].dtype == got[1].dtype == dtype and got[2].dtype == got[3].dtype == torch.float32
    assert got[2].shape == (Cout, C, 3, c3.K[geometry], c3.K[geometry])
    _check(c3.truth(name, geometry, shape, c3.key(opts)), c3.bars(name, geometry, shape, c3.key(opts)), got[:4],
           "conv3d_frames %s %s %s %s" % (geometry, name, shape, opts))
    (x, w, b, add), g = c3.leaves(name, geometry, shape, c3.key(opts))
    if add is not None:
        assert torch.equal(got[4], g)
    with torch.no_grad():                             # the forward is the inference launch, bit for bit
        assert torch.equal(got[0], gfla.conv3d_frames(x, w, b, geometry=geometry, pre_slope=opts.get("slope"), add=add))
    if opts.get("slope") is not None:
        assert (x == 0).any()


@pytest.mark.parametrize("name,shape", c3.POOL_CASES, ids=c3.case_id)
def test_pool_forward_and_backward(gfla, name, shape):
    x, g = c3.pool_inputs(name, shape)
    xg = x.cuda().requires_grad_()
    junk = [torch.full_like(xg, float("nan")) for _ in range(4)]       # grad_x comes from torch.empty: every element is the
    del junk                                                           # kernel's own write, the zero row and column too
    p = gfla.avg_pool_frames(xg, grad="kernels")
    assert type(p.grad_fn).__name__ == "AvgPoolFramesFunctionBackward" and p.dtype == x.dtype
    p.backward(g.cuda())
    t = c3.pool_truth(name, shape)
    _check(t, c3.pool_bars_of(t, x.dtype), (p.detach(), xg.grad), "avg_pool_frames %s %s" % (name, shape), ("p", "gx"))
    B, L, C, H, W = shape
    if H % 2:
        assert not xg.grad[:, :, :, H - 1, :].any()
    if W % 2:
        assert not xg.grad[:, :, :, :, W - 1].any()
    with torch.no_grad():
        assert torch.equal(gfla.avg_pool_frames(x.cuda()), p)
    again = x.cuda().requires_grad_()
    gfla.avg_pool_frames(again, grad="kernels").backward(g.cuda())
    assert torch.equal(again.grad, xg.grad)
    y = gfla.avg_pool_frames(x.cuda().requires_grad_())                # the default is the torch composition
    assert "AvgPoolFrames" not in type(y.grad_fn).__name__


# ---- bit reproducibility and in-place use ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gu.ALL)
@pytest.mark.parametrize("geometry,shape,opts", [c3.ROWS[1], c3.ROWS[5]], ids=c3.case_id)
def test_reproducible_and_only_what_is_asked_for(gfla, name, geometry, shape, opts):
    first, second = _run(gfla, name, geometry, shape, opts), _run(gfla, name, geometry, shape, opts)
    assert all(torch.equal(a, b) for a, b in zip(first[:4], second[:4]))
    only_x = _run(gfla, name, geometry, shape, opts, needs=(True, False, False, False))
    assert only_x[2] is None and only_x[3] is None and torch.equal(only_x[1], first[1])
    only_p = _run(gfla, name, geometry, shape, opts, needs=(False, True, True, False))
    assert only_p[1] is None and torch.equal(only_p[2], first[2]) and torch.equal(only_p[3], first[3])


@pytest.mark.parametrize("name", gu.ALL)
@pytest.mark.parametrize("geometry,shape,opts", [("k333", (2, 4, 20, 40, 17, 9), {"add": True}), c3.ROWS[7]], ids=c3.case_id)
def test_addend_aliasing_the_output(gfla, name, geometry, shape, opts):
    """the C entry point with the addend's buffer as the output: the bits of a separate addend"""
    from global_flow_local_attention_amd import _lib, conv3d
    x, w, b, add, _ = (t.cuda() for t in c3.inputs(name, geometry, shape, c3.key(opts)))
    with torch.no_grad():
        want = gfla.conv3d_frames(x, w, b, geometry=geometry, add=add)
    B, L, C, H, W = x.shape
    y = add.clone()
    g = conv3d.GEOMETRIES.index(geometry)
    wp = conv3d._packed(g, w, x.dtype, False)
    b32 = b.to(x.dtype).float().contiguous()
    _lib.call("gfla_conv3d_fwd_" + _lib.SUFFIX[x.dtype], x, _lib.ptr(x), _lib.ptr(wp), _lib.ptr(b32), _lib.ptr(y), _lib.ptr(y),
              B, L, C, w.size(0), H, W, g, 0, 0.0)
    assert torch.equal(y, want)


# ---- non-finite values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gu.ALL)
@pytest.mark.parametrize("geometry,shape,frame", [("k333", (2, 5, 6, 8, 6, 7), 0), ("k333", (2, 5, 6, 8, 6, 7), 2),
                                                  ("k344", (2, 6, 6, 8, 6, 7), 0), ("k344", (2, 6, 6, 8, 6, 7), 3)],
                         ids=["k333-frame0", "k333-frame2", "k344-frame0", "k344-frame3"])
def test_nan_poisons_exactly_the_windows_that_hold_it(gfla, name, geometry, shape, frame):
    """a NaN frame of x (sample 1) reaches the output samples whose window contains that frame and no others; a NaN frame of
    grad_y reaches the samples of grad_x whose adjoint window contains it.  What torch leaves finite stays finite."""
    x, w, b, _, g = (None if t is None else t.clone() for t in c3.inputs(name, geometry, shape, c3.key({})))
    B, L = shape[:2]
    lout, pt = c3.out_size(geometry, L, shape[4], shape[5])[0], c3.PADDING[geometry][0]
    x[1, frame] = float("nan")
    (xg, wg, bg), gg = [t.cuda().requires_grad_() for t in (x, w, b)], g.cuda()
    y = gfla.conv3d_frames(xg, wg, bg, geometry=geometry, grad="kernels")
    hit = [lo for lo in range(lout) if lo - pt <= frame <= lo - pt + 2]
    assert hit
    for lo in range(lout):
        assert torch.isfinite(y[0, lo]).all()
        assert torch.isnan(y[1, lo]).all() if lo in hit else torch.isfinite(y[1, lo]).all(), lo
    want = c3.torch_layout(F.conv3d(c3.torch_layout(x.double()), w.double(), b.double(), stride=c3.STRIDE[geometry],
                                    padding=c3.PADDING[geometry]))
    assert torch.equal(torch.isnan(y).cpu(), torch.isnan(want))
    # the data gradient: x finite again, a NaN frame in grad_y
    x, w, b, _, g = (None if t is None else t.clone() for t in c3.inputs(name, geometry, shape, c3.key({})))
    gframe = min(frame, lout - 1)
    g[1, gframe] = float("nan")
    xg = x.cuda().requires_grad_()
    gfla.conv3d_frames(xg, w.cuda(), b.cuda(), geometry=geometry, grad="kernels").backward(g.cuda())
    for l in range(L):
        inside = l - (2 - pt) <= gframe <= l + pt
        assert torch.isfinite(xg.grad[0, l]).all()
        assert torch.isnan(xg.grad[1, l]).all() if inside else torch.isfinite(xg.grad[1, l]).all(), l


# ---- placement ---------------------------------------------------------------------------------------------------------------
PLACED = [("k333", (2, 4, 20, 40, 17, 9), {"slope": 0.1}), ("k344", (1, 5, 16, 72, 19, 21), {"add": True})]
PLACED_PARAMS = [(n, g, s, o, p) for n in gu.ALL for g, s, o in PLACED for p in pu.placements(gu.DTYPES[n])]


@pytest.mark.parametrize("name,geometry,shape,opts,placement", PLACED_PARAMS,
                         ids=["%s-%s-%s" % (p[0], p[1], p[4]) for p in PLACED_PARAMS])
def test_conv_at_every_pointer_phase(gfla, name, geometry, shape, opts, placement):
    from global_flow_local_attention_amd import _lib
    x, w, b, add, g = c3.inputs(name, geometry, shape, c3.key(opts))

    def run(dev):
        xg, wg, bg = dev(x).requires_grad_(), dev(w).requires_grad_(), dev(b).requires_grad_()
        y = gfla.conv3d_frames(xg, wg, bg, geometry=geometry, pre_slope=opts.get("slope"),
                               add=None if add is None else dev(add), grad="kernels")
        y.backward(dev(g))
        return {"y": y.detach(), "gx": xg.grad, "gw": wg.grad, "gb": bg.grad}
    got, records, refused, _ = pu.run_placed(run, placement, "cuda", pu.package_functions(), _lib.Unsupported)
    torch.cuda.synchronize()
    assert refused is None, refused
    pu.check_zones(records)
    t = c3.truth_of(geometry, x, w, b, add, g, opts.get("slope"))
    _check(t, c3.bars_of(t, geometry, gu.DTYPES[name], shape, add is not None), [got[k] for k in ("y", "gx", "gw", "gb")],
           "placed %s conv3d_frames %s %s" % (placement, geometry, name))
    assert pu.covering(records, got["y"]) is not None and pu.covering(records, got["gx"]) is not None


POOL_PLACED = [(n, s, p) for n in gu.ALL for s in ((2, 5, 20, 21, 19), (1, 4, 8, 70, 80)) for p in pu.placements(gu.DTYPES[n])]


@pytest.mark.parametrize("name,shape,placement", POOL_PLACED, ids=["%s-%s-%s" % (p[0], "x".join(map(str, p[1])), p[2])
                                                                   for p in POOL_PLACED])
def test_pool_at_every_pointer_phase(gfla, name, shape, placement):
    """the 16-byte route and the element route give the same bits: the aligned run is the reference"""
    from global_flow_local_attention_amd import _lib
    x, g = c3.pool_inputs(name, shape)
    xa = x.cuda().requires_grad_()
    pa = gfla.avg_pool_frames(xa, grad="kernels")
    pa.backward(g.cuda())

    def run(dev):
        xg = dev(x).requires_grad_()
        p = gfla.avg_pool_frames(xg, grad="kernels")
        p.backward(dev(g))
        return {"p": p.detach(), "gx": xg.grad}
    got, records, refused, _ = pu.run_placed(run, placement, "cuda", pu.package_functions(), _lib.Unsupported)
    torch.cuda.synchronize()
    assert refused is None, refused
    pu.check_zones(records)
    t = c3.pool_truth(name, shape)
    _check(t, c3.pool_bars_of(t, x.dtype), (got["p"], got["gx"]), "placed %s avg_pool_frames %s" % (placement, name), ("p", "gx"))
    assert pu.bit_equal(got["p"], pa) and pu.bit_equal(got["gx"], xa.grad)


# ---- the whole network -------------------------------------------------------------------------------------------------
def _loss(net, videos):
    return (net(videos[0]) + net(videos[1])).square().mean()


def _rewrite(gfla, net):
    assert gfla.fuse_spectral_norm(net, grad="kernels", pointwise="kernels", temporal="kernels") == 10
    assert not c3.hooked_convs(net)
    assert not any(type(m) in (torch.nn.Conv2d, torch.nn.Conv3d, torch.nn.AvgPool2d, torch.nn.AvgPool3d) for m in net.modules())


def test_whole_network_parity(gfla):
    """The rule of test_spectral_norm_gpu / test_conv1x1_gpu: two steps of D(a), D(b), backward, SGD; outputs, every
    parameter's gradient and every buffer of the rewritten network within 4x the distance of the unrewritten float32 GPU
    network from the float64 host network, measured here and printed."""
    (fused, plain), host, videos = c3.temporal_discriminators("cuda")
    _rewrite(gfla, fused)
    nets = {"host": (host, [v.double() for v in videos]), "plain": (plain, [v.cuda() for v in videos]),
            "fused": (fused, [v.cuda() for v in videos])}
    opts = {k: torch.optim.SGD(n.parameters(), lr=0.05) for k, (n, _) in nets.items()}
    for step in range(2):
        outs = {}
        for k, (net, vids) in nets.items():
            opts[k].zero_grad(set_to_none=True)
            _loss(net, vids).backward()
            outs[k] = net.eval()(vids[0]).detach().cpu().double()
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
        buf_measured = max(du.distance(b, c) for (_, b), (_, c) in zip(plain.named_buffers(), host.named_buffers()))
        buf_own = max(du.distance(b, c) for (_, b), (_, c) in zip(fused.named_buffers(), host.named_buffers()))
        print("temporal discriminator step %d: gradients, unrewritten float32 network %.3e from float64, bar %.3e, rewritten "
              "%.3e; outputs %.3e, bar %.3e, rewritten %.3e; buffers %.3e, bar %.3e, rewritten %.3e"
              % (step, measured, 4 * measured, own, out_measured, 4 * out_measured, out_own, buf_measured, 4 * buf_measured,
                 buf_own))
        assert 0 < measured < 1e-4 and 0 < out_measured < 1e-4 and 0 < buf_measured < 1e-4
        assert out_own <= 4 * out_measured and buf_own <= 4 * buf_measured
        for k in want:
            assert ((got[k] - want[k]).abs().max() / scale[k]).item() <= 4 * measured, (step, k)
        for opt in opts.values():
            opt.step()


def test_patched_network_runs_frames_major_with_the_same_bits(gfla):
    """the class-wide wrappers of patch_reference_discriminators (one conversion at entry, one permute copy at the exit of
    the 3-D part) against the per-block route of fuse_spectral_norm: the same kernels on the same values"""
    import types
    Block3D, Net = c3.standin_classes()
    gfla.patch_reference_discriminators(types.SimpleNamespace(TemporalDiscriminator=Net),
                                        types.SimpleNamespace(ResBlock3DEncoder=Block3D), grad="kernels", pointwise="kernels",
                                        temporal="kernels")
    (per_block,), _, videos = c3.temporal_discriminators("cuda", copies=1)
    (patched,), _, _ = c3.temporal_discriminators("cuda", copies=1, cls=Net)
    _rewrite(gfla, per_block)
    assert not c3.hooked_convs(patched) and "forward" not in patched.block0.__dict__
    v = [t.cuda() for t in videos]
    ya, yb = per_block(v[0]), patched(v[0])
    assert torch.equal(ya, yb)
    ya.square().mean().backward()
    yb.square().mean().backward()
    for (k, a), (_, b) in zip(per_block.named_parameters(), patched.named_parameters()):
        assert torch.equal(a.grad, b.grad), k


def _trap(*args, **kwargs):
    raise AssertionError("vendor library call in the training step")


_TRAPS = ((F, "conv3d"), (torch, "conv3d"), (F, "avg_pool3d"), (torch._C._nn, "avg_pool3d"),
          (F, "conv2d"), (torch, "conv2d"), (F, "conv_transpose2d"), (torch, "conv_transpose2d"), (torch, "bmm"),
          (torch.nn.grad, "conv2d_input"), (torch.nn.grad, "conv2d_weight"), (torch, "mv"), (torch, "dot"), (torch, "matmul"),
          (F, "avg_pool2d"), (torch._C._nn, "avg_pool2d"))


def test_training_step_behind_the_vendor_fence(gfla, monkeypatch):
    """with every vendor convolution and pool trapped -- the 3-D ones and the 2-D traps of test_conv1x1_gpu -- a training
    step of the rewritten network completes with finite non-zero gradients on every parameter; rewritten with the defaults
    it trips the trap"""
    (fused, default), _, videos = c3.temporal_discriminators("cuda")
    _rewrite(gfla, fused)
    assert gfla.fuse_spectral_norm(default) == 4
    for mod, name in _TRAPS:
        monkeypatch.setattr(mod, name, _trap)
    monkeypatch.setattr(torch, "avg_pool2d", _trap, raising=False)
    monkeypatch.setattr(torch, "avg_pool3d", _trap, raising=False)
    vids = [v.cuda() for v in videos]
    _loss(fused, vids).backward()
    for key, p in fused.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, key
    with pytest.raises(AssertionError, match="vendor library call"):
        _loss(default, vids).backward()


def test_one_batched_normalisation_per_forward(gfla):
    """the profiler sees the launches of one batched call per forward, the 3-D weights among them: as many device events
    with the six Conv3d weights in the batch as the 2-D convolutions alone take"""
    from torch.profiler import ProfilerActivity, profile
    (fused, flat), _, videos = c3.temporal_discriminators("cuda")
    _rewrite(gfla, fused)
    assert gfla.fuse_spectral_norm(flat) == 4
    v = videos[0].cuda()
    counts = {}
    for key, net in (("fused", fused), ("flat", flat)):
        with torch.no_grad():
            for _ in range(2):                                         # steady state: the table exists
                net(v)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                net(v)
                torch.cuda.synchronize()
        counts[key] = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "sn_" in e.name]
    print("normalisation launches per forward: 10 convolutions %s, the 4 two-dimensional ones %s" % (counts["fused"], counts["flat"]))
    assert 0 < len(counts["fused"]) == len(counts["flat"]) <= 3
    normed = [m for m in fused.modules() if isinstance(m, (gfla.SpectralConv, gfla.SpectralConv3d))]
    assert len(normed) == 10 and all(m.__dict__["_handed"] is None for m in normed)
