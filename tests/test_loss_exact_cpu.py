"""Host side of the exact loss-side tests (tests/loss_exact_util.py, tests/test_loss_exact_gpu.py): the premises under which
the kernels' float32 arithmetic is exact on the structured inputs, the restated oracles against the project's own
(oracle.cpu_modules.max_cosine_cpu, tests/style_util.py, the op-by-op blend), and the planted bugs: a host evaluation of
each op with one defect passes the EXISTING rule (restated from the existing GPU tests) and fails the new one
(test_planted_bug asserts every row; the defects are spelled out in the docstring of tests/loss_exact_util.py):

| bug | op         | defect                                                                   | existing rule | new rule |
|-----|------------|--------------------------------------------------------------------------|---------------|----------|
| T1  | max cosine | a tie across the tile step resolves to the higher row                    | passes        | FAILS    |
| T2  | max cosine | the last valid row of the ragged tile is ignored (existing shapes)       | passes        | FAILS    |
| T3  | max cosine | on equal keys the later split unit wins                                  | passes        | FAILS    |
| G1  | Gram       | the k tail is dropped for one quiet channel                              | passes        | FAILS    |
| G2  | Gram       | a dead channel's entries of S come out +1 (its D is +tiny, not 0)        | passes        | FAILS    |
| G3  | Gram       | a quiet row of the mirrored tile is taken from the wrong tile            | passes        | FAILS    |
| M1  | mask blend | the last channel chunk (quiet) is missing from mask_p's gradient         | passes        | FAILS    |
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_exact_util as L  # noqa: E402
import style_util as su  # noqa: E402

ALL_COSINE = L.COSINE_SHAPES + L.COSINE_SHAPES_16


# ------------------------------------------------------------------------------------------------------- max cosine
@pytest.mark.parametrize("flavour", [0, 1])
@pytest.mark.parametrize("shape", ALL_COSINE, ids=str)
def test_cosine_case_premises(shape, flavour):
    from oracle.cpu_modules import max_cosine_cpu
    c = L.cosine_case(shape, flavour)
    B, C, Ns, Nt = shape
    src, tgt = c["src"], c["tgt"]
    for x in (src, tgt):
        for dt in L.DTYPES.values():            # the same numbers in all three storage types
            assert torch.equal(x.to(dt).double(), x)
        mag = x.abs()
        assert bool(((mag == 0) | ((mag >= 0.25) & (mag <= 1024))).all())
        q = (x != 0).sum(1)
        assert bool(((q == 0) | (q == 1) | (q == 4) | (q == 16)).all())
        # float32: the squared norm is exact, its root a power of two that absorbs eps
        s32 = x.float().pow(2).sum(1)
        assert torch.equal(s32.double(), x.pow(2).sum(1))
        root = s32.sqrt()
        assert torch.equal((root + 1e-8)[root > 0], root[root > 0])   # (a zero vector: dot = 0, whatever its scale)
        nz = root[root > 0].double()
        assert torch.equal(torch.log2(nz), torch.log2(nz).round()) and float(nz.min()) >= 0.25
    # float32 evaluation in the kernel's order of operations is the float64 cosine bit for bit
    cos, want, want_index = L.exact_cosine(src, tgt)
    rs = torch.where(src.float().pow(2).sum(1) > 0, 1 / (src.float().pow(2).sum(1).sqrt() + 1e-8), torch.tensor(1e8))
    rt = torch.where(tgt.float().pow(2).sum(1) > 0, 1 / (tgt.float().pow(2).sum(1).sqrt() + 1e-8), torch.tensor(1e8))
    dot32 = torch.einsum("bcs,bct->bst", src.float(), tgt.float())
    assert torch.equal(dot32.double(), torch.einsum("bcs,bct->bst", src, tgt))
    assert torch.equal(((dot32 * rs.unsqueeze(2)) * rt.unsqueeze(1)).double(), cos)
    assert torch.equal(want.float().double(), want)
    # the restated oracle against the project's: eps / norm <= 1e-8 / 0.25 = 4e-8 per factor
    ref, ref_index = max_cosine_cpu(src, tgt)
    err = float((ref - want).abs().max())
    print(shape, flavour, "restated best vs max_cosine_cpu: %.2e" % err)
    assert err <= 1e-7
    # what the case must contain
    n = c["notes"]
    rows = L.forced_rows(Ns)
    assert {p for _, p, _ in n["forced"]} == set(rows) or Nt < len(rows) + 2
    for b, p, col in n["forced"]:
        assert int(want_index[b, col]) == p and float(want[b, col]) == 1.0
        word = tgt[b, :, col].sign()
        assert not bool((src[b, :, :p].sign() == word.view(-1, 1)).all(0).any()), "forced codeword present before its row"
        if p != Ns - 1:
            later = int((src[b, :, p + 1:].sign() == word.view(-1, 1)).all(0).sum())
            assert later == len(n["repeats"][(b, p)])
            # none only where forced codewords hold every later row of its tile and of the next
            assert later >= 1 or all(r in n["forced_at"][b] for r in range(p + 1, min(Ns, (p // L.TM + 2) * L.TM)))
    edge_hits = {col for _, _, col in n["forced"]}
    assert set(L.edge_columns(Nt)) <= edge_hits
    assert n["last_row"], "no column whose best is the last source row"
    for b, col in n["last_row"]:
        assert int((cos[b, :, col] == want[b, col]).sum()) == 1 and int(want_index[b, col]) == Ns - 1
    assert n["zero_target"]
    for b, col in n["zero_target"]:
        assert float(want[b, col]) == 0.0 and int(want_index[b, col]) == 0 and float(c["up"][b, col]) == 0.0
    for b, col in n["negative"]:
        assert float(cos[b, :, col].max()) < 0 and (int((cos[b, :, col] == want[b, col]).sum()) >= 2 or Ns == 1)
    for b, col in n["second_book"]:
        assert 0.25 <= float(want[b, col]) <= 0.6875
        assert int((cos[b, :, col] == want[b, col]).sum()) >= 2 or Ns == 1
    samples = {(b + flavour) % 2 for b in range(B)}
    assert bool(n["negative"]) == (1 in samples) and (bool(n["zero_source"]) == (0 in samples) or Ns == 1)
    if Nt > 16:
        assert n["second_book"]
    tied = (cos == want.unsqueeze(1)).sum(1) >= 2
    print(shape, flavour, "columns with a tied maximum: %d of %d; rows that win: %d of %d" % (
        int(tied.sum()), tied.numel(), len({(b, int(i)) for b in range(B) for i in want_index[b]}), B * Ns))
    if Ns > 1 and Nt > 16:
        assert float(tied.double().mean()) >= 0.5


def test_cosine_cases_cover_both_flavours_and_the_second_channel_pass():
    got = {}
    for shape in ALL_COSINE:
        for flavour in (0, 1):
            n = L.cosine_case(shape, flavour)["notes"]
            got[(shape, flavour)] = (bool(n["negative"]), bool(n["zero_source"]))
    assert any(v[0] for v in got.values()) and any(v[1] for v in got.values())
    c = L.cosine_case((1, 544, 136, 136), 0)
    hits = [(b, p) for b, p, col in c["notes"]["forced"] if bool((c["tgt"][b, 512:, col] != 0).any())]
    assert len(hits) >= 8, "forced codewords hardly reach the second pass of 512 channels"


@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("shape", [(2, 32, 264, 136), (2, 20, 300, 257), (1, 7, 130, 5)], ids=str)
def test_cosine_host_reduction_without_a_bug_meets_the_new_rule(shape, split):
    c = L.cosine_case(shape, 0)
    best, index = L.cosine_host(c["src"], c["tgt"], split)
    L.cosine_new_rule(best, index, c)
    L.cosine_old_rule(best, index, c["src"], c["tgt"])


def test_cosine_gradient_oracle_is_autograd_through_the_host_oracle():
    """where no maximum is tied, torch's own routing and the explicit one agree"""
    from oracle.cpu_modules import max_cosine_cpu
    src, tgt = L.old_cosine_features((2, 12, 90), 7).double(), L.old_cosine_features((2, 12, 70), 8).double()
    s, t = src.clone().requires_grad_(), tgt.clone().requires_grad_()
    best, index = max_cosine_cpu(s, t)
    up = torch.linspace(-1, 1, 140, dtype=torch.float64).view(2, 70)
    gs, gt = torch.autograd.grad(best, (s, t), up)
    hs, ht = L.cosine_grads64(src, tgt, index, up)
    assert float((gs - hs).abs().max()) <= 1e-12 * float(gs.abs().max())
    assert float((gt - ht).abs().max()) <= 1e-12 * float(gt.abs().max())


# ------------------------------------------------------------------------------------------------------------- Gram
@pytest.mark.parametrize("shape", L.GRAM_SHAPES, ids=str)
def test_gram_case_premises(gfla, shape):
    c = L.gram_case(shape)
    B, C, H, W = shape
    e = c["e"]
    for side in ("x", "y"):
        for dt in L.DTYPES.values():
            assert torch.equal(c[side].to(dt).double(), c[side])
    assert int(e.max()) == 6 and int(e.min()) == -6 and int(e[0]) == 6 and int(e[C - 1]) == -6
    if C > 128:
        assert int(e[127]) == -6 and int(e[128]) == 6
    share = float((c["x"] != c["y"]).double().mean())
    assert 0.02 <= share <= 0.06, share
    assert not bool(c["x"][:, L.GRAM_DEAD].any()) and not bool(c["y"][:, L.GRAM_DEAD].any())
    o = L.gram_oracle(c)
    blk = slice(*L.GRAM_BLOCK)
    assert bool(o["same"][:, blk, blk].all()) and bool(o["same"][:, L.GRAM_DEAD].all())
    # the exactness budget: integer sums far below 2^24 quanta (below 2^22: two different sums also stay different after
    # the product with 1 / (N C)), and S F below 24 bits
    bud = L.gram_budget(c)
    print(shape, bud)
    assert bud["gram"] < 2 ** 22 and bud["sf"] < 2 ** 24 and bud["sf_bits_bound"] < 24
    # float32 sums in another order give the same bits
    f = c["x"].reshape(B, C, -1).float()
    g32 = f.bmm(f.transpose(1, 2))
    g32_rev = f.flip(2).bmm(f.flip(2).transpose(1, 2))
    f64 = c["x"].reshape(B, C, -1)
    assert torch.equal(g32, g32_rev) and torch.equal(g32.double(), f64.bmm(f64.transpose(1, 2)))
    # the restated oracle against tests/style_util.py
    want, d_ref, gx = su.reference(c["x"], c["y"])
    assert float((o["d"] - d_ref).abs().max()) <= 1e-12 * float(gx.abs().max())
    assert abs(o["loss"] - want) <= 1e-12 * want
    assert float((o["d"] - d_ref).abs().div(torch.maximum(o["gx"], o["gy"]).clamp_min(1e-300)).max()) <= 1e-12
    gref = su.reference_grad(c["x"], o["d"].sign())
    assert float((L.gram_grad_oracle(c, o["d"]) - gref).abs().max()) <= 1e-12 * float(gref.abs().max())
    # what the existing entry bar leaves unexamined on these inputs
    nonzero = o["d"] != 0
    under = (o["d"].abs() <= 2e-6 * gx.abs().max()) & nonzero
    print(shape, "non-zero entries of D under the existing bar 2e-6 max|G|: %.1f %%" % (100 * float(under.sum()) / float(nonzero.sum())))
    # the host evaluation without a bug meets the new rule in every storage type
    for dt in L.DTYPES.values():
        scale = 1.0 if dt == torch.float32 else 2.0 ** 16
        loss, d, grad = L.gram_host(c, dt, grad_scale=scale)
        L.gram_new_rule(c, loss, d, grad, dt, grad_scale=scale)
    # the chunk rule, through the workspace size
    lib = gfla._lib.lib()
    assert lib.gfla_gram_l1_workspace_bytes(B, C, H * W) == L.gram_workspace_bytes(B, C, H * W)


def test_gram_chunked_shape_has_two_chunks():
    B, C, H, W = L.GRAM_CHUNKED
    assert B == 1 and L.gram_chunks(B, C, H * W)[1] >= 2
    assert all(L.gram_chunks(*s[:2], s[2] * s[3])[1] == 1 for s in L.GRAM_SHAPES if s != L.GRAM_CHUNKED)
    assert (1, 136, 1, 321) in L.GRAM_SHAPES and 321 > 256 and 321 % 4 and 321 % 8


# ------------------------------------------------------------------------------------------------------- mask blend
@pytest.mark.parametrize("shape", L.BLEND_SHAPES, ids=str)
def test_blend_case_premises(shape):
    c = L.blend_case(shape)
    exact = L.blend_steps(*c["leaves"])
    for t in c["leaves"][:3] + (c["up"],):
        assert float((t / (2.0 ** c["e"].double()).view(1, -1, 1, 1)).abs().max()) <= 3 and int(c["e"].abs().max()) <= 3
    for m in c["leaves"][3:]:
        assert set(m.unique().tolist()) <= {0.0, 0.25, 0.5, 1.0}
    for dt in L.DTYPES.values():
        steps = L.blend_steps(*[t.to(dt) for t in c["leaves"]])
        for i, (got, want) in enumerate(zip(steps, exact)):
            assert got.dtype == dt and torch.equal(got.double(), want), (dt, i)
        assert torch.equal(c["up"].to(dt).double(), c["up"])
        y, grads = L.blend_host(c, dt)
        L.blend_new_rule(c, y, grads, dt)
        L.blend_old_rule(c, y, grads, dt)
    bud = L.blend_budget(c)
    print(shape, "largest channel sum of a mask gradient: %.0f quanta (2^%.1f)" % (bud, torch.log2(torch.tensor(bud)).item()))
    assert bud < 2 ** 24
    # the five gradients of the exact expression are exact in float64 and, but for the masks', in every storage type
    _, want_g = L.blend_oracle(c)
    for g in want_g[:3]:
        for dt in L.DTYPES.values():
            assert torch.equal(g.to(dt).double(), g)
    assert torch.equal(want_g[3].float().double(), want_g[3]) and torch.equal(want_g[4].float().double(), want_g[4])


# ------------------------------------------------------------------------------------------------------- planted bugs
T2_SHAPES = [(1, 48, 1023, 515), (2, 7, 130, 5), (2, 32, 264, 136)]


def _passes(fn):
    try:
        fn()
        return True
    except AssertionError as err:
        print("   fails:", str(err)[:160])
        return False


def _cosine_bug(bug):
    shape, split = ((2, 32, 264, 136), 1) if bug != "T3" else ((2, 20, 300, 257), 3)
    c = L.cosine_case(shape, 0)
    good = L.cosine_host(c["src"], c["tgt"], split)
    bad = L.cosine_host(c["src"], c["tgt"], split, bug)
    assert not (torch.equal(good[0], bad[0]) and torch.equal(good[1], bad[1])), "the planted bug changes nothing"
    new = _passes(lambda: L.cosine_new_rule(bad[0], bad[1], c))
    if bug == "T2":     # the existing rule on the existing generators and shapes
        old = True
        for shp in T2_SHAPES:
            B, C, Ns, Nt = shp
            src, tgt = L.old_cosine_features((B, C, Ns), 1).double(), L.old_cosine_features((B, C, Nt), 2).double()
            _, _, first = L.exact_cosine(src, tgt)
            assert not bool((first == Ns - 1).any()), "a target's best is the last source row"
            b2 = L.cosine_host(src, tgt, 1, bug)
            old = old and _passes(lambda: L.cosine_old_rule(b2[0], b2[1], src, tgt))
    else:
        old = _passes(lambda: L.cosine_old_rule(bad[0], bad[1], c["src"], c["tgt"]))
    return old, new


def _gram_bug(bug):
    c = L.gram_case((1, 136, 1, 321), twin=(bug == "G3"))
    olds, news = [], []
    for dt in L.DTYPES.values():
        scale = 1.0 if dt == torch.float32 else 2.0 ** 16
        good = L.gram_host(c, dt, None, scale)
        L.gram_new_rule(c, *good, dt, grad_scale=scale)
        share = L.gram_old_rule(c, *good, dt, grad_scale=scale)
        bad = L.gram_host(c, dt, bug, scale)
        assert not torch.equal(good[1], bad[1]), "the planted bug changes nothing"
        olds.append(_passes(lambda: L.gram_old_rule(c, *bad, dt, grad_scale=scale)))
        news.append(_passes(lambda: L.gram_new_rule(c, *bad, dt, grad_scale=scale)))
    print("   share of the entries of D inside the existing sign mask: %.3f (its cap: 1e-3)" % share)
    return all(olds), any(news)


def _blend_bug(bug):
    c = L.blend_case((1, 130, 5, 33))
    olds, news = [], []
    for dt in (torch.bfloat16, torch.float16):      # the existing rule holds the mask gradients to 2^-6 of the top there
        good, bad = L.blend_host(c, dt), L.blend_host(c, dt, bug)
        assert not torch.equal(good[1][3], bad[1][3]), "the planted bug changes nothing"
        olds.append(_passes(lambda: L.blend_old_rule(c, *bad, dt)))
        news.append(_passes(lambda: L.blend_new_rule(c, *bad, dt)))
    return all(olds), any(news)


@pytest.mark.parametrize("bug", ["T1", "T2", "T3", "G1", "G2", "G3", "M1"])
def test_planted_bug(bug):
    old, new = {"T": _cosine_bug, "G": _gram_bug, "M": _blend_bug}[bug[0]](bug)
    print("%s: existing rule %s, new rule %s" % (bug, "passes" if old else "FAILS", "passes" if new else "FAILS"))
    assert old, "the existing rule already sees %s" % bug
    assert not new, "the new rule does not see %s" % bug
