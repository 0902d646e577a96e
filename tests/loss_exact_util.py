"""Structured inputs, float64 oracles and rules for the exact loss-side tests (tests/test_loss_exact_cpu.py on the host,
tests/test_loss_exact_gpu.py on the device): `max_cosine_similarity` (csrc/max_cosine.hip), `gram_l1` (csrc/gram_l1.hip)
and `MaskBlendFunction` (csrc/mask_blend.hip).  Every input is built so that the kernel's float32 arithmetic is EXACT in
any order, so the rules below leave no element out and need no bar relative to the largest entry.

Max cosine.  Every position is a codeword (q in {1, 4, 16} channels of +-1) times 2^e, e in [-2, 10]: its norm 2^e sqrt(q) is a
power of two >= 2^-2, which absorbs the `+ 1e-8` in float32; dots are sums of at most 16 terms +-2^(es + et) <= 2^20 and
`(dot * rs) * rt` is the rational cosine bit for bit.  The rule: best == the float64 cosine and index == the FIRST maximal row.

Gram.  x = integers 0..3 times a per-channel 2^(e_c), e_c in [-6, 6].  Entry (i, j) of F F^T is an integer < 9 N times
2^(e_i + e_j): exact.  ROUNDING COUNTS, read from the kernels' text:
  * D (gram_finish_kernel, `sx = gx * inv_nc, sy = gy * inv_nc; d = sx - sy`, contraction off): the constant inv_nc =
    float(1 / (N C)) (relative d0, shared by both products), the two products (d1, d2) and the difference (d3), each
    <= u = 2^-24.  d - D = D (d0 + d3) + Gx d1 - Gy d2, and with Gx, Gy >= 0 and, say, Gx >= Gy this is at most
    (2 (Gx - Gy) + Gx + Gy) u = (3 Gx - Gy) u <= 3 u max(Gx, Gy): GRAM_D_ROUNDINGS = 3 roundings of max(|Gx|, |Gy|) AT THAT
    ENTRY.  Where N C is a power of two nothing rounds and the rule is torch.equal.
  * gradient (gram_bwd_kernel, `scale = *grad_loss * coef; grad = (T)(acc * scale)`): acc = S F is exact; coef is rounded to
    float32 once on the host, `*grad_loss * coef` is exact for the power-of-two grad_loss the tests use, `acc * scale` rounds
    once: GRAM_GRAD_ROUNDINGS = 2 roundings of that element, plus the storage half-ulp and float16's subnormal floor.
Second-order terms (u^2) are covered by the factor 1 + 2^-20 on both bars.

Mask blend.  Integers of magnitude <= 3 times 2^(e_c), |e_c| <= 3, masks in {0, 0.25, 0.5, 1}: every product and sum of the
op-by-op expression has at most 5 significant bits, and the channel sums of the mask gradients stay under 2^24 quanta, so
the forward and all five gradients equal the float64 result rounded once to the storage type.

Planted bugs (tests/test_loss_exact_cpu.py::test_planted_bug): a host evaluation with one defect each.

| bug | op          | defect                                                                          | existing rule | new rule |
|-----|-------------|---------------------------------------------------------------------------------|---------------|----------|
| T1  | max cosine  | a tie across the tile step resolves to the higher row                           | passes        | FAILS    |
| T2  | max cosine  | the last valid row of the ragged tile is ignored                                | passes (*)    | FAILS    |
| T3  | max cosine  | on equal keys the later split unit wins                                         | passes        | FAILS    |
| G1  | Gram        | the k tail (k = N - 1) is dropped for one quiet channel                         | passes        | FAILS    |
| G2  | Gram        | a dead channel's entries of D are +tiny instead of 0: its entries of S are +1   | passes        | FAILS    |
| G3  | Gram        | a quiet row of the mirrored tile (1, 0) is read from tile (0, 0)                | passes        | FAILS    |
| M1  | mask blend  | the last channel chunk (quiet channels) is missing from mask_p's gradient       | passes        | FAILS    |

(*) on the existing generators at (1, 48, 1023, 515), (2, 7, 130, 5) and (2, 32, 264, 136), where no target's best match is
the last source row; the new rule fails it on the structured case, whose last row is one column's unique best.
The existing Gram rule is restated without its cap on the share of entries inside the sign mask: the cap is a property
of the inputs alone (it says nothing about the kernel) and these inputs exceed it, which is why the existing test could
not be pointed at them.  G3 uses the `twin` variant of the Gram case: channel 7 carries twice the quiet channel 135, so
the misread row has the right signs and passes the existing sign-symmetry check."""
import functools
import math

import torch

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
U32 = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
HALF_ULP = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
HALF_SUBNORMAL = {torch.float32: 0.0, torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}

# ------------------------------------------------------------------------------------------------------- max cosine
COSINE_SHAPES = [(2, 32, 264, 136), (2, 20, 300, 257), (1, 7, 130, 5), (1, 33, 1, 200)]
COSINE_SHAPES_16 = [(1, 288, 264, 264), (1, 544, 136, 136)]
COSINE_SPLITS = (0, 1, 2, 3)
COSINE_EPS = 1e-8      # the loss's eps (PerceptualCorrectness.eps)
FORCED_ROWS = (0, 3, 4, 7, 8, 31, 32, 63, 64, 127, 128, 129, 255, 256)      # and Ns - 4, Ns - 1
EDGE_COLUMNS = (0, 31, 32, 127, 128, 255, 256)                             # and Nt - 1
TM = 128   # source rows per tile in both kernels (kTM, kTM16)
COSINE_GRAD_BAR = {torch.float32: 1e-5, torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}


def _codeword(g, C, q, must=None):
    """q channels of +-1 (channel `must` among them with +1, if given)"""
    perm = torch.randperm(C, generator=g).tolist()
    if must is not None:
        perm = [must] + [c for c in perm if c != must]
    w = torch.zeros(C, dtype=torch.float64)
    sign = torch.randint(0, 2, (q,), generator=g).double() * 2 - 1
    w[perm[:q]] = sign
    if must is not None:
        w[must] = 1.0
    return w


def _codebook(g, C, count, must=None, taken=()):
    qs = [q for q in (1, 4, 16) if q <= C]
    seen = {tuple(w.tolist()) for w in taken}
    words = []
    while len(words) < count:
        # mostly the widest codewords: C channels offer only 2 C codewords of one channel
        q = qs[int(torch.randint(0, len(qs), (1,), generator=g))] if len(words) % 4 == 3 else qs[-1]
        if must is not None and q == 1:
            q = qs[min(1, len(qs) - 1)]
        w = _codeword(g, C, q, must)
        if tuple(w.tolist()) not in seen:
            seen.add(tuple(w.tolist()))
            words.append(w)
    return words


def forced_rows(Ns):
    rows = [p for p in FORCED_ROWS + (Ns - 4, Ns - 1) if 0 <= p < Ns]
    return sorted(set(rows))


def edge_columns(Nt):
    return sorted({c for c in EDGE_COLUMNS + (Nt - 1,) if 0 <= c < Nt})


def exact_cosine(src, tgt):
    """float64 (B, Ns, Nt) cosines dot / (|s| |t|), 0 for a zero vector (0 / (0 + eps) in the reference), and per column the
    maximum and its FIRST row"""
    s, t = src.double(), tgt.double()
    dot = torch.einsum("bcs,bct->bst", s, t)
    ns, nt = s.pow(2).sum(1).sqrt(), t.pow(2).sum(1).sqrt()
    den = ns.unsqueeze(2) * nt.unsqueeze(1)
    cos = torch.where(den > 0, dot / den.clamp_min(1e-300), torch.zeros_like(dot))
    best = cos.max(dim=1).values
    rows = torch.arange(s.size(2)).view(1, -1, 1).expand_as(cos)
    index = torch.where(cos == best.unsqueeze(1), rows, torch.full_like(rows, s.size(2))).min(dim=1).values
    return cos, best, index


@functools.lru_cache(maxsize=None)
def cosine_case(shape, flavour=0):
    """(B, C, Ns, Nt) -> dict(src, tgt float64; want, want_index; notes).  Sample b has zero source vectors when
    (b + flavour) is even, and otherwise an all-negative column (every source codeword then holds channel 0 with +1 and
    the column is -e_0: its cosines are -1 / sqrt(q), the maximum -1/4 tied among all 16-channel rows)."""
    B, C, Ns, Nt = shape
    g = torch.Generator().manual_seed(1000 * C + Ns + Nt + flavour)
    src = torch.zeros(B, C, Ns, dtype=torch.float64)
    tgt = torch.zeros(B, C, Nt, dtype=torch.float64)
    notes = {"forced": [], "zero_target": [], "negative": [], "last_row": [], "second_book": [], "zero_source": [],
             "repeats": {}, "forced_at": {}}
    rows = forced_rows(Ns)
    tiles = (Ns + TM - 1) // TM
    for b in range(B):
        negative = (b + flavour) % 2 == 1
        must = 0 if negative else None
        forced = _codebook(g, C, len(rows), must)
        if C > 512:       # the 16-bit kernel's second pass of 512 channels must matter: move one channel of each into it
            for i, w in enumerate(forced):
                c_from = int(w.abs().argmax()) if must is None else int(w[1:].abs().argmax()) + 1
                c_to = 512 + (5 * i) % (C - 512)
                if w[c_to] == 0:
                    w[c_to], w[c_from] = w[c_from], 0.0
        filler = _codebook(g, C, 12, must, taken=forced)
        e_s = torch.randint(-2, 11, (Ns,), generator=g)
        word_of = [None] * Ns                      # None: filler to be drawn; ("F", i): forced codeword i
        for i, p in enumerate(rows):
            word_of[p] = ("F", i)
        for i, p in reversed(list(enumerate(rows))):   # repeats at other scales: same tile, next tile, last tile
            if p == Ns - 1:                        # (the late rows choose first: the ragged tail has few free rows)
                continue
            spots = []
            tile = p // TM
            for lo, hi in ((p + 1, min(Ns, (tile + 1) * TM)), ((tile + 1) * TM, min(Ns, (tile + 2) * TM)),
                           ((tiles - 1) * TM, Ns)):
                free = [r for r in range(max(lo, p + 1), hi) if word_of[r] is None and r not in spots]
                if free:
                    spots.append(free[int(torch.randint(0, len(free), (1,), generator=g))])
            notes["repeats"][(b, p)] = sorted(spots)
            for r in spots:
                word_of[r] = ("F", i)
                if int(e_s[r]) == int(e_s[p]):
                    e_s[r] = -2 + (int(e_s[r]) + 3) % 13
        notes["forced_at"][b] = {r for r in range(Ns) if word_of[r] is not None}
        zero_rows = []
        for r in range(Ns):
            if word_of[r] is None:
                if not negative and Ns > 1 and int(torch.randint(0, 12, (1,), generator=g)) == 0:
                    zero_rows.append(r)
                    continue
                word_of[r] = ("G", int(torch.randint(0, len(filler), (1,), generator=g)))
        for r in range(Ns):
            if word_of[r] is not None:
                kind, i = word_of[r]
                src[b, :, r] = (forced if kind == "F" else filler)[i] * 2.0 ** int(e_s[r])
        notes["zero_source"] += [(b, r) for r in zero_rows]
        # ---- targets
        e_t = torch.randint(-2, 11, (Nt,), generator=g)
        # the forced codewords, those of the ragged tail and of the tile step first; rotated by the sample
        order = sorted(range(len(rows)), key=lambda i: (rows[i] not in (Ns - 1, Ns - 4, 128, 127, 129), -rows[i]))
        turn = (5 * b) % len(order)
        order = order[turn:] + order[:turn]
        edges = edge_columns(Nt)
        others = [c for c in range(Nt) if c not in edges]
        col_word = {}
        queue = list(order)
        for n, c in enumerate(edges):              # (fewer forced codewords than edges: they go round)
            col_word[c] = ("F", queue.pop(0) if queue else order[n % len(order)])
        specials = ["zero"] + (["negative"] if negative else []) + [("F", i) for i in queue]
        for c, what in zip(others, specials):
            col_word[c] = what
        rest = [c for c in range(Nt) if c not in col_word]
        present = sorted({w for w in word_of if w is not None})
        for n, c in enumerate(rest):
            col_word[c] = "B" if n % 2 else present[int(torch.randint(0, len(present), (1,), generator=g))]
        second = []
        for c in range(Nt):
            what = col_word[c]
            if what == "zero":
                notes["zero_target"].append((b, c))
            elif what == "negative":
                tgt[b, 0, c] = -(2.0 ** int(e_t[c]))
                notes["negative"].append((b, c))
            elif what == "B":
                second.append(c)
            else:
                kind, i = what
                tgt[b, :, c] = (forced if kind == "F" else filler)[i] * 2.0 ** int(e_t[c])
                if kind == "F":
                    notes["forced"].append((b, rows[i], c))
                    if rows[i] == Ns - 1:
                        notes["last_row"].append((b, c))
        # second codebook: codewords whose best cosine against THIS sample's sources lies in [0.25, 0.6875] and is tied
        tries = 0
        while second:
            tries += 1
            assert tries < 20000, "no second-codebook word found"
            if tries % 2:     # a source codeword with some signs flipped and, every other time, one channel moved
                w = src[b, :, int(torch.randint(0, Ns, (1,), generator=g))].sign()
                on = w.nonzero().flatten()
                if len(on) == 0:
                    continue
                on = on[torch.randperm(len(on), generator=g)]
                flips = 1 if len(on) < 16 else 2 + int(torch.randint(0, 5, (1,), generator=g))
                w[on[:min(flips, len(on) - 1)]] *= -1
                off = (w == 0).nonzero().flatten()
                if tries % 4 == 1 and len(off) and len(on) > 1:
                    c_to = off[int(torch.randint(0, len(off), (1,), generator=g))]
                    w[c_to], w[on[-1]] = w[on[-1]].clone(), 0.0
            else:
                qs = [q for q in (1, 4, 16) if q <= C]
                w = _codeword(g, C, qs[int(torch.randint(0, len(qs), (1,), generator=g))])
            cos, best, _ = exact_cosine(src[b:b + 1], w.view(1, C, 1))
            ties = int((cos[0, :, 0] == best[0, 0]).sum())
            if 0.25 <= float(best) <= 0.6875 and (ties >= 2 or Ns == 1):
                c = second.pop()
                tgt[b, :, c] = w * 2.0 ** int(e_t[c])
                notes["second_book"].append((b, c))
    _, want, want_index = exact_cosine(src, tgt)
    return {"shape": shape, "src": src, "tgt": tgt, "want": want, "want_index": want_index, "notes": notes,
            "up": cosine_upstream(shape, notes)}


def cosine_upstream(shape, notes):
    """the gradient handed to `best`: small integers / 4, and 0 at the zero target vectors, whose gradient t / (0 + eps)
    is 1e8 times a unit vector: it overflows float16 and would be the scale of every other entry's bar"""
    B, _, _, Nt = shape
    g = torch.Generator().manual_seed(Nt)
    up = torch.randint(-8, 9, (B, Nt), generator=g).double() / 4
    for b, c in notes["zero_target"]:
        up[b, c] = 0.0
    return up


def cosine_grads64(src, tgt, index, up, eps=COSINE_EPS):
    """float64 autograd through the host oracle's expression (oracle.cpu_modules.max_cosine_cpu) with the maximum taken
    at `index`"""
    s, t = src.double().clone().requires_grad_(), tgt.double().clone().requires_grad_()
    s_unit = s / (s.norm(dim=1, keepdim=True) + eps)
    t_unit = t / (t.norm(dim=1, keepdim=True) + eps)
    picked = torch.gather(s_unit, 2, index.long().unsqueeze(1).expand(-1, s.size(1), -1))
    best = (picked * t_unit).sum(1)
    gs, gt = torch.autograd.grad(best, (s, t), up.double())
    return gs, gt


def cosine_new_rule(best, index, case):
    """no element left out: the values and the first maximal rows"""
    assert best.dtype == torch.float32 and tuple(best.shape) == tuple(case["want"].shape)
    assert torch.equal(best.cpu(), case["want"].float()), "best: %d of %d differ" % (
        int((best.cpu() != case["want"].float()).sum()), best.numel())
    wrong = index.cpu().long() != case["want_index"]
    assert not bool(wrong.any()), "index: %d of %d differ, first at %s" % (
        int(wrong.sum()), wrong.numel(), wrong.nonzero()[0].tolist())
    for b, c in case["notes"]["zero_target"]:
        assert best[b, c].item() == 0.0 and int(index[b, c]) == 0


def assert_close(got, want, tol, what=""):
    """tests/util.py's assert_close: max |got - want| <= tol * max(1, max |want|)"""
    scale = max(1.0, want.double().abs().max().item())
    err = (got.double() - want.double()).abs().max().item()
    assert err <= tol * scale, "%s: max abs err %.3e > %.1e * %.3g" % (what, err, tol, scale)
    return err


def cosine_old_rule(best, index, src, tgt, tol=2e-6):
    """check_best of tests/test_correctness_gpu.py and tests/test_correctness_half_gpu.py: the value against the host
    bmm / max, the index by the value it points at"""
    from oracle.cpu_modules import max_cosine_cpu
    want, _ = max_cosine_cpu(src.double(), tgt.double())
    assert_close(best, want, tol, "best")
    s = src.double() / (src.double().norm(dim=1, keepdim=True) + 1e-8)
    t = tgt.double() / (tgt.double().norm(dim=1, keepdim=True) + 1e-8)
    picked = torch.gather(s, 2, index.long().unsqueeze(1).expand(-1, s.size(1), -1))
    assert_close((picked * t).sum(1), want, tol, "value at index")
    assert int(index.min()) >= 0 and int(index.max()) < src.size(2)


def cosine_host(src, tgt, split=1, bug=None):
    """the kernel's reduction on the host in float64: first maximum inside a tile of 128 rows (strict >), tiles in order
    inside a unit, units (ranges of tiles, as max_cosine_kernel cuts them) merged with the lower row winning a tie.
    bug: "T1" a later tile wins a tie; "T2" the last valid row of a ragged tile is ignored; "T3" a later unit wins a tie."""
    cos, _, _ = exact_cosine(src, tgt)
    B, Ns, Nt = cos.shape
    tiles = (Ns + TM - 1) // TM
    split = max(1, min(split, tiles))
    best = torch.full((B, Nt), -float("inf"), dtype=torch.float64)
    index = torch.zeros(B, Nt, dtype=torch.long)
    for part in range(split):
        u_best = torch.full((B, Nt), -float("inf"), dtype=torch.float64)
        u_index = torch.zeros(B, Nt, dtype=torch.long)
        for mt in range(tiles * part // split, tiles * (part + 1) // split):
            hi = min(Ns, (mt + 1) * TM)
            if bug == "T2" and hi == Ns and Ns % TM:
                hi -= 1
            if hi <= mt * TM:
                continue
            blk = cos[:, mt * TM:hi]
            v = blk.max(dim=1).values
            rows = torch.arange(mt * TM, hi).view(1, -1, 1).expand_as(blk)
            i = torch.where(blk == v.unsqueeze(1), rows, torch.full_like(rows, Ns)).min(dim=1).values
            take = (v >= u_best) if bug == "T1" else (v > u_best)
            u_best, u_index = torch.where(take, v, u_best), torch.where(take, i, u_index)
        take = (u_best >= best) if bug == "T3" else (u_best > best)
        take = take & (u_best > -float("inf"))
        best, index = torch.where(take, u_best, best), torch.where(take, u_index, index)
    return best.float(), index.int()


def old_cosine_features(shape, seed):
    """the generator of tests/test_correctness_gpu.py (and of the non-finite list)"""
    from util import randn
    x = randn(shape, seed=seed).relu() * (1 + randn(shape[:1] + (1,) + shape[2:], seed=seed + 1).abs())
    return x.contiguous()


# ------------------------------------------------------------------------------------------------------------- Gram
GRAM_D_ROUNDINGS = 3
GRAM_GRAD_ROUNDINGS = 2
GRAM_LOSS_BAR = 2e-6
GRAM_CHUNKED = (1, 40, 8, 65)      # N = 520: 9 units of 64 k, at least 4 per chunk -> 2 chunks of 5 and 4 units at B = 1
GRAM_SHAPES = [(1, 40, 9, 7), (1, 136, 1, 321), (2, 64, 8, 8), GRAM_CHUNKED]
GRAM_BLOCK = (10, 15)              # channels identical in x and y
GRAM_DEAD = 20
GRAM_TWIN = (7, 135)               # the `twin` variant: channel 7 = 2 x channel 135 (for planted bug G3)
NUM_CU, GT = 256, 128              # kNumCU (gfla_common.h), kGT (gram_l1.hip)


def gram_chunks(B, C, N):
    """gram_chunks of csrc/gram_l1.hip: N in units of 64 k -> (units per chunk, chunks)"""
    cdiv = lambda a, b: -(-a // b)
    units, t = cdiv(N, 64), cdiv(C, GT)
    tiles = t * (t + 1) // 2
    want = cdiv(2 * NUM_CU, 2 * B * tiles)
    most = max(units // 4, 1)
    want = max(1, min(want, most))
    per = cdiv(units, want)
    return per, cdiv(units, per)


def gram_workspace_bytes(B, C, N):
    """gfla_gram_l1_workspace_bytes restated: the partial tiles of both sides and one float64 slot per finishing workgroup"""
    t = -(-C // GT)
    return 2 * B * gram_chunks(B, C, N)[1] * (t * (t + 1) // 2) * GT * GT * 4 + -(-B * C * C // 256) * 8


@functools.lru_cache(maxsize=None)
def gram_case(shape, twin=False):
    """x, y float64 (B, C, H, W) and the per-channel exponents"""
    B, C, H, W = shape
    N = H * W
    g = torch.Generator().manual_seed(C + H + W)
    e = torch.randint(-6, 7, (C,), generator=g)
    e[0], e[C - 1] = 6, -6
    if C > 128:
        e[127], e[128] = -6, 6
    xi = torch.randint(0, 4, (B, C, N), generator=g).double()
    redraw = torch.rand(B, C, N, generator=g) < 0.05
    yi = torch.where(redraw, torch.randint(0, 4, (B, C, N), generator=g).double(), xi)
    yi[:, GRAM_BLOCK[0]:GRAM_BLOCK[1]] = xi[:, GRAM_BLOCK[0]:GRAM_BLOCK[1]]
    xi[:, GRAM_DEAD], yi[:, GRAM_DEAD] = 0.0, 0.0
    # the last k of the quiet last channel differs between x and y: a dropped k tail there changes D
    xi[:, C - 1, N - 1], yi[:, C - 1, N - 1] = 1.0, 2.0
    if twin:
        lo, hi = GRAM_TWIN
        assert C > hi
        # a sparse quiet channel (entries 0 / 1, the same in x and y but for the last k) and its double in tile 0
        # wherever it is 1 no channel differs between x and y: D[7, i] comes from the last k alone
        sparse = (torch.rand(B, N, generator=g) < 0.1).double()
        yi = torch.where(sparse.unsqueeze(1) > 0, xi, yi)
        xi[:, hi], yi[:, hi] = sparse, sparse.clone()
        xi[:, hi, N - 1], yi[:, hi, N - 1] = 1.0, 0.0
        xi[:, lo], yi[:, lo] = xi[:, hi], yi[:, hi]
        e[hi], e[lo] = -6, -5
    scale = (2.0 ** e.double()).view(1, C, 1)
    return {"shape": shape, "x": (xi * scale).reshape(B, C, H, W), "y": (yi * scale).reshape(B, C, H, W), "e": e,
            "xi": xi, "yi": yi}


def gram_oracle(case):
    """float64: Gx, Gy, D (exact rationals rounded once), the integer sums, and the exactness budget"""
    B, C, H, W = case["shape"]
    N = H * W
    e = case["e"].double()
    ix, iy = case["xi"].bmm(case["xi"].transpose(1, 2)), case["yi"].bmm(case["yi"].transpose(1, 2))   # exact integers
    pair = (2.0 ** (e.view(C, 1) + e.view(1, C))).unsqueeze(0)
    gx, gy = ix * pair / (N * C), iy * pair / (N * C)
    d = (ix - iy) * pair / (N * C)
    return {"gx": gx, "gy": gy, "d": d, "same": ix == iy, "max_int_sum": float(torch.maximum(ix, iy).max()),
            "loss": d.abs().mean().item()}


def gram_grad_oracle(case, d, side="x", grad_scale=1.0):
    """+-coef S F in float64 with S = sign(d); coef is the float32 the launcher passes"""
    B, C, H, W = case["shape"]
    f = case[side].reshape(B, C, H * W)
    coef = (2.0 if side == "x" else -2.0) / (float(B) * C * C * C * (H * W))
    return (coef * grad_scale * d.sign().bmm(f)).reshape(B, C, H, W)


def gram_budget(case):
    """bits the exact sums need: every integer sum of F F^T in its own quantum, and S F in the smallest quantum of F"""
    B, C, H, W = case["shape"]
    f = case["x"].reshape(B, C, -1).abs()
    quantum = 2.0 ** float(case["e"].min())
    sf = max(float(case[s].reshape(B, C, -1).abs().sum(1).max()) for s in ("x", "y")) / quantum
    spread = float(case["e"].max() - case["e"].min())
    return {"gram": gram_oracle(case)["max_int_sum"], "sf": sf, "sf_bits_bound": spread + 2 + math.log2(C)}


def gram_new_rule(case, loss, diff, grad, dtype, side="x", grad_scale=1.0):
    """loss (float), diff (B, C, C) float32, grad (B, C, H, W) in `dtype` or None"""
    o = gram_oracle(case)
    B, C, H, W = case["shape"]
    diff = diff.detach().cpu()
    assert diff.dtype == torch.float32 and tuple(diff.shape) == (B, C, C)
    d = diff.double()
    assert torch.equal(diff, diff.transpose(1, 2).contiguous()), "D is not symmetric bit for bit"
    assert not bool(d[o["same"]].any()), "D is not exactly 0 where the integer sums of x and y agree"
    assert torch.equal(d.sign(), o["d"].sign()), "sign of D: %d entries differ" % int((d.sign() != o["d"].sign()).sum())
    if (H * W * C) & (H * W * C - 1) == 0:
        assert torch.equal(diff, o["d"].float()) and torch.equal(o["d"].float().double(), o["d"])
    bar = GRAM_D_ROUNDINGS * U32 * SLACK * torch.maximum(o["gx"].abs(), o["gy"].abs())
    err = (d - o["d"]).abs()
    assert bool((err <= bar).all()), "D: worst err / bar %.3g" % float((err / bar.clamp_min(1e-300)).max())
    assert abs(loss - o["loss"]) <= GRAM_LOSS_BAR * o["loss"], (loss, o["loss"])
    if grad is None:
        return
    want = gram_grad_oracle(case, o["d"], side, grad_scale)
    got = grad.detach().cpu()
    assert got.dtype == dtype and got.shape == want.shape
    got = got.double()
    assert not bool(got[want == 0].any()), "gradient is not exactly 0 where the oracle is"
    tol = GRAM_GRAD_ROUNDINGS * U32 * SLACK * want.abs()
    if dtype != torch.float32:
        tol = tol + (HALF_ULP[dtype] * want.abs()).clamp_min(HALF_SUBNORMAL[dtype])
    tol = torch.where(want == 0, torch.zeros_like(tol), tol)
    gerr = (got - want).abs()
    assert bool((gerr <= tol).all()), "gradient: worst err / bar %.3g" % float((gerr / tol.clamp_min(1e-300)).max())


def gram_old_rule(case, loss, diff, grad, dtype, grad_scale=1.0):
    """_check_forward / _check_grad of tests/test_style_loss_gpu.py ("independent" inputs) against tests/style_util.py,
    without the cap on the share of entries inside the sign mask (a statement about the inputs alone)"""
    import style_util as su
    x, y = case["x"].to(dtype), case["y"].to(dtype)
    want, d_ref, gx = su.reference(x, y)
    top = gx.abs().max().item()
    d = diff.detach().cpu().double()
    assert (d - d_ref).abs().max().item() <= 2e-6 * top, "entry bar"
    assert abs(loss - want) <= 2e-6 * abs(want), "loss bar"
    unclear = d_ref.abs() <= 2e-6 * gx.abs().max()
    s_kernel = d.sign()
    assert torch.equal(s_kernel[~unclear], d_ref.sign()[~unclear]), "sign outside the mask"
    assert torch.equal(s_kernel, s_kernel.transpose(1, 2)), "sign symmetry"
    sign = torch.where(unclear, s_kernel, d_ref.sign())
    gwant = su.reference_grad(x, sign) * grad_scale
    gtop = gwant.abs().max().item()
    err = (grad.detach().cpu().double() - gwant).abs()
    tol = 1e-5 * gtop + (HALF_ULP[dtype] * gwant.abs()).clamp_min(HALF_SUBNORMAL[dtype])
    assert bool((err <= tol).all()), "gradient bar"
    return float(unclear.double().mean())


def gram_host(case, dtype=torch.float32, bug=None, grad_scale=1.0):
    """the kernels' result on the host with every sum exact (float64) and the roundings of the finishing kernel applied
    in float32: (loss, D float32, d/dx in `dtype`).  bug: "G1", "G2", "G3" of the module docstring."""
    B, C, H, W = case["shape"]
    N = H * W
    fx, fy = case["x"].reshape(B, C, N), case["y"].reshape(B, C, N)
    quiet = C - 1

    def gram(f):
        g = f.bmm(f.transpose(1, 2))
        if bug == "G1":      # channel `quiet` without its last k, as row and as column
            tail = f[:, quiet, N - 1:N] * f[:, :, N - 1]             # (B, C)
            g[:, quiet, :] -= tail
            g[:, :, quiet] -= tail
            g[:, quiet, quiet] += tail[:, quiet]
        return g.float()     # exact: integers below 2^24 quanta
    inv = torch.tensor(1.0 / (float(N) * C), dtype=torch.float32)
    d = gram(fx) * inv - gram(fy) * inv
    if bug == "G2":
        d[:, GRAM_DEAD, :] = 2.0 ** -120
        d[:, :, GRAM_DEAD] = 2.0 ** -120
    if bug == "G3":          # row `quiet` of the mirrored tile (1, 0): tile (0, 0) at the same local coordinates
        assert quiet >= GT
        d[:, quiet, :GT] = d[:, :GT, quiet - GT]
    loss = d.double().abs().mean().item()
    coef = torch.tensor(2.0 / (float(B) * C * C * C * N), dtype=torch.float32) * torch.tensor(grad_scale, dtype=torch.float32)
    acc = d.double().sign().bmm(fx).float()
    grad = (acc * coef).to(dtype).reshape(B, C, H, W)
    return loss, d, grad


# ------------------------------------------------------------------------------------------------------- mask blend
BLEND_SHAPES = [(1, 130, 5, 33), (2, 20, 9, 7)]
BLEND_NAMES = ("out", "attn_p", "attn_r", "mask_p", "mask_r")
BLEND_CHUNK = 16     # kBlendChunk


@functools.lru_cache(maxsize=None)
def blend_case(shape):
    """float64 leaves (out, attn_p, attn_r, mask_p, mask_r) and the upstream gradient.  Channels of the last chunk of 16
    are the quietest (2^-3), in the features and in the upstream gradient."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(C + H + W)
    e = torch.randint(-3, 4, (C,), generator=g)
    e[0] = 3
    e[(C - 1) // BLEND_CHUNK * BLEND_CHUNK:] = -3
    scale = (2.0 ** e.double()).view(1, C, 1, 1)
    ints = lambda: torch.randint(-3, 4, (B, C, H, W), generator=g).double()
    levels = torch.tensor([0.0, 0.25, 0.5, 1.0], dtype=torch.float64)
    mask = lambda: levels[torch.randint(0, 4, (B, 1, H, W), generator=g)]
    leaves = (ints() * scale, ints() * scale, ints() * scale, mask(), mask())
    return {"shape": shape, "leaves": leaves, "up": ints() * scale, "e": e}


def blend_steps(out, a_p, a_r, m_p, m_r):
    """generator.py:496-499 op by op: every intermediate torch rounds, in order"""
    n_p, n_r = 1 - m_p, 1 - m_r
    o_p, o_r, b_p, b_r = out * n_p, out * n_r, a_p * m_p, a_r * m_r
    s_p, s_r = o_p + b_p, o_r + b_r
    return [n_p, n_r, o_p, o_r, b_p, b_r, s_p, s_r, s_p + s_r]


def blend_oracle(case):
    """float64: the forward and the five gradients"""
    leaves = [t.clone().requires_grad_() for t in case["leaves"]]
    y = blend_steps(*leaves)[-1]
    grads = torch.autograd.grad(y, leaves, case["up"])
    return y.detach(), list(grads)


def blend_budget(case):
    """quanta the largest channel sum of a mask gradient needs (sum of |terms| over the smallest term's quantum)"""
    out, a_p, a_r, _, _ = case["leaves"]
    quantum = 2.0 ** (2 * float(case["e"].min()))
    return max(float((case["up"] * (a - out)).abs().sum(1).max()) for a in (a_p, a_r)) / quantum


def blend_new_rule(case, y, grads, dtype):
    want_y, want_g = blend_oracle(case)
    assert y.dtype == dtype and torch.equal(y.detach().cpu(), want_y.to(dtype)), "forward"
    for g, w, name in zip(grads, want_g, BLEND_NAMES):
        assert g.dtype == dtype and torch.equal(g.detach().cpu(), w.to(dtype)), "gradient of %s: %d of %d differ" % (
            name, int((g.detach().cpu() != w.to(dtype)).sum()), w.numel())


def blend_old_rule(case, y, grads, dtype):
    """test_mask_blend_kernel_equals_op_by_op of tests/test_face_step_gpu.py: the op-by-op expression and its autograd in
    the storage type; forward bit for bit, gradients within 1e-5 (float32) or 2^-6 (16-bit) of the largest entry"""
    leaves = [t.to(dtype).requires_grad_() for t in case["leaves"]]
    want = blend_steps(*leaves)[-1]
    want.backward(case["up"].to(dtype))
    assert torch.equal(y.detach().cpu(), want.detach())
    tol = 1e-5 if dtype == torch.float32 else 2 ** -6
    for g, t, name in zip(grads, leaves, BLEND_NAMES):
        w = t.grad.float()
        assert (g.detach().cpu().float() - w).abs().max().item() <= tol * max(1e-30, w.abs().max().item()), name


def blend_host(case, dtype, bug=None):
    """the kernels' result on the host: exact sums, one rounding to the storage type.  bug "M1": the last chunk of 16
    channels is missing from mask_p's gradient."""
    y, grads = blend_oracle(case)
    if bug == "M1":
        out, a_p = case["leaves"][0], case["leaves"][1]
        C = out.size(1)
        last = (C - 1) // BLEND_CHUNK * BLEND_CHUNK
        grads[3] = grads[3] - (case["up"] * (a_p - out))[:, last:].sum(1, keepdim=True)
    return y.to(dtype), [g.to(dtype) for g in grads]
