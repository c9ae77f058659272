"""The kernels that turn logits into tokens, at their edges: csrc/sample.hip (argmax, greedy verify, tree fork and its split
form), csrc/stochastic.hip (top-k, Gumbel sampling, log-sum-exp, ratio verification, the RNG key) and the state kernels of
csrc/misc.hip (step-row store, draft advance, cache lookup).

A wrong tie-break, a column read past V or a skipped stride iteration gives no NaN and no norm error here: it gives another,
plausible token.  So every case compares integers exactly against plain torch on the CPU over the first V columns (or
oracle.ops), pads rows with hostile values (+inf / NaN, not only the -inf that hides a read past V), allocates outputs
sentinel-filled, and uses vocabularies at which the 1024-thread strided loops iterate more than once.  The distribution tests
assert on the CPU, before the kernel runs, that their bins are populated (so a badly chosen seed fails loudly)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ops as O
from tests.test_hip_stochastic import BF, H, chi2_ok, dev, rng  # noqa: F401  (H is the fixture)

INF, NAN = float("inf"), float("nan")
FILLS = (-INF, INF, NAN)
SENT = -777                       # sentinel of every integer output
NAMED = (0, 1023, 1024, 1025, 2047, 2048, 2599)      # one index in every iteration / border of a 1024-stride loop over V = 2600
V3 = 2600


def roundup8(v):
    return (v + 7) // 8 * 8


def pad_rows(x, ld, fill):
    """x [R, V] bf16 -> [R, ld] with columns [V, ld) = fill."""
    out = torch.full((x.shape[0], ld), fill, dtype=BF)
    out[:, :x.shape[1]] = x
    return out


def ints(n, dtype=torch.int64):
    return torch.full((n,) if isinstance(n, int) else tuple(n), SENT, dtype=dtype, device="cuda")


def fbits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def refuses(fn, *a, **k):
    from ssd_amd.hip.lib import SsdHipError
    with pytest.raises(SsdHipError):
        fn(*a, **k)


def same(results, what):
    """results: one tuple of CPU tensors per padding fill; all must be identical."""
    for r in results[1:]:
        for i, (u, v) in enumerate(zip(results[0], r)):
            assert torch.equal(u, v), f"{what}: output {i} depends on the padding past V"


# =====================================================================================================================
# 1. hostile padding: columns [V, ld) hold -inf, +inf or NaN; nothing may depend on them
# =====================================================================================================================
def test_hostile_padding_argmax_topk_sample_lse(H):
    torch.manual_seed(11)
    V, T = 1027, 6
    ld = roundup8(V) + 8
    x = (torch.randn(T, V) * 2).to(BF)
    x[0, V - 1] = 9.0                          # the maximum in the V % 8 tail
    x[1, 1024] = 9.0
    x[2, 1023] = 9.0                           # last body element
    want = O.argmax_rows(x)
    want_top = torch.argsort(x.float(), dim=-1, descending=True, stable=True)[:, :8].to(torch.int32)
    temps = torch.tensor([0.7, 1.3])
    want_lse = torch.logsumexp(x.double() / temps.double().repeat_interleave(3).unsqueeze(1), dim=-1)
    N = 64                                     # draws: 64 copies of row 3 under one seed and salt
    tight = dev(x[3:4].repeat(N, 1))
    d0 = ints(N)
    H.sample_rows(tight, V, N, V, dev(torch.full((N,), 0.9)), 1, rng(21), 6, d0)
    res = []
    for fill in FILLS:
        xp = dev(pad_rows(x, ld, fill))
        a, a2, ai, av = ints(T), ints(T), ints(T), torch.full((T,), NAN, device="cuda")
        H.argmax_rows(xp, ld, T, V, a, a2)
        H.argmax_rows_val(xp, ld, T, V, 0, ai, av)
        top = ints((T, 8), torch.int32)
        H.topk_rows(xp, ld, T, V, 8, top)
        g = ints(T)
        H.sample_rows(xp, ld, T, V, dev(torch.zeros(T)), 1, rng(21), 6, g)
        lse = torch.full((T,), NAN, device="cuda")
        H.row_lse(xp, ld, T, V, dev(temps), 3, lse)
        d = ints(N)
        H.sample_rows(dev(pad_rows(x[3:4].repeat(N, 1), ld, fill)), ld, N, V, dev(torch.full((N,), 0.9)), 1, rng(21), 6, d)
        res.append((a.cpu(), a2.cpu(), ai.cpu(), fbits(av), top.cpu(), g.cpu(), fbits(lse), d.cpu()))
        assert a.cpu().tolist() == want.tolist() == a2.cpu().tolist() == ai.cpu().tolist() == g.cpu().tolist(), fill
        assert torch.equal(fbits(av), fbits(x.float().max(-1).values)), fill
        assert torch.equal(top.cpu(), want_top), fill
        err = (lse.cpu().double() - want_lse).abs().max().item()
        print(f"pad {fill}: lse err {err:.2e}")
        assert err < 2e-3, fill
        assert torch.equal(d.cpu(), d0.cpu()), f"draws with ld = {ld}, pad {fill} differ from the draws with ld = V"
    same(res, "argmax / topk / sample / lse")
    assert 8 < len(set(d0.cpu().tolist())), "the draws should be spread over the vocabulary"


def test_hostile_padding_verify_ratio(H):
    torch.manual_seed(12)
    V, B, K = 1027, 48, 3
    ld_p, ld_q = roundup8(V) + 8, roundup8(V) + 16
    lp = (torch.randn(B, K + 1, V) * 1.5).to(BF)
    lq = (lp[:, :K].float() + torch.randn(B, K, V) * 0.7).to(BF)
    spec = torch.randint(0, V, (B, K + 1), dtype=torch.int64)
    spec[:, 1:] = lq.float().argmax(-1)                             # the mode of q: acceptance probabilities away from 0
    tt = torch.tensor([0.9, 0.0, 0.6])[torch.arange(B) % 3].contiguous()
    tq = torch.tensor([1.1, 0.8, 0.0, 0.5])[torch.arange(B) % 4].contiguous()
    spec[(torch.arange(B) % 5 == 0) & (tq > 0), 2] = V - 1          # a draft token in the tail (sampled drafts only: q(x) > 0)
    ratio = (torch.arange(B) % 7 != 0)
    _, _, want_ap = O.verify_full(lp, lq, spec, tt, tq, cache_hits=ratio, jit_speculate=False)
    preds_ref = O.argmax_rows(lp)
    g_acc, _ = O.verify_greedy(preds_ref, spec)
    res = []
    for fill in FILLS:
        d_lp = dev(pad_rows(lp.view(-1, V), ld_p, fill))
        d_lq = dev(pad_rows(lq.view(-1, V), ld_q, fill))
        preds = ints(B * (K + 1))
        H.argmax_rows(d_lp, ld_p, B * (K + 1), V, preds)
        lse_p, lse_q = torch.full((B * (K + 1),), NAN, device="cuda"), torch.full((B * K,), NAN, device="cuda")
        H.row_lse(d_lp, ld_p, B * (K + 1), V, dev(tt), K + 1, lse_p)
        H.row_lse(d_lq, ld_q, B * K, V, dev(tq), K, lse_q)
        acc, rec, packed = ints(B, torch.int32), ints(B), ints((B, K + 3))
        ap = torch.full((B, K), NAN, device="cuda")
        H.verify_ratio(d_lp, ld_p, d_lq, ld_q, V, B, K, dev(spec), preds, lse_p, lse_q, dev(tt), dev(tq), dev(ratio.to(torch.int32)),
                       rng(5), 2, acc, rec, packed, ap)
        res.append((preds.cpu(), fbits(lse_p), fbits(lse_q), acc.cpu(), rec.cpu(), packed.cpu(), fbits(ap)))
        assert torch.equal(preds.cpu().view(B, K + 1), preds_ref), fill
        a, r, pk = acc.cpu(), rec.cpu(), packed.cpu()
        assert bool(((a >= 0) & (a <= K)).all()) and bool(((r >= 0) & (r < V)).all()), fill
        assert torch.equal(pk[:, 0], a.long()) and torch.equal(pk[:, 1], r) and torch.equal(pk[:, 2:], spec), fill
        rows = ((tt > 0) | (tq > 0)) & ratio
        err = (ap.cpu()[rows] - want_ap[rows]).abs().max().item()
        print(f"pad {fill}: accept_prob err {err:.2e}")
        assert err < 2e-3, fill
        assert a[~rows].tolist() == g_acc[~rows].tolist(), fill
        z = tt == 0
        assert all(int(r[b]) == int(preds_ref[b, int(a[b])]) for b in range(B) if z[b]), fill
    same(res, "verify_ratio")


def fork_case(V, B, K, counts, seed, levels=4):
    """Quantised logits (ties by the thousand), a unique row maximum, and the excluded token x_{j+1} placed as the row maximum
    (j = 0), as the first element of a slice of the split form other than the maximum's (j = 1) and at V - 1 (j >= 2); the latter
    two carry the top quantised level, so they would be picked early were they not excluded."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B * (K + 1), V, generator=g) * levels).round().clamp(-levels, levels) / levels * 0.5
    top = float(x.max())
    S = (V + 4095) // 4096
    chunk = ((V // 8) + S - 1) // S * 8          # elements per slice of ssd_fork_topf_split
    returned = torch.randint(0, V, (B, K + 1), generator=g, dtype=torch.int64)
    for b in range(B):
        for j in range(K + 1):
            row = b * (K + 1) + j
            m = int(torch.randint(0, V, (1,), generator=g))
            x[row, m] = top + 1.0                # the unique maximum
            if j >= K:
                continue
            if j == 0:
                e = m
            elif j == 1:
                s = (m // chunk + 1) % S
                e = s * chunk if s * chunk != m else s * chunk + 1
                x[row, e] = top
            else:
                e = V - 1 if m != V - 1 else V - 2
                x[row, e] = top
            returned[b, j + 1] = e
    x = x.to(BF)
    cnt = torch.tensor(counts, dtype=torch.int32)
    offs = (torch.cumsum(cnt, 1) - cnt + 1 + 2 * torch.arange(K + 1)).to(torch.int32)     # gaps between the ranges: they keep the sentinel
    mq = int(offs[:, -1].max() + cnt[:, -1].max()) + 3
    want = torch.full((B, mq), SENT, dtype=torch.int64)
    ref = O.fork_topf(x.view(B, K + 1, V), returned, cnt.tolist())
    for b in range(B):
        o = 0
        for j in range(K + 1):
            c = int(cnt[b, j])
            want[b, int(offs[b, j]):int(offs[b, j]) + c] = ref[b, o:o + c]
            o += c
    return x, returned, cnt, offs, mq, want


FORK_COUNTS = [[0, 3, 15, 15], [15, 0, 3, 15]]      # fan-outs 0 and 15 in one launch; position K (no exclusion) forks 15


def test_hostile_padding_fork(H):
    B, K = 2, 3
    for V, split in ((1027, False), (1032, True)):
        ld = roundup8(V) + 8
        x, returned, cnt, offs, mq, want = fork_case(V, B, K, FORK_COUNTS, seed=V)
        for fill in FILLS:
            xp = dev(pad_rows(x, ld, fill))
            out = ints((B, mq))
            H.fork_topf(xp, ld, V, dev(returned), dev(cnt), dev(offs), B, K, mq, out)
            assert torch.equal(out.cpu(), want), (V, fill)
            if split:
                ws = torch.full((H.fork_topf_workspace_bytes(V, B, K) // 8,), -1, dtype=torch.int64, device="cuda")
                out2 = ints((B, mq))
                H.fork_topf_split(xp, ld, V, dev(returned), dev(cnt), dev(offs), B, K, mq, ws, out2)
                assert torch.equal(out2.cpu(), want), (V, fill)


# =====================================================================================================================
# 2. vocabulary geometry of the greedy kernels (exact)
# =====================================================================================================================
@pytest.mark.parametrize("V", [1, 7, 8, 9, 1023, 1025, 8192, 8203])
def test_argmax_rows_vocabulary_geometry(H, V):
    """16-byte body + V % 8 tail: V below one chunk, one full pass of the block (8 x 1024), a second pass plus a tail."""
    torch.manual_seed(V)
    body = V // 8 * 8                          # first tail index (== V when there is no tail)
    rows, pin = [], []

    def add(r, want=None):
        rows.append(r)
        pin.append(want)

    def rand():
        return torch.randn(V) * 2
    r = rand(); r[0] = 50.0; add(r, 0)
    r = rand(); r[V - 1] = 50.0; add(r, V - 1)                                   # inside the tail when V % 8
    r = rand(); r[max(body - 1, 0)] = 50.0; add(r, max(body - 1, 0))             # the last body element
    lo, hi = (body - 1, body) if 0 < body < V else (0, V - 1)                    # a tie across the body / tail border
    r = rand(); r[lo] = 50.0; r[hi] = 50.0; add(r, lo)
    if V >= 2:                                                                   # +0.0 == -0.0: the lowest index wins, whichever sign
        a, b = (lo, hi) if lo != hi else (0, 1)
        r = -rand().abs() - 1; r[a] = 0.0; r[b] = -0.0; add(r, a)
        r = -rand().abs() - 1; r[a] = -0.0; r[b] = 0.0; add(r, a)
    r = torch.full((V,), -INF); r[V - 1] = -5.0; add(r, V - 1)                   # the only finite value sits in the tail
    add(torch.full((V,), -INF), 0)                                               # all -inf: 0, as torch
    add((torch.randint(0, 5, (V,)) * 0.5 - 1.0))                                 # ties everywhere
    n_cmp = len(rows)
    add(torch.full((V,), NAN))                                                   # nothing comparable: any token in [0, V)
    x = torch.stack(rows).to(BF)
    T = x.shape[0]
    want = O.argmax_rows(x[:n_cmp])
    for i in range(n_cmp):
        assert pin[i] is None or pin[i] == int(want[i]), "the case is not what it is meant to be"
    ld = roundup8(V) + 8
    xp = dev(pad_rows(x, ld, INF))
    out, out2 = ints(T + 1), ints(T + 1)
    H.argmax_rows(xp, ld, T, V, out, out2)
    OFF = 5_000_000_000                                                          # a shard offset past 2^32
    oi, ov = ints(T + 1), torch.full((T + 1,), NAN, device="cuda")
    H.argmax_rows_val(xp, ld, T, V, OFF, oi, ov)
    o, o2, oi, ov = out.cpu(), out2.cpu(), oi.cpu(), ov.cpu()
    assert o[:n_cmp].tolist() == want.tolist()
    assert torch.equal(o, o2) and torch.equal(oi[:T], o[:T] + OFF)
    assert 0 <= int(o[T - 1]) < V, "an all-NaN row must still give a token of the vocabulary"
    assert int(o[T]) == SENT and int(oi[T]) == SENT and math.isnan(float(ov[T])), "wrote past T rows"
    picked = x[torch.arange(n_cmp), want].float()                                # the value output, by bits (incl. the sign of zero)
    assert torch.equal(fbits(ov[:n_cmp]), fbits(picked))


def test_argmax_rows_refusals(H):
    x = dev(torch.zeros(2, 16, dtype=BF))
    out, val = ints(2), torch.zeros(2, device="cuda")
    refuses(H.argmax_rows, x, 12, 2, 9, out)
    refuses(H.argmax_rows, x, 16, 0, 9, out)
    refuses(H.argmax_rows, x, 16, 2, 0, out)
    refuses(H.argmax_rows_val, x, 12, 2, 9, 0, out, val)
    refuses(H.argmax_rows_val, x, 16, 0, 9, 0, out, val)
    refuses(H.argmax_rows_val, x, 16, 2, 0, 0, out, val)
    assert out.cpu().tolist() == [SENT, SENT]


@pytest.mark.parametrize("V", [8, 1025, 2600])
@pytest.mark.parametrize("k", [1, 8])
def test_topk_rows_with_ties_everywhere(H, V, k):
    """About five distinct values per row: the k largest are decided by index alone, in every stride iteration and across them."""
    torch.manual_seed(V + k)
    T = 5
    x = torch.randint(0, 5, (T, V)) * 0.5 - 1.0
    x[0] = -1.0                                                                  # row 0: the top level only at the loop's borders
    x[0, [i for i in (V - 1, 2048, 2047, 1024, 1023, 5) if i < V]] = 1.0
    x[1] = 0.5                                                                   # row 1: one value
    x = x.to(BF)
    want = torch.argsort(x.float(), dim=-1, descending=True, stable=True)[:, :k].to(torch.int32)
    ld = V + 3
    out = ints((T + 1, k), torch.int32)
    H.topk_rows(dev(pad_rows(x, ld, INF)), ld, T, V, k, out)
    assert torch.equal(out.cpu()[:T], want)
    assert bool((out.cpu()[T] == SENT).all())


def test_topk_rows_refusals(H):
    x = dev(torch.zeros(1, 16, dtype=BF))
    out = ints((1, 9), torch.int32)
    refuses(H.topk_rows, x, 16, 1, 16, 0, out)
    refuses(H.topk_rows, x, 16, 1, 16, 9, out)
    refuses(H.topk_rows, x, 16, 1, 4, 5, out)
    assert bool((out.cpu() == SENT).all())


@pytest.mark.parametrize("V,S", [(4096, 1), (4104, 2), (12296, 4), (196608, 48)])
def test_fork_slice_geometry(H, V, S):
    """ssd_fork_topf == oracle, ssd_fork_topf_split == both: one slice, an uneven last slice at S = 2 (257 + 256 chunks), an
    uneven S = 4, and the largest vocabulary the split form takes (S = 48)."""
    B, K = 2, 3
    assert (V + 4095) // 4096 == S
    x, returned, cnt, offs, mq, want = fork_case(V, B, K, FORK_COUNTS, seed=V)
    ld = V + 8
    xp = dev(pad_rows(x, ld, INF))
    a, b_ = ints((B, mq)), ints((B, mq))
    H.fork_topf(xp, ld, V, dev(returned), dev(cnt), dev(offs), B, K, mq, a)
    nbytes = H.fork_topf_workspace_bytes(V, B, K)
    assert nbytes == B * (K + 1) * S * 16 * 8
    ws = torch.full((nbytes // 8,), -1, dtype=torch.int64, device="cuda")
    H.fork_topf_split(xp, ld, V, dev(returned), dev(cnt), dev(offs), B, K, mq, ws, b_)
    assert torch.equal(a.cpu(), want), "fork_topf"
    assert torch.equal(b_.cpu(), want), "fork_topf_split"


def test_fork_count_cap_and_refusals(H):
    """A fan-out of 16 is clamped to 15: the 15 best are written, slot offsets + 15 keeps its sentinel."""
    from ssd_amd.hip.lib import load_library
    V = 4096
    torch.manual_seed(5)
    x = (torch.randint(0, 7, (1, V)) * 0.25).to(BF)
    want = torch.argsort(x.float(), dim=-1, descending=True, stable=True)[0, :15]
    returned = torch.zeros(1, 1, dtype=torch.int64)
    cnt, offs = torch.tensor([[16]], dtype=torch.int32), torch.tensor([[1]], dtype=torch.int32)
    ws = torch.full((H.fork_topf_workspace_bytes(V, 1, 0) // 8,), -1, dtype=torch.int64, device="cuda")
    for split in (False, True):
        out = ints((1, 18))
        if split:
            H.fork_topf_split(dev(x), V, V, dev(returned), dev(cnt), dev(offs), 1, 0, 18, ws, out)
        else:
            H.fork_topf(dev(x), V, V, dev(returned), dev(cnt), dev(offs), 1, 0, 18, out)
        o = out.cpu()[0]
        assert o[1:16].tolist() == want.tolist(), split
        assert int(o[0]) == SENT and o[16:].tolist() == [SENT, SENT], split
    lib = load_library()
    assert lib.ssd_fork_topf_workspace_bytes(196616, 2, 3) < 0           # 49 slices
    assert lib.ssd_fork_topf_workspace_bytes(4100, 2, 3) < 0             # V % 8
    assert H.fork_topf_workspace_bytes(196616, 2, 3) == 0 and H.fork_topf_workspace_bytes(4100, 2, 3) == 0
    assert H.fork_topf_workspace_bytes(196608, 3, 5) == 3 * 6 * 48 * 16 * 8
    big = torch.zeros(1, 196616, dtype=BF, device="cuda")
    out = ints((1, 18))
    refuses(H.fork_topf_split, big, 196616, 196616, dev(returned), dev(cnt), dev(offs), 1, 0, 18, ws, out)
    refuses(H.fork_topf_split, big, 4104, 4100, dev(returned), dev(cnt), dev(offs), 1, 0, 18, ws, out)
    refuses(H.fork_topf_split, big, 4100, 4096, dev(returned), dev(cnt), dev(offs), 1, 0, 18, ws, out)      # ld % 8
    assert bool((out.cpu() == SENT).all())


def test_verify_greedy_at_k0_and_the_k62_cap(H):
    B = 70
    g = torch.Generator().manual_seed(62)
    for K in (0, 62):
        preds = torch.randint(0, 1000, (B, K + 1), generator=g, dtype=torch.int64)
        spec = torch.randint(0, 1000, (B, K + 1), generator=g, dtype=torch.int64)
        spec[:, 1:] = preds[:, :K]
        want_n = []
        for b in range(B):
            kind = b % 4 if K else 0
            if kind == 1:                         # a mismatch at the last lane only
                spec[b, K] += 1
            elif kind == 2:                       # at lane 0
                spec[b, 1] += 1
            elif kind == 3:                       # at two lanes: the first wins
                i = b % (K - 1)
                spec[b, 1 + i] += 1
                spec[b, 1 + min(i + 1 + b % 7, K - 1)] += 1
            want_n.append({0: K, 1: K - 1, 2: 0, 3: b % max(K - 1, 1)}[kind])
        if K:
            acc_w, rec_w = O.verify_greedy(preds, spec)
        else:                                     # no draft token (the oracle's argmax has nothing to reduce): accept 0, recover preds[b][0]
            acc_w, rec_w = torch.zeros(B, dtype=torch.int64), preds[:, 0].clone()
        assert acc_w.tolist() == want_n
        acc, rec, packed = ints(B + 1, torch.int32), ints(B + 1), ints((B + 1, K + 3))
        H.verify_greedy(dev(preds), dev(spec), B, K, acc, rec, packed)
        a, r, pk = acc.cpu(), rec.cpu(), packed.cpu()
        assert a[:B].tolist() == acc_w.tolist() and r[:B].tolist() == rec_w.tolist()
        assert torch.equal(pk[:B], torch.cat([acc_w.view(B, 1), rec_w.view(B, 1), spec], 1))
        assert int(a[B]) == SENT and int(r[B]) == SENT and bool((pk[B] == SENT).all())
    acc, rec = ints(1, torch.int32), ints(1)
    refuses(H.verify_greedy, dev(torch.zeros(1, 64, dtype=torch.int64)), dev(torch.zeros(1, 64, dtype=torch.int64)), 1, 63, acc, rec)
    refuses(H.verify_greedy, dev(torch.zeros(1, 4, dtype=torch.int64)), dev(torch.zeros(1, 4, dtype=torch.int64)), 0, 3, acc, rec)
    assert int(acc.cpu()) == SENT and int(rec.cpu()) == SENT


# =====================================================================================================================
# 3. distributions at V = 2600: every iteration of the 1024-stride loops and every wave holds probability mass
# =====================================================================================================================
def live_logits(rows, seed, n_live=40):
    """[rows, 2600] bf16: -60 everywhere but ~40 live tokens (randn * 1.5) per row; the live set holds NAMED, each with a logit at
    or above the live median."""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((rows, V3), -60.0)
    for r in range(rows):
        others = [int(i) for i in torch.randperm(V3, generator=g)[:n_live].tolist() if i not in NAMED][:n_live - len(NAMED)]
        idx = torch.tensor(list(NAMED) + others)
        val = torch.randn(len(idx), generator=g) * 1.5
        med = val.median()
        nm = val[:len(NAMED)]
        val[:len(NAMED)] = torch.where(nm < med, 2 * med - nm, nm)            # reflect the named ones above the median
        x[r, idx] = val
    return x.to(BF)


def check_bins(probs, n, what, named=NAMED, min_bins=30, max_pooled=0.01):
    """The condition a chi-square over V = 2600 needs, asserted on the CPU before the kernel runs.  (The recovery distributions of
    verify_ratio get a fraction of the draws, and the residual max(0, p - q) vanishes on about half of the live tokens: 12 bins,
    5 % pooled -- the pooled remainder is still one tested bin -- and a bin of its own in every iteration of the strided loop.)"""
    keep = probs * n >= 5
    assert int(keep.sum()) >= min_bins, f"{what}: only {int(keep.sum())} bins with an expected count >= 5"
    assert all(bool(keep[i]) for i in named), f"{what}: a named index fell into the pooled remainder"
    assert float(probs[~keep].sum()) < max_pooled, f"{what}: the pooled remainder carries {float(probs[~keep].sum()):.4f}"


SAMPLE_SEED = 7


def test_sample_rows_distribution_across_stride_iterations(H):
    V, N, T = V3, 40000, 0.8
    logits = live_logits(1, SAMPLE_SEED)[0]
    probs = torch.softmax(logits.float() / T, -1)
    boosted = O.sampler_x_rescale(probs.unsqueeze(0), 0.4, 3)[0]
    check_bins(probs, N, "sample_rows")
    check_bins(boosted, N, "sample_rows with sampler_x")
    d_rows = dev(logits.unsqueeze(0).repeat(N, 1))
    temps = dev(torch.full((N,), T))
    out, out2 = ints(N + 1), ints(N + 1)
    H.sample_rows(d_rows, V, N, V, temps, 1, rng(3), 11, out, out2)
    o = out.cpu()
    assert int(o[N]) == SENT and torch.equal(o, out2.cpu()) and bool(((o[:N] >= 0) & (o[:N] < V)).all())
    chi2_ok(torch.bincount(o[:N], minlength=V), probs, "sample_rows T=0.8 V=2600")
    # sampler_x: the 4 most probable tokens (ssd_topk_rows) scaled by 0.4
    top = ints((N, 4), torch.int32)
    H.topk_rows(d_rows, V, N, V, 4, top)
    want_top = torch.argsort(logits.float(), descending=True, stable=True)[:4].to(torch.int32)
    assert torch.equal(top.cpu()[0], want_top) and torch.equal(top[0], top[N - 1])
    outb = ints(N)
    H.sample_rows(d_rows, V, N, V, temps, 1, rng(4), 9, outb, boost_idx=top, boost_k=4, boost_x=0.4)
    chi2_ok(torch.bincount(outb.cpu(), minlength=V), boosted, "sample_rows with sampler_x V=2600")


def test_sample_rows_mixed_temperatures_in_one_launch(H):
    """rows_per_temp = 3: groups of three rows alternate between temperature 0 (== argmax, lowest index on ties) and 0.8."""
    torch.manual_seed(8)
    V, G = V3, 8
    x = torch.randint(0, 6, (3 * G, V)) * 0.5                                # ties everywhere
    x[0] = 0.0; x[0, 2599] = 3.0                                             # the maximum only in the last partial iteration
    x[1] = 0.0; x[1, [1024, 2048]] = 3.0                                     # a tie between iterations 1 and 2
    x[2] = 0.0; x[2, [1023, 1024]] = 3.0                                     # and across the border of iteration 0
    x = x.to(BF)
    temps = torch.tensor([0.0, 0.8] * (G // 2))
    out = ints(3 * G)
    H.sample_rows(dev(x), V, 3 * G, V, dev(temps), 3, rng(2), 1, out)
    o = out.cpu().view(G, 3)
    want = O.argmax_rows(x).view(G, 3)
    assert want[0].tolist() == [2599, 1024, 1023]
    assert torch.equal(o[0::2], want[0::2])
    assert bool(((o >= 0) & (o < V)).all())
    assert not torch.equal(o[1::2], want[1::2]), "temperature 0.8 rows over flat logits should not all be the argmax"


VR_SEED, VR_SEED_GREEDY_DRAFT = 6, 8     # chosen on the CPU so that the conditions asserted in check_ratio_case hold


@pytest.fixture(scope="module")
def ratio_setup():
    """One (p, q) pair of K + 1 / K live-token rows per seed, N identical sequences of it on the device (one seed at a time), shared
    by the verify_ratio cases."""
    K, N, Tt, Tq = 3, 30000, 0.9, 1.1
    cache = {}

    def get(seed):
        if seed not in cache:
            cache.clear()
            lp1 = live_logits(K + 1, seed)
            g = torch.Generator().manual_seed(seed + 100)
            live = lp1[:K].float() > -50
            lq1 = torch.where(live, lp1[:K].float() + torch.randn(K, V3, generator=g) * 0.8, lp1[:K].float()).to(BF)
            p = torch.softmax(lp1.float() / Tt, -1)
            q = torch.softmax(lq1.float() / Tq, -1)
            d_lp = dev(lp1).unsqueeze(0).expand(N, K + 1, V3).contiguous().view(N * (K + 1), V3)
            d_lq = dev(lq1).unsqueeze(0).expand(N, K, V3).contiguous().view(N * K, V3)
            cache[seed] = dict(K=K, N=N, Tt=Tt, Tq=Tq, lp1=lp1, lq1=lq1, p=p, q=q, d_lp=d_lp, d_lq=d_lq)
        return cache[seed]
    return get


def run_ratio(H, s, spec, tt, tq, ratio_rows, seed=5, salt=2):
    """As test_hip_stochastic.run_verify, on the shared device logits; spec [N, K + 1], tt / tq / ratio_rows scalars."""
    K, N, V = s["K"], s["N"], V3
    d_lp, d_lq = s["d_lp"], s["d_lq"]
    d_tt, d_tq = dev(torch.full((N,), tt)), dev(torch.full((N,), tq))
    preds = ints(N * (K + 1))
    H.argmax_rows(d_lp, V, N * (K + 1), V, preds)
    lse_p, lse_q = torch.full((N * (K + 1),), NAN, device="cuda"), torch.full((N * K,), NAN, device="cuda")
    H.row_lse(d_lp, V, N * (K + 1), V, d_tt, K + 1, lse_p)
    H.row_lse(d_lq, V, N * K, V, d_tq, K, lse_q)
    acc, rec, packed = ints(N, torch.int32), ints(N), ints((N, K + 3))
    ap = torch.full((N, K), NAN, device="cuda")
    H.verify_ratio(d_lp, V, d_lq, V, V, N, K, dev(spec), preds, lse_p, lse_q, d_tt, d_tq,
                   dev(torch.full((N,), ratio_rows, dtype=torch.int32)), rng(seed), salt, acc, rec, packed, ap)
    torch.cuda.synchronize()
    a, r, pk = acc.cpu(), rec.cpu(), packed.cpu()
    assert torch.equal(pk[:, 0], a.long()) and torch.equal(pk[:, 1], r) and torch.equal(pk[:, 2:], spec)
    assert bool(((r >= 0) & (r < V)).all())
    return a, r, ap.cpu()


def accept_len_probs(a):
    K = len(a)
    pn, run = torch.zeros(K + 1, dtype=torch.float64), 1.0
    for i in range(K):
        pn[i] = run * (1 - float(a[i]))
        run *= float(a[i])
    pn[K] = run
    return pn


def oracle_accept_prob(s, spec1, tt, tq):
    B = 2
    lp, lq = s["lp1"].unsqueeze(0).repeat(B, 1, 1), s["lq1"].unsqueeze(0).repeat(B, 1, 1)
    _, _, ap = O.verify_full(lp, lq, spec1.unsqueeze(0).repeat(B, 1), torch.full((B,), tt), torch.full((B,), tq), jit_speculate=True)
    return ap[0]


def check_ratio_case(H, s, x, tt, tq, recovery_dist, what):
    """N identical ratio sequences: accept_prob against the oracle, the accepted-length distribution P(n) = prod_{i<n} a_i (1 - a_n)
    and the recovery token given n against recovery_dist(n), every n tested (its expected count is asserted first)."""
    K, N = s["K"], s["N"]
    spec1 = torch.cat([torch.tensor([7]), x])
    want_ap = oracle_accept_prob(s, spec1, tt, tq)
    pn = accept_len_probs(want_ap.double())
    assert float(pn.min()) * N >= 1000, f"{what}: an accepted length would be too rare to test its recovery: {pn.tolist()}"
    dists = [recovery_dist(n) for n in range(K + 1)]
    for n, r in enumerate(dists):
        check_bins(r, int(float(pn[n]) * N), f"{what}: recovery | n={n}", named=(), min_bins=12, max_pooled=0.05)
        live = r * float(pn[n]) * N >= 5         # bins of their own in every iteration of the 1024-stride loop
        assert bool(live[:1024].any()) and bool(live[1024:2048].any()) and bool(live[2048:].any()), f"{what}: recovery | n={n}"
    a, r, ap = run_ratio(H, s, spec1.unsqueeze(0).repeat(N, 1).contiguous(), tt, tq, 1)
    assert torch.equal(fbits(ap), fbits(ap[:1]).expand(N, K)), "identical sequences, different accept_prob"
    err = (ap[0] - want_ap).abs().max().item()
    print(f"{what}: accept_prob {ap[0].tolist()} err {err:.2e}")
    assert err < 2e-3
    chi2_ok(torch.bincount(a.long(), minlength=K + 1), pn.float(), f"{what}: accepted length")
    for n in range(K + 1):
        chi2_ok(torch.bincount(r[a == n], minlength=V3), dists[n], f"{what}: recovery | n={n}")


def pick_draft(p, q, lo=0.4, hi=0.8):
    """A draft token per position whose acceptance probability min(1, p/q) lies in [lo, hi]: the most probable such token under q."""
    xs = []
    for i in range(q.shape[0]):
        a = p[i] / q[i]
        ok = (a >= lo) & (a <= hi) & (q[i] > 0.01)
        assert bool(ok.any()), "no draft token with a mid-range acceptance probability: choose another seed"
        xs.append(int(torch.where(ok, q[i], torch.zeros_like(q[i])).argmax()))
    return torch.tensor(xs)


def test_verify_ratio_distributions_across_stride_iterations(H, ratio_setup):
    s = ratio_setup(VR_SEED)
    K, p, q = s["K"], s["p"], s["q"]
    x = pick_draft(p, q)

    def rec(n):
        if n == K:
            return p[K]
        r = (p[n] - q[n]).clamp(min=0)
        return r / r.sum()
    check_ratio_case(H, s, x, s["Tt"], s["Tq"], rec, "Tt=0.9 Tq=1.1")


def test_verify_ratio_greedy_target_and_non_ratio_rows(H, ratio_setup):
    s = ratio_setup(VR_SEED)
    K, N, p = s["K"], s["N"], s["p"]
    preds1 = O.argmax_rows(s["lp1"])
    # Tt = 0, Tq = 1.1: p is one-hot at the argmax, acceptance and recovery are exactly the greedy branch; the first mismatch
    # (none for b % 4 == 3) differs between sequences
    spec = torch.cat([torch.full((N, 1), 7), preds1[:K].unsqueeze(0).repeat(N, 1)], 1)
    bad = torch.arange(N) % (K + 1)
    sel = bad < K
    spec[sel, 1 + bad[sel]] = (spec[sel, 1 + bad[sel]] + 1 + torch.arange(N)[sel] % 5) % V3
    acc_w, rec_w = O.verify_greedy(preds1.unsqueeze(0).repeat(N, 1), spec)
    assert acc_w.tolist() == bad.tolist()
    a, r, ap = run_ratio(H, s, spec.contiguous(), 0.0, s["Tq"], 1)
    assert torch.equal(a.long(), acc_w) and torch.equal(r, rec_w)
    assert torch.equal(ap, (spec[:, 1:] == preds1[:K]).float())
    # a non-ratio row (cache miss without JIT) at Tt = 0.9: greedy acceptance, recovery ~ p at the stopping row
    for stop in (1, K):
        x = preds1[:K].clone()
        if stop < K:
            x[stop] = (x[stop] + 1) % V3
        spec1 = torch.cat([torch.tensor([7]), x])
        check_bins(p[stop], N, f"non-ratio recovery at row {stop}")
        a, r, ap = run_ratio(H, s, spec1.unsqueeze(0).repeat(N, 1).contiguous(), s["Tt"], s["Tq"], 0, seed=9)
        assert bool((a == stop).all())
        assert torch.equal(ap, (x == preds1[:K]).float().unsqueeze(0).expand(N, K))
        chi2_ok(torch.bincount(r, minlength=V3), p[stop], f"recovery of a non-ratio row stopping at {stop} ~ p")


def test_verify_ratio_greedy_draft(H, ratio_setup):
    """Tq = 0: the draft proposed its argmax, q is one-hot at x: accept with min(1, p(x)), recover from p without x."""
    s = ratio_setup(VR_SEED_GREEDY_DRAFT)
    K, p = s["K"], s["p"]
    x = s["lq1"].float().argmax(-1)

    def rec(n):
        if n == K:
            return p[K]
        r = p[n].clone()
        r[x[n]] = 0
        return r / r.sum()
    check_ratio_case(H, s, x, s["Tt"], 0.0, rec, "Tt=0.9 Tq=0")


@pytest.mark.parametrize("V", [7, 1025, 2600])
def test_row_lse_at_extreme_temperatures(H, V):
    """logit / T reaches +-600 at T = 0.05; float64 logsumexp of the same bf16 logits over the float32 temperature."""
    torch.manual_seed(V)
    temps = torch.tensor([0.05, 1.0, 4.0, 0.0])
    T = 3 * len(temps)
    x = torch.rand(T, V) * 60 - 30
    x[1] = torch.rand(V) * 10 - 30                                           # a row whose maximum is far below zero
    x[4, ::3] = -INF                                                         # -inf entries inside [0, V)
    x[0, V // 2] = 30.0
    x = x.to(BF)
    ld = V + 5
    lse = torch.full((T + 1,), NAN, device="cuda")
    H.row_lse(dev(pad_rows(x, ld, NAN)), ld, T, V, dev(temps), 3, lse)
    got = lse.cpu()
    assert math.isnan(float(got[T])), "wrote past T rows"
    assert got[9:12].tolist() == [0.0, 0.0, 0.0], "a temperature-0 row writes 0"
    tr = temps[:3].double().repeat_interleave(3).unsqueeze(1)
    want = torch.logsumexp(x[:9].double() / tr, dim=-1)
    f32 = torch.logsumexp(x[:9].float() / tr.float(), dim=-1)
    err = (got[:9].double() - want).abs()
    err32 = (f32.double() - want).abs()
    for i in range(9):
        print(f"V={V} T={float(tr[i]):.2f} lse={float(want[i]):.4f} kernel err {float(err[i]):.2e} torch-fp32 err {float(err32[i]):.2e}")
    assert float(err.max()) < 2e-3


# =====================================================================================================================
# 4. degenerate rows: never a token id outside the vocabulary
# =====================================================================================================================
@pytest.mark.parametrize("fill", [NAN, -INF])
def test_degenerate_rows_give_tokens_of_the_vocabulary(H, fill):
    V, T = 1304, 4                             # two iterations of the 1024-stride loops; V % 8 == 0 for ssd_argmax_rows
    x = dev(torch.full((T, V), fill, dtype=BF))
    top = ints((T, 8), torch.int32)
    H.topk_rows(x, V, T, V, 8, top)
    t = top.cpu()
    bad = []                                   # every kernel is run before the first assertion: the message names all offenders
    if not bool(((t >= 0) & (t < V)).all()):
        bad.append(f"topk_rows: {t[0].tolist()}")
    for temp in (0.0, 0.8):
        out, out2 = ints(T), ints(T)
        H.sample_rows(x, V, T, V, dev(torch.full((T,), temp)), 1, rng(1), 1, out, out2)
        o = out.cpu()
        if not (bool(((o >= 0) & (o < V)).all()) and torch.equal(o, out2.cpu())):
            bad.append(f"sample_rows T={temp}: {o.tolist()}")
    if fill == -INF:
        assert t.tolist() == [list(range(8))] * T, "all -inf: the lowest indices, as a stable sort"
    # verify_ratio: the degenerate row is the target row at the stopping position, Tt > 0
    torch.manual_seed(4)
    B, K = 4, 2
    lp = (torch.randn(B, K + 1, V) * 1.5).to(BF)
    lq = (torch.randn(B, K, V) * 1.5).to(BF)
    spec = torch.full((B, K + 1), 3, dtype=torch.int64)
    lp[:, :K, 3] = 30.0                      # p(x) ~ 1 >= q(x) at every position: accepted whatever the draw, greedy or ratio
    # seq 0 / 3: ratio / non-ratio row, everything accepted: the recovery is drawn from the degenerate bonus row K
    # seq 1: non-ratio row, a greedy mismatch at the degenerate row 1 (its argmax is 0, the draft said 3): recovery from row 1
    # seq 2: ratio row with the degenerate row at position 1 (wherever it stops, the recovery is a token)
    lp[0, K] = fill
    lp[3, K] = fill
    lp[1, 1] = fill
    lp[2, 1] = fill
    ratio = torch.tensor([1, 0, 1, 0], dtype=torch.int32)
    d_lp, d_lq = dev(lp.view(-1, V)), dev(lq.view(-1, V))
    tt, tq = dev(torch.full((B,), 0.9)), dev(torch.full((B,), 1.1))
    preds = ints(B * (K + 1))
    H.argmax_rows(d_lp, V, B * (K + 1), V, preds)
    lse_p, lse_q = torch.zeros(B * (K + 1), device="cuda"), torch.zeros(B * K, device="cuda")
    H.row_lse(d_lp, V, B * (K + 1), V, tt, K + 1, lse_p)
    H.row_lse(d_lq, V, B * K, V, tq, K, lse_q)
    acc, rec, packed = ints(B, torch.int32), ints(B), ints((B, K + 3))
    H.verify_ratio(d_lp, V, d_lq, V, V, B, K, dev(spec), preds, lse_p, lse_q, tt, tq, dev(ratio), rng(5), 2, acc, rec, packed)
    a, r = acc.cpu(), rec.cpu()
    if not bool(((r >= 0) & (r < V)).all()):
        bad.append(f"verify_ratio recovery: {r.tolist()}")
    assert not bad, "token ids outside [0, V): " + "; ".join(bad)
    assert [int(a[0]), int(a[1]), int(a[3])] == [K, 1, K] and 0 <= int(a[2]) <= K
    assert torch.equal(packed.cpu()[:, 1], r)


# =====================================================================================================================
# 5. RNG streams: salt, row and index do not alias
# =====================================================================================================================
def test_rng_streams_of_salt_and_row_do_not_alias(H):
    torch.manual_seed(9)
    V, N, T = 4096, 512, 1.5
    logits = (torch.randn(V) * 0.1).to(BF)
    probs = torch.softmax(logits.double() / T, -1)
    assert float((probs ** 2).sum()) < 0.01, "two independent draws must rarely coincide"
    rows = dev(logits.unsqueeze(0).repeat(N, 1))
    temps = dev(torch.full((N,), T))
    st = rng(12345)

    def draw(salt):
        out = ints(N)
        H.sample_rows(rows, V, N, V, temps, 1, st, salt, out)
        o = out.cpu()
        assert bool(((o >= 0) & (o < V)).all())
        return o

    def differ(a, b):
        return (a != b).float().mean().item()
    s0, s1, s0_again = draw(0), draw(1), draw(0)
    assert torch.equal(s0, s0_again)
    d = {"rows 256.. under salt 0 vs rows 0.. under salt 1": differ(s0[256:], s1[:256]),
         "rows r vs r + 256 under salt 0": differ(s0[:256], s0[256:]),
         "rows r vs r + 256 under salt 1": differ(s1[:256], s1[256:]),
         "salt 0 vs salt 1 at equal rows": differ(s0, s1),
         "salt 3 vs salt 4 at equal rows": differ(draw(3), draw(4)),
         "salt 1 vs salt 1 + 2^24 at equal rows": differ(s1, draw(1 + (1 << 24))),
         "rows 256.. under salt 1 vs rows 0.. under salt 0": differ(s1[256:], s0[:256])}
    print(d)
    for what, frac in d.items():
        assert frac > 0.5, f"{what}: the same stream ({frac:.3f} of the draws differ)"


# =====================================================================================================================
# 6. state kernels of csrc/misc.hip
# =====================================================================================================================
@pytest.mark.parametrize("V", [8, 8200])
def test_store_step_rows(H, V):
    """Row [b][step] of the destination is written for step < K and nothing else ever; 8200 / 8 = 1025 sixteen-byte chunks."""
    torch.manual_seed(V)
    B, K = 3, 4
    ld = V + 8
    src = pad_rows(torch.randn(B, V).to(BF), ld, NAN)
    d_src = dev(src)
    blank = torch.full((B, K, V), 0x7a5a, dtype=torch.int16)
    for step in (0, K - 1, K, K + 3):
        dst = dev(blank.clone())
        d_step = dev(torch.tensor([step], dtype=torch.int32))
        H.store_step_rows(d_src, ld, dst.view(BF), B, V, K, d_step)
        want = blank.clone()
        if step < K:
            want[:, step] = src[:, :V].view(torch.int16)
        assert torch.equal(dst.cpu(), want), step
        assert int(d_step.cpu()) == step
    dst, d_step = dev(blank.clone()), dev(torch.tensor([0], dtype=torch.int32))
    refuses(H.store_step_rows, d_src, ld, dst.view(BF), B, V - 4, K, d_step)
    refuses(H.store_step_rows, d_src, ld - 4, dst.view(BF), B, V, K, d_step)
    refuses(H.store_step_rows, d_src, ld, dst.view(BF), B, V, 0, d_step)
    assert torch.equal(dst.cpu(), blank)


def advance_ref(nxt, ids, pos, slots, ctx, bt, bs, spec, K, step):
    if step + 1 <= K:
        spec[:, step + 1] = nxt
    pos = pos + 1
    blk = bt[torch.arange(len(nxt)), pos // bs].long()
    slots = torch.where(blk >= 0, blk * bs + pos % bs, torch.full_like(blk, -1)).to(torch.int32)
    return nxt.clone(), pos, slots, ctx + 1, spec, step + 1


@pytest.mark.parametrize("B", [65, 1024])
@pytest.mark.parametrize("step", [1, 4, 7])
def test_draft_advance_and_the_fused_tail_past_one_wave(H, B, step):
    """ssd_draft_advance and ssd_argmax_parts_advance on the same state against four lines of Python: more than one wave of
    sequences, block size 256 with positions at the last slot of a block, -1 block-table entries, and step + 1 > K (the
    speculation table is left alone, the step is still bumped)."""
    g = torch.Generator().manual_seed(B + step)
    K, bs, mb, nparts, stride = 4, 256, 4, 5, 7
    bt = torch.randperm(B * mb, generator=g).to(torch.int32).view(B, mb)
    pos = torch.randint(0, 3 * bs - 1, (B,), generator=g, dtype=torch.int64)
    pos[::3] = bs - 1                                    # the next slot opens block 1
    pos[1::7] = 2 * bs - 1
    bt[::5, 1] = -1                                      # ... which some sequences do not have
    bt[3::11] = -1
    pv = torch.randint(0, 4, (B, stride), generator=g).float()             # ties between candidates: the lowest index wins
    pi = torch.randint(0, 50000, (B, stride), generator=g).to(torch.int32)
    pv[:, nparts:], pi[:, nparts:] = 99.0, 7                               # candidates past nparts are not read
    key = pv[:, :nparts].double() * 1e6 - pi[:, :nparts].double()
    nxt = pi[torch.arange(B), key.argmax(-1)].long()
    ids = torch.full((B,), SENT, dtype=torch.int64)
    slots = torch.full((B,), SENT, dtype=torch.int32)
    ctx = (pos + 1).to(torch.int32)
    spec = torch.full((B, K + 1), SENT, dtype=torch.int64)
    want = advance_ref(nxt, ids, pos, slots, ctx, bt, bs, spec.clone(), K, step)
    assert int((want[2] == -1).sum()) > 0 and int((want[2] % bs == 0).sum()) > 0

    def state():
        return [dev(t) for t in (ids, pos, slots, ctx, bt, spec, torch.tensor([step], dtype=torch.int32))]

    def check(s, what):
        got = [t.cpu() for t in s]
        assert torch.equal(got[0], want[0]), what + ": input_ids"
        assert torch.equal(got[1], want[1]), what + ": positions"
        assert torch.equal(got[2], want[2]), what + ": slots"
        assert torch.equal(got[3], want[3]), what + ": context_lens"
        assert torch.equal(got[4], bt), what + ": block tables"
        assert torch.equal(got[5], want[4]), what + ": speculation table"
        assert int(got[6]) == want[5] == step + 1, what + ": step"
    a, b_ = state(), state()
    H.draft_advance(dev(nxt), a[0], a[1], a[2], a[3], a[4], mb, bs, a[5], K, a[6], B)
    check(a, "draft_advance")
    nxt1 = ints(B)
    H.argmax_parts_advance(dev(pv), dev(pi), nparts, stride, nxt1, b_[0], b_[1], b_[2], b_[3], b_[4], mb, bs, b_[5], K, b_[6], B)
    assert torch.equal(nxt1.cpu(), nxt)
    check(b_, "argmax_parts_advance")


def test_draft_advance_refuses_more_than_1024_sequences(H):
    B = 1025
    z64, z32 = torch.zeros(B, dtype=torch.int64, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    bt, spec, step = torch.zeros(B, 2, dtype=torch.int32, device="cuda"), ints((B, 3)), dev(torch.tensor([0], dtype=torch.int32))
    refuses(H.draft_advance, z64, z64.clone(), z64.clone(), z32, z32.clone(), bt, 2, 16, spec, 2, step, B)
    pv, pi = torch.zeros(B, 4, device="cuda"), torch.zeros(B, 4, dtype=torch.int32, device="cuda")
    refuses(H.argmax_parts_advance, pv, pi, 4, 4, z64, z64.clone(), z64.clone(), z32, z32.clone(), bt, 2, 16, spec, 2, step, B)
    assert int(step.cpu()) == 0 and bool((spec.cpu() == SENT).all())


def test_cache_lookup_past_one_pass_of_the_block(H):
    """Bc * W = 600 entries against 256 threads: matches in the second and third pass, a key stored three times (the lowest entry
    wins), keys that match on two fields of three, and a request batch of one."""
    Bc, W = 25, 24
    seq = torch.arange(Bc, dtype=torch.int64) + 100
    seq[[12, 18, 24]] = 77                               # three cache rows of one sequence id
    cj = (torch.arange(Bc * W, dtype=torch.int32) % 8).view(Bc, W).contiguous()
    forks = (torch.arange(Bc * W, dtype=torch.int64) + 1000).view(Bc, W).contiguous()
    for b, i in ((12, 5), (18, 2), (24, 23)):            # entries 293, 434, 599
        cj[b, i], forks[b, i] = 6, 4242
    cj[0, 3], forks[0, 3] = 2, 555                       # entries 3 and 259: one thread in two passes, two sequence ids
    cj[10, 19], forks[10, 19] = 2, 555
    keys = [(77, 6, 4242),                               # three times: 293
            (100, 2, 555), (110, 2, 555),                # 3 and 259
            (int(seq[24]), int(cj[24, 22]), int(forks[24, 22])),     # 598, third pass
            (77, 6, 4243), (77, 5, 4242), (78, 6, 4242),             # two fields of three
            (110, int(cj[0, 4]), int(forks[0, 4])),      # sequence of row 10, position and token of entry 4
            (int(seq[11]), int(cj[11, 0]), int(forks[11, 0]))]       # 264
    flat_seq = seq.repeat_interleave(W)

    def ref(k):
        hit = (flat_seq == k[0]) & (cj.view(-1).long() == k[1]) & (forks.view(-1) == k[2])
        return int(hit.nonzero()[0]) if bool(hit.any()) else -1
    want = [ref(k) for k in keys]
    assert want == [293, 3, 259, 598, -1, -1, -1, -1, 264]
    d_seq, d_cj, d_forks = dev(seq), dev(cj), dev(forks)
    out = ints(len(keys) + 1, torch.int32)
    H.cache_lookup(dev(torch.tensor(keys, dtype=torch.int64)), d_seq, d_cj, d_forks, len(keys), Bc, W, out)
    assert out.cpu().tolist() == want + [SENT]
    for k, w in zip(keys[:5], want[:5]):                 # a request batch of one
        one = ints(2, torch.int32)
        H.cache_lookup(dev(torch.tensor([k], dtype=torch.int64)), d_seq, d_cj, d_forks, 1, Bc, W, one)
        assert one.cpu().tolist() == [w, SENT]
