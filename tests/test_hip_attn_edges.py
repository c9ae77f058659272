"""Paged attention (csrc/attention.hip: causal, tree and fused-o_proj forms) at the cache and mask edges tests/test_hip_ops.py and
test_hip_fuzz.py do not visit:

  A  poisoned caches   every (page, row) that is not key < ctx of some sequence is bf16 NaN in K and in V, and block-table entries past
                       a sequence's last page name an all-NaN page.  The kernel's addressing claim -- "never an unwritten row, never
                       an unallocated page" -- rests on clamps; a clamp off by one reads a row that the mask then sets to p = 0, and
                       0 * finite = 0 is bit-identical while 0 * NaN in the P.V MFMA is NaN.  The same launch on the clean and on the
                       poisoned cache must be finite, bit-identical, and within ATTN_TOL of the oracle (gather_paged reads valid rows only).
  C  tree mask         against O.attn_tree at the engine's shapes: block size 256 as well as 16, three head geometries, an empty trunk,
                       glue columns across a page and a 32-key tile edge, B = 3, both ways of naming a branch's glue position (fan-out
                       division and the explicit table the engine passes), and a tree wide enough for the two-row-tile kernel.
  E  writer -> reader  what ssd_rope_store_kv wrote, read by ssd_attn_paged through the same slots and block table (the two kernels share
                       slot = block * bs + pos and the HND page layout; each was only checked against oracle/layout.py's converter).

(B, the NaN-filled split workspaces, is tests/test_hip_ops.py run_attn_dev, which every launch here goes through.)  Every case is tens
of rows and at most a few hundred keys."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import layout as LY
from oracle import ops as O
from tests.test_hip_ops import ATTN_TOL, BF, H, dev, make_paged_poisoned, run_attn, run_attn_dev  # noqa: F401  (H is the fixture)
from tests.util import assert_close_bf16

HEADS = [(32, 8, 64), (16, 8, 128)]
BLOCK_SIZES = [16, 64, 256]


def bits(t):
    return t.contiguous().view(torch.int16)


def edge_ctx(bs):
    return [1, 15, 16, 17, 31, 33, bs - 1, bs, bs + 1, 2 * bs + 17]


def causal_cases(bs, heads):
    """Six launches of one (block size, head geometry): two batches of three mixed lengths (1 and 7 queries per sequence) and four
    single sequences, which between them take every edge length once; the start of the walk through the lengths and through the
    (waves, splits) pairs moves with the combination, so that each length meets different decompositions.  (B, qps, ctx, waves, splits)."""
    c = BLOCK_SIZES.index(bs) * len(HEADS) + HEADS.index(heads)
    e = edge_ctx(bs)
    e = e[3 * c % 10:] + e[:3 * c % 10]
    ws = [(1, 1), (8, 1), (1, 3), (8, 3)]
    shapes = [(3, 1, e[0:3]), (3, 7, e[3:6]), (1, 1, e[6:7]), (1, 7, e[7:8]), (1, 1, e[8:9]), (1, 7, e[9:10])]
    return [(B, qps, [max(qps, L) for L in ctx]) + ws[(c + i) % 4] for i, (B, qps, ctx) in enumerate(shapes)]


def test_causal_case_table_covers_every_axis_value_twice():
    """The hand-picked subset (36 launches) instead of the full product: each value of each axis at least twice."""
    seen = {}
    n = 0
    for bs in BLOCK_SIZES:
        for heads in HEADS:
            for B, qps, ctx, waves, splits in causal_cases(bs, heads):
                n += 1
                for key in [("bs", bs), ("heads", heads), ("B", B), ("qps", qps), ("waves", waves), ("splits", splits)] + \
                           [("ctx", bs, i) for i, L in enumerate(edge_ctx(bs)) if max(qps, L) in ctx]:
                    seen[key] = seen.get(key, 0) + 1
    assert n == 36
    want = [("bs", b) for b in BLOCK_SIZES] + [("heads", h) for h in HEADS] + [("B", 1), ("B", 3), ("qps", 1), ("qps", 7)] + \
           [("waves", 1), ("waves", 8), ("splits", 1), ("splits", 3)] + [("ctx", b, i) for b in BLOCK_SIZES for i in range(10)]
    for key in want:
        assert seen.get(key, 0) >= 2, key


def check_poisoned(H, q, caches, ctx_lens, nh, nkv, hd, bs, ref, what, **kw):
    kc, vc, kp, vp, bt, mb = caches
    ctx = torch.tensor(ctx_lens, dtype=torch.int32)
    T = q.shape[0]
    clean = run_attn(H, q.view(T, -1), kc, vc, bt, mb, ctx, nh, nkv, hd, bs, **kw)
    pois = run_attn(H, q.view(T, -1), kp, vp, bt, mb, ctx, nh, nkv, hd, bs, **kw)
    assert torch.isfinite(pois.float()).all(), f"{what}: a row past ctx or a page no sequence owns reached the output"
    assert torch.equal(bits(pois), bits(clean)), f"{what}: the poisoned cache changed the output"
    assert_close_bf16(pois, ref, what=what, **ATTN_TOL)


# ---------------------------------------------------------------------------------------------------------------------
# A. Poisoned caches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,nkv,hd", HEADS)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_poisoned_cache_causal(H, bs, nh, nkv, hd):
    for B, qps, ctx_lens, waves, splits in causal_cases(bs, (nh, nkv, hd)):
        caches = make_paged_poisoned(B, ctx_lens, nkv, hd, bs, seed=bs + hd + qps + sum(ctx_lens))
        torch.manual_seed(sum(ctx_lens) + qps)
        q = torch.randn(B * qps, nh, hd).to(BF)
        ctx = torch.tensor(ctx_lens, dtype=torch.int32)
        cu = torch.arange(B + 1, dtype=torch.int32) * qps
        ref = O.attn_paged(q, caches[0], caches[1], ctx, caches[4], hd ** -0.5, cu_q=cu).reshape(B * qps, nh * hd)
        check_poisoned(H, q, caches, ctx_lens, nh, nkv, hd, bs, ref, f"poisoned bs{bs} B{B} q{qps} ctx{ctx_lens} w{waves} s{splits} hd{hd}",
                       q_per_seq=qps, waves=waves, splits=splits)


@pytest.mark.parametrize("nh,nkv,hd,bs", [(32, 8, 64, 16), (16, 8, 128, 256)])
def test_poisoned_cache_varlen_prefill(H, nh, nkv, hd, bs):
    """cu_q = [0, 5, 38] over ctx = [5, 40]: the second sequence is prefix-cache style (33 queries over 40 keys)."""
    ctx_lens = [5, 40]
    caches = make_paged_poisoned(2, ctx_lens, nkv, hd, bs, seed=bs + hd)
    torch.manual_seed(bs)
    q = torch.randn(38, nh, hd).to(BF)
    cu = torch.tensor([0, 5, 38], dtype=torch.int32)
    ref = O.attn_paged(q, caches[0], caches[1], torch.tensor(ctx_lens, dtype=torch.int32), caches[4], hd ** -0.5, cu_q=cu).reshape(38, nh * hd)
    check_poisoned(H, q, caches, ctx_lens, nh, nkv, hd, bs, ref, f"poisoned varlen bs{bs} hd{hd}", cu_q=cu)


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("nh,nkv,hd", HEADS)
def test_poisoned_cache_transpose_read_and_plain_read(H, nh, nkv, hd, flags):
    """flags bit 0 reads the staged V tile element by element instead of through the transpose-read: the same rows of the same tile."""
    bs, B, qps, ctx_lens = 64, 3, 7, [17, 63, 145]
    caches = make_paged_poisoned(B, ctx_lens, nkv, hd, bs, seed=hd)
    torch.manual_seed(hd)
    q = torch.randn(B * qps, nh, hd).to(BF)
    cu = torch.arange(B + 1, dtype=torch.int32) * qps
    ref = O.attn_paged(q, caches[0], caches[1], torch.tensor(ctx_lens, dtype=torch.int32), caches[4], hd ** -0.5, cu_q=cu).reshape(B * qps, nh * hd)
    check_poisoned(H, q, caches, ctx_lens, nh, nkv, hd, bs, ref, f"poisoned flags{flags} hd{hd}", q_per_seq=qps, waves=8, flags=flags)


def test_poisoned_cache_tree(H):
    nh, nkv, hd, bs, K, F, step = 32, 8, 64, 256, 7, 3, 3
    MQ = F * (K + 1)
    ctx_lens = [p + K + 1 + (step + 1) * MQ for p in (0, 253)]
    caches = make_paged_poisoned(2, ctx_lens, nkv, hd, bs, seed=41)
    torch.manual_seed(41)
    q = torch.randn(2 * MQ, nh, hd).to(BF)
    jidx = [i // F for i in range(MQ)]
    ref = O.attn_tree(q, caches[0], caches[1], torch.tensor(ctx_lens, dtype=torch.int32), caches[4], hd ** -0.5, step, K,
                      [jidx, jidx]).reshape(2 * MQ, nh * hd)
    for waves in (1, 8):
        check_poisoned(H, q, caches, ctx_lens, nh, nkv, hd, bs, ref, f"poisoned tree w{waves}", q_per_seq=MQ, waves=waves, mode=H.MODE_TREE,
                       tree_K=K, tree_mq=MQ, tree_step=step, tree_F=F)


@pytest.mark.parametrize("bs", [16, 256])
@pytest.mark.parametrize("ctx_len", [37, 260])
@pytest.mark.parametrize("nh,nkv,hd,N,T", [(32, 8, 64, 2048, 8), (16, 8, 128, 1024, 3)])
def test_poisoned_cache_attention_oproj_slabs(H, nh, nkv, hd, N, T, ctx_len, bs):
    """ssd_attn_oproj_parts (T = 8 at four q heads per kv head is its two-row-tile variant): the fp32 slabs over the poisoned cache are
    finite and the clean cache's, bit for bit.  (Their values are tests/test_hip_attn_oproj.py's subject.)"""
    kc, vc, kp, vp, bt, mb = make_paged_poisoned(1, [ctx_len], nkv, hd, bs, seed=ctx_len + T)
    torch.manual_seed(T + hd)
    q = torch.randn(T, nh * hd).to(BF)
    wf = dev(LY.rows_to_frag_ref((torch.randn(N, nh * hd) * 0.05).to(BF)))
    qd, btd, cd = dev(q), dev(bt), dev(torch.tensor([ctx_len], dtype=torch.int32))
    slabs = []
    for k, v in ((kc, vc), (kp, vp)):
        got = torch.full((nkv, T, N), float("nan"), dtype=torch.float32, device="cuda")
        H.attn_oproj_parts(qd, dev(LY.kv_nhd_to_hnd(k)), dev(LY.kv_nhd_to_hnd(v)), btd, mb, cd, T, nh, nkv, hd, bs, hd ** -0.5, wf, N, got)
        torch.cuda.synchronize()
        slabs.append(got.cpu())
    assert torch.isfinite(slabs[0]).all()
    assert torch.isfinite(slabs[1]).all(), "a row past ctx or a page no sequence owns reached the slabs"
    assert torch.equal(slabs[0].view(torch.int32), slabs[1].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# C. Tree mask against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def tree_setup(B, prefixes, K, MQ, step, nh, nkv, hd, bs, seed):
    ctx_lens = [p + K + 1 + (step + 1) * MQ for p in prefixes]
    kc, vc, kp, vp, bt, mb = make_paged_poisoned(B, ctx_lens, nkv, hd, bs, seed=seed)
    torch.manual_seed(seed)
    q = torch.randn(B * MQ, nh, hd).to(BF)
    ctx = torch.tensor(ctx_lens, dtype=torch.int32)
    return q, kc, vc, dev(LY.kv_nhd_to_hnd(kp)), dev(LY.kv_nhd_to_hnd(vp)), bt, mb, ctx


@pytest.mark.parametrize("bs", [16, 256])
@pytest.mark.parametrize("nh,nkv,hd", [(32, 8, 64), (16, 8, 128), (8, 1, 128)])
def test_tree_mask_vs_oracle(H, nh, nkv, hd, bs):
    """B = 3 with trunk prefixes [0, bs - 3, 2 bs + 5]: an empty trunk, glue columns (K + 1 of them, from the prefix on) that cross a
    page and a 32-key tile edge, and a trunk of several pages; first and last tree step; the structural way (branch / fan_out) and the
    engine's (tree_F = 1 with the explicit branch -> glue-position table), which must agree bit for bit where both apply.  (The caches
    are the poisoned ones: the oracle reads valid rows only.)"""
    B, prefixes = 3, [0, bs - 3, 2 * bs + 5]
    trees = [(7, 3, [[i // 3 for i in range(24)]] * 3),
             (3, None, [[j for j, f in enumerate(l) for _ in range(f)] for l in ([2, 2, 3, 1], [3, 2, 2, 1], [1, 1, 1, 5])])]
    for K, F, jl in trees:
        MQ = len(jl[0])
        jd = dev(torch.tensor(jl, dtype=torch.int32))
        for step in (0, K - 1):
            q, kc, vc, kd, vd, bt, mb, ctx = tree_setup(B, prefixes, K, MQ, step, nh, nkv, hd, bs, seed=K * 10 + step + bs)
            ref = O.attn_tree(q, kc, vc, ctx, bt, hd ** -0.5, step, K, jl).reshape(B * MQ, nh * hd)
            for waves, splits in ((1, 1), (8, 1), (2, 3)):
                what = f"tree K{K} MQ{MQ} step{step} bs{bs} w{waves} s{splits} heads {nh}/{nkv}x{hd}"
                kw = dict(q_per_seq=MQ, waves=waves, splits=splits, mode=H.MODE_TREE, tree_K=K, tree_mq=MQ, tree_step=step)
                table = run_attn_dev(H, q.view(B * MQ, -1), kd, vd, bt, mb, ctx, nh, nkv, hd, bs, tree_F=1, tree_jidx=jd, **kw)
                assert_close_bf16(table, ref, what=what + " (branch table)", **ATTN_TOL)
                if F is not None:
                    struct = run_attn_dev(H, q.view(B * MQ, -1), kd, vd, bt, mb, ctx, nh, nkv, hd, bs, tree_F=F, **kw)
                    assert_close_bf16(struct, ref, what=what + " (fan-out)", **ATTN_TOL)
                    assert torch.equal(bits(struct), bits(table)), what + ": fan-out and branch table differ"


@pytest.mark.parametrize("step", [0, 6])
def test_wide_tree_one_and_two_row_tiles_per_workgroup(H, step):
    """K = 7, F = 5: 40 branches x 4 q heads per kv head = 160 rows, ten row tiles -- the two-row-tile kernel by default, the
    one-row-tile kernel with flags bit 2 (what the engine always sets).  The same key split per wave, so the same bits."""
    nh, nkv, hd, bs, K, F, B = 32, 8, 64, 256, 7, 5, 2
    MQ = F * (K + 1)
    jl = [[i // F for i in range(MQ)]] * B
    q, kc, vc, kd, vd, bt, mb, ctx = tree_setup(B, [0, 253], K, MQ, step, nh, nkv, hd, bs, seed=step + 5)
    ref = O.attn_tree(q, kc, vc, ctx, bt, hd ** -0.5, step, K, jl).reshape(B * MQ, nh * hd)
    for waves in (1, 4):
        kw = dict(q_per_seq=MQ, waves=waves, mode=H.MODE_TREE, tree_K=K, tree_mq=MQ, tree_step=step, tree_F=F)
        two = run_attn_dev(H, q.view(B * MQ, -1), kd, vd, bt, mb, ctx, nh, nkv, hd, bs, **kw)
        one = run_attn_dev(H, q.view(B * MQ, -1), kd, vd, bt, mb, ctx, nh, nkv, hd, bs, flags=4, **kw)
        assert torch.equal(bits(one), bits(two)), f"wide tree step {step} waves {waves}: row tiles per workgroup change the bits"
        assert_close_bf16(two, ref, what=f"wide tree step {step} waves {waves}, two row tiles", **ATTN_TOL)
        assert_close_bf16(one, ref, what=f"wide tree step {step} waves {waves}, one row tile", **ATTN_TOL)


# ---------------------------------------------------------------------------------------------------------------------
# E. Writer -> reader round trip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_store_then_attention_round_trip(H, hd):
    """ssd_rope_store_kv writes two sequences (300 and 70 tokens, block size 256, shuffled block table) into a device cache prefilled
    with the bf16 NaN 0x7FC0, in two calls -- the second appends across a page edge -- and ssd_attn_paged reads that same cache for a
    7-row verify at the end of each sequence and for a single-token decode.  Oracle: O.rope + O.store_kv + O.attn_paged on
    reference-layout caches.  Rows past ctx were never written and are NaN, so this is part A once more, end to end."""
    nh, nkv, bs, lens, nb, mb = 8, 2, 256, [300, 70], 5, 3
    first = [250, 60]                                        # tokens of each sequence in the first call
    torch.manual_seed(hd)
    pages = torch.randperm(nb)
    bt = torch.full((2, mb), int(pages[4]), dtype=torch.int32)     # entries past the last page: an allocated page nobody writes
    bt[0, :2] = pages[0:2].to(torch.int32)
    bt[1, :1] = pages[2:3].to(torch.int32)
    cache = O.make_cos_sin_cache(hd, 512, 5e5)
    sent = lambda *shape: torch.full(shape, 0x7FC0, dtype=torch.int16).view(BF)
    kd, vd = sent(nb, nkv, bs, hd).cuda(), sent(nb, nkv, bs, hd).cuda()
    kref, vref = sent(nb, bs, nkv, hd), sent(nb, bs, nkv, hd)
    qkv = [torch.randn(L, (nh + 2 * nkv) * hd).to(BF) for L in lens]
    qref = [None, None]
    qdev = [[], []]
    for lo_hi in ([(0, first[0]), (0, first[1])], [(first[0], lens[0]), (first[1], lens[1])]):
        rows = torch.cat([qkv[b][lo:hi] for b, (lo, hi) in enumerate(lo_hi)])
        pos = torch.cat([torch.arange(lo, hi) for lo, hi in lo_hi])
        slots = torch.cat([bt[b, torch.arange(lo, hi) // bs] * bs + torch.arange(lo, hi).to(torch.int32) % bs
                           for b, (lo, hi) in enumerate(lo_hi)]).to(torch.int32)
        T = rows.shape[0]
        q_out = torch.full((T, nh * hd), float("nan"), dtype=BF, device="cuda")
        H.rope_store_kv(dev(rows), dev(pos), dev(cache), dev(slots), q_out, kd, vd, T, nh, nkv, hd, bs)
        torch.cuda.synchronize()
        n0 = lo_hi[0][1] - lo_hi[0][0]
        qdev[0].append(q_out.cpu()[:n0])
        qdev[1].append(q_out.cpu()[n0:])
    for b in range(2):
        q, k, v = qkv[b].split([nh * hd, nkv * hd, nkv * hd], dim=1)
        pos = torch.arange(lens[b])
        qr, kr = O.rope(pos, q.contiguous(), k.contiguous(), cache, hd)
        slots = (bt[b, pos // bs] * bs + pos.to(torch.int32) % bs).to(torch.int32)
        O.store_kv(kr.view(-1, nkv, hd), v.contiguous().view(-1, nkv, hd), kref, vref, slots)
        qref[b] = qr
        assert torch.equal(bits(torch.cat(qdev[b])), bits(qr))          # (no head norm: the rotation is the oracle's arithmetic)
    ctx = torch.tensor(lens, dtype=torch.int32)
    for qps in (7, 1):
        q = torch.cat([qref[b][lens[b] - qps:] for b in range(2)]).view(2 * qps, nh, hd)
        cu = torch.arange(3, dtype=torch.int32) * qps
        ref = O.attn_paged(q, kref, vref, ctx, bt, hd ** -0.5, cu_q=cu).reshape(2 * qps, nh * hd)
        assert torch.isfinite(ref.float()).all()
        for waves, splits in ((1, 1), (8, 2)):
            got = run_attn_dev(H, q.view(2 * qps, -1), kd, vd, bt, mb, ctx, nh, nkv, hd, bs, q_per_seq=qps, waves=waves, splits=splits)
            assert_close_bf16(got, ref, what=f"round trip hd{hd} q{qps} w{waves} s{splits}", **ATTN_TOL)     # (asserts finite as well)
