"""The FP8 KV cache kernels (include/ssd_hip_kv8.h) on the GPU, through the C ABI:

  1  store       ssd_rope_store_kv_fp8 against ssd_rope_store_kv: q rows bit for bit, the WHOLE byte cache == kv_fp8_encode of the bf16
                 kernel's whole cache (both prefilled with a sentinel, so a stray store shows), ssd_kv_fp8_dequant == decode.
  2  exact       ssd_attn_paged_fp8 with scales 1.0 and per-head powers of two against ssd_attn_paged over the bf16 cache bf16(s * c):
                 that product is exact and a power of two commutes with every rounding in the kernel, so the outputs are bit-identical.
  3  general     scales {0.37, 1.9} against oracle.ops.attn_paged on the fp32 cache s * c, to the existing ATTN_TOL.
  4  poisoned    every (page, row) that is not key < ctx of some sequence holds the NaN code 0x7F in K and in V: finite and bit-identical
                 to the clean run.
  5  repeats     bit-identical repeats, and one hipGraph replay of store -> attention through one block table.

Every case is tens of rows and at most 300 keys."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import layout as LY
from oracle import ops as O
from tests import kv8_ref
from tests.test_hip_ops import ATTN_TOL, BF, H, dev, make_paged_poisoned, run_attn_dev  # noqa: F401  (H is the fixture)
from tests.util import assert_close_bf16

SENTINEL = 0x55           # e4m3 13.0


@pytest.fixture(scope="module")
def KV8(H):
    from ssd_amd.hip import kv8_ops
    kv8_ops.load_kv8_library()
    return kv8_ops


def bits(t):
    return t.contiguous().view(torch.int16)


def head_scales(kind, nkv):
    vals = {"one": [1.0], "pow2": [0.5, 2.0], "pow2x": [0.5, 2.0, 4.0], "gen": [0.37, 1.9]}[kind]
    k = torch.tensor([vals[h % len(vals)] for h in range(nkv)], dtype=torch.float32)
    v = torch.tensor([vals[(h + 1) % len(vals)] for h in range(nkv)], dtype=torch.float32)
    return k, v


class Fp8Attn:
    """What run_attn_dev needs of `ops`, with attn_paged going to ssd_attn_paged_fp8 under fixed scales."""

    def __init__(self, H, KV8, k_scale, v_scale):
        self.frag_numel = H.frag_numel
        self.KV8, self.ks, self.vs = KV8, dev(k_scale), dev(v_scale)

    def attn_paged(self, q, kd, vd, bt, mb, ctx, B, T, max_q, nh, nkv, hd, bs, scale, **kw):
        self.KV8.attn_paged_fp8(q, kd, vd, bt, mb, ctx, B, T, max_q, nh, nkv, hd, bs, scale, k_scale=self.ks, v_scale=self.vs, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 1. Store
# ---------------------------------------------------------------------------------------------------------------------
STORE = [  # nh, nkv, hd, bs, qkv_perm, scales, head norm
    (4, 2, 64, 16, 0, "one", False), (4, 2, 64, 16, 1, "pow2", False), (4, 2, 64, 16, 0, "gen", True),
    (8, 2, 128, 256, 1, "one", False), (8, 2, 128, 256, 0, "pow2", False), (8, 2, 128, 256, 1, "gen", False),
    (8, 2, 128, 256, 1, "pow2", True),
]


@pytest.mark.parametrize("nh,nkv,hd,bs,perm,sk,norm", STORE)
def test_store_equals_the_encoded_bf16_store(H, KV8, nh, nkv, hd, bs, perm, sk, norm):
    from ssd_amd.quant import kv_fp8_encode, kv_fp8_decode
    T, nblocks = 5, 5
    slots = torch.tensor([-1, 0, bs - 1, bs, 3 * bs + 7], dtype=torch.int32)
    pos = torch.tensor([3, 0, 17, 40, 100], dtype=torch.int64)
    g = torch.Generator().manual_seed(nh + hd + perm)
    qkv = (torch.randn(T, (nh + 2 * nkv) * hd, generator=g) * 2).to(BF)            # N(0, 4)
    ks, vs = head_scales(sk, nkv)
    for t in range(T):          # planted values in every k and v head of every row: beyond the range, at it, the tie, -0.0
        for h in range(nkv):
            for base, s in ((nh * hd + h * hd, ks[h].item()), ((nh + nkv) * hd + h * hd, vs[h].item())):
                plant = torch.tensor([1000.0, -1000.0, 448.0 * s, -448.0 * s, 2.0 ** -10 * s, -0.0]).to(BF)
                qkv[t, base + 2 * t: base + 2 * t + 6] = plant
                qkv[t, base + hd // 2 + t: base + hd // 2 + t + 6] = plant
    cache = O.make_cos_sin_cache(hd, 128, 10000.0)
    qn = (1 + 0.1 * torch.randn(hd, generator=g)).to(BF) if norm else None
    kn = (1 + 0.1 * torch.randn(hd, generator=g)).to(BF) if norm else None
    nw = dict(q_norm_w=None if qn is None else dev(qn), k_norm_w=None if kn is None else dev(kn), eps=1e-6 if norm else 0.0, qkv_perm=perm)
    # bf16 kernel over a cache prefilled, per head, with the bf16 value that encodes to the sentinel under that head's scale (13.0 at 1.0)
    shape = (nblocks, nkv, bs, hd)
    kb = (kv_fp8_decode(torch.full(shape, SENTINEL, dtype=torch.uint8), ks.view(1, -1, 1, 1))).to(BF)
    vb = (kv_fp8_decode(torch.full(shape, SENTINEL, dtype=torch.uint8), vs.view(1, -1, 1, 1))).to(BF)
    assert (kv_fp8_encode(kb, 1.0 / ks.view(1, -1, 1, 1)) == SENTINEL).all() and (kv_fp8_encode(vb, 1.0 / vs.view(1, -1, 1, 1)) == SENTINEL).all()
    kb, vb = dev(kb), dev(vb)
    q_ref = torch.full((T, nh * hd), float("nan"), dtype=BF, device="cuda")
    H.rope_store_kv(dev(qkv), dev(pos), dev(cache), dev(slots), q_ref, kb, vb, T, nh, nkv, hd, bs, **nw)
    k8 = torch.full(shape, SENTINEL, dtype=torch.uint8, device="cuda")
    v8 = torch.full(shape, SENTINEL, dtype=torch.uint8, device="cuda")
    q_got = torch.full((T, nh * hd), float("nan"), dtype=BF, device="cuda")
    one = sk == "one"           # NULL scale pointers mean 1.0
    KV8.rope_store_kv_fp8(dev(qkv), dev(pos), dev(cache), dev(slots), q_got, k8, v8, T, nh, nkv, hd, bs,
                          k_inv_scale=None if one else dev(1.0 / ks), v_inv_scale=None if one else dev(1.0 / vs), **nw)
    torch.cuda.synchronize()
    assert torch.equal(bits(q_got.cpu()), bits(q_ref.cpu())), "q rows differ from ssd_rope_store_kv"
    for name, c8, cb, s in (("k", k8, kb, ks), ("v", v8, vb, vs)):
        want = kv_fp8_encode(cb.cpu(), 1.0 / s.view(1, -1, 1, 1))
        got = c8.cpu()
        assert torch.equal(got, want), f"{name} cache: {(got != want).sum().item()} bytes differ from encode(bf16 cache)"
        assert (got != SENTINEL).any() and not ((got == 0x7F) | (got == 0xFF)).any()
        deq = torch.full(shape, float("nan"), dtype=BF, device="cuda")
        KV8.kv_fp8_dequant(c8, None if one else dev(s), deq, nblocks, nkv, bs, hd)
        torch.cuda.synchronize()
        assert torch.equal(bits(deq.cpu()), bits(kv_fp8_decode(got, s.view(1, -1, 1, 1)).to(BF))), f"{name} dequant"
    # the planted values landed as specified (V passes through unrotated): saturation both ways, the range edge, the tie, -0.0
    blk, off = divmod(int(slots[4]), bs)
    assert v8[blk, 1, off, 8:14].cpu().tolist() == [0x7E, 0xFE, 0x7E, 0xFE, 0x00, 0x80]


# ---------------------------------------------------------------------------------------------------------------------
# 2-4. Attention
# ---------------------------------------------------------------------------------------------------------------------
def shape_of(kind):
    """(B, queries per sequence or None, ctx lens, cu_q or None, launch keywords)"""
    return {
        "decode": (3, 1, [1, 17, 48], None, {}),
        "verify": (2, 8, [8, 45], None, {}),
        "waves1": (1, 8, [300], None, dict(waves=1)),
        "waves8": (1, 8, [300], None, dict(waves=8)),
        "splits": (1, 8, [200], None, dict(splits=2, waves=4)),            # 7 key tiles over 2 x 4 parts: one wave sits idle
        "varlen": (2, None, [40, 21], [0, 40, 45], {}),                  # the second sequence behind a 16-key cached prefix
    }[kind]


# kind, nh, nkv, hd, bs, scales, flags -- each of hd 64 / 128, block 16 / 256, G 1 / 4 / 8 in at least two cases
EXACT = [
    ("decode", 4, 4, 64, 16, "one", 0), ("decode", 8, 2, 128, 256, "pow2x", 0), ("decode", 8, 1, 128, 16, "pow2x", 0),
    ("verify", 2, 2, 128, 256, "one", 0), ("verify", 8, 2, 64, 16, "pow2x", 0), ("verify", 16, 2, 64, 256, "pow2x", 1),
    ("waves1", 8, 2, 128, 256, "pow2x", 0), ("waves8", 8, 1, 64, 16, "one", 0), ("splits", 8, 2, 128, 16, "pow2x", 0),
    ("varlen", 8, 2, 128, 16, "pow2x", 0), ("varlen", 16, 4, 64, 256, "one", 0),
]
_CACHE = {}


def make_case(kind, nh, nkv, hd, bs):
    """q, random codes over the 254 finite values in the reference layout [blocks][bs][nkv][hd], the poisoned copies (0x7F in every
    row that is not key < ctx of some sequence), the block table.  Built once per case and shared, never modified."""
    key = (kind, nh, nkv, hd, bs)
    if key not in _CACHE:
        B, qps, ctx_lens, cu, kw = shape_of(kind)
        _, _, kp, _, bt, mb = make_paged_poisoned(B, ctx_lens, nkv, hd, bs, seed=nh + hd + bs + len(kind))
        invalid = torch.isnan(kp[:, :, 0, 0].float())            # [blocks][bs]
        g = torch.Generator().manual_seed(hd + bs + nh)
        fin = kv8_ref.FINITE_CODES
        kc = fin[torch.randint(0, 254, kp.shape, generator=g)]
        vc = fin[torch.randint(0, 254, kp.shape, generator=g)]
        kpo, vpo = kc.clone(), vc.clone()
        kpo[invalid] = 0x7F
        vpo[invalid] = 0x7F
        T = B * qps if cu is None else cu[-1]
        # q small enough that logits of |k| <= 448 keys stay in a range where the softmax has more than one live key
        q = (torch.randn(T, nh * hd, generator=g) * 0.02).to(BF)
        _CACHE[key] = dict(q=q, kc=kc, vc=vc, kp=kpo, vp=vpo, bt=bt, mb=mb, ctx=torch.tensor(ctx_lens, dtype=torch.int32),
                           cu=None if cu is None else torch.tensor(cu, dtype=torch.int32), qps=qps or 0, kw=kw, invalid=invalid)
    return _CACHE[key]


def run8(H, KV8, c, kc, vc, ks, vs, nh, nkv, hd, bs, flags):
    return run_attn_dev(Fp8Attn(H, KV8, ks, vs), c["q"], dev(LY.kv_nhd_to_hnd(kc)), dev(LY.kv_nhd_to_hnd(vc)), c["bt"], c["mb"], c["ctx"],
                        nh, nkv, hd, bs, cu_q=c["cu"], q_per_seq=c["qps"], flags=flags, **c["kw"])


def test_exact_case_table_covers_every_axis_value_twice():
    seen = {}
    for kind, nh, nkv, hd, bs, sk, flags in EXACT:
        for key in (("hd", hd), ("bs", bs), ("G", nh // nkv), ("scales", sk)):
            seen[key] = seen.get(key, 0) + 1
    for key in [("hd", 64), ("hd", 128), ("bs", 16), ("bs", 256), ("G", 1), ("G", 4), ("G", 8), ("scales", "one"), ("scales", "pow2x")]:
        assert seen.get(key, 0) >= 2, key
    assert {k for k, *_ in EXACT} == {"decode", "verify", "waves1", "waves8", "splits", "varlen"}
    assert sum(f & 1 for *_, f in EXACT) == 1
    c = shape_of("varlen")
    assert c[3][1] * 4 == 160 and c[2][1] - (c[3][2] - c[3][1]) == 16      # two row tiles per workgroup at G = 4; a 16-key prefix


@pytest.mark.parametrize("kind,nh,nkv,hd,bs,sk,flags", EXACT)
def test_attention_with_exact_scales_is_bit_identical_to_the_bf16_kernel(H, KV8, kind, nh, nkv, hd, bs, sk, flags):
    c = make_case(kind, nh, nkv, hd, bs)
    ks, vs = head_scales(sk, nkv)
    kb = kv8_ref.decode(c["kc"], ks.view(1, 1, -1, 1))
    vb = kv8_ref.decode(c["vc"], vs.view(1, 1, -1, 1))
    assert torch.equal(kb.to(BF).float(), kb) and torch.equal(vb.to(BF).float(), vb)           # bf16(s * c) is exact
    want = run_attn_dev(H, c["q"], dev(LY.kv_nhd_to_hnd(kb.to(BF))), dev(LY.kv_nhd_to_hnd(vb.to(BF))), c["bt"], c["mb"], c["ctx"], nh, nkv, hd,
                        bs, cu_q=c["cu"], q_per_seq=c["qps"], flags=flags, **c["kw"])
    got = run8(H, KV8, c, c["kc"], c["vc"], ks, vs, nh, nkv, hd, bs, flags)
    assert torch.isfinite(got.float()).all()
    assert got.float().abs().max() > 0
    assert torch.equal(bits(got), bits(want)), f"{kind}: {(bits(got) != bits(want)).sum().item()} elements differ from the bf16 kernel"
    # 5: a repeat reproduces the bits
    assert torch.equal(bits(run8(H, KV8, c, c["kc"], c["vc"], ks, vs, nh, nkv, hd, bs, flags)), bits(got))


def test_null_scale_pointers_mean_one(H, KV8):
    kind, nh, nkv, hd, bs = "verify", 8, 2, 64, 16
    c = make_case(kind, nh, nkv, hd, bs)
    ks, vs = head_scales("one", nkv)
    want = run8(H, KV8, c, c["kc"], c["vc"], ks, vs, nh, nkv, hd, bs, 0)

    class Null(Fp8Attn):
        def attn_paged(self, q, kd, vd, bt, mb, ctx, B, T, max_q, nh, nkv, hd, bs, scale, **kw):
            self.KV8.attn_paged_fp8(q, kd, vd, bt, mb, ctx, B, T, max_q, nh, nkv, hd, bs, scale, **kw)
    got = run_attn_dev(Null(H, KV8, ks, vs), c["q"], dev(LY.kv_nhd_to_hnd(c["kc"])), dev(LY.kv_nhd_to_hnd(c["vc"])), c["bt"], c["mb"], c["ctx"],
                       nh, nkv, hd, bs, q_per_seq=c["qps"])
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("kind,nh,nkv,hd,bs", [("decode", 8, 2, 128, 256), ("verify", 8, 2, 64, 16), ("splits", 8, 2, 128, 16),
                                                ("varlen", 8, 2, 128, 16), ("waves8", 8, 1, 64, 16)])
def test_attention_with_general_scales_against_the_oracle(H, KV8, kind, nh, nkv, hd, bs):
    c = make_case(kind, nh, nkv, hd, bs)
    ks, vs = head_scales("gen", nkv)
    kf = kv8_ref.decode(c["kc"], ks.view(1, 1, -1, 1))
    vf = kv8_ref.decode(c["vc"], vs.view(1, 1, -1, 1))
    T = c["q"].shape[0]
    cu = c["cu"] if c["cu"] is not None else torch.arange(c["ctx"].numel() + 1, dtype=torch.int32) * c["qps"]
    ref = O.attn_paged(c["q"].view(T, nh, hd), kf, vf, c["ctx"], c["bt"], hd ** -0.5, cu_q=cu).reshape(T, nh * hd)
    got = run8(H, KV8, c, c["kc"], c["vc"], ks, vs, nh, nkv, hd, bs, 0)
    assert_close_bf16(got, ref, what=f"fp8 KV {kind} general scales", **ATTN_TOL)


@pytest.mark.parametrize("kind,nh,nkv,hd,bs,sk,flags", [e for e in EXACT if e[0] in ("decode", "verify", "varlen")])
def test_poisoned_cache_is_never_read(H, KV8, kind, nh, nkv, hd, bs, sk, flags):
    c = make_case(kind, nh, nkv, hd, bs)
    assert c["invalid"].any() and (c["kp"][c["invalid"]] == 0x7F).all() and (c["vp"][c["invalid"]] == 0x7F).all()
    ks, vs = head_scales(sk, nkv)
    clean = run8(H, KV8, c, c["kc"], c["vc"], ks, vs, nh, nkv, hd, bs, flags)
    pois = run8(H, KV8, c, c["kp"], c["vp"], ks, vs, nh, nkv, hd, bs, flags)
    assert torch.isfinite(pois.float()).all(), f"{kind}: a row past ctx or a page no sequence owns reached the output"
    assert torch.equal(bits(pois), bits(clean)), f"{kind}: the poisoned cache changed the output"


# ---------------------------------------------------------------------------------------------------------------------
# 5. store -> attention through one block table, eager and as one hipGraph replay
# ---------------------------------------------------------------------------------------------------------------------
def test_store_then_attention_eager_and_graph_replay(H, KV8):
    from ssd_amd.quant import kv_fp8_encode
    nh, nkv, hd, bs, nblocks = 8, 2, 128, 16, 6
    P, n = 37, 8                       # 37 cached keys, then 8 verify rows stored and attended over in the same graph
    T = P + n
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(T, (nh + 2 * nkv) * hd, generator=g).to(BF)
    table = [4, 1, 5, 0]
    slots = torch.tensor([table[p // bs] * bs + p % bs for p in range(T)], dtype=torch.int32)
    pos = torch.arange(T, dtype=torch.int64)
    cache = dev(O.make_cos_sin_cache(hd, 128, 10000.0))
    ks, vs = head_scales("pow2", nkv)
    ksd, vsd, kid, vid = dev(ks), dev(vs), dev(1.0 / ks), dev(1.0 / vs)
    bt = dev(torch.tensor([table], dtype=torch.int32))
    ctx = dev(torch.tensor([T], dtype=torch.int32))
    shape = (nblocks, nkv, bs, hd)
    k8 = torch.full(shape, 0x7F, dtype=torch.uint8, device="cuda")          # whatever is not stored stays NaN
    v8 = torch.full(shape, 0x7F, dtype=torch.uint8, device="cuda")
    qd, pd, sd = dev(qkv), dev(pos), dev(slots)
    qo = torch.zeros(T, nh * hd, dtype=BF, device="cuda")
    out = torch.zeros(n, nh * hd, dtype=BF, device="cuda")
    KV8.rope_store_kv_fp8(qd[:P], pd[:P], cache, sd[:P], qo[:P], k8, v8, P, nh, nkv, hd, bs, k_inv_scale=kid, v_inv_scale=vid)

    def step():
        KV8.rope_store_kv_fp8(qd[P:], pd[P:], cache, sd[P:], qo[P:], k8, v8, n, nh, nkv, hd, bs, k_inv_scale=kid, v_inv_scale=vid)
        KV8.attn_paged_fp8(qo[P:], k8, v8, bt, 4, ctx, 1, n, n, nh, nkv, hd, bs, hd ** -0.5, k_scale=ksd, v_scale=vsd, q_per_seq=n,
                           out_rows=out, waves=2)
    step()
    torch.cuda.synchronize()
    eager = out.clone()
    assert torch.isfinite(eager.float()).all()
    # the same through the bf16 kernels on bf16(s * code): bit-identical (power-of-two scales)
    kb = torch.zeros(shape, dtype=BF, device="cuda")
    vb = torch.zeros(shape, dtype=BF, device="cuda")
    qb = torch.zeros(T, nh * hd, dtype=BF, device="cuda")
    H.rope_store_kv(qd, pd, cache, sd, qb, kb, vb, T, nh, nkv, hd, bs)
    sk, sv = ks.view(1, -1, 1, 1), vs.view(1, -1, 1, 1)
    kq = kv8_ref.decode(kv_fp8_encode(kb.cpu(), 1.0 / sk), sk).to(BF)
    vq = kv8_ref.decode(kv_fp8_encode(vb.cpu(), 1.0 / sv), sv).to(BF)
    want = torch.zeros(n, nh * hd, dtype=BF, device="cuda")
    H.attn_paged(qb[P:], dev(kq), dev(vq), bt, 4, ctx, 1, n, n, nh, nkv, hd, bs, hd ** -0.5, q_per_seq=n, out_rows=want, waves=2)
    torch.cuda.synchronize()
    assert torch.equal(bits(eager.cpu()), bits(want.cpu()))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with H.CGraph(s) as gr:
            step()
        rows = [table[p // bs] * bs + p % bs for p in range(P, T)]
        for blk, off in {divmod(r, bs) for r in rows}:          # un-store the verify rows: the replay must write them again
            k8[blk, :, off] = 0x7F
            v8[blk, :, off] = 0x7F
        out.zero_()
        gr.launch()
        s.synchronize()
        assert torch.equal(bits(out), bits(eager))
        gr.destroy()
