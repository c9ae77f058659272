"""ssd_rope_store_kv / ssd_rope_store_kv_parts (csrc/rope.hip) at the edges tests/test_hip_ops.py does not visit: the default block
size 256 (and 64) next to 16, so that slot / bs and slot % bs see them; slots 0, bs - 1, bs and the cache's last; positions up to
8191; more items per token than one 512-thread workgroup holds (nh = 64, nkv = 8, hd = 128: 704 items, a second trip of the item loop,
with the head norm's shuffles inside it); hd = 256, which the launch accepts; the rotation-paired input order against the oracle rather
than against itself; and caches prefilled with a sentinel (bf16 NaN 0x7FC0) and compared WHOLE by bits, so that a store outside the
addressed rows shows -- over zeros a stray store of zeros does not.

Oracle: O.rmsnorm per head where there is a head norm, then O.rope, then O.store_kv into reference-layout caches prefilled alike.
Bars: without a head norm q, K and V are bit-exact (the kernel's separately rounded multiply / subtract is the oracle's arithmetic, as
in test_rope_store_golden); with one, q and K within 1 bf16 ulp on at most 1 % of the elements (test_rope_head_norm's bar: the sum of
squares is taken in another order) and every unaddressed row still the sentinel; V is bit-exact always."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import layout as LY
from oracle import ops as O
from tests.test_hip_fused import qkv_perm
from tests.test_hip_ops import BF, H, dev  # noqa: F401  (H is the fixture)
from tests.util import assert_close_bf16

SENTINEL = 0x7FC0
T, NB, EPS = 24, 4, 1e-6
EDGE_POS = [0, 1, 255, 256, 4095, 8191]
_COS_SIN = {}


def bits(t):
    return t.contiguous().view(torch.int16)


def sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16).view(BF)


def cos_sin(hd):
    if hd not in _COS_SIN:
        _COS_SIN[hd] = O.make_cos_sin_cache(hd, 8192, 5e5)
    return _COS_SIN[hd]


def make_case(nh, nkv, hd, bs, norm, seed):
    """Inputs shared by every form of one case, and the oracle's q / caches."""
    g = torch.Generator().manual_seed(seed)
    N = (nh + 2 * nkv) * hd
    S = 5
    parts = torch.randn(S, T, N, generator=g) * 0.5
    parts[:, 3, :64] = -0.0
    rows = {}
    for s in (1, 3, 5):                                       # fp32 sum of the first s slabs, in slab order
        acc = parts[0].clone()
        for z in range(1, s):
            acc = acc + parts[z]
        rows[s] = acc.to(BF)
    edge = [0, bs - 1, bs, NB * bs - 1]
    rest = [s for s in torch.randperm(NB * bs, generator=g).tolist() if s not in edge][:T - 5]
    slots = torch.tensor(edge + [-1] + rest, dtype=torch.int32)[torch.randperm(T, generator=g)]
    pos = torch.cat([torch.tensor(EDGE_POS), torch.randint(0, 8192, (T - 6,), generator=g)])[torch.randperm(T, generator=g)]
    qn, kn = ((1 + 0.1 * torch.randn(hd, generator=g)).to(BF), (1 + 0.1 * torch.randn(hd, generator=g)).to(BF)) if norm else (None, None)
    return parts, rows, slots, pos, qn, kn


def oracle(rows, slots, pos, qn, kn, nh, nkv, hd, bs):
    q, k, v = [t.contiguous() for t in rows.split([nh * hd, nkv * hd, nkv * hd], dim=1)]
    if qn is not None:
        q = O.rmsnorm(q.view(-1, hd), qn, EPS).view(T, nh * hd)
        k = O.rmsnorm(k.view(-1, hd), kn, EPS).view(T, nkv * hd)
    qr, kr = O.rope(pos, q, k, cos_sin(hd), hd)
    kref, vref = sentinel(NB, bs, nkv, hd), sentinel(NB, bs, nkv, hd)
    O.store_kv(kr.view(T, nkv, hd), v.view(T, nkv, hd), kref, vref, slots)
    return qr, kref, vref


def launch(H, fn, src, extra, slots, pos, qn, kn, nh, nkv, hd, bs, perm):
    q_out = sentinel(T, nh * hd).cuda()
    kc, vc = sentinel(NB, nkv, bs, hd).cuda(), sentinel(NB, nkv, bs, hd).cuda()
    fn(src, *extra, dev(pos), dev(cos_sin(hd)), dev(slots), q_out, kc, vc, T, nh, nkv, hd, bs,
       q_norm_w=None if qn is None else dev(qn), k_norm_w=None if kn is None else dev(kn), eps=EPS, qkv_perm=perm)
    torch.cuda.synchronize()
    return q_out.cpu(), LY.kv_hnd_to_nhd(kc.cpu()), LY.kv_hnd_to_nhd(vc.cpu())


def check(got, ref, slots, norm, what):
    (q, kc, vc), (qr, kref, vref) = got, ref
    assert torch.equal(bits(vc), bits(vref)), f"{what}: V cache"
    if not norm:
        assert torch.equal(bits(q), bits(qr)), f"{what}: q"
        assert torch.equal(bits(kc), bits(kref)), f"{what}: K cache"
        return
    assert_close_bf16(q, qr, max_ulp=1, max_frac=0.01, what=f"{what}: q")
    written = torch.zeros(kc.shape[0] * kc.shape[1], dtype=torch.bool)
    written[slots[slots >= 0].long()] = True
    kg, kr = kc.view(written.numel(), -1), kref.view(written.numel(), -1)
    assert torch.equal(bits(kg[~written]), bits(kr[~written])), f"{what}: a K row no slot addresses was written"
    assert_close_bf16(kg[written], kr[written], max_ulp=1, max_frac=0.01, what=f"{what}: K cache")


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("bs", [16, 64, 256])
@pytest.mark.parametrize("nh,nkv,hd", [(64, 8, 128), (4, 2, 64), (2, 1, 256)])
def test_rope_store_edges(H, nh, nkv, hd, bs, norm):
    parts, rows, slots, pos, qn, kn = make_case(nh, nkv, hd, bs, norm, seed=nh + hd + bs + norm)
    pidx = qkv_perm(nh, nkv, hd)
    refs = {s: oracle(rows[s], slots, pos, qn, kn, nh, nkv, hd, bs) for s in rows}
    for perm in (0, 1):
        shuffle = (lambda t: t[..., pidx].contiguous()) if perm else (lambda t: t)
        arg = (slots, pos, qn, kn, nh, nkv, hd, bs, perm)
        for s in (1, 3, 5):
            what = f"heads {nh}/{nkv}x{hd} bs{bs} norm{int(norm)} perm{perm} S{s}"
            from_rows = launch(H, H.rope_store_kv, dev(shuffle(rows[s])), (), *arg)
            check(from_rows, refs[s], slots, norm, what + " rows form")
            from_parts = launch(H, H.rope_store_kv_parts, dev(shuffle(parts[:s])), (s,), *arg)
            check(from_parts, refs[s], slots, norm, what + " parts form")
            for a, b in zip(from_rows, from_parts):
                assert torch.equal(bits(a), bits(b)), f"{what}: the parts form differs from the rows form"
