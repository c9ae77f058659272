"""Sliding-window paged attention (include/ssd_hip_swa.h) on the GPU, through the C ABI: ssd_attn_paged_window and its fp8-cache twin
against a float64 SDPA under the mask lim - W <= key < lim, at the smallest shapes at which the windowed walk can go wrong -- the
window start on and beside a 32-key tile edge and a page edge, fewer tiles than (split, wave) shares, every verify row with its own
edge, a prefill whose row tiles each have their own first tile.  Every launch also runs over a cache whose rows and pages in front of
the window are NaN: never read.  Every case is at most 300 keys."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import layout as LY
from tests import kv8_ref
from tests.test_hip_ops import ATTN_TOL, BF, H, dev, make_paged_poisoned, run_attn_dev  # noqa: F401  (H is the fixture)
from tests.util import assert_close_bf16


@pytest.fixture(scope="module")
def SWA(H):
    from ssd_amd.hip import swa_ops
    swa_ops.load_swa_library()
    return swa_ops


def bits(t):
    return t.contiguous().view(torch.int16)


class WinAttn:
    """What run_attn_dev needs of `ops`, with attn_paged going to the windowed entry (over an fp8 cache when scales are given)."""

    def __init__(self, H, SWA, window, scales=None):
        self.frag_numel = H.frag_numel
        self.SWA, self.window, self.scales = SWA, window, scales

    def attn_paged(self, *a, **kw):
        if self.scales is None:
            return self.SWA.attn_paged_window(*a, window=self.window, **kw)
        self.SWA.attn_paged_fp8_window(*a, k_scale=dev(self.scales[0]), v_scale=dev(self.scales[1]), window=self.window, **kw)


def sdpa_window_f64(q, kc, vc, bt, ctx, cu, W, nh, nkv, hd, bs):
    """float64 attention of the packed rows q [T, nh, hd] over the paged cache (reference layout [page][row][kv head][d]); row t of
    sequence b, causal limit lim = ctx_b - (Tq_b - 1 - t), sees the keys lim - W <= key < lim."""
    out = torch.zeros(q.shape[0], nh, hd, dtype=torch.float64)
    for b, L in enumerate(ctx.tolist()):
        rows = slice(int(cu[b]), int(cu[b + 1]))
        slots = (bt[b].long().view(-1, 1) * bs + torch.arange(bs)).view(-1)[:L]
        k = kc.reshape(-1, nkv, hd)[slots].double().repeat_interleave(nh // nkv, 1)
        v = vc.reshape(-1, nkv, hd)[slots].double().repeat_interleave(nh // nkv, 1)
        lim = (L - (rows.stop - rows.start - 1) + torch.arange(rows.stop - rows.start)).view(-1, 1)
        key = torch.arange(L).view(1, -1)
        s = torch.einsum("thd,lhd->htl", q[rows].double(), k) * hd ** -0.5
        s = s.masked_fill(~((key < lim) & (key >= lim - W)), float("-inf"))
        out[rows] = torch.einsum("htl,lhd->thd", s.softmax(-1), v)
    return out.reshape(q.shape[0], nh * hd)


def poison_front(kp, vp, bt, ctx, qlens, W, bs):
    """On top of make_paged_poisoned: every row with key < lo_b = max(0, lim of b's first query row - W) is NaN, and the block-table
    entries of the pages wholly in front of lo_b name the all-NaN page (the last column of the table always does)."""
    kp, vp, bt2 = kp.clone(), vp.clone(), bt.clone()
    poison = int(bt[0, -1])
    for b, (L, tq) in enumerate(zip(ctx.tolist(), qlens)):
        lo = max(0, L - (tq - 1) - W)
        slots = (bt[b].long().view(-1, 1) * bs + torch.arange(bs)).view(-1)[:lo]
        kp.view(-1, *kp.shape[2:])[slots] = float("nan")
        vp.view(-1, *vp.shape[2:])[slots] = float("nan")
        bt2[b, :lo // bs] = poison
    return kp, vp, bt2


PREFILL = dict(ctx=[150, 60, 90], qlens=[150, 37, 5])       # 300 rows at G = 2: 19 row tiles, two per workgroup unless flag bit 2
# W, ctx lens, queries per sequence (or PREFILL), (waves, splits), (nh, nkv, hd), flags, block size
CASES = [
    (1, [1, 2, 34], 1, (1, 1), (32, 8, 64), 0, 16),
    (1, [32, 19, 300], 8, (8, 3), (16, 8, 128), 0, 16),
    (16, [15, 16, 17], 1, (8, 3), (32, 8, 64), 0, 16),          # one tile for 24 shares
    (16, [47, 49, 300], 8, (1, 3), (16, 8, 128), 0, 16),
    (17, [16, 18, 48], 8, (8, 1), (16, 8, 128), 0, 16),
    (17, [50, 51, 300], 1, (1, 1), (32, 8, 64), 0, 16),
    (32, [31, 32, 33], 1, (1, 3), (16, 8, 128), 0, 16),
    (32, [63, 65, 81], 8, (8, 3), (32, 8, 64), 0, 16),
    (33, [32, 34, 64], 8, (1, 1), (32, 8, 64), 0, 16),
    (33, [66, 83, 300], 1, (8, 1), (16, 8, 128), 0, 16),
    (100, [99, 100, 101], 8, (8, 3), (16, 8, 128), 0, 16),
    (100, [131, 133, 217], 1, (1, 3), (32, 8, 64), 0, 16),
    (100, [300, 217, 133], 8, (8, 1), (32, 8, 64), 0, 16),
    (40, PREFILL, None, (2, 1), (16, 8, 128), 0, 16),
    (40, PREFILL, None, (2, 1), (16, 8, 128), 4, 16),
    (40, PREFILL, None, (1, 3), (32, 8, 64), 4, 16),
    (33, [66, 83, 300], 8, (8, 3), (16, 8, 128), 0, 256),
]
_CACHE = {}


def make_case(ctx, qps, heads, bs):
    """q, the clean and the make_paged_poisoned caches, the table, cu_q.  Built once per shape and shared, never modified."""
    nh, nkv, hd = heads
    lens, qlens = (ctx["ctx"], ctx["qlens"]) if qps is None else (ctx, [qps] * len(ctx))
    key = (tuple(lens), tuple(qlens), heads, bs)
    if key not in _CACHE:
        kc, vc, kp, vp, bt, mb = make_paged_poisoned(len(lens), lens, nkv, hd, bs, seed=sum(lens) + hd + bs)
        g = torch.Generator().manual_seed(sum(qlens) + nh)
        cu = torch.tensor([0] + qlens, dtype=torch.int32).cumsum(0).to(torch.int32)
        _CACHE[key] = dict(q=torch.randn(sum(qlens), nh * hd, generator=g).to(BF), kc=kc, vc=vc, kp=kp, vp=vp, bt=bt, mb=mb, cu=cu,
                           ctx=torch.tensor(lens, dtype=torch.int32), qlens=qlens)
    return _CACHE[key]


def launch(ops, c, k, v, bt, heads, bs, qps, waves, splits, flags):
    nh, nkv, hd = heads
    return run_attn_dev(ops, c["q"], dev(LY.kv_nhd_to_hnd(k)), dev(LY.kv_nhd_to_hnd(v)), bt, c["mb"], c["ctx"], nh, nkv, hd, bs,
                        cu_q=c["cu"] if qps is None else None, q_per_seq=qps or 0, splits=splits, flags=flags, waves=waves)


@pytest.mark.parametrize("W,ctx,qps,ws,heads,flags,bs", CASES)
def test_window_against_float64_and_front_of_window_never_read(H, SWA, W, ctx, qps, ws, heads, flags, bs):
    c = make_case(ctx, qps, heads, bs)
    ref = sdpa_window_f64(c["q"].view(-1, heads[0], heads[2]), c["kc"], c["vc"], c["bt"], c["ctx"], c["cu"], W, *heads, bs)
    ops = WinAttn(H, SWA, W)
    clean = launch(ops, c, c["kc"], c["vc"], c["bt"], heads, bs, qps, *ws, flags)
    kp, vp, bt2 = poison_front(c["kp"], c["vp"], c["bt"], c["ctx"], c["qlens"], W, bs)
    pois = launch(ops, c, kp, vp, bt2, heads, bs, qps, *ws, flags)
    assert torch.isfinite(pois.float()).all(), "a row or a page in front of the window, or past ctx, reached the output"
    assert torch.equal(bits(pois), bits(clean)), "the poisoned cache changed the output"
    assert_close_bf16(pois, ref.to(BF), what=f"W{W} ctx{c['ctx'].tolist()} q{qps} (waves, splits) {ws}", **ATTN_TOL)


@pytest.mark.parametrize("W,ctx,qps,ws,heads,flags,bs", [CASES[3], CASES[7]])
def test_fp8_cache_twin_is_bit_identical_to_the_bf16_window_kernel(H, SWA, W, ctx, qps, ws, heads, flags, bs):
    """Power-of-two scales: bf16(scale * code) is exact and commutes with every rounding, as in tests/test_hip_kv8.py."""
    c = dict(make_case(ctx, qps, heads, bs))
    nkv = heads[1]
    g = torch.Generator().manual_seed(W)
    c["q"] = (torch.randn(c["q"].shape, generator=g) * 0.02).to(BF)
    k8 = kv8_ref.FINITE_CODES[torch.randint(0, 254, c["kc"].shape, generator=g)]
    v8 = kv8_ref.FINITE_CODES[torch.randint(0, 254, c["kc"].shape, generator=g)]
    ks = torch.tensor([[0.5, 2.0, 4.0][h % 3] for h in range(nkv)])
    vs = torch.tensor([[2.0, 4.0, 0.5][h % 3] for h in range(nkv)])
    kb, vb = kv8_ref.decode(k8, ks.view(1, 1, -1, 1)).to(BF), kv8_ref.decode(v8, vs.view(1, 1, -1, 1)).to(BF)
    want = launch(WinAttn(H, SWA, W), c, kb, vb, c["bt"], heads, bs, qps, *ws, flags)
    kp, vp, bt2 = poison_front(c["kp"], c["vp"], c["bt"], c["ctx"], c["qlens"], W, bs)
    nan = torch.isnan(kp[..., 0, 0].float())                 # [page][row]: not owned, or in front of the window
    k8[nan], v8[nan] = 0x7F, 0x7F
    got = launch(WinAttn(H, SWA, W, (ks, vs)), c, k8, v8, bt2, heads, bs, qps, *ws, flags)
    assert got.float().abs().max() > 0
    assert torch.equal(bits(got), bits(want)), f"{(bits(got) != bits(want)).sum().item()} elements differ from the bf16 window kernel"


@pytest.mark.parametrize("W,case", [(300, CASES[1]), (2 ** 31 - 1, CASES[12]), (150, CASES[14])])
def test_a_window_that_cuts_nothing_off_is_bit_identical_to_the_unwindowed_kernel(H, SWA, W, case):
    _, ctx, qps, ws, heads, flags, bs = case
    c = make_case(ctx, qps, heads, bs)
    want = launch(H, c, c["kp"], c["vp"], c["bt"], heads, bs, qps, *ws, flags)
    got = launch(WinAttn(H, SWA, W), c, c["kp"], c["vp"], c["bt"], heads, bs, qps, *ws, flags)
    assert torch.equal(bits(got), bits(want))
    zero = launch(WinAttn(H, SWA, 0), c, c["kp"], c["vp"], c["bt"], heads, bs, qps, *ws, flags)      # window 0 forwards
    assert torch.equal(bits(zero), bits(want))


@pytest.mark.parametrize("kw", [dict(window=-1), dict(window=16, mode=1, tree_mq=1, tree_F=1)])
def test_refusals_return_err_arg_and_launch_nothing(H, SWA, kw):
    from ssd_amd.hip.lib import SsdHipError
    _, ctx, qps, ws, heads, flags, bs = CASES[0]
    nh, nkv, hd = heads
    c = make_case(ctx, qps, heads, bs)
    out = torch.full((c["q"].shape[0], nh * hd), 7.0, dtype=BF, device="cuda")
    args = (dev(c["q"]), dev(LY.kv_nhd_to_hnd(c["kc"])), dev(LY.kv_nhd_to_hnd(c["vc"])), dev(c["bt"]), c["mb"], dev(c["ctx"]), 3, 3, 1,
            nh, nkv, hd, bs, hd ** -0.5)
    with pytest.raises(SsdHipError, match="code -3"):
        SWA.attn_paged_window(*args, q_per_seq=1, out_rows=out, **kw)
    if "mode" not in kw:
        with pytest.raises(SsdHipError, match="code -3"):
            SWA.attn_paged_fp8_window(*args, q_per_seq=1, out_rows=out, **kw)
    else:
        with pytest.raises(SsdHipError, match="code -3"):
            SWA.attn_paged_fp8_window(*args, q_per_seq=1, out_rows=out, window=16, mode=1)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full_like(out, 7.0).cpu())
