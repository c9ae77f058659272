"""The LoRA kernels on the MI355X through the C ABI (csrc/lora.hip, include/ssd_hip_lora.h): ssd_lora_shrink and ssd_lora_expand
against the float64 reference of tests/lora_ref.py.

Outputs and workspaces are filled with a sentinel before every launch, the padding rows of x_frag are bf16 NaN.  Bars (lora_ref):
t (the slab sum rounded to bf16) within 1 bf16 ulp of float64, differences below 2^-20 * sum|x a| exempt; y against float64 computed
from the kernel's OWN t, the same bar with |y0| + scale * sum|t b| in the floor.  Rows without a slot keep their bits."""
import itertools

import pytest
import torch

from tests import lora_ref as LR

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
MS = (1, 7, 16, 17, 24, 33, 130)
KS = (64, 2080, 2048)
RS = (32, 64, 96, 192)
NS = (16, 48, 2064)
SLOTS = (1, 4)
SENT = 0x7fc1          # a bf16 NaN pattern no kernel produces (f2bf quiets to ...40)
SCALES = (2.0, 0.53125, 1.28125, 3.09375)


def _cases():
    """Every (M, K) pair and every (R, N, slots) triple of the grid, the other parameters cycling, so that every value meets every
    other at least along these two faces (the full product is 1512 shapes)."""
    out, seen = [], set()
    tri = list(itertools.product(RS, NS, SLOTS))
    for i, (M, K) in enumerate(itertools.product(MS, KS)):
        out.append((M, K) + tri[(5 * i) % len(tri)])
    for i, t in enumerate(tri):
        out.append((MS[i % len(MS)], KS[i % len(KS)]) + t)
    out.append((24, 2048, 64, 48, 4))                           # the three 8-row runs need 24 rows and four slots
    return [c for c in out if not (c in seen or seen.add(c))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda")


def _frag(rows: torch.Tensor) -> torch.Tensor:
    from ssd_amd.hip import ops as H
    R, K = rows.shape
    out = torch.empty(H.frag_numel(R, K), dtype=BF, device=rows.device)
    H.rows_to_frag(rows.contiguous(), out, R, K)
    return out


def _tables(mats: torch.Tensor) -> torch.Tensor:
    """[slots, R, K] -> the slot table: one fragment-major matrix after the other."""
    return torch.cat([_frag(m) for m in mats])


def _sentinel(n, dev, dtype=torch.int16):
    if dtype == torch.float32:
        return torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    return torch.full((n,), SENT, dtype=torch.int16, device=dev)


def _patterns(M: int, slots: int):
    pats = {"none": [-1] * M, "one": [slots - 1] * M, "alternating": [m % slots for m in range(M)],
            "holes": [(-1 if m % 3 == 1 else (m // 2) % slots) for m in range(M)]}
    if M == 24 and slots == 4:
        pats["runs"] = [m // 8 + 1 for m in range(M)]           # three 8-row runs, one slot each: every tile mixes two slots
    if slots == 4:
        pats["out_of_range"] = [(7 if m % 4 == 2 else (-5 if m % 4 == 3 else m % slots)) for m in range(M)]
    return pats


class _Data:
    def __init__(self, M, K, R, N, slots, dev, ldy=None):
        g = torch.Generator(device=dev).manual_seed(M * 7 + K + R * 3 + N + slots)
        self.M, self.K, self.R, self.N, self.slots, self.dev = M, K, R, N, slots, dev
        Mp = -(-M // 16) * 16
        self.x = torch.randn(M, K, generator=g, device=dev).to(BF)
        xr = torch.full((Mp, K), float("nan"), dtype=BF, device=dev)
        xr[:M] = self.x
        self.xf = _frag(xr)
        self.A = (torch.randn(slots, R, K, generator=g, device=dev) / K ** 0.5).to(BF)
        self.B = (torch.randn(slots, N, R, generator=g, device=dev) / R ** 0.5).to(BF)
        self.af, self.bf = _tables(self.A), _tables(self.B)
        self.scale = torch.tensor(SCALES[:slots], dtype=torch.float32, device=dev)
        self.y0 = torch.randn(M, N, generator=g, device=dev).to(BF)
        self.ldy = N if ldy is None else ldy

    def run(self, row_slot, splits, epilogue=0):
        """-> (ws fp32 [Smax + 1 slab of sentinel], y int16 [M + 3][ldy], act int16 or None, S)"""
        from ssd_amd.hip import lora_ops as L
        M, K, R, N = self.M, self.K, self.R, self.N
        S = splits or L.lora_default_splits(K)
        rs = torch.tensor(row_slot, dtype=torch.int32, device=self.dev)
        ws = _sentinel(S * M * R + 64, self.dev, torch.float32)
        y = _sentinel((M + 3) * self.ldy, self.dev).view(M + 3, self.ldy)
        y[:M, :N] = self.y0.view(torch.int16)
        act = _sentinel(-(-M // 16) * 16 * (N // 2), self.dev) if epilogue else None
        L.lora_shrink(self.xf, self.af, rs, ws, M, K, R, self.slots, splits)
        L.lora_expand(ws, self.bf, self.scale, rs, y, self.ldy, M, N, K, R, self.slots, splits, epilogue, act)
        torch.cuda.synchronize()
        return ws, y, act, S, rs

    def check(self, row_slot, splits, what):
        M, K, R, N = self.M, self.K, self.R, self.N
        ws, y, _, S, rs = self.run(row_slot, splits)
        sane = LR.sane_slots(rs, self.slots)
        on = sane >= 0
        slabs = ws[:S * M * R].view(S, M, R)
        assert bool(torch.isnan(ws[S * M * R:]).all()), f"{what}: the shrink wrote past its slabs"
        assert bool(torch.isnan(slabs[:, ~on]).all()), f"{what}: a row without a slot was written"
        assert not bool(torch.isnan(slabs[:, on]).any()), f"{what}: a slab entry of an adapted row was not written (or NaN leaked in)"
        acc = slabs[0].clone()
        for s in range(1, S):
            acc += slabs[s]                                    # fp32, slab order: the expand's own sum
        t = torch.where(on[:, None], acc, torch.zeros_like(acc)).to(BF)
        t64, tmag = LR.shrink_exact(self.x, self.A, rs)
        LR.assert_within_bar(t[on], t64[on], tmag[on], f"{what} t")
        want, mag = LR.expand_exact(self.y0, t, self.B, self.scale, rs)
        got = y[:M, :N].view(BF)
        LR.assert_within_bar(got[on], want[on], mag[on], f"{what} y")
        assert torch.equal(y[:M, :N][~on], self.y0.view(torch.int16)[~on]), f"{what}: a row without a slot changed"
        assert bool((y[M:] == SENT).all()) and bool((y[:, N:] == SENT).all()), f"{what}: a write outside [M][N]"
        if bool(on.any()):
            assert not torch.equal(got[on], self.y0[on]), f"{what}: the delta was not applied"
        return ws, y


@pytest.mark.parametrize("M,K,R,N,slots", _cases())
def test_shrink_expand_against_float64(dev, M, K, R, N, slots):
    from ssd_amd.hip import lora_ops as L
    d = _Data(M, K, R, N, slots, dev, ldy=N + 2 if (M + K + R) % 64 == 0 and N > 16 else None)
    assert 1 <= L.lora_default_splits(K) <= min(16, K // 32)
    assert L.lora_workspace_bytes(M, K, R) == min(16, K // 32) * M * R * 4
    for name, pat in _patterns(M, slots).items():
        for splits in (1, 0, min(16, K // 32)):
            d.check(pat, splits, f"M={M} K={K} R={R} N={N} slots={slots} {name} splits={splits}")


def test_unaligned_row_pitch(dev):
    """ldy % 4 != 0: the rows are read and written two bytes at a time."""
    d = _Data(17, 64, 32, 48, 4, dev, ldy=51)
    d.check(_patterns(17, 4)["holes"], 0, "ldy=51")


def test_two_runs_give_equal_bits(dev):
    d = _Data(24, 2080, 64, 2064, 4, dev)
    pat = _patterns(24, 4)["runs"]
    assert sorted(set(pat)) == [1, 2, 3]
    a = d.run(pat, 0)
    b = d.run(pat, 0)
    on = LR.sane_slots(a[4], 4) >= 0
    S = a[3]
    assert torch.equal(a[0][:S * 24 * 64].view(S, 24, 64)[:, on].view(torch.int32), b[0][:S * 24 * 64].view(S, 24, 64)[:, on].view(torch.int32))
    assert torch.equal(a[1], b[1])


@pytest.mark.parametrize("M,K,R,N,slots", [(1, 64, 32, 64, 1), (17, 2080, 96, 192, 4), (24, 2048, 64, 2112, 4), (33, 64, 192, 64, 4),
                                           (130, 2048, 32, 192, 1)])
def test_silu_epilogue_equals_silu_mul_of_the_updated_rows(dev, M, K, R, N, slots):
    """Epilogue 1 = ssd_silu_mul of the de-interleaved epilogue-0 rows, by bits, for every row (with and without a slot)."""
    from ssd_amd.hip import ops as H
    d = _Data(M, K, R, N, slots, dev)
    for name, pat in _patterns(M, slots).items():
        _, y, _, _, _ = d.run(pat, 0, epilogue=0)
        _, y1, act, _, _ = d.run(pat, 0, epilogue=1)
        assert torch.equal(y1[:M, :N], d.y0.view(torch.int16)), "epilogue 1 leaves y as it was"
        upd = y[:M, :N].reshape(M, N // 32, 2, 16)             # packed order: alternating 16-column groups (gate, up)
        rows = torch.cat([upd[:, :, 0].reshape(M, N // 2), upd[:, :, 1].reshape(M, N // 2)], dim=1).contiguous()
        want = _sentinel(act.numel(), dev)
        H.silu_mul(rows, M, N // 2, out_frag=want)
        torch.cuda.synchronize()
        assert torch.equal(act, want), f"M={M} N={N} {name}"


def test_refusals(dev):
    from ssd_amd.hip import lora_ops as L
    from ssd_amd.hip.lib import SsdHipError
    M, K, R, N, slots = 8, 64, 32, 64, 2
    d = _Data(M, K, R, N, slots, dev)
    rs = torch.zeros(M, dtype=torch.int32, device=dev)
    ws = torch.zeros(2 * M * R, dtype=torch.float32, device=dev)
    y = d.y0.clone()
    act = torch.zeros(16 * N // 2, dtype=BF, device=dev)

    def shrink(**kw):
        a = dict(x_frag=d.xf, a_frag=d.af, row_slot=rs, ws=ws, M=M, K=K, R=R, slots=slots, splits=0)
        a.update(kw)
        L.lora_shrink(**a)

    def expand(**kw):
        a = dict(ws=ws, b_frag=d.bf, scale=d.scale, row_slot=rs, y=y, ldy=N, M=M, N=N, K=K, R=R, slots=slots, splits=0, epilogue=0,
                 act_frag=None)
        a.update(kw)
        L.lora_expand(**a)

    shrink()
    expand()
    expand(epilogue=1, act_frag=act)
    torch.cuda.synchronize()
    for kw in (dict(x_frag=None), dict(a_frag=None), dict(row_slot=None), dict(ws=None), dict(K=48), dict(R=16), dict(R=48), dict(R=224),
               dict(splits=-1), dict(splits=17), dict(splits=3), dict(slots=0), dict(M=0), dict(ws=ws[:2 * M * R - 1], splits=2),
               dict(ws=ws[:M * R - 1])):
        with pytest.raises(SsdHipError):
            shrink(**kw)
    for kw in (dict(ws=None), dict(b_frag=None), dict(scale=None), dict(row_slot=None), dict(y=None), dict(K=48), dict(R=16), dict(R=224),
               dict(N=24), dict(ldy=N - 16), dict(epilogue=1), dict(epilogue=1, act_frag=act, N=48, ldy=48), dict(epilogue=2),
               dict(splits=17), dict(splits=3), dict(slots=0), dict(ws=ws[:M * R - 1])):
        with pytest.raises(SsdHipError):
            expand(**kw)
    assert L.lora_default_splits(48) == 0 and L.lora_workspace_bytes(8, 64, 224) == 0
    torch.cuda.synchronize()
