"""The norm, activation and embedding kernels of csrc/norm.hip at the edges tests/test_hip_ops.py does not visit: every H at which
rmsnorm_kernel changes its trip count or its thread count (fewer chunks than one wave, one chunk short of / at / one past a full trip of
256 threads, both sides of the 256 / 1024-thread switch at H = 4096, a ragged second trip of 1024 threads, NORM_MAXH); every slab count
class of ssd_rmsnorm_parts (the clamped odd counts and the S > 8 second pass); the in-place residual (res_in == res_out, as the engine
calls it, although both kernel parameters are __restrict__) against the out-of-place call, bit for bit; ssd_rmsnorm_pair with halves of
different magnitude; ssd_head_rmsnorm around one workgroup of 256 items; ssd_silu_mul on the saturation side of __expf; ssd_embedding at
one chunk and at more than one trip, with ids on both borders of the shard -- and the refusals of every entry point.

Reference: float64 on the bf16 operand values with the kernel's rounding points.  The residual sum is bf16(fp32(x) + fp32(res)): one fp32
add, bit-exact on the CPU.  The norm runs on the UNROUNDED fp32 sum (rmsnorm_kernel keeps it in v[][] and writes the rounded one to
res_out): y = bf16(r64 * rsqrt(mean(r64^2) + eps) * w64).

Bar, every element, none exempt: |HIP - bf16(f64)| <= 1 bf16 ulp (sign-magnitude distance of the two bit patterns).  The fp32 result is
within a few 2^-24 of the exact one (two products, one rsqrt, and a sum of squares of at most 16384 terms taken as a tree), far less than
half a bf16 ulp (2^-9), so the two roundings are equal or adjacent.  The share that differs is printed, not asserted.

Every output is prefilled with the bf16 NaN 0x7FC0, allocated with rows past T and a fragment tail, and compared there by bits.  The rows
of every input hold, in turn: magnitude 2^-10 (mean square ~ eps: a missing eps or a wrong divisor shows, see the unmarked sensitivity
test), zeros, magnitude 2^20, N(0, 1) with one spike of 2^12, N(0, 1).  The case tables are plain Python; the unmarked tests check what
they cover, the GPU tests run them."""
from __future__ import annotations

from typing import NamedTuple

import pytest
import torch

from oracle import layout as LY
from oracle import ops as O
from tests.test_hip_bf16_edges import TAIL, ceil16
from tests.test_hip_mxfp4 import assert_within_ulp, dev  # noqa: F401  (dev is the fixture)
from tests.test_hip_quant_edges import SENTINEL, _bits

gpu = pytest.mark.gpu
BF = torch.bfloat16
EPS = 1e-6
PAD_ROWS = 3                    # sentinel rows past T in every row-major output
NORM_MAXH = 16384
NORM_H = (32, 64, 224, 256, 2016, 2048, 2080, 4064, 4096, 4128, 8192, 12320, 16384)
NORM_H_REFUSED = (16416, 24)
ROW_KINDS = ("small", "zero", "big", "spike", "plain", "plain")
PARTS_S = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16)
PAIR_T = (1, 16, 17, 33)
SHARD = (100, 37)               # vocab_start, vocab_count of the embedding shard


def norm_threads(H: int) -> int:
    return 1024 if H >= 4096 else 256


# ---------------------------------------------------------------------------------------------------------------------
# Bars, sentinels, reports
# ---------------------------------------------------------------------------------------------------------------------
def key(t: torch.Tensor) -> torch.Tensor:
    """bf16 bit patterns on a line: adjacent values differ by 1, +0 and -0 coincide."""
    x = t.contiguous().view(torch.int16).int()
    return torch.where(x < 0, -(x & 0x7FFF), x)


def report(test: str, kind: str, ratio: float, share: float | None = None):
    print(f"norm_fused_edges | {test} | {kind} | worst {ratio:.2f} x bar" + ("" if share is None else f" | {share:.4f} of elements differ"))


def assert_1ulp(got: torch.Tensor, want64: torch.Tensor, what: str):
    """Every element of `got` (bf16) within 1 bf16 ulp of bf16(want64); returns (worst distance in ulp, share that differs)."""
    got = got.cpu()
    assert got.shape == want64.shape, (got.shape, want64.shape)
    assert bool(torch.isfinite(got.float()).all()), f"{what}: a non-finite output (or one left unwritten)"
    d = (key(got) - key(want64.to(BF))).abs()
    worst, share = int(d.max()), float((d > 0).float().mean())
    assert worst <= 1, f"{what}: {int((d > 1).sum())} outputs beyond 1 ulp of bf16(f64), worst {worst} ulp"
    return float(worst), share


def sentinel(*shape, device="cpu"):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device=device).view(BF)


def is_sentinel(t: torch.Tensor) -> bool:
    return bool((_bits(t) == SENTINEL).all())


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


# ---------------------------------------------------------------------------------------------------------------------
# Inputs and the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def scale_rows(t: torch.Tensor, spike: bool = True) -> torch.Tensor:
    """Row i of an N(0, 1) matrix becomes ROW_KINDS[i % 6]."""
    t = t.clone()
    for i in range(t.shape[0]):
        kind = ROW_KINDS[i % len(ROW_KINDS)]
        if kind == "small":
            t[i] *= 2.0 ** -10
        elif kind == "zero":
            t[i] = 0.0
        elif kind == "big":
            t[i] *= 2.0 ** 20
        elif kind == "spike" and spike:
            t[i, t.shape[1] // 3] = 4096.0
    return t


def norm_weight(H: int, g: torch.Generator) -> torch.Tensor:
    w = 1 + 0.1 * torch.randn(H, generator=g)
    w[1] = -w[1]
    return w.to(BF)


def norm_inputs(T: int, H: int, seed: int):
    """x, res [T, H] and w [H] in bf16."""
    g = torch.Generator().manual_seed(seed)
    x = scale_rows(torch.randn(T, H, generator=g)).to(BF)
    r = scale_rows(torch.randn(T, H, generator=g), spike=False).to(BF)
    return x, r, norm_weight(H, g)


def norm_ref64(x, w, eps, res=None, drop_eps=False, div_extra=0):
    """(y in float64, the residual the kernel stores) -- with two deliberate mistakes on request, for the sensitivity test."""
    s32 = x.float() if res is None else x.float() + res.float()
    r64 = s32.double()
    ms = r64.pow(2).sum(-1, keepdim=True) / (x.shape[-1] + div_extra)
    return r64 * torch.rsqrt(ms + (0.0 if drop_eps else eps)) * w.double(), s32.to(BF)


def slab_sum(parts: torch.Tensor, S: int) -> torch.Tensor:
    """bf16 of the fp32 sum of the first S slabs in slab order, starting from zero as the kernels do."""
    acc = torch.zeros_like(parts[0])
    for z in range(S):
        acc = acc + parts[z]
    return acc.to(BF)


def check_zero_rows(y: torch.Tensor, what: str):
    for i in range(y.shape[0]):
        if ROW_KINDS[i % len(ROW_KINDS)] == "zero":
            assert bool((y[i].float() == 0).all()), f"{what}: the row of zeros did not come out as zeros"


@pytest.mark.parametrize("H", [32, 64])
def test_reference_sees_a_dropped_eps_and_a_wrong_divisor(H):
    """On the reference alone: in the row of magnitude 2^-10 the mean square is about eps (2^-20 against 1e-6), so dropping eps
    multiplies the row by about sqrt(2), and dividing by H + 8 instead of H (a row padded to the next chunk) at H = 32 / 64 moves
    mean + eps by 10 % / 5 % -- both at least 2 ulp on at least half of the row, which the GPU bar of 1 ulp cannot let through.
    (At H >= 224 the divisor mistake is below 1 % of the mean and no longer 2 ulp: the small H of NORM_H carry that check.)"""
    x, r, w = norm_inputs(6, H, seed=H)
    assert ROW_KINDS[0] == "small"
    for res in (None, r):
        good = key(norm_ref64(x, w, EPS, res)[0].to(BF))[0]
        for what, kw in (("eps dropped", dict(drop_eps=True)), ("divisor H + 8", dict(div_extra=8))):
            moved = (key(norm_ref64(x, w, EPS, res, **kw)[0].to(BF))[0] - good).abs() >= 2
            assert float(moved.float().mean()) >= 0.5, f"H {H} {what}: only {float(moved.float().mean()):.2f} of the small row moves by 2 ulp"


@pytest.mark.parametrize("H", NORM_H)
def test_reference_sees_a_dropped_eps_at_every_h(H):
    x, _, w = norm_inputs(1, H, seed=H)
    moved = (key(norm_ref64(x, w, EPS, drop_eps=True)[0].to(BF)) - key(norm_ref64(x, w, EPS)[0].to(BF))).abs() >= 2
    assert float(moved.float().mean()) >= 0.5


# =====================================================================================================================
# ssd_rmsnorm / ssd_rmsnorm_parts
# =====================================================================================================================
class NormCase(NamedTuple):
    H: int
    T: int
    res_in: bool
    res_out: bool
    rows: bool
    frag: bool
    gather: bool     # T_out = 9 rows gathered from the T input rows, repeated and descending
    S: int           # 0: ssd_rmsnorm; else ssd_rmsnorm_parts over S slabs
    slab_pad: int    # slab_rows - T


GATHER = (5, 5, 3, 2, 1, 0, 0, 4, 2)


def norm_table() -> list[NormCase]:
    t: list[NormCase] = []
    for H in NORM_H:
        T = 6
        t.append(NormCase(H, T, True, True, True, True, False, 0, 0))        # the engine's form, plus both outputs
        t.append(NormCase(H, T, False, False, True, False, False, 0, 0))     # norm_forward: rows only
        t.append(NormCase(H, T, True, False, False, True, False, 0, 0))      # res_in without res_out, fragment only
        t.append(NormCase(H, T, False, True, True, True, False, 0, 0))       # res_out without res_in: a copy of x
        t.append(NormCase(H, T, True, False, False, True, True, 0, 0))       # gather, T_out != T_in, fragment
        t.append(NormCase(H, T, False, False, True, True, True, 0, 0))
    for H in (256, 2080, 4096, 16384):
        for T in (1, 17, 33):
            t.append(NormCase(H, T, True, True, True, True, False, 0, 0))
    # parts: every S with both slab strides at a ragged H on each side of the thread switch; elsewhere S walks the list
    for H in (2080, 4128):
        for S in PARTS_S:
            for pad in (0, 3):
                t.append(NormCase(H, 6, True, True, True, True, False, S, pad))
    for i, H in enumerate(NORM_H):
        for j in (0, 1):
            S = PARTS_S[(2 * i + j) % len(PARTS_S)]
            t.append(NormCase(H, 6 if j else 17, bool(j), True, bool(j), True, False, S, 3 * j))
    return [c for i, c in enumerate(t) if c not in t[:i]]


def test_norm_case_table_covers_every_trip_count_and_every_slab_class():
    t = norm_table()
    assert len(set(t)) == len(t) and all(1 <= c.T <= 33 and c.H % 32 == 0 and c.H <= NORM_MAXH for c in t)
    assert {c.H for c in t if not c.S} == set(NORM_H) == {c.H for c in t if c.S}
    chunks = lambda H: H // 8                                          # noqa: E731
    assert any(chunks(H) < 64 for H in NORM_H), "no H with fewer chunks than one wave"
    assert {2016, 2048, 2080} <= set(NORM_H) and [chunks(H) for H in (2016, 2048, 2080)] == [252, 256, 260]   # H % 32 == 0 around one trip of 256
    assert norm_threads(4064) == 256 and norm_threads(4096) == 1024 and {4064, 4096, 4128} <= set(NORM_H)
    assert any(norm_threads(H) == 1024 and chunks(H) > 1024 and chunks(H) % 1024 for H in NORM_H), "no ragged second trip of 1024"
    assert any(norm_threads(H) == 256 and chunks(H) > 256 and chunks(H) % 256 for H in NORM_H), "no ragged later trip of 256"
    assert NORM_MAXH in NORM_H and all(H > NORM_MAXH or H % 32 for H in NORM_H_REFUSED)
    for H in NORM_H:
        mine = [c for c in t if c.H == H and not c.S]
        assert {(c.res_in, c.res_out) for c in mine} == {(a, b) for a in (False, True) for b in (False, True)}, H
        assert {(c.rows, c.frag) for c in mine} == {(True, False), (False, True), (True, True)}, H
        assert any(c.gather and c.frag for c in mine) and len(GATHER) != 6 and sorted(GATHER) != list(GATHER) and len(set(GATHER)) < len(GATHER)
    assert {c.S for c in t if c.S} == set(PARTS_S) and {1, 3, 5, 7, 9} <= set(PARTS_S) and max(PARTS_S) == 16
    for S in PARTS_S:
        assert {c.slab_pad for c in t if c.S == S} == {0, 3} and len({c.H for c in t if c.S == S}) >= 2, S
    assert {c.T for c in t} >= {1, 6, 17, 33}


def _launch_norm(dev, c: NormCase, x, r, w, parts=None, inplace=False):
    """One launch into sentinel buffers.  Returns (y rows or None, y through the fragment or None, res_out or None), on the CPU, after
    checking that rows past T, the fragment's padding rows and its tail are still the sentinel and that rows and fragment agree."""
    from ssd_amd.hip import ops as Hh
    what = f"{c} inplace {inplace}"
    H, T_in = c.H, c.T
    T_out = len(GATHER) if c.gather else T_in
    yb = sentinel(T_out + PAD_ROWS, H, device=dev) if c.rows else None
    fb = sentinel(Hh.frag_numel(T_out, H) + TAIL, device=dev) if c.frag else None
    res_in = rb = None
    if inplace:
        assert c.res_in and c.res_out and not c.gather
        rb = sentinel(T_in + PAD_ROWS, H, device=dev)
        rb[:T_in] = r.to(dev)
        res_in = rb
    else:
        res_in = r.to(dev).contiguous() if c.res_in else None
        rb = sentinel(T_out + PAD_ROWS, H, device=dev) if c.res_out else None
    wd = w.to(dev)
    if c.S:
        Hh.rmsnorm_parts(parts, c.S, T_in + c.slab_pad, wd, EPS, T_in, H, res_in=res_in, res_out=rb, out_rows=yb, out_frag=fb)
    else:
        gi = torch.tensor(GATHER, dtype=torch.int32, device=dev) if c.gather else None
        Hh.rmsnorm(x.to(dev).contiguous(), wd, EPS, T_out, H, res_in=res_in, res_out=rb, out_rows=yb, out_frag=fb, gather=gi)
    torch.cuda.synchronize()
    y = yf = ro = None
    if yb is not None:
        yb = yb.cpu()
        assert is_sentinel(yb[T_out:]), f"{what}: a row >= T of out_rows was written"
        y = yb[:T_out]
    if fb is not None:
        fb, n = fb.cpu(), Hh.frag_numel(T_out, H)
        assert is_sentinel(fb[n:]), f"{what}: memory past the output fragment was written"
        full = LY.frag_to_rows_ref(fb[:n], ceil16(T_out), H)
        assert is_sentinel(full[T_out:]), f"{what}: a padding row of the output fragment was written"
        yf = full[:T_out]
        assert y is None or same_bits(y, yf), f"{what}: out_frag differs from out_rows"
    if rb is not None:
        rb = rb.cpu()
        assert is_sentinel(rb[T_out:]), f"{what}: a row >= T of res_out was written"
        ro = rb[:T_out]
    return y, yf, ro


def _parts_for(dev, c: NormCase, seed: int):
    """fp32 slabs [17][slab_rows][H]: NaN in the rows >= T of every slab and in every slab >= S."""
    g = torch.Generator().manual_seed(seed)
    live = torch.stack([scale_rows(torch.randn(c.T, c.H, generator=g), spike=(z == 0)) for z in range(c.S)])
    buf = torch.full((17, c.T + c.slab_pad, c.H), float("nan"))
    buf[:c.S, :c.T] = live
    return live, buf.to(dev)


@gpu
def test_rmsnorm_every_form_at_every_h(dev):
    worst, share, n = 0.0, 0.0, 0
    for c in (c for c in norm_table() if not c.S):
        x, r, w = norm_inputs(c.T, c.H, seed=c.H + c.T)
        y, yf, ro = _launch_norm(dev, c, x, r, w)
        idx = torch.tensor(GATHER if c.gather else range(c.T))
        want, res_want = norm_ref64(x[idx], w, EPS, r[idx] if c.res_in else None)
        out = y if y is not None else yf
        a, b = assert_1ulp(out, want, f"rmsnorm {c}")
        worst, share, n = max(worst, a), max(share, b), n + 1
        zero = [i for i, s in enumerate(idx.tolist()) if ROW_KINDS[s % len(ROW_KINDS)] == "zero"]
        assert bool((out[zero].float() == 0).all()), f"rmsnorm {c}: the row of zeros did not come out as zeros"
        if c.res_out:
            assert same_bits(ro, res_want), f"rmsnorm {c}: res_out is not bf16(fp32(x) + fp32(res))"
    assert n == len([c for c in norm_table() if not c.S])
    report("test_rmsnorm_every_form_at_every_h", "1 ulp of bf16(f64)", worst, share)


@gpu
def test_rmsnorm_parts_every_slab_count(dev):
    """Bit-equal to ssd_rmsnorm of bf16(the fp32 sum in slab order), and within the bar of float64."""
    worst, share, n = 0.0, 0.0, 0
    for c in (c for c in norm_table() if c.S):
        _, r, w = norm_inputs(c.T, c.H, seed=c.H + c.T + c.S)
        live, buf = _parts_for(dev, c, seed=c.H + c.S)
        xs = slab_sum(live, c.S)
        y, yf, ro = _launch_norm(dev, c, None, r, w, parts=buf)
        y2, yf2, ro2 = _launch_norm(dev, c._replace(S=0, slab_pad=0), xs, r, w)
        for got, twin, name in ((y, y2, "out_rows"), (yf, yf2, "out_frag"), (ro, ro2, "res_out")):
            assert (got is None) == (twin is None) and (got is None or same_bits(got, twin)), f"parts {c}: {name} differs from ssd_rmsnorm of the rounded sum"
        want, res_want = norm_ref64(xs, w, EPS, r if c.res_in else None)
        a, b = assert_1ulp(yf, want, f"parts {c}")
        worst, share, n = max(worst, a), max(share, b), n + 1
        check_zero_rows(yf, f"parts {c}")
        assert same_bits(ro, res_want), f"parts {c}: res_out"
    assert n == len([c for c in norm_table() if c.S])
    report("test_rmsnorm_parts_every_slab_count", "1 ulp of bf16(f64)", worst, share)


@gpu
def test_rmsnorm_in_place_residual_equals_out_of_place(dev):
    """The engine passes one buffer as res_in and res_out.  Each thread reads its chunk of res_in before it writes the same chunk of
    res_out, and no other thread touches it: the call must equal the out-of-place one bit for bit, at every H, for both entry points."""
    n = 0
    for H in NORM_H:
        for S in (0, PARTS_S[n % len(PARTS_S)], 16):
            c = NormCase(H, 6, True, True, True, True, False, S, 3 if S else 0)
            x, r, w = norm_inputs(c.T, H, seed=H + S)
            buf = None
            if S:
                _, buf = _parts_for(dev, c, seed=H + S)
            a = _launch_norm(dev, c, x, r, w, parts=buf)
            b = _launch_norm(dev, c, x, r, w, parts=buf, inplace=True)
            for got, twin, name in zip(b, a, ("out_rows", "out_frag", "res_out")):
                assert same_bits(got, twin), f"{c}: {name} of the in-place call differs"
            n += 1
    report("test_rmsnorm_in_place_residual_equals_out_of_place", "bit-exact", 0.0)
    print(f"in-place residual: {n} cases, each run twice")


# =====================================================================================================================
# ssd_rmsnorm_pair
# =====================================================================================================================
PAIR_H = tuple(H for H in NORM_H if H <= 8192)


def pair_table() -> list[tuple[int, int]]:
    t = [(H, PAIR_T[i % len(PAIR_T)]) for i, H in enumerate(PAIR_H)] + [(H, T) for H in (2080, 4096) for T in PAIR_T]
    return sorted(set(t))


def test_pair_case_table():
    t = pair_table()
    assert {H for H, _ in t} == set(PAIR_H) and max(PAIR_H) == 8192 and len(PAIR_H) == 11
    for T in PAIR_T:
        assert len([1 for _, t_ in t if t_ == T]) >= 2


@gpu
def test_rmsnorm_pair_halves_of_different_magnitude(dev):
    """Half 0 ~ 2^-3 N(0, 1), half 1 ~ 2^5 N(0, 1), each with its own weight: a swap of the halves, of the weights, or one rs shared by
    both misses the bar by far.  Checked per half through the [T][2H] fragment."""
    from ssd_amd.hip import ops as Hh
    worst, share = 0.0, 0.0
    for H, T in pair_table():
        g = torch.Generator().manual_seed(H + T)
        x0 = (scale_rows(torch.randn(T, H, generator=g)) * 2.0 ** -3).to(BF)
        x1 = (scale_rows(torch.randn(T, H, generator=g)[list(range(T - 1, -1, -1))]) * 2.0 ** 5).to(BF)
        w0, w1 = norm_weight(H, g), (0.5 * norm_weight(H, g).float()).to(BF)
        n = Hh.frag_numel(T, 2 * H)
        fb = sentinel(n + TAIL, device=dev)
        Hh.rmsnorm_pair(x0.to(dev), w0.to(dev), x1.to(dev), w1.to(dev), EPS, T, H, fb)
        torch.cuda.synchronize()
        fb = fb.cpu()
        assert is_sentinel(fb[n:]), f"pair {(H, T)}: memory past the fragment was written"
        full = LY.frag_to_rows_ref(fb[:n], ceil16(T), 2 * H)
        assert is_sentinel(full[T:]), f"pair {(H, T)}: a padding row of the fragment was written"
        want = torch.cat((norm_ref64(x0, w0, EPS)[0], norm_ref64(x1, w1, EPS)[0]), dim=1)
        a, b = assert_1ulp(full[:T], want, f"pair {(H, T)}")
        worst, share = max(worst, a), max(share, b)
    report("test_rmsnorm_pair_halves_of_different_magnitude", "1 ulp of bf16(f64)", worst, share)


# =====================================================================================================================
# ssd_head_rmsnorm
# =====================================================================================================================
# (T, heads, hd): T * heads * hd / 16 items in workgroups of 256 -- the nearest reachable counts below, at and above 256 per hd (one
# head is hd / 16 items), one head per token, 40 heads per token
HEAD_CASES = ((1, 63, 64), (1, 64, 64), (1, 65, 64), (1, 31, 128), (1, 32, 128), (1, 33, 128), (1, 15, 256), (1, 16, 256), (1, 17, 256),
              (33, 1, 64), (17, 1, 128), (5, 1, 256), (3, 40, 64), (3, 40, 128), (2, 40, 256))
HEAD_REFUSED = (32, 96)


def test_head_case_table_straddles_one_workgroup():
    for hd in (64, 128, 256):
        items = sorted(T * h * hd // 16 for T, h, d in HEAD_CASES if d == hd and T == 1)
        assert items == [256 - hd // 16, 256, 256 + hd // 16], (hd, items)
        assert any(h == 1 and T > 1 for T, h, d in HEAD_CASES if d == hd) and any(h == 40 for T, h, d in HEAD_CASES if d == hd)
        assert any((T * h * hd // 16) % 256 and T * h * hd // 16 > 256 for T, h, d in HEAD_CASES if d == hd)


@gpu
def test_head_rmsnorm_around_one_workgroup(dev):
    """Against float64 at 1 ulp, and bit-equal to the q output of ssd_rope_store_kv with a q norm at position 0 (cos = 1, sin = 0: the
    rotation is the identity)."""
    from ssd_amd.hip import ops as Hh
    worst, share = 0.0, 0.0
    for T, heads, hd in HEAD_CASES:
        what = f"head_rmsnorm T {T} heads {heads} hd {hd}"
        g = torch.Generator().manual_seed(T + heads + hd)
        q = scale_rows(torch.randn(T * heads, hd, generator=g), spike=False).to(BF)
        q[-1] *= 2.0 ** 6                                             # the last head: a neighbour's sum of squares would show
        w = norm_weight(hd, g)
        ob = sentinel(T * heads + PAD_ROWS, hd, device=dev)
        Hh.head_rmsnorm(q.to(dev), w.to(dev), EPS, ob, T, heads, hd)
        torch.cuda.synchronize()
        ob = ob.cpu()
        assert is_sentinel(ob[T * heads:]), f"{what}: memory past the last head was written"
        out = ob[:T * heads]
        a, b = assert_1ulp(out, norm_ref64(q, w, EPS)[0], what)
        worst, share = max(worst, a), max(share, b)
        check_zero_rows(out, what)
        nkv = 1
        qkv = torch.cat((q.view(T, heads * hd), torch.randn(T, 2 * nkv * hd, generator=g).to(BF)), dim=1).contiguous()
        q_out = sentinel(T, heads * hd, device=dev)
        kc, vc = sentinel(2, nkv, 16, hd, device=dev), sentinel(2, nkv, 16, hd, device=dev)
        Hh.rope_store_kv(qkv.to(dev), torch.zeros(T, dtype=torch.int64, device=dev), O.make_cos_sin_cache(hd, 4, 5e5).to(dev),
                         torch.full((T,), -1, dtype=torch.int32, device=dev), q_out, kc, vc, T, heads, nkv, hd, 16,
                         q_norm_w=w.to(dev), k_norm_w=w.to(dev), eps=EPS)
        torch.cuda.synchronize()
        assert same_bits(q_out.view(T * heads, hd), out), f"{what}: differs from the norm fused into ssd_rope_store_kv"
        assert is_sentinel(kc) and is_sentinel(vc)
    report("test_head_rmsnorm_around_one_workgroup", "1 ulp of bf16(f64)", worst, share)


# =====================================================================================================================
# ssd_silu_mul
# =====================================================================================================================
SILU_CASES = ((1, 32), (17, 32), (1, 96), (17, 96), (23, 96), (1, 8192), (17, 8192))         # (T, I)
SILU_BANDS = ((-101.0, -30.0), (-30.0, -10.0), (-10.0, 10.0), (10.0, 101.0))


def silu_inputs(T: int, I: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    gate = (torch.rand(T, I, generator=g) * 200 - 100)
    gate.view(-1)[:8] = torch.tensor([0.0, -0.0, -88.0, -20.0, 100.0, -100.0, 88.0, 20.0])
    gate.view(-1)[8:24] = torch.linspace(-100, 100, 16)
    lo = torch.rand(T, I, generator=g) < 0.5                          # half of the gates where SiLU bends
    gate = torch.where(lo & (torch.arange(T * I).view(T, I) >= 24), gate * 0.08, gate)
    up = torch.randn(T, I, generator=g)
    up.view(-1)[1::7] = 0.0
    up.view(-1)[3::11] = 2.0 ** 15
    return torch.cat((gate, up), dim=1).to(BF)


def test_silu_case_table():
    items = [T * I // 8 for T, I in SILU_CASES]
    assert {I for _, I in SILU_CASES} == {32, 96, 8192} and {T for T, _ in SILU_CASES} >= {1, 17}
    assert any(n > 256 and n % 256 for n in items), "no item count that crosses a workgroup unevenly"
    assert any(n < 64 for n in items) and any(n % 256 == 0 for n in items)
    x = silu_inputs(1, 32, 0).float()
    assert {0.0, -88.0, -20.0, 100.0, -100.0} <= set(x[0, :32].tolist()) and bool((x[0, :32] == 0).sum() >= 2)
    assert {0.0, 2.0 ** 15} <= set(x[0, 32:].tolist())


@gpu
def test_silu_mul_over_the_whole_gate_range(dev):
    """float64 g * sigmoid(g) * u at the SiLU bar: 1 ulp, the ulp floored at 2^-6 of the output rms -- taken per band of the gate and
    apart for the up values of 2^15, so that each floor comes from that band's own outputs (never looser than over the whole tensor)."""
    from ssd_amd.hip import ops as Hh
    worst = 0.0
    for T, I in SILU_CASES:
        what = f"silu_mul T {T} I {I}"
        x = silu_inputs(T, I, seed=T + I)
        outs = {}
        for rows, frag in ((True, False), (False, True), (True, True)):
            yb = sentinel(T + PAD_ROWS, I, device=dev) if rows else None
            n = Hh.frag_numel(T, I)
            fb = sentinel(n + TAIL, device=dev) if frag else None
            Hh.silu_mul(x.to(dev), T, I, out_rows=yb, out_frag=fb)
            torch.cuda.synchronize()
            if rows:
                yb = yb.cpu()
                assert is_sentinel(yb[T:]), f"{what}: a row >= T was written"
                outs[(rows, frag, "rows")] = yb[:T]
            if frag:
                fb = fb.cpu()
                assert is_sentinel(fb[n:]), f"{what}: memory past the fragment was written"
                full = LY.frag_to_rows_ref(fb[:n], ceil16(T), I)
                assert is_sentinel(full[T:]), f"{what}: a padding row of the fragment was written"
                outs[(rows, frag, "frag")] = full[:T]
        y = outs[(True, False, "rows")]
        assert all(same_bits(y, o) for o in outs.values()), f"{what}: out_rows, out_frag and both differ"
        assert bool(torch.isfinite(y.float()).all()), f"{what}: a non-finite output"
        g64, u64 = x[:, :I].double(), x[:, I:].double()
        want = g64 * torch.sigmoid(g64) * u64
        big = u64 == 2.0 ** 15
        for lo, hi in SILU_BANDS:
            for sel in ((g64 >= lo) & (g64 < hi) & ~big, (g64 >= lo) & (g64 < hi) & big):
                if bool(sel.any()):
                    worst = max(worst, assert_within_ulp(y[sel], want[sel], f"{what} gate [{lo}, {hi})"))
    report("test_silu_mul_over_the_whole_gate_range", "1 ulp, floor 2^-6 rms", worst)


# =====================================================================================================================
# ssd_embedding
# =====================================================================================================================
EMB_H = (8, 504, 2048, 2056)


def emb_ids():
    s, n = SHARD
    return [s, s + n - 1, s - 1, s + n, 0, -5, s + 17, s, 2 ** 40]


def test_embedding_case_table():
    s, n = SHARD
    assert EMB_H[0] // 8 == 1 and EMB_H[-1] // 8 > 256 and all(H % 8 == 0 for H in EMB_H) and any(H % 32 for H in EMB_H)
    assert {s, s + n - 1, s - 1, s + n, 0} <= set(emb_ids()) and min(emb_ids()) < 0 and s > 0


@gpu
def test_embedding_shard_borders(dev):
    from ssd_amd.hip import ops as Hh
    s, n = SHARD
    ids = torch.tensor(emb_ids(), dtype=torch.int64)
    T = ids.numel()
    for H in EMB_H:
        g = torch.Generator().manual_seed(H)
        table = torch.randint(-32768, 32768, (n, H), generator=g, dtype=torch.int32).to(torch.int16).view(BF)   # any bit pattern
        ob = sentinel(T + PAD_ROWS, H, device=dev)
        Hh.embedding(ids.to(dev), table.to(dev), ob, T, H, vocab_start=s, vocab_count=n)
        torch.cuda.synchronize()
        ob = ob.cpu()
        assert is_sentinel(ob[T:]), f"embedding H {H}: a row >= T was written"
        for i, tok in enumerate(ids.tolist()):
            if s <= tok < s + n:
                assert same_bits(ob[i], table[tok - s]), f"embedding H {H}: id {tok} is not row {tok - s} of the shard"
            else:
                assert bool((_bits(ob[i]) == 0).all()), f"embedding H {H}: id {tok} outside the shard is not all zero"
    report("test_embedding_shard_borders", "bit-exact", 0.0)


# =====================================================================================================================
# Refusals: an error code, nothing written, and a valid launch afterwards still right
# =====================================================================================================================
SHAPE, ARG = -1, -3
# (entry point, what, code, the line of csrc/norm.hip that refuses)
NORM_REFUSALS = (
    ("rmsnorm", "H 16416", SHAPE, "ssd_rmsnorm: H > NORM_MAXH"), ("rmsnorm", "H 24", SHAPE, "ssd_rmsnorm: H & 31"),
    ("rmsnorm", "T 0", SHAPE, "ssd_rmsnorm: T <= 0"), ("rmsnorm", "no x", ARG, "ssd_rmsnorm: !x_rows"),
    ("rmsnorm", "no weight", ARG, "ssd_rmsnorm: !weight"), ("rmsnorm", "no output", ARG, "ssd_rmsnorm: !out_rows && !out_frag && !res_out"),
    ("parts", "H 16416", SHAPE, "ssd_rmsnorm_parts: H > NORM_MAXH"), ("parts", "H 24", SHAPE, "ssd_rmsnorm_parts: H & 31"),
    ("parts", "S 0", SHAPE, "ssd_rmsnorm_parts: splits < 1"), ("parts", "S 17", SHAPE, "ssd_rmsnorm_parts: splits > 16"),
    ("parts", "slab_rows < T", SHAPE, "ssd_rmsnorm_parts: slab_rows < T"), ("parts", "no parts", ARG, "ssd_rmsnorm_parts: !parts"),
    ("parts", "no weight", ARG, "ssd_rmsnorm_parts: !weight"), ("parts", "no output", ARG, "ssd_rmsnorm_parts: !out_rows && !out_frag && !res_out"),
    ("pair", "H 16416", SHAPE, "ssd_rmsnorm_pair: H > NORM_MAXH"), ("pair", "H 24", SHAPE, "ssd_rmsnorm_pair: H & 31"),
    ("pair", "no x1", ARG, "ssd_rmsnorm_pair: !x1_rows"), ("pair", "no weight0", ARG, "ssd_rmsnorm_pair: !weight0"),
    ("pair", "no output", ARG, "ssd_rmsnorm_pair: !out_frag"),
    ("head", "hd 32", SHAPE, "ssd_head_rmsnorm: hd != 64 && hd != 128 && hd != 256"), ("head", "hd 96", SHAPE, "ssd_head_rmsnorm: hd"),
    ("head", "heads 0", SHAPE, "ssd_head_rmsnorm: heads <= 0"), ("head", "no weight", ARG, "ssd_head_rmsnorm: !weight"),
    ("head", "no output", ARG, "ssd_head_rmsnorm: !out_rows"),
    ("silu", "I 24", SHAPE, "ssd_silu_mul: I & 31"), ("silu", "T 0", SHAPE, "ssd_silu_mul: T <= 0"),
    ("silu", "no x", ARG, "ssd_silu_mul: !x_rows"), ("silu", "no output", ARG, "ssd_silu_mul: !out_rows && !out_frag"),
    ("embedding", "H 12", SHAPE, "ssd_embedding: H & 7"), ("embedding", "vocab_count 0", SHAPE, "ssd_embedding: vocab_count <= 0"),
    ("embedding", "vocab_count -1", SHAPE, "ssd_embedding: vocab_count <= 0"), ("embedding", "no ids", ARG, "ssd_embedding: !ids"),
    ("embedding", "no table", ARG, "ssd_embedding: !table"), ("embedding", "no output", ARG, "ssd_embedding: !out_rows"),
)


def refused_with(dev, what, code, call, *buffers):
    """`call` raises with the expected code and leaves every sentinel buffer as it was."""
    from ssd_amd.hip.lib import SsdHipError
    before = [b.clone() for b in buffers]
    with pytest.raises(SsdHipError) as e:
        call()
    assert str(e.value).endswith(f"code {code}"), f"{what}: {e.value}, expected code {code}"
    torch.cuda.synchronize()
    for b, b0 in zip(buffers, before):
        assert torch.equal(_bits(b), _bits(b0)), f"{what}: refused, yet something was written"


def test_norm_refusal_table_names_every_entry_point():
    assert {r[0] for r in NORM_REFUSALS} == {"rmsnorm", "parts", "pair", "head", "silu", "embedding"}
    assert len(set(r[:2] for r in NORM_REFUSALS)) == len(NORM_REFUSALS) and {r[2] for r in NORM_REFUSALS} == {SHAPE, ARG}
    assert all(any(f"H {H}" == r[1] for r in NORM_REFUSALS if r[0] == ep) for H in NORM_H_REFUSED for ep in ("rmsnorm", "parts", "pair"))
    assert all(any(f"hd {hd}" == r[1] for r in NORM_REFUSALS) for hd in HEAD_REFUSED)


@gpu
def test_norm_refusals_return_their_code_and_write_nothing(dev):
    from ssd_amd.hip import ops as Hh
    T, H = 4, 64
    big = 16416
    x, r, w = (t.to(dev) for t in norm_inputs(T, big, seed=1))
    parts = torch.randn(2, T, big, device=dev)
    ids = torch.tensor([1, 2, 3, 0], dtype=torch.int64, device=dev)
    yb, fb, rb = (sentinel(32 * big, device=dev) for _ in range(3))
    calls = {
        ("rmsnorm", "H 16416"): lambda: Hh.rmsnorm(x, w, EPS, T, big, res_in=r, res_out=rb, out_rows=yb, out_frag=fb),
        ("rmsnorm", "H 24"): lambda: Hh.rmsnorm(x, w, EPS, T, 24, res_in=r, res_out=rb, out_rows=yb, out_frag=fb),
        ("rmsnorm", "T 0"): lambda: Hh.rmsnorm(x, w, EPS, 0, H, out_rows=yb),
        ("rmsnorm", "no x"): lambda: Hh.rmsnorm(None, w, EPS, T, H, out_rows=yb),
        ("rmsnorm", "no weight"): lambda: Hh.rmsnorm(x, None, EPS, T, H, out_rows=yb),
        ("rmsnorm", "no output"): lambda: Hh.rmsnorm(x, w, EPS, T, H, res_in=r),
        ("parts", "H 16416"): lambda: Hh.rmsnorm_parts(parts, 2, T, w, EPS, T, big, out_rows=yb),
        ("parts", "H 24"): lambda: Hh.rmsnorm_parts(parts, 2, T, w, EPS, T, 24, out_rows=yb),
        ("parts", "S 0"): lambda: Hh.rmsnorm_parts(parts, 0, T, w, EPS, T, H, out_rows=yb, res_out=rb),
        ("parts", "S 17"): lambda: Hh.rmsnorm_parts(parts, 17, T, w, EPS, T, H, out_rows=yb, res_out=rb),
        ("parts", "slab_rows < T"): lambda: Hh.rmsnorm_parts(parts, 2, T - 1, w, EPS, T, H, out_rows=yb),
        ("parts", "no parts"): lambda: Hh.rmsnorm_parts(None, 2, T, w, EPS, T, H, out_rows=yb),
        ("parts", "no weight"): lambda: Hh.rmsnorm_parts(parts, 2, T, None, EPS, T, H, out_frag=fb),
        ("parts", "no output"): lambda: Hh.rmsnorm_parts(parts, 2, T, w, EPS, T, H, res_in=r),
        ("pair", "H 16416"): lambda: Hh.rmsnorm_pair(x, w, r, w, EPS, T, big, fb),
        ("pair", "H 24"): lambda: Hh.rmsnorm_pair(x, w, r, w, EPS, T, 24, fb),
        ("pair", "no x1"): lambda: Hh.rmsnorm_pair(x, w, None, w, EPS, T, H, fb),
        ("pair", "no weight0"): lambda: Hh.rmsnorm_pair(x, None, r, w, EPS, T, H, fb),
        ("pair", "no output"): lambda: Hh.rmsnorm_pair(x, w, r, w, EPS, T, H, None),
        ("head", "hd 32"): lambda: Hh.head_rmsnorm(x, w, EPS, yb, T, 2, 32),
        ("head", "hd 96"): lambda: Hh.head_rmsnorm(x, w, EPS, yb, T, 2, 96),
        ("head", "heads 0"): lambda: Hh.head_rmsnorm(x, w, EPS, yb, T, 0, 64),
        ("head", "no weight"): lambda: Hh.head_rmsnorm(x, None, EPS, yb, T, 2, 64),
        ("head", "no output"): lambda: Hh.head_rmsnorm(x, w, EPS, None, T, 2, 64),
        ("silu", "I 24"): lambda: Hh.silu_mul(x, T, 24, out_rows=yb, out_frag=fb),
        ("silu", "T 0"): lambda: Hh.silu_mul(x, 0, 32, out_rows=yb),
        ("silu", "no x"): lambda: Hh.silu_mul(None, T, 32, out_rows=yb),
        ("silu", "no output"): lambda: Hh.silu_mul(x, T, 32),
        ("embedding", "H 12"): lambda: Hh.embedding(ids, x, yb, T, 12, 0, 4),
        ("embedding", "vocab_count 0"): lambda: Hh.embedding(ids, x, yb, T, H, 0, 0),
        ("embedding", "vocab_count -1"): lambda: Hh.embedding(ids, x, yb, T, H, 0, -1),
        ("embedding", "no ids"): lambda: Hh.embedding(None, x, yb, T, H, 0, 4),
        ("embedding", "no table"): lambda: Hh.embedding(ids, None, yb, T, H, 0, 4),
        ("embedding", "no output"): lambda: Hh.embedding(ids, x, None, T, H, 0, 4),
    }
    assert set(calls) == {r_[:2] for r_ in NORM_REFUSALS}
    for ep, what, code, line in NORM_REFUSALS:
        refused_with(dev, f"{ep} {what} ({line})", code, calls[(ep, what)], yb, fb, rb)
    # a valid launch of each entry point afterwards is still right
    c = NormCase(64, 6, True, True, True, True, False, 0, 0)
    xs, rs, ws = norm_inputs(6, 64, seed=2)
    y, _, ro = _launch_norm(dev, c, xs, rs, ws)
    want, res_want = norm_ref64(xs, ws, EPS, rs)
    assert_1ulp(y, want, "rmsnorm after the refusals")
    assert same_bits(ro, res_want)
    print(f"norm refusals: {len(NORM_REFUSALS)} refused, nothing written")
