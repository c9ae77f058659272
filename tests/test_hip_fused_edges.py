"""The fused decode-layer GEMMs of csrc/gemm_fused.hip (gemm_fused_kernel<NT, EPI, XNORM, MAXC>, gemm_qkv_rope_m32_kernel<NT>) at the
edges tests/test_hip_fused.py does not visit, checked stage by stage so that each stage meets a sharp bar instead of the loose end-to-end one:

  1  residual    res_out is bit-equal to the CPU's fp32 add of the bf16 inputs (of bf16(fp32 slab sum in order) with h_parts); rows >= M of
                 an oversized res_out stay the sentinel.
  2  prologue    FEPI_ROWS with the bf16 identity as the weight: every output is one product by 1.0 plus zeros, so y IS the LDS image x^,
                 value for value (a -0 may come back as +0: compared as numbers).  Held to the float64 norm reference of
                 tests/test_hip_norm_edges.py at 1 ulp on every element, and bit-identical across every (nt, waves): the prologue's
                 arithmetic does not depend on the decomposition, and the cached and the uncached path must agree.  For K > 2048 the
                 identity is applied in blocks of 128 columns, so no weight is larger than [128 x K].
  3  GEMM        real weights ~ 0.05 N(0, 1), with and without bias, against the float64 product of W with the x^ stage 2 returned for
                 the same inputs (the given x for the x_frag form): 1 bf16 ulp with the ulp floored at 2^-6 of the output rms
                 (assert_within_ulp, the project's ROWS bar); columns [N, ldy) and rows >= M stay the sentinel.
  4  epilogues   FEPI_ROWS, then FEPI_QKV_ROPE / FEPI_SILU_FRAG with identical weights, inputs, nt and waves: the accumulation order is the
                 same and the epilogue works on round_bf(s + bias), which is what ROWS stored.  q_out and the WHOLE K and V caches equal
                 O.rope + O.store_kv of the un-permuted rows BY BITS (sentinel-prefilled: a store to a row no slot addresses shows); the
                 SiLU fragment equals ssd_silu_mul of the de-interleaved rows by bits, and float64 silu(g) * u of them at 1 ulp.

Two token tiles (17 <= M <= 32) have no ROWS twin: V against the float64 product at the ROWS bar, q and K at the first-order bar
1 ulp of the result + ulp(x) |cos| + ulp(partner) |sin| (a 1-ulp flip of a pre-RoPE value moves the rotated one by that much).  Rows
below 17 are bit-identical whatever M is, and rows 0..15 equal by bits the M = 16 launch of gemm_fused_kernel that deals K to the waves in
the same order: nt = 4 there (U = 2 k-tiles per run, as the two-tile kernel), at the same wave count.  With nt <= 2 that kernel has
U = 4, its waves' partial sums cover other k-tiles, a legitimately different fp32 order, so those pairs are not compared.

Every output is prefilled with the bf16 NaN 0x7FC0; slabs past S are NaN; the padding rows of x_frag are poisoned in a sweep of their own;
every launch runs twice into fresh buffers and must repeat bit for bit.  The case tables are plain Python: the unmarked tests check
what they cover (every axis value in at least two cases, every template instantiation), the GPU tests run them."""
from __future__ import annotations

from typing import NamedTuple

import pytest
import torch

from oracle import layout as LY
from oracle import ops as O
from ssd_amd.hip.ops import FEPI_QKV_ROPE, FEPI_ROWS, FEPI_SILU_FRAG
from tests.test_hip_bf16_edges import TAIL, ceil16
from tests.test_hip_fused import qkv_perm
from tests.test_hip_mxfp4 import assert_within_ulp, bf16_ulp, dev  # noqa: F401  (dev is the fixture)
from tests.test_hip_norm_edges import (ARG, EPS, PAD_ROWS, SHAPE, assert_1ulp, is_sentinel, key, norm_ref64, norm_weight, refused_with, report,
                                       same_bits, scale_rows, sentinel, slab_sum)
from tests.test_hip_quant_edges import SENTINEL
from tests.test_hip_rope_edges import EDGE_POS, cos_sin

gpu = pytest.mark.gpu
BF = torch.bfloat16
R, SI, Q = FEPI_ROWS, FEPI_SILU_FRAG, FEPI_QKV_ROPE
K_LIST = (32, 64, 96, 160, 288, 512, 1056, 2048)
WAVES = (1, 2, 3, 5, 8, 16)
NTS = (1, 2, 4)
M_EDGE = (1, 7, 15, 16)
M_ALL = tuple(range(1, 17))
K_SMALL = 96                                    # the small shape every M runs at
FUSED_S = (1, 2, 5, 16)
QKV_GEO = ((4, 2, 64), (2, 1, 128), (1, 1, 256), (6, 2, 64))       # the last: 40 row groups, a q : kv ratio of 3
BLOCK_SIZES = (16, 64, 256)
NB = 3                                          # cache blocks
ROWS_N = 192                                    # 12 row groups: nt = 1, 2, 4 all divide
SILU_I = (32, 96)
LDS_LIMIT = 160 * 1024
# the cached / uncached switch of the prologue, M * K / 8 <= waves * 64: (M, K at the switch, the next valid K, waves)
SWITCH = ((16, 256, 288, 8), (16, 512, 544, 16), (1, 4096, 4128, 8))
CEILING = (15, 4096, 1, 8)                      # M, K, nt, waves: the largest shape launch_fused_c accepts; M = 16 is refused
M32_M = (17, 24, 31, 32)
M32_K = (32, 96, 1024)
M32_WAVES = (1, 3, 8, 16)
M32_GEO = ((4, 2, 64), (6, 2, 64))


# ---------------------------------------------------------------------------------------------------------------------
# The launch rules of fused_impl / launch_fused / launch_fused_c, restated
# ---------------------------------------------------------------------------------------------------------------------
def fused_u(nt: int) -> int:
    return 4 if nt <= 2 else 2


def cached(M: int, K: int, waves: int) -> bool:
    return M * (K // 8) <= waves * 64


def lds_bytes(M: int, K: int, nt: int, waves: int, xnorm: bool) -> int:
    lds = waves * nt * 64 * 16
    if xnorm:
        chunks = M * (K // 8)
        need = chunks * 4 + waves * 64
        if lds < need:
            lds = (need + 15) & ~15
        lds += chunks * 16
    return lds


def instantiation(c) -> tuple:
    xnorm = c.src != "frag"
    return (c.nt, c.epi, xnorm, 1 if not xnorm or cached(c.M, c.K, c.waves) else 0)


ALL_INSTANTIATIONS = {(nt, epi, xn, mc) for nt in NTS for epi in (R, SI, Q) for xn, mc in ((False, 1), (True, 1), (True, 0))
                      if not (epi == SI and nt == 1)}


class FC(NamedTuple):
    sweep: str       # "probe" | "rows" | "qkv" | "silu" | "poison"
    epi: int
    M: int
    N: int
    K: int
    nt: int
    waves: int
    src: str         # "h" | "parts" | "frag"
    S: int           # slabs, src == "parts"
    res_in: bool
    res_out: bool
    bias: bool
    geo: int         # index into QKV_GEO (epi == Q)
    bs: int          # block size (epi == Q)


def fused_valid(c: FC) -> bool:
    if not 1 <= c.M <= 16 or c.N % 16 or c.K % 32 or c.nt not in NTS or (c.N // 16) % c.nt or not 1 <= c.waves <= 16:
        return False
    if c.epi == SI and (c.nt % 2 or c.N % 64 or c.bias):
        return False
    if c.epi == Q and c.N != (QKV_GEO[c.geo][0] + 2 * QKV_GEO[c.geo][1]) * QKV_GEO[c.geo][2]:
        return False
    if c.src == "frag" and (c.res_in or c.res_out):
        return False
    if c.src == "parts" and c.S not in range(1, 17):
        return False
    return lds_bytes(c.M, c.K, c.nt, c.waves, c.src != "frag") <= LDS_LIMIT


def decomps(N: int, nts=NTS, waves=WAVES):
    return [(nt, w) for nt in nts if (N // 16) % nt == 0 for w in waves]


def sources(i: int):
    """(src, S, residual) forms: rows + residual, slabs (S walks FUSED_S) + residual, rows alone, fragment-major x, slabs alone."""
    return (("h", 0, True), ("parts", FUSED_S[i % len(FUSED_S)], True), ("h", 0, False), ("frag", 0, False),
            ("parts", FUSED_S[(i + 1) % len(FUSED_S)], False))


def ceil64(n: int) -> int:
    return (n + 63) // 64 * 64


def probe_n(K: int) -> int:
    """The identity probe's N: all of K (in whole groups of 4 row tiles, so that nt = 4 divides) or one block of 128 columns at a time."""
    return ceil64(K) if K <= 2048 else 128


def shapes_mk():
    return [(M, K) for K in K_LIST for M in M_EDGE] + [(M, K_SMALL) for M in M_ALL if M not in M_EDGE]


def probe_table() -> list[FC]:
    t: list[FC] = []
    for i, (M, K) in enumerate(shapes_mk()):
        for src, S, res in sources(i):
            if src != "frag":
                t += [FC("probe", R, M, probe_n(K), K, nt, w, src, S, res, True, False, 0, 0) for nt, w in decomps(probe_n(K))]
    for M, K0, K1, w in SWITCH:
        for K in (K0, K1):
            for nt, wv in ((1, w), (2, w), (1, 5), (2, 16)):
                t += [FC("probe", R, M, probe_n(K), K, nt, wv, "h", 0, True, True, False, 0, 0), FC("probe", R, M, probe_n(K), K, nt, wv, "parts", 2, False, True, False, 0, 0)]
    M, K, nt, w = CEILING
    t += [FC("probe", R, M, probe_n(K), K, nt, w, "h", 0, True, True, False, 0, 0), FC("probe", R, M, probe_n(K), K, nt, w, "parts", 5, True, True, False, 0, 0)]
    return sorted(set(t))


def rows_table() -> list[FC]:
    t: list[FC] = []
    for i, (M, K) in enumerate(shapes_mk()):
        for src, S, res in sources(i)[:4]:
            for j, (nt, w) in enumerate(decomps(ROWS_N)):
                t.append(FC("rows", R, M, ROWS_N, K, nt, w, src, S, res, res and j % 3 != 1, (i + j) % 2 == 0, 0, 0))
    for M, K0, K1, w in SWITCH:                                         # both sides of the switch, a small N
        for K in (K0, K1):
            t += [FC("rows", R, M, 64, K, nt, w, "h", 0, True, True, nt == 2, 0, 0) for nt in NTS]
    M, K, nt, w = CEILING
    t += [FC("rows", R, M, 64, K, nt, w, "h", 0, True, True, False, 0, 0), FC("rows", R, M, 128, K, nt, w, "parts", 5, True, True, True, 0, 0)]
    return t


def qkv_table() -> list[FC]:
    t: list[FC] = []
    n = 0
    for gi, (nh, nkv, hd) in enumerate(QKV_GEO):
        N = (nh + 2 * nkv) * hd
        for mi, M in enumerate(M_EDGE + ((3, 9) if gi == 0 else ())):
            for kk in range(2):
                K = K_LIST[(gi * 4 + mi * 2 + kk) % len(K_LIST)]
                for j, (nt, w) in enumerate(decomps(N)):
                    src, S, res = sources(n)[(n + j) % 4]
                    t.append(FC("qkv", Q, M, N, K, nt, w, src, S, res, res, (n + j) % 3 != 0, gi, BLOCK_SIZES[(n + j) % 3]))
                n += 1
    N = (4 + 4) * 64
    t += [FC("qkv", Q, M, N, K_SMALL, nt, w, "h", 0, True, True, True, 0, 16) for M in M_ALL for nt, w in ((1, 3), (4, 2))]
    return t


def silu_table() -> list[FC]:
    t: list[FC] = []
    for i, (M, K) in enumerate(shapes_mk()):
        I = SILU_I[i % 2] if K != K_SMALL else 32
        for j, (nt, w) in enumerate(decomps(2 * I, nts=(2, 4))):
            src, S, res = sources(i)[(i + j) % 4]
            t.append(FC("silu", SI, M, 2 * I, K, nt, w, src, S, res, res, False, 0, 0))
    return t


def poison_table() -> list[FC]:
    t: list[FC] = []
    for M in (1, 7, 15):
        for K in (96, 288):
            for nt, w in ((1, 1), (2, 3), (4, 16)):
                t.append(FC("poison", R, M, ROWS_N, K, nt, w, "frag", 0, False, False, True, 0, 0))
                t.append(FC("poison", Q, M, 512, K, nt, w, "frag", 0, False, False, True, 0, 64))
                if nt > 1:
                    t.append(FC("poison", SI, M, 192, K, nt, w, "frag", 0, False, False, False, 0, 0))
    return t


def all_cases() -> list[FC]:
    return probe_table() + rows_table() + qkv_table() + silu_table() + poison_table()


class M32(NamedTuple):
    M: int
    K: int
    nt: int
    waves: int
    geo: tuple
    bs: int


def m32_table() -> list[M32]:
    return [M32(M, K, nt, w, geo, BLOCK_SIZES[(i + j) % 3]) for i, geo in enumerate(M32_GEO) for j, K in enumerate(M32_K) for M in M32_M
            for nt in NTS for w in M32_WAVES]


def slots_and_positions(M: int, bs: int, seed: int):
    """M distinct slots out of 0, bs - 1, bs, the cache's last, -1 and random ones, and M positions out of EDGE_POS and random ones:
    the edge values first, rotated by the seed, so that small M see all of them across the table."""
    g = torch.Generator().manual_seed(seed)
    edge = [0, bs - 1, bs, NB * bs - 1, -1]
    edge = edge[seed % 5:] + edge[:seed % 5]
    rest = [s for s in torch.randperm(NB * bs, generator=g).tolist() if s not in edge]
    slots = torch.tensor((edge + rest)[:M], dtype=torch.int32)[torch.randperm(M, generator=g)]
    ep = list(EDGE_POS[seed % 6:]) + list(EDGE_POS[:seed % 6])
    pos = torch.tensor((ep + torch.randint(0, 8192, (32,), generator=g).tolist())[:M], dtype=torch.int64)[torch.randperm(M, generator=g)]
    return slots, pos


def _seed(c) -> int:
    return c.M * 131 + c.K + 7 * c.nt + 3 * c.waves


# ---------------------------------------------------------------------------------------------------------------------
# Unmarked: what the tables cover
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_case_tables_cover_every_instantiation_and_every_axis_twice():
    t = all_cases()
    assert all(fused_valid(c) for c in t), [c for c in t if not fused_valid(c)][:3]
    assert {instantiation(c) for c in t} == ALL_INSTANTIATIONS and len(ALL_INSTANTIATIONS) == 24
    assert {instantiation(c) for c in t if c.sweep == "probe"} == {(nt, R, True, mc) for nt in NTS for mc in (0, 1)}
    twice = lambda values, got: all(sum(1 for g in got if g == v) >= 2 for v in values)            # noqa: E731
    for sweep in ("probe", "rows", "qkv", "silu"):
        mine = [c for c in t if c.sweep == sweep]
        assert twice(M_EDGE, [c.M for c in mine]) and twice(K_LIST, [c.K for c in mine]) and twice(WAVES, [c.waves for c in mine]), sweep
        assert twice(NTS if sweep != "silu" else (2, 4), [c.nt for c in mine]), sweep
        assert twice(FUSED_S, [c.S for c in mine if c.src == "parts"]), sweep
        assert set(M_ALL) <= {c.M for c in mine if c.K == K_SMALL}, f"{sweep}: not every M at the small shape"
        assert any(c.waves < c.nt for c in mine) and any(c.waves not in (1, 2, 4, 8, 16) for c in mine)
        for nt in NTS if sweep != "silu" else (2, 4):
            U = fused_u(nt)
            mine_nt = [c for c in mine if c.nt == nt]
            assert any(c.K // 32 < U for c in mine_nt), f"{sweep} nt {nt}: no K below one run of U k-tiles"
            assert any((c.K // 32) % U and c.K // 32 > U for c in mine_nt), f"{sweep} nt {nt}: no left-over k-tiles after full runs"
            assert any(0 < (c.K // 32) // U < c.waves for c in mine_nt), f"{sweep} nt {nt}: no idle wave"
        if sweep != "probe":
            assert any(c.src == "frag" for c in mine)
        assert any(c.src == "h" and c.res_in for c in mine) and any(c.src == "h" and not c.res_in for c in mine)
    rows = [c for c in t if c.sweep == "rows"]
    assert any(c.res_in and not c.res_out for c in rows), "no res_in without res_out"
    assert {c.bias for c in rows} == {False, True}
    for M, K0, K1, w in SWITCH:                                         # at the switch and one valid K above it, waves 8 and 16
        assert M * (K0 // 8) == w * 64 and K1 == K0 + 32 and cached(M, K0, w) and not cached(M, K1, w)
        for sweep in ("probe", "rows"):
            assert all(any(c.sweep == sweep and (c.M, c.K, c.waves) == (M, K, w) for c in t) for K in (K0, K1))
    assert {w for _, _, _, w in SWITCH} == {8, 16}
    M, K, nt, w = CEILING
    assert 148 * 1024 < lds_bytes(M, K, nt, w, True) <= LDS_LIMIT < lds_bytes(M + 1, K, nt, w, True)
    assert sum(1 for c in t if (c.M, c.K, c.nt, c.waves) == CEILING) >= 2 and all(c.N <= 128 for c in rows if c.K >= 4096)
    qkv = [c for c in t if c.sweep == "qkv"]
    assert twice(range(len(QKV_GEO)), [c.geo for c in qkv]) and twice(BLOCK_SIZES, [c.bs for c in qkv])
    assert any(QKV_GEO[c.geo] == (6, 2, 64) and c.nt == 4 and c.N // 16 == 40 for c in qkv)
    assert {QKV_GEO[c.geo][2] for c in qkv} == {64, 128, 256}
    kinds, poss = [], []
    for c in qkv:
        slots, pos = slots_and_positions(c.M, c.bs, _seed(c))
        assert len(set(slots.tolist())) == c.M
        kinds += [("0", "bs-1", "bs", "last", "-1")[i] for i, s in enumerate((0, c.bs - 1, c.bs, NB * c.bs - 1, -1)) if s in slots.tolist()]
        poss += [p for p in pos.tolist() if p in EDGE_POS]
    assert twice(("0", "bs-1", "bs", "last", "-1"), kinds) and twice(EDGE_POS, poss)
    assert {c.epi for c in t if c.sweep == "poison"} == {R, SI, Q} and {c.M for c in t if c.sweep == "poison"} == {1, 7, 15}
    assert all(c.K <= 2048 or c.sweep in ("probe", "rows") for c in t) and all(c.N * c.K <= 4096 * 2048 for c in t)


def test_two_tile_case_table():
    t = m32_table()
    assert {c.M for c in t} == set(M32_M) and {c.K for c in t} == set(M32_K) and {c.nt for c in t} == {1, 2, 4}
    assert {c.waves for c in t} == set(M32_WAVES) and {c.bs for c in t} == set(BLOCK_SIZES)
    assert any(c.K // 32 < 2 for c in t) and any((c.K // 32) % 2 for c in t) and any(0 < c.K // 64 < c.waves for c in t)
    assert all(((g[0] + 2 * g[1]) * g[2] // 16) % 4 == 0 for g in M32_GEO)      # the M = 16 twin runs at nt = 4


# ---------------------------------------------------------------------------------------------------------------------
# Operands
# ---------------------------------------------------------------------------------------------------------------------
class _Src:
    """One x source on both sides: h / parts / x_frag, the residual, the norm weight; xin = the bf16 rows the prologue starts from."""

    def __init__(self, dev, M, K, src, S, res, seed):
        from ssd_amd.hip import ops as Hh
        g = torch.Generator().manual_seed(seed)
        self.src, self.S, self.M, self.K = src, S, M, K
        self.nw = norm_weight(K, g)
        self.res = scale_rows(torch.randn(M, K, generator=g), spike=False).to(BF) if res else None
        self.kw = {}
        if src == "frag":
            self.x = torch.randn(M, K, generator=g).to(BF)
            self.kw["x_frag"] = LY.rows_to_frag_ref(self.x).to(dev)
            assert self.kw["x_frag"].numel() == Hh.frag_numel(M, K)
            return
        if src == "parts":
            live = torch.stack([scale_rows(torch.randn(M, K, generator=g), spike=(z == 0)) for z in range(S)])
            buf = torch.full((17, M, K), float("nan"))
            buf[:S] = live
            self.xin = slab_sum(live, S)
            self.kw.update(h_parts=buf.to(dev), splits=S)
        else:
            self.xin = scale_rows(torch.randn(M, K, generator=g)).to(BF)
            self.kw["h_rows"] = self.xin.to(dev)
        self.kw.update(norm_w=self.nw.to(dev), eps=EPS, res_in=None if self.res is None else self.res.to(dev))
        self.xhat64, self.res_want = norm_ref64(self.xin, self.nw, EPS, self.res)


def _frag_src(dev, x):
    """An x_frag source over given rows."""
    s = _Src.__new__(_Src)
    s.src, s.S, s.M, s.K, s.x, s.res = "frag", 0, x.shape[0], x.shape[1], x, None
    s.kw = {"x_frag": LY.rows_to_frag_ref(x).to(dev)}
    return s


class _Weights:
    def __init__(self, dev):
        self.dev, self.cache = dev, {}

    def _frag(self, w, mode=0, geo=None):
        from ssd_amd.hip import ops as Hh
        wf = torch.empty(w.numel(), dtype=BF, device=self.dev)
        if geo:
            Hh.rows_to_frag_qkv(w.to(self.dev), wf, *geo, w.shape[1])
        else:
            Hh.rows_to_frag(w.to(self.dev), wf, w.shape[0], w.shape[1], mode)
        return wf

    def eye(self, c0, N, K):
        """Rows [c0, c0 + N) of the K x K identity, zero rows past K."""
        if ("eye", c0, N, K) not in self.cache:
            w = torch.zeros(N, K, dtype=BF)
            n = min(N, K - c0)
            w[torch.arange(n), c0 + torch.arange(n)] = 1.0
            self.cache[("eye", c0, N, K)] = self._frag(w)
        return self.cache[("eye", c0, N, K)]

    def real(self, kind, N, K, geo=None):
        """(fragment form, W in the kernel's row order as float64, bias in that order bf16)."""
        if (kind, N, K, geo) not in self.cache:
            g = torch.Generator().manual_seed(N + K + len(kind))
            w = (torch.randn(N, K, generator=g) * 0.05).to(BF)
            w[3, :] = 0.5                                               # asymmetric structure: a permuted tile cannot pass
            bias = (torch.randn(N, generator=g) * 0.1).to(BF)
            if kind == "qkv":
                order = qkv_perm(*geo)
                wf = self._frag(w, geo=geo)
            elif kind == "silu":
                order = LY.interleave_gate_up_rows(torch.arange(N).view(N, 1)).view(-1)
                wf = self._frag(w, mode=1)
            else:
                order = torch.arange(N)
                wf = self._frag(w)
            self.cache[(kind, N, K, geo)] = (wf, w[order].double(), bias[order].contiguous(), order)
        return self.cache[(kind, N, K, geo)]


def _rows_launch(dev, wf, c, s, bias=None, N=None, xf=None):
    """FEPI_ROWS into sentinel-guarded y [M + PAD][N + 64] and res_out [M + PAD][K]; returns (y [M, N], res_out [M, K] or None), CPU."""
    from ssd_amd.hip import ops as Hh
    N = c.N if N is None else N
    ldy = N + 64
    yb = sentinel(c.M + PAD_ROWS, ldy, device=dev)
    rb = sentinel(c.M + PAD_ROWS, c.K, device=dev) if c.res_out else None
    kw = dict(s.kw, x_frag=xf) if xf is not None else s.kw
    Hh.gemm_fused(wf, c.M, N, c.K, R, nt=c.nt, waves=c.waves, bias=bias, y=yb, ldy=ldy, **kw, **({"res_out": rb} if s.src != "frag" else {}))
    torch.cuda.synchronize()
    yb = yb.cpu()
    assert is_sentinel(yb[c.M:]), f"{c}: a row >= M of y was written"
    assert is_sentinel(yb[:c.M, N:]), f"{c}: a column in [N, ldy) was written"
    ro = None
    if rb is not None:
        rb = rb.cpu()
        assert is_sentinel(rb[c.M:]), f"{c}: a row >= M of res_out was written"
        ro = rb[:c.M]
    return yb[:c.M, :N].contiguous(), ro


def _read_xhat(dev, weights, c, s):
    """Stages 1 and 2: the LDS image through identity weights (blocks of 128 columns when K > 2048), and the residual."""
    blk = 2048 if c.K <= 2048 else 128
    cols, ro = [], None
    for c0 in range(0, c.K, blk):
        n = min(blk, c.K - c0)
        y, ro = _rows_launch(dev, weights.eye(c0, ceil64(n), c.K), c, s, N=ceil64(n))     # rows past K of the identity are zero rows
        assert bool((y[:, n:].float() == 0).all()), f"{c}: a zero row of the weight gave a non-zero output"
        cols.append(y[:, :n])
        if ro is not None:
            assert same_bits(ro, s.res_want), f"{c}: res_out is not the fp32 add of the bf16 inputs, rounded once"
    return torch.cat(cols, dim=1)


def _same_numbers(a, b) -> bool:
    return bool(torch.equal(key(a), key(b)))


# =====================================================================================================================
# Stages 1 and 2
# =====================================================================================================================
def _probe_groups(pred):
    groups: dict = {}
    for c in probe_table():
        if pred(c):
            groups.setdefault((c.M, c.K, c.src, c.S, c.res_in), []).append(c)
    return groups


def _run_probe(dev, pred, name):
    weights = _Weights(dev)
    worst, share, n = 0.0, 0.0, 0
    for (M, K, src, S, res), cases in _probe_groups(pred).items():
        s = _Src(dev, M, K, src, S, res, seed=M * 131 + K + S)
        first = None
        for c in cases:
            xh = _read_xhat(dev, weights, c, s)
            a, b = assert_1ulp(xh, s.xhat64, f"x^ {c}")
            worst, share, n = max(worst, a), max(share, b), n + 1
            for i in range(M):
                if not bool(s.xhat64[i].any()):
                    assert bool((xh[i].float() == 0).all()), f"{c}: the row of zeros is not zeros in x^"
            if first is None:
                first = (c, xh)
            assert _same_numbers(xh, first[1]), f"x^ {c}: differs from {first[0]} (cached {cached(c.M, c.K, c.waves)} / {cached(c.M, c.K, first[0].waves)})"
        if K > 2048:
            weights.cache.clear()
    assert n
    report(name, "x^: 1 ulp of bf16(f64); res_out and decompositions bit-exact", worst, share)
    print(f"{name}: {n} read-outs of x^")


@gpu
def test_prologue_read_out_through_identity_weights(dev):
    """Every (M, K) of the table with every (nt, waves): K below one run of U k-tiles (the last wave's tail loop does the whole product),
    left-over k-tiles, idle waves feeding zeros into the combine, waves < nt, wave counts that are no power of two."""
    _run_probe(dev, lambda c: c.K <= 2048 and (c.M, c.K) not in {(m, k) for m, k0, k1, _ in SWITCH for k in (k0, k1)}, "test_prologue_read_out_through_identity_weights")


@gpu
def test_prologue_cached_and_uncached_paths_agree_at_the_switch(dev):
    """M * K / 8 == waves * 64 and the next valid K, for 8 and 16 waves; each shape also with a wave count on the other side."""
    _run_probe(dev, lambda c: (c.M, c.K) in {(m, k) for m, k0, k1, _ in SWITCH for k in (k0, k1)} and (c.M, c.K) != CEILING[:2],
               "test_prologue_cached_and_uncached_paths_agree_at_the_switch")


@gpu
def test_prologue_at_the_lds_ceiling(dev):
    """M = 15, K = 4096, nt = 1, 8 waves: about 150 KiB of dynamic LDS, the largest shape the launch accepts."""
    _run_probe(dev, lambda c: (c.M, c.K) == CEILING[:2], "test_prologue_at_the_lds_ceiling")


# =====================================================================================================================
# Stage 3
# =====================================================================================================================
@gpu
def test_rows_gemm_against_float64_of_the_read_out_prologue(dev):
    weights = _Weights(dev)
    worst, n = 0.0, 0
    groups: dict = {}
    for c in rows_table():
        groups.setdefault((c.M, c.K, c.src, c.S, c.res_in), []).append(c)
    for (M, K, src, S, res), cases in groups.items():
        s = _Src(dev, M, K, src, S, res, seed=M * 131 + K + S)
        if src == "frag":
            x64 = s.x.double()
        else:                                                           # the x^ of THIS launch family, read out exactly (stage 2)
            x64 = _read_xhat(dev, weights, cases[0]._replace(res_out=True), s).double()
        for c in cases:
            wf, w64, bias, _ = weights.real("rows", c.N, K)
            want = x64 @ w64.T + (bias.double() if c.bias else 0.0)
            b = bias.to(dev) if c.bias else None
            y, ro = _rows_launch(dev, wf, c, s, bias=b)
            y2, ro2 = _rows_launch(dev, wf, c, s, bias=b)
            assert same_bits(y, y2) and (ro is None or same_bits(ro, ro2)), f"{c}: the second launch differs"
            assert ro is None or same_bits(ro, s.res_want), f"{c}: res_out"
            worst, n = max(worst, assert_within_ulp(y, want, f"rows {c}")), n + 1
        if K > 2048:
            weights.cache.clear()
    # nt = 0, waves = 0: the default decomposition
    c = FC("rows", R, 7, ROWS_N, 288, 0, 0, "h", 0, True, True, True, 0, 0)
    s = _Src(dev, 7, 288, "h", 0, True, seed=5)
    wf, w64, bias, _ = weights.real("rows", ROWS_N, 288)
    x64 = _read_xhat(dev, weights, c._replace(nt=1, waves=8), s).double()
    worst = max(worst, assert_within_ulp(_rows_launch(dev, wf, c, s, bias=bias.to(dev))[0], x64 @ w64.T + bias.double(), f"rows {c}"))
    assert n == len(rows_table())
    report("test_rows_gemm_against_float64_of_the_read_out_prologue", "ROWS: 1 ulp, floor 2^-6 rms", worst)
    print(f"rows: {n} cases, each run twice")


# =====================================================================================================================
# Stage 4
# =====================================================================================================================
_CS_DEV: dict = {}


def cs_dev(dev, hd):
    if hd not in _CS_DEV:
        _CS_DEV[hd] = cos_sin(hd).to(dev)
    return _CS_DEV[hd]


def _qkv_buffers(dev, M, nh, nkv, hd, bs):
    return sentinel(M + PAD_ROWS, nh * hd, device=dev), sentinel(NB, nkv, bs, hd, device=dev), sentinel(NB, nkv, bs, hd, device=dev)


def _qkv_launch(dev, wf, c, s, bias, slots, pos, geo, bs, M=None, xf=None):
    from ssd_amd.hip import ops as Hh
    nh, nkv, hd = geo
    M = c.M if M is None else M
    q_out, kc, vc = _qkv_buffers(dev, M, nh, nkv, hd, bs)
    rb = sentinel(M + PAD_ROWS, c.K, device=dev) if s.src != "frag" and c.res_out else None
    kw = dict(s.kw, x_frag=xf) if xf is not None else s.kw
    Hh.gemm_fused(wf, M, (nh + 2 * nkv) * hd, c.K, Q, nt=c.nt, waves=c.waves, bias=bias, positions=pos.to(dev), cos_sin=cs_dev(dev, hd),
                  slots=slots.to(dev), q_out=q_out, k_cache=kc, v_cache=vc, nh=nh, nkv=nkv, hd=hd, block_size=bs, **kw,
                  **({"res_out": rb} if s.src != "frag" else {}))
    torch.cuda.synchronize()
    q_out = q_out.cpu()
    assert is_sentinel(q_out[M:]), f"{c}: a row >= M of q_out was written"
    if rb is not None:
        rb = rb.cpu()
        assert is_sentinel(rb[M:]) and same_bits(rb[:M], s.res_want), f"{c}: res_out"
    return q_out[:M].contiguous(), LY.kv_hnd_to_nhd(kc.cpu()), LY.kv_hnd_to_nhd(vc.cpu())


def _rope_store_oracle(rows, order, slots, pos, geo, bs):
    """O.rope + O.store_kv of the ROWS output (kernel row order -> natural order) into sentinel-prefilled reference caches."""
    nh, nkv, hd = geo
    M = rows.shape[0]
    nat = torch.empty_like(rows)
    nat[:, order] = rows
    q, k, v = [t.contiguous() for t in nat.split([nh * hd, nkv * hd, nkv * hd], dim=1)]
    qr, kr = O.rope(pos, q, k, cos_sin(hd), hd)
    kref, vref = sentinel(NB, bs, nkv, hd), sentinel(NB, bs, nkv, hd)
    O.store_kv(kr.view(M, nkv, hd), v.view(M, nkv, hd), kref, vref, slots)
    return qr, kref, vref


@gpu
def test_qkv_rope_epilogue_equals_rope_and_store_of_the_rows_epilogue_by_bits(dev):
    weights = _Weights(dev)
    srcs: dict = {}
    n = 0
    for c in qkv_table():
        geo = QKV_GEO[c.geo]
        sk = (c.M, c.K, c.src, c.S, c.res_in)
        if sk not in srcs:
            srcs[sk] = _Src(dev, c.M, c.K, c.src, c.S, c.res_in, seed=c.M * 131 + c.K + c.S)
        s = srcs[sk]
        wf, _, bias, order = weights.real("qkv", c.N, c.K, geo)
        b = bias.to(dev) if c.bias else None
        slots, pos = slots_and_positions(c.M, c.bs, _seed(c))
        rows, _ = _rows_launch(dev, wf, c, s, bias=b)
        want = _rope_store_oracle(rows, order, slots, pos, geo, c.bs)
        got = _qkv_launch(dev, wf, c, s, b, slots, pos, geo, c.bs)
        again = _qkv_launch(dev, wf, c, s, b, slots, pos, geo, c.bs)
        for name, g, w, a in zip(("q_out", "K cache", "V cache"), got, want, again):
            assert same_bits(g, w), f"{c}: {name} differs from rope + store of the rows epilogue ({int((g.view(torch.int16) != w.view(torch.int16)).sum())} elements)"
            assert same_bits(g, a), f"{c}: {name} of the second launch differs"
        if -1 in slots.tolist():
            assert bool(torch.isfinite(got[0].float()).all()), f"{c}: the q row of the slot -1 token was not written"
        n += 1
    report("test_qkv_rope_epilogue_equals_rope_and_store_of_the_rows_epilogue_by_bits", "bit-exact", 0.0)
    print(f"qkv: {n} cases, each run twice")


def _silu_launch(dev, wf, c, s, xf=None):
    from ssd_amd.hip import ops as Hh
    I = c.N // 2
    n = Hh.frag_numel(c.M, I)
    fb = sentinel(n + TAIL, device=dev)
    rb = sentinel(c.M + PAD_ROWS, c.K, device=dev) if s.src != "frag" and c.res_out else None
    kw = dict(s.kw, x_frag=xf) if xf is not None else s.kw
    Hh.gemm_fused(wf, c.M, c.N, c.K, SI, nt=c.nt, waves=c.waves, y=fb, **kw, **({"res_out": rb} if s.src != "frag" else {}))
    torch.cuda.synchronize()
    fb = fb.cpu()
    assert is_sentinel(fb[n:]), f"{c}: memory past the output fragment was written"
    full = LY.frag_to_rows_ref(fb[:n], ceil16(c.M), I)
    assert is_sentinel(full[c.M:]), f"{c}: a padding row of the output fragment was written"
    if rb is not None:
        rb = rb.cpu()
        assert is_sentinel(rb[c.M:]) and same_bits(rb[:c.M], s.res_want), f"{c}: res_out"
    return full[:c.M].contiguous()


def _deinterleave(rows, I):
    v = rows.view(rows.shape[0], I // 16, 2, 16)
    return torch.cat((v[:, :, 0].reshape(-1, I), v[:, :, 1].reshape(-1, I)), dim=1).contiguous()


@gpu
def test_silu_epilogue_equals_silu_mul_of_the_rows_epilogue_by_bits(dev):
    from ssd_amd.hip import ops as Hh
    weights = _Weights(dev)
    worst, share, n = 0.0, 0.0, 0
    for c in silu_table():
        I = c.N // 2
        s = _Src(dev, c.M, c.K, c.src, c.S, c.res_in, seed=c.M * 131 + c.K + c.S)
        wf = weights.real("silu", c.N, c.K)[0]
        gu = _deinterleave(_rows_launch(dev, wf, c, s)[0], I)
        twin = torch.empty(c.M, I, dtype=BF, device=dev)
        Hh.silu_mul(gu.to(dev), c.M, I, out_rows=twin)
        got, again = _silu_launch(dev, wf, c, s), _silu_launch(dev, wf, c, s)
        assert same_bits(got, twin), f"{c}: differs from ssd_silu_mul of the rows epilogue"
        assert same_bits(got, again), f"{c}: the second launch differs"
        g64, u64 = gu[:, :I].double(), gu[:, I:].double()
        a, b = assert_1ulp(got, g64 * torch.sigmoid(g64) * u64, f"silu {c}")
        worst, share, n = max(worst, a), max(share, b), n + 1
    report("test_silu_epilogue_equals_silu_mul_of_the_rows_epilogue_by_bits", "bit-exact; 1 ulp of bf16(f64 silu(g) u)", worst, share)
    print(f"silu: {n} cases, each run twice")


# =====================================================================================================================
# Poisoned padding rows of x_frag
# =====================================================================================================================
def _poisoned_frag(dev, x, rows):
    M, K = x.shape
    poison = torch.tensor([0x7FC0, 0x7F80, -128, SENTINEL, -1, 0x7F81], dtype=torch.int16)
    pad = poison[torch.arange((rows - M) * K) % poison.numel()].view(rows - M, K)
    xf = LY.rows_to_frag_ref(torch.cat((x.view(torch.int16), pad)).view(BF))
    assert not bool(torch.isfinite(xf.float()).all())
    return xf.to(dev)



@gpu
def test_poisoned_padding_rows_of_x_frag_never_reach_an_output(dev):
    """NaN and Inf patterns in rows M..15 of x_frag (M..31 in the two-tile form): both kernels guard the load with mcol < M, and an MFMA
    output column depends only on the same column of its B operand, so no real output may change by one bit."""
    weights = _Weights(dev)
    n = 0
    for c in poison_table():
        s = _Src(dev, c.M, c.K, "frag", 0, False, seed=c.M + c.K)
        xp = _poisoned_frag(dev, s.x, 16)
        if c.epi == R:
            wf, _, bias, _ = weights.real("rows", c.N, c.K)
            clean, dirty = _rows_launch(dev, wf, c, s, bias=bias.to(dev))[0], _rows_launch(dev, wf, c, s, bias=bias.to(dev), xf=xp)[0]
            assert same_bits(clean, dirty), f"{c}: padding rows of x changed y"
        elif c.epi == SI:
            wf = weights.real("silu", c.N, c.K)[0]
            assert same_bits(_silu_launch(dev, wf, c, s), _silu_launch(dev, wf, c, s, xf=xp)), f"{c}: padding rows of x changed the fragment"
        else:
            geo = QKV_GEO[c.geo]
            wf, _, bias, _ = weights.real("qkv", c.N, c.K, geo)
            slots, pos = slots_and_positions(c.M, c.bs, _seed(c))
            clean = _qkv_launch(dev, wf, c, s, bias.to(dev), slots, pos, geo, c.bs)
            dirty = _qkv_launch(dev, wf, c, s, bias.to(dev), slots, pos, geo, c.bs, xf=xp)
            assert all(same_bits(a, b) for a, b in zip(clean, dirty)), f"{c}: padding rows of x changed q or a cache"
        n += 1
    for M in (17, 24, 31):                                              # the two-tile form
        for K in (96, 1024):
            for nt, w in ((1, 3), (2, 8)):
                geo, bs = (4, 2, 64), 16
                c = FC("poison", Q, M, 512, K, nt, w, "frag", 0, False, False, True, 0, bs)
                s = _Src(dev, M, K, "frag", 0, False, seed=M + K)
                wf, _, bias, _ = weights.real("qkv", 512, K, geo)
                slots, pos = slots_and_positions(M, bs, _seed(c))
                clean = _qkv_launch(dev, wf, c, s, bias.to(dev), slots, pos, geo, bs)
                dirty = _qkv_launch(dev, wf, c, s, bias.to(dev), slots, pos, geo, bs, xf=_poisoned_frag(dev, s.x, 32))
                assert all(same_bits(a, b) for a, b in zip(clean, dirty)), f"{c}: padding rows of x changed q or a cache"
                n += 1
    report("test_poisoned_padding_rows_of_x_frag_never_reach_an_output", "bit-exact", 0.0)
    print(f"poison: {n} cases, each run clean and poisoned")


# =====================================================================================================================
# Two token tiles
# =====================================================================================================================
def _first_order_ratio(got, x64, cos, sin, hd, floor, what):
    """got bf16 [M, heads * hd] against the float64 rotation of bf16(x64), bar 1 ulp of the result + ulp(x) |cos| + ulp(partner) |sin|,
    the ulp of a pre-RoPE value floored as in the ROWS bar that value meets."""
    M = x64.shape[0]
    xb = x64.to(BF).double().view(M, -1, hd)
    x1, x2 = xb.chunk(2, dim=-1)
    want = torch.cat((x1 * cos - x2 * sin, x2 * cos + x1 * sin), dim=-1).view(M, -1)
    u = bf16_ulp(torch.maximum(xb.abs(), floor))
    u1, u2 = u.chunk(2, dim=-1)
    slack = torch.cat((u1 * cos.abs() + u2 * sin.abs(), u2 * cos.abs() + u1 * sin.abs()), dim=-1).view(M, -1)
    wb = want.to(BF).double()
    assert bool(torch.isfinite(got.float()).all()), f"{what}: a non-finite output (or one left unwritten)"
    tol = bf16_ulp(torch.maximum(got.double().abs(), wb.abs())) + slack
    ratio = ((got.double() - wb).abs() / tol).max().item()
    assert ratio <= 1.0, f"{what}: {ratio:.2f} x the first-order bar"
    return ratio


@gpu
def test_two_token_tiles_against_float64_and_across_m(dev):
    weights = _Weights(dev)
    worst_v, worst_qk, n = 0.0, 0.0, 0
    by: dict = {}
    for geo in M32_GEO:
        nh, nkv, hd = geo
        N = (nh + 2 * nkv) * hd
        for K in M32_K:
            wf, w64, bias, order = weights.real("qkv", N, K, geo)
            s32 = _Src(dev, 32, K, "frag", 0, False, seed=K + nh)
            nat = torch.empty(32, N, dtype=torch.float64)
            nat[:, order] = s32.x.double() @ w64.T + bias.double()                       # pre-RoPE qkv in float64, natural row order
            floor = nat.pow(2).mean().sqrt() * 2 ** -6
            for c in (c for c in m32_table() if c.geo == geo and c.K == K and c.M == M32_M[0]):
                bs = c.bs
                slots32, pos32 = slots_and_positions(32, bs, K + c.waves)             # (not nt: nt = 4 is compared with nt = 2 below)
                cos, sin = (t.double().unsqueeze(1) for t in cos_sin(hd)[pos32].chunk(2, dim=-1))
                outs = {}
                for M in M32_M + (16,):
                    fc = FC("m32", Q, M, N, K, c.nt if M > 16 else 4, c.waves, "frag", 0, False, False, True, 0, bs)
                    s = _frag_src(dev, s32.x[:M].contiguous())
                    slots, pos = slots32[:M], pos32[:M]
                    got = _qkv_launch(dev, wf, fc, s, bias.to(dev), slots, pos, geo, bs)
                    again = _qkv_launch(dev, wf, fc, s, bias.to(dev), slots, pos, geo, bs)
                    assert all(same_bits(a, b) for a, b in zip(got, again)), f"{fc}: the second launch differs"
                    outs[M] = got
                    if M == 16:
                        continue
                    q, kc, vc = got
                    ok = slots >= 0
                    idx = slots[ok].long()
                    written = torch.zeros(NB * bs, dtype=torch.bool)
                    written[idx] = True
                    kg, vg = kc.view(NB * bs, nkv * hd), vc.view(NB * bs, nkv * hd)
                    assert is_sentinel(kg[~written]) and is_sentinel(vg[~written]), f"{fc}: a cache row no slot addresses was written"
                    qn, kn, vn = nat[:M].split([nh * hd, nkv * hd, nkv * hd], dim=1)
                    worst_qk = max(worst_qk, _first_order_ratio(q, qn, cos[:M], sin[:M], hd, floor, f"{fc} q"))
                    worst_qk = max(worst_qk, _first_order_ratio(kg[idx], kn[ok], cos[:M][ok], sin[:M][ok], hd, floor, f"{fc} K"))
                    worst_v = max(worst_v, assert_within_ulp(vg[idx], vn[ok], f"{fc} V"))
                    n += 1
                # a token's result does not depend on how many rows share the launch
                for M in M32_M[1:]:
                    assert same_bits(outs[M][0][:17], outs[17][0]), f"m32 {c} M {M}: q rows < 17 differ from the M = 17 launch"
                m16 = outs[16]
                for M in M32_M:
                    assert same_bits(outs[M][0][:16], m16[0]), f"m32 {c} M {M}: q rows < 16 differ from gemm_fused_kernel<4> at M = 16"
                    sl = slots32[:16]
                    idx16 = sl[sl >= 0].long()
                    for name, a, b in (("K", outs[M][1], m16[1]), ("V", outs[M][2], m16[2])):
                        assert same_bits(a.view(NB * bs, -1)[idx16], b.view(NB * bs, -1)[idx16]), f"m32 {c} M {M}: {name} rows of tokens < 16 differ from M = 16"
                by[(geo, K, c.waves, c.nt)] = outs[32]
    for (geo, K, w, nt), o in by.items():                               # nt = 4 is mapped to 2
        if nt == 4:
            assert all(same_bits(a, b) for a, b in zip(o, by[(geo, K, w, 2)])), f"m32 {(geo, K, w)}: nt = 4 differs from nt = 2"
    report("test_two_token_tiles_against_float64_and_across_m", "V ROWS bar", worst_v)
    report("test_two_token_tiles_against_float64_and_across_m", "q, K first-order bar", worst_qk)
    print(f"m32: {n} cases, each run twice")


# =====================================================================================================================
# Refusals
# =====================================================================================================================
# (what, code, changed arguments, the line of csrc/gemm_fused.hip fused_impl / launch_fused_* that refuses)
FUSED_REFUSALS = (
    ("M 0", SHAPE, dict(M=0), "M <= 0"), ("M 17 with h_rows", SHAPE, dict(M=17), "M > 16 && !m32"),
    ("M 17 x_frag ROWS", SHAPE, dict(M=17, src="frag"), "M > 16 && !m32 (m32 needs FEPI_QKV_ROPE)"),
    ("M 33 two tiles", SHAPE, dict(M=33, src="frag", epi=Q), "M > 16 && !m32 (M <= 32)"),
    ("M 17 h_rows QKV", SHAPE, dict(M=17, epi=Q), "M > 16 && !m32 (m32 needs x_frag)"),
    ("N 200", SHAPE, dict(N=200, ldy=264), "N & 15"), ("K 80", SHAPE, dict(K=80), "K & 31"),
    ("two x sources", ARG, dict(src="both"), "exactly one x source"), ("no x source", ARG, dict(src="none"), "exactly one x source"),
    ("no norm_w", ARG, dict(norm_w=False), "(h_rows || h_parts) && !norm_w"), ("no w_frag", ARG, dict(w=False), "!w_frag"),
    ("S 0", ARG, dict(src="parts", S=0), "h_parts && S < 1"), ("S 17", ARG, dict(src="parts", S=17), "h_parts && S > 16"),
    ("res_out == res_in", ARG, dict(inplace=True), "res_out == res_in"),
    ("waves 17", ARG, dict(waves=17), "waves > 16"), ("nt 3", ARG, dict(nt=3), "launch_fused_nt: nt not 1, 2, 4"),
    ("nt 8", ARG, dict(nt=8), "groups % nt"), ("nt 4 of 10 groups", ARG, dict(nt=4, N=160, ldy=160), "groups % nt"),
    ("ROWS no y", ARG, dict(y=False), "FEPI_ROWS && !y"), ("ROWS ldy 0", SHAPE, dict(ldy=0), "FEPI_ROWS && ldy < N"),
    ("ROWS ldy N - 16", SHAPE, dict(ldy=ROWS_N - 16), "FEPI_ROWS && ldy < N"),
    ("SILU no y", ARG, dict(epi=SI, nt=2, y=False), "FEPI_SILU_FRAG && !y"), ("SILU nt 1", ARG, dict(epi=SI, nt=1), "FEPI_SILU_FRAG && (nt & 1)"),
    ("SILU nt 3", ARG, dict(epi=SI, nt=3), "FEPI_SILU_FRAG && (nt & 1)"),
    ("SILU N 96", SHAPE, dict(epi=SI, nt=2, N=96), "FEPI_SILU_FRAG && (N & 63): N % 32 != 0, and N / 2 not whole k-tiles"),
    ("SILU N 80", SHAPE, dict(epi=SI, nt=1, N=80), "FEPI_SILU_FRAG && (N & 63)"),
    ("SILU bias", ARG, dict(epi=SI, nt=2, bias=True), "FEPI_SILU_FRAG && bias"),
    ("epilogue 2", ARG, dict(epi=2), "switch (epilogue) default"), ("epilogue 7", ARG, dict(epi=7), "switch (epilogue) default"),
    ("QKV no positions", ARG, dict(epi=Q, drop="positions"), "!positions"), ("QKV no cos_sin", ARG, dict(epi=Q, drop="cos_sin"), "!cos_sin"),
    ("QKV no slots", ARG, dict(epi=Q, drop="slots"), "!slots"), ("QKV no q_out", ARG, dict(epi=Q, drop="q_out"), "!q_out"),
    ("QKV no k_cache", ARG, dict(epi=Q, drop="k_cache"), "!k_cache"), ("QKV no v_cache", ARG, dict(epi=Q, drop="v_cache"), "!v_cache"),
    ("QKV hd 96", SHAPE, dict(epi=Q, hd=96), "hd != 64 && hd != 128 && hd != 256"), ("QKV N mismatch", SHAPE, dict(epi=Q, nh=5), "N != (nh + 2 nkv) hd"),
    ("QKV block_size 0", SHAPE, dict(epi=Q, bs=0), "block_size <= 0"), ("QKV block_size -16", SHAPE, dict(epi=Q, bs=-16), "block_size <= 0"),
    ("LDS ceiling M 16 K 4096", SHAPE, dict(M=16, K=4096, N=64, ldy=64, nt=1, waves=8), "launch_fused_c: lds > 160 KiB"),
    ("LDS ceiling, parts", SHAPE, dict(M=16, K=4096, N=64, ldy=64, nt=1, waves=8, src="parts", S=2), "launch_fused_c: lds > 160 KiB"),
)


def test_fused_refusal_table():
    whats = [r[0] for r in FUSED_REFUSALS]
    assert len(set(whats)) == len(whats) and {r[1] for r in FUSED_REFUSALS} == {SHAPE, ARG}
    for need in ("no w_frag", "ROWS no y", "SILU no y", "ROWS ldy 0", "QKV block_size 0", "SILU N 96", "waves 17", "S 0", "S 17", "M 33 two tiles",
                 "nt 4 of 10 groups", "SILU nt 3", "LDS ceiling M 16 K 4096"):
        assert need in whats
    M, K, nt, w = CEILING
    assert lds_bytes(16, K, nt, w, True) > LDS_LIMIT


@gpu
def test_fused_refusals_return_their_code_and_write_nothing(dev):
    from ssd_amd.hip import ops as Hh
    Kmax = 4096
    g = torch.Generator().manual_seed(0)
    h = torch.randn(33, Kmax, generator=g).to(BF).to(dev)
    res = torch.randn(33, Kmax, generator=g).to(BF).to(dev)
    parts = torch.randn(2, 33, Kmax, generator=g).to(dev)
    xf = torch.randn(48 * Kmax, generator=g).to(BF).to(dev)
    nw = norm_weight(Kmax, g).to(dev)
    wf = (torch.randn(512 * Kmax, generator=g) * 0.05).to(BF).to(dev)
    bias = torch.zeros(512, dtype=BF, device=dev)
    nh, nkv, hd, bs = 4, 2, 64, 16
    yb, rb = sentinel(48 * 512, device=dev), sentinel(33 * Kmax, device=dev)
    q_out, kc, vc = sentinel(33, nh * hd, device=dev), sentinel(NB, nkv, bs, hd, device=dev), sentinel(NB, nkv, bs, hd, device=dev)
    pos = torch.zeros(33, dtype=torch.int64, device=dev)
    slots = torch.arange(33, dtype=torch.int32, device=dev)

    def call(a):
        epi = a.get("epi", R)
        N = a.get("N", 512 if epi == Q else ROWS_N)
        kw = dict(nt=a.get("nt", 1 if epi != SI else 2), waves=a.get("waves", 4), bias=bias if a.get("bias") else None)
        src = a.get("src", "h")
        if src in ("h", "both"):
            kw.update(h_rows=h)
        if src in ("frag", "both"):
            kw.update(x_frag=xf)
        if src == "parts":
            kw.update(h_parts=parts, splits=a["S"])
        if src != "frag":
            kw.update(norm_w=nw if a.get("norm_w", True) else None, eps=EPS, res_in=res, res_out=res if a.get("inplace") else rb)
        if epi != Q:
            kw.update(y=yb if a.get("y", True) else None, ldy=a.get("ldy", N if epi == R else 0))
        if epi == Q:
            rope = dict(positions=pos, cos_sin=cs_dev(dev, 64), slots=slots, q_out=q_out, k_cache=kc, v_cache=vc)
            rope.pop(a.get("drop", ""), None)
            kw.update(rope, nh=a.get("nh", nh), nkv=nkv, hd=a.get("hd", hd), block_size=a.get("bs", bs))
        Hh.gemm_fused(wf if a.get("w", True) else None, a.get("M", 8), N, a.get("K", 96), epi, **kw)

    for what, code, a, line in FUSED_REFUSALS:
        refused_with(dev, f"fused {what} ({line})", code, lambda: call(a), yb, rb, q_out, kc, vc)
    # a valid launch afterwards still works
    weights = _Weights(dev)
    c = FC("rows", R, 8, ROWS_N, 96, 2, 4, "h", 0, True, True, True, 0, 0)
    s = _Src(dev, 8, 96, "h", 0, True, seed=9)
    wr, w64, b, _ = weights.real("rows", ROWS_N, 96)
    x64 = _read_xhat(dev, weights, c, s).double()
    assert_within_ulp(_rows_launch(dev, wr, c, s, bias=b.to(dev))[0], x64 @ w64.T + b.double(), "rows after the refusals")
    print(f"fused refusals: {len(FUSED_REFUSALS)} refused, nothing written")
