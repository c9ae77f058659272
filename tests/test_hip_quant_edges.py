"""The three weight-only GEMM families (csrc/gemm_fp8.hip, gemm_w4a16.hip, gemm_mxfp4.hip) at the edges their per-format test files do
not visit.  The three families are instantiations of one kernel skeleton (wq_gemm_kernel, csrc/gemm_wq.h: K dealt to the waves in
runs of U units with a remainder loop on the last wave, a token-tile clamp, a next-tile prefetch with a pointer advance, an LDS
split-K combine, two epilogues) with a per-format policy struct for the K unit, the side-band and the conversion -- so one harness
drives all three through a small per-format adapter:

  * K unit counts that are not a multiple of U, smaller than U, and smaller than waves * U (idle waves in the combine);
  * every M around the 16-row tile boundaries, so every token-tile template runs with tiles past the last one and a ragged last tile;
  * consecutive tiles per workgroup (tpw) with a ragged last workgroup and tpw beyond the tile count: bit-identical across tpw;
  * sentinel-guarded outputs (rows >= M, columns in [N, ldy), the tail past the SILU fragment);
  * NaN / Inf in the padding rows of the x fragment: rows < M bit-identical to the zero-padded run;
  * SILU_FRAG with a bias in packed (gate / up interleaved) order;
  * 1, 2, 3, 5 row groups, and the refusals of the _cfg forms.

Reference: float64 x @ W_exact.T (+ bias), W_exact from each format's definition.  Bars (those of tests/test_hip_mxfp4.py, imported):
ROWS |HIP - bf16(f64)| <= 1 bf16 ulp with the ulp floored at 2^-6 of the output rms; SILU_FRAG 3 ulp plus the first-order gate / up
term.  The case table is plain Python (`table(fmt)`): the unmarked test checks what it covers, the GPU tests run it and count."""
from __future__ import annotations

from typing import NamedTuple

import pytest
import torch

from ssd_amd.hip.ops import EPI_ROWS, EPI_SILU_FRAG
from tests.test_hip_fp8 import _quantized as _f8_quantized
from tests.test_hip_mxfp4 import _codes as _mx4_codes, _exact as _mx4_exact, _frag as _mx4_frag
from tests.test_hip_mxfp4 import _x, assert_silu_within_bar, assert_within_ulp, dev  # noqa: F401  (dev is the fixture)
from tests.test_hip_prefill_long import SENTINEL
from tests.test_hip_w4a16 import _codes as _w4_codes, _frag as _w4_frag

gpu = pytest.mark.gpu
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------
# Per-format adapters.  `kernels` restates each policy's FORMS table (Fp8::FORMS, W4<ZP>::FORMS, Mx4::FORMS in the three .hip files):
# (token-tile template, nt, deep) -> (U, x staged with the codes).
# ---------------------------------------------------------------------------------------------------------------------
_W4_KERNELS = {
    (1, 1, False): (2, True), (1, 1, True): (8, False), (1, 2, False): (1, True), (1, 2, True): (4, False),
    (1, 4, False): (1, True), (1, 4, True): (2, False), (2, 1, False): (2, True), (2, 2, False): (1, True),
    (4, 1, False): (1, True), (4, 2, False): (1, True), (8, 1, False): (1, False), (8, 2, False): (1, False),
}


class _Fp8:
    """e4m3fn codes [N, K] (uint8) and one fp32 scale per row; a unit is 64 columns."""
    name, kunit = "fp8", 64
    kernels = {
        (1, 1, False): (4, True), (1, 1, True): (6, True), (1, 2, False): (2, True), (1, 2, True): (4, True),
        (1, 4, False): (1, True), (1, 4, True): (2, True), (2, 1, False): (2, True), (2, 2, False): (2, True),
        (4, 1, False): (1, True), (4, 2, False): (1, True), (8, 1, False): (1, True), (8, 2, False): (1, True),
    }

    def rows(self, N, K, dev, seed):
        q, s, _, _ = _f8_quantized(N, K, dev, seed)
        return q.view(torch.uint8), s

    def exact(self, rows):
        """(-1)^sign * 2^(e - 7) * (1 + m / 8), subnormal 2^-6 * m / 8 at e = 0 (OCP e4m3fn), times the row's scale."""
        codes, s = rows
        c = codes.to(torch.int64)
        assert not bool(((c & 0x7f) == 0x7f).any()), "a NaN code"
        e, m = ((c >> 3) & 15).double(), (c & 7).double()
        v = torch.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * torch.exp2(e - 7))
        return torch.where((c & 0x80) != 0, -v, v) * s.double()[:, None]

    def frag(self, rows, N, K, dev, rmap):
        from ssd_amd.hip import quant_ops as Q
        codes, s = rows
        out = torch.empty(N * K, dtype=torch.uint8, device=dev)
        Q.fp8_rows_to_frag(codes, out, N, K, row_map=rmap)
        return out, (s if rmap is None else s[rmap.long()].contiguous())

    def gemm(self, xf, w, y, M, N, K, ldy, epilogue, bias, cfg):
        from ssd_amd.hip import quant_ops as Q
        Q.gemm_fp8(xf, w[0], w[1], y, M, N, K, ldy, epilogue=epilogue, bias=bias, cfg=cfg)


class _W4:
    """int4 codes in [-8, 7] and one bf16 scale per row and 128 columns; a unit is 128 columns."""
    name, kunit, kernels = "w4a16", 128, _W4_KERNELS

    def rows(self, N, K, dev, seed):
        return _w4_codes(N, K, dev, seed)                       # q, s, packed

    def exact(self, rows):
        """s[n, k / 128] * q[n, k], q decoded from the packed words the kernel is given: column 8j + i in bits 4i .. 4i+3 of word j,
        stored as q + 8."""
        q, s, packed = rows
        shifts = torch.arange(0, 32, 4, dtype=torch.int64, device=packed.device)
        codes = (((packed.to(torch.int64)[..., None] >> shifts) & 15) - 8).reshape(q.shape)
        assert torch.equal(codes, q.to(torch.int64))
        return codes.double() * s.double().repeat_interleave(128, dim=1)

    def frag(self, rows, N, K, dev, rmap):
        return _w4_frag(rows[2], rows[1], N, K, dev, rmap)

    def gemm(self, xf, w, y, M, N, K, ldy, epilogue, bias, cfg):
        from ssd_amd.hip import w4_ops as W4
        W4.gemm_w4a16(xf, w[0], w[1], y, M, N, K, ldy, epilogue=epilogue, bias=bias, cfg=cfg)


class _Mx4:
    """e2m1 codes and one e8m0 scale byte per row and 32 columns; a unit is 128 columns."""
    name, kunit, kernels = "mxfp4", 128, _W4_KERNELS

    def rows(self, N, K, dev, seed):
        return _mx4_codes(N, K, dev, seed)                      # packed, s

    def exact(self, rows):
        return _mx4_exact(rows[0], rows[1])

    def frag(self, rows, N, K, dev, rmap):
        return _mx4_frag(rows[0], rows[1], N, K, dev, rmap)

    def gemm(self, xf, w, y, M, N, K, ldy, epilogue, bias, cfg):
        from ssd_amd.hip import mx4_ops as MX4
        MX4.gemm_mxfp4(xf, w[0], w[1], y, M, N, K, ldy, epilogue=epilogue, bias=bias, cfg=cfg)


FORMATS = {f.name: f for f in (_Fp8(), _W4(), _Mx4())}
FMT = pytest.mark.parametrize("fmt", list(FORMATS.values()), ids=list(FORMATS))


# ---------------------------------------------------------------------------------------------------------------------
# The case table
# ---------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    sweep: str
    M: int
    N: int
    K: int
    epilogue: int
    bias: bool
    nt: int          # 0: the default dispatch (deep, waves, tpw unused)
    deep: bool
    waves: int
    tpw: int         # 0: not given (one tile per workgroup)


SWEEPS = ("m", "k", "tile", "bounds", "poison", "silu_bias")
M_SWEEP = (1, 2, 15, 16, 17, 31, 32, 33, 40, 47, 48, 49, 63, 64, 65, 80, 81, 96, 97, 111, 112, 113, 127, 128)
K_UNITS = (1, 2, 3, 5, 7, 9, 11, 13, 17, 20, 21, 22)
TILE_GROUPS = (1, 2, 3, 5, 6, 12, 20, 36)
TILE_TPW = (1, 2, 3, 5, 8)
POISON_M = (1, 7, 17, 40, 100)


def mtr(M: int) -> int:
    """The token-tile template (MT) the _cfg forms pick for M rows."""
    t = (M + 15) // 16
    return 1 if t == 1 else 2 if t == 2 else 4 if t <= 4 else 8


def valid(fmt, M, N, K, epilogue, nt, deep, waves) -> bool:
    """The rules of the headers and of wq_gemm_cfg / the FORMS tables / wq_launch (csrc/gemm_wq.h)."""
    if not 1 <= M <= 128 or N <= 0 or N % 16 or K <= 0 or K % fmt.kunit:
        return False
    if not 1 <= waves <= 8 or nt not in (1, 2, 4) or (N // 16) % nt:
        return False
    if epilogue == EPI_SILU_FRAG and (nt % 2 or N % 64):
        return False
    if (deep or nt == 4) and M > 16:
        return False
    return waves * nt * mtr(M) * 1024 <= 65536


def decomps(fmt, M, N, K, epilogue, waves=range(1, 9)):
    return [(nt, deep, w) for nt in (1, 2, 4) for deep in (False, True) for w in waves if valid(fmt, M, N, K, epilogue, nt, deep, w)]


def table(fmt) -> list[Case]:
    ku = fmt.kunit
    R, S = EPI_ROWS, EPI_SILU_FRAG
    t: list[Case] = []

    # M sweep: a small matrix with an odd unit count (9 x 128, 17 x 64), every valid explicit decomposition and the default one
    N, K = 192, 1152 if ku == 128 else 1088
    for M in M_SWEEP:
        for epi, bias in ((R, False), (R, True), (S, False)):
            t.append(Case("m", M, N, K, epi, bias, 0, False, 0, 0))
            t += [Case("m", M, N, K, epi, bias, nt, deep, w, 0) for nt, deep, w in decomps(fmt, M, N, K, epi)]
    for N, K, forms in ((6144, 4096, ((R, True),)), (28672, 4096, ((S, False), (R, False)))):    # 8B qkv and gate_up grids ...
        for M in (40, 72, 100, 120):                                                             # ... at 3, 5, 7, 8 token tiles
            t += [Case("m", M, N, K, epi, bias, 0, False, 0, 0) for epi, bias in forms]

    # K sweep
    N = 192
    for units in K_UNITS:
        for M in (8, 24, 40, 72):
            for epi in (R, S):
                t += [Case("k", M, N, units * ku, epi, epi == R, nt, deep, w, 0) for nt, deep, w in decomps(fmt, M, N, units * ku, epi)]
    for N, K in ((2560, 9728), (19456, 2560), (896, 4864), (1152, 896)):    # hidden 2560 / MLP 9728, hidden 896 / MLP 4864
        for M in (8, 40):
            t.append(Case("k", M, N, K, R, True, 0, False, 0, 0))
            if N == 19456:
                t.append(Case("k", M, N, K, S, False, 0, False, 0, 0))

    # tile sweep: 5 K units (not a multiple of, or fewer than, every U > 1)
    K = 5 * ku
    for groups in TILE_GROUPS:
        N = groups * 16
        for M in (8, 24, 40, 100):
            for epi in (R, S) if N % 64 == 0 else (R,):
                t.append(Case("tile", M, N, K, epi, epi == R, 0, False, 0, 0))
                for nt, deep, w in decomps(fmt, M, N, K, epi, waves=(1, 3, 8)):
                    t += [Case("tile", M, N, K, epi, epi == R, nt, deep, w, tpw) for tpw in TILE_TPW]

    # bounds: a ragged M for every token-tile template, every nt, with and without consecutive tiles
    N, K = 320, 5 * ku
    for M in (7, 23, 39, 55, 100, 121):
        for epi in (R, S):
            t.append(Case("bounds", M, N, K, epi, True, 0, False, 0, 0))
            for nt, deep, w in decomps(fmt, M, N, K, epi, waves=(2, 5)):
                t += [Case("bounds", M, N, K, epi, True, nt, deep, w, tpw) for tpw in (0, 3)]

    # poisoned padding
    N, K = 192, 9 * ku
    for M in POISON_M:
        for epi in (R, S):
            t.append(Case("poison", M, N, K, epi, False, 0, False, 0, 0))
            t += [Case("poison", M, N, K, epi, False, nt, deep, w, 2) for nt, deep, w in decomps(fmt, M, N, K, epi, waves=(4,))]

    # SILU_FRAG + bias: 32 gate / up pairs of row groups, one and several token tiles
    N, K = 1024, 9 * ku
    for M in (8, 24, 40, 100):
        t.append(Case("silu_bias", M, N, K, S, True, 0, False, 0, 0))
        for nt, deep, w in decomps(fmt, M, N, K, S, waves=(1, 4)):
            t += [Case("silu_bias", M, N, K, S, True, nt, deep, w, tpw) for tpw in (0, 3)]
    return t


@FMT
def test_case_table_covers_every_kernel_and_every_edge(fmt):
    t = table(fmt)
    assert len(set(t)) == len(t), "duplicate cases"
    assert {c.sweep for c in t} == set(SWEEPS)            # each sweep is run, and counted, by one GPU test below
    explicit = [c for c in t if c.nt]
    assert all(valid(fmt, c.M, c.N, c.K, c.epilogue, c.nt, c.deep, c.waves) for c in explicit)
    assert all(c.M <= 128 and c.N % 16 == 0 and c.K % fmt.kunit == 0 for c in t)
    assert all(c.K <= 2816 and c.N <= 1024 for c in explicit)           # small shapes: the f64 reference stays cheap
    for (mt, nt, deep), (U, xs) in fmt.kernels.items():
        mine = [c for c in explicit if (mtr(c.M), c.nt, c.deep) == (mt, nt, deep)]
        units = lambda c: c.K // fmt.kunit                              # noqa: E731
        what = f"{fmt.name} kernel MT {mt} NT {nt} U {U} staged-x {xs}"
        if U > 1:                                                       # with U = 1 there is no remainder
            assert any(units(c) % U and units(c) > U for c in mine), f"{what}: no K with a remainder after full runs"
            assert any(units(c) < U for c in mine), f"{what}: no K below one run"
        assert any(c.waves * U > units(c) for c in mine), f"{what}: no idle wave"
        assert any(c.tpw and ((c.N // 16) // c.nt) % c.tpw for c in mine), f"{what}: no ragged last workgroup"
        assert any(c.tpw > (c.N // 16) // c.nt for c in mine), f"{what}: no tpw beyond the tile count"
        for epi in (EPI_ROWS, EPI_SILU_FRAG) if nt > 1 else (EPI_ROWS,):
            assert any(c.epilogue == epi for c in mine), f"{what}: epilogue {epi} not run"
    for sweep in ("m", "bounds"):
        for tiles in range(1, 9):
            ms = {c.M for c in t if c.sweep == sweep and (c.M + 15) // 16 == tiles}
            if sweep == "m":
                assert any(m % 16 == 0 for m in ms), f"no full last tile at {tiles} token tiles"
            if sweep == "m" or tiles in (1, 2, 3, 4, 7, 8):
                assert any(m % 16 for m in ms), f"{sweep}: no ragged last tile at {tiles} token tiles"
    assert {c.M for c in t if c.sweep == "m" and c.N == 192} == set(M_SWEEP)
    assert {c.K // fmt.kunit for c in t if c.sweep == "k" and c.nt} == set(K_UNITS)
    assert {c.N // 16 for c in t if c.sweep == "tile"} == set(TILE_GROUPS) and {c.tpw for c in t if c.sweep == "tile" and c.nt} == set(TILE_TPW)
    assert {c.M for c in t if c.sweep == "poison"} == set(POISON_M)
    assert {mtr(c.M) for c in t if c.sweep == "bounds" and c.M % 16} == {1, 2, 4, 8}
    assert any(c.sweep == "silu_bias" and mtr(c.M) == 1 for c in t) and any(c.sweep == "silu_bias" and mtr(c.M) > 1 for c in t)


# ---------------------------------------------------------------------------------------------------------------------
# The harness
# ---------------------------------------------------------------------------------------------------------------------
class _Harness:
    """Weights, their fragment forms, x and the f64 reference of one (N, K) at a time (the table is shape-major)."""

    def __init__(self, fmt, dev):
        self.fmt, self.dev, self.shape, self.ran = fmt, dev, None, 0

    def _at(self, N, K):
        if self.shape == (N, K):
            return
        self.shape = self.w = self.frags = self.xs = self.refs = self.biases = None
        torch.cuda.empty_cache()
        self.shape, self.frags, self.xs, self.refs, self.biases = (N, K), {}, {}, {}, {}
        self.rows = self.fmt.rows(N, K, self.dev, seed=N + K)
        self.w = self.fmt.exact(self.rows)
        assert self.w.shape == (N, K) and self.w.dtype == torch.float64

    def rmap(self, c):
        from ssd_amd.quant import gate_up_row_map
        return gate_up_row_map(c.N).to(self.dev) if c.epilogue == EPI_SILU_FRAG else None

    def frag(self, c):
        silu = c.epilogue == EPI_SILU_FRAG
        if silu not in self.frags:
            self.frags[silu] = self.fmt.frag(self.rows, c.N, c.K, self.dev, self.rmap(c))
        return self.frags[silu]

    def x(self, c):
        if c.M not in self.xs:
            self.xs[c.M] = _x(c.M, c.K, self.dev, seed=c.M)          # fragment padding rows are zero
        return self.xs[c.M]

    def bias(self, c):
        """bf16 [N] in the order of the kernel's rows (packed for SILU_FRAG), or None."""
        if not c.bias:
            return None
        if c.epilogue not in self.biases:
            g = torch.Generator(device=self.dev).manual_seed(7 + c.epilogue)
            self.biases[c.epilogue] = (torch.randn(c.N, generator=g, device=self.dev) * 0.1).to(BF)
        return self.biases[c.epilogue]

    def ref(self, c):
        """f64 [M, N] in SOURCE row order (gate rows, then up rows): x @ W.T + bias[packed index of the row]."""
        key = (c.M, c.epilogue, c.bias)
        if key not in self.refs:
            want = self.x(c)[0].double() @ self.w.T
            if c.bias:
                b, rmap = self.bias(c).double(), self.rmap(c)
                if rmap is None:
                    want = want + b
                else:
                    src = torch.empty_like(b)
                    src[rmap.long()] = b                               # packed row d holds source row rmap[d]
                    want = want + src
            self.refs[key] = want
        return self.refs[key]

    def launch(self, c, y, ldy, xf=None):
        self._at(c.N, c.K)
        cfg = None if not c.nt else (c.nt | (256 if c.deep else 0), c.waves | (c.tpw << 8))
        self.fmt.gemm(self.x(c)[1] if xf is None else xf, self.frag(c), y, c.M, c.N, c.K, ldy, c.epilogue, self.bias(c), cfg)
        self.ran += 1

    def out(self, c, xf=None):
        """The kernel's output as bf16 rows: [M, N], or [M, N / 2] through the SILU fragment."""
        from ssd_amd.hip import ops as H
        if c.epilogue == EPI_ROWS:
            y = torch.empty(c.M, c.N, dtype=BF, device=self.dev)
            self.launch(c, y, c.N, xf)
            return y
        I = c.N // 2
        yf = torch.zeros(H.frag_numel(c.M, I), dtype=BF, device=self.dev)
        self.launch(c, yf, 0, xf)
        y = torch.empty(c.M, I, dtype=BF, device=self.dev)
        H.frag_to_rows(yf, y, c.M, I)
        return y

    def check(self, c, y):
        what = f"{self.fmt.name} {c}"
        if c.epilogue == EPI_ROWS:
            assert_within_ulp(y, self.ref(c), what)
        else:
            assert_silu_within_bar(y, self.ref(c), c.N // 2, what)


def _cases(fmt, sweep):
    cases = [c for c in table(fmt) if c.sweep == sweep]
    assert cases
    return cases


def _bits(y):
    return y.contiguous().view(torch.int16)


def _run_and_check(fmt, dev, sweep):
    h, cases = _Harness(fmt, dev), _cases(fmt, sweep)
    for c in cases:
        h.check(c, h.out(c))
    assert h.ran == len(cases)
    print(f"{fmt.name} {sweep}: {h.ran} cases")


@gpu
@FMT
def test_m_sweep(dev, fmt):
    """Every M around the tile boundaries: tiles past the last one re-read it (MT = 4 / 8 templates), ragged last tiles."""
    _run_and_check(fmt, dev, "m")


@gpu
@FMT
def test_k_sweep(dev, fmt):
    """K remainder loop, K below one run (all work on the last wave), idle waves in the combine."""
    _run_and_check(fmt, dev, "k")


@gpu
@FMT
def test_silu_frag_with_bias_in_packed_order(dev, fmt):
    _run_and_check(fmt, dev, "silu_bias")


@gpu
@FMT
def test_tile_sweep_bit_identical_across_tiles_per_workgroup(dev, fmt):
    """tpw changes which workgroup owns a tile, never the K order: runs that differ only in tpw are bit-identical."""
    h, cases, first = _Harness(fmt, dev), _cases(fmt, "tile"), {}
    for c in cases:
        y = h.out(c)
        h.check(c, y)
        if c.nt:
            base = first.setdefault(c._replace(tpw=0), (c.tpw, y))
            assert torch.equal(_bits(y), _bits(base[1])), f"{fmt.name} {c}: differs from the tpw = {base[0]} run"
    assert h.ran == len(cases)
    print(f"{fmt.name} tile: {h.ran} cases")


@gpu
@FMT
def test_cfg_refusals_return_an_error_and_launch_nothing(dev, fmt):
    from ssd_amd.hip.lib import SsdHipError
    h, ku = _Harness(fmt, dev), fmt.kunit
    R, S = EPI_ROWS, EPI_SILU_FRAG
    refused = [
        Case("refuse", 8, 48, 5 * ku, R, False, 2, False, 4, 0),        # nt does not divide 3 row groups
        Case("refuse", 8, 96, 5 * ku, R, False, 4, False, 4, 0),        # ... nor 6
        Case("refuse", 8, 80, 5 * ku, R, False, 2, False, 4, 0),        # ... nor 5
        Case("refuse", 8, 192, 5 * ku, R, False, 3, False, 4, 0),       # nt not in {1, 2, 4}
        Case("refuse", 8, 192, 5 * ku, S, False, 1, False, 4, 0),       # SILU_FRAG needs gate / up pairs
        Case("refuse", 8, 96, 5 * ku, S, False, 2, False, 4, 0),        # SILU_FRAG needs N % 64 == 0
        Case("refuse", 8, 192, 5 * ku, R, False, 1, False, 9, 0),       # waves beyond 8
        Case("refuse", 24, 192, 5 * ku, R, False, 2, True, 4, 0),       # deep is for one token tile
        Case("refuse", 24, 192, 5 * ku, R, False, 4, False, 4, 0),      # so is nt = 4
        Case("refuse", 100, 192, 5 * ku, R, False, 2, False, 8, 0),     # combine beyond 64 KiB of LDS
        Case("refuse", 100, 192, 5 * ku, S, False, 2, False, 5, 0),
    ]
    for c in refused:
        assert not valid(fmt, c.M, c.N, c.K, c.epilogue, c.nt, c.deep, c.waves)
        rows = (c.M + 15) // 16 * 16
        yb = torch.full((rows * c.N,), SENTINEL, dtype=torch.int16, device=dev)
        with pytest.raises(SsdHipError):
            h.launch(c, yb.view(BF), c.N)
        torch.cuda.synchronize()
        assert bool((yb == SENTINEL).all()), f"{fmt.name} {c}: refused, yet something was written"
    # waves = 0, ldy < N and a K that is no multiple of the unit are refused before any weight is touched
    c = Case("refuse", 8, 192, 5 * ku, R, False, 1, False, 4, 0)
    h._at(c.N, c.K)
    yb = torch.full((16 * c.N,), SENTINEL, dtype=torch.int16, device=dev)
    x, w = h.x(c)[1], h.frag(c)
    for M, N, K, ldy, cfg in ((8, c.N, c.K, c.N, (1, 0)), (8, c.N, c.K, c.N - 16, (1, 4)), (8, c.N, c.K - 32, c.N, (1, 4)),
                              (129, c.N, c.K, c.N, (1, 4)), (8, c.N - 8, c.K, c.N, (1, 4))):
        with pytest.raises(SsdHipError):
            fmt.gemm(x, w, yb.view(BF), M, N, K, ldy, R, None, cfg)
        if cfg == (1, 4):
            with pytest.raises(SsdHipError):
                fmt.gemm(x, w, yb.view(BF), M, N, K, ldy, R, None, None)
    torch.cuda.synchronize()
    assert bool((yb == SENTINEL).all())


@gpu
@FMT
def test_bounds_rows_past_m_columns_past_n_and_the_fragment_tail_stay_untouched(dev, fmt):
    """ROWS into ceil16(M) + 16 rows of N + 64 columns (a whole token tile of slack, so an unguarded store of a wrong kernel still
    lands in this allocation); SILU_FRAG into its fragment plus a tail.  All prefilled with a NaN pattern no kernel produces."""
    from ssd_amd.hip import ops as H
    h, cases = _Harness(fmt, dev), _cases(fmt, "bounds")
    for c in cases:
        if c.epilogue == EPI_ROWS:
            rows, ldy = (c.M + 15) // 16 * 16 + 16, c.N + 64
            yb = torch.full((rows * ldy,), SENTINEL, dtype=torch.int16, device=dev)
            h.launch(c, yb.view(BF), ldy)
            raw = yb.view(rows, ldy)
            assert bool((raw[c.M:] == SENTINEL).all()), f"{fmt.name} {c}: a row >= M was written"
            assert bool((raw[:c.M, c.N:] == SENTINEL).all()), f"{fmt.name} {c}: a column >= N (inside ldy) was written"
            y = yb.view(BF).view(rows, ldy)[:c.M, :c.N].contiguous()
        else:
            I, tail = c.N // 2, 4096
            numel = H.frag_numel(c.M, I)
            yb = torch.full((numel + tail,), SENTINEL, dtype=torch.int16, device=dev)
            h.launch(c, yb.view(BF), 0)
            assert bool((yb[numel:] == SENTINEL).all()), f"{fmt.name} {c}: memory past the output fragment was written"
            y = torch.empty(c.M, I, dtype=BF, device=dev)
            H.frag_to_rows(yb.view(BF)[:numel].contiguous(), y, c.M, I)
        assert bool(torch.isfinite(y.float()).all()), f"{fmt.name} {c}: an output element was left unwritten"
        h.check(c, y)
    assert h.ran == len(cases)
    print(f"{fmt.name} bounds: {h.ran} cases")


@gpu
@FMT
def test_poisoned_x_padding_rows_never_reach_a_real_output(dev, fmt):
    """With nt > 1 the kernels load the padding rows (>= M) of the last x tile, and the engine reuses x buffers.  An MFMA output
    column depends only on the same column of its B operand -- one token row here -- so rows < M must not change by one bit."""
    from ssd_amd.hip import ops as H
    h, cases = _Harness(fmt, dev), _cases(fmt, "poison")
    poison = torch.tensor([0x7FC0, 0x7F80, -128, SENTINEL, -1, 0x7F81], dtype=torch.int16, device=dev)   # NaNs, +Inf, -Inf (0xFF80)
    for c in cases:
        clean = h.out(c)
        h.check(c, clean)
        x, xf = h.x(c)
        rows = (c.M + 15) // 16 * 16
        pad = poison[torch.arange((rows - c.M) * c.K, device=dev) % poison.numel()].view(rows - c.M, c.K)
        x16 = torch.cat((x.view(torch.int16), pad)).contiguous().view(BF)
        xp = torch.empty_like(xf)
        H.rows_to_frag(x16, xp, rows, c.K)
        assert not torch.equal(_bits(xp), _bits(xf)) and not bool(torch.isfinite(xp.float()).all())
        dirty = h.out(c, xf=xp)
        assert torch.equal(_bits(dirty), _bits(clean)), f"{fmt.name} {c}: padding rows of x changed a row < M"
    assert h.ran == 2 * len(cases)
    print(f"{fmt.name} poison: {len(cases)} cases, each run twice")
