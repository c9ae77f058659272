"""The bf16 GEMM families (csrc/gemm.hip, gemm_sk.hip, gemm_pf.hip at M <= 128) at the edges tests/test_hip_ops.py and test_hip_fuzz.py
do not visit -- the walk the weight-only kernels of tests/test_hip_quant_edges.py were copied from, under the same harness:

  A  ssd_gemm_wf_cfg / ssd_gemm_wf   gemm_wf_kernel<MT, NT, EPI, DEEP>: K remainders, K below one run, idle waves, every M around the
                                     16-row borders with every valid decomposition (MT = 4 / 8 templates included), tiles per workgroup;
  B  ssd_gemm_splitk                 gemm_sk_kernel: uneven K slices, slices shorter than one run, more waves than runs, counters;
  C  ssd_gemm_parts                  gemm_sp_kernel<TPW, MT>: every TPW template with clamped slots, slabs and their consumer's sum;
  D  ssd_gemm_pf_cfg / ssd_gemm_pf   gemm_pf_kernel at 17 <= M <= 128: every instantiation at ragged M, nk == U (every look-ahead load
                                     clamped), the three epilogues split and unsplit, launch-shape identity at every M;

each with sentinel-guarded outputs (rows >= M, columns in [N, ldy), fragment and workspace tails), NaN-prefilled workspaces, NaN / Inf in
the padding rows of the x fragment, and the refusals of the entry points (an error, nothing written).

One weight matrix per K, [1024, K] in the kernels' own row order: a GEMM over N <= 1024 rows reads a prefix of its fragment form, so
every N shares one float64 reference.  For SILU_FRAG the 16-row groups of that order alternate gate, up, and so does the bias.

Reference and bars (tests/test_hip_mxfp4.py's, imported): float64 x @ W.T (+ bias) on the bf16 operand values; ROWS |HIP - bf16(f64)|
<= 1 bf16 ulp with the ulp floored at 2^-6 of the output rms; SILU_FRAG 3 ulp plus the first-order gate / up term; fp32 rows and fp32
slabs 1e-3 absolute (tests/test_hip_ops.py test_gemm_vs_oracle) against the f64 product over the same K range, x ~ N(0, 1),
W ~ 0.05 N(0, 1).  The case tables are plain Python: the unmarked tests check what they cover, the GPU tests run them and count."""
from __future__ import annotations

from typing import NamedTuple

import pytest
import torch

from ssd_amd.hip.ops import EPI_ROWS, EPI_ROWS_F32, EPI_SILU_FRAG, PF_EPI_PARTIALS
from tests.test_hip_mxfp4 import _x, assert_silu_within_bar, assert_within_ulp, dev  # noqa: F401  (dev is the fixture)
from tests.test_hip_quant_edges import K_UNITS as QUANT_K_UNITS
from tests.test_hip_quant_edges import M_SWEEP, POISON_M, SENTINEL, TILE_GROUPS, TILE_TPW, Case, _bits, mtr

gpu = pytest.mark.gpu
BF = torch.bfloat16
R, S, F = EPI_ROWS, EPI_SILU_FRAG, EPI_ROWS_F32
SENTINEL32 = 0x7FA5A5A5        # an fp32 NaN pattern no kernel produces
F32_BAR = 1e-3
NW = 1024                      # rows of the shared weight matrix
TAIL = 4096


def ceil16(M: int) -> int:
    return (M + 15) // 16 * 16


# ---------------------------------------------------------------------------------------------------------------------
# Operands and references
# ---------------------------------------------------------------------------------------------------------------------
class _Mats:
    """W [rows, K] (rows = 1024, or N of a real grid), its fragment form and float64 values; x per M; float64 x @ W.T per (K, M)."""

    def __init__(self, dev):
        self.dev, self.ws, self.xs, self.refs, self.biases = dev, {}, {}, {}, {}

    def w(self, N, K):
        from ssd_amd.hip import ops as H
        rows = NW if N <= NW else N
        if (rows, K) not in self.ws:
            if rows > NW:                                                # a real grid: one at a time
                self.ws, self.refs = {}, {}
                torch.cuda.empty_cache()
            g = torch.Generator(device=self.dev).manual_seed(rows + K)
            w = (torch.randn(rows, K, generator=g, device=self.dev) * 0.05).to(BF)
            w[3, :] = 0.5                                                # asymmetric structure: a permuted tile cannot pass
            wf = torch.empty(rows * K, dtype=BF, device=self.dev)
            H.rows_to_frag(w, wf, rows, K)
            self.ws[(rows, K)] = (wf, w.double())
        return self.ws[(rows, K)]

    def x(self, M, K):
        if (M, K) not in self.xs:
            self.xs[(M, K)] = _x(M, K, self.dev, seed=M)                 # fragment padding rows are zero
        return self.xs[(M, K)]

    def bias(self, N):
        rows = NW if N <= NW else N
        if rows not in self.biases:
            g = torch.Generator(device=self.dev).manual_seed(7 + rows)
            self.biases[rows] = (torch.randn(rows, generator=g, device=self.dev) * 0.1).to(BF)
        return self.biases[rows][:N]

    def ref(self, M, N, K, bias=False, silu=False, k0=0, k1=None):
        """f64 [M, N] over the columns [k0, k1) of K; for silu in (gate | up) order, as assert_silu_within_bar takes it."""
        key = (M, NW if N <= NW else N, K, k0, k1)
        if key not in self.refs:
            w64 = self.w(N, K)[1]
            self.refs[key] = self.x(M, K)[0].double()[:, k0:k1] @ w64[:, k0:k1].T
        want = self.refs[key][:, :N]
        if bias:
            want = want + self.bias(N).double()
        if silu:
            cols = torch.arange(N, device=self.dev).view(-1, 2, 16)
            want = want[:, torch.cat((cols[:, 0].flatten(), cols[:, 1].flatten()))]
        return want

    def poisoned(self, M, K):
        """The x fragment with NaN / Inf / sentinel patterns in rows [M, ceil16(M))."""
        from ssd_amd.hip import ops as H
        x, xf = self.x(M, K)
        rows = ceil16(M)
        assert rows > M
        poison = torch.tensor([0x7FC0, 0x7F80, -128, SENTINEL, -1, 0x7F81], dtype=torch.int16, device=self.dev)
        pad = poison[torch.arange((rows - M) * K, device=self.dev) % poison.numel()].view(rows - M, K)
        x16 = torch.cat((x.view(torch.int16), pad)).contiguous().view(BF)
        xp = torch.empty_like(xf)
        H.rows_to_frag(x16, xp, rows, K)
        assert not torch.equal(_bits(xp), _bits(xf)) and not bool(torch.isfinite(xp.float()).all())
        return xp


class _Worst:
    """Case count and worst ratio to the bar per kind of check, printed once per family and sweep."""

    def __init__(self, name):
        self.name, self.n, self.worst = name, 0, {}

    def add(self, kind, ratio):
        self.worst[kind] = max(self.worst.get(kind, 0.0), ratio)

    def report(self):
        unit = {"ROWS_F32": "x 1e-3", "slab": "x 1e-3"}
        print(f"{self.name}: {self.n} cases, worst " + ", ".join(f"{k} {v:.2f} {unit.get(k, 'x tol')}" for k, v in sorted(self.worst.items())))


def _f32_ratio(got, want64, what):
    ratio = (got.double() - want64).abs().max().item() / F32_BAR
    assert ratio <= 1.0, f"{what}: {ratio:.2f} x 1e-3"
    return ratio


def _guarded_rows(dev, M, N, f32=False):
    """ceil16(M) + 16 rows of N + 64 columns of sentinel: a whole token tile of slack, so an unguarded store of a wrong kernel still
    lands in this allocation."""
    rows, ldy = ceil16(M) + 16, N + 64
    if f32:
        return torch.full((rows * ldy,), SENTINEL32, dtype=torch.int32, device=dev), rows, ldy
    return torch.full((rows * ldy,), SENTINEL, dtype=torch.int16, device=dev), rows, ldy


def _check_guarded_rows(yb, rows, ldy, M, N, what, f32=False):
    sent = SENTINEL32 if f32 else SENTINEL
    raw = yb.view(rows, ldy)
    assert bool((raw[M:] == sent).all()), f"{what}: a row >= M was written"
    assert bool((raw[:M, N:] == sent).all()), f"{what}: a column >= N (inside ldy) was written"
    y = yb.view(torch.float32 if f32 else BF).view(rows, ldy)[:M, :N].contiguous()
    assert bool(torch.isfinite(y.float()).all()), f"{what}: an output element was left unwritten"
    return y


def _guarded_frag(dev, M, I):
    from ssd_amd.hip import ops as H
    return torch.full((H.frag_numel(M, I) + TAIL,), SENTINEL, dtype=torch.int16, device=dev)


def _check_guarded_frag(yb, M, I, what):
    from ssd_amd.hip import ops as H
    numel, rows = H.frag_numel(M, I), ceil16(M)
    assert bool((yb[numel:] == SENTINEL).all()), f"{what}: memory past the output fragment was written"
    y = torch.empty(rows, I, dtype=BF, device=yb.device)
    H.frag_to_rows(yb.view(BF)[:numel].contiguous(), y, rows, I)
    assert bool((_bits(y)[M:] == SENTINEL).all()), f"{what}: a padding row of the output fragment was written"
    y = y[:M].contiguous()
    assert bool(torch.isfinite(y.float()).all()), f"{what}: an output element was left unwritten"
    return y


# =====================================================================================================================
# Family A: ssd_gemm_wf_cfg / ssd_gemm_wf
# =====================================================================================================================
# (token-tile template MT, NT, deep) -> U, the k-tiles per stage: 4 if MT + NT <= 3, 2 if <= 6, else 1; twice that when DEEP
WF_KERNELS = {
    (1, 1, False): 4, (1, 2, False): 4, (1, 4, False): 2, (1, 2, True): 8, (1, 4, True): 4, (2, 1, False): 4, (2, 2, False): 2,
    (2, 4, False): 2, (4, 1, False): 2, (4, 2, False): 2, (8, 1, False): 1, (8, 2, False): 1,
}
WF_SWEEPS = ("m", "k", "tile", "bounds", "poison", "silu_bias")
KU = 32                                          # a K unit: one k-tile
K_UNITS = QUANT_K_UNITS + (67,)                  # 67 > 16 waves x 4: full runs plus a remainder for the 16-wave forms
LDS_KIB = 160


def wf_valid(M, N, K, epilogue, nt, deep, waves) -> bool:
    """The rules of include/ssd_hip_tune.h and of ssd_gemm_wf_cfg / launch_nt / launch_t."""
    if not 1 <= M <= 128 or N <= 0 or N % 16 or K <= 0 or K % KU:
        return False
    if nt not in (1, 2, 4) or (N // 16) % nt or not 1 <= waves <= (8 if deep else 16):
        return False
    if epilogue == S and (nt % 2 or N % 64):
        return False
    if deep and (M > 16 or nt == 1 or epilogue == F):
        return False
    if nt == 4 and mtr(M) > 2:
        return False
    return waves * nt * mtr(M) <= LDS_KIB


def wf_decomps(M, N, K, epilogue, waves=range(1, 17)):
    return [(nt, deep, w) for nt in (1, 2, 4) for deep in (False, True) for w in waves if wf_valid(M, N, K, epilogue, nt, deep, w)]


def wf_table() -> list[Case]:
    t: list[Case] = []

    # M sweep: a small matrix with an odd unit count, every valid explicit decomposition and the default one
    N, K = 192, 37 * KU
    for M in M_SWEEP:
        for epi, bias, waves in ((R, False, range(1, 17)), (R, True, range(1, 17)), (S, False, range(1, 17)), (F, False, (1, 5, 16))):
            t.append(Case("m", M, N, K, epi, bias, 0, False, 0, 0))
            t += [Case("m", M, N, K, epi, bias, nt, deep, w, 0) for nt, deep, w in wf_decomps(M, N, K, epi, waves)]
    for N, K, forms in ((6144, 4096, ((R, True),)), (28672, 4096, ((S, False), (R, False)))):    # 8B qkv and gate_up grids ...
        for M in (40, 72, 100, 120):                                                             # ... at 3, 5, 7, 8 token tiles
            t += [Case("m", M, N, K, epi, bias, 0, False, 0, 0) for epi, bias in forms]

    # K sweep
    N = 192
    for units in K_UNITS:
        for M in (8, 24, 40, 72):
            for epi, waves in ((R, (1, 2, 3, 5, 8, 13, 16)), (S, (1, 2, 3, 5, 8, 13, 16)), (F, (3,))):
                t += [Case("k", M, N, units * KU, epi, epi == R, nt, deep, w, 0) for nt, deep, w in wf_decomps(M, N, units * KU, epi, waves)]

    # tile sweep: 5 K units (not a multiple of, or fewer than, every U > 1)
    K = 5 * KU
    for groups in TILE_GROUPS:
        N = groups * 16
        for M in (8, 24, 40, 100):
            for epi in (R, S) if N % 64 == 0 else (R,):
                t.append(Case("tile", M, N, K, epi, epi == R, 0, False, 0, 0))
                for nt, deep, w in wf_decomps(M, N, K, epi, waves=(1, 3, 16)):
                    t += [Case("tile", M, N, K, epi, epi == R, nt, deep, w, tpw) for tpw in TILE_TPW]

    # bounds: a ragged M for every token-tile template, every nt, with and without consecutive tiles
    N, K = 320, 5 * KU
    for M in (7, 23, 39, 55, 100, 121):
        for epi in (R, S, F):
            t.append(Case("bounds", M, N, K, epi, True, 0, False, 0, 0))
            for nt, deep, w in wf_decomps(M, N, K, epi, waves=(2, 5, 16)):
                t += [Case("bounds", M, N, K, epi, True, nt, deep, w, tpw) for tpw in (0, 3)]

    # poisoned padding
    N, K = 192, 9 * KU
    for M in POISON_M:
        for epi in (R, S):
            t.append(Case("poison", M, N, K, epi, False, 0, False, 0, 0))
            t += [Case("poison", M, N, K, epi, False, nt, deep, w, 2) for nt, deep, w in wf_decomps(M, N, K, epi, waves=(4,))]

    # SILU_FRAG + bias: 32 gate / up pairs of row groups, one and several token tiles
    N, K = 1024, 9 * KU
    for M in (8, 24, 40, 100):
        t.append(Case("silu_bias", M, N, K, S, True, 0, False, 0, 0))
        for nt, deep, w in wf_decomps(M, N, K, S, waves=(1, 4)):
            t += [Case("silu_bias", M, N, K, S, True, nt, deep, w, tpw) for tpw in (0, 3)]
    return t


def test_wf_case_table_covers_every_kernel_and_every_edge():
    t = wf_table()
    assert len(set(t)) == len(t), "duplicate cases"
    assert {c.sweep for c in t} == set(WF_SWEEPS)
    explicit = [c for c in t if c.nt]
    assert all(wf_valid(c.M, c.N, c.K, c.epilogue, c.nt, c.deep, c.waves) for c in explicit)
    assert all(c.M <= 128 and c.N % 16 == 0 and c.K % KU == 0 for c in t)
    assert all(c.K <= 2816 and c.N <= NW for c in explicit)             # small shapes: the f64 reference stays cheap
    for (mt, nt, deep), U in WF_KERNELS.items():
        assert U == (4 if mt + nt <= 3 else 2 if mt + nt <= 6 else 1) * (2 if deep else 1)
        mine = [c for c in explicit if (mtr(c.M), c.nt, c.deep) == (mt, nt, deep)]
        units = lambda c: c.K // KU                                     # noqa: E731
        what = f"gemm_wf_kernel MT {mt} NT {nt} deep {deep} U {U}"
        if U > 1:                                                       # with U = 1 there is no remainder
            assert any(units(c) % U and units(c) > U for c in mine), f"{what}: no K with a remainder after full runs"
            assert any(units(c) < U for c in mine), f"{what}: no K below one run"
        assert any(c.waves * U > units(c) for c in mine), f"{what}: no idle wave"
        assert any(c.tpw and ((c.N // 16) // c.nt) % c.tpw for c in mine), f"{what}: no ragged last workgroup"
        assert any(c.tpw > (c.N // 16) // c.nt for c in mine), f"{what}: no tpw beyond the tile count"
        for epi in (R,) + ((S,) if nt > 1 else ()) + (() if deep else (F,)):
            assert any(c.epilogue == epi for c in mine), f"{what}: epilogue {epi} not run"
        if not deep:                                                    # the 16-wave forms, up to the LDS of a workgroup
            assert max(c.waves for c in mine) == min(16, LDS_KIB // (mt * nt)), f"{what}: the widest combine is not run"
    assert {(mtr(c.M), c.nt, c.deep) for c in explicit} == set(WF_KERNELS)
    for sweep in ("m", "bounds"):
        for tiles in range(1, 9):
            ms = {c.M for c in t if c.sweep == sweep and (c.M + 15) // 16 == tiles}
            if sweep == "m":
                assert any(m % 16 == 0 for m in ms), f"no full last tile at {tiles} token tiles"
            if sweep == "m" or tiles in (1, 2, 3, 4, 7, 8):
                assert any(m % 16 for m in ms), f"{sweep}: no ragged last tile at {tiles} token tiles"
    assert {c.M for c in t if c.sweep == "m" and c.N == 192} == set(M_SWEEP)
    assert {c.K // KU for c in t if c.sweep == "k" and c.nt} == set(K_UNITS) and max(K_UNITS) > 16 * 4
    assert {c.N // 16 for c in t if c.sweep == "tile"} == set(TILE_GROUPS) and {c.tpw for c in t if c.sweep == "tile" and c.nt} == set(TILE_TPW)
    assert {c.M for c in t if c.sweep == "poison"} == set(POISON_M)
    assert {c.nt for c in t if c.sweep == "poison"} == {0, 1, 2, 4}     # NT = 1 predicates the padding lanes off, NT > 1 loads them
    assert {mtr(c.M) for c in t if c.sweep == "bounds" and c.M % 16} == {1, 2, 4, 8}
    assert {c.epilogue for c in t if c.sweep == "bounds"} == {R, S, F}
    assert any(c.sweep == "silu_bias" and mtr(c.M) == 1 for c in t) and any(c.sweep == "silu_bias" and mtr(c.M) > 1 for c in t)


class _Wf:
    def __init__(self, dev, sweep):
        self.dev, self.mats, self.ran, self.worst = dev, _Mats(dev), 0, _Worst(f"bf16 wf {sweep}")
        self.cases = [c for c in wf_table() if c.sweep == sweep]
        assert self.cases

    def launch(self, c, y, ldy, xf=None):
        from ssd_amd.hip import ops as H
        cfg = None if not c.nt else (c.nt | (256 if c.deep else 0), c.waves | (c.tpw << 8))
        wf = self.mats.w(c.N, c.K)[0]
        H.gemm(self.mats.x(c.M, c.K)[1] if xf is None else xf, wf, y, c.M, c.N, c.K, ldy, c.epilogue,
               self.mats.bias(c.N) if c.bias else None, cfg)
        self.ran += 1

    def out(self, c, xf=None):
        """The kernel's output as rows: bf16 or fp32 [M, N], or bf16 [M, N / 2] through the SILU fragment."""
        from ssd_amd.hip import ops as H
        if c.epilogue != S:
            y = torch.empty(c.M, c.N, dtype=torch.float32 if c.epilogue == F else BF, device=self.dev)
            self.launch(c, y, c.N, xf)
            return y
        I = c.N // 2
        yf = torch.zeros(H.frag_numel(c.M, I), dtype=BF, device=self.dev)
        self.launch(c, yf, 0, xf)
        y = torch.empty(c.M, I, dtype=BF, device=self.dev)
        H.frag_to_rows(yf, y, c.M, I)
        return y

    def check(self, c, y):
        want = self.mats.ref(c.M, c.N, c.K, c.bias, c.epilogue == S)
        if c.epilogue == R:
            self.worst.add("ROWS", assert_within_ulp(y, want, f"wf {c}"))
        elif c.epilogue == S:
            self.worst.add("SILU_FRAG", assert_silu_within_bar(y, want, c.N // 2, f"wf {c}"))
        else:
            self.worst.add("ROWS_F32", _f32_ratio(y, want, f"wf {c}"))
        self.worst.n += 1

    def done(self, launches_per_case=1):
        assert self.ran == launches_per_case * len(self.cases) and self.worst.n == len(self.cases)
        self.worst.report()


def _wf_run_and_check(dev, sweep):
    h = _Wf(dev, sweep)
    for c in h.cases:
        h.check(c, h.out(c))
    h.done()


@gpu
def test_wf_m_sweep(dev):
    """Every M around the tile boundaries with every valid decomposition: tiles past the last one re-read it (MT = 4 / 8 templates),
    ragged last tiles, combine areas up to 128 KiB."""
    _wf_run_and_check(dev, "m")


@gpu
def test_wf_k_sweep(dev):
    """K remainder loop, K below one run (all work on the last wave), idle waves in the combine."""
    _wf_run_and_check(dev, "k")


@gpu
def test_wf_silu_frag_with_bias_in_packed_order(dev):
    _wf_run_and_check(dev, "silu_bias")


@gpu
def test_wf_tile_sweep_bit_identical_across_tiles_per_workgroup(dev):
    """tpw changes which workgroup owns a tile, never the K order: runs that differ only in tpw are bit-identical."""
    h, first = _Wf(dev, "tile"), {}
    for c in h.cases:
        y = h.out(c)
        h.check(c, y)
        if c.nt:
            base = first.setdefault(c._replace(tpw=0), (c.tpw, y))
            assert torch.equal(_bits(y), _bits(base[1])), f"wf {c}: differs from the tpw = {base[0]} run"
    h.done()


@gpu
def test_wf_bounds_rows_past_m_columns_past_n_and_the_fragment_tail_stay_untouched(dev):
    """ROWS and ROWS_F32 into ceil16(M) + 16 rows of N + 64 columns, SILU_FRAG into its fragment plus a tail, all prefilled with a NaN
    pattern no kernel produces."""
    h = _Wf(dev, "bounds")
    for c in h.cases:
        if c.epilogue == S:
            yb = _guarded_frag(dev, c.M, c.N // 2)
            h.launch(c, yb.view(BF), 0)
            y = _check_guarded_frag(yb, c.M, c.N // 2, f"wf {c}")
        else:
            f32 = c.epilogue == F
            yb, rows, ldy = _guarded_rows(dev, c.M, c.N, f32)
            h.launch(c, yb.view(torch.float32 if f32 else BF), ldy)
            y = _check_guarded_rows(yb, rows, ldy, c.M, c.N, f"wf {c}", f32)
        h.check(c, y)
    h.done()


@gpu
def test_wf_poisoned_x_padding_rows_never_reach_a_real_output(dev):
    """With NT > 1 the kernel loads the padding rows (>= M) of the last x tile (NT = 1 predicates those lanes off), and the engine
    reuses x buffers across different T.  An MFMA output column depends only on the same column of its B operand -- one token row
    here -- so rows < M must not change by one bit."""
    h = _Wf(dev, "poison")
    for c in h.cases:
        clean = h.out(c)
        h.check(c, clean)
        dirty = h.out(c, xf=h.mats.poisoned(c.M, c.K))
        assert torch.equal(_bits(dirty), _bits(clean)), f"wf {c}: padding rows of x changed a row < M"
    h.done(launches_per_case=2)


def _refused(dev, what, call, *buffers):
    """`call` raises and leaves every sentinel buffer as it was."""
    from ssd_amd.hip.lib import SsdHipError
    before = [b.clone() for b in buffers]
    with pytest.raises(SsdHipError):
        call()
    torch.cuda.synchronize()
    for b, b0 in zip(buffers, before):
        assert torch.equal(b, b0), f"{what}: refused, yet something was written"


WF_REFUSED = [
    # M, N, K units, epilogue, nt, deep, waves, ldy - N
    (8, 48, 5, R, 2, False, 4, 0),          # nt does not divide 3 row groups
    (8, 96, 5, R, 4, False, 4, 0),          # ... nor 6
    (8, 80, 5, R, 2, True, 4, 0),           # ... nor 5 (DEEP)
    (8, 192, 5, R, 3, False, 4, 0),         # nt not in {1, 2, 4}
    (8, 192, 5, R, 0, False, 4, 0),         # ... nt = 0 on the plain path (was a division by zero on the host)
    (8, 192, 5, R, 8, False, 4, 0),
    (8, 192, 5, S, 1, False, 4, 0),         # SILU_FRAG needs gate / up pairs
    (8, 96, 5, S, 2, False, 4, 0),          # SILU_FRAG needs N % 64 == 0: N / 2 = 48 is not a fragment width
    (8, 96, 5, S, 2, True, 4, 0),
    (40, 160, 5, S, 2, False, 4, 0),
    (24, 192, 5, R, 2, True, 4, 0),         # DEEP is for one token tile,
    (8, 192, 5, R, 2, True, 9, 0),          # ... at most 8 waves,
    (8, 192, 5, R, 2, True, 0, 0),          # ... at least one,
    (8, 192, 5, R, 1, True, 4, 0),          # ... nt 2 / 4,
    (8, 192, 5, F, 2, True, 4, 0),          # ... bf16 rows or SiLU
    (40, 192, 5, R, 4, False, 4, 0),        # nt = 4 at MT > 2
    (100, 192, 5, S, 4, False, 2, 0),
    (8, 192, 5, R, 1, False, 0, 0),         # waves of 0 and 17
    (8, 192, 5, R, 1, False, 17, 0),
    (0, 192, 5, R, 1, False, 4, 0),         # M of 0 and 129
    (129, 192, 5, R, 1, False, 4, 0),
    (8, 184, 5, R, 1, False, 4, 8),         # ragged N
    (8, 192, 4.5, R, 1, False, 4, 0),       # ragged K
    (8, 192, 5, R, 1, False, 4, -16),       # ldy < N
    (8, 192, 5, F, 2, False, 4, -16),
    (100, 192, 5, R, 2, False, 11, 0),      # combine beyond the 160 KiB of LDS: 176 and 256 KiB
    (100, 192, 5, R, 2, False, 16, 0),
    (100, 192, 5, S, 2, False, 12, 0),
    (8, 192, 5, 3, 1, False, 4, 0),         # the argmax epilogue has its own entry point
    (8, 192, 5, 7, 1, False, 4, 0),
]


@gpu
def test_wf_refusals_return_an_error_and_launch_nothing(dev):
    from ssd_amd.hip import ops as H
    mats = _Mats(dev)
    wf = mats.w(192, 5 * KU)[0]
    yb = torch.full((144 * 256,), SENTINEL, dtype=torch.int16, device=dev)
    for M, N, units, epi, nt, deep, waves, dl in WF_REFUSED:
        K = int(units * KU)
        assert not wf_valid(M, N, K, epi, nt, deep, waves) or dl < 0 or epi not in (R, S, F)
        xf = mats.x(max(1, min(M, 128)), 5 * KU)[1]
        y = yb.view(torch.float32) if epi == F else yb.view(BF)
        cfg = (nt | (256 if deep else 0), waves)
        _refused(dev, f"wf_cfg {(M, N, K, epi, nt, deep, waves, dl)}", lambda: H.gemm(xf, wf, y, M, N, K, N + dl, epi, None, cfg), yb)
    # the default dispatch refuses what no decomposition takes
    for M, N, K, epi, ldy in ((8, 96, 160, S, 0), (40, 160, 160, S, 0), (8, 192, 160, R, 176), (40, 192, 160, R, 176), (40, 192, 160, F, 0),
                              (0, 192, 160, R, 192), (129, 192, 160, R, 192), (8, 184, 160, R, 192), (8, 192, 144, R, 192)):
        xf = mats.x(max(1, min(M, 128)), 5 * KU)[1]
        _refused(dev, f"wf {(M, N, K, epi, ldy)}", lambda: H.gemm(xf, wf, yb.view(BF), M, N, K, ldy, epi), yb)


# =====================================================================================================================
# Family B: ssd_gemm_splitk (gemm_sk_kernel, U = 4, M <= 16)
# =====================================================================================================================
class SkCase(NamedTuple):
    M: int
    N: int
    KT: int          # k-tiles (K / 32)
    splits: int
    waves: int
    bias: bool


SK_U = 4
SK_M = (1, 7, 15, 16)


def slices(KT, splits):
    return [KT * (z + 1) // splits - KT * z // splits for z in range(splits)]


def sk_valid(c) -> bool:
    return 1 <= c.M <= 16 and c.N % 16 == 0 and 1 <= c.splits <= 8 and 1 <= c.waves <= 16 and c.KT >= c.splits


def sk_table() -> list[SkCase]:
    return [SkCase(M, 80, KT, splits, waves, (M + splits) % 2 == 0)
            for KT in (67, 29, 13, 8, 3) for splits in range(1, 9) if KT >= splits for waves in (1, 3, 16) for M in SK_M]


def test_splitk_case_table_covers_uneven_slices_short_slices_and_idle_waves():
    t = sk_table()
    assert len(set(t)) == len(t) and all(sk_valid(c) for c in t) and all(c.KT * 32 <= 2816 and c.N <= NW for c in t)
    for splits in range(2, 9):
        assert any(c.splits == splits and c.KT % splits and len(set(slices(c.KT, splits))) > 1 for c in t), f"no uneven slices at {splits} splits"
    assert any(c.splits == 1 for c in t)
    assert any(c.splits > 1 and max(slices(c.KT, c.splits)) < SK_U for c in t), "no slice shorter than one run"
    assert any(c.splits > 1 and c.KT == c.splits for c in t), "no KT == splits"
    assert any(min(slices(c.KT, c.splits)) // SK_U >= 1 and c.waves > max(slices(c.KT, c.splits)) // SK_U for c in t), "no idle wave"
    assert any(c.waves == 1 and max(slices(c.KT, c.splits)) // SK_U > 1 for c in t), "no wave with several runs"
    assert any(s % SK_U and s > SK_U for c in t for s in slices(c.KT, c.splits)), "no remainder after full runs"
    assert {c.M for c in t} == set(SK_M) and {c.bias for c in t} == {False, True}
    assert (80 // 16) % 2                                            # an odd row-group count


@gpu
def test_splitk_sweep(dev):
    """Sentinel-guarded rows, a NaN workspace (every partial read was written in this launch), counters back at zero after every
    launch, and a second launch on the same counters -- never re-zeroed -- bit-identical to the first."""
    from ssd_amd.hip import ops as H
    mats, worst, t = _Mats(dev), _Worst("bf16 splitk"), sk_table()
    N = t[0].N
    counters = torch.zeros(N // 16, dtype=torch.int32, device=dev)
    ws = torch.empty((N // 16) * 8 * 256, dtype=torch.float32, device=dev)
    for c in t:
        K, what = c.KT * 32, f"splitk {c}"
        wf, xf, bias = mats.w(c.N, K)[0], mats.x(c.M, K)[1], mats.bias(c.N) if c.bias else None
        ys = []
        for _ in range(2):
            ws.fill_(float("nan"))
            yb, rows, ldy = _guarded_rows(dev, c.M, c.N)
            H.gemm_splitk(xf, wf, yb.view(BF), c.M, c.N, K, ldy, c.splits, c.waves, ws, counters, bias=bias)
            ys.append(_check_guarded_rows(yb, rows, ldy, c.M, c.N, what))
            assert not bool(counters.any()), f"{what}: counters not back at zero"
        assert torch.equal(_bits(ys[0]), _bits(ys[1])), f"{what}: the second launch differs"
        worst.add("ROWS", assert_within_ulp(ys[0], mats.ref(c.M, c.N, K, c.bias), what))
        worst.n += 1
    assert worst.n == len(t)
    worst.report()


@gpu
def test_splitk_refusals_return_an_error_and_launch_nothing(dev):
    from ssd_amd.hip import ops as H
    mats = _Mats(dev)
    N, K = 192, 160
    wf, xf = mats.w(N, K)[0], mats.x(8, K)[1]
    yb = torch.full((32 * 256,), SENTINEL, dtype=torch.int16, device=dev)
    ws = torch.full((12 * 8 * 256,), SENTINEL32, dtype=torch.int32, device=dev)
    counters = torch.zeros(12, dtype=torch.int32, device=dev)
    bad = [  # M, N, K, ldy, splits, waves, workspace, counters
        (8, N, K, N, 0, 4, True, True), (8, N, K, N, 9, 4, True, True),           # splits of 0 and 9
        (8, N, 96, N, 4, 4, True, True),                                          # K / 32 < splits
        (8, N, K, N, 2, 4, False, True), (8, N, K, N, 2, 4, True, False),         # missing workspace / counters
        (8, N, K, N, 2, 0, True, True), (8, N, K, N, 2, 17, True, True),          # waves of 0 and 17
        (0, N, K, N, 2, 4, True, True), (17, N, K, N, 2, 4, True, True),          # M of 0 and 17
        (8, N - 8, K, N, 2, 4, True, True), (8, N, K - 16, N, 2, 4, True, True),  # ragged N, K
        (8, N, K, N - 16, 2, 4, True, True), (8, N, K, 0, 1, 4, True, True),      # ldy < N
    ]
    for M, n, k, ldy, splits, waves, w_on, c_on in bad:
        _refused(dev, f"splitk {(M, n, k, ldy, splits, waves, w_on, c_on)}",
                 lambda: H.gemm_splitk(xf, wf, yb.view(BF), M, n, k, ldy, splits, waves, ws.view(torch.float32) if w_on else None,
                                       counters if c_on else None), yb, ws, counters)


# =====================================================================================================================
# Family C: ssd_gemm_parts (gemm_sp_kernel<TPW, MT>, M <= 32)
# =====================================================================================================================
class SpCase(NamedTuple):
    sweep: str       # "slabs" | "rows" | "poison"
    M: int
    N: int
    KT: int
    splits: int
    waves: int
    bias: bool


SP_M = (1, 15, 16, 17, 31, 32)
# (KT, splits, waves): ceil(ceil(KT / splits) / waves) = 1, 2, 3, 4, 5, 8 (every TPW template, 3 and 5 rounded up to 4 and 8 with clamped slots)
SP_SLABS = ((40, 3, 16), (67, 3, 16), (67, 3, 8), (67, 3, 6), (67, 3, 5), (67, 3, 3), (29, 2, 2), (13, 5, 2), (7, 7, 2), (88, 16, 2), (50, 16, 4))
SP_ROWS = ((8, 1, 1), (5, 1, 2), (4, 1, 2), (37, 1, 16), (67, 1, 16), (16, 1, 16), (16, 1, 2), (1, 1, 2))


def sp_tpw(KT, splits, waves) -> int:
    per_wg = -(-KT // splits)
    return -(-per_wg // waves)


def sp_template(KT, splits, waves) -> int:
    t = sp_tpw(KT, splits, waves)
    return 1 if t <= 1 else 2 if t <= 2 else 4 if t <= 4 else 8


def sp_valid(c) -> bool:
    return (1 <= c.M <= 32 and c.N % 16 == 0 and 1 <= c.splits <= 16 and 1 <= c.waves <= 16 and c.KT >= c.splits
            and c.waves >= (c.M + 15) // 16 and sp_tpw(c.KT, c.splits, c.waves) <= 8 and (c.sweep != "rows" or c.splits == 1)
            and (c.sweep == "rows" or not c.bias))


def sp_table() -> list[SpCase]:
    t = [SpCase("slabs", M, 80, *d, False) for d in SP_SLABS for M in SP_M]
    t += [SpCase("rows", M, 80, *d, b) for d in SP_ROWS for M in SP_M if d[2] >= (M + 15) // 16 for b in (False, True)]
    t += [SpCase("poison", M, 80, *d, False) for d in SP_SLABS[1:8] for M in (1, 15, 17, 31)]
    return t


def test_parts_case_table_covers_every_template_and_every_slice_shape():
    t = sp_table()
    assert len(set(t)) == len(t) and all(sp_valid(c) for c in t) and all(c.KT * 32 <= 2816 and c.N <= NW for c in t)
    for sweep in ("slabs", "rows"):
        for mt in (1, 2):
            mine = [c for c in t if c.sweep == sweep and (c.M + 15) // 16 == mt]
            tpws = {sp_tpw(c.KT, c.splits, c.waves) for c in mine}
            assert {sp_template(c.KT, c.splits, c.waves) for c in mine} == {1, 2, 4, 8}, f"{sweep} MT {mt}: a TPW template is not run"
            if sweep == "slabs":
                assert {1, 2, 3, 4, 5, 8} <= tpws, f"MT {mt}: tiles per wave {sorted(tpws)}"
            else:
                assert {3, 5} & tpws and 8 in tpws, f"rows MT {mt}: no rounded-up template, or no full one"
            assert {c.M for c in mine} == {m for m in SP_M if (m + 15) // 16 == mt}
    slabs = [c for c in t if c.sweep == "slabs"]
    assert any(len(set(slices(c.KT, c.splits))) > 1 for c in slabs), "no uneven slices"
    assert any(min(slices(c.KT, c.splits)) < c.waves for c in slabs), "no slice with fewer tiles than waves"
    assert any(c.KT == c.splits for c in slabs) and any(c.splits == 16 for c in slabs)
    assert any(c.M > 16 and c.waves == 2 for c in slabs), "no waves == 2 at two token tiles"
    # a clamped slot: some wave's last slot lies past its slice
    assert all(any(sp_tpw(c.KT, c.splits, c.waves) * c.waves > min(slices(c.KT, c.splits)) for c in slabs if sp_template(c.KT, c.splits, c.waves) == tp)
               for tp in (1, 2, 4, 8))
    assert {c.M for c in t if c.sweep == "poison"} == {1, 15, 17, 31} and {c.bias for c in t if c.sweep == "rows"} == {False, True}


def _parts_launch(dev, mats, c, xf=None):
    """One slab launch into a sentinel buffer with a tail: the slabs fp32 [splits, M, N], every element written, the tail untouched."""
    from ssd_amd.hip import ops as H
    K, n = c.KT * 32, c.splits * c.M * c.N
    pb = torch.full((n + TAIL,), SENTINEL32, dtype=torch.int32, device=dev)
    H.gemm_parts(mats.x(c.M, K)[1] if xf is None else xf, mats.w(c.N, K)[0], c.M, c.N, K, parts=pb.view(torch.float32), splits=c.splits,
                 waves=c.waves)
    assert bool((pb[n:] == SENTINEL32).all()), f"parts {c}: memory past the slabs was written"
    slabs = pb[:n].view(torch.float32).view(c.splits, c.M, c.N)
    assert bool(torch.isfinite(slabs).all()), f"parts {c}: a slab element was left unwritten"
    return slabs


def _check_slabs(mats, worst, slabs, M, N, K, bounds, what):
    """Each slab against the f64 product over its own K range at the fp32 bar; bf16 of the fp32 slab-order sum (what the consumer
    forms) against the full f64 product under the ROWS bar."""
    acc = torch.zeros_like(slabs[0])
    for z, (k0, k1) in enumerate(bounds):
        worst.add("slab", _f32_ratio(slabs[z], mats.ref(M, N, K, k0=k0, k1=k1), f"{what} slab {z}"))
        acc = slabs[z].clone() if z == 0 else acc + slabs[z]
    worst.add("consumer ROWS", assert_within_ulp(acc.to(BF), mats.ref(M, N, K), what))


@gpu
def test_parts_slabs_and_their_consumer_sum(dev):
    mats, worst = _Mats(dev), _Worst("bf16 parts slabs")
    for c in (c for c in sp_table() if c.sweep == "slabs"):
        slabs = _parts_launch(dev, mats, c)
        bounds = [(32 * (c.KT * z // c.splits), 32 * (c.KT * (z + 1) // c.splits)) for z in range(c.splits)]
        _check_slabs(mats, worst, slabs, c.M, c.N, c.KT * 32, bounds, f"parts {c}")
        worst.n += 1
    assert worst.n == len(SP_SLABS) * len(SP_M)
    worst.report()


@gpu
def test_parts_rows_with_bias_sentinel_guarded(dev):
    """parts == None, splits = 1: bf16 rows plus bias."""
    from ssd_amd.hip import ops as H
    mats, worst = _Mats(dev), _Worst("bf16 parts rows")
    for c in (c for c in sp_table() if c.sweep == "rows"):
        K = c.KT * 32
        yb, rows, ldy = _guarded_rows(dev, c.M, c.N)
        H.gemm_parts(mats.x(c.M, K)[1], mats.w(c.N, K)[0], c.M, c.N, K, y=yb.view(BF), ldy=ldy, splits=1, waves=c.waves,
                     bias=mats.bias(c.N) if c.bias else None)
        y = _check_guarded_rows(yb, rows, ldy, c.M, c.N, f"parts {c}")
        worst.add("ROWS", assert_within_ulp(y, mats.ref(c.M, c.N, K, c.bias), f"parts {c}"))
        worst.n += 1
    assert worst.n
    worst.report()


@gpu
def test_parts_poisoned_x_padding_rows_never_reach_a_real_row(dev):
    mats, n = _Mats(dev), 0
    for c in (c for c in sp_table() if c.sweep == "poison"):
        clean = _parts_launch(dev, mats, c)
        dirty = _parts_launch(dev, mats, c, xf=mats.poisoned(c.M, c.KT * 32))
        assert torch.equal(clean.view(torch.int32), dirty.view(torch.int32)), f"parts {c}: padding rows of x changed a row < M"
        n += 1
    print(f"bf16 parts poison: {n} cases, each run twice")


@gpu
def test_parts_refusals_return_an_error_and_launch_nothing(dev):
    from ssd_amd.hip import ops as H
    mats = _Mats(dev)
    N = 192
    wf = mats.w(N, 67 * 32)[0]
    yb = torch.full((48 * 256,), SENTINEL, dtype=torch.int16, device=dev)
    pb = torch.full((16 * 32 * N,), SENTINEL32, dtype=torch.int32, device=dev)
    bad = [  # M, N, KT, ldy, splits, waves, y, parts
        (8, N, 67, N, 1, 8, False, True),                                         # 9 k-tiles per wave: TPW > 8
        (8, N, 67, N, 2, 4, False, True),
        (17, N, 8, N, 1, 1, False, True),                                         # waves < ceil(M / 16)
        (8, N, 3, N, 4, 4, False, True),                                          # KT < splits
        (8, N, 8, N, 1, 4, True, True), (8, N, 8, N, 1, 4, False, False),         # both / neither of y and parts
        (8, N, 8, N, 2, 4, True, False),                                          # splits > 1 without parts
        (8, N, 8, N - 16, 1, 4, True, False), (8, N, 8, 0, 1, 4, True, False),    # ldy < N
        (0, N, 8, N, 1, 4, False, True), (33, N, 8, N, 1, 4, False, True),        # M of 0 and 33
        (8, N, 8, N, 1, 0, False, True), (8, N, 8, N, 1, 17, False, True),        # waves of 0 and 17
        (8, N, 32, N, 0, 4, False, True), (8, N, 32, N, 17, 4, False, True),      # splits of 0 and 17
        (8, N - 8, 8, N, 1, 4, False, True), (8, N, 7.5, N, 1, 4, False, True),   # ragged N, K
    ]
    for M, n, KT, ldy, splits, waves, y_on, p_on in bad:
        K = int(KT * 32)
        xf = mats.x(max(1, min(M, 32)), 67 * 32)[1]
        _refused(dev, f"parts {(M, n, KT, ldy, splits, waves, y_on, p_on)}",
                 lambda: H.gemm_parts(xf, wf, M, n, K, parts=pb.view(torch.float32) if p_on else None, splits=splits, waves=waves,
                                      y=yb.view(BF) if y_on else None, ldy=ldy), yb, pb)


# =====================================================================================================================
# Family D: ssd_gemm_pf_cfg / ssd_gemm_pf at 17 <= M <= 128 (gemm_pf_kernel)
# =====================================================================================================================
# pf_launch_d's instantiation list: (MT, NT) -> (uu, waves, bps, bpre)
PF_INST = {
    (4, 2): ((4, 4, 1, 0), (8, 4, 1, 0), (4, 8, 1, 0), (8, 8, 1, 0)),
    (4, 4): ((4, 4, 1, 0),),
    (8, 1): ((4, 4, 1, 0), (8, 4, 1, 0), (8, 4, 2, 0), (8, 8, 1, 0), (8, 8, 2, 0)),
    (8, 2): ((4, 4, 1, 0), (8, 4, 1, 0), (4, 8, 1, 0), (8, 8, 1, 0), (8, 4, 2, 0), (8, 8, 2, 0), (8, 4, 2, 2), (8, 8, 2, 2), (8, 5, 2, 2),
             (8, 3, 1, 0), (8, 3, 2, 0), (8, 5, 1, 0), (8, 5, 2, 0), (8, 6, 2, 0), (8, 7, 1, 0), (8, 7, 2, 0)),
    (8, 4): ((4, 4, 1, 0),),
}
PF_M = (17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 81, 96, 97, 111, 112, 113, 127, 128)
# (K, splits) -> nk = K / 32 / splits k-steps per split: 4 (one pass, every look-ahead load clamped to the last k-step), 8 (one pass for
# uu = 8), 12 (uu = 4 only), 16, 24
PF_KS = ((128, 1), (512, 4), (256, 1), (512, 2), (384, 1), (1152, 3), (512, 1), (1024, 2), (768, 1), (2304, 3))
PF_BASE = (2, 4, 4, 1, 0)          # the plain 4-wave form: nt, waves, uu, bps, bpre
PF_BASE_N = 768                    # a multiple of every 16 x nt x waves below: each launch shape is compared on a prefix of its columns
P = PF_EPI_PARTIALS


class PfCase(NamedTuple):
    sweep: str       # "m" | "k" | "poison"
    M: int
    N: int
    K: int
    epilogue: int
    bias: bool
    nt: int          # 0: the default dispatch (ssd_gemm_pf; waves .. bpre unused, splits 0 = its own pick)
    waves: int
    uu: int          # 0: the kernel's default for nk
    bps: int
    bpre: int
    splits: int


def pmt(M: int) -> int:
    return 4 if M <= 64 else 8


def pf_uu(c) -> int:
    nk = c.K // 32 // c.splits
    return c.uu or (8 if c.nt <= 2 and nk % 8 == 0 else 4)


def pf_valid(c) -> bool:
    """The rules of ssd_gemm_pf_cfg and pf_launch_d."""
    if not 17 <= c.M <= 128 or c.K <= 0 or c.K % 128 or c.nt not in (1, 2, 4):
        return False
    if c.nt == 1 and (c.epilogue == S or c.M <= 64):
        return False
    if c.waves != 4 and not (3 <= c.waves <= 8 and c.nt <= 2):
        return False
    if c.N <= 0 or c.N % (16 * c.nt * c.waves) or (c.epilogue == S and c.N % 64) or (c.epilogue == P and c.bias):
        return False
    if not 1 <= c.splits <= 16 or (c.K // 32) % (4 * c.splits):
        return False
    return (c.K // 32 // c.splits) % pf_uu(c) == 0 and (pf_uu(c), c.waves, c.bps, c.bpre) in PF_INST[(pmt(c.M), c.nt)]


def pf_widths(nt, waves, epilogue):
    """One workgroup's worth of columns and three; two where SILU_FRAG needs N % 64 == 0 (nt = 2 with 3, 5, 7 waves)."""
    wg = 16 * nt * waves
    return [2 * wg] if epilogue == S and wg % 64 else [wg, 3 * wg]


def pf_table() -> list[PfCase]:
    t: list[PfCase] = []
    # M sweep and launch-shape identity: every instantiation at every M, unsplit (in-kernel epilogue) and split (epilogue kernel)
    K = 768
    for M in PF_M:
        t.append(PfCase("m", M, PF_BASE_N, K, R, True, 0, 0, 0, 0, 0, 0))
        for splits in (1, 3):
            for nt in (2, 1, 4):                                         # the plain form first: the others are compared with it
                for uu, waves, bps, bpre in PF_INST.get((pmt(M), nt), ()):
                    t.append(PfCase("m", M, PF_BASE_N if (nt, waves, uu, bps, bpre) == PF_BASE else 3 * 16 * nt * waves, K, R, True,
                                    nt, waves, uu, bps, bpre, splits))
    # K sweep: every instantiation whose uu divides nk, three epilogues, two widths
    for K, splits in PF_KS:
        nk = K // 32 // splits
        for M in (31, 49, 72, 127):
            for nt in (1, 2, 4):
                insts = [i for i in PF_INST.get((pmt(M), nt), ()) if nk % i[0] == 0] + ([(0, 4, 1, 0)] if nt > 1 else [])
                for uu, waves, bps, bpre in insts:
                    for epi in (R, S, P) if nt > 1 else (R, P):
                        t += [PfCase("k", M, N, K, epi, epi != P, nt, waves, uu, bps, bpre, splits) for N in pf_widths(nt, waves, epi)]
    # poisoned padding rows of the last x tile: one width, rows and slabs, unsplit and split
    for K, splits in ((512, 1), (512, 2)):
        for M in (17, 47, 72, 100):
            for nt in (1, 2, 4):
                for uu, waves, bps, bpre in PF_INST.get((pmt(M), nt), ()):
                    t += [PfCase("poison", M, 16 * nt * waves, K, epi, False, nt, waves, uu, bps, bpre, splits) for epi in (R, P)]
    # the default dispatch at real grids: 8B qkv and gate_up at 3, 5, 7, 8 token tiles
    for N, K, forms in ((6144, 4096, ((R, True),)), (28672, 4096, ((S, False), (R, False)))):
        for M in (40, 72, 100, 120):
            t += [PfCase("k", M, N, K, epi, bias, 0, 0, 0, 0, 0, 0) for epi, bias in forms]
    return t


def test_pf_case_table_covers_every_instantiation_at_a_ragged_m():
    t = pf_table()
    assert len(set(t)) == len(t), "duplicate cases"
    explicit = [c for c in t if c.nt]
    assert all(pf_valid(c) for c in explicit), [c for c in explicit if not pf_valid(c)][:3]
    assert all(c.K <= 2816 and c.N <= NW for c in explicit)
    for (mt, nt), insts in PF_INST.items():
        for inst in insts:
            mine = [c for c in explicit if (pmt(c.M), c.nt) == (mt, nt) and (pf_uu(c), c.waves, c.bps, c.bpre) == inst]
            what = f"gemm_pf_kernel MT {mt} NT {nt} (uu, waves, bps, bpre) {inst}"
            assert any(c.M % 16 for c in mine), f"{what}: no ragged M"
            if mt == 8:
                assert any(65 <= c.M <= 79 for c in mine), f"{what}: no M in 65..79 (x tiles past the last one are clamped re-reads)"
            nks = {c.K // 32 // c.splits for c in mine}
            assert inst[0] in nks, f"{what}: no single pass (nk == uu)"
            assert {16, 24} <= nks and (inst[0] == 8 or {4, 12} <= nks), f"{what}: nk {sorted(nks)}"
            for epi in (R, P) + ((S,) if nt > 1 else ()):
                for split in (False, True):
                    assert any(c.epilogue == epi and (c.splits > 1) == split for c in mine), f"{what}: epilogue {epi} split {split} not run"
            assert any(c.sweep == "poison" and c.M % 16 for c in mine), f"{what}: no poisoned padding"
            assert {c.M for c in mine if c.sweep == "m"} == {m for m in PF_M if pmt(m) == mt}, f"{what}: M list"
            assert {1, 3} <= {c.N // (16 * nt * c.waves) for c in mine}, f"{what}: one workgroup's worth of columns and three"
    assert {(c.K, c.splits) for c in explicit if c.sweep == "k"} == set(PF_KS)
    assert {K // 32 // s for K, s in PF_KS} == {4, 8, 12, 16, 24}
    assert all(c.N <= PF_BASE_N for c in explicit if c.sweep == "m")    # each launch shape is compared on a prefix of the base's columns
    assert PF_INST[(4, 2)][0] == PF_INST[(8, 2)][0] == (PF_BASE[2], PF_BASE[1], PF_BASE[3], PF_BASE[4])      # ... which comes first
    assert any(not c.nt and c.N > NW for c in t) and any(not c.nt and c.N == PF_BASE_N for c in t)


class _Pf:
    def __init__(self, dev, sweep):
        self.dev, self.mats, self.worst = dev, _Mats(dev), _Worst(f"bf16 pf {sweep}")
        self.cases = [c for c in pf_table() if c.sweep == sweep]
        assert self.cases

    def splits(self, c):
        from ssd_amd.hip import ops as H
        return c.splits or H.gemm_pf_workspace_bytes(c.M, c.N, c.K) // (4 * c.M * c.N)

    def run(self, c, xf=None):
        """One launch, everything guarded: y in a sentinel frame, the workspace prefilled with a NaN pattern and followed by a
        sentinel tail.  Returns bf16 rows [M, N], bf16 [M, N / 2] through the SILU fragment, or the fp32 slabs [splits, M, N]."""
        from ssd_amd.hip import ops as H
        what = f"pf {c}"
        n = self.splits(c) * c.M * c.N
        ws = torch.full((n + TAIL,), SENTINEL32, dtype=torch.int32, device=self.dev)
        nt = c.nt | c.waves << 8 | c.uu << 16 | c.bps << 24 | c.bpre << 28 if c.nt else 0
        xf = self.mats.x(c.M, c.K)[1] if xf is None else xf
        wf, bias = self.mats.w(c.N, c.K)[0], self.mats.bias(c.N) if c.bias else None
        if c.epilogue == R:
            yb, rows, ldy = _guarded_rows(self.dev, c.M, c.N)
        elif c.epilogue == S:
            yb, ldy = _guarded_frag(self.dev, c.M, c.N // 2), 0
        else:
            yb, ldy = torch.full((TAIL,), SENTINEL, dtype=torch.int16, device=self.dev), c.N
        H.gemm_pf(xf, wf, yb.view(BF), c.M, c.N, c.K, ldy, ws.view(torch.float32), epilogue=c.epilogue, bias=bias, splits=c.splits, nt=nt)
        assert bool((ws[n:] == SENTINEL32).all()), f"{what}: memory past the workspace's splits * M * N floats was written"
        if c.epilogue == R:
            return _check_guarded_rows(yb, rows, ldy, c.M, c.N, what)
        if c.epilogue == S:
            return _check_guarded_frag(yb, c.M, c.N // 2, what)
        assert bool((yb == SENTINEL).all()), f"{what}: PARTIALS wrote y"
        slabs = ws[:n].view(torch.float32).view(-1, c.M, c.N)
        assert bool(torch.isfinite(slabs).all()), f"{what}: a slab element was left unwritten"
        return slabs

    def check(self, c, out):
        what = f"pf {c}"
        if c.epilogue == R:
            self.worst.add("ROWS", assert_within_ulp(out, self.mats.ref(c.M, c.N, c.K, c.bias), what))
        elif c.epilogue == S:
            self.worst.add("SILU_FRAG", assert_silu_within_bar(out, self.mats.ref(c.M, c.N, c.K, c.bias, True), c.N // 2, what))
        else:
            s = out.shape[0]
            _check_slabs(self.mats, self.worst, out, c.M, c.N, c.K, [(c.K // s * z, c.K // s * (z + 1)) for z in range(s)], what)
        self.worst.n += 1

    def done(self):
        assert self.worst.n == len(self.cases)
        self.worst.report()


@gpu
def test_pf_m_sweep_every_launch_shape_bit_identical_to_the_plain_four_wave_form(dev):
    """At fixed splits every accumulator walks its split's k-steps in one sequential order, whatever the launch shape (nt, waves,
    uu 4 or 8, k-steps per barrier, B operands read up front): each shape equals the plain 4-wave form bit for bit on its columns,
    at every M of the list, through the in-kernel epilogue (unsplit) and the epilogue kernel (split)."""
    h, base, identical = _Pf(dev, "m"), {}, 0
    for c in h.cases:
        y = h.run(c)
        h.check(c, y)
        if (c.nt, c.waves, c.uu, c.bps, c.bpre) == PF_BASE:
            base[(c.M, c.splits)] = y
        elif c.nt:
            assert torch.equal(_bits(y), _bits(base[(c.M, c.splits)][:, :c.N])), f"pf {c}: differs from the plain 4-wave form"
            identical += 1
    h.done()
    assert identical == len(h.cases) - 3 * len(PF_M)
    print(f"bf16 pf m: {identical} launch shapes bit-identical to the plain 4-wave form")


@gpu
def test_pf_k_sweep_three_epilogues_split_and_unsplit(dev):
    """nk = 4 (a single pass, every look-ahead load clamped to the last k-step), 8, 12, 16, 24; ROWS and SILU_FRAG unsplit in the
    kernel and split through the epilogue kernel, PARTIALS as slabs; one workgroup's worth of columns and several; the default
    dispatch at the 8B grids."""
    h = _Pf(dev, "k")
    for c in h.cases:
        h.check(c, h.run(c))
    h.done()


@gpu
def test_pf_poisoned_x_padding_rows_never_reach_a_real_row(dev):
    """Rows [M, ceil16(M)) of the x fragment are staged in LDS and multiplied by this kernel: rows < M must not change by one bit."""
    h = _Pf(dev, "poison")
    for c in h.cases:
        clean = h.run(c)
        h.check(c, clean)
        dirty = h.run(c, xf=h.mats.poisoned(c.M, c.K))
        same = torch.equal(clean.view(torch.int32), dirty.view(torch.int32)) if c.epilogue == P else torch.equal(_bits(clean), _bits(dirty))
        assert same, f"pf {c}: padding rows of x changed a row < M"
    h.done()


@gpu
def test_pf_refusals_return_an_error_and_launch_nothing(dev):
    from ssd_amd.hip import ops as H
    mats = _Mats(dev)
    K = 768
    wf, b = mats.w(768, K)[0], mats.bias(768)
    yb = torch.full((144 * 1024,), SENTINEL, dtype=torch.int16, device=dev)
    ws = torch.full((4 * 128 * 768,), SENTINEL32, dtype=torch.int32, device=dev)

    def shape(nt, waves=0, uu=0, bps=0, bpre=0):
        return nt | waves << 8 | uu << 16 | bps << 24 | bpre << 28

    bad = [  # M, N, K, ldy, epilogue, bias, nt word, splits, workspace floats (None: all)
        (40, 768, K, 768, R, False, shape(1), 1, None),                 # nt = 1 at M <= 64
        (100, 768, K, 0, S, False, shape(1), 1, None),                  # ... or with SILU_FRAG
        (100, 448, K, 448, R, False, shape(4, 7), 1, None),             # 7 waves with nt = 4
        (100, 768, K, 768, R, False, shape(2, 5), 1, None),             # N no multiple of 16 x nt x waves
        (100, 768, K, 768, R, False, shape(2, 2), 1, None),             # waves of 2 and 9
        (100, 576, K, 576, R, False, shape(2, 9), 1, None),
        (100, 768, K, 768, R, False, shape(3), 1, None),                # nt of 3, 0 (with a launch shape) and 8
        (100, 768, K, 768, R, False, shape(0, 4), 1, None),
        (100, 768, K, 768, R, False, shape(8), 1, None),
        (100, 768, 384, 768, R, False, shape(2), 2, None),              # KT = 12 no multiple of 4 x splits
        (100, 768, K, 768, R, False, shape(2), 17, None),               # splits beyond 16 (and KT % (4 x 17))
        (100, 768, K, 768, R, False, shape(2), 2, 2 * 100 * 768 - 4),   # a workspace too small
        (100, 768, K, 768, P, False, shape(2), 1, 100 * 768 - 4),
        (100, 768, K, 768, R, False, shape(2), 3, 0),                   # ... or missing
        (100, 768, K, 768, P, True, shape(2), 2, None),                 # PARTIALS with a bias
        (100, 768, K, 768, 3, False, shape(2), 1, None),                # no such epilogue
        (16, 768, K, 768, R, False, shape(2), 1, None),                 # M of 16 (and below) belongs to ssd_gemm_wf
        (0, 768, K, 768, R, False, shape(2), 1, None),
        (100, 768, K - 64, 768, R, False, shape(2), 1, None),           # K % 128
        (100, 760, K, 768, R, False, shape(2), 1, None),                # ragged N
        (100, 96, K, 0, S, False, shape(2, 3), 1, None),                # SILU_FRAG needs N % 64 == 0: N / 2 = 48, 80, 112
        (100, 160, K, 0, S, False, shape(2, 5), 3, None),
        (100, 224, K, 0, S, False, shape(2, 7, 8, 2), 1, None),
        (100, 768, K, 752, R, False, shape(2), 1, None),                # ldy < N, unsplit and split
        (100, 768, K, 0, R, False, shape(2), 3, None),
        (100, 768, K, 768, R, False, shape(2, 6, 8, 1), 1, None),       # launch shapes that are not instantiated: 6 waves x 1 k-step,
        (100, 768, 384, 768, R, False, shape(2, 4, 8, 1), 1, None),     # ... uu = 8 at nk = 12,
        (40, 768, K, 768, R, False, shape(2, 4, 8, 2), 1, None),        # ... two k-steps per barrier at M <= 64,
        (100, 768, K, 768, R, False, shape(4, 4, 8, 1), 1, None),       # ... uu = 8 with nt = 4,
        (100, 768, K, 768, R, False, shape(2, 4, 4, 2), 1, None),       # ... two k-steps per barrier with uu = 4
        (100, 768, K, 768, R, False, shape(1, 4, 8, 2, 2), 1, None),    # ... B operands up front with nt = 1
    ]
    for M, N, k, ldy, epi, bias, nt, splits, wsn in bad:
        xf = mats.x(max(17, M), K)[1]
        w = ws.view(torch.float32)[:ws.numel() if wsn is None else wsn] if wsn != 0 else torch.empty(0, dtype=torch.float32, device=dev)
        _refused(dev, f"pf_cfg {(M, N, k, ldy, epi, bias, hex(nt), splits, wsn)}",
                 lambda: H.gemm_pf(xf, wf, yb.view(BF), M, N, k, ldy, w, epilogue=epi, bias=b[:N] if bias else None, splits=splits, nt=nt),
                 yb, ws)
    # the default dispatch: N % 128, a K split that does not divide, ldy < N
    for M, N, k, ldy, splits in ((100, 704, K, 704, 0), (100, 768, K, 768, 5), (100, 768, K, 752, 0), (100, 768, K - 64, 768, 0)):
        xf = mats.x(M, K)[1]
        _refused(dev, f"pf {(M, N, k, ldy, splits)}", lambda: H.gemm_pf(xf, wf, yb.view(BF), M, N, k, ldy, ws.view(torch.float32), splits=splits),
                 yb, ws)


# =====================================================================================================================
# Refusals that return before any HIP call: no GPU needed
# =====================================================================================================================
def test_bad_configurations_are_refused_on_the_host_without_a_gpu():
    """Through ctypes with null operands: whatever is wrong with a configuration is answered before any HIP call, and a valid
    configuration with null operands is an argument error, not a launch.  nt = 0 used to divide by zero on the host."""
    import ctypes
    from ssd_amd.hip.lib import load_library
    lib = load_library()
    z = ctypes.c_void_p(0)
    SHAPE, ARG = -1, -3

    def wf_cfg(M, N, K, ldy, epi, nt, waves):
        return lib.ssd_gemm_wf_cfg(z, z, z, z, M, N, K, ldy, epi, nt, waves, z)

    for nt in (0, 3, 5, 8, 255, 256, 256 | 3, 256 | 8):                 # nt = 0 with and without the DEEP bit
        for epi in (R, S, F):
            assert wf_cfg(8, 192, 160, 192, epi, nt, 4) == ARG, (nt, epi)
    assert wf_cfg(8, 96, 160, 0, S, 2, 4) == SHAPE and wf_cfg(8, 96, 160, 0, S, 2 | 256, 4) == SHAPE       # SILU_FRAG, N % 64
    assert wf_cfg(8, 192, 160, 176, R, 1, 4) == SHAPE and wf_cfg(8, 192, 160, 0, F, 1, 4) == SHAPE         # ldy < N
    assert wf_cfg(8, 192, 160, 176, R, 2 | 256, 4) == SHAPE
    assert wf_cfg(8, 192, 160, 0, S, 2, 4) == ARG                       # valid, SILU_FRAG ignores ldy: null operands
    for waves in (0, 9, 17):
        assert wf_cfg(8, 192, 160, 192, R, 2 | 256, waves) == ARG       # DEEP: 1..8 waves
    for waves in (0, 17, 255):
        assert wf_cfg(8, 192, 160, 192, R, 1, waves) == ARG
    assert wf_cfg(24, 192, 160, 192, R, 2 | 256, 4) == ARG and wf_cfg(8, 192, 160, 192, R, 1 | 256, 4) == ARG
    assert wf_cfg(8, 48, 160, 48, R, 2, 4) == ARG and wf_cfg(8, 192, 160, 0, S, 1, 4) == ARG
    for M, N, K in ((0, 192, 160), (129, 192, 160), (8, 184, 160), (8, 192, 144), (8, 0, 160), (8, 192, 0), (-1, 192, 160)):
        assert wf_cfg(M, N, K, 192, R, 1, 4) == SHAPE, (M, N, K)
        assert lib.ssd_gemm_wf(z, z, z, z, M, N, K, 192, R, z) < 0, (M, N, K)
    assert wf_cfg(100, 192, 160, 192, R, 2, 4) == ARG                   # valid: null operands
    for M, N, ldy, epi in ((8, 96, 0, S), (40, 160, 0, S), (8, 192, 176, R), (40, 192, 176, R), (100, 192, 0, F)):
        assert lib.ssd_gemm_wf(z, z, z, z, M, N, 160, ldy, epi, z) == SHAPE, (M, N, ldy, epi)

    def splitk(M, N, K, ldy, splits, waves):
        return lib.ssd_gemm_splitk(z, z, z, z, M, N, K, ldy, splits, waves, z, z, z)

    assert splitk(8, 192, 160, 176, 1, 4) == SHAPE and splitk(8, 192, 160, 0, 1, 4) == SHAPE
    for M, N, K in ((0, 192, 160), (17, 192, 160), (8, 184, 160), (8, 192, 144)):
        assert splitk(M, N, K, 192, 1, 4) == SHAPE
    for splits, waves, K in ((0, 4, 160), (9, 4, 512), (2, 0, 160), (2, 17, 160), (2, 4, 160), (4, 4, 96), (1, 4, 160)):
        assert splitk(8, 192, K, 192, splits, waves) == ARG, (splits, waves, K)

    def parts(M, N, K, ldy, splits, waves, y, p):
        return lib.ssd_gemm_parts(z, z, z, ctypes.c_void_p(y), ctypes.c_void_p(p), M, N, K, ldy, splits, waves, z)

    # (non-null y / parts here are never dereferenced: every one of these is refused, the last as null x / w operands)
    assert parts(8, 192, 256, 192, 1, 4, 0, 0) == ARG and parts(8, 192, 256, 192, 1, 4, 16, 16) == ARG and parts(8, 192, 256, 192, 2, 4, 16, 0) == ARG
    assert parts(8, 192, 256, 176, 1, 4, 16, 0) == SHAPE and parts(8, 192, 256, 0, 1, 4, 16, 0) == SHAPE
    assert parts(8, 192, 67 * 32, 192, 1, 8, 0, 16) == ARG and parts(17, 192, 256, 192, 1, 1, 0, 16) == ARG and parts(8, 192, 96, 192, 4, 4, 0, 16) == ARG
    for M, N, K in ((0, 192, 256), (33, 192, 256), (8, 184, 256), (8, 192, 240)):
        assert parts(M, N, K, 192, 1, 4, 0, 16) == SHAPE
    for splits, waves in ((0, 4), (17, 4), (1, 0), (1, 17)):
        assert parts(8, 192, 1024, 192, splits, waves, 0, 16) == ARG
    assert parts(8, 192, 256, 0, 2, 4, 0, 16) == ARG                    # valid: null x / w

    def pf_cfg(M, N, K, ldy, epi, nt, splits, wbytes=1 << 40, bias=0, ws=16):
        return lib.ssd_gemm_pf_cfg(z, z, ctypes.c_void_p(bias), z, M, N, K, ldy, epi, ctypes.c_void_p(ws), ctypes.c_int64(wbytes), nt, splits, z)

    for nt in (0 | 4 << 8, 3, 8, 255):
        assert pf_cfg(100, 768, 768, 768, R, nt, 1) == ARG, nt
    assert pf_cfg(40, 768, 768, 768, R, 1, 1) == ARG and pf_cfg(100, 768, 768, 0, S, 1, 1) == ARG
    assert pf_cfg(100, 448, 768, 448, R, 4 | 7 << 8, 1) == ARG and pf_cfg(100, 768, 768, 768, R, 2 | 2 << 8, 1) == ARG
    assert pf_cfg(100, 768, 768, 768, R, 2 | 5 << 8, 1) == SHAPE and pf_cfg(100, 760, 768, 768, R, 2, 1) == SHAPE
    assert pf_cfg(100, 768, 384, 768, R, 2, 2) == ARG and pf_cfg(100, 768, 768, 768, R, 2, 17) == ARG
    assert pf_cfg(100, 768, 768, 768, R, 2, 2, wbytes=2 * 100 * 768 * 4 - 1) == ARG and pf_cfg(100, 768, 768, 768, R, 2, 2, ws=0) == ARG
    assert pf_cfg(100, 768, 768, 768, P, 2, 2, bias=16) == ARG and pf_cfg(100, 768, 768, 768, 3, 2, 1) == ARG
    assert pf_cfg(16, 768, 768, 768, R, 2, 1) == SHAPE and pf_cfg(100, 768, 704, 768, R, 2, 1) == SHAPE
    assert pf_cfg(100, 96, 768, 0, S, 2 | 3 << 8, 1) == SHAPE and pf_cfg(100, 160, 768, 0, S, 2 | 5 << 8, 3) == SHAPE
    assert pf_cfg(100, 768, 768, 752, R, 2, 1) == SHAPE and pf_cfg(100, 768, 768, 0, R, 2, 3) == SHAPE
    assert pf_cfg(100, 768, 768, 768, R, 2, 1) == ARG and pf_cfg(100, 768, 768, 0, P, 2, 3) == ARG      # valid: null operands
