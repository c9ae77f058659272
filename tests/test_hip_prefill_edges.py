"""Family E of the bf16 edge harness (tests/test_hip_bf16_edges.py): the long-prefill GEMM, ssd_gemm_pf_cfg / ssd_gemm_pf at
128 < M <= 16384 (csrc/gemm_pf.hip gemm_lm_kernel<BM, BN, WM, WN, DIRECT> and gemm_pf_epilogue_kernel behind its K split), at the
edges tests/test_hip_prefill_long.py does not visit with its workload-sized shapes:

  * every tile form at every M around the 16-row group and the 128 / 256-row tile borders (clamped x row groups, a ragged last tile);
  * a ragged N tile: the 256-wide forms 1 and 2 at N % 256 == 128 (clamped W row groups, the `>= ng_valid` skips of the three
    epilogues), alone and together with a ragged M tile;
  * K slices of 1, 2, 3 stages and even / odd counts beyond (one `issue`, no restage; the last stage in buffer 0 or 1), splits of
    1, 2, 3, 4 and 16;
  * workgroup counts 1..7 and every residue mod 8 from 8 on: the XCD remap is a bijection only if every output is written;
  * ROWS and SILU_FRAG, with and without a bias, in the kernel (unsplit) and through the epilogue kernel (split), on every form;
  * the default dispatch on every shape of the table, and M at the ceiling of 16384;
  * NaN / Inf in the x fragment's padding rows, which row groups past ceil(M / 16) are clamped onto;
  * guards as wide as a tile: 256 sentinel rows past M and 256 sentinel columns past N (an unguarded store of a 256-wide tile at
    N = 128 lands in a guard, not in the next row's real columns), exact workspaces with a sentinel tail, NaN-prefilled;
  * one launch against the engine's loop of <= 128-row chunks, hipGraph replay, the dequantize-then-GEMM route of the four
    weight-only formats, and the refusals (an error, nothing written), `ldy < N` among them.

Reference and bars are the harness's own: float64 x @ W.T (+ bias) on the bf16 operand values; ROWS within 1 bf16 ulp of bf16(f64)
with the ulp floored at 2^-6 of the output rms (assert_within_ulp), SILU_FRAG under assert_silu_within_bar; operands as in family D.
The case table is plain Python: the unmarked tests check what it covers and hold the Python restatement of lm_gemm's rules to the
library's return codes, the GPU tests run it and count."""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import pytest
import torch

from ssd_amd.hip.ops import EPI_ROWS, EPI_SILU_FRAG
from tests.test_hip_bf16_edges import SENTINEL, SENTINEL32, TAIL, _check_guarded_frag, _check_guarded_rows, _guarded_frag, _Mats
from tests.test_hip_bf16_edges import _refused, _Worst, ceil16
from tests.test_hip_mxfp4 import assert_silu_within_bar, assert_within_ulp, dev  # noqa: F401  (dev is the fixture)
from tests.test_hip_quant_edges import _bits

gpu = pytest.mark.gpu
BF = torch.bfloat16
R, S = EPI_ROWS, EPI_SILU_FRAG
SHAPE, ARG = -1, -3                # SSD_ERR_SHAPE, SSD_ERR_ARG
GUARD = 256                        # guard rows past M and guard columns past N: a whole tile of the widest form each way
LM_BM = {1: 256, 2: 128, 3: 256, 4: 128}
LM_BN = {1: 256, 2: 256, 3: 128, 4: 128}
FORMS = (1, 2, 3, 4)
LM_M = (129, 143, 144, 145, 255, 256, 257, 271, 272, 273, 383, 384, 385, 511, 512, 513)
# (K, splits) -> nkb = K / 64 / splits stages per slice: 2, 1, 6, 3, 2, 10, 5, 16, 4, 1
LM_KS = ((128, 1), (128, 2), (384, 1), (384, 2), (384, 3), (640, 1), (640, 2), (1024, 1), (1024, 4), (1024, 16))
LM_POISON_M = (129, 257, 385, 513)
LM_SWEEPS = ("m", "n", "k", "wg", "epi", "poison", "ceiling")
CEILING = (16384, 128, 128)


class LmCase(NamedTuple):
    sweep: str
    M: int
    N: int
    K: int
    epilogue: int
    bias: bool
    form: int        # 0: the default dispatch (ssd_gemm_pf, splits 0 = its own pick)
    splits: int


class LmGeom(NamedTuple):
    BM: int
    BN: int
    tiles_m: int
    tiles_n: int
    nwg: int
    nkb: int
    ragged_m: bool
    ragged_n: bool


def lm_geom(form, M, N, K, splits) -> LmGeom:
    """lm_go's launch geometry: tiles of BM x rows by BN W rows, one workgroup per tile and K slice, nkb 64-deep stages per slice."""
    BM, BN = LM_BM[form], LM_BN[form]
    tiles_m, tiles_n = -(-M // BM), -(-N // BN)
    return LmGeom(BM, BN, tiles_m, tiles_n, tiles_m * tiles_n * splits, K // 64 // splits, M % BM != 0, N % BN != 0)


def lm_valid(form, M, N, K, splits) -> bool:
    """What lm_gemm takes with an explicit form and split."""
    return (128 < M <= 16384 and N > 0 and N % 128 == 0 and K > 0 and K % 128 == 0 and form in FORMS and 1 <= splits <= 16
            and (K // 64) % splits == 0)


def lm_rc(M, N, K, form, splits, epilogue=R, ldy=None) -> int:
    """lm_gemm's checks ahead of the operands, in its order: the code of the first broken rule, 0 where none is broken (null operands
    or a short workspace are then an argument error).  form 0 / splits <= 0 stand for the default pick, which always divides K / 64."""
    ldy = N if ldy is None else ldy
    if not 128 < M <= 16384 or N <= 0 or K <= 0 or N % 128 or K % 128:
        return SHAPE
    if epilogue not in (R, S):
        return ARG
    if epilogue == R and ldy < N:
        return SHAPE
    if not 0 <= form <= 4:
        return ARG
    if splits > 16 or (splits >= 1 and (K // 64) % splits):
        return ARG
    return 0


def lm_table() -> list[LmCase]:
    t: list[LmCase] = []
    # M sweep: every form at every M of the list, at an N that is ragged for the 256-wide forms
    for M in LM_M:
        t += [LmCase("m", M, 384, 256, R, True, form, 1) for form in FORMS]
    # N sweep: N % 256 == 128 and whole, with a ragged M tile (300) and a whole one (256), both epilogues, direct and split
    for N in (128, 256, 384, 512, 640):
        for form in FORMS:
            t += [LmCase("n", 300, N, 256, epi, True, form, splits) for splits in (1, 2) for epi in (R, S)]
            t.append(LmCase("n", 256, N, 256, R, True, form, 1))
    # stage counts
    for K, splits in LM_KS:
        t += [LmCase("k", 300, 384, K, epi, True, form, splits) for form in FORMS for epi in (R, S)]
    # workgroup counts: form 4 at 2 and 3 M tiles, form 3 at one M tile, one workgroup, and splits on top
    t += [LmCase("wg", 200, N, 256, R, False, 4, 1) for N in range(128, 1025, 128)]             # 2, 4, .. 16
    t += [LmCase("wg", 300, N, 256, R, False, 4, 1) for N in range(128, 641, 128)]              # 3, 6, 9, 12, 15
    t += [LmCase("wg", 200, N, 256, R, False, 3, 1) for N in (128, 640, 896, 1408, 1664)]       # 1, 5, 7, 11, 13
    t += [LmCase("wg", 200, 256, 256, R, False, 1, 1), LmCase("wg", 300, 384, 384, R, False, 4, 3),                  # 1, 27
          LmCase("wg", 200, 640, 256, R, False, 3, 2), LmCase("wg", 300, 384, 256, R, False, 2, 4)]                  # 10, 24
    # epilogues: with and without a bias, direct and split, every form, at a ragged M tile and N % 256 == 128
    t += [LmCase("epi", 273, 384, 256, epi, bias, form, splits)
          for form in FORMS for epi in (R, S) for bias in (False, True) for splits in (1, 2)]
    # poisoned padding rows of x
    t += [LmCase("poison", M, 384, 256, epi, False, form, splits)
          for M in LM_POISON_M for form in FORMS for splits in (1, 2) for epi in (R, S)]
    # the ceiling
    t.append(LmCase("ceiling", *CEILING, R, True, 1, 1))
    # the default dispatch on every shape above
    seen: dict = {}
    for c in t:
        seen.setdefault((c.M, c.N, c.K), c.sweep)
    t += [LmCase(sweep, M, N, K, R, True, 0, 0) for (M, N, K), sweep in seen.items()]
    return t


def lm_shapes() -> list[tuple[int, int, int]]:
    """Every (M, N, K) of the table, one weight matrix after the other."""
    return sorted({(c.M, c.N, c.K) for c in lm_table()}, key=lambda s: (s[1], s[2], s[0]))


def test_lm_case_table_covers_every_form_at_every_edge():
    t = lm_table()
    assert len(set(t)) == len(t), "duplicate cases"
    assert {c.sweep for c in t} == set(LM_SWEEPS)
    explicit = [c for c in t if c.form]
    assert all(lm_valid(c.form, c.M, c.N, c.K, c.splits) for c in explicit)
    assert all(c.epilogue in (R, S) and 128 < c.M and c.N % 128 == 0 and c.K % 128 == 0 for c in t)
    assert all((c.M <= 600 and c.N <= 1664 and c.K <= 1024) or (c.M, c.N, c.K) == CEILING for c in t)    # small shapes only
    geom = lambda c: lm_geom(c.form, c.M, c.N, c.K, c.splits)       # noqa: E731

    # M sweep: a ragged and a whole last 16-row group, a ragged and a whole last M tile for both BM
    for form in FORMS:
        assert {c.M for c in explicit if c.sweep == "m" and c.form == form} == set(LM_M), f"form {form}: M list"
    for BM in (128, 256):
        assert any(m % BM == 0 for m in LM_M) and any(m % BM and m % 16 == 0 for m in LM_M) and any(m % 16 for m in LM_M)
        assert any(m % BM == 1 for m in LM_M) and any(m % BM == BM - 1 for m in LM_M)

    # ragged N
    for form in (1, 2):
        mine = [c for c in explicit if c.form == form]
        assert {128, 384, 640} <= {c.N for c in mine if geom(c).ragged_n}, f"form {form}: N % 256 == 128"
        assert any(geom(c).ragged_n and geom(c).ragged_m for c in mine) and any(geom(c).ragged_n and not geom(c).ragged_m for c in mine)
        assert any(not geom(c).ragged_n for c in mine), f"form {form}: no whole N"
        for epi in (R, S):
            for split in (False, True):
                assert any(c.epilogue == epi and (c.splits > 1) == split and c.N == 128 for c in mine), f"form {form}: epilogue {epi} at N = 128"
                assert any(c.epilogue == epi and (c.splits > 1) == split and geom(c).ragged_n and c.bias for c in mine)
    for form in (3, 4):
        assert {128, 384} <= {c.N for c in explicit if c.form == form}

    # stage counts
    assert {(c.K, c.splits) for c in explicit if c.sweep == "k"} == set(LM_KS)
    assert {(128, 1), (128, 2), (384, 1), (384, 2), (384, 3), (1024, 1), (1024, 4), (1024, 16)} <= set(LM_KS)
    for form in FORMS:
        for epi in (R, S):
            nkbs = {geom(c).nkb for c in explicit if c.form == form and c.epilogue == epi}
            assert {1, 2, 3} <= nkbs and any(n >= 4 and n % 2 == 0 for n in nkbs) and any(n >= 4 and n % 2 for n in nkbs), (form, epi, nkbs)
            assert {1, 2, 3, 4, 16} <= {c.splits for c in explicit if c.form == form and c.epilogue == epi}

    # workgroup counts
    nwgs = {geom(c).nwg for c in explicit}
    assert set(range(1, 8)) <= nwgs, sorted(nwgs)
    assert {n % 8 for n in nwgs if n >= 8} == set(range(8)), sorted(nwgs)
    assert {8, 9, 10, 12, 14, 15, 16} <= {geom(c).nwg for c in explicit if c.form == 4 and geom(c).tiles_m in (2, 3)}
    assert {11, 13} <= {geom(c).nwg for c in explicit if c.form == 3 and geom(c).tiles_m == 1 and c.N in (1408, 1664)}
    assert any(c.splits > 1 and geom(c).nwg % 8 for c in explicit)

    # epilogues
    for form in FORMS:
        for epi in (R, S):
            for bias in (False, True):
                for split in (False, True):
                    assert any(c.form == form and c.epilogue == epi and c.bias == bias and (c.splits > 1) == split for c in explicit), \
                        f"form {form} epilogue {epi} bias {bias} split {split} not run"

    # poisoned padding, the default dispatch on every shape, the ceiling
    assert {c.M for c in t if c.sweep == "poison"} == set(LM_POISON_M) and all(m % 16 for m in LM_POISON_M) and set(LM_POISON_M) <= set(LM_M)
    for form in FORMS:
        assert {(c.epilogue, c.splits > 1) for c in explicit if c.sweep == "poison" and c.form == form} == {(R, False), (R, True), (S, False), (S, True)}
    assert {(c.M, c.N, c.K) for c in t if not c.form} == {(c.M, c.N, c.K) for c in t} == set(lm_shapes())
    assert all(c.splits == 0 for c in t if not c.form)
    assert {c.form for c in t if (c.M, c.N, c.K) == CEILING} == {0, 1}


# ---------------------------------------------------------------------------------------------------------------------
# The rules of lm_gemm against the library's return codes: null operands, nothing launched, no GPU needed
# ---------------------------------------------------------------------------------------------------------------------
# what, M, N, K, form (0: ssd_gemm_pf), splits, epilogue, ldy - N, bytes the workspace is short of splits * M * N * 4, null y
LM_REFUSED = [
    ("M past the ceiling", 16385, 256, 256, 0, 0, R, 0, 0, False),
    ("M past the ceiling", 16385, 256, 256, 1, 1, R, 0, 0, False),
    ("N % 128", 300, 192, 256, 0, 0, R, 0, 0, False),
    ("N % 128", 300, 192, 256, 4, 1, R, 0, 0, False),
    ("K % 128", 300, 256, 192, 0, 0, R, 0, 0, False),
    ("K % 128", 300, 256, 192, 4, 1, R, 0, 0, False),
    ("form 5", 300, 256, 256, 5, 1, R, 0, 0, False),
    ("17 splits", 300, 256, 2176, 4, 17, R, 0, 0, False),
    ("3 splits of 8 stages", 300, 256, 512, 4, 3, R, 0, 0, False),
    ("3 splits of 8 stages", 300, 256, 512, 0, 3, R, 0, 0, False),
    ("the partials epilogue", 129, 256, 256, 0, 0, 2, 0, 0, False),
    ("the partials epilogue", 129, 256, 256, 4, 2, 2, 0, 0, False),
    ("a workspace 4 bytes short", 300, 256, 256, 4, 2, R, 0, 4, False),
    ("a workspace 4 bytes short", 300, 256, 256, 1, 2, S, 0, 4, False),
    ("a null y", 300, 256, 256, 0, 0, R, 0, 0, True),
    ("a null y", 300, 256, 256, 4, 2, S, 0, 0, True),
    ("ldy < N", 300, 256, 256, 0, 0, R, -8, 0, False),
    ("ldy < N", 300, 256, 256, 1, 1, R, -8, 0, False),
    ("ldy < N", 300, 256, 256, 4, 2, R, -8, 0, False),
    ("ldy = 0", 300, 256, 256, 0, 0, R, -256, 0, False),
]
LM_REFUSED_CODE = {"M past the ceiling": SHAPE, "N % 128": SHAPE, "K % 128": SHAPE, "ldy < N": SHAPE, "ldy = 0": SHAPE}     # else ARG


def _null_call(lib, M, N, K, form, splits, epilogue, ldy, ws=16, wbytes=1 << 40):
    """ssd_gemm_pf_cfg (form > 0) or ssd_gemm_pf with null x, W, bias and y: every answer comes before any HIP call."""
    z, w = ctypes.c_void_p(0), ctypes.c_void_p(ws)
    if form:
        return lib.ssd_gemm_pf_cfg(z, z, z, z, M, N, K, ldy, epilogue, w, ctypes.c_int64(wbytes), form, splits, z)
    return lib.ssd_gemm_pf(z, z, z, z, M, N, K, ldy, epilogue, w, ctypes.c_int64(wbytes), splits, z)


def _ldy_below_n_is_refused_on_the_host(lib) -> bool:
    """M = 300, N = K = 256, ldy = 248, SSD_EPI_ROWS, null operands: exactly SSD_ERR_SHAPE from both entry points."""
    return _null_call(lib, 300, 256, 256, 0, 0, R, 248) == SHAPE and all(_null_call(lib, 300, 256, 256, f, 1, R, 248) == SHAPE for f in FORMS)


def test_lm_ldy_below_n_is_a_shape_error_without_a_gpu():
    """include/ssd_hip.h asks ldy >= N of SSD_EPI_ROWS; at M > 128 a call with ldy < N used to be launched: its rows overlap and the
    last one is written past the end of y.  Refused beside the other shape checks, ahead of the null-pointer checks."""
    from ssd_amd.hip.lib import load_library
    lib = load_library()
    assert _ldy_below_n_is_refused_on_the_host(lib)
    for splits in (2, 4):
        assert _null_call(lib, 300, 256, 256, 4, splits, R, 248) == SHAPE
    assert _null_call(lib, 300, 256, 256, 0, 0, R, 255) == SHAPE and _null_call(lib, 16384, 128, 128, 1, 1, R, 0) == SHAPE
    assert _null_call(lib, 300, 256, 256, 0, 0, R, 256) == ARG              # ldy == N: valid, the null operands are the error
    assert _null_call(lib, 300, 256, 256, 0, 0, S, 0) == ARG                # SILU_FRAG ignores ldy
    assert _null_call(lib, 100, 256, 256, 2, 1, R, 248) == SHAPE            # the M <= 128 rule, as before


def test_lm_validity_rules_restated_in_python_match_the_library_without_a_gpu():
    """Every table case is valid by lm_valid and answered as a null-operand argument error; every refusal is answered with the code
    of lm_rc, the restatement of lm_gemm's checks in their order."""
    from ssd_amd.hip.lib import load_library
    lib = load_library()
    for c in lm_table():
        if c.form:
            assert lm_valid(c.form, c.M, c.N, c.K, c.splits), c
        ldy = 0 if c.epilogue == S else c.N + GUARD
        assert lm_rc(c.M, c.N, c.K, c.form, c.splits, c.epilogue, ldy) == 0
        assert _null_call(lib, c.M, c.N, c.K, c.form, c.splits, c.epilogue, ldy) == ARG, c
    for what, M, N, K, form, splits, epi, dl, short, null_y in LM_REFUSED:
        want = LM_REFUSED_CODE.get(what, ARG)
        assert (lm_rc(M, N, K, form, splits, epi, N + dl) or ARG) == want, what
        assert (lm_rc(M, N, K, form, splits, epi, N + dl) == 0) == bool(short or null_y), what     # else a rule is what refuses it
        wbytes = (splits * M * N * 4 - short) if short else 1 << 40
        assert _null_call(lib, M, N, K, form, splits, epi, N + dl, wbytes=wbytes) == want, (what, form)
    # the rules one by one around their borders
    for form in range(1, 7):
        for splits in range(-1, 19):
            for M, N, K in ((129, 256, 256), (16384, 128, 128), (16385, 128, 128), (300, 128, 64), (300, 64, 128), (300, 256, 384),
                            (300, 256, 1024), (300, 256, 2176), (300, 0, 256), (300, 256, 0)):
                got = _null_call(lib, M, N, K, form, splits, R, N)
                assert got == (lm_rc(M, N, K, form, splits, R, N) or ARG), (form, splits, M, N, K, got)
                if splits >= 1:
                    assert lm_valid(form, M, N, K, splits) == (lm_rc(M, N, K, form, splits, R, N) == 0), (form, splits, M, N, K)


# ---------------------------------------------------------------------------------------------------------------------
# The GPU harness
# ---------------------------------------------------------------------------------------------------------------------
class _Bufs(NamedTuple):
    yb: torch.Tensor         # int16, sentinel-filled: the ROWS frame or the SILU fragment plus its tail
    rows: int
    ldy: int
    ws: torch.Tensor         # int32, sentinel-filled: the workspace's n floats plus its tail
    n: int


class _Lm:
    def __init__(self, dev, name, sweep=None):
        self.dev, self.mats, self.worst = dev, _Mats(dev), _Worst(f"bf16 lm {name}")
        self.cases = sorted((c for c in lm_table() if c.sweep == sweep), key=lambda c: (c.N, c.K, c.M))

    def ws_floats(self, c) -> int:
        """An explicit split gets exactly splits * M * N floats, the default dispatch exactly what the workspace query answers."""
        from ssd_amd.hip import ops as H
        if not c.form:
            return H.gemm_pf_workspace_bytes(c.M, c.N, c.K) // 4
        return c.splits * c.M * c.N if c.splits > 1 else 0

    def buffers(self, c) -> _Bufs:
        n = self.ws_floats(c)
        ws = torch.full((n + TAIL,), SENTINEL32, dtype=torch.int32, device=self.dev)
        if c.epilogue == S:
            return _Bufs(_guarded_frag(self.dev, c.M, c.N // 2), 0, 0, ws, n)
        rows, ldy = c.M + GUARD, c.N + GUARD
        return _Bufs(torch.full((rows * ldy,), SENTINEL, dtype=torch.int16, device=self.dev), rows, ldy, ws, n)

    def launch(self, c, b, xf=None, wf=None):
        from ssd_amd.hip import ops as H
        xf = self.mats.x(c.M, c.K)[1] if xf is None else xf
        wf = self.mats.w(c.N, c.K)[0] if wf is None else wf
        H.gemm_pf(xf, wf, b.yb.view(BF), c.M, c.N, c.K, b.ldy, b.ws.view(torch.float32)[:b.n], epilogue=c.epilogue,
                  bias=self.mats.bias(c.N) if c.bias else None, splits=c.splits, nt=c.form)

    def collect(self, c, b):
        """The guards, then the output as bf16 rows: [M, N], or [M, N / 2] through the SILU fragment."""
        what = f"lm {c}"
        assert bool((b.ws[b.n:] == SENTINEL32).all()), f"{what}: memory past the workspace's {b.n} floats was written"
        if c.epilogue == S:
            return _check_guarded_frag(b.yb, c.M, c.N // 2, what)
        return _check_guarded_rows(b.yb, b.rows, b.ldy, c.M, c.N, what)

    def run(self, c, xf=None, wf=None):
        b = self.buffers(c)
        self.launch(c, b, xf, wf)
        return self.collect(c, b)

    def check(self, c, y, want=None):
        what, how = f"lm {c}", "default" if not c.form else "direct" if c.splits == 1 else "split"
        if c.epilogue == R:
            want = self.mats.ref(c.M, c.N, c.K, c.bias) if want is None else want
            self.worst.add(f"ROWS {how}", assert_within_ulp(y, want, what))
        else:
            want = self.mats.ref(c.M, c.N, c.K, c.bias, True) if want is None else want
            self.worst.add(f"SILU_FRAG {how}", assert_silu_within_bar(y, want, c.N // 2, what))
        self.worst.n += 1


@gpu
@pytest.mark.parametrize("sweep", LM_SWEEPS)
def test_lm_sweep_against_float64_with_tile_wide_guards(dev, sweep):
    """Every table case to the bars, ROWS into a frame of 256 sentinel rows past M and 256 sentinel columns past N, SILU_FRAG into its
    fragment plus a tail, the workspace exact, NaN-prefilled and followed by a tail; every output written, two runs bit-equal."""
    h = _Lm(dev, sweep, sweep)
    assert h.cases
    for c in h.cases:
        y = h.run(c)
        h.check(c, y)
        assert torch.equal(_bits(h.run(c)), _bits(y)), f"lm {c}: two runs differ"
    assert h.worst.n == len(h.cases)
    h.worst.report()


@gpu
def test_lm_forms_compute_the_same_bits_on_every_table_shape(dev):
    """A form changes who computes a tile, never the K order: unsplit, forms 2, 3, 4 equal form 1 bit for bit, ROWS + bias and
    SILU_FRAG + bias, on every shape of the table -- N % 256 == 128 included, where forms 1 and 2 clamp and skip."""
    h, n = _Lm(dev, "forms"), 0
    for M, N, K in lm_shapes():
        for epi in (R, S):
            base = h.run(LmCase("forms", M, N, K, epi, True, 1, 1))
            for form in (2, 3, 4):
                y = h.run(LmCase("forms", M, N, K, epi, True, form, 1))
                assert torch.equal(_bits(y), _bits(base)), f"lm {(M, N, K)} epilogue {epi}: form {form} differs from form 1"
                n += 1
    print(f"bf16 lm forms: {n} launches bit-identical to form 1 over {len(lm_shapes())} shapes")


def chunks(M: int) -> list[tuple[int, int]]:
    """(m0, m): <= 128-row chunks at 16-row offsets, each of more than 16 rows -- ssd_gemm_pf_cfg's floor; the engine sends a shorter
    tail to ssd_gemm_wf -- so a remainder of <= 16 rows takes 16 rows from the chunk before it."""
    out, m0 = [], 0
    while m0 < M:
        m = min(128, M - m0)
        if 0 < M - m0 - m <= 16:
            m -= 16
        out.append((m0, m))
        m0 += m
    return out


def test_chunks_are_the_engine_s_up_to_a_short_tail():
    assert chunks(255) == [(0, 128), (128, 127)] and chunks(256) == [(0, 128), (128, 128)] and chunks(300) == [(0, 128), (128, 128), (256, 44)]
    assert chunks(257) == [(0, 128), (128, 112), (240, 17)]
    for M in range(129, 601):
        cs = chunks(M)
        assert sum(m for _, m in cs) == M and all(m0 % 16 == 0 and 16 < m <= 128 for m0, m in cs)
        assert all(a[0] + a[1] == b[0] for a, b in zip(cs, cs[1:]))


@gpu
@pytest.mark.parametrize("N,K", [(512, 512), (768, 384)])
def test_lm_one_launch_equals_the_chunk_loop_by_bits(dev, N, K):
    """gemm_lm_kernel and gemm_pf_kernel both walk K in ascending 32-deep steps into one accumulator with the same mfma16(w, x, acc),
    and share the epilogue arithmetic: one unsplit long launch equals the loop of <= 128-row chunks through
    ssd_gemm_pf_cfg(nt = 2, splits = 1) at HipDecoder._gemm's offsets bit for bit, ROWS and SILU_FRAG, both with a bias."""
    from ssd_amd.hip import ops as H
    h = _Lm(dev, "chunks")
    wf, bias, I = h.mats.w(N, K)[0], h.mats.bias(N), N // 2
    none = torch.empty(0, dtype=torch.float32, device=dev)
    for M in (255, 256, 257, 300):
        xf = h.mats.x(M, K)[1]
        for form in (1, 4):
            long_rows = h.run(LmCase("chunks", M, N, K, R, True, form, 1))
            long_silu = h.run(LmCase("chunks", M, N, K, S, True, form, 1))
            if form == 1:
                h.check(LmCase("chunks", M, N, K, R, True, form, 1), long_rows)
                h.check(LmCase("chunks", M, N, K, S, True, form, 1), long_silu)
            yb = torch.full((M * N,), SENTINEL, dtype=torch.int16, device=dev)
            fb = _guarded_frag(dev, M, I)
            for m0, m in chunks(M):
                x_off = (m0 // 16) * (K // 32) * 512
                H.gemm_pf(xf[x_off:], wf, yb.view(BF)[m0 * N:], m, N, K, N, none, epilogue=R, bias=bias, splits=1, nt=2)
                H.gemm_pf(xf[x_off:], wf, fb.view(BF)[(m0 // 16) * (I // 32) * 512:], m, N, K, 0, none, epilogue=S, bias=bias, splits=1, nt=2)
            assert torch.equal(yb.view(M, N), _bits(long_rows)), f"lm form {form} M {M} N {N} K {K}: ROWS differ from the chunk loop"
            chunk_silu = _check_guarded_frag(fb, M, I, f"chunk loop M {M}")
            assert torch.equal(_bits(chunk_silu), _bits(long_silu)), f"lm form {form} M {M} N {N} K {K}: SILU_FRAG differs from the chunk loop"
    h.worst.report()


@gpu
def test_lm_poisoned_x_padding_rows_never_reach_a_real_row(dev):
    """Rows [M, ceil16(M)) of the x fragment are staged by LDS-DMA and multiplied, in the last real row group and in every group past
    it that is clamped onto it; an MFMA output column depends on its own token row only, so no row < M may change by one bit."""
    h = _Lm(dev, "poison", "poison")
    explicit = [c for c in h.cases if c.form]
    for c in explicit:
        assert c.M % 16 and ceil16(c.M) > c.M
        clean = h.run(c)
        h.check(c, clean)
        dirty = h.run(c, xf=h.mats.poisoned(c.M, c.K))
        assert torch.equal(_bits(dirty), _bits(clean)), f"lm {c}: padding rows of x changed a row < M"
    assert h.worst.n == len(explicit) == len(LM_POISON_M) * len(FORMS) * 4
    h.worst.report()


@gpu
@pytest.mark.parametrize("N,K", [(256, 512), (1280, 1024), (128, 1024)])
def test_lm_one_workspace_sized_at_the_longest_prompt_serves_every_shorter_one(dev, N, K):
    """As the engine sizes it: exactly gemm_pf_workspace_bytes(600, N, K) bytes, NaN-prefilled, with a sentinel tail.  Every M of the
    list succeeds through the default dispatch with that one buffer and meets the bar; the tail stays untouched."""
    from ssd_amd.hip import ops as H
    h = _Lm(dev, f"workspace N {N} K {K}")
    n = H.gemm_pf_workspace_bytes(600, N, K) // 4
    wf, bias = h.mats.w(N, K)[0], h.mats.bias(N)
    for M in LM_M:
        c = LmCase("ws", M, N, K, R, True, 0, 0)
        assert H.gemm_pf_workspace_bytes(M, N, K) // 4 <= n, f"{c}: a shorter prompt needs more than the longest"
        b = h.buffers(c)._replace(ws=torch.full((n + TAIL,), SENTINEL32, dtype=torch.int32, device=dev), n=n)
        h.launch(c, b)
        h.check(c, h.collect(c, b))
    print(f"workspace for M <= 600 at N {N} K {K}: {n * 4} bytes")
    h.worst.report()


@gpu
def test_lm_hipgraph_replay_equals_eager(dev):
    """A split ROWS case (GEMM + epilogue kernel) and a direct SILU_FRAG case, captured and replayed twice with the output and the
    workspace poisoned again in between."""
    h = _Lm(dev, "graph")
    for c in (LmCase("graph", 300, 384, 384, R, True, 4, 3), LmCase("graph", 273, 384, 256, S, True, 1, 1)):
        eager = h.run(c)
        h.check(c, eager)
        b = h.buffers(c)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):         # warm-up on the capture stream
            h.launch(c, b)
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            h.launch(c, b)
        for _ in range(2):
            b.yb.fill_(SENTINEL)
            b.ws.fill_(SENTINEL32)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(h.collect(c, b)), _bits(eager)), f"lm {c}: a replay differs from eager"
    h.worst.report()


def _quantized(fmt, N, K, dev):
    """(dequantize into a bf16 fragment, the host-dequantized bf16 [N, K]) of one format's random codes, in its row form."""
    from ssd_amd import quant as QT
    if fmt == "fp8":
        from ssd_amd.hip import quant_ops as Q
        from tests.test_hip_quant_edges import _Fp8
        rows = _Fp8().rows(N, K, dev, 3)
        qf, s = _Fp8().frag(rows, N, K, dev, None)
        return (lambda out: Q.fp8_dequant_frag(qf, s, out, N, K)), QT.dequantize_fp8(rows[0].view(torch.float8_e4m3fn), rows[1])
    if fmt == "w4a16":
        from ssd_amd.hip import w4_ops as W4
        from tests.test_hip_quant_edges import _W4
        rows = _W4().rows(N, K, dev, 3)
        qf, sf = _W4().frag(rows, N, K, dev, None)
        return (lambda out: W4.w4_dequant_frag(qf, sf, out, N, K)), QT.dequantize_w4a16(rows[2], rows[1])
    if fmt == "w4a16_zp":
        from ssd_amd.hip import w4zp_ops as W4Z
        from tests.test_hip_w4zp import _codes, _frag
        u, s, z, packed = _codes(N, K, dev, 3)
        qf, sf, zf = _frag(packed, s, z, N, K, dev)
        return (lambda out: W4Z.w4zp_dequant_frag(qf, sf, zf, out, N, K)), QT.dequantize_w4zp(packed, s, z)
    from ssd_amd.hip import mx4_ops as MX4
    from tests.test_hip_quant_edges import _Mx4
    rows = _Mx4().rows(N, K, dev, 3)
    qf, sf = _Mx4().frag(rows, N, K, dev, None)
    return (lambda out: MX4.mx4_dequant_frag(qf, sf, out, N, K)), QT.dequantize_mxfp4(rows[0], rows[1])


@gpu
@pytest.mark.parametrize("fmt", ["fp8", "w4a16", "w4a16_zp", "mxfp4"])
def test_lm_quantized_long_route_dequantizes_into_a_larger_dirty_scratch(dev, fmt):
    """The engine's route for a quantized target at M > 128: *_dequant_frag into _deq -- sized for the largest matrix and still
    holding the one before -- then gemm_pf on it.  The scratch here is N * K elements plus as many again of a NaN pattern: the
    result equals gemm_pf on the fragment form of the host-dequantized matrix bit for bit and meets the ROWS bar over those
    values, and the scratch past N * K is untouched."""
    from ssd_amd.hip import ops as H
    N, K = 256, 512
    h = _Lm(dev, f"quantized {fmt}")
    dequant, w_host = _quantized(fmt, N, K, dev)
    assert w_host.dtype == BF and w_host.shape == (N, K) and bool(torch.isfinite(w_host.float()).all())
    scratch = torch.full((2 * N * K,), SENTINEL, dtype=torch.int16, device=dev)
    dequant(scratch.view(BF))
    assert bool((scratch[N * K:] == SENTINEL).all()), f"{fmt}: the scratch past N * K was written"
    wf_host = torch.empty(N * K, dtype=BF, device=dev)
    H.rows_to_frag(w_host.contiguous(), wf_host, N, K)
    for M in (257, 300):
        c = LmCase("quant", M, N, K, R, False, 0, 0)
        y = h.run(c, wf=scratch.view(BF))
        assert torch.equal(_bits(y), _bits(h.run(c, wf=wf_host))), f"{fmt} M {M}: differs from the host-dequantized run"
        h.check(c, y, want=h.mats.x(M, K)[0].double() @ w_host.double().T)
    assert bool((scratch[N * K:] == SENTINEL).all()), f"{fmt}: the scratch past N * K was written"
    h.worst.report()


@gpu
def test_lm_refusals_return_an_error_and_write_nothing(dev):
    """Each refusal raises and leaves a sentinel-filled y and workspace as they were.  The `ldy < N` calls are sent only to a library
    that refuses them with null operands first: an unfixed one would launch the overlapping store."""
    from ssd_amd.hip import ops as H
    from ssd_amd.hip.lib import load_library
    assert _ldy_below_n_is_refused_on_the_host(load_library()), "this library launches ldy < N at M > 128: not sent to the GPU"
    mats = _Mats(dev)
    xf, wf = mats.x(300, 256)[1], mats.w(256, 256)[0]
    yb = torch.full((600 * 512,), SENTINEL, dtype=torch.int16, device=dev)
    ws = torch.full((16 * 300 * 256,), SENTINEL32, dtype=torch.int32, device=dev)
    for what, M, N, K, form, splits, epi, dl, short, null_y in LM_REFUSED:
        n = ws.numel() if not short else (splits * M * N * 4 - short) // 4
        _refused(dev, f"lm {what} (form {form})",
                 lambda: H.gemm_pf(xf, wf, None if null_y else yb.view(BF), M, N, K, N + dl, ws.view(torch.float32)[:n], epilogue=epi,
                                   splits=splits, nt=form), yb, ws)
    # a split call without any workspace
    none = torch.empty(0, dtype=torch.float32, device=dev)
    _refused(dev, "lm no workspace", lambda: H.gemm_pf(xf, wf, yb.view(BF), 300, 256, 256, 256, none, splits=2, nt=4), yb, ws)
