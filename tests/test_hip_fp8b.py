"""Block-scaled FP8 kernels on the MI355X (csrc/gemm_fp8b.hip, include/ssd_hip_fp8b.h): ssd_fp8b_dequant_frag against
bf16(fp32(s) * fp32(q)) computed in torch, by bits; the default dispatch ssd_gemm_fp8b against float64 arithmetic on the exact
weights, on small ragged shapes and on one layer's four matrices of Llama-3.1-8B and Qwen3-32B.

The scale tables here are GROUP-granular -- one independent, non-power-of-two scale per 16-row group and 128-column block, spread
over six binades -- so that an indexing error in either direction changes the result (at the checkpoint's 128-row granularity most
small shapes would have a single scale).  Bars: those of tests/test_hip_quant_edges.py (imported from tests/test_hip_mxfp4.py): ROWS
1 bf16 ulp floored at 2^-6 of the output rms; SILU_FRAG its own bar."""
import pytest
import torch

from tests.test_hip_mxfp4 import SHAPES, mats, _x, assert_silu_within_bar, assert_within_ulp, dev  # noqa: F401  (dev is the fixture)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SMALL = ((16, 64), (48, 192), (160, 320))       # one unit / a half last block, three groups / a ragged group count and half block
MS = (1, 8, 17, 128)


def _codes(N, K, dev, seed):
    """e4m3 codes uint8 [N, K] without NaN codes and a group table fp32 [N / 16, ceil(K / 128)] = 2^e * m, e uniform in -12..-7 and
    m uniform in [1.0625, 1.9375): never a power of two."""
    g = torch.Generator(device=dev).manual_seed(seed)
    codes = torch.randint(0, 256, (N, K), generator=g, device=dev, dtype=torch.uint8)
    codes[(codes & 0x7f) == 0x7f] = 0x3c
    shape = (N // 16, -(-K // 128))
    e = torch.randint(-12, -6, shape, generator=g, device=dev).float()
    m = 1.0625 + 0.875 * torch.rand(shape, generator=g, device=dev)
    return codes, (m * torch.exp2(e)).float().contiguous()


def _values(codes):
    """f64 (-1)^sign * 2^(e - 7) * (1 + m / 8), subnormal 2^-6 * m / 8 at e = 0 (OCP e4m3fn), from the definition."""
    c = codes.to(torch.int64)
    assert not bool(((c & 0x7f) == 0x7f).any()), "a NaN code"
    e, m = ((c >> 3) & 15).double(), (c & 7).double()
    v = torch.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * torch.exp2(e - 7))
    return torch.where((c & 0x80) != 0, -v, v)


def _elem(table, N, K):
    """The group table expanded to one scale per element, in the row order the table is in."""
    return table.repeat_interleave(16, dim=0).repeat_interleave(128, dim=1)[:N, :K]


def _exact(codes, table):
    N, K = codes.shape
    return _values(codes) * _elem(table, N, K).double()


def _frag(codes, table, N, K, dev, rmap=None):
    """(fp8 frag codes, group table in packed row order): expand to one scale row per output row, permute, take one per group."""
    from ssd_amd.hip import quant_ops as Q
    from ssd_amd.quant import fp8_block_group_scales
    qf = torch.empty(N * K, dtype=torch.uint8, device=dev)
    Q.fp8_rows_to_frag(codes, qf, N, K, row_map=rmap)
    return qf, fp8_block_group_scales(table.repeat_interleave(16, dim=0), rmap, "test")


@pytest.mark.parametrize("N,K,gate_up", [(16, 64, False), (48, 192, False), (160, 320, False), (64, 128, True)])
def test_dequant_frag_bit_equal_to_torch(dev, N, K, gate_up):
    from ssd_amd.hip import fp8b_ops as F8B
    from ssd_amd.hip import ops as H
    from ssd_amd.quant import gate_up_row_map
    codes, table = _codes(N, K, dev, N + K)
    rmap = gate_up_row_map(N).to(dev) if gate_up else None
    qf, tp = _frag(codes, table, N, K, dev, rmap)
    wf = torch.full((N * K,), float("nan"), dtype=BF, device=dev)
    F8B.fp8b_dequant_frag(qf, tp, wf, N, K)
    rows = torch.empty(N, K, dtype=BF, device=dev)
    H.frag_to_rows(wf, rows, N, K)
    want = (codes.view(torch.float8_e4m3fn).float() * _elem(table, N, K)).to(BF)          # source row order
    if rmap is not None:
        want = want[rmap.long()]
        assert not torch.equal(tp, table)                                                 # the map did move scales
    assert torch.equal(rows.view(torch.int16), want.view(torch.int16))


def _run_default(dev, codes, table, N, K, silu, what):
    """ssd_gemm_fp8b's own decomposition at every M of MS against f64 on the exact weights (computed once per matrix)."""
    from ssd_amd.hip import fp8b_ops as F8B
    from ssd_amd.hip import ops as H
    from ssd_amd.quant import gate_up_row_map
    w = _exact(codes, table)
    qf, tp = _frag(codes, table, N, K, dev, gate_up_row_map(N).to(dev) if silu else None)
    bias = (torch.randn(N, generator=torch.Generator(device=dev).manual_seed(3), device=dev) * 0.1).to(BF)
    for M in MS:
        x, xf = _x(M, K, dev, seed=M)
        want = x.double() @ w.T
        if silu:
            I = N // 2
            yf = torch.zeros(H.frag_numel(M, I), dtype=BF, device=dev)
            F8B.gemm_fp8b(xf, qf, tp, yf, M, N, K, 0, epilogue=H.EPI_SILU_FRAG)
            y = torch.empty(M, I, dtype=BF, device=dev)
            H.frag_to_rows(yf, y, M, I)
            assert_silu_within_bar(y, want, I, f"{what} silu M={M}")
        else:
            b = bias if M % 2 == 0 else None
            y = torch.empty(M, N, dtype=BF, device=dev)
            F8B.gemm_fp8b(xf, qf, tp, y, M, N, K, N, bias=b)
            assert_within_ulp(y, want if b is None else want + b.double(), f"{what} M={M}")


@pytest.mark.parametrize("N,K", SMALL + ((64, 128),))
def test_default_dispatch_small_shapes(dev, N, K):
    codes, table = _codes(N, K, dev, 7 * N + K)
    _run_default(dev, codes, table, N, K, False, f"{N}x{K}")
    if N % 64 == 0:
        _run_default(dev, codes, table, N, K, True, f"{N}x{K}")


@pytest.mark.parametrize("kind", ["qkv", "o", "gate_up", "down"])
@pytest.mark.parametrize("model", ["8b", "qwen3-32b"])
def test_default_dispatch_real_shapes(dev, model, kind):
    N, K = mats(SHAPES[model])[kind]
    codes, table = _codes(N, K, dev, N + K)
    _run_default(dev, codes, table, N, K, kind == "gate_up", f"{model} {kind}")
    del codes, table
    torch.cuda.empty_cache()
