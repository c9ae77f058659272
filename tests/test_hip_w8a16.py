"""W8A16 weight kernels on the MI355X (csrc/gemm_w8a16.hip): rows -> frag -> rows by bits, the dequantize kernel by bits, the GEMM
against float64 arithmetic on the exact weights s * q (the bar of tests/test_hip_w4a16.py: the same arithmetic contract), every
explicit decomposition against the default's bits, hipGraph replay."""
import pytest
import torch

from tests.test_hip_w4a16 import assert_within_ulp, bf16_ulp, _x

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _codes(N, K, dev, seed):
    """Random codes over the full range (as q and as the row form's bytes u = q + 128) and bf16 scales of a 0.02-std weight's size."""
    g = torch.Generator(device=dev).manual_seed(seed)
    q = torch.randint(-128, 128, (N, K), generator=g, device=dev, dtype=torch.int16)
    s = (torch.rand(N, K // 128, generator=g, device=dev) * 4e-4 + 1e-4).to(BF)
    return q, s, (q + 128).to(torch.uint8)


def _frag(u, s, N, K, dev, rmap=None):
    from ssd_amd.hip import w8_ops as W8
    qf = torch.empty(N * K, dtype=torch.uint8, device=dev)
    sf = torch.empty(N * K // 128, dtype=BF, device=dev)
    W8.w8_rows_to_frag(u, s, qf, sf, N, K, row_map=rmap)
    return qf, sf


def _exact(q, s):
    return q.double() * s.double().repeat_interleave(128, dim=1)


@pytest.mark.parametrize("mapped", [False, True])
def test_rows_to_frag_is_the_documented_layout_and_round_trips(dev, mapped):
    from ssd_amd.quant import gate_up_row_map
    from ssd_amd.hip import w8_ops as W8
    N, K = 32, 256
    q, s, u = _codes(N, K, dev, 1)
    order = gate_up_row_map(N).long() if mapped else torch.arange(N)
    qf, sf = _frag(u, s, N, K, dev, order.to(torch.int32).to(dev) if mapped else None)
    # [N/16][K/64][64 lanes][16 bytes]: lane l = row l & 15, bytes 0..7 / 8..15 = columns 8 (l >> 4) + 0..7 of k-tiles 2p / 2p+1
    src = q[order.to(dev)].to(torch.int8).reshape(N // 16, 16, K // 64, 2, 4, 8)           # g, r, p, h, l >> 4, e
    want = src.permute(0, 2, 4, 1, 3, 5).reshape(-1)                                        # g, p, l >> 4, r, h, e
    assert torch.equal(qf.view(torch.int8), want)
    assert torch.equal(sf.view(torch.int16), s[order.to(dev)].reshape(N // 16, 16, K // 128).transpose(1, 2).reshape(-1).view(torch.int16))
    back_u, back_s = torch.empty_like(u), torch.empty_like(s)
    W8.w8_frag_to_rows(qf, sf, back_u, back_s, N, K)
    assert torch.equal(back_u, u[order.to(dev)]) and torch.equal(back_s.view(torch.int16), s[order.to(dev)].view(torch.int16))


def test_dequant_frag_is_bf16_of_s_times_q_for_every_code_in_every_byte_position(dev):
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import w8_ops as W8
    from ssd_amd.quant import dequantize_w8a16
    N, K = 256, 1024
    # 16 row groups x 16 code units: unit (g, p) holds code (16 g + p + row + column) % 256 - 128 at its (row, column), so every
    # (lane, byte) position sees all 256 codes; the scales alternate between nearly the largest that keeps 128 s finite and a tiny one
    n, k = torch.arange(N, device=dev)[:, None], torch.arange(K, device=dev)[None, :]
    q = ((16 * (n // 16) + k // 64 + n % 16 + k % 64) % 256 - 128).to(torch.int16)
    s = torch.tensor([3.0e38 / 128, 2.0 ** -120], device=dev).to(BF)[(n + torch.arange(K // 128, device=dev)[None, :]) % 2].contiguous()
    u = (q + 128).to(torch.uint8)
    qf, sf = _frag(u, s, N, K, dev)
    wf = torch.empty(N * K, dtype=BF, device=dev)
    W8.w8_dequant_frag(qf, sf, wf, N, K)
    rows = torch.empty(N, K, dtype=BF, device=dev)
    H.frag_to_rows(wf, rows, N, K)
    want = (s.float().repeat_interleave(128, dim=1) * q.float()).to(BF)
    assert torch.isfinite(want.float()).all()
    assert torch.equal(rows.view(torch.int16), want.view(torch.int16))
    assert torch.equal(rows.view(torch.int16), dequantize_w8a16(u, s).view(torch.int16))


def _gemm(dev, M, N, K, epi_silu, bias_on, seed, cfg=None, operands=None):
    """(y rows bf16 [M, N], or [M, N / 2] of silu(gate) * up; the f64 x . (s q)^T + bias [M, N] before any rounding)."""
    from ssd_amd.quant import gate_up_row_map
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import w8_ops as W8
    q, s, u = _codes(N, K, dev, seed)
    x, xf = _x(M, K, dev, seed + 1)
    bias = (torch.randn(N, device=dev) * 0.1).to(BF) if bias_on else None
    if operands is not None:
        q, s, u, x, xf, bias = operands
    rmap = gate_up_row_map(N).to(dev) if epi_silu else None
    qf, sf = _frag(u, s, N, K, dev, rmap)
    want = x.double() @ _exact(q, s).T
    if bias is not None:
        want = want + bias.double()
    if not epi_silu:
        y = torch.empty(M, N, dtype=BF, device=dev)
        W8.gemm_w8a16(xf, qf, sf, y, M, N, K, N, bias=bias, cfg=cfg)
        return y, want
    yf = torch.zeros(H.frag_numel(M, N // 2), dtype=BF, device=dev)
    packed_bias = None if bias is None else bias[rmap.long()].contiguous()       # the bias follows its rows into the packed order
    W8.gemm_w8a16(xf, qf, sf, yf, M, N, K, 0, epilogue=H.EPI_SILU_FRAG, bias=packed_bias, cfg=cfg)
    y = torch.empty(M, N // 2, dtype=BF, device=dev)
    H.frag_to_rows(yf, y, M, N // 2)
    return y, want


@pytest.mark.parametrize("bias_on", [False, True])
@pytest.mark.parametrize("N", [64, 208])
@pytest.mark.parametrize("K", [128, 384, 1152])
@pytest.mark.parametrize("M", [1, 16, 17, 64, 128])
def test_gemm_w8a16_rows_within_one_ulp_of_f64(dev, M, K, N, bias_on):
    y, want = _gemm(dev, M, N, K, False, bias_on, seed=M + K + N)
    assert_within_ulp(y, want, f"rows M={M} N={N} K={K} bias={bias_on}")


@pytest.mark.parametrize("bias_on", [False, True])
@pytest.mark.parametrize("K", [128, 384, 1152])
@pytest.mark.parametrize("M", [1, 16, 17, 64, 128])
def test_gemm_w8a16_silu_within_the_w4a16_bar_of_f64(dev, M, K, bias_on):
    """SILU_FRAG needs N % 64 == 0 (the entry refuses 208, as ssd_gemm_w4a16 does): N = 64 and 192.  The bar is _check_silu's of
    tests/test_hip_w4a16.py."""
    for N in (64, 192):
        y, yg = _gemm(dev, M, N, K, True, bias_on, seed=M + K + N)
        I = N // 2
        g, u = yg[:, :I].to(BF).double(), yg[:, I:].to(BF).double()
        sg = torch.sigmoid(g)
        want = g * sg * u
        slack = (u * sg * (1 + g * (1 - sg))).abs() * bf16_ulp(g) + (g * sg).abs() * bf16_ulp(u)
        floor = want.pow(2).mean().sqrt() * 2 ** -6
        tol = 3.0 * bf16_ulp(torch.maximum(want.to(BF).double().abs(), floor)) + slack
        d = (y.double() - want.to(BF).double()).abs()
        assert not bool((d > tol).any()), f"silu M={M} N={N} K={K}: worst {(d / tol).max().item():.2f} x tol"


def test_every_explicit_decomposition_gives_the_defaults_bits_and_graph_replay_equals_eager(dev):
    """N = 256, K = 2048 (32 code units: every wave count has work, U = 6 leaves a remainder) at M = 8 / 24 / 128.  Decompositions
    split K over waves differently, so their fp32 sums are taken in different orders; the operands here make every fp32 operation
    exact (x integers in [-4, 4], power-of-two scales 2^-9 .. 2^-6, bias in eighths: every partial is an integer below 2^15 and every
    sum a multiple of 2^-9 below 2^14), so the order cannot matter and each decomposition must give the default's bits -- which are
    bf16 of the float64 value."""
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import w8_ops as W8
    N, K = 256, 2048
    g = torch.Generator(device=dev).manual_seed(5)
    q = torch.randint(-128, 128, (N, K), generator=g, device=dev, dtype=torch.int16)
    s = torch.exp2(torch.randint(-9, -5, (N, K // 128), generator=g, device=dev).float()).to(BF)
    bias = (torch.randint(-16, 17, (N,), generator=g, device=dev).float() / 8).to(BF)
    for M, nts, wvs in ((8, (1, 2, 4, 1 | 256, 2 | 256, 4 | 256), (1, 4, 8, 8 | (2 << 8))), (24, (1, 2), (1, 2, 4)), (128, (1, 2), (1, 2, 4))):
        x = torch.randint(-4, 5, (M, K), generator=g, device=dev).to(BF)
        xf = torch.zeros(H.frag_numel(M, K), dtype=BF, device=dev)
        H.rows_to_frag(x, xf, M, K)
        ops = (q, s, (q + 128).to(torch.uint8), x, xf, bias)
        y0, want = _gemm(dev, M, N, K, False, True, 0, operands=ops)
        assert torch.equal(y0.view(torch.int16), want.to(BF).view(torch.int16)), f"default M={M}"
        for nt in nts:
            for waves in wvs:
                y, _ = _gemm(dev, M, N, K, False, True, 0, cfg=(nt, waves), operands=ops)
                assert torch.equal(y.view(torch.int16), y0.view(torch.int16)), f"M={M} cfg nt {nt} waves {waves}"
    q, s, u = _codes(N, K, dev, 9)
    qf, sf = _frag(u, s, N, K, dev)
    x, xf = _x(8, K, dev, 10)
    y_e, y_g = torch.empty(8, N, dtype=BF, device=dev), torch.empty(8, N, dtype=BF, device=dev)
    W8.gemm_w8a16(xf, qf, sf, y_e, 8, N, K, N)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):         # warm-up on the capture stream
        W8.gemm_w8a16(xf, qf, sf, y_g, 8, N, K, N)
    st.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        W8.gemm_w8a16(xf, qf, sf, y_g, 8, N, K, N)
    y_g.zero_()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_g.view(torch.int16), y_e.view(torch.int16))
