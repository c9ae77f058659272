"""Zero-point W4A16 kernels on the MI355X (csrc/gemm_w4a16.hip, ZP instantiations; include/ssd_hip_w4zp.h): the re-tiling against
the numpy restatements (tests/w4a16_ref.py for the unchanged code and scale layouts, tests/w4zp_ref.py for the zero-point table),
bit for bit, with and without row maps, and back; the dequantize kernel over every (code, zero point, position); the GEMM against
float64 arithmetic on the exact weights s * (u - z); z = 8 against the symmetric kernel; repeat determinism; hipGraph replay.

Bars: those of tests/test_hip_w4a16.py, imported -- |HIP - bf16(f64)| <= 1 bf16 ulp of the reference value, the ulp taken at no less
than 2^-6 of the output's rms, no exempt share; SILU_FRAG under that file's bar (3 ulp plus the first-order gate / up term)."""
import numpy as np
import pytest
import torch

from tests import w4a16_ref as R4
from tests import w4zp_ref as R
from tests.test_hip_w4a16 import SHAPES, mats, dev, bf16_ulp, assert_within_ulp, _x  # noqa: F401  (dev is the fixture)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _codes(N, K, dev, seed, zero=None):
    """Random unsigned codes over 0..15, zero points over 0..15 (both extremes forced into the first rows, next to codes 0 and 15, so
    u - z reaches -15 and 15) and bf16 scales of a 0.02-std weight's size, in the row form.  zero: a constant zero point instead."""
    from ssd_amd.quant import pack_w4u
    g = torch.Generator(device=dev).manual_seed(seed)
    u = torch.randint(0, 16, (N, K), generator=g, device=dev, dtype=torch.uint8)
    z = torch.randint(0, 16, (N, K // 128), generator=g, device=dev, dtype=torch.uint8)
    s = (torch.rand(N, K // 128, generator=g, device=dev) * 6e-3 + 2e-3).to(BF)
    if zero is None:
        z[0, :], z[1, :] = 0, 15
        u[0, 0::2], u[0, 1::2] = 15, 0
        u[1, 0::2], u[1, 1::2] = 0, 15
    else:
        z[:] = zero
    return u, s, z, pack_w4u(u)


def _frag(packed, s, z, N, K, dev, rmap=None):
    from ssd_amd.hip import w4zp_ops as W4Z
    qf = torch.empty(N * K // 2, dtype=torch.uint8, device=dev)
    sf = torch.empty(N * K // 128, dtype=BF, device=dev)
    zf = torch.empty(N * K // 128, dtype=torch.uint8, device=dev)
    W4Z.w4zp_rows_to_frag(packed, s, z, qf, sf, zf, N, K, row_map=rmap)
    return qf, sf, zf


def _exact(u, s, z):
    """f64 s * (u - z) [N, K]."""
    return (u.double() - z.double().repeat_interleave(128, dim=1)) * s.double().repeat_interleave(128, dim=1)


def _bits(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def test_rows_to_frag_round_trip_bit_exact_with_and_without_row_maps(dev):
    from ssd_amd.quant import qkv_row_map, gate_up_row_map
    from ssd_amd.hip import w4zp_ops as W4Z
    N, K = 384, 1152
    u, s, z, packed = _codes(N, K, dev, 1)
    u_np, s_np, z_np = u.cpu().numpy(), _bits(s), z.cpu().numpy()
    for rmap in (None, gate_up_row_map(N), qkv_row_map(4, 1, 64)):
        order = np.arange(N) if rmap is None else rmap.numpy().astype(np.int64)
        qf, sf, zf = _frag(packed, s, z, N, K, dev, None if rmap is None else rmap.to(dev))
        assert np.array_equal(qf.cpu().numpy().view(np.uint32), R4.to_frag(u_np[order].astype(np.int64) - 8))
        assert np.array_equal(_bits(sf), R4.scale_frag(s_np[order]))
        assert np.array_equal(zf.cpu().numpy(), R.zero_frag(z_np[order]))
        back_q, back_s, back_z = torch.empty_like(packed), torch.empty_like(s), torch.empty_like(z)
        W4Z.w4zp_frag_to_rows(qf, sf, zf, back_q, back_s, back_z, N, K)
        assert np.array_equal(back_q.cpu().numpy(), R.pack(u_np[order]))
        assert np.array_equal(_bits(back_s), s_np[order])
        assert np.array_equal(back_z.cpu().numpy(), z_np[order])


def test_dequant_frag_every_code_zero_point_and_position(dev):
    """Row n has zero point n % 16 and, at column k, the code (k + n // 16) % 16: over the 256 rows every one of the 128 column
    positions of a unit (every nibble of every word of every k-tile) meets all 16 codes under all 16 zero points."""
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import w4zp_ops as W4Z
    from ssd_amd.quant import dequantize_w4zp, pack_w4u
    N, K = 256, 256
    n, k = torch.arange(N, device=dev)[:, None], torch.arange(K, device=dev)[None, :]
    u = ((k + n // 16) % 16).to(torch.uint8)
    z = (n % 16).to(torch.uint8).expand(N, K // 128).contiguous()
    g = torch.Generator(device=dev).manual_seed(2)
    s = (torch.rand(N, K // 128, generator=g, device=dev) * 6e-3 + 2e-3).to(BF)
    seen = {(int(a), int(b), int(c)) for a, b, c in zip(u[:, :128].cpu().flatten(), z[:, :1].expand(N, 128).cpu().flatten(),
                                                         k[:, :128].expand(N, 128).cpu().flatten())}
    assert len(seen) == 16 * 16 * 128
    packed = pack_w4u(u)
    qf, sf, zf = _frag(packed, s, z, N, K, dev)
    wf = torch.empty(N * K, dtype=BF, device=dev)
    W4Z.w4zp_dequant_frag(qf, sf, zf, wf, N, K)
    rows = torch.empty(N, K, dtype=BF, device=dev)
    H.frag_to_rows(wf, rows, N, K)
    assert np.array_equal(_bits(rows), R.dequant(u.cpu().numpy(), _bits(s), z.cpu().numpy()))
    assert torch.equal(rows.view(torch.int16), dequantize_w4zp(packed, s, z).view(torch.int16))
    assert torch.equal(rows.cpu().view(torch.int16), dequantize_w4zp(packed.cpu(), s.cpu(), z.cpu()).view(torch.int16))


def _check_rows(dev, M, N, K, bias_on, what, seed=0, cfg=None, zero=None, also_symmetric=False):
    from ssd_amd.hip import w4zp_ops as W4Z
    u, s, z, packed = _codes(N, K, dev, seed, zero=zero)
    qf, sf, zf = _frag(packed, s, z, N, K, dev)
    x, xf = _x(M, K, dev, seed + 1)
    bias = (torch.randn(N, device=dev) * 0.1).to(BF) if bias_on else None
    y = torch.empty(M, N, dtype=BF, device=dev)
    W4Z.gemm_w4a16_zp(xf, qf, sf, zf, y, M, N, K, N, bias=bias, cfg=cfg)
    want = x.double() @ _exact(u, s, z).T
    if bias is not None:
        want = want + bias.double()
    assert_within_ulp(y, want, what)
    if also_symmetric:
        from ssd_amd.hip import w4_ops as W4
        y2 = torch.empty(M, N, dtype=BF, device=dev)
        W4.gemm_w4a16(xf, qf, sf, y2, M, N, K, N, bias=bias, cfg=cfg)
        assert_within_ulp(y2, want, what + " (symmetric kernel)")
        # at z = 8 the factor (z - 8) / 136 is exactly 0 and t = fma(0, corr, p) = p: the symmetric kernel's value, bit for bit
        assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), f"{what}: differs in bits from the symmetric kernel's output"


def _check_silu(dev, M, I, K, what, seed=0):
    from ssd_amd.quant import gate_up_row_map
    from ssd_amd.hip import w4zp_ops as W4Z
    from ssd_amd.hip import ops as H
    u, s, z, packed = _codes(2 * I, K, dev, seed)
    qf, sf, zf = _frag(packed, s, z, 2 * I, K, dev, gate_up_row_map(2 * I).to(dev))
    x, xf = _x(M, K, dev, seed + 1)
    yf = torch.zeros(H.frag_numel(M, I), dtype=BF, device=dev)
    W4Z.gemm_w4a16_zp(xf, qf, sf, zf, yf, M, 2 * I, K, 0, epilogue=H.EPI_SILU_FRAG)
    y = torch.empty(M, I, dtype=BF, device=dev)
    H.frag_to_rows(yf, y, M, I)
    yg = x.double() @ _exact(u, s, z).T
    g, up = yg[:, :I].to(BF).double(), yg[:, I:].to(BF).double()
    sg = torch.sigmoid(g)
    want = g * sg * up
    # the bar of tests/test_hip_w4a16.py::_check_silu
    slack = (up * sg * (1 + g * (1 - sg))).abs() * bf16_ulp(g) + (g * sg).abs() * bf16_ulp(up)
    floor = want.pow(2).mean().sqrt() * 2 ** -6
    tol = 3.0 * bf16_ulp(torch.maximum(want.to(BF).double().abs(), floor)) + slack
    d = (y.double() - want.to(BF).double()).abs()
    bad = d > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} outputs beyond the bar, worst {(d / tol).max().item():.2f} x tol"


@pytest.mark.parametrize("M", [1, 7, 8, 24, 32, 64, 128])
@pytest.mark.parametrize("model", list(SHAPES))
def test_gemm_w4a16_zp_within_one_ulp_of_f64(dev, model, M):
    m = SHAPES[model]
    for i, (kind, (N, K)) in enumerate(mats(m).items()):
        if kind == "gate_up":
            _check_silu(dev, M, m["I"], K, f"{model} gate_up silu M={M}", seed=i)
            _check_rows(dev, M, N, K, bias_on=False, what=f"{model} gate_up rows M={M}", seed=i)
        else:
            _check_rows(dev, M, N, K, bias_on=(i + M) % 2 == 0, what=f"{model} {kind} M={M}", seed=i)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("M", [1, 8, 24, 64, 128])
def test_zero_point_eight_everywhere_matches_the_symmetric_kernel(dev, M):
    """z = 8 is the symmetric format: both kernels meet the same bar on the same codes and scales (8B o_proj and 1B down_proj)."""
    for N, K in ((4096, 4096), (2048, 8192)):
        _check_rows(dev, M, N, K, bias_on=M % 2 == 0, what=f"z=8 [{N}, {K}] M={M}", seed=M, zero=8, also_symmetric=True)


def test_every_explicit_decomposition_computes_the_same_function(dev):
    N, K = 2048, 2048
    for b in (False, True):
        for nt in (1, 2, 4, 1 | 256, 2 | 256, 4 | 256):
            for waves in (1, 4, 8, 8 | (2 << 8)):
                _check_rows(dev, 8, N, K, b, f"cfg nt {nt} waves {waves} bias {b}", seed=5, cfg=(nt, waves))
    for M in (24, 64, 128):
        for nt in (1, 2):
            for waves in (1, 2, 4):
                _check_rows(dev, M, N, K, True, f"M={M} cfg nt {nt} waves {waves}", seed=6, cfg=(nt, waves))


def test_repeats_bit_identical_and_hipgraph_replay_equals_eager(dev):
    from ssd_amd.hip import w4zp_ops as W4Z
    from ssd_amd.hip import ops as H
    from ssd_amd.quant import gate_up_row_map
    N, K, M, I = 8192, 8192, 8, 4096
    u, s, z, packed = _codes(N, K, dev, 21)
    qf, sf, zf = _frag(packed, s, z, N, K, dev)
    u2, s2, z2, packed2 = _codes(2 * I, K, dev, 23)
    qf2, sf2, zf2 = _frag(packed2, s2, z2, 2 * I, K, dev, gate_up_row_map(2 * I).to(dev))
    x, xf = _x(M, K, dev, 22)
    y_e, y_g = torch.empty(M, N, dtype=BF, device=dev), torch.empty(M, N, dtype=BF, device=dev)
    a_e, a_g = (torch.zeros(H.frag_numel(M, I), dtype=BF, device=dev) for _ in range(2))
    W4Z.gemm_w4a16_zp(xf, qf, sf, zf, y_e, M, N, K, N)
    W4Z.gemm_w4a16_zp(xf, qf2, sf2, zf2, a_e, M, 2 * I, K, 0, epilogue=H.EPI_SILU_FRAG)
    for _ in range(3):
        y_r = torch.empty_like(y_e)
        W4Z.gemm_w4a16_zp(xf, qf, sf, zf, y_r, M, N, K, N)
        assert torch.equal(y_r.view(torch.int16), y_e.view(torch.int16))
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):         # warm-up on the capture stream
        W4Z.gemm_w4a16_zp(xf, qf, sf, zf, y_g, M, N, K, N)
    st.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        W4Z.gemm_w4a16_zp(xf, qf, sf, zf, y_g, M, N, K, N)
        W4Z.gemm_w4a16_zp(xf, qf2, sf2, zf2, a_g, M, 2 * I, K, 0, epilogue=H.EPI_SILU_FRAG)
    y_g.zero_()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_g.view(torch.int16), y_e.view(torch.int16))
    assert torch.equal(a_g.view(torch.int16), a_e.view(torch.int16))
