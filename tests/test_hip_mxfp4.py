"""MXFP4 weight kernels on the MI355X (csrc/gemm_mxfp4.hip): the re-tiling against the numpy restatement (tests/mxfp4_ref.py), bit
for bit, with and without row maps, and back; the dequantize kernel bit-equal to the host dequantization for every code, scale byte,
nibble and k-tile position (this pins the conversion instruction's nibble order and scale handling); the quantizer on the device
equal to the CPU run; the GEMM against float64 arithmetic on the exact weights; every explicit decomposition; repeat determinism;
hipGraph replay.

Bar for the GEMM (that of tests/test_hip_w4a16.py): |HIP - bf16(f64)| <= 1 bf16 ulp of the reference value, the ulp taken at no less
than 2^-6 of the output's rms; SILU_FRAG 3 ulp plus the first-order effect of one ulp in gate and in up."""
import numpy as np
import pytest
import torch

from tests import mxfp4_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SHAPES = {
    "1b": dict(nh=32, nkv=8, hd=64, h=2048, I=8192),
    "8b": dict(nh=32, nkv=8, hd=128, h=4096, I=14336),
    "70b": dict(nh=64, nkv=8, hd=128, h=8192, I=28672),
    "qwen3-32b": dict(nh=64, nkv=8, hd=128, h=5120, I=25600),
}


def mats(m):
    qkv = (m["nh"] + 2 * m["nkv"]) * m["hd"]
    return {"qkv": (qkv, m["h"]), "o": (m["h"], m["nh"] * m["hd"]), "gate_up": (2 * m["I"], m["h"]), "down": (m["h"], m["I"])}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    a = x.abs().clamp_min(1e-30)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def assert_within_ulp(got: torch.Tensor, want64: torch.Tensor, what: str, ulps: float = 1.0):
    want = want64.to(BF).double()
    floor = want64.pow(2).mean().sqrt() * 2 ** -6
    tol = ulps * bf16_ulp(torch.maximum(want.abs(), floor))
    d = (got.double() - want).abs()
    bad = d > tol
    print(f"{what}: worst {(d / tol).max().item():.2f} x tol")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} outputs beyond {ulps} ulp, worst {(d / tol).max().item():.2f} x tol"
    return (d / tol).max().item()


def _codes(N, K, dev, seed):
    """Codes uniform over all 16 values, scale bytes uniform in 117..123 (the magnitude of 0.02-std weights), in the host form."""
    g = torch.Generator(device=dev).manual_seed(seed)
    packed = torch.randint(0, 256, (N, K // 2), generator=g, device=dev, dtype=torch.uint8)
    s = torch.randint(117, 124, (N, K // 32), generator=g, device=dev, dtype=torch.uint8)
    return packed, s


def _frag(packed, s, N, K, dev, rmap=None):
    from ssd_amd.hip import mx4_ops as MX4
    qf = torch.empty(N * K // 2, dtype=torch.uint8, device=dev)
    sf = torch.empty(N * K // 32, dtype=torch.uint8, device=dev)
    MX4.mx4_rows_to_frag(packed, s, qf, sf, N, K, row_map=rmap)
    return qf, sf


def _exact(packed, s):
    """f64 2^(b - 127) * e2m1(q) [N, K], on the device, from the definition (not through ssd_amd.quant)."""
    dev = packed.device
    mags = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6], dtype=torch.float64, device=dev)
    p = packed.to(torch.int64)
    c = torch.stack((p & 15, p >> 4), dim=-1).reshape(packed.shape[0], -1)
    v = mags[c & 7] * torch.where((c & 8) != 0, -1.0, 1.0).double()
    return v * torch.exp2(s.double() - 127).repeat_interleave(32, dim=1)


def test_rows_to_frag_round_trip_bit_exact_with_and_without_row_maps(dev):
    from ssd_amd.quant import qkv_row_map, gate_up_row_map
    from ssd_amd.hip import mx4_ops as MX4
    N, K = 384, 1152
    packed, s = _codes(N, K, dev, 1)
    p_np, s_np = packed.cpu().numpy(), s.cpu().numpy()
    for rmap in (None, gate_up_row_map(N), qkv_row_map(4, 1, 64)):
        order = np.arange(N) if rmap is None else rmap.numpy().astype(np.int64)
        qf, sf = _frag(packed, s, N, K, dev, None if rmap is None else rmap.to(dev))
        assert np.array_equal(qf.cpu().numpy().view(np.uint32), R.to_frag(p_np[order]))
        assert np.array_equal(sf.cpu().numpy(), R.scale_frag(s_np[order]))
        back_q, back_s = torch.empty_like(packed), torch.empty_like(s)
        MX4.mx4_frag_to_rows(qf, sf, back_q, back_s, N, K)
        assert np.array_equal(back_q.cpu().numpy(), p_np[order])
        assert np.array_equal(back_s.cpu().numpy(), s_np[order])


def test_dequant_frag_bit_equal_to_host_for_every_code_scale_nibble_and_ktile(dev):
    """[16 rows][128 columns] = one device unit per scale setting: row r carries code r in every even column (low nibbles) and all 16
    codes in the odd columns (high nibbles) of every 32-column block, so every code sits in both nibble positions of every k-tile; the
    four k-tiles of the unit carry four different scale bytes; stacking 63 such units covers every b in 2..252."""
    from ssd_amd.hip import ops as H
    from ssd_amd.hip import mx4_ops as MX4
    from ssd_amd.quant import dequantize_mxfp4, pack_mxfp4
    codes = torch.zeros(16, 128, dtype=torch.uint8)
    codes[:, 0::2] = torch.arange(16, dtype=torch.uint8)[:, None]
    codes[:, 1::2] = (torch.arange(64) % 16).to(torch.uint8)[None, :]
    b0s = list(range(2, 253, 4))
    packed = pack_mxfp4(codes).repeat(len(b0s), 1).to(dev)                       # [16 * 63, 64]
    s = torch.tensor([[min(b0 + (j + r) % 4, 252) for j in range(4)] for b0 in b0s for r in range(16)], dtype=torch.uint8, device=dev)
    assert set(s.flatten().tolist()) == set(range(2, 253))
    N, K = packed.shape[0], 128
    qf, sf = _frag(packed, s, N, K, dev)
    wf = torch.empty(N * K, dtype=BF, device=dev)
    MX4.mx4_dequant_frag(qf, sf, wf, N, K)
    rows = torch.empty(N, K, dtype=BF, device=dev)
    H.frag_to_rows(wf, rows, N, K)
    got = rows.cpu().view(torch.int16).numpy().view(np.uint16)
    want = R.bf16_bits_exact(R.exact(R.unpack(packed.cpu().numpy()), s.cpu().numpy()))
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} weights differ"
    assert torch.equal(rows.view(torch.int16), dequantize_mxfp4(packed, s).view(torch.int16))


def test_quantizer_on_the_device_equals_the_cpu_run(dev):
    from ssd_amd.quant import quantize_mxfp4
    g = torch.Generator().manual_seed(9)
    w = (torch.randn(256, 1024, generator=g) * 0.02).to(BF)
    w[3, 64:96] = 0
    a, b = quantize_mxfp4(w), quantize_mxfp4(w.to(dev))
    assert torch.equal(a.packed, b.packed.cpu()) and torch.equal(a.scale, b.scale.cpu())
    c_ref, b_ref = R.quantize(w)
    assert np.array_equal(b.packed.cpu().numpy(), R.pack(c_ref)) and np.array_equal(b.scale.cpu().numpy(), b_ref)


def _x(M, K, dev, seed):
    from ssd_amd.hip import ops as H
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(M, K, generator=g, device=dev).to(BF)
    xf = torch.zeros(H.frag_numel(M, K), dtype=BF, device=dev)
    H.rows_to_frag(x, xf, M, K)
    return x, xf


def _check_rows(dev, M, N, K, bias_on, what, seed=0, cfg=None):
    from ssd_amd.hip import mx4_ops as MX4
    packed, s = _codes(N, K, dev, seed)
    qf, sf = _frag(packed, s, N, K, dev)
    x, xf = _x(M, K, dev, seed + 1)
    bias = (torch.randn(N, device=dev) * 0.1).to(BF) if bias_on else None
    y = torch.empty(M, N, dtype=BF, device=dev)
    MX4.gemm_mxfp4(xf, qf, sf, y, M, N, K, N, bias=bias, cfg=cfg)
    want = x.double() @ _exact(packed, s).T
    if bias is not None:
        want = want + bias.double()
    assert_within_ulp(y, want, what)


def assert_silu_within_bar(y: torch.Tensor, yg: torch.Tensor, I: int, what: str):
    """The SILU_FRAG bar: y bf16 [M, I] from the kernel against yg = the f64 [M, 2I] (gate | up) sums before any rounding."""
    g, u = yg[:, :I].to(BF).double(), yg[:, I:].to(BF).double()
    sg = torch.sigmoid(g)
    want = g * sg * u
    # gate and up are each within 1 ulp of their bf16(f64) (the ROWS bar); silu(g) * u carries that ulp through its partial
    # derivatives (large for very negative g, where silu(g) ~ g e^g), plus 3 ulp of its own value for the product and the rounding
    slack = (u * sg * (1 + g * (1 - sg))).abs() * bf16_ulp(g) + (g * sg).abs() * bf16_ulp(u)
    floor = want.pow(2).mean().sqrt() * 2 ** -6
    tol = 3.0 * bf16_ulp(torch.maximum(want.to(BF).double().abs(), floor)) + slack
    d = (y.double() - want.to(BF).double()).abs()
    bad = d > tol
    print(f"{what}: worst {(d / tol).max().item():.2f} x tol")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} outputs beyond the bar, worst {(d / tol).max().item():.2f} x tol"
    return (d / tol).max().item()


def _check_silu(dev, M, I, K, what, seed=0):
    from ssd_amd.quant import gate_up_row_map
    from ssd_amd.hip import mx4_ops as MX4
    from ssd_amd.hip import ops as H
    packed, s = _codes(2 * I, K, dev, seed)
    qf, sf = _frag(packed, s, 2 * I, K, dev, gate_up_row_map(2 * I).to(dev))
    x, xf = _x(M, K, dev, seed + 1)
    yf = torch.zeros(H.frag_numel(M, I), dtype=BF, device=dev)
    MX4.gemm_mxfp4(xf, qf, sf, yf, M, 2 * I, K, 0, epilogue=H.EPI_SILU_FRAG)
    y = torch.empty(M, I, dtype=BF, device=dev)
    H.frag_to_rows(yf, y, M, I)
    assert_silu_within_bar(y, x.double() @ _exact(packed, s).T, I, what)


@pytest.mark.parametrize("M", [1, 7, 8, 24, 32, 64, 128])
@pytest.mark.parametrize("model", list(SHAPES))
def test_gemm_mxfp4_within_one_ulp_of_f64(dev, model, M):
    m = SHAPES[model]
    for i, (kind, (N, K)) in enumerate(mats(m).items()):
        if kind == "gate_up":
            _check_silu(dev, M, m["I"], K, f"{model} gate_up silu M={M}", seed=i)
            _check_rows(dev, M, N, K, bias_on=False, what=f"{model} gate_up rows M={M}", seed=i)
            _check_rows(dev, M, N, K, bias_on=True, what=f"{model} gate_up rows bias M={M}", seed=i)
        else:
            _check_rows(dev, M, N, K, bias_on=False, what=f"{model} {kind} M={M}", seed=i)
            _check_rows(dev, M, N, K, bias_on=True, what=f"{model} {kind} bias M={M}", seed=i)
    torch.cuda.empty_cache()


def test_every_explicit_decomposition_computes_the_same_function(dev):
    """1B o_proj at M = 8 with and without bias, every (nt, deep, waves, tpw) the _cfg form accepts at one token tile; and the two-
    and eight-tile forms at M = 24 / 128."""
    N, K = 2048, 2048
    for b in (False, True):
        for nt in (1, 2, 4, 1 | 256, 2 | 256, 4 | 256):
            for waves in (1, 4, 8, 8 | (2 << 8)):
                _check_rows(dev, 8, N, K, b, f"cfg nt {nt} waves {waves} bias {b}", seed=5, cfg=(nt, waves))
    for M in (24, 128):
        for nt in (1, 2):
            for waves in (1, 2, 4):
                _check_rows(dev, M, N, K, True, f"M={M} cfg nt {nt} waves {waves}", seed=6, cfg=(nt, waves))


def test_repeats_bit_identical_and_hipgraph_replay_equals_eager(dev):
    from ssd_amd.hip import mx4_ops as MX4
    from ssd_amd.hip import ops as H
    from ssd_amd.quant import gate_up_row_map
    N, K, M, I = 8192, 8192, 8, 4096
    packed, s = _codes(N, K, dev, 21)
    qf, sf = _frag(packed, s, N, K, dev)
    packed2, s2 = _codes(2 * I, K, dev, 23)
    qf2, sf2 = _frag(packed2, s2, 2 * I, K, dev, gate_up_row_map(2 * I).to(dev))
    x, xf = _x(M, K, dev, 22)
    y_e, y_g = torch.empty(M, N, dtype=BF, device=dev), torch.empty(M, N, dtype=BF, device=dev)
    a_e, a_g = (torch.zeros(H.frag_numel(M, I), dtype=BF, device=dev) for _ in range(2))
    MX4.gemm_mxfp4(xf, qf, sf, y_e, M, N, K, N)
    MX4.gemm_mxfp4(xf, qf2, sf2, a_e, M, 2 * I, K, 0, epilogue=H.EPI_SILU_FRAG)
    for _ in range(3):
        y_r = torch.empty_like(y_e)
        MX4.gemm_mxfp4(xf, qf, sf, y_r, M, N, K, N)
        assert torch.equal(y_r.view(torch.int16), y_e.view(torch.int16))
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):         # warm-up on the capture stream
        MX4.gemm_mxfp4(xf, qf, sf, y_g, M, N, K, N)
    st.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        MX4.gemm_mxfp4(xf, qf, sf, y_g, M, N, K, N)
        MX4.gemm_mxfp4(xf, qf2, sf2, a_g, M, 2 * I, K, 0, epilogue=H.EPI_SILU_FRAG)
    y_g.zero_()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_g.view(torch.int16), y_e.view(torch.int16))
    assert torch.equal(a_g.view(torch.int16), a_e.view(torch.int16))
