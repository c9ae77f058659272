"""FP8 weight kernels on the MI355X (csrc/gemm_fp8.hip): the quantizer + re-tiling against the torch restatement (tests/fp8_ref.py),
bit for bit, in the packed row orders; the layout round trip; the fp8 GEMM against float64 arithmetic on the exact dequantized
weights; the long-prompt route (dequantize + the bf16 prefill GEMM); hipGraph replay.

Bar for the GEMM: |HIP - bf16(f64)| <= 1 bf16 ulp of the reference value, the ulp taken at no less than 2^-6 of the output's rms
(an output that cancels to nearly zero carries the fp32 accumulation's absolute error, which no bf16 ulp of a tiny value bounds)."""
import math

import pytest
import torch

from tests import fp8_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
# (N, K) of qkv, o, gate_up, down
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
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} outputs beyond {ulps} ulp, worst {(d / tol).max().item():.2f} x tol"


@pytest.mark.parametrize("model", list(SHAPES))
def test_quantizer_and_retile_bit_equal_in_packed_orders(dev, model):
    from ssd_amd.quant import quantize_fp8, qkv_row_map, gate_up_row_map
    from ssd_amd.hip import quant_ops as Q
    m = SHAPES[model]
    g = torch.Generator(device=dev).manual_seed(11)
    for kind, (N, K) in mats(m).items():
        w = (torch.randn(N, K, generator=g, device=dev) * 0.02).to(BF)
        w[3] = 0
        q, s = quantize_fp8(w)
        q_ref, s_ref = fp8_ref.quantize(w)
        assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8)) and torch.equal(s, s_ref), (model, kind)
        if kind == "qkv":
            order, rmap = fp8_ref.qkv_order(m["nh"], m["nkv"], m["hd"]), qkv_row_map(m["nh"], m["nkv"], m["hd"]).to(dev)
        elif kind == "gate_up":
            order, rmap = fp8_ref.gate_up_order(N), gate_up_row_map(N).to(dev)
        else:
            order, rmap = list(range(N)), None
        out = torch.empty(N * K, dtype=torch.uint8, device=dev)
        Q.fp8_rows_to_frag(q.view(torch.uint8), out, N, K, row_map=rmap)
        want = fp8_ref.to_frag(q_ref[torch.tensor(order, device=dev)])
        assert torch.equal(out, want), (model, kind)
        del w, q, s, q_ref, s_ref, out, want
    torch.cuda.empty_cache()


def test_fragment_round_trip_and_dequant(dev):
    from ssd_amd.hip import quant_ops as Q
    from ssd_amd.hip import ops as H
    N, K = 384, 1088
    codes = torch.randint(0, 256, (N, K), dtype=torch.uint8, device=dev)
    codes[(codes & 0x7f) == 0x7f] = 0                    # no NaN codes (the quantizer saturates: it never emits one)
    frag = torch.empty(N * K, dtype=torch.uint8, device=dev)
    back = torch.empty_like(codes)
    Q.fp8_rows_to_frag(codes, frag, N, K)
    Q.fp8_frag_to_rows(frag, back, N, K)
    assert torch.equal(back, codes)
    assert torch.equal(frag, fp8_ref.to_frag(codes))
    s = torch.rand(N, device=dev) * 1e-2 + 1e-4
    wf = torch.empty(N * K, dtype=BF, device=dev)
    Q.fp8_dequant_frag(frag, s, wf, N, K)
    rows = torch.empty(N, K, dtype=BF, device=dev)
    H.frag_to_rows(wf, rows, N, K)
    want = fp8_ref.dequant(codes.view(torch.float8_e4m3fn), s)
    assert torch.equal(rows.view(torch.int16), want.view(torch.int16))


def _quantized(N, K, dev, seed, rmap=None):
    from ssd_amd.quant import quantize_fp8
    from ssd_amd.hip import quant_ops as Q
    g = torch.Generator(device=dev).manual_seed(seed)
    q, s = quantize_fp8((torch.randn(N, K, generator=g, device=dev) * 0.02).to(BF))
    frag = torch.empty(N * K, dtype=torch.uint8, device=dev)
    Q.fp8_rows_to_frag(q.view(torch.uint8), frag, N, K, row_map=rmap)
    s_packed = s if rmap is None else s[rmap.long()].contiguous()
    return q, s, frag, s_packed


def _x(M, K, dev, seed):
    from ssd_amd.hip import ops as H
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(M, K, generator=g, device=dev).to(BF)
    xf = torch.zeros(H.frag_numel(M, K), dtype=BF, device=dev)
    H.rows_to_frag(x, xf, M, K)
    return x, xf


def _check_rows(dev, M, N, K, bias_on, what, seed=0):
    from ssd_amd.hip import quant_ops as Q
    q, s, frag, sp = _quantized(N, K, dev, seed)
    x, xf = _x(M, K, dev, seed + 1)
    bias = (torch.randn(N, device=dev) * 0.1).to(BF) if bias_on else None
    y = torch.empty(M, N, dtype=BF, device=dev)
    Q.gemm_fp8(xf, frag, sp, y, M, N, K, N, bias=bias)
    want = x.double() @ (q.double() * s.double()[:, None]).T
    if bias is not None:
        want = want + bias.double()
    assert_within_ulp(y, want, what)


def _silu_ref(x, q, s, I):
    yg = (x.double() @ (q.double() * s.double()[:, None]).T)
    g, u = yg[:, :I].to(BF).float(), yg[:, I:].to(BF).float()
    return (g / (1 + torch.exp(-g))) * u


def _check_silu(dev, M, I, K, what, seed=0):
    from ssd_amd.quant import gate_up_row_map
    from ssd_amd.hip import quant_ops as Q
    from ssd_amd.hip import ops as H
    rmap = gate_up_row_map(2 * I).to(dev)
    q, s, frag, sp = _quantized(2 * I, K, dev, seed, rmap)
    x, xf = _x(M, K, dev, seed + 1)
    yf = torch.zeros(H.frag_numel(M, I), dtype=BF, device=dev)
    Q.gemm_fp8(xf, frag, sp, yf, M, 2 * I, K, 0, epilogue=H.EPI_SILU_FRAG)
    y = torch.empty(M, I, dtype=BF, device=dev)
    H.frag_to_rows(yf, y, M, I)
    want = _silu_ref(x, q, s, I)
    # gate and up are each within 1 ulp before the product; silu(g)*u then moves by up to ~2 ulp of its own value
    assert_within_ulp(y, want.double(), what, ulps=3.0)


@pytest.mark.parametrize("M", [1, 7, 8, 24, 32])
@pytest.mark.parametrize("model", ["1b", "8b", "70b"])
def test_gemm_fp8_rows_within_one_ulp_of_f64(dev, model, M):
    for i, (kind, (N, K)) in enumerate(mats(SHAPES[model]).items()):
        _check_rows(dev, M, N, K, bias_on=(i + M) % 2 == 0, what=f"{model} {kind} M={M}", seed=i)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("M", [1, 8, 32])
@pytest.mark.parametrize("model", ["1b", "8b", "70b"])
def test_gemm_fp8_silu_epilogue(dev, model, M):
    m = SHAPES[model]
    _check_silu(dev, M, m["I"], m["h"], f"{model} gate_up silu M={M}")


def test_gemm_fp8_bias_both_ways_and_explicit_configs(dev):
    """Every decomposition the _cfg form accepts computes the same function (1B o_proj, M = 8, with and without bias)."""
    from ssd_amd.hip import quant_ops as Q
    N, K, M = 2048, 2048, 8
    q, s, frag, sp = _quantized(N, K, dev, 5)
    x, xf = _x(M, K, dev, 6)
    bias = (torch.randn(N, device=dev) * 0.1).to(BF)
    for b in (None, bias):
        want = x.double() @ (q.double() * s.double()[:, None]).T + (0 if b is None else b.double())
        for nt in (1, 2, 4, 1 | 256, 2 | 256, 4 | 256):
            for waves in (1, 4, 8, 8 | (2 << 8)):
                y = torch.empty(M, N, dtype=BF, device=dev)
                Q.gemm_fp8(xf, frag, sp, y, M, N, K, N, bias=b, cfg=(nt, waves))
                assert_within_ulp(y, want, f"cfg nt {nt} waves {waves} bias {b is not None}")


@pytest.mark.parametrize("M", [64, 128])
def test_prefill_chunks_on_the_fp8_gemm(dev, M):
    m = SHAPES["70b"]
    for i, (kind, (N, K)) in enumerate(mats(m).items()):
        if kind == "gate_up":
            _check_silu(dev, M, m["I"], m["h"], f"70b gate_up silu M={M}", seed=i)
        else:
            _check_rows(dev, M, N, K, bias_on=False, what=f"70b {kind} M={M}", seed=i)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("M", [900, 2048])
def test_long_prompt_route_dequant_then_bf16_prefill_gemm(dev, M):
    """M > 128: bf16(s*q) into a scratch, then ssd_gemm_pf -- the bf16-weight bound (1 ulp of f64 on the dequantized weights)."""
    from ssd_amd.hip import quant_ops as Q
    from ssd_amd.hip import ops as H
    for N, K in ((8192, 8192), (8192, 28672)):
        q, s, frag, sp = _quantized(N, K, dev, 9)
        x, xf = _x(M, K, dev, 10)
        wdq = torch.empty(N * K, dtype=BF, device=dev)
        Q.fp8_dequant_frag(frag, sp, wdq, N, K)
        ws = torch.empty(max(H.gemm_pf_workspace_bytes(M, N, K) // 4, 1), dtype=torch.float32, device=dev)
        y = torch.empty(M, N, dtype=BF, device=dev)
        H.gemm_pf(xf, wdq, y, M, N, K, N, ws)
        want = x.double() @ fp8_ref.dequant(q, s).double().T
        assert_within_ulp(y, want, f"long prompt {N}x{K} M={M}")
        del q, s, frag, wdq, ws
    torch.cuda.empty_cache()


def test_hipgraph_replay_is_bit_equal_to_eager(dev):
    from ssd_amd.hip import quant_ops as Q
    from ssd_amd.hip import ops as H
    N, K, M = 8192, 8192, 8
    q, s, frag, sp = _quantized(N, K, dev, 21)
    x, xf = _x(M, K, dev, 22)
    y_e, y_g = torch.empty(M, N, dtype=BF, device=dev), torch.empty(M, N, dtype=BF, device=dev)
    I = 4096
    from ssd_amd.quant import gate_up_row_map
    rmap = gate_up_row_map(2 * I).to(dev)
    _, _, frag2, sp2 = _quantized(2 * I, K, dev, 23, rmap)
    a_e, a_g = (torch.zeros(H.frag_numel(M, I), dtype=BF, device=dev) for _ in range(2))
    Q.gemm_fp8(xf, frag, sp, y_e, M, N, K, N)
    Q.gemm_fp8(xf, frag2, sp2, a_e, M, 2 * I, K, 0, epilogue=H.EPI_SILU_FRAG)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):         # warm-up on the capture stream
        Q.gemm_fp8(xf, frag, sp, y_g, M, N, K, N)
    st.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        Q.gemm_fp8(xf, frag, sp, y_g, M, N, K, N)
        Q.gemm_fp8(xf, frag2, sp2, a_g, M, 2 * I, K, 0, epilogue=H.EPI_SILU_FRAG)
    y_g.zero_()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_g.view(torch.int16), y_e.view(torch.int16))
    assert torch.equal(a_g.view(torch.int16), a_e.view(torch.int16))
