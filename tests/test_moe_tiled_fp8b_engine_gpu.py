"""A block-scaled FP8 Qwen3-MoE target prefills prompts of HipDecoder.MOE_TILED_FP8B_MIN_T rows and more on ssd_moe_gemm_tiled_fp8b: the
tiny pair of tests/test_moe_fp8b_engine_gpu.py, one prompt, once as shipped and once with the threshold out of reach, each at that
file's bar against float64 truth over the dequantized weights (each run with its own routes forced)."""
import pytest

from tests.test_moe_engine_gpu import _assert_forced_route_bar, _hip_rows
from tests.test_moe_fp8b_engine_gpu import _pair, gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def test_long_prefill_runs_the_tiled_fp8b_expert_gemm(gpu, monkeypatch):
    from ssd_amd.hip import moe_ops
    from ssd_amd.model import HipDecoder
    cfg, host, deq, _, _ = _pair()
    T = HipDecoder.MOE_TILED_FP8B_MIN_T + 44
    tokens = [(53 * i + 7) % 512 for i in range(T)]
    calls = []
    real = moe_ops.moe_gemm_tiled_fp8b
    monkeypatch.setattr(moe_ops, "moe_gemm_tiled_fp8b", lambda *a, **k: (calls.append(a[6]), real(*a, **k))[1])
    nblocks = -(-T // 16) + 2
    dec = HipDecoder(cfg, max_tokens=T + 20, max_seqs=1, max_blocks=nblocks, block_size=16, max_model_len=T + 36, device=gpu,
                     quantization="fp8")
    dec.load_weights(iter(host.items()))
    dec.alloc_kv(nblocks)
    assert dec.moe and dec.fp8
    for name, min_t in (("shipped", HipDecoder.MOE_TILED_FP8B_MIN_T), ("patched out", T + 1)):
        monkeypatch.setattr(HipDecoder, "MOE_TILED_FP8B_MIN_T", min_t)
        del calls[:]
        got, rl, ids = _hip_rows(dec, tokens, [T], gpu)
        assert calls == ([T] * 2 * cfg.num_layers if name == "shipped" else []), f"{name}: tiled fp8b launches {calls}"
        _assert_forced_route_bar(cfg, deq, tokens, got, rl, ids, f"tiny fp8 MoE prefill {T}, {name}")
