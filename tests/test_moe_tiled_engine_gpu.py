"""A bf16 Qwen3-MoE target prefills prompts of HipDecoder.MOE_TILED_MIN_T rows and more on ssd_moe_gemm_tiled: the tiny pair of
tests/test_moe_engine_gpu.py, one prompt, once as shipped and once with the threshold out of reach, each at that file's bar against
float64 truth over all logits, the last row's among them (each run with its own routes forced)."""
import pytest

from tests.test_moe_engine_gpu import _assert_forced_route_bar, _decoder, _hip_rows, _pair, gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def test_long_prefill_runs_the_tiled_expert_gemm(gpu, monkeypatch):
    from ssd_amd.hip import moe_ops
    from ssd_amd.model import HipDecoder
    cfg, w, _, _ = _pair()
    T = HipDecoder.MOE_TILED_MIN_T + 44
    assert HipDecoder.MOE_TILED_MIN_T >= 256
    tokens = [(53 * i + 7) % 512 for i in range(T)]
    calls = []
    real = moe_ops.moe_gemm_tiled
    monkeypatch.setattr(moe_ops, "moe_gemm_tiled", lambda *a, **k: (calls.append(a[5]), real(*a, **k))[1])
    dec = _decoder(cfg, w, gpu, T + 20, -(-T // 16) + 2)
    for name, min_t in (("shipped", HipDecoder.MOE_TILED_MIN_T), ("patched out", T + 1)):
        monkeypatch.setattr(HipDecoder, "MOE_TILED_MIN_T", min_t)
        del calls[:]
        got, rl, ids = _hip_rows(dec, tokens, [T], gpu)
        assert calls == ([T] * 2 * cfg.num_layers if name == "shipped" else []), f"{name}: tiled launches {calls}"
        _assert_forced_route_bar(cfg, w, tokens, got, rl, ids, f"tiny MoE prefill {T}, {name}")
