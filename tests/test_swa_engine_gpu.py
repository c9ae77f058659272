"""Sliding-window models through the decoder and the engine on the GPU: the tiny Llama with sliding_window = 24 and the tiny Qwen3 with
layer_windows alternating 24 / 0 (block size 16), against tests/swa_ref.py's float64 forward to the bar tests/test_model_gpu.py holds the
tiny models to (max |delta logit| <= 0.05, mean <= 0.01); the full-attention forward lies outside that bar once the context exceeds
the window, so the window is on.  Greedy streams: eager against hipGraphs, synchronous speculation against autoregressive."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import swa_ref
from tests.test_kv8_engine_gpu import _golden_model
from tests.test_model_gpu import COMMON, gpu, hip_factory, i32, i64, slots  # noqa: F401  (gpu is the fixture)
from tests.util import assert_stream_matches, seq_margins

W = 24
TOKENS = [(37 * i + 11) % 512 for i in range(54)]         # 40 prefilled, 6 decoded one by one, 8 verified in one forward


def windowed(golden, name):
    cfg, w, _, _ = _golden_model(golden, name)
    return (dataclasses.replace(cfg, sliding_window=W) if name == "tiny_llama" else dataclasses.replace(cfg, sliding_window=W, layer_windows=(W, 0))), w


@pytest.mark.parametrize("name", ["tiny_llama", "tiny_qwen3"])
def test_logits_of_prefill_decode_and_verify_against_float64(gpu, golden, name):
    from ssd_amd.hip import ops as H
    from ssd_amd.model import HipDecoder, AttnMeta
    cfg, w = windowed(golden, name)
    dec = HipDecoder(cfg, max_tokens=64, max_seqs=1, max_blocks=5, block_size=16, max_model_len=512, device=gpu)
    dec.load_weights(iter({k: v for k, v in w.items() if not (cfg.tie_word_embeddings and k == "lm_head.weight")}.items()))
    dec.alloc_kv(6)
    table = [4, 2, 0, 5, 1]
    bt = i32(table).view(1, -1)
    rows = []
    for lo, hi in [(0, 40)] + [(p, p + 1) for p in range(40, 46)] + [(46, 54)]:
        n = hi - lo
        kw = dict(cu_q=i32([0, n])) if lo == 0 else dict(q_per_seq=n)
        dec.forward(i64(TOKENS[lo:hi]), i64(range(lo, hi)), n, AttnMeta(H.MODE_CAUSAL, 1, n, slots(table, range(lo, hi)), i32([hi]), bt, **kw))
        rows.append(dec.logits[:dec.compute_logits(n)].double().cpu())
    got = torch.cat(rows)
    ref = swa_ref.forward(cfg, w, TOKENS)
    full = swa_ref.forward(dataclasses.replace(cfg, sliding_window=0, layer_windows=()), w, TOKENS)
    d, d_full = (got - ref).abs(), (got - full).abs()
    print(f"{name}: |HIP - float64 windowed| max {d.max():.4f} mean {d.mean():.4f}; against the full-attention forward, rows past the "
          f"window: max {d_full[W:].max():.4f} mean {d_full[W:].mean():.4f}")
    assert torch.isfinite(got).all()
    assert d.max() <= 0.05 and d.mean() <= 0.01
    assert d_full[:W].max() <= 0.05 and d_full[W:].max() > 0.05, "the window is not on"
    assert dec.swa and not (dec.chain_seg or dec.tree_seg or dec.fuse_attn_o)


def stream(golden, margins=None, **kw):
    """24 greedy tokens after the 40-token prompt from one engine on the windowed tiny Llama (also its own draft)."""
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    cfg, w = windowed(golden, "tiny_llama")
    factory = hip_factory(w, w)
    factory.supports_swa = True
    if kw.get("speculate"):
        kw.update(draft="d", draft_hf_config=cfg, speculate_k=3)
    eng = LLMEngine("t", hf_config=cfg, runner_factory=factory, **COMMON, **kw)
    if margins is not None:
        eng.model_runner.margin_log = {}
    out, _ = eng.generate([TOKENS[:40]], SamplingParams(temperature=0, max_new_tokens=24, ignore_eos=True), use_tqdm=False)
    if margins is not None:
        margins.update(seq_margins(eng.model_runner.margin_log, 0))
    eng.exit()
    return out[0]["token_ids"]


def test_greedy_streams_eager_graphs_and_synchronous_speculation(gpu, golden, monkeypatch):
    from ssd_amd.hip import ops as H

    def refuse(*a, **k):
        raise AssertionError("a windowed model took a route that runs attention inside another kernel")
    for name in ("attn_oproj_parts", "chain_segment", "tree_segment"):
        monkeypatch.setattr(H, name, refuse)
    margins = {}
    ar = stream(golden, margins=margins, enforce_eager=True)
    assert len(ar) == 24 and stream(golden) == ar
    sync = stream(golden, speculate=True)
    assert stream(golden, speculate=True, enforce_eager=True) == sync
    assert_stream_matches(sync, ar, margins, 40, "synchronous speculation against autoregressive")
    kv8 = stream(golden, kv_cache_dtype="fp8")
    assert len(kv8) == 24 and stream(golden, kv_cache_dtype="fp8", enforce_eager=True) == kv8
