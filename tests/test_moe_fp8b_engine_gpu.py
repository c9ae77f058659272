"""A Qwen3-MoE target with block-scaled FP8 experts end to end on the MI355X, by the rules of tests/test_moe_mxfp4_engine_gpu.py:
logits against moe_ref.forward in float64 over the DEQUANTIZED weights with the decoder's own routes forced, equal greedy streams,
graph replays against eager runs, weight_bytes.  Pair: tiny_moe_config with moe_intermediate_size 128 and head_dim 64, router_gain 8,
and that file's dense draft.  Experts are quantized on the CPU with quantize_fp8_block, the attention linears with quantize_fp8; the
forced-route decoder takes those host forms bit for bit, the engines quantize the dequantized image on load.  SEED: on the CPU, every
k-th / (k+1)-th router margin of the bf16 pipeline over the weights the engines compute with is >= MIN_ULPS bf16 ulps
(12 for this seed over the prompt and 24 greedy tokens; the autoregressive trace on the GPU read 6)."""
import gc

import pytest
import torch

from tests import moe_ref as R
from tests.test_moe_engine_gpu import _hip_rows, _assert_forced_route_bar, _factory, PROMPT, ENGINE_KW, MIN_ULPS, GAIN, STD

pytestmark = pytest.mark.gpu

SEED = 175
_W = {}


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda", 0)


def _pair():
    """(target config, host forms, dequantized weights, draft config, draft weights): generated once, never modified."""
    if not _W:
        from ssd_amd import quant, weights as W
        from ssd_amd.model_config import ModelConfig
        t = R.tiny_moe_config(head_dim=64, moe_intermediate_size=128)
        d = ModelConfig("qwen3", 128, 2, 4, 2, 64, 256, 512, 1e-6, 1e6, 1024, True, True)
        host, deq = {}, {}
        for name, w in W.synthetic_state_dict(t, seed=SEED, std=STD, recipe={"router_gain": GAIN}).items():
            if name.endswith((W.MOE_GATE_UP, W.MOE_DOWN)):
                per = [quant.quantize_fp8_block(w[e]) for e in range(w.shape[0])]
                w = quant.FP8BTensor(torch.stack([p.codes for p in per]), torch.stack([p.rowscale for p in per]))
            elif quant.is_quantized_linear(name):
                w = quant.quantize_fp8(w)
            host[name], deq[name] = w, (w.dequantize() if quant.is_prequantized(w) else w)
        _W["pair"] = (t, host, deq, d, W.synthetic_state_dict(d, seed=SEED + 1, std=STD))
    return _W["pair"]


@pytest.mark.parametrize("chunks", [[24] + [1] * 6 + [8], [150]], ids=["prefill24_decode6_verify8", "prefill150"])
def test_forced_route_logits(gpu, chunks):
    from ssd_amd.model import HipDecoder
    cfg, host, deq, _, _ = _pair()
    T = sum(chunks)
    tokens = [(37 * i + 11) % 512 for i in range(T)]
    nblocks = -(-T // 16) + 1
    dec = HipDecoder(cfg, max_tokens=max(64, T + 10), max_seqs=1, max_blocks=nblocks, block_size=16, max_model_len=512, device=gpu,
                     quantization="fp8")
    dec.load_weights(iter(host.items()))
    dec.alloc_kv(nblocks)
    p = "model.layers.0.mlp.experts."
    assert dec.moe and dec.fp8 and all(dec.w[p + n].dtype == torch.uint8 and dec.w[p + n + "_bscale"].dtype == torch.float32
                                       for n in ("gate_up_proj", "down_proj"))
    assert dec.w["model.layers.0.mlp.gate.weight"].dtype == torch.bfloat16 and "model.layers.0.self_attn.o_proj.weight_scale" in dec.w
    got, rl, ids = _hip_rows(dec, tokens, chunks, gpu)
    _assert_forced_route_bar(cfg, deq, tokens, got, rl, ids, f"tiny fp8 MoE {chunks[:2]}..")


def _generate(mode, eager=False, trace=False, n=24):
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    t, _, deq, d, wd = _pair()
    kw = dict(ENGINE_KW, hf_config=t, runner_factory=_factory(deq, wd), enforce_eager=eager, quantization="fp8")
    if mode == "sync":
        kw.update(draft="d", draft_hf_config=d, speculate=True, speculate_k=3)
    eng = LLMEngine("moe", **kw)
    m = eng.model_runner.model
    assert m.moe and m.fp8
    eng.model_runner.margin_log = {}
    if trace:
        m.moe_trace = []
    out, _ = eng.generate([PROMPT], SamplingParams(temperature=0, max_new_tokens=n, ignore_eos=True), use_tqdm=False)
    res = dict(tokens=out[0]["token_ids"], margins=dict(eng.model_runner.margin_log), trace=m.moe_trace,
               graphs=sorted({k[0] for k in eng.model_runner.graphs}), weight_bytes=m.weight_bytes())
    eng.exit()
    del eng
    gc.collect()
    return res


@pytest.fixture(scope="module")
def ar_eager(gpu):
    return _generate("ar", eager=True, trace=True)


def test_streams_equal_and_graph_replays_give_the_eager_tokens(gpu, ar_eager):
    from tests.util import assert_stream_matches, seq_margins
    cfg = _pair()[0]
    k = cfg.num_experts_per_tok
    assert len(ar_eager["tokens"]) == 24
    worst = float("inf")
    for logits, ids in ar_eager["trace"]:
        assert torch.equal(R.topk_ids(logits, k), ids.long())
        margin, big = R.kth_margins(logits, k)
        worst = min(worst, float((margin / R.bf16_ulp(big)).min()))
    print(f"autoregressive trace: smallest k-th / (k+1)-th router margin {worst:.2f} bf16 ulps of the larger value")
    assert worst >= MIN_ULPS, f"input problem, not a product failure: a routing margin of {worst:.2f} ulps < {MIN_ULPS} (choose another SEED)"
    margins = seq_margins(ar_eager["margins"], 0)
    ar_graph, sync_eager, sync_graph = _generate("ar"), _generate("sync", eager=True), _generate("sync")
    for run in (ar_graph, sync_graph):
        assert any(g.startswith("decode") or g.startswith("verify") for g in run["graphs"]), run["graphs"]
    assert ar_graph["tokens"] == ar_eager["tokens"] and sync_graph["tokens"] == sync_eager["tokens"], "graph replays differ from the eager launches"
    assert_stream_matches(sync_graph["tokens"], ar_eager["tokens"], margins, len(PROMPT), what="fp8 MoE target sync vs autoregressive")


def test_weight_bytes_counts_codes_scales_and_the_bf16_remainder(gpu, ar_eager):
    c = _pair()[0]
    h, I, E, L, hd, V = c.hidden_size, c.moe_intermediate_size, c.num_experts, c.num_layers, c.head_dim, c.vocab_size
    qn, qkv_n = c.num_heads * hd, (c.num_heads + 2 * c.num_kv_heads) * hd
    experts = L * E * (2 * I * h + h * I)                                       # one code byte each + one fp32 scale per 16 x 128 of them
    attn = L * (qkv_n * h + h * qn)                                             # one code byte each + one fp32 scale per output row
    bf16 = L * (16 * h + 2 * h + 2 * hd) + h + V * h                            # router (padded to 16 rows), four norms; final norm, LM head
    assert ar_eager["weight_bytes"] == experts + 4 * experts // (16 * 128) + attn + 4 * L * (qkv_n + h) + 2 * bf16
