"""A target with an FP8 (e4m3) KV cache end to end on the MI355X: model logits against float64 arithmetic over what the cache holds
(bar: rms|HIP - truth_kv8| <= 1.25 rms|Kv8Oracle - truth_kv8| + 1e-3 over all logits, same argmax outside near-ties -- an element that
rounds to the neighbouring e4m3 code costs the oracle against the truth exactly as it costs HIP, so the bar calibrates itself), greedy
engine streams in lock step with an oracle engine whose target model sees k / v through the same cache (sync and async speculation,
batching + prefix caching + preemption), the blocks that fit, and the default (kv_cache_dtype=None) path left as it was."""
import dataclasses
import gc
import random

import pytest
import torch

from tests import kv8_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
_SHARED = {}
MEASURED = {}          # what the logits tests of this file measured at run time: max |HIP - Kv8Oracle| over their rows


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def pow2_scales(L, nkv):
    """Non-trivial powers of two, different per layer, K / V and head."""
    vals = [0.5, 2.0, 0.25, 4.0]
    k = torch.tensor([[vals[(li + h) % 4] for h in range(nkv)] for li in range(L)])
    v = torch.tensor([[vals[(li + h + 2) % 4] for h in range(nkv)] for li in range(L)])
    return k, v


def _logits_vs_truth(cfg, w, prompt, n_verify, gpu, what, scales=None, quantization=None):
    """HIP decoder with an fp8 KV cache: prefill of the prompt, then one verify forward of n_verify rows; Kv8OracleModel and the float64
    truth over the whole sequence; the rows of both forwards are held to the rms bar.  Prints the four figures."""
    from oracle.model import Ctx
    from ssd_amd.hip import ops as H
    from ssd_amd.model import HipDecoder, AttnMeta
    w_orc, w_truth = w, w
    if quantization == "w4a16":
        from tests.test_w4a16_engine_gpu import quantized
        w_orc, w_truth = quantized(w)
    seq = list(prompt)
    P, T = len(prompt) - n_verify, len(prompt)
    bs = 16
    nblocks = -(-T // bs) + 1
    qkw = {"quantization": quantization} if quantization else {}
    dec = HipDecoder(cfg, max_tokens=max(T, 64), max_seqs=1, max_blocks=nblocks, block_size=bs, max_model_len=max(512, T + 16),
                     device=gpu, kv_cache_dtype="fp8", **qkw)
    ws = dict(w)
    if cfg.tie_word_embeddings:
        ws.pop("lm_head.weight", None)
    dec.load_weights(iter(ws.items()))
    dec.alloc_kv(nblocks)
    assert dec.kv_cache.dtype == torch.uint8
    ks, vs = scales if scales is not None else (None, None)
    if scales is not None:
        dec.set_kv_scales(ks, vs)
    table = list(range(nblocks))
    bt = torch.tensor([table], dtype=torch.int32, device=gpu)
    sl = lambda ps: torch.tensor([table[p // bs] * bs + p % bs for p in ps], dtype=torch.int32, device=gpu)
    i64 = lambda x: torch.tensor(list(x), dtype=torch.int64, device=gpu)
    i32 = lambda x: torch.tensor(list(x), dtype=torch.int32, device=gpu)
    dec.forward(i64(seq[:P]), i64(range(P)), P, AttnMeta(H.MODE_CAUSAL, 1, P, sl(range(P)), i32([P]), bt, cu_q=i32([0, P])))
    n = dec.compute_logits(P)
    got_p = dec.logits[:n].double().cpu()
    dec.forward(i64(seq[P:]), i64(range(P, T)), n_verify,
                AttnMeta(H.MODE_CAUSAL, 1, n_verify, sl(range(P, T)), i32([T]), bt, q_per_seq=n_verify))
    n = dec.compute_logits(n_verify)
    got = torch.cat([got_p, dec.logits[:n].double().cpu()])
    strip = lambda d: {k: v for k, v in d.items() if not (cfg.tie_word_embeddings and k == "lm_head.weight")}
    orc = kv8_ref.Kv8OracleModel(cfg, strip(w_orc), nblocks, bs)
    orc.set_kv_scales(ks, vs)
    cu = torch.tensor([0, T], dtype=torch.int32)
    ref_h = orc.forward(torch.tensor(seq), torch.arange(T),
                        Ctx("prefill", slot_mapping=torch.tensor([table[p // bs] * bs + p % bs for p in range(T)], dtype=torch.int32), cu_q=cu, cu_k=cu))
    ref_h = ref_h[0] if isinstance(ref_h, tuple) else ref_h
    ref = orc.compute_logits(ref_h).double()
    truth = kv8_ref.truth_forward_kv8(cfg, strip(w_truth), seq, ks, vs)
    e_hip, e_ref = (got - truth).abs(), (ref - truth).abs()
    r_hip, r_ref = e_hip.pow(2).mean().sqrt().item(), e_ref.pow(2).mean().sqrt().item()
    d_max = (got - ref).abs().max().item()
    print(f"{what}: rms|HIP-truth_kv8| {r_hip:.5f} (max {e_hip.max():.4f}) | rms|Kv8Oracle-truth_kv8| {r_ref:.5f} (max {e_ref.max():.4f}) | "
          f"max|HIP-Kv8Oracle| {d_max:.4f} | near-tie thr {max(0.0625, 2 * d_max):.4f}")
    assert torch.isfinite(got).all()
    assert r_hip <= 1.25 * r_ref + 1e-3, f"{what}: rms |HIP - truth_kv8| {r_hip:.5f} > 1.25 x {r_ref:.5f} + 1e-3"
    top2 = ref.topk(2, dim=-1).values
    thr = max(0.0625, 2 * d_max)
    assert bool(((got.argmax(-1) == ref.argmax(-1)) | ((top2[:, 0] - top2[:, 1]) < thr)).all()), f"{what}: argmax differs beyond a near-tie"
    MEASURED[what] = d_max
    return dec


def _golden_model(golden, name):
    from tests.test_model_gpu import mk_cfg
    g = golden(name)
    cfg = mk_cfg(g, "qwen3", tie=True, qk_norm=True) if name == "tiny_qwen3" else mk_cfg(g, "llama")
    w = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    return cfg, w, g["prompt"].tolist() + g["verify_tokens"].tolist(), len(g["verify_tokens"])


@pytest.mark.parametrize("scales", ["one", "pow2"])
def test_tiny_llama_kv8_logits(gpu, golden, scales):
    cfg, w, prompt, nv = _golden_model(golden, "tiny_llama")
    sc = pow2_scales(cfg.num_layers, cfg.num_kv_heads) if scales == "pow2" else None
    dec = _logits_vs_truth(cfg, w, prompt, nv, gpu, f"tiny llama kv8 scales {scales}", scales=sc)
    # every form that writes or reads KV inside another kernel is off; what does not touch KV stays
    assert dec.kv8 and not dec.quantized
    assert not (dec.chain_seg or dec.tree_seg or dec.fuse_attn_o)
    assert all(dec.fusion_plan(T) == (False, False) for T in (1, 8, 16, 24))
    from ssd_amd.model import HipDecoder
    plain = HipDecoder(cfg, max_tokens=64, max_seqs=1, max_blocks=4, block_size=16, max_model_len=512, device=gpu)
    assert dec.use_parts == plain.use_parts and dec.pf_parts == plain.pf_parts


@pytest.mark.parametrize("scales", ["one", "pow2"])
def test_tiny_qwen3_kv8_logits(gpu, golden, scales):
    cfg, w, prompt, nv = _golden_model(golden, "tiny_qwen3")
    sc = pow2_scales(cfg.num_layers, cfg.num_kv_heads) if scales == "pow2" else None
    _logits_vs_truth(cfg, w, prompt, nv, gpu, f"tiny qwen3 kv8 scales {scales}", scales=sc)


def test_tiny_llama_kv8_with_w4a16_weights_logits(gpu, golden):
    cfg, w, prompt, nv = _golden_model(golden, "tiny_llama")
    dec = _logits_vs_truth(cfg, w, prompt, nv, gpu, "tiny llama kv8 + w4a16", quantization="w4a16")
    assert dec.kv8 and dec.w4


@pytest.mark.parametrize("scales", ["one", "pow2"])
def test_two_layer_70b_cut_kv8_logits(gpu, scales):
    """A 168-token prompt (one long-prefill launch per linear, varlen attention over the freshly stored codes) then an 8-row verify."""
    from ssd_amd import weights as W
    from ssd_amd.model_config import PRESETS
    cfg = dataclasses.replace(PRESETS["llama-3.1-70b"], num_layers=2, vocab_size=16384)
    if "w70" not in _SHARED:          # generated once for both runs, never modified
        _SHARED["w70"] = W.synthetic_state_dict(cfg, seed=4, std=0.02)
    w = _SHARED["w70"]
    random.seed(3)
    prompt = [random.randint(0, cfg.vocab_size - 1) for _ in range(168)]
    sc = pow2_scales(cfg.num_layers, cfg.num_kv_heads) if scales == "pow2" else None
    _logits_vs_truth(cfg, w, prompt, 8, gpu, f"70B x 2 layers kv8 scales {scales}", scales=sc)


# ---------------------------------------------------------------------------------------------------------------------
# engine streams
# ---------------------------------------------------------------------------------------------------------------------
def _factory(w):
    from ssd_amd.engine.llm_engine import hip_runner_factory

    def f(config, model_cfg, *, is_draft, topo, **kw):
        return hip_runner_factory(config, model_cfg, is_draft=is_draft, topo=topo, weight_source=iter(w[is_draft].items()), **kw)
    return f


def _kv8_oracle_engine(wt, wd, **kw):
    """The oracle engine with its TARGET runner's model turned into a Kv8OracleModel (the instance is patched; the draft stays plain)."""
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    eng = LLMEngine("t", runner_factory=oracle_runner_factory(wt, wd), **kw)
    kv8_ref.as_kv8_oracle(eng.model_runner.model)
    return eng


def _engine_thr(gpu, golden):
    """The near-tie threshold of the lock-step comparison: twice what the logits test of this file measured between HIP and the
    Kv8Oracle on the engine_golden target at run time (measured here if that test has not run in this process), floored at 0.0625."""
    what = "engine_golden target kv8"
    if what not in MEASURED:
        from tests.test_model_gpu import mk_cfg, weights
        g = golden("engine_golden")
        prompt = g["prompt"].tolist()
        _logits_vs_truth(mk_cfg(g, "llama", "t_"), weights(g, "t."), prompt + g["sd_diff_tokens"].tolist()[:8], 8, gpu, what)
    return max(0.0625, 2 * MEASURED[what])


def test_engine_golden_target_kv8_logits(gpu, golden):
    thr = _engine_thr(gpu, golden)
    print(f"lock-step near-tie threshold from the measured logits difference: {thr:.4f}")
    assert thr >= 0.0625


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_kv8_target_engine_lockstep_with_oracle(gpu, golden, mode):
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    from ssd_amd.utils.topology import Topology
    from tests.lockstep import compare_lockstep
    from tests.test_model_gpu import mk_cfg, weights
    g = golden("engine_golden")
    wt, wd = weights(g, "t."), weights(g, "d.")
    thr = _engine_thr(gpu, golden)
    kw = dict(hf_config=mk_cfg(g, "llama", "t_"), draft="d", draft_hf_config=mk_cfg(g, "llama", "d_"), speculate=True,
              max_model_len=512, max_num_batched_tokens=512, kvcache_block_size=16, num_kvcache_blocks=64, num_draft_kvcache_blocks=64)
    if mode == "async":
        kw.update(speculate_k=3, draft_async=True, async_fan_out=2, jit_speculate=True)
    else:
        kw.update(speculate_k=int(g["sd_K"]))
    gpu_eng = LLMEngine("t", runner_factory=_factory({False: wt, True: wd}), inprocess_draft=mode == "async", kv_cache_dtype="fp8", **kw)
    assert gpu_eng.model_runner.model.kv8 and gpu_eng.model_runner.model.kv_cache.dtype == torch.uint8
    cpu_eng = _kv8_oracle_engine(wt, wd, inprocess_draft=mode == "async", topology=Topology(0, 1, torch.device("cpu"), "target", 0, 1), **kw)
    rep = compare_lockstep(gpu_eng, cpu_eng, g["prompt"].tolist(), 24,
                           lambda n: SamplingParams(temperature=0, max_new_tokens=n, ignore_eos=True),
                           fan_out=2 if mode == "async" else None, thr=thr, what=f"kv8 target {mode}")
    gpu_eng.exit()
    print(f"kv8 target {mode} (thr {thr:.4f}): {rep.summary()}")
    assert rep.tokens == 24 and rep.tokens_compared >= 0.8 * rep.tokens, rep.summary()


def test_kv8_target_batch_prefix_cache_and_temperature(gpu):
    """b > 1 with shared prefixes and preemption against the oracle engine whose target sees k / v through the fp8 cache; then a
    temperature > 0 run completes with in-vocabulary tokens."""
    from ssd_amd import weights as W
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.model_config import ModelConfig
    from ssd_amd.sampling_params import SamplingParams
    from tests.util import assert_stream_matches, seq_margins
    t = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 512, 1e-5, 5e5, 1024, False)
    d = ModelConfig("llama", 128, 1, 2, 1, 64, 256, 512, 1e-5, 5e5, 1024, True)
    wt = W.synthetic_state_dict(t, seed=0, std=0.1)
    wd = W.synthetic_state_dict(d, seed=1, std=0.1)
    wd.pop("lm_head.weight", None)
    shared = [(7 * j + 3) % 512 for j in range(40)]
    prompts = [shared + [(11 * i + j) % 512 for j in range(5 + 3 * i)] for i in range(4)]
    kw = dict(hf_config=t, draft="d", draft_hf_config=d, speculate=True, speculate_k=3, max_num_seqs=3, max_model_len=256,
              max_num_batched_tokens=256, kvcache_block_size=16, num_kvcache_blocks=16, num_draft_kvcache_blocks=16)
    sp = SamplingParams(temperature=0, max_new_tokens=14, ignore_eos=True)
    eng = LLMEngine("t", runner_factory=_factory({False: wt, True: wd}), kv_cache_dtype="fp8", **kw)
    assert eng.model_runner.model.kv8
    gpu_out, _ = eng.generate(prompts, sp, use_tqdm=False)
    cpu_eng = _kv8_oracle_engine(wt, wd, **kw)
    cpu_out, _ = cpu_eng.generate(prompts, sp, use_tqdm=False)
    for i, (a, b) in enumerate(zip(gpu_out, cpu_out)):
        n = assert_stream_matches(a["token_ids"], b["token_ids"], seq_margins(cpu_eng.model_runner.margin_log, i), len(prompts[i]),
                                  what=f"kv8 batch/prefix seq {i}")
        print("kv8 batch/prefix: identical tokens", n, "of", len(b["token_ids"]))
    out, _ = eng.generate(prompts[:2], SamplingParams(temperature=0.8, max_new_tokens=10, ignore_eos=True), use_tqdm=False)
    assert all(len(o["token_ids"]) == 10 and all(0 <= x < 512 for x in o["token_ids"]) for o in out)


# ---------------------------------------------------------------------------------------------------------------------
# capacity and the default path
# ---------------------------------------------------------------------------------------------------------------------
def test_auto_sized_cache_holds_at_least_19_tenths_of_the_bf16_blocks(gpu):
    from ssd_amd import weights as W
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.model_config import ModelConfig
    t = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 512, 1e-5, 5e5, 1024, False)
    wt = W.synthetic_state_dict(t, seed=0, std=0.1)
    kw = dict(hf_config=t, max_model_len=256, max_num_batched_tokens=256, kvcache_block_size=256, gpu_memory_utilization=0.01)
    blocks = {}
    for dt in (None, "fp8"):
        eng = LLMEngine("t", runner_factory=_factory({False: wt}), kv_cache_dtype=dt, **kw)
        blocks[dt] = eng.model_runner.num_kvcache_blocks
        assert eng.model_runner.model.kv_cache.shape[2] == blocks[dt]
        eng.exit()
        del eng
        gc.collect()
        torch.cuda.empty_cache()
    print(f"auto-sized KV blocks at the same utilisation: bf16 {blocks[None]}, fp8 {blocks['fp8']} ({blocks['fp8'] / blocks[None]:.3f}x)")
    assert blocks["fp8"] >= 1.9 * blocks[None]


def test_default_kv_cache_dtype_keeps_todays_stream(gpu, golden):
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    from tests.test_model_gpu import mk_cfg, weights, COMMON
    from tests.util import common_prefix
    g = golden("engine_golden")
    wt, wd = weights(g, "t."), weights(g, "d.")
    kw = dict(hf_config=mk_cfg(g, "llama", "t_"), draft="d", draft_hf_config=mk_cfg(g, "llama", "d_"), speculate=True,
              speculate_k=int(g["sd_K"]), **COMMON)
    want = g["sd_diff_tokens"].tolist()
    sp = SamplingParams(temperature=0, max_new_tokens=len(want), ignore_eos=True)
    outs = []
    for extra in ({}, {"kv_cache_dtype": None}):
        eng = LLMEngine("t", runner_factory=_factory({False: wt, True: wd}), **extra, **kw)
        assert not eng.model_runner.model.kv8 and eng.model_runner.model.kv_cache.dtype == BF
        outs.append(eng.generate([g["prompt"].tolist()], sp, use_tqdm=False)[0][0]["token_ids"])
    assert outs[0] == outs[1]
    n = common_prefix(outs[0], want)
    ref_lens = [(row >= 0).sum().item() for row in g["sd_diff_suffix"]]
    if n < len(want):
        acc, step = 0, 0
        while acc + ref_lens[step] <= n:
            acc += ref_lens[step]
            step += 1
        assert g["sd_diff_margins"].tolist()[step] < 0.0625, f"diverged in step {step}"
