"""An FP8 (e4m3 weight-only) target end to end on the MI355X: model logits against float64 arithmetic on the exact dequantized weights
(bar: rms|HIP - f64| <= 1.25 rms|oracle - f64| + 1e-3 over all logits, same argmax outside near-ties, the oracle being the unmodified CPU oracle given bf16(s*q) weights), greedy
engine streams in lock step with the oracle engine on those weights (sync and async speculation, batching + prefix caching), the
weight bytes of the 70B target, and the default (quantization=None) path left as it was."""
import dataclasses
import random

import pytest
import torch

from tests import fp8_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def dequantized(w: dict) -> dict:
    """The weights an fp8 target computes with: every decoder linear as bf16(s * q) of its own quantization (same math on any device)."""
    from ssd_amd.quant import is_quantized_linear
    out = {}
    for n, t in w.items():
        if is_quantized_linear(n):
            q, s = fp8_ref.quantize(t.to("cuda"))
            t = fp8_ref.dequant(q, s).cpu()
        out[n] = t
    return out


def _logits_vs_truth(cfg, w, prompt, n_verify, gpu, what):
    """HIP fp8 decoder: prefill of the prompt, then one verify forward of n_verify rows; oracle (bf16(s*q) weights) and float64 truth
    over the whole sequence; the rows of both forwards are held to the rms bar."""
    from oracle.model import OracleModel, Ctx
    from ssd_amd.hip import ops as H
    from ssd_amd.model import HipDecoder, AttnMeta
    from tests.util import truth_forward
    wq = dequantized(w)
    seq = list(prompt)
    P, T = len(prompt) - n_verify, len(prompt)
    bs = 16
    nblocks = -(-T // bs) + 1
    dec = HipDecoder(cfg, max_tokens=max(T, 64), max_seqs=1, max_blocks=nblocks, block_size=bs, max_model_len=max(512, T + 16),
                     device=gpu, quantization="fp8")
    ws = dict(w)
    if cfg.tie_word_embeddings:
        ws.pop("lm_head.weight", None)
    dec.load_weights(iter(ws.items()))
    dec.alloc_kv(nblocks)
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
    wo = {k: v for k, v in wq.items() if not (cfg.tie_word_embeddings and k == "lm_head.weight")}
    orc = OracleModel(cfg, wo, nblocks, bs)
    cu = torch.tensor([0, T], dtype=torch.int32)
    ref_h = orc.forward(torch.tensor(seq), torch.arange(T), Ctx("prefill", slot_mapping=torch.tensor([table[p // bs] * bs + p % bs for p in range(T)], dtype=torch.int32), cu_q=cu, cu_k=cu))
    ref_h = ref_h[0] if isinstance(ref_h, tuple) else ref_h
    ref = orc.compute_logits(ref_h).double()
    truth = truth_forward(cfg, wo, seq)
    rms = lambda e: e.pow(2).mean(-1).sqrt()
    e_hip, e_ref = (got - truth).abs(), (ref - truth).abs()
    print(f"{what}: |HIP-f64| rms {rms(e_hip).mean():.5f} max {e_hip.max():.4f} | |oracle-f64| rms {rms(e_ref).mean():.5f} "
          f"max {e_ref.max():.4f}")
    assert torch.isfinite(got).all()
    # the bar over all logits of the two forwards (per row, a 512-entry vocabulary is too few samples: two independent bf16 pipelines
    # trade places row by row)
    r_hip, r_ref = e_hip.pow(2).mean().sqrt().item(), e_ref.pow(2).mean().sqrt().item()
    assert r_hip <= 1.25 * r_ref + 1e-3, f"{what}: rms |HIP - f64| {r_hip:.5f} > 1.25 x {r_ref:.5f} + 1e-3"
    top2 = ref.topk(2, dim=-1).values
    thr = torch.clamp(2 * (got - ref).abs().max(-1).values, min=0.0625)
    assert bool(((got.argmax(-1) == ref.argmax(-1)) | ((top2[:, 0] - top2[:, 1]) < thr)).all()), f"{what}: argmax differs beyond a near-tie"
    return dec


def test_tiny_llama_fp8_logits(gpu, golden):
    from tests.test_model_gpu import mk_cfg
    g = golden("tiny_llama")
    cfg = mk_cfg(g, "llama")
    w = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    prompt = g["prompt"].tolist() + g["verify_tokens"].tolist()
    dec = _logits_vs_truth(cfg, w, prompt, len(g["verify_tokens"]), gpu, "tiny llama fp8")
    assert dec.fp8 and dec.w["model.layers.0.mlp.down_proj.weight"].dtype == torch.uint8
    assert not (dec.chain_seg or dec.tree_seg or dec.use_parts or dec.pf_parts or dec.fuse_attn_o)


def test_tiny_qwen3_fp8_logits(gpu, golden):
    from tests.test_model_gpu import mk_cfg
    g = golden("tiny_qwen3")
    cfg = mk_cfg(g, "qwen3", tie=True, qk_norm=True)
    w = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    prompt = g["prompt"].tolist() + g["verify_tokens"].tolist()
    _logits_vs_truth(cfg, w, prompt, len(g["verify_tokens"]), gpu, "tiny qwen3 fp8")


def test_two_layer_70b_cut_fp8_logits(gpu):
    """A 160-token prompt (> 128 rows: the dequantize + bf16 prefill route) then an 8-row verify (the fp8 GEMM), 70B layer shapes."""
    from ssd_amd import weights as W
    from ssd_amd.model_config import PRESETS
    cfg = dataclasses.replace(PRESETS["llama-3.1-70b"], num_layers=2, vocab_size=16384)
    w = W.synthetic_state_dict(cfg, seed=4, std=0.02)
    random.seed(3)
    prompt = [random.randint(0, cfg.vocab_size - 1) for _ in range(168)]
    _logits_vs_truth(cfg, w, prompt, 8, gpu, "70B x 2 layers fp8")


# ---------------------------------------------------------------------------------------------------------------------
# engine streams
# ---------------------------------------------------------------------------------------------------------------------
def _factory(w):
    from ssd_amd.engine.llm_engine import hip_runner_factory

    def f(config, model_cfg, *, is_draft, topo, **kw):
        return hip_runner_factory(config, model_cfg, is_draft=is_draft, topo=topo, weight_source=iter(w[is_draft].items()), **kw)
    return f


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_fp8_target_engine_lockstep_with_oracle(gpu, golden, mode):
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    from ssd_amd.utils.topology import Topology
    from tests.lockstep import compare_lockstep
    from tests.test_model_gpu import mk_cfg, weights
    g = golden("engine_golden")
    wt, wd = weights(g, "t."), weights(g, "d.")
    kw = dict(hf_config=mk_cfg(g, "llama", "t_"), draft="d", draft_hf_config=mk_cfg(g, "llama", "d_"), speculate=True,
              max_model_len=512, max_num_batched_tokens=512, kvcache_block_size=16, num_kvcache_blocks=64, num_draft_kvcache_blocks=64)
    if mode == "async":
        kw.update(speculate_k=3, draft_async=True, async_fan_out=2, jit_speculate=True)
    else:
        kw.update(speculate_k=int(g["sd_K"]))
    gpu_eng = LLMEngine("t", runner_factory=_factory({False: wt, True: wd}), inprocess_draft=mode == "async", quantization="fp8", **kw)
    assert gpu_eng.model_runner.model.fp8
    cpu_eng = LLMEngine("t", runner_factory=oracle_runner_factory(dequantized(wt), wd), inprocess_draft=mode == "async",
                        topology=Topology(0, 1, torch.device("cpu"), "target", 0, 1), **kw)
    rep = compare_lockstep(gpu_eng, cpu_eng, g["prompt"].tolist(), 24,
                           lambda n: SamplingParams(temperature=0, max_new_tokens=n, ignore_eos=True),
                           fan_out=2 if mode == "async" else None, what=f"fp8 target {mode}")
    gpu_eng.exit()
    print(f"fp8 target {mode}: {rep.summary()}")
    assert rep.tokens == 24 and rep.tokens_compared >= 0.8 * rep.tokens, rep.summary()


def test_fp8_target_batch_prefix_cache_and_temperature(gpu):
    """b > 1 with shared prefixes and preemption against the oracle engine on bf16(s*q) weights; then a temperature > 0 run
    completes with in-vocabulary tokens."""
    from oracle.runner import oracle_runner_factory
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
    eng = LLMEngine("t", runner_factory=_factory({False: wt, True: wd}), quantization="fp8", **kw)
    gpu_out, _ = eng.generate(prompts, sp, use_tqdm=False)
    cpu_eng = LLMEngine("t", runner_factory=oracle_runner_factory(dequantized(wt), wd), **kw)
    cpu_out, _ = cpu_eng.generate(prompts, sp, use_tqdm=False)
    for i, (a, b) in enumerate(zip(gpu_out, cpu_out)):
        n = assert_stream_matches(a["token_ids"], b["token_ids"], seq_margins(cpu_eng.model_runner.margin_log, i), len(prompts[i]),
                                  what=f"fp8 batch/prefix seq {i}")
        print("fp8 batch/prefix: identical tokens", n, "of", len(b["token_ids"]))
    out, _ = eng.generate(prompts[:2], SamplingParams(temperature=0.8, max_new_tokens=10, ignore_eos=True), use_tqdm=False)
    assert all(len(o["token_ids"]) == 10 and all(0 <= x < 512 for x in o["token_ids"]) for o in out)


def test_70b_fp8_weight_bytes_at_most_052_of_bf16(gpu):
    """Every matrix of the full 80-layer 70B target (zero-valued: the byte count does not depend on the values)."""
    from ssd_amd import weights as W
    from ssd_amd.model import HipDecoder
    from ssd_amd.model_config import PRESETS
    cfg = PRESETS["llama-3.1-70b"]
    shapes = W.param_shapes(cfg)
    bf16_bytes = sum(2 * torch.Size(s).numel() for n, s in shapes if n != "model.embed_tokens.weight")
    dec = HipDecoder(cfg, max_tokens=16, max_seqs=1, max_blocks=2, block_size=256, max_model_len=512, device=gpu, quantization="fp8")
    dec.load_weights((n, torch.zeros(s, dtype=BF, device=gpu)) for n, s in shapes)
    fp8_bytes = dec.weight_bytes()
    print(f"70B weight bytes: bf16 {bf16_bytes / 1e9:.2f} GB, fp8 {fp8_bytes / 1e9:.2f} GB ({fp8_bytes / bf16_bytes:.4f})")
    assert fp8_bytes <= 0.52 * bf16_bytes
    del dec
    torch.cuda.empty_cache()


def test_default_quantization_none_keeps_todays_stream(gpu, golden):
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    from tests.test_model_gpu import mk_cfg, weights, COMMON
    g = golden("engine_golden")
    wt, wd = weights(g, "t."), weights(g, "d.")
    kw = dict(hf_config=mk_cfg(g, "llama", "t_"), draft="d", draft_hf_config=mk_cfg(g, "llama", "d_"), speculate=True,
              speculate_k=int(g["sd_K"]), **COMMON)
    want = g["sd_diff_tokens"].tolist()
    sp = SamplingParams(temperature=0, max_new_tokens=len(want), ignore_eos=True)
    outs = []
    for extra in ({}, {"quantization": None}):
        eng = LLMEngine("t", runner_factory=_factory({False: wt, True: wd}), **extra, **kw)
        assert not eng.model_runner.model.fp8 and eng.model_runner.model.w["model.layers.0.mlp.down_proj.weight"].dtype == BF
        outs.append(eng.generate([g["prompt"].tolist()], sp, use_tqdm=False)[0][0]["token_ids"])
    assert outs[0] == outs[1]
    from tests.util import common_prefix
    n = common_prefix(outs[0], want)
    ref_lens = [(row >= 0).sum().item() for row in g["sd_diff_suffix"]]
    if n < len(want):
        acc, step = 0, 0
        while acc + ref_lens[step] <= n:
            acc += ref_lens[step]
            step += 1
        assert g["sd_diff_margins"].tolist()[step] < 0.0625, f"diverged in step {step}"
