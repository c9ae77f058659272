"""A block-scaled FP8 checkpoint (128 x 128 weight_scale_inv) end to end on the MI355X: the tiny goldens' weights through
quantize_fp8_block, written as a checkpoint directory and read back by load_safetensors; model logits under the bars of
tests/test_fp8_engine_gpu.py (its helper, given these weights: rms|HIP - f64| <= 1.25 rms|oracle - f64| + 1e-3, same argmax outside
near-ties, the oracle being the unmodified CPU oracle on dequantize_fp8_block weights); a 130-row prompt on the dequantize route;
greedy engine streams in lock step with the oracle engine (sync and async); LLM(<directory>) with and without quantization="fp8";
the routing keys; and the default and per-row fp8 paths left as they were."""
import json
import os
import random

import pytest
import torch

from tests import test_fp8_engine_gpu as F
from tests.test_fp8_engine_gpu import gpu  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HF_PARTS = {"self_attn.qkv_proj": ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"),
            "mlp.gate_up_proj": ("mlp.gate_proj", "mlp.up_proj")}


def write_block_checkpoint(d, cfg, sd):
    """sd's decoder linears through quantize_fp8_block, q / k / v and gate / up each on its own block grid (HF names), written with
    fp32 weight_scale_inv tensors; norms, embedding and LM head stay bf16."""
    from safetensors.torch import save_file
    from ssd_amd.quant import is_quantized_linear, quantize_fp8_block
    hd, nh, nkv, I = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads, cfg.intermediate_size
    rows = {"self_attn.qkv_proj": (nh * hd, nkv * hd, nkv * hd), "mlp.gate_up_proj": (I, I)}
    tensors = {}
    for n, t in sd.items():
        if cfg.tie_word_embeddings and n == "lm_head.weight":
            continue
        if not is_quantized_linear(n):
            tensors[n] = t.to(BF).contiguous()
            continue
        base = n[:-len(".weight")]
        key = next((k for k in HF_PARTS if base.endswith(k)), None)
        parts, r0 = ([(base, 0, t.shape[0])] if key is None else []), 0
        for part, nr in zip(HF_PARTS.get(key, ()), rows.get(key, ())):
            parts.append((base[:-len(key)] + part, r0, r0 + nr))
            r0 += nr
        for name, a, b in parts:
            q = quantize_fp8_block(t[a:b].to(BF))
            tensors[name + ".weight"] = q.codes.contiguous()
            tensors[name + ".weight_scale_inv"] = q.rowscale[::128].contiguous()          # one row of scales per block row
    save_file(tensors, os.path.join(d, "model.safetensors"))
    qc = {"quant_method": "fp8", "fmt": "e4m3", "weight_block_size": [128, 128], "activation_scheme": "dynamic",
          "modules_to_not_convert": ["lm_head"]}
    hf = {"model_type": cfg.family, "hidden_size": cfg.hidden_size, "num_hidden_layers": cfg.num_layers, "num_attention_heads": nh,
          "num_key_value_heads": nkv, "head_dim": hd, "intermediate_size": I, "vocab_size": cfg.vocab_size,
          "tie_word_embeddings": cfg.tie_word_embeddings, "quantization_config": qc}
    json.dump(hf, open(os.path.join(d, "config.json"), "w"))


def loaded(d, cfg):
    """The directory as an fp8 target reads it: {name: bf16 tensor or FP8BTensor}."""
    from ssd_amd import weights as W
    assert W.checkpoint_quantization(d) == "fp8"
    return dict(W.load_safetensors(cfg, d, fp8=True))


def dequantized(w: dict) -> dict:
    """The weights a block-scaled fp8 target computes with: dequantize_fp8_block of every block-scaled linear."""
    from ssd_amd.quant import FP8BTensor, dequantize_fp8_block
    return {n: (dequantize_fp8_block(*t).cpu() if isinstance(t, FP8BTensor) else t) for n, t in w.items()}


def assert_block_routing(dec):
    """Every decoder linear holds a group table under _bscale and no per-row _scale."""
    from ssd_amd.quant import is_quantized_linear
    lin = [n for n in dec.w if is_quantized_linear(n)]
    assert len(lin) == 4 * dec.cfg.num_layers
    for n in lin:
        N = dec.w[n + "_bscale"].shape[0] * 16
        K = dec.w[n].numel() // N
        assert dec.w[n].dtype == torch.uint8 and n + "_scale" not in dec.w, n
        assert dec.w[n + "_bscale"].dtype == torch.float32 and tuple(dec.w[n + "_bscale"].shape) == (N // 16, -(-K // 128)), n
    assert dec.weight_bytes() >= sum(dec.w[n].numel() + 4 * dec.w[n + "_bscale"].numel() for n in lin)


def _logits(monkeypatch, cfg, sd, prompt, n_verify, gpu, tmp_path, what):
    """tests/test_fp8_engine_gpu._logits_vs_truth on the weights read back from the directory: the decoder is handed FP8BTensors
    (no re-quantization), the oracle and the f64 truth their dequantize_fp8_block."""
    write_block_checkpoint(str(tmp_path), cfg, sd)
    w = loaded(str(tmp_path), cfg)
    monkeypatch.setattr(F, "dequantized", dequantized)
    dec = F._logits_vs_truth(cfg, w, prompt, n_verify, gpu, what)
    assert dec.fp8
    assert_block_routing(dec)
    return dec


def test_tiny_llama_block_fp8_logits(gpu, golden, monkeypatch, tmp_path):
    from tests.test_model_gpu import mk_cfg
    g = golden("tiny_llama")
    cfg = mk_cfg(g, "llama")
    sd = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    prompt = g["prompt"].tolist() + g["verify_tokens"].tolist()
    _logits(monkeypatch, cfg, sd, prompt, len(g["verify_tokens"]), gpu, tmp_path, "tiny llama block fp8")


def test_tiny_qwen3_block_fp8_logits(gpu, golden, monkeypatch, tmp_path):
    from tests.test_model_gpu import mk_cfg
    g = golden("tiny_qwen3")
    cfg = mk_cfg(g, "qwen3", tie=True, qk_norm=True)
    sd = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    prompt = g["prompt"].tolist() + g["verify_tokens"].tolist()
    _logits(monkeypatch, cfg, sd, prompt, len(g["verify_tokens"]), gpu, tmp_path, "tiny qwen3 block fp8")


def test_130_row_prompt_takes_the_dequantize_route(gpu, golden, monkeypatch, tmp_path):
    from ssd_amd.model import HipDecoder
    from tests.test_model_gpu import mk_cfg
    g = golden("tiny_llama")
    cfg = mk_cfg(g, "llama")
    sd = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    random.seed(5)
    prompt = [random.randint(0, cfg.vocab_size - 1) for _ in range(130 + 8)]
    assert 130 > HipDecoder.FP8_DIRECT_MAX_T
    dec = _logits(monkeypatch, cfg, sd, prompt, 8, gpu, tmp_path, "130-row prompt block fp8")
    assert dec._deq is not None


def _factory(target_source, wd):
    from ssd_amd.engine.llm_engine import hip_runner_factory

    def f(config, model_cfg, *, is_draft, topo, **kw):
        src = iter(wd.items()) if is_draft else target_source()
        return hip_runner_factory(config, model_cfg, is_draft=is_draft, topo=topo, weight_source=src, **kw)
    return f


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_block_fp8_target_engine_lockstep_with_oracle(gpu, golden, mode, tmp_path):
    from oracle.runner import oracle_runner_factory
    from ssd_amd import weights as W
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    from ssd_amd.utils.topology import Topology
    from tests.lockstep import compare_lockstep
    from tests.test_model_gpu import mk_cfg, weights
    g = golden("engine_golden")
    wt, wd = weights(g, "t."), weights(g, "d.")
    cfg_t = mk_cfg(g, "llama", "t_")
    d = str(tmp_path)
    write_block_checkpoint(d, cfg_t, wt)
    kw = dict(hf_config=cfg_t, draft="d", draft_hf_config=mk_cfg(g, "llama", "d_"), speculate=True,
              max_model_len=512, max_num_batched_tokens=512, kvcache_block_size=16, num_kvcache_blocks=64, num_draft_kvcache_blocks=64)
    if mode == "async":
        kw.update(speculate_k=3, draft_async=True, async_fan_out=2, jit_speculate=True)
    else:
        kw.update(speculate_k=int(g["sd_K"]))
    source = lambda: W.load_safetensors(cfg_t, d, out_device=str(gpu), fp8=True)       # noqa: E731  (what the runner calls for a directory)
    gpu_eng = LLMEngine("t", runner_factory=_factory(source, wd), inprocess_draft=mode == "async", quantization="fp8", **kw)
    assert gpu_eng.model_runner.model.fp8
    assert_block_routing(gpu_eng.model_runner.model)
    cpu_eng = LLMEngine("t", runner_factory=oracle_runner_factory(dequantized(loaded(d, cfg_t)), wd), inprocess_draft=mode == "async",
                        topology=Topology(0, 1, torch.device("cpu"), "target", 0, 1), **kw)
    rep = compare_lockstep(gpu_eng, cpu_eng, g["prompt"].tolist(), 24,
                           lambda n: SamplingParams(temperature=0, max_new_tokens=n, ignore_eos=True),
                           fan_out=2 if mode == "async" else None, what=f"block fp8 target {mode}")
    gpu_eng.exit()
    print(f"block fp8 target {mode}: {rep.summary()}")
    assert rep.tokens == 24 and rep.tokens_compared >= 0.8 * rep.tokens, rep.summary()


@pytest.mark.parametrize("quantization", ["fp8", None])
def test_llm_generates_from_a_block_fp8_checkpoint_directory(gpu, tmp_path, quantization):
    """LLM(<directory>, quantization="fp8") runs the block-scaled GEMM on the checkpoint's own codes and scales; LLM(<directory>)
    reads the same directory dequantized into a bf16 target.  Both follow the oracle engine on dequantize_fp8_block weights."""
    from oracle.runner import oracle_runner_factory
    from ssd_amd import weights as W
    from ssd_amd.llm import LLM
    from ssd_amd.model_config import ModelConfig
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    from tests.util import assert_stream_matches, seq_margins
    cfg = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 512, 1e-5, 5e5, 1024, False)
    sd = W.synthetic_state_dict(cfg, seed=3, std=0.05)
    d = str(tmp_path)
    write_block_checkpoint(d, cfg, sd)
    kw = dict(hf_config=cfg, max_model_len=256, max_num_batched_tokens=256, kvcache_block_size=16, num_kvcache_blocks=32)
    sp = SamplingParams(temperature=0, max_new_tokens=12, ignore_eos=True)
    prompt = [(5 * j + 1) % 512 for j in range(20)]
    eng = LLM(d, quantization=quantization, **kw)
    dec = eng.model_runner.model
    if quantization == "fp8":
        assert dec.fp8
        assert_block_routing(dec)
    else:
        assert not dec.quantized and dec.w["model.layers.0.mlp.down_proj.weight"].dtype == BF
        assert not any(n.endswith(("_bscale", "_scale")) for n in dec.w)
    out, _ = eng.generate([prompt], sp, use_tqdm=False)
    eng.exit()
    cpu_eng = LLMEngine("t", runner_factory=oracle_runner_factory(dequantized(loaded(d, cfg)), None), **kw)
    ref, _ = cpu_eng.generate([prompt], sp, use_tqdm=False)
    n = assert_stream_matches(out[0]["token_ids"], ref[0]["token_ids"], seq_margins(cpu_eng.model_runner.margin_log, 0), len(prompt),
                              what=f"block fp8 directory, quantization={quantization}")
    print(f"block fp8 directory, quantization={quantization}: identical tokens {n} of {len(ref[0]['token_ids'])}")
    assert len(out[0]["token_ids"]) == 12


def test_default_and_per_row_fp8_paths_are_left_as_they_were(gpu, golden):
    """quantization=None against the recorded trace (tests/golden/engine_golden.npz sd_diff_tokens, near-tie rule on its margins);
    a per-row fp8 target still stores row scales, no group table, and follows the oracle on its own bf16(s * q) weights."""
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.quant import is_quantized_linear
    from ssd_amd.sampling_params import SamplingParams
    from tests.test_model_gpu import mk_cfg, weights, COMMON
    from tests.util import assert_stream_matches, seq_margins
    F.test_default_quantization_none_keeps_todays_stream(gpu, golden)
    g = golden("engine_golden")
    wt, wd = weights(g, "t."), weights(g, "d.")
    kw = dict(hf_config=mk_cfg(g, "llama", "t_"), draft="d", draft_hf_config=mk_cfg(g, "llama", "d_"), speculate=True,
              speculate_k=int(g["sd_K"]), **COMMON)
    prompt = g["prompt"].tolist()
    sp = SamplingParams(temperature=0, max_new_tokens=len(g["sd_diff_tokens"]), ignore_eos=True)
    eng = LLMEngine("t", runner_factory=F._factory({False: wt, True: wd}), quantization="fp8", **kw)
    dec = eng.model_runner.model
    lin = [n for n in dec.w if is_quantized_linear(n)]
    assert lin and all(n + "_scale" in dec.w and dec.w[n + "_scale"].dim() == 1 and n + "_bscale" not in dec.w for n in lin)
    out, _ = eng.generate([prompt], sp, use_tqdm=False)
    cpu_eng = LLMEngine("t", runner_factory=oracle_runner_factory(F.dequantized(wt), wd), **kw)
    ref, _ = cpu_eng.generate([prompt], sp, use_tqdm=False)
    assert_stream_matches(out[0]["token_ids"], ref[0]["token_ids"], seq_margins(cpu_eng.model_runner.margin_log, 0), len(prompt),
                          what="per-row fp8 target")
