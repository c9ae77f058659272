"""Sliding-window attention without a GPU: the window rules of ModelConfig.from_hf against transformers' own configs, every Config /
engine refusal by name, the C ABI of include/ssd_hip_swa.h, and tests/swa_ref.py's float64 forward against transformers'
MistralForCausalLM -- which ties the mask convention (W keys, the query's own included) to the published one."""
import dataclasses
import os
import re
import subprocess

import pytest
import torch

from ssd_amd.config import Config
from ssd_amd.model_config import ModelConfig
from tests import swa_ref
from tests.conftest import ROOT
from tests.util import truth_forward_masked

TINY = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=32, intermediate_size=256,
            vocab_size=512, max_position_embeddings=1024, tie_word_embeddings=False)


def windows(cfg):
    return [cfg.window_of(li) for li in range(cfg.num_layers)]


def test_from_hf_reads_the_three_window_rules_as_transformers_does():
    from transformers import MistralConfig, Qwen3Config
    m = ModelConfig.from_hf(MistralConfig(sliding_window=8, **TINY))
    assert (m.family, m.sliding_window, m.layer_windows, m.windowed) == ("llama", 8, (), True) and windows(m) == [8, 8]
    for none in (MistralConfig(sliding_window=None, **TINY), Qwen3Config(**TINY), Qwen3Config(use_sliding_window=False, sliding_window=8, **TINY)):
        c = ModelConfig.from_hf(none)
        assert (c.sliding_window, c.layer_windows, c.windowed) == (0, (), False)
    four = dict(TINY, num_hidden_layers=4)
    for hc in (Qwen3Config(use_sliding_window=True, sliding_window=8, max_window_layers=1, **four),
               Qwen3Config(use_sliding_window=True, sliding_window=8, max_window_layers=0, **four),
               Qwen3Config(use_sliding_window=True, sliding_window=8, layer_types=["sliding_attention", "full_attention"] * 2, **four)):
        c = ModelConfig.from_hf(hc)
        assert c.family == "qwen3" and windows(c) == [8 if t == "sliding_attention" else 0 for t in hc.layer_types], hc.layer_types
    assert windows(ModelConfig.from_hf(Qwen3Config(use_sliding_window=True, sliding_window=8, max_window_layers=1, **four))) == [0, 8, 8, 8]
    # the fallback itself, on a config object that carries no layer_types
    bare = argparse_like(model_type="qwen2", use_sliding_window=True, sliding_window=8, max_window_layers=3, **four)
    assert windows(ModelConfig.from_hf(bare)) == [0, 0, 0, 8]
    for bad in (["sliding_attention"] * 3, ["sliding_attention", "chunked_attention"] * 2):
        with pytest.raises(ValueError, match="layer_types"):
            ModelConfig.from_hf(argparse_like(model_type="qwen3", sliding_window=8, layer_types=bad, **four))
    with pytest.raises(ValueError, match="sliding_window"):
        ModelConfig.from_hf(argparse_like(model_type="qwen3", sliding_window=None, layer_types=["sliding_attention"] * 4, **four))


def argparse_like(**kw):
    import types
    return types.SimpleNamespace(rms_norm_eps=1e-6, rope_theta=1e6, **kw)


def test_mistral_preset_and_every_refusal_by_name():
    m = Config("mistral-7b-v0.1").hf_config
    assert (m.family, m.hidden_size, m.num_layers, m.num_heads, m.num_kv_heads, m.head_dim, m.intermediate_size, m.vocab_size, m.rms_norm_eps,
            m.rope_theta, m.max_position_embeddings, m.sliding_window) == ("llama", 4096, 32, 32, 8, 128, 14336, 32000, 1e-5, 1e4, 32768, 4096)
    t = ModelConfig("llama", 128, 2, 4, 2, 32, 256, 512, sliding_window=8)
    full = dataclasses.replace(t, sliding_window=0)
    sync = dict(speculate=True, draft="d", speculate_k=2)
    # accepted: target in every mode, draft in synchronous speculation, with the weight and cache formats and adapters
    Config("t", hf_config=t)
    Config("t", hf_config=t, draft_hf_config=t, **sync)
    Config("t", hf_config=t, draft_hf_config=full, draft_async=True, num_gpus=2, **sync)
    Config("t", hf_config=dataclasses.replace(t, layer_windows=(8, 0)), kv_cache_dtype="fp8", quantization="fp8", enable_lora=True)
    with pytest.raises(ValueError, match="draft_async"):
        Config("t", hf_config=full, draft_hf_config=t, draft_async=True, num_gpus=2, **sync)
    with pytest.raises(ValueError, match="use_eagle"):
        Config("t", hf_config=t, draft="eagle3-llama-3.1-8b", draft_hf_config=dataclasses.replace(full, num_layers=1, draft_vocab_size=512),
               speculate=True, draft_async=True, jit_speculate=True, use_eagle=True, eagle_layers=[0, 1], num_gpus=2)
    with pytest.raises(ValueError, match="num_gpus"):
        Config("t", hf_config=t, num_gpus=2)
    moe = dict(num_experts=8, num_experts_per_tok=2, moe_intermediate_size=64)
    with pytest.raises(ValueError, match="sliding_window.*mixture-of-experts"):
        Config("t", hf_config=dataclasses.replace(t, family="qwen3_moe", qk_norm=True, **moe))
    for bad in (dict(sliding_window=-1), dict(layer_windows=(8, -8)), dict(layer_windows=(8, 0, 8)), dict(sliding_window=True)):
        with pytest.raises(ValueError, match="sliding_window|layer_windows"):
            Config("t", hf_config=dataclasses.replace(t, **bad))


def test_engine_refuses_a_windowed_model_before_building_a_runner_without_the_kernel():
    from ssd_amd.engine.llm_engine import LLMEngine
    built = []

    def factory(config, model_cfg, **kw):
        built.append(model_cfg)
        raise AssertionError("a runner was built")
    t = ModelConfig("llama", 128, 2, 4, 2, 32, 256, 512, sliding_window=8)
    with pytest.raises(ValueError, match="sliding-window.*kernel"):
        LLMEngine("t", hf_config=t, runner_factory=factory, kvcache_block_size=16, max_model_len=64, max_num_batched_tokens=64)
    assert not built


def test_decoder_gives_up_the_routes_that_run_attention_inside_another_kernel():
    from ssd_amd.model import HipDecoder
    from ssd_amd.model_config import PRESETS
    kw = dict(max_tokens=32, max_seqs=1, max_blocks=2048, block_size=16, max_model_len=32768, device=torch.device("cpu"))
    cfg = dataclasses.replace(PRESETS["llama-3.2-1b"], num_layers=2)
    a, b = HipDecoder(cfg, **kw), HipDecoder(dataclasses.replace(cfg, layer_windows=(4096, 0)), **kw)
    assert a.chain_seg and a.tree_seg and a.fuse_attn_o and not a.swa
    assert b.swa and not (b.chain_seg or b.tree_seg or b.fuse_attn_o)
    assert b.fusion_plan(1) == a.fusion_plan(1) == (True, True) and b.use_parts == a.use_parts       # the QKV epilogue is unaffected
    meta = type("M", (), dict(max_q=1, B=1, ctx_hint=32768))()
    assert b._attn_cfg(1, meta) == a._attn_cfg(1, meta) and a._attn_cfg(1, meta)[0] == 16
    assert b._attn_cfg(1, meta, 4096)[0] == 8                         # a 32k context under a 4k window: 8 splits, not 16
    meta.ctx_hint = 2048
    assert b._attn_cfg(1, meta, 4096) == a._attn_cfg(1, meta)         # a context inside the window: the unwindowed decomposition


def test_header_symbols_exported_bound_and_consumer_links(tmp_path):
    from ssd_amd.hip.lib import SIGNATURES, build_library, lib_path
    from ssd_amd.hip.swa_ops import SWA_SIGNATURES, load_swa_library
    if not os.path.exists(lib_path()):
        build_library()
    head = open(os.path.join(ROOT, "include", "ssd_hip_swa.h")).read()
    syms = sorted(re.findall(r"^int\s+(ssd_\w+)\s*\(", head, flags=re.M))
    assert syms == ["ssd_attn_paged_fp8_window", "ssd_attn_paged_window"] == sorted(SWA_SIGNATURES) and not set(syms) & set(SIGNATURES)
    lib = load_swa_library()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        decl = re.search(r"^int\s+" + s + r"\s*\(([^;]*)\);", head, flags=re.M | re.S).group(1)
        assert len(SWA_SIGNATURES[s]) == len(decl.split(",")), s
    src = os.path.join(ROOT, "tests", "swa_abi_consumer.c")
    exe, libdir = str(tmp_path / "swa_abi_consumer"), os.path.dirname(lib_path())
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "0 failures" in run.stdout, run.stdout + run.stderr


def test_float64_windowed_forward_equals_transformers_mistral():
    from transformers import MistralConfig, MistralForCausalLM
    from ssd_amd import weights as W
    from tests.test_moe_cpu import _hf_state_dict
    hc = MistralConfig(sliding_window=8, rms_norm_eps=1e-5, rope_theta=1e4, **TINY)
    cfg = ModelConfig.from_hf(hc)
    w = W.synthetic_state_dict(cfg, seed=5, std=0.1, norm_jitter=0.1)
    tokens = [(37 * i + 11) % 512 for i in range(40)]
    sd = {}
    for name, t in _hf_state_dict(cfg, w, torch.float64).items():
        if "gate_up_proj" in name:
            sd[name.replace("gate_up_proj", "gate_proj")], sd[name.replace("gate_up_proj", "up_proj")] = t.chunk(2, 0)
        else:
            sd[name] = t
    model = MistralForCausalLM(hc).double().eval()
    model.load_state_dict(sd, strict=True)
    with torch.no_grad():
        want = model(torch.tensor([tokens])).logits[0]
    got = swa_ref.forward(cfg, w, tokens)
    full = swa_ref.forward(dataclasses.replace(cfg, sliding_window=0), w, tokens)
    # one window for every layer: swa_ref is the existing masked reference under the window mask
    masked = truth_forward_masked(cfg, w, tokens, list(range(40)), swa_ref.visible(40, 8))
    assert float((got - masked).abs().max() / masked.abs().max()) <= 1e-12          # float64 both, operations in another order
    rel = float((got - want).abs().max() / want.abs().max())
    rel_full = float((full[8:] - want[8:]).abs().max() / want.abs().max())
    print(f"swa_ref forward vs MistralForCausalLM float64: max relative difference {rel:.3e}; the full-attention forward {rel_full:.3e}")
    # transformers keeps the rotary table and every RMSNorm's normalisation in float32 whatever the model's dtype: the bound and its
    # reason are tests/test_moe_cpu.py's for its truth proper
    assert rel <= 1e-5, rel
    assert torch.equal(full[:8], got[:8]) and rel_full > 1e-3, rel_full          # the window matters from position 8 on
