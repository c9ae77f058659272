"""Qwen3-MoE targets with block-scaled FP8 experts, without a GPU: what Config accepts and refuses, the loader of per-expert
.weight (float8_e4m3fn) + .weight_scale_inv tensors (bit for bit into one FP8BTensor with a leading expert dimension; the exact
bf16(s * q) image for a bf16 consumer), and the C ABI of include/ssd_hip_moe_fp8b.h."""
import json
import os
import subprocess

import pytest
import torch

from tests import moe_ref as R

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(max_model_len=256, max_num_batched_tokens=256, kvcache_block_size=16)


def test_config_accepts_fp8_experts_and_names_the_field_off_the_grid():
    from ssd_amd.config import Config
    ok = R.tiny_moe_config(moe_intermediate_size=128, head_dim=64)
    assert Config("moe", hf_config=ok, quantization="fp8", **KW).quantization == "fp8"
    Config("qwen3-235b-a22b", quantization="fp8", **KW)
    for bad, field in ((dict(moe_intermediate_size=64), "moe_intermediate_size"), (dict(moe_intermediate_size=128, hidden_size=192), "hidden_size"),
                       (dict(moe_intermediate_size=128, head_dim=16), r"num_heads \* head_dim")):
        with pytest.raises(ValueError, match="quantization.*" + field + " to be a multiple of 128"):
            Config("moe", hf_config=R.tiny_moe_config(**bad), quantization="fp8", **KW)
    for extra, word in ((dict(kv_cache_dtype="fp8"), "kv_cache_dtype"), (dict(enable_lora=True), "enable_lora"), (dict(num_gpus=2), "one GPU")):
        with pytest.raises(ValueError, match=word):
            Config("moe", hf_config=ok, quantization="fp8", **extra, **KW)
    with pytest.raises(ValueError, match="quantization='w4a16'"):
        Config("moe", hf_config=ok, quantization="w4a16", **KW)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """A one-layer checkpoint: q / k / v / o and every expert's gate / up / down as .weight float8_e4m3fn + .weight_scale_inv fp32
    [N / 128, K / 128], the router and the rest bf16."""
    from safetensors.torch import save_file
    from ssd_amd.quant import FP8
    path = str(tmp_path_factory.mktemp("moe_fp8b"))
    cfg = R.tiny_moe_config(num_layers=1, moe_intermediate_size=128, head_dim=64)
    g = torch.Generator().manual_seed(4)
    h, I, E, p = cfg.hidden_size, cfg.moe_intermediate_size, cfg.num_experts, "model.layers.0."
    t = {n: torch.randn(*s, generator=g).to(BF) for n, s in (("model.embed_tokens.weight", (512, h)), ("lm_head.weight", (512, h)),
                                                             (p + "mlp.gate.weight", (E, h)))}
    t.update({n: torch.ones(s, dtype=BF) for n, s in (("model.norm.weight", h), (p + "input_layernorm.weight", h),
                                                      (p + "post_attention_layernorm.weight", h), (p + "self_attn.q_norm.weight", 64),
                                                      (p + "self_attn.k_norm.weight", 64))})
    shapes = {"self_attn.q_proj": (256, h), "self_attn.k_proj": (128, h), "self_attn.v_proj": (128, h), "self_attn.o_proj": (h, 256)}
    for e in range(E):
        shapes.update({f"mlp.experts.{e}.gate_proj": (I, h), f"mlp.experts.{e}.up_proj": (I, h), f"mlp.experts.{e}.down_proj": (h, I)})
    for name, (n, k) in shapes.items():
        codes = torch.randint(0, 127, (n, k), generator=g, dtype=torch.uint8) | (torch.randint(0, 2, (n, k), generator=g, dtype=torch.uint8) << 7)
        t[p + name + ".weight"] = codes.view(FP8)
        t[p + name + ".weight_scale_inv"] = torch.exp2(4.0 * torch.rand(n // 128, k // 128, generator=g) - 9.0) * (1.0 + torch.rand(n // 128, k // 128, generator=g))
    save_file(t, os.path.join(path, "model.safetensors"))
    qc = {"quant_method": "fp8", "fmt": "e4m3", "activation_scheme": "dynamic", "weight_block_size": [128, 128],
          "modules_to_not_convert": ["lm_head", "model.layers.0.mlp.gate"]}
    json.dump({"model_type": "qwen3_moe", "quantization_config": qc}, open(os.path.join(path, "config.json"), "w"))
    return cfg, path, t


@pytest.mark.parametrize("fp8", [True, False])
def test_loader_stacks_per_expert_tensors(ckpt, fp8):
    """An fp8 target gets the codes and the expanded scales bit for bit, one FP8BTensor [E, N, K] per tensor; a bf16 consumer the
    exact bf16(s * q) matrix."""
    from ssd_amd.quant import FP8BTensor, expand_fp8_block_scales
    from ssd_amd.weights import load_safetensors
    cfg, path, t = ckpt
    got = dict(load_safetensors(cfg, path, fp8=fp8))
    E, p = cfg.num_experts, "model.layers.0.mlp.experts."
    for name, parts in ((p + "gate_up_proj", ("gate_proj", "up_proj")), (p + "down_proj", ("down_proj",))):
        w = got[name]
        for e in range(E):
            src = [p + f"{e}.{x}" for x in parts]
            codes = torch.cat([t[s + ".weight"].view(torch.uint8) for s in src])
            scales = torch.cat([expand_fp8_block_scales(t[s + ".weight_scale_inv"], t[s + ".weight"].shape[0]) for s in src])
            if fp8:
                assert isinstance(w, FP8BTensor) and w.shape() == (E, *codes.shape) and w.dequantize().shape == (E, *codes.shape)
                assert torch.equal(w.codes[e].view(torch.uint8), codes) and torch.equal(w.rowscale[e], scales), (name, e)
            else:
                want = (codes.view(torch.float8_e4m3fn).float() * scales.repeat_interleave(128, dim=1)).to(BF)      # the product in fp32
                assert w.dtype == BF and tuple(w.shape) == (E, *codes.shape) and torch.equal(w[e], want), (name, e)
    assert isinstance(got["model.layers.0.self_attn.qkv_proj.weight"], FP8BTensor) == fp8
    assert torch.equal(got["model.layers.0.mlp.gate.weight"], t["model.layers.0.mlp.gate.weight"])


def test_header_symbol_bound_and_c_consumer(tmp_path):
    import re
    from ssd_amd.hip.lib import build_library, lib_path
    from ssd_amd.hip.moe_ops import MOE_FP8B_SIGNATURES, MOE_MX4_SIGNATURES, load_moe_fp8b_library
    if not os.path.exists(lib_path()):
        build_library()
    text = open(os.path.join(ROOT, "include", "ssd_hip_moe_fp8b.h")).read()
    assert sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", text, flags=re.M))) == sorted(MOE_FP8B_SIGNATURES) == ["ssd_moe_gemm_fp8b"]
    assert len(MOE_FP8B_SIGNATURES["ssd_moe_gemm_fp8b"]) == len(MOE_MX4_SIGNATURES["ssd_moe_gemm_mxfp4"]) == 13
    assert hasattr(load_moe_fp8b_library(), "ssd_moe_gemm_fp8b") and "ACCUMULATION ORDER (normative)" in text
    src, exe, libdir = os.path.join(ROOT, "tests", "moe_fp8b_abi_consumer.c"), str(tmp_path / "consumer"), os.path.dirname(lib_path())
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "0 failures" in run.stdout, run.stdout + run.stderr
