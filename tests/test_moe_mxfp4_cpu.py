"""Qwen3-MoE targets with MXFP4 experts, without a GPU: what Config accepts and refuses, the registry entry, the loader of per-expert
mxfp4-pack-quantized tensors (bit for bit into one MX4Tensor with a leading expert dimension; exact bf16 for a bf16 consumer), which
names are quantized linears, and the C ABI of include/ssd_hip_moe_mxfp4.h."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import moe_ref as R
from tests import mxfp4_ref as X

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(max_model_len=256, max_num_batched_tokens=256, kvcache_block_size=16)


def test_config_accepts_mxfp4_experts_and_names_the_field_off_the_grid():
    from ssd_amd.config import Config, resolve_model_config
    ok = R.tiny_moe_config(moe_intermediate_size=128)
    assert Config("moe", hf_config=ok, quantization="mxfp4", **KW).quantization == "mxfp4"
    for bad, field in ((dict(moe_intermediate_size=64), "moe_intermediate_size"), (dict(moe_intermediate_size=128, hidden_size=192), "hidden_size"),
                       (dict(moe_intermediate_size=128, head_dim=16), r"num_heads \* head_dim")):
        with pytest.raises(ValueError, match=field + " to be a multiple of 128"):
            Config("moe", hf_config=R.tiny_moe_config(**bad), quantization="mxfp4", **KW)
    for extra, word in ((dict(kv_cache_dtype="fp8"), "kv_cache_dtype"), (dict(enable_lora=True), "enable_lora"), (dict(num_gpus=2), "one GPU")):
        with pytest.raises(ValueError, match=word):
            Config("moe", hf_config=ok, quantization="mxfp4", **extra, **KW)
    c = resolve_model_config("qwen3-235b-a22b")
    assert (c.family, c.hidden_size, c.num_layers, c.num_heads, c.num_kv_heads, c.head_dim) == ("qwen3_moe", 4096, 94, 64, 4, 128)
    assert (c.num_experts, c.num_experts_per_tok, c.moe_intermediate_size, c.norm_topk_prob, c.qk_norm) == (128, 8, 1536, True, True)
    Config("qwen3-235b-a22b", quantization="mxfp4", **KW)


def test_the_router_and_the_expert_tensors_are_not_dense_quantized_linears():
    from ssd_amd.quant import is_quantized_linear
    p = "model.layers.3."
    assert not is_quantized_linear(p + "mlp.gate.weight")
    assert not is_quantized_linear(p + "mlp.experts.gate_up_proj") and not is_quantized_linear(p + "mlp.experts.down_proj")
    assert is_quantized_linear(p + "self_attn.qkv_proj.weight") and is_quantized_linear(p + "self_attn.o_proj.weight")


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """A one-layer checkpoint: q / k / v / o and every expert's gate / up / down as .weight_packed + .weight_scale, the rest bf16."""
    from safetensors.torch import save_file
    path = str(tmp_path_factory.mktemp("moe_mx4"))
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
    want = {}
    for name, (n, k) in shapes.items():
        codes = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8).numpy()
        b = torch.randint(112, 126, (n, k // 32), generator=g, dtype=torch.uint8)
        t[p + name + ".weight_packed"], t[p + name + ".weight_scale"] = torch.from_numpy(X.pack(codes)), b
        want[name] = (codes, b.numpy())
    save_file(t, os.path.join(path, "model.safetensors"))
    wq = {"num_bits": 4, "type": "float", "symmetric": True, "strategy": "group", "group_size": 32, "dynamic": False}
    qc = {"quant_method": "compressed-tensors", "format": "mxfp4-pack-quantized", "ignore": ["lm_head"],
          "config_groups": {"group_0": {"targets": ["Linear"], "weights": wq, "input_activations": None}}}
    json.dump({"model_type": "qwen3_moe", "quantization_config": qc}, open(os.path.join(path, "config.json"), "w"))
    return cfg, path, t, want


def _expert_rows(want, e, up):
    parts = [f"mlp.experts.{e}.gate_proj", f"mlp.experts.{e}.up_proj"] if up else [f"mlp.experts.{e}.down_proj"]
    return np.concatenate([want[x][0] for x in parts]), np.concatenate([want[x][1] for x in parts])


@pytest.mark.parametrize("mxfp4", [True, False])
def test_loader_stacks_per_expert_tensors(ckpt, mxfp4):
    """An mxfp4 target gets the codes and scale bytes bit for bit, one MX4Tensor [E, ...] per tensor; a bf16 consumer the exact matrix."""
    from ssd_amd.quant import MX4Tensor
    from ssd_amd.weights import load_safetensors
    cfg, path, t, want = ckpt
    got = dict(load_safetensors(cfg, path, mxfp4=mxfp4))
    E = cfg.num_experts
    for name, up in (("model.layers.0.mlp.experts.gate_up_proj", True), ("model.layers.0.mlp.experts.down_proj", False)):
        w = got[name]
        for e in range(E):
            codes, b = _expert_rows(want, e, up)
            if mxfp4:
                assert isinstance(w, MX4Tensor) and w.packed.dtype == torch.uint8 and w.shape() == (E, *codes.shape)
                assert np.array_equal(w.packed[e].numpy(), X.pack(codes)) and np.array_equal(w.scale[e].numpy(), b), (name, e)
            else:
                assert w.dtype == BF and tuple(w.shape) == (E, *codes.shape)
                assert np.array_equal(w[e].view(torch.int16).numpy().view(np.uint16), X.bf16_bits_exact(X.exact(codes, b))), (name, e)
    assert isinstance(got["model.layers.0.self_attn.qkv_proj.weight"], MX4Tensor) == mxfp4
    assert torch.equal(got["model.layers.0.mlp.gate.weight"], t["model.layers.0.mlp.gate.weight"])


def test_header_symbol_bound_and_c_consumer(tmp_path):
    import re
    from ssd_amd.hip.lib import build_library, lib_path
    from ssd_amd.hip.moe_ops import MOE_MX4_SIGNATURES, load_moe_mx4_library
    if not os.path.exists(lib_path()):
        build_library()
    text = open(os.path.join(ROOT, "include", "ssd_hip_moe_mxfp4.h")).read()
    assert sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", text, flags=re.M))) == sorted(MOE_MX4_SIGNATURES) == ["ssd_moe_gemm_mxfp4"]
    assert hasattr(load_moe_mx4_library(), "ssd_moe_gemm_mxfp4") and "ACCUMULATION ORDER (normative)" in text
    src, exe, libdir = os.path.join(ROOT, "tests", "moe_mxfp4_abi_consumer.c"), str(tmp_path / "consumer"), os.path.dirname(lib_path())
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "0 failures" in run.stdout, run.stdout + run.stderr
