"""FP8 weight-only quantization, the parts that need no GPU: the configuration surface, the compressed-tensors checkpoint loader, the
torch-side quantizer and row orders, and the C ABI of include/ssd_hip_quant.h (exports, ctypes table, INTEGRATION.md, a plain-C
consumer walking every entry point's argument validation)."""
import json
import os
import re
import subprocess
import types

import pytest
import torch

from tests.conftest import ROOT
from tests import fp8_ref

HEADER = os.path.join(ROOT, "include", "ssd_hip_quant.h")


def quant_header_symbols():
    return sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


# ---------------------------------------------------------------------------------------------------------------------
# Config
# ---------------------------------------------------------------------------------------------------------------------
def test_config_accepts_fp8_and_defaults_to_none():
    from ssd_amd.config import Config
    assert Config("llama-3.1-70b").quantization is None
    assert Config("llama-3.1-70b", quantization="fp8").quantization == "fp8"
    c = Config("llama-3.1-70b", quantization="fp8", speculate=True, draft="llama-3.2-1b", speculate_k=4)
    assert c.quantization == "fp8"


def test_config_refuses_unsupported_fp8_combinations():
    from ssd_amd.config import Config
    with pytest.raises(ValueError, match="one GPU"):
        Config("llama-3.1-70b", quantization="fp8", num_gpus=2)
    with pytest.raises(ValueError, match="use_eagle"):
        Config("llama-3.1-8b", quantization="fp8", speculate=True, draft="eagle3-llama-3.1-8b", draft_async=True,
               jit_speculate=True, use_eagle=True)
    with pytest.raises(ValueError, match="quantization"):
        Config("llama-3.1-8b", quantization="int4")


def test_llm_keyword_reaches_config():
    """LLM(model, quantization=...) keeps the keyword (unknown keywords are dropped by name against Config's fields)."""
    from dataclasses import fields
    from ssd_amd.config import Config
    assert "quantization" in {f.name for f in fields(Config)}


# ---------------------------------------------------------------------------------------------------------------------
# Quantizer and row orders (torch on the CPU here; the GPU test runs the same on the device)
# ---------------------------------------------------------------------------------------------------------------------
def test_quantizer_matches_restatement_and_zero_rows():
    from ssd_amd.quant import quantize_fp8, dequantize_fp8
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(96, 192, generator=g) * 0.03).to(torch.bfloat16)
    w[5] = 0
    w[7, 3] = 2.5                                   # an outlier row
    q, s = quantize_fp8(w)
    q_ref, s_ref = fp8_ref.quantize(w)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32
    assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8))
    assert torch.equal(s, s_ref)
    assert s[5] == 1 and (q[5].float() == 0).all()
    assert q.float().abs().max() <= 448
    rel = ((dequantize_fp8(q, s).float() - w.float()).abs().amax(1) / w.float().abs().amax(1).clamp_min(1e-30))
    assert rel.max() <= 2 ** -4                     # 3 mantissa bits: half an ulp of the largest element of a row


def test_row_maps_match_the_bf16_packed_orders():
    from ssd_amd.quant import qkv_row_map, gate_up_row_map
    from ssd_amd.model import HipDecoder
    for nh, nkv, hd in ((2, 1, 64), (64, 8, 128), (32, 8, 64)):
        got = qkv_row_map(nh, nkv, hd).tolist()
        assert got == fp8_ref.qkv_order(nh, nkv, hd)
        me = types.SimpleNamespace(nh=nh, nkv=nkv, hd=hd)
        assert got == HipDecoder._qkv_row_perm(me).tolist()      # the order the bf16 qkv bias is permuted with
    for N in (512, 2 * 28672):
        assert gate_up_row_map(N).tolist() == fp8_ref.gate_up_order(N)


# ---------------------------------------------------------------------------------------------------------------------
# compressed-tensors checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def _tiny_cfg():
    from ssd_amd.model_config import ModelConfig
    return ModelConfig("llama", 128, 1, 2, 1, 64, 256, 512)


def _write_ckpt(path, cfg, *, strategy="channel", method="compressed-tensors", wtype="float", extra=None, seed=0):
    """A one-layer checkpoint with unpacked q/k/v and gate/up (HF names).  q/k/v and gate/up carry per-TENSOR scales, o/down per-row
    [N, 1] ones, every weight has an input_scale, lm_head and the embedding are bf16."""
    from safetensors.torch import save_file
    g = torch.Generator().manual_seed(seed)
    h, hd, nh, nkv, I, V = cfg.hidden_size, cfg.head_dim, cfg.num_heads, cfg.num_kv_heads, cfg.intermediate_size, cfg.vocab_size
    p = "model.layers.0."
    t = {"model.embed_tokens.weight": torch.randn(V, h, generator=g).to(torch.bfloat16),
         "lm_head.weight": torch.randn(V, h, generator=g).to(torch.bfloat16),
         "model.norm.weight": torch.ones(h, dtype=torch.bfloat16),
         p + "input_layernorm.weight": torch.ones(h, dtype=torch.bfloat16),
         p + "post_attention_layernorm.weight": torch.ones(h, dtype=torch.bfloat16)}
    want = {}
    shapes = {"self_attn.q_proj": (nh * hd, h), "self_attn.k_proj": (nkv * hd, h), "self_attn.v_proj": (nkv * hd, h),
              "self_attn.o_proj": (h, nh * hd), "mlp.gate_proj": (I, h), "mlp.up_proj": (I, h), "mlp.down_proj": (h, I)}
    for name, (n, k) in shapes.items():
        q = (torch.randn(n, k, generator=g) * 100).clamp(-448, 448).to(torch.float8_e4m3fn)
        per_tensor = name in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "mlp.gate_proj", "mlp.up_proj")
        s = torch.rand((), generator=g) * 1e-3 + 1e-4 if per_tensor else torch.rand(n, 1, generator=g) * 1e-3 + 1e-4
        t[p + name + ".weight"] = q
        t[p + name + ".weight_scale"] = s.float()
        t[p + name + ".input_scale"] = torch.tensor([0.5])
        want[name] = (q, s.float().reshape(-1).expand(n).clone())
    t.update(extra or {})
    save_file(t, os.path.join(path, "model.safetensors"))
    qc = {"quant_method": method, "format": "float-quantized", "ignore": ["lm_head"],
          "config_groups": {"group_0": {"targets": ["Linear"], "weights": {"num_bits": 8, "type": wtype, "strategy": strategy,
                                                                          "symmetric": True, "dynamic": False},
                                        "input_activations": {"num_bits": 8, "type": "float", "strategy": "tensor", "dynamic": False}}}}
    json.dump({"model_type": "llama", "quantization_config": qc}, open(os.path.join(path, "config.json"), "w"))
    return t, want


def test_compressed_tensors_loader_yields_packed_q_and_row_scales(tmp_path):
    from ssd_amd.weights import load_safetensors, checkpoint_quantization
    cfg = _tiny_cfg()
    t, want = _write_ckpt(str(tmp_path), cfg)
    assert checkpoint_quantization(str(tmp_path)) == "fp8"
    got = dict(load_safetensors(cfg, str(tmp_path), fp8=True))
    p = "model.layers.0."
    packs = {"self_attn.qkv_proj": ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"],
             "mlp.gate_up_proj": ["mlp.gate_proj", "mlp.up_proj"], "self_attn.o_proj": ["self_attn.o_proj"],
             "mlp.down_proj": ["mlp.down_proj"]}
    for packed, parts in packs.items():
        q, s = got[p + packed + ".weight"]
        assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and s.dim() == 1
        assert torch.equal(q.view(torch.uint8), torch.cat([want[x][0] for x in parts]).view(torch.uint8))
        assert torch.equal(s, torch.cat([want[x][1] for x in parts]))
    # per-tensor scales became one per row, constant over each source matrix
    s_qkv = got[p + "self_attn.qkv_proj.weight"][1]
    assert s_qkv[0] == s_qkv[127] and s_qkv[128] == s_qkv[191]
    assert got["lm_head.weight"].dtype == torch.bfloat16 and torch.equal(got["lm_head.weight"], t["lm_head.weight"])
    assert not any(k.endswith("_scale") for k in got)
    # a bf16 target reads the same checkpoint as bf16(s * q)
    bf = dict(load_safetensors(cfg, str(tmp_path)))
    q, s = got[p + "mlp.gate_up_proj.weight"]
    assert bf[p + "mlp.gate_up_proj.weight"].dtype == torch.bfloat16
    assert torch.equal(bf[p + "mlp.gate_up_proj.weight"], fp8_ref.dequant(q, s))


@pytest.mark.parametrize("kw,match", [
    (dict(method="fp8"), "quant_method"),
    (dict(strategy="block"), "strategy"),
    (dict(wtype="int"), "type"),
])
def test_compressed_tensors_loader_refuses_other_schemes(tmp_path, kw, match):
    from ssd_amd.weights import load_safetensors
    cfg = _tiny_cfg()
    _write_ckpt(str(tmp_path), cfg, **kw)
    with pytest.raises(ValueError, match=match):
        list(load_safetensors(cfg, str(tmp_path), fp8=True))


def test_loader_refuses_block_scales_and_fnuz(tmp_path):
    from ssd_amd.weights import load_safetensors
    cfg = _tiny_cfg()
    d1, d2 = tmp_path / "a", tmp_path / "b"
    d1.mkdir()
    d2.mkdir()
    _write_ckpt(str(d1), cfg, extra={"model.layers.0.mlp.down_proj.weight_scale_inv": torch.ones(1, 2)})
    with pytest.raises(ValueError, match="weight_scale_inv"):
        list(load_safetensors(cfg, str(d1), fp8=True))
    _write_ckpt(str(d2), cfg)
    from safetensors.torch import load_file, save_file
    f = os.path.join(str(d2), "model.safetensors")
    t = load_file(f)
    t["model.layers.0.self_attn.o_proj.weight"] = t["model.layers.0.self_attn.o_proj.weight"].view(torch.uint8).view(torch.float8_e4m3fnuz)
    save_file(t, f)
    with pytest.raises(ValueError, match="e4m3fn"):
        list(load_safetensors(cfg, str(d2), fp8=True))


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _built_lib():
    from ssd_amd.hip.lib import build_library, lib_path
    if not os.path.exists(lib_path()):
        build_library()
    return lib_path()


def test_quant_header_symbols_exported_bound_and_documented():
    from ssd_amd.hip.lib import SIGNATURES
    from ssd_amd.hip.quant_ops import QUANT_SIGNATURES, load_quant_library
    _built_lib()
    lib = load_quant_library()
    syms = quant_header_symbols()
    assert len(syms) == 5
    assert sorted(QUANT_SIGNATURES) == syms
    assert not set(syms) & set(SIGNATURES)             # lib.SIGNATURES stays exactly ssd_hip.h + ssd_hip_tune.h
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        assert f"`{s}(" in doc, f"{s} has no line in INTEGRATION.md"
    common = open(os.path.join(ROOT, "ssd_amd", "csrc", "common.h")).read()
    assert '#include "ssd_hip_quant.h"' in common


def test_c_consumer_walks_every_fp8_validation_path(tmp_path):
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "fp8_abi_consumer.c")
    body = open(src).read()
    for s in quant_header_symbols():
        assert f"{s}(" in body, s
    exe = str(tmp_path / "fp8_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout
