"""W4A16 weight-only quantization, the parts that need no GPU: the configuration surface, the torch quantizer and packing against the
numpy restatement (tests/w4a16_ref.py), the compressed-tensors pack-quantized checkpoint loader and its refusals, and the C ABI of
include/ssd_hip_w4a16.h (exports, ctypes table, INTEGRATION.md, a plain-C consumer walking every entry point's argument
validation)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests import w4a16_ref as R

HEADER = os.path.join(ROOT, "include", "ssd_hip_w4a16.h")
P = "model.layers.0."


def w4_header_symbols():
    return sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


def bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------
# Config
# ---------------------------------------------------------------------------------------------------------------------
def test_config_accepts_w4a16():
    from ssd_amd.config import Config
    assert Config("llama-3.1-70b", quantization="w4a16").quantization == "w4a16"
    c = Config("llama-3.1-70b", quantization="w4a16", speculate=True, draft="llama-3.2-1b", speculate_k=4)
    assert c.quantization == "w4a16"


def test_config_refuses_w4a16_with_tp_or_eagle_and_other_spellings():
    from ssd_amd.config import Config
    with pytest.raises(ValueError, match="one GPU"):
        Config("llama-3.1-70b", quantization="w4a16", num_gpus=2)
    with pytest.raises(ValueError, match="use_eagle"):
        Config("llama-3.1-8b", quantization="w4a16", speculate=True, draft="eagle3-llama-3.1-8b", draft_async=True,
               jit_speculate=True, use_eagle=True)
    for bad in ("int4", "W4A16", "w4"):
        with pytest.raises(ValueError, match="quantization"):
            Config("llama-3.1-8b", quantization=bad)


def test_decoder_refuses_w4a16_off_the_group_grid():
    """hidden_size 64 (tests/test_async_cpu.py's tiny geometry) is not a multiple of the 128-column group."""
    from ssd_amd.model import HipDecoder
    from ssd_amd.model_config import ModelConfig
    cfg = ModelConfig("llama", 64, 1, 2, 1, 32, 128, 256)
    with pytest.raises(ValueError, match="multiples of 128"):
        HipDecoder(cfg, max_tokens=16, max_seqs=1, max_blocks=2, block_size=16, max_model_len=64, device=torch.device("cpu"),
                   quantization="w4a16")


# ---------------------------------------------------------------------------------------------------------------------
# Quantizer and packing (torch on the CPU here; the GPU tests run the same on the device)
# ---------------------------------------------------------------------------------------------------------------------
def test_quantizer_bit_exact_against_numpy_with_zero_groups_and_ties():
    from ssd_amd.quant import quantize_w4a16, dequantize_w4a16, unpack_w4
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(48, 512, generator=g) * 0.03).to(torch.bfloat16)
    w[2, 128:256] = 0                                    # an all-zero group: s = 1, q = 0
    w[5, :] = 0                                          # an all-zero row
    # ties: amax 7 -> s = 1 exactly, so w / s lands on .5 and must round to even
    w[7, 0:8] = torch.tensor([7.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5], dtype=torch.bfloat16)
    w[7, 8:128] = 0
    w[9, 0] = 3.0                                        # an outlier group
    t = quantize_w4a16(w)
    q_ref, s_ref = R.quantize(w)
    assert t.packed.dtype == torch.int32 and tuple(t.packed.shape) == (48, 64)
    assert t.scale.dtype == torch.bfloat16 and tuple(t.scale.shape) == (48, 4)
    assert np.array_equal(t.packed.numpy(), R.pack(q_ref))
    assert np.array_equal(bits(t.scale), s_ref)
    q = unpack_w4(t.packed)
    assert np.array_equal(q.numpy(), q_ref)
    assert t.scale[2, 1].item() == 1.0 and (q[2, 128:256] == 0).all() and (t.scale[5] == 1).all()
    assert t.scale[7, 0].item() == 1.0
    assert q[7, :8].tolist() == [7, 0, 2, 2, 0, -2, -2, 4]
    assert int(q.min()) >= -8 and int(q.max()) <= 7
    assert np.array_equal(bits(dequantize_w4a16(t.packed, t.scale)), R.dequant(q_ref, s_ref))
    # half a step of the group's scale, plus the bf16 rounding of s * q, bounds the error
    wg = w.float().reshape(48, 4, 128)
    err = (dequantize_w4a16(t.packed, t.scale).float().reshape(48, 4, 128) - wg).abs().amax(-1)
    assert bool((err <= t.scale.float() * 0.5 + wg.abs().amax(-1) * 2 ** -8).all())


def test_pack_unpack_extremes_and_layout():
    from ssd_amd.quant import pack_w4, unpack_w4
    q = torch.tensor([[-8, 7, 0, -1, 1, -8, 7, 3] * 32], dtype=torch.int8).repeat(16, 1)
    p = pack_w4(q)
    assert np.array_equal(p.numpy(), R.pack(q.numpy()))
    # column 8j+i in bits 4i..4i+3 as q + 8: word 0 = 0, 15, 8, 7, 9, 0, 15, 11 (low nibble first)
    assert p[0, 0].item() == np.array([0xBF0978F0], dtype=np.uint32).view(np.int32)[0]
    assert torch.equal(unpack_w4(p), q)
    rnd = torch.randint(-8, 8, (32, 256), dtype=torch.int8)
    assert torch.equal(unpack_w4(pack_w4(rnd)), rnd)


# ---------------------------------------------------------------------------------------------------------------------
# compressed-tensors pack-quantized checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def _tiny_cfg():
    from ssd_amd.model_config import ModelConfig
    return ModelConfig("llama", 128, 1, 2, 1, 64, 256, 512)


SHAPES = {"self_attn.q_proj": (128, 128), "self_attn.k_proj": (64, 128), "self_attn.v_proj": (64, 128), "self_attn.o_proj": (128, 128),
          "mlp.gate_proj": (256, 128), "mlp.up_proj": (256, 128), "mlp.down_proj": (128, 256)}
PACKS = {"self_attn.qkv_proj": ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"],
         "mlp.gate_up_proj": ["mlp.gate_proj", "mlp.up_proj"], "self_attn.o_proj": ["self_attn.o_proj"], "mlp.down_proj": ["mlp.down_proj"]}


def _write_w4_ckpt(path, *, scale_dtype=torch.bfloat16, fmt="pack-quantized", symmetric=True, strategy="group", group_size=128,
                   actorder=None, extra=None, seed=0):
    """A one-layer pack-quantized checkpoint with unpacked q/k/v and gate/up (HF names); lm_head, embedding and norms bf16.
    Returns the codes and the scales as the checkpoint stores them (before any rounding of fp16 / fp32 scales)."""
    from safetensors.torch import save_file
    cfg = _tiny_cfg()
    g = torch.Generator().manual_seed(seed)
    h, V = cfg.hidden_size, cfg.vocab_size
    t = {"model.embed_tokens.weight": torch.randn(V, h, generator=g).to(torch.bfloat16),
         "lm_head.weight": torch.randn(V, h, generator=g).to(torch.bfloat16),
         "model.norm.weight": torch.ones(h, dtype=torch.bfloat16),
         P + "input_layernorm.weight": torch.ones(h, dtype=torch.bfloat16),
         P + "post_attention_layernorm.weight": torch.ones(h, dtype=torch.bfloat16)}
    want = {}
    for name, (n, k) in SHAPES.items():
        q = torch.randint(-8, 8, (n, k), generator=g, dtype=torch.int8).numpy()
        s = (torch.rand(n, k // 128, generator=g, dtype=torch.float64) * 3e-3 + 1e-4).to(scale_dtype)
        t[P + name + ".weight_packed"] = torch.from_numpy(R.pack(q))
        t[P + name + ".weight_scale"] = s
        t[P + name + ".weight_shape"] = torch.tensor([n, k], dtype=torch.int64)
        want[name] = (q, s)
    t.update(extra or {})
    save_file(t, os.path.join(path, "model.safetensors"))
    wq = {"num_bits": 4, "type": "int", "symmetric": symmetric, "strategy": strategy, "group_size": group_size, "dynamic": False}
    if actorder is not None:
        wq["actorder"] = actorder
    qc = {"quant_method": "compressed-tensors", "format": fmt, "ignore": ["lm_head"],
          "config_groups": {"group_0": {"targets": ["Linear"], "weights": wq, "input_activations": None}}}
    json.dump({"model_type": "llama", "quantization_config": qc}, open(os.path.join(path, "config.json"), "w"))
    return cfg, t, want


def _scale_bits(s: torch.Tensor) -> np.ndarray:
    """The bf16 bits a loaded scale must have: bf16 as is, fp16 / fp32 rounded to nearest even once."""
    if s.dtype == torch.bfloat16:
        return bits(s)
    return R.bf16_bits(s.float().numpy())


@pytest.mark.parametrize("scale_dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_pack_quantized_loader_keeps_codes_and_scales(tmp_path, scale_dtype):
    from ssd_amd.quant import W4Tensor
    from ssd_amd.weights import load_safetensors, checkpoint_quantization
    cfg, t, want = _write_w4_ckpt(str(tmp_path), scale_dtype=scale_dtype)
    assert checkpoint_quantization(str(tmp_path)) == "w4a16"
    got = dict(load_safetensors(cfg, str(tmp_path), w4a16=True))
    for packed, parts in PACKS.items():
        w = got[P + packed + ".weight"]
        assert isinstance(w, W4Tensor) and w.packed.dtype == torch.int32 and w.scale.dtype == torch.bfloat16
        assert np.array_equal(w.packed.numpy(), R.pack(np.concatenate([want[x][0] for x in parts])))
        assert np.array_equal(bits(w.scale), np.concatenate([_scale_bits(want[x][1]) for x in parts]))
    assert torch.equal(got["lm_head.weight"], t["lm_head.weight"])
    assert not any(k.endswith(("_packed", "_scale", "_shape")) for k in got)


def test_fp16_scales_round_to_nearest_even_bf16(tmp_path):
    """A scale halfway between two bf16 values rounds to the even one (fp16 0x3C01 = 1 + 2^-10 -> bf16 1.0; 1 + 3 * 2^-8 ->
    1 + 2^-6 rounds up to the even mantissa)."""
    from ssd_amd.weights import load_safetensors
    from safetensors.torch import load_file, save_file
    cfg, _, _ = _write_w4_ckpt(str(tmp_path), scale_dtype=torch.float16)
    f = os.path.join(str(tmp_path), "model.safetensors")
    t = load_file(f)
    s = t[P + "self_attn.o_proj.weight_scale"]
    s[0, 0], s[1, 0], s[2, 0] = 1.0 + 2 ** -10, 1.0 + 3 * 2 ** -8, 1.0 + 2 ** -8
    save_file(t, f)
    got = dict(load_safetensors(cfg, str(tmp_path), w4a16=True))[P + "self_attn.o_proj.weight"].scale
    assert got[0, 0].item() == 1.0 and got[1, 0].item() == 1.0 + 2 ** -6 and got[2, 0].item() == 1.0


def test_bf16_target_reads_w4_checkpoint_as_dequantized_and_tp_shards(tmp_path):
    from ssd_amd.weights import load_safetensors, shard_param
    cfg, _, want = _write_w4_ckpt(str(tmp_path))
    full = dict(load_safetensors(cfg, str(tmp_path)))
    deq = {}
    for packed, parts in PACKS.items():
        w = full[P + packed + ".weight"]
        assert w.dtype == torch.bfloat16
        q = np.concatenate([want[x][0] for x in parts])
        s = np.concatenate([bits(want[x][1]) for x in parts])
        assert np.array_equal(bits(w), R.dequant(q, s)), packed
        deq[P + packed + ".weight"] = w
    for rank in range(2):
        sh = dict(load_safetensors(cfg, str(tmp_path), rank, 2))
        for name, w in deq.items():
            assert torch.equal(sh[name], shard_param(cfg, name, w, rank, 2)), (name, rank)


@pytest.mark.parametrize("kw,match", [
    (dict(symmetric=False), "asymmetric"),
    (dict(actorder="weight"), "actorder"),
    (dict(group_size=64), "group_size"),
    (dict(group_size=None, strategy="channel"), "strategy"),
    (dict(fmt="int-quantized"), "format"),
    (dict(extra={P + "self_attn.o_proj.weight_zero_point": torch.zeros(128, 1, dtype=torch.int32)}), "zero point"),
    (dict(extra={P + "self_attn.o_proj.weight_g_idx": torch.zeros(128, dtype=torch.int32)}), "g_idx"),
])
def test_pack_quantized_loader_refuses_other_schemes(tmp_path, kw, match):
    from ssd_amd.weights import load_safetensors
    cfg, _, _ = _write_w4_ckpt(str(tmp_path), **kw)
    for target in (dict(w4a16=True), dict()):
        with pytest.raises(ValueError, match=match):
            list(load_safetensors(cfg, str(tmp_path), **target))


def test_w4_and_fp8_checkpoints_refuse_the_other_target(tmp_path):
    from ssd_amd.weights import load_safetensors
    from tests.test_fp8_cpu import _write_ckpt
    d1, d2 = tmp_path / "w4", tmp_path / "fp8"
    d1.mkdir()
    d2.mkdir()
    cfg, _, _ = _write_w4_ckpt(str(d1))
    with pytest.raises(ValueError, match="fp8 target"):
        list(load_safetensors(cfg, str(d1), fp8=True))
    _write_ckpt(str(d2), _tiny_cfg())
    with pytest.raises(ValueError, match="w4a16 target"):
        list(load_safetensors(_tiny_cfg(), str(d2), w4a16=True))


def test_bf16_checkpoint_into_w4a16_target_yields_bf16_for_on_load_quantization(tmp_path):
    from ssd_amd import weights as W
    from safetensors.torch import save_file
    cfg = _tiny_cfg()
    sd = W.synthetic_state_dict(cfg, seed=1, std=0.02)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(str(tmp_path), "model.safetensors"))
    got = dict(W.load_safetensors(cfg, str(tmp_path), w4a16=True))
    assert all(isinstance(v, torch.Tensor) and v.dtype == torch.bfloat16 for v in got.values())
    assert torch.equal(got[P + "mlp.down_proj.weight"], sd[P + "mlp.down_proj.weight"])


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _built_lib():
    from ssd_amd.hip.lib import build_library, lib_path
    if not os.path.exists(lib_path()):
        build_library()
    return lib_path()


def test_w4_header_symbols_exported_bound_and_documented():
    from ssd_amd.hip.lib import SIGNATURES
    from ssd_amd.hip.quant_ops import QUANT_SIGNATURES
    from ssd_amd.hip.w4_ops import W4_SIGNATURES, load_w4_library
    _built_lib()
    lib = load_w4_library()
    syms = w4_header_symbols()
    assert len(syms) == 5
    assert sorted(W4_SIGNATURES) == syms
    assert not set(syms) & set(SIGNATURES)
    assert not set(syms) & set(QUANT_SIGNATURES)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        assert f"`{s}(" in doc, f"{s} has no line in INTEGRATION.md"
    common = open(os.path.join(ROOT, "ssd_amd", "csrc", "common.h")).read()
    assert '#include "ssd_hip_w4a16.h"' in common
    mk = open(os.path.join(ROOT, "ssd_amd", "csrc", "Makefile")).read()
    assert "gemm_w4a16.hip" in mk and "ssd_hip_w4a16.h" in mk


def test_c_consumer_walks_every_w4_validation_path(tmp_path):
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "w4a16_abi_consumer.c")
    body = open(src).read()
    for s in w4_header_symbols():
        assert f"{s}(" in body, s
    exe = str(tmp_path / "w4a16_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout
