"""MXFP4 weight-only quantization, the parts that need no GPU: the configuration surface, the torch quantizer, packing and exact
dequantization against the numpy restatement (tests/mxfp4_ref.py), the compressed-tensors mxfp4-pack-quantized checkpoint loader and
its refusals, and the C ABI of include/ssd_hip_mxfp4.h (exports, ctypes table, INTEGRATION.md, a plain-C consumer walking every entry
point's argument validation)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests import mxfp4_ref as R

HEADER = os.path.join(ROOT, "include", "ssd_hip_mxfp4.h")
P = "model.layers.0."
BF = torch.bfloat16


def mx4_header_symbols():
    return sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


def bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------
# Config
# ---------------------------------------------------------------------------------------------------------------------
def test_config_accepts_mxfp4():
    from ssd_amd.config import Config
    assert Config("llama-3.1-70b", quantization="mxfp4").quantization == "mxfp4"
    c = Config("llama-3.1-70b", quantization="mxfp4", speculate=True, draft="llama-3.2-1b", speculate_k=4)
    assert c.quantization == "mxfp4"


def test_config_refuses_mxfp4_with_tp_or_eagle_and_other_spellings():
    from ssd_amd.config import Config
    with pytest.raises(ValueError, match="one GPU"):
        Config("llama-3.1-70b", quantization="mxfp4", num_gpus=2)
    with pytest.raises(ValueError, match="use_eagle"):
        Config("llama-3.1-8b", quantization="mxfp4", speculate=True, draft="eagle3-llama-3.1-8b", draft_async=True,
               jit_speculate=True, use_eagle=True)
    for bad in ("fp4", "MXFP4", "mx4"):
        with pytest.raises(ValueError, match="quantization"):
            Config("llama-3.1-8b", quantization=bad)


def test_decoder_refuses_mxfp4_off_the_128_grid():
    from ssd_amd.model import HipDecoder
    from ssd_amd.model_config import ModelConfig
    cfg = ModelConfig("llama", 64, 1, 2, 1, 32, 128, 256)
    with pytest.raises(ValueError, match="multiples of 128"):
        HipDecoder(cfg, max_tokens=16, max_seqs=1, max_blocks=2, block_size=16, max_model_len=64, device=torch.device("cpu"),
                   quantization="mxfp4")


# ---------------------------------------------------------------------------------------------------------------------
# Quantizer, packing, dequantization
# ---------------------------------------------------------------------------------------------------------------------
TIES = [(0.25, 0), (0.75, 2), (1.25, 2), (1.75, 4), (2.5, 4), (3.5, 6), (5.0, 6)]     # scaled magnitude -> code (values 0, 1, 1, 2, 2, 4, 4)


def _constructed():
    """[16, 256] bf16: one constructed 32-column block per (row, block) cell, the rest small noise with a block amax of 4 .. 8."""
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(16, 256, generator=g) * 0.02).to(BF)
    # row 0, block 0: amax 4 -> scale 2^0 = 1 (b = 127): every tie, both signs, at scale 1
    w[0, :32] = 0
    w[0, 0] = 4.0
    for i, (m, _) in enumerate(TIES):
        w[0, 1 + 2 * i], w[0, 2 + 2 * i] = m, -m
    # row 1, block 0: the same ties at scale 2^-7 (amax 4 * 2^-7)
    w[1, :32] = w[0, :32] * 2.0 ** -7
    w[2, 32:64] = 0                                       # a zero block: b = 127, codes 0
    w[3, :32] = 0
    w[3, 5] = 2.0 ** -5                                   # amax an exact power of two: b = -5 - 2 + 127 = 120, the element = 4 -> code 6
    # row 4: saturation.  amax 7.5 -> floor(log2) = 2 -> scale 1; 6.5, 7, 7.5 all lie above 6 -> code 7, -7.5 -> code 15
    w[4, :32] = 0
    w[4, 0:4] = torch.tensor([6.5, 7.0, 7.5, -7.5], dtype=BF)
    # row 5: bf16 subnormals only (2^-133 .. 2^-127): the b >= 2 clamp
    w[5, :32] = 0
    w[5, 0:3] = torch.tensor([2.0 ** -133, -(2.0 ** -127), 2.0 ** -130], dtype=torch.float64).to(BF)
    # row 6: amax at the top of the bf16 range: exponent field 254 -> b = 252
    w[6, :32] = 0
    w[6, 0:2] = torch.tensor([3.3895313892515355e38, -1.0e38], dtype=torch.float64).to(BF)
    return w


def test_quantizer_bit_exact_against_numpy_random_and_constructed_blocks():
    from ssd_amd.quant import quantize_mxfp4, dequantize_mxfp4, unpack_mxfp4, MX4Tensor
    g = torch.Generator().manual_seed(5)
    for w in ((torch.randn(48, 512, generator=g) * 0.03).to(BF), (torch.randn(32, 256, generator=g) * 3.0).to(BF), _constructed()):
        t = quantize_mxfp4(w)
        assert isinstance(t, MX4Tensor) and t.packed.dtype == torch.uint8 and t.scale.dtype == torch.uint8
        assert tuple(t.packed.shape) == (w.shape[0], w.shape[1] // 2) and tuple(t.scale.shape) == (w.shape[0], w.shape[1] // 32)
        c_ref, b_ref = R.quantize(w)
        assert np.array_equal(t.scale.numpy(), b_ref)
        assert np.array_equal(unpack_mxfp4(t.packed).numpy(), c_ref)
        assert np.array_equal(t.packed.numpy(), R.pack(c_ref))
        assert int(t.scale.min()) >= 2 and int(t.scale.max()) <= 252
        assert np.array_equal(bits(dequantize_mxfp4(t.packed, t.scale)), R.bf16_bits_exact(R.exact(c_ref, b_ref)))
    w = _constructed()
    t = quantize_mxfp4(w)
    q, b = unpack_mxfp4(t.packed), t.scale
    assert b[0, 0].item() == 127 and b[1, 0].item() == 120
    for row in (0, 1):
        assert q[row, 0].item() == 6
        for i, (_, code) in enumerate(TIES):
            assert q[row, 1 + 2 * i].item() == code and q[row, 2 + 2 * i].item() == (code | 8), (row, i)
    assert b[2, 1].item() == 127 and (q[2, 32:64] == 0).all()
    assert b[3, 0].item() == 120 and q[3, 5].item() == 6
    assert b[4, 0].item() == 127 and q[4, :4].tolist() == [7, 7, 7, 15]
    assert b[5, 0].item() == 2
    assert b[6, 0].item() == 252
    # the error of one element, from the format alone: a = |w| / 2^(b - 127) lies in [0, 8) (b is floor(log2(amax)) - 2).  Up to a = 6
    # rounding to nearest leaves at most half the widest e2m1 step, 1; above 6 the code saturates at 6 and leaves a - 6 < 2.
    wr = (torch.randn(48, 512, generator=g) * 0.03).to(BF)
    tr = quantize_mxfp4(wr)
    sc = torch.exp2(tr.scale.float() - 127).repeat_interleave(32, dim=1)
    a = wr.float().abs() / sc
    err = (dequantize_mxfp4(*tr).float() - wr.float()).abs() / sc
    assert bool((a < 8).all()) and bool((a > 6).any())
    assert bool((err[a <= 6] <= 1).all())
    assert bool((err[a > 6] == a[a > 6] - 6).all())


def test_pack_unpack_all_codes_in_both_nibbles_and_exact_dequant_for_every_scale():
    from ssd_amd.quant import pack_mxfp4, unpack_mxfp4, dequantize_mxfp4
    # [16 rows = the code in the low nibble][128 columns]: column 2j holds the row's code, column 2j+1 holds code j % 16
    codes = torch.zeros(16, 128, dtype=torch.uint8)
    codes[:, 0::2] = torch.arange(16, dtype=torch.uint8)[:, None]
    codes[:, 1::2] = (torch.arange(64) % 16).to(torch.uint8)[None, :]
    p = pack_mxfp4(codes)
    assert p.dtype == torch.uint8 and tuple(p.shape) == (16, 64)
    assert p[3, 5].item() == 3 | (5 << 4)                # byte j: column 2j in bits 0..3, column 2j+1 in bits 4..7
    assert np.array_equal(p.numpy(), R.pack(codes.numpy()))
    assert torch.equal(unpack_mxfp4(p), codes) and np.array_equal(R.unpack(p.numpy()), codes.numpy())
    for b0 in range(2, 253, 4):
        sc = torch.tensor([[min(b0 + j, 252) for j in range(4)]] * 16, dtype=torch.uint8)
        got = dequantize_mxfp4(p, sc)
        want = R.exact(codes.numpy(), sc.numpy())
        assert got.dtype == BF and np.array_equal(got.double().numpy(), want), b0
        assert np.array_equal(bits(got), R.bf16_bits_exact(want))


# ---------------------------------------------------------------------------------------------------------------------
# compressed-tensors mxfp4-pack-quantized checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def _tiny_cfg():
    from ssd_amd.model_config import ModelConfig
    return ModelConfig("llama", 128, 1, 2, 1, 64, 256, 512)


SHAPES = {"self_attn.q_proj": (128, 128), "self_attn.k_proj": (64, 128), "self_attn.v_proj": (64, 128), "self_attn.o_proj": (128, 128),
          "mlp.gate_proj": (256, 128), "mlp.up_proj": (256, 128), "mlp.down_proj": (128, 256)}
PACKS = {"self_attn.qkv_proj": ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"],
         "mlp.gate_up_proj": ["mlp.gate_proj", "mlp.up_proj"], "self_attn.o_proj": ["self_attn.o_proj"], "mlp.down_proj": ["mlp.down_proj"]}


def _write_mx4_ckpt(path, *, fmt="mxfp4-pack-quantized", group_size=32, scale_dtype=None, scale_tensor_dtype=torch.uint8, extra=None,
                    poke=None, seed=0):
    """A one-layer MXFP4 checkpoint with unpacked q/k/v and gate/up (HF names); lm_head, embedding and norms bf16."""
    from safetensors.torch import save_file
    cfg = _tiny_cfg()
    g = torch.Generator().manual_seed(seed)
    h, V = cfg.hidden_size, cfg.vocab_size
    t = {"model.embed_tokens.weight": torch.randn(V, h, generator=g).to(BF),
         "lm_head.weight": torch.randn(V, h, generator=g).to(BF),
         "model.norm.weight": torch.ones(h, dtype=BF),
         P + "input_layernorm.weight": torch.ones(h, dtype=BF),
         P + "post_attention_layernorm.weight": torch.ones(h, dtype=BF)}
    want = {}
    for name, (n, k) in SHAPES.items():
        codes = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8).numpy()
        b = torch.randint(112, 126, (n, k // 32), generator=g, dtype=torch.uint8)
        if poke is not None and name == "self_attn.o_proj":
            b[1, 2] = poke
        t[P + name + ".weight_packed"] = torch.from_numpy(R.pack(codes))
        t[P + name + ".weight_scale"] = b if scale_tensor_dtype == torch.uint8 else b.float().to(scale_tensor_dtype)
        want[name] = (codes, b.numpy())
    t.update(extra or {})
    save_file(t, os.path.join(path, "model.safetensors"))
    wq = {"num_bits": 4, "type": "float", "symmetric": True, "strategy": "group", "group_size": group_size, "dynamic": False}
    if scale_dtype is not None:
        wq["scale_dtype"] = scale_dtype
    qc = {"quant_method": "compressed-tensors", "format": fmt, "ignore": ["lm_head"],
          "config_groups": {"group_0": {"targets": ["Linear"], "weights": wq, "input_activations": None}}}
    json.dump({"model_type": "llama", "quantization_config": qc}, open(os.path.join(path, "config.json"), "w"))
    return cfg, t, want


def test_mxfp4_loader_keeps_codes_and_scales_bit_for_bit(tmp_path):
    from ssd_amd.quant import MX4Tensor
    from ssd_amd.weights import load_safetensors, checkpoint_quantization
    cfg, t, want = _write_mx4_ckpt(str(tmp_path))
    assert checkpoint_quantization(str(tmp_path)) == "mxfp4"
    got = dict(load_safetensors(cfg, str(tmp_path), mxfp4=True))
    for packed, parts in PACKS.items():
        w = got[P + packed + ".weight"]
        assert isinstance(w, MX4Tensor) and w.packed.dtype == torch.uint8 and w.scale.dtype == torch.uint8
        assert np.array_equal(w.packed.numpy(), R.pack(np.concatenate([want[x][0] for x in parts])))
        assert np.array_equal(w.scale.numpy(), np.concatenate([want[x][1] for x in parts]))
    assert torch.equal(got["lm_head.weight"], t["lm_head.weight"])
    assert not any(k.endswith(("_packed", "_scale")) for k in got)


def test_bf16_target_reads_mxfp4_checkpoint_as_the_exact_matrix_and_tp_shards(tmp_path):
    from ssd_amd.weights import load_safetensors, shard_param
    cfg, _, want = _write_mx4_ckpt(str(tmp_path))
    full = dict(load_safetensors(cfg, str(tmp_path)))
    deq = {}
    for packed, parts in PACKS.items():
        w = full[P + packed + ".weight"]
        assert w.dtype == BF
        ex = R.exact(np.concatenate([want[x][0] for x in parts]), np.concatenate([want[x][1] for x in parts]))
        assert np.array_equal(bits(w), R.bf16_bits_exact(ex)), packed
        deq[P + packed + ".weight"] = w
    for rank in range(2):
        sh = dict(load_safetensors(cfg, str(tmp_path), rank, 2))
        for name, w in deq.items():
            assert torch.equal(sh[name], shard_param(cfg, name, w, rank, 2)), (name, rank)


@pytest.mark.parametrize("kw,match", [
    (dict(group_size=16), "NVFP4"),
    (dict(fmt="nvfp4-pack-quantized"), "NVFP4"),
    (dict(scale_dtype="torch.float8_e4m3fn"), "scale_dtype"),
    (dict(scale_tensor_dtype=torch.float8_e4m3fn), "weight_scale is"),
    (dict(extra={P + "self_attn.o_proj.weight_global_scale": torch.ones(1)}), "weight_global_scale"),
    (dict(poke=0), r"o_proj\.weight_scale.*scale byte 0 "),
    (dict(poke=1), r"o_proj\.weight_scale.*scale byte 1 "),
    (dict(poke=253), r"o_proj\.weight_scale.*scale byte 253 "),
    (dict(poke=255), r"o_proj\.weight_scale.*scale byte 255 "),
])
def test_mxfp4_loader_refuses_other_float4_schemes_and_scale_bytes_out_of_range(tmp_path, kw, match):
    from ssd_amd.weights import load_safetensors
    cfg, _, _ = _write_mx4_ckpt(str(tmp_path), **kw)
    for target in (dict(mxfp4=True), dict()):
        with pytest.raises(ValueError, match=match):
            list(load_safetensors(cfg, str(tmp_path), **target))


def test_mxfp4_checkpoints_and_the_other_quantized_targets_refuse_each_other(tmp_path):
    from ssd_amd.weights import load_safetensors
    from tests.test_fp8_cpu import _write_ckpt
    from tests.test_w4a16_cpu import _write_w4_ckpt
    d1, d2, d3 = tmp_path / "mx4", tmp_path / "fp8", tmp_path / "w4"
    for d in (d1, d2, d3):
        d.mkdir()
    cfg, _, _ = _write_mx4_ckpt(str(d1))
    with pytest.raises(ValueError, match="fp8 target"):
        list(load_safetensors(cfg, str(d1), fp8=True))
    with pytest.raises(ValueError, match="w4a16 target"):
        list(load_safetensors(cfg, str(d1), w4a16=True))
    _write_ckpt(str(d2), _tiny_cfg())
    with pytest.raises(ValueError, match="mxfp4 target"):
        list(load_safetensors(_tiny_cfg(), str(d2), mxfp4=True))
    _write_w4_ckpt(str(d3))
    with pytest.raises(ValueError, match="mxfp4 target"):
        list(load_safetensors(_tiny_cfg(), str(d3), mxfp4=True))


def test_bf16_checkpoint_into_mxfp4_target_yields_bf16_for_on_load_quantization(tmp_path):
    from ssd_amd import weights as W
    from safetensors.torch import save_file
    cfg = _tiny_cfg()
    sd = W.synthetic_state_dict(cfg, seed=1, std=0.02)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(str(tmp_path), "model.safetensors"))
    got = dict(W.load_safetensors(cfg, str(tmp_path), mxfp4=True))
    assert all(isinstance(v, torch.Tensor) and v.dtype == BF for v in got.values())
    assert torch.equal(got[P + "mlp.down_proj.weight"], sd[P + "mlp.down_proj.weight"])


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _built_lib():
    from ssd_amd.hip.lib import build_library, lib_path
    if not os.path.exists(lib_path()):
        build_library()
    return lib_path()


def test_mx4_header_symbols_exported_bound_and_documented():
    from ssd_amd.hip.lib import SIGNATURES
    from ssd_amd.hip.quant_ops import QUANT_SIGNATURES
    from ssd_amd.hip.w4_ops import W4_SIGNATURES
    from ssd_amd.hip.mx4_ops import MX4_SIGNATURES, load_mx4_library
    _built_lib()
    lib = load_mx4_library()
    syms = mx4_header_symbols()
    assert len(syms) == 5
    assert sorted(MX4_SIGNATURES) == syms
    assert not set(syms) & (set(SIGNATURES) | set(QUANT_SIGNATURES) | set(W4_SIGNATURES))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        assert f"`{s}(" in doc, f"{s} has no line in INTEGRATION.md"
    common = open(os.path.join(ROOT, "ssd_amd", "csrc", "common.h")).read()
    assert '#include "ssd_hip_mxfp4.h"' in common
    mk = open(os.path.join(ROOT, "ssd_amd", "csrc", "Makefile")).read()
    assert "gemm_mxfp4.hip" in mk and "ssd_hip_mxfp4.h" in mk


def test_c_consumer_walks_every_mx4_validation_path(tmp_path):
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "mxfp4_abi_consumer.c")
    body = open(src).read()
    for s in mx4_header_symbols():
        assert f"{s}(" in body, s
    exe = str(tmp_path / "mxfp4_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout
