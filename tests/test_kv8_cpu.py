"""FP8 KV cache, the parts that need no GPU: the format in torch (ssd_amd/quant.py against torch's own table and against the
restatement in tests/kv8_ref.py), the configuration surface, the decoder's cache bytes, and the C ABI of include/ssd_hip_kv8.h
(exports, ctypes table, INTEGRATION.md, a plain-C consumer walking every entry point's argument validation)."""
import os
import re
import subprocess

import pytest
import torch

from tests.conftest import ROOT
from tests import kv8_ref

HEADER = os.path.join(ROOT, "include", "ssd_hip_kv8.h")
BF = torch.bfloat16


def kv8_header_symbols():
    return sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


# ---------------------------------------------------------------------------------------------------------------------
# Format
# ---------------------------------------------------------------------------------------------------------------------
def test_decode_of_all_256_codes_is_torchs_table_and_the_bit_field_table():
    from ssd_amd.quant import kv_fp8_decode
    codes = torch.arange(256, dtype=torch.uint8)
    got = kv_fp8_decode(codes, 1.0)
    want = codes.view(torch.float8_e4m3fn).float()
    assert got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))        # bit compare: NaN codes and -0.0 included
    nan = torch.isnan(got)
    assert nan.nonzero().flatten().tolist() == [0x7F, 0xFF]
    ref = kv8_ref.decode(codes, 1.0)
    assert torch.equal(got[~nan].view(torch.int32), ref[~nan].view(torch.int32)) and torch.isnan(ref[nan]).all()
    assert got[~nan].abs().max() == 448.0
    # every code is an exact bf16 value
    assert torch.equal(got[~nan].to(BF).float(), got[~nan])


@pytest.mark.parametrize("scale", [1.0, 0.5, 2.0])
def test_encode_inverts_decode_on_the_254_finite_codes(scale):
    from ssd_amd.quant import kv_fp8_encode, kv_fp8_decode
    c = kv8_ref.FINITE_CODES
    assert c.numel() == 254
    x = kv_fp8_decode(c, scale)
    assert torch.equal(x.to(BF).float(), x)           # a power-of-two scale keeps the value a bf16 value
    for enc in (kv_fp8_encode, kv8_ref.encode):
        assert torch.equal(enc(x.to(BF), 1.0 / scale), c)


def test_saturation_negative_zero_and_the_tie_to_even():
    from ssd_amd.quant import kv_fp8_encode, kv_fp8_decode
    x = torch.tensor([500.0, -1000.0, 460.0, 448.0, -448.0, -0.0, 0.0, 2.0 ** -10, -(2.0 ** -10), 3 * 2.0 ** -10, 2.0 ** -9],
                     dtype=BF)
    want = [0x7E, 0xFE, 0x7E, 0x7E, 0xFE, 0x80, 0x00, 0x00, 0x80, 0x02, 0x01]
    for enc in (kv_fp8_encode, kv8_ref.encode):
        assert enc(x, 1.0).tolist() == want
    # torch's cast alone does not saturate: the clamp in front of it is part of the definition
    assert torch.isnan(torch.tensor([500.0]).to(torch.float8_e4m3fn).float()).all()
    # with a scale: +-448 * s saturate exactly, 2^-10 * s is the tie that rounds to zero
    for s in (0.5, 2.0, 0.37, 1.9):
        sb = torch.tensor([448.0 * s, -448.0 * s, 1000.0, 2.0 ** -10 * s], dtype=torch.float32)
        inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(s, dtype=torch.float32)
        codes = kv_fp8_encode(sb.to(BF), inv)
        assert codes[2].item() == 0x7E and not torch.isnan(kv_fp8_decode(codes, s)).any()
        assert torch.equal(codes, kv8_ref.encode(sb.to(BF), inv))
    # a finite input never produces a NaN code
    g = torch.Generator().manual_seed(0)
    y = (torch.randn(4096, generator=g) * 300).to(BF)
    c = kv_fp8_encode(y, 1.0)
    assert not ((c == 0x7F) | (c == 0xFF)).any()
    assert torch.equal(c, kv8_ref.encode(y, 1.0))


def test_per_head_scales_broadcast_over_the_cache_layout():
    from ssd_amd.quant import kv_fp8_encode, kv_fp8_decode
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(3, 2, 16, 64, generator=g) * 2).to(BF)         # [pages][nkv][block][hd]
    s = torch.tensor([0.37, 1.9]).view(1, 2, 1, 1)
    c = kv_fp8_encode(x, 1.0 / s)
    assert c.shape == x.shape and c.dtype == torch.uint8
    for h in range(2):
        assert torch.equal(c[:, h], kv8_ref.encode(x[:, h], 1.0 / s[0, h, 0, 0]))
    y = kv_fp8_decode(c, s)
    # in units of the scale: half an ulp is at most 2^-4 of the value (3 mantissa bits), and 2^-10 below the smallest normal 2^-6
    # (subnormal spacing 2^-9); the 1e-6 covers the fp32 rounding of x * (1 / s)
    err, mag = (y - x.float()).abs() / s, x.float().abs() / s
    assert (err <= torch.maximum(mag * 2.0 ** -4, torch.tensor(2.0 ** -10)) * (1 + 1e-6)).all()


# ---------------------------------------------------------------------------------------------------------------------
# Config / decoder
# ---------------------------------------------------------------------------------------------------------------------
def test_config_accepts_fp8_kv_with_every_weight_mode_and_defaults_to_none():
    from dataclasses import fields
    from ssd_amd.config import Config
    assert "kv_cache_dtype" in {f.name for f in fields(Config)}
    assert Config("llama-3.1-70b").kv_cache_dtype is None
    assert Config("llama-3.1-70b", kv_cache_dtype=None).kv_cache_dtype is None
    for q in (None, "fp8", "w4a16", "mxfp4"):
        c = Config("llama-3.1-70b", kv_cache_dtype="fp8", quantization=q, speculate=True, draft="llama-3.2-1b", speculate_k=4)
        assert c.kv_cache_dtype == "fp8" and c.quantization == q
    assert Config("llama-3.1-70b", kv_cache_dtype="fp8", quantization="w4a16", w4_zero_point=True).w4_zero_point


def test_config_refuses_other_dtypes_tensor_parallel_and_eagle_by_name():
    from ssd_amd.config import Config
    for bad in ("fp8_e5m2", "int8", "bf16", "auto"):
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            Config("llama-3.1-8b", kv_cache_dtype=bad)
    with pytest.raises(ValueError, match="kv_cache_dtype.*one GPU"):
        Config("llama-3.1-70b", kv_cache_dtype="fp8", num_gpus=2)
    with pytest.raises(ValueError, match="kv_cache_dtype.*use_eagle"):
        Config("llama-3.1-8b", kv_cache_dtype="fp8", speculate=True, draft="eagle3-llama-3.1-8b", draft_async=True,
               jit_speculate=True, use_eagle=True)
    # the unchanged defaults still construct
    assert Config("llama-3.1-70b", num_gpus=2).kv_cache_dtype is None
    assert Config("llama-3.1-8b", speculate=True, draft="eagle3-llama-3.1-8b", draft_async=True, jit_speculate=True,
                  use_eagle=True).kv_cache_dtype is None


def test_decoder_cache_bytes_halve_and_the_kv_forms_are_off():
    from ssd_amd.model import HipDecoder
    from ssd_amd.model_config import ModelConfig
    cfg = ModelConfig("llama", 128, 2, 2, 1, 64, 256, 512)
    kw = dict(max_tokens=32, max_seqs=1, max_blocks=4, block_size=16, max_model_len=64, device=torch.device("cpu"))
    a, b = HipDecoder(cfg, **kw), HipDecoder(cfg, kv_cache_dtype="fp8", **kw)
    assert HipDecoder(cfg, kv_cache_dtype=None, **kw).kv_block_bytes() == a.kv_block_bytes()
    assert 2 * b.kv_block_bytes() == a.kv_block_bytes() == 2 * 2 * 16 * 1 * 64 * 2
    assert b.kv8 and not a.kv8 and a.kv_scale is None
    a.alloc_kv(3)
    b.alloc_kv(3)
    assert a.kv_cache.dtype == BF and b.kv_cache.dtype == torch.uint8 and a.kv_cache.shape == b.kv_cache.shape == (2, 2, 3, 1, 16, 64)
    assert b.kv_cache.numel() * b.kv_cache.element_size() == 3 * b.kv_block_bytes()
    # every form that writes or reads KV inside another kernel is off, at every row count
    assert not (b.chain_seg or b.tree_seg or b.fuse_attn_o)
    assert all(b.fusion_plan(T) == (False, False) for T in (1, 8, 16, 17, 32))
    assert b.use_parts == a.use_parts                     # what does not touch KV stays as for a bf16-weight target
    # scales: 1.0 until set; the inverse is the host's fp32 reciprocal; the tables are written in place
    assert torch.equal(b.kv_scale, torch.ones(2, 2, 1)) and torch.equal(b.kv_inv_scale, torch.ones(2, 2, 1))
    ps, pi = b.kv_scale.data_ptr(), b.kv_inv_scale.data_ptr()
    b.set_kv_scales(torch.tensor([[0.37], [2.0]]), torch.tensor([[1.9], [0.5]]))
    assert (b.kv_scale.data_ptr(), b.kv_inv_scale.data_ptr()) == (ps, pi)
    assert b.kv_scale[:, 0, 0].tolist() == torch.tensor([0.37, 2.0]).tolist()
    assert torch.equal(b.kv_inv_scale, 1.0 / b.kv_scale)
    with pytest.raises(ValueError, match="positive"):
        b.set_kv_scales(torch.zeros(2, 1), torch.ones(2, 1))
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        a.set_kv_scales(torch.ones(2, 1), torch.ones(2, 1))
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        HipDecoder(cfg, kv_cache_dtype="int8", **kw)
    with pytest.raises(ValueError, match="head_dim"):
        HipDecoder(ModelConfig("llama", 512, 1, 2, 1, 256, 256, 512), kv_cache_dtype="fp8", **kw)


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _built_lib():
    from ssd_amd.hip.lib import build_library, lib_path
    if not os.path.exists(lib_path()):
        build_library()
    return lib_path()


def test_kv8_header_symbols_exported_bound_and_documented():
    from ssd_amd.hip.lib import SIGNATURES
    from ssd_amd.hip.kv8_ops import KV8_SIGNATURES, load_kv8_library
    _built_lib()
    lib = load_kv8_library()
    syms = kv8_header_symbols()
    assert syms == ["ssd_attn_paged_fp8", "ssd_attn_prefill_varlen_fp8", "ssd_kv_fp8_dequant", "ssd_rope_store_kv_fp8"]
    assert sorted(KV8_SIGNATURES) == syms
    assert not set(syms) & set(SIGNATURES)             # lib.SIGNATURES stays exactly ssd_hip.h + ssd_hip_tune.h
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    head = open(HEADER).read()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        assert f"`{s}(" in doc, f"{s} has no line in INTEGRATION.md"
        # the ctypes table has one entry per parameter of the declaration
        decl = re.search(r"^int\s+" + s + r"\s*\(([^;]*)\);", head, flags=re.M | re.S).group(1)
        assert len(KV8_SIGNATURES[s]) == len(decl.split(",")), s
    common = open(os.path.join(ROOT, "ssd_amd", "csrc", "common.h")).read()
    assert '#include "ssd_hip_kv8.h"' in common
    mk = open(os.path.join(ROOT, "ssd_amd", "csrc", "Makefile")).read()
    assert mk.count("../../include/ssd_hip_kv8.h") == 2        # the product and the trace objects both depend on it


def test_c_consumer_walks_every_kv8_validation_path(tmp_path):
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "kv8_abi_consumer.c")
    body = open(src).read()
    for s in kv8_header_symbols():
        assert f"{s}(" in body, s
    for what in ("hd 256", "mode 1", "splits without workspaces", "null"):
        assert what in body
    exe = str(tmp_path / "kv8_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout
