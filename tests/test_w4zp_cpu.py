"""W4A16 with zero points, the parts that need no GPU: the torch quantizer and packing against the numpy restatement
(tests/w4zp_ref.py), the AutoAWQ and GPTQ checkpoint loaders and their refusals, the configuration keyword, and the C ABI of
include/ssd_hip_w4zp.h (exports, ctypes table, INTEGRATION.md, a plain-C consumer walking every entry point's argument validation)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests import w4zp_ref as R
from tests.test_w4a16_cpu import bits, _tiny_cfg, SHAPES, PACKS, P, _built_lib

HEADER = os.path.join(ROOT, "include", "ssd_hip_w4zp.h")


def w4zp_header_symbols():
    return sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


# ---------------------------------------------------------------------------------------------------------------------
# Config
# ---------------------------------------------------------------------------------------------------------------------
def test_config_w4_zero_point_needs_w4a16():
    from ssd_amd.config import Config
    assert Config("llama-3.1-70b", quantization="w4a16", w4_zero_point=True).w4_zero_point is True
    assert Config("llama-3.1-70b", quantization="w4a16").w4_zero_point is False
    for q in (None, "fp8", "mxfp4"):
        with pytest.raises(ValueError, match="w4_zero_point"):
            Config("llama-3.1-8b", quantization=q, w4_zero_point=True)
    with pytest.raises(ValueError, match="one GPU"):
        Config("llama-3.1-70b", quantization="w4a16", w4_zero_point=True, num_gpus=2)


# ---------------------------------------------------------------------------------------------------------------------
# Quantizer and packing
# ---------------------------------------------------------------------------------------------------------------------
def _quantizer_input():
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(48, 512, generator=g) * 0.03).to(torch.bfloat16)
    w[1] += 0.02                                         # a shifted row: the zero point moves off 8
    w[2, 128:256] = 0                                    # all-equal groups: 0, a positive and a negative value
    w[3, 0:128] = 0.0173
    w[4, 256:384] = -3.5
    w[5, :] = 0
    w[6, 0:128] = w[6, 0:128].abs()                      # an all-positive group (z = 0) and an all-negative one (z = 15)
    w[6, 128:256] = -w[6, 128:256].abs()
    # range 15 -> s = 1 exactly; w / s lands on .5 and must round to even
    w[7, 0:8] = torch.tensor([-7.0, 8.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5], dtype=torch.bfloat16)
    w[7, 8:128] = 0
    w[9, 0] = 3.0                                        # an outlier group
    return w


def test_zp_quantizer_bit_exact_against_numpy():
    from ssd_amd.quant import quantize_w4a16_zp, dequantize_w4zp, unpack_w4u, W4ZTensor
    w = _quantizer_input()
    t = quantize_w4a16_zp(w)
    u_ref, s_ref, z_ref = R.quantize(w)
    assert isinstance(t, W4ZTensor)
    assert t.packed.dtype == torch.int32 and tuple(t.packed.shape) == (48, 64)
    assert t.scale.dtype == torch.bfloat16 and tuple(t.scale.shape) == (48, 4)
    assert t.zero.dtype == torch.uint8 and tuple(t.zero.shape) == (48, 4)
    assert np.array_equal(t.packed.numpy(), R.pack(u_ref))
    assert np.array_equal(bits(t.scale), s_ref)
    assert np.array_equal(t.zero.numpy(), z_ref)
    u = unpack_w4u(t.packed)
    assert np.array_equal(u.numpy(), u_ref) and int(u.max()) <= 15 and int(t.zero.max()) <= 15
    assert np.array_equal(bits(dequantize_w4zp(*t)), R.dequant(u_ref, s_ref, z_ref))
    assert t.zero[6, 0].item() == 0 and t.zero[6, 1].item() == 15
    assert t.scale[7, 0].item() == 1.0 and t.zero[7, 0].item() == 7
    assert u[7, :8].tolist() == [0, 15, 7, 9, 9, 7, 5, 5]          # rne(.5) = 0, rne(1.5) = 2, rne(2.5) = 2, and their negatives
    # half a step of the group's scale bounds the error away from the clamp (the zero point is itself rounded, so the two ends of
    # the range may clip by up to another half step), plus the bf16 rounding of the product
    wg = w.float().reshape(48, 4, 128)
    err = (dequantize_w4zp(*t).float().reshape(48, 4, 128) - wg).abs().amax(-1)
    assert bool((err <= t.scale.float() * 1.0 + wg.abs().amax(-1) * 2 ** -8).all())


def test_all_equal_groups_are_exact():
    """An all-equal group of value c takes the range 15 |c|: s = |c| exactly and u - z = sign(c), so the group survives bit for
    bit (c = 0 included)."""
    from ssd_amd.quant import quantize_w4a16_zp, dequantize_w4zp
    for c in (0.0, 0.0173, -3.5, 2.0 ** -20, -1e-30):
        w = torch.full((16, 256), c).to(torch.bfloat16)
        w[:, 128:] = torch.randn(16, 128).to(torch.bfloat16)
        t = quantize_w4a16_zp(w)
        d = dequantize_w4zp(*t)
        assert torch.equal(d[:, :128], w[:, :128]), c
        if c != 0:
            assert bool((t.scale[:, 0].float() == abs(w[0, 0].float())).all())


def test_round_trip_is_exact_on_representable_weights():
    """Weights built as s * (u - z) with power-of-two scales dequantize to themselves, and packing is the identity on the codes."""
    from ssd_amd.quant import W4ZTensor, dequantize_w4zp, pack_w4u, unpack_w4u, W4Tensor, dequantize_w4a16
    g = torch.Generator().manual_seed(3)
    u = torch.randint(0, 16, (32, 256), generator=g, dtype=torch.uint8)
    u[0, :16] = torch.arange(16, dtype=torch.uint8)
    z = torch.randint(0, 16, (32, 2), generator=g, dtype=torch.uint8)
    z[0, 0], z[1, 0] = 0, 15
    s = (2.0 ** torch.randint(-12, -4, (32, 2), generator=g).float()).to(torch.bfloat16)
    p = pack_w4u(u)
    assert np.array_equal(p.numpy(), R.pack(u.numpy())) and torch.equal(unpack_w4u(p), u)
    # column 8j+i in bits 4i..4i+3: word 0 of row 0 holds codes 0..7, low nibble first
    assert p[0, 0].item() == 0x76543210
    d = dequantize_w4zp(p, s, z)
    want = R.weights_f64(u.numpy(), bits(s), z.numpy())
    assert np.array_equal(d.double().numpy(), want)
    # z = 8 everywhere is the symmetric format
    z8 = torch.full_like(z, 8)
    assert torch.equal(dequantize_w4zp(p, s, z8), dequantize_w4a16(*W4Tensor(p, s)))


def test_zero_point_quantizer_beats_the_symmetric_one():
    from ssd_amd.quant import quantize_w4a16, dequantize_w4a16, quantize_w4a16_zp, dequantize_w4zp
    g = torch.Generator().manual_seed(0)
    w = (0.02 * torch.randn(512, 4096, generator=g)).to(torch.bfloat16)
    wf = w.float()

    def rel(d):
        return ((d.float() - wf).norm() / wf.norm()).item()

    e_zp, e_sym = rel(dequantize_w4zp(*quantize_w4a16_zp(w))), rel(dequantize_w4a16(*quantize_w4a16(w)))
    print(f"relative Frobenius error: zero-point {e_zp:.4f}, symmetric {e_sym:.4f}")
    assert e_zp < e_sym


# ---------------------------------------------------------------------------------------------------------------------
# AutoAWQ / GPTQ checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def write_int4_ckpt(path, kind, *, seed=0, cfg=None, shapes=None, qc_over=None, g_idx=None, sym=None, skip=(), layers=1,
                    float_dtype=torch.float16):
    """A checkpoint in the format `kind` ("awq", "gptq", "gptq_v2", "gptq_sym") with unpacked q/k/v and gate/up (HF names); the LM
    head, the embedding and the norms are fp16.  Linears named in `skip` are stored as an unquantized fp16 .weight.  Returns
    (cfg, tensors, want); g_idx: K -> the g_idx tensor to store instead of k // 128; want[layer prefix + name] = (u uint8 [N, K], scales fp16 [N, K/128] as stored, z uint8 [N, K/128])."""
    from safetensors.torch import save_file
    cfg = cfg or _tiny_cfg()
    shapes = shapes or SHAPES
    g = torch.Generator().manual_seed(seed)
    h, V = cfg.hidden_size, cfg.vocab_size
    t = {"model.embed_tokens.weight": torch.randn(V, h, generator=g).to(float_dtype),
         "lm_head.weight": (torch.randn(V, h, generator=g) * 0.05).to(float_dtype),
         "model.norm.weight": (1 + 0.1 * torch.randn(h, generator=g)).to(float_dtype)}
    want = {}
    for li in range(layers):
        lp = f"model.layers.{li}."
        t[lp + "input_layernorm.weight"] = (1 + 0.1 * torch.randn(h, generator=g)).to(float_dtype)
        t[lp + "post_attention_layernorm.weight"] = (1 + 0.1 * torch.randn(h, generator=g)).to(float_dtype)
        for name, (n, k) in shapes.items():
            u = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8).numpy()
            z = torch.randint(0, 16, (n, k // 128), generator=g, dtype=torch.uint8).numpy()
            if kind == "gptq_sym":
                z[:] = 8
            else:
                z[0, 0], z[1, 0] = 0, 15
            s = (torch.rand(n, k // 128, generator=g, dtype=torch.float64) * 3e-3 + 1e-4).to(torch.float16).numpy()
            want[lp + name] = (u, s, z)
            if name in skip:
                t[lp + name + ".weight"] = torch.from_numpy(R.weights_f64(u, R.bf16_bits(s.astype(np.float32)), z)).to(float_dtype)
                continue
            tensors = R.awq_pack(u, s, z) if kind == "awq" else R.gptq_pack(u, s, z, v1=kind in ("gptq", "gptq_sym"), g_idx=g_idx(k) if g_idx else None)
            for suffix, arr in tensors.items():
                t[lp + name + "." + suffix] = torch.from_numpy(np.ascontiguousarray(arr))
    save_file(t, os.path.join(path, "model.safetensors"))
    if kind == "awq":
        qc = {"quant_method": "awq", "bits": 4, "group_size": 128, "zero_point": True, "version": "GEMM",
              "modules_to_not_convert": list(skip) or None}
    else:
        qc = {"quant_method": "gptq", "bits": 4, "group_size": 128, "desc_act": False, "sym": kind == "gptq_sym", "damp_percent": 0.1}
        if kind == "gptq_v2":
            qc["checkpoint_format"] = "gptq_v2"
        elif kind == "gptq_sym":
            qc["checkpoint_format"] = "gptq"
    qc.update(qc_over or {})
    json.dump({"model_type": "llama", "quantization_config": qc}, open(os.path.join(path, "config.json"), "w"))
    return cfg, t, want


def _cat(want, parts, i):
    return np.concatenate([want[P + x][i] for x in parts])


@pytest.mark.parametrize("kind", ["awq", "gptq", "gptq_v2"])
def test_w4a16_target_gets_codes_zeros_and_scale_bits(tmp_path, kind):
    from ssd_amd.quant import W4ZTensor
    from ssd_amd.weights import load_safetensors, checkpoint_quantization
    cfg, t, want = write_int4_ckpt(str(tmp_path), kind)
    assert checkpoint_quantization(str(tmp_path)) == "w4a16"
    got = dict(load_safetensors(cfg, str(tmp_path), w4a16=True))
    for packed, parts in PACKS.items():
        w = got[P + packed + ".weight"]
        assert isinstance(w, W4ZTensor), packed
        assert w.packed.dtype == torch.int32 and w.scale.dtype == torch.bfloat16 and w.zero.dtype == torch.uint8
        assert np.array_equal(w.packed.numpy(), R.pack(_cat(want, parts, 0))), packed
        assert np.array_equal(w.zero.numpy(), _cat(want, parts, 2)), packed
        assert np.array_equal(bits(w.scale), R.bf16_bits(_cat(want, parts, 1).astype(np.float32))), packed
    # fp16 LM head, embedding and norms load as bf16
    for name in ("lm_head.weight", "model.embed_tokens.weight", "model.norm.weight", P + "input_layernorm.weight"):
        assert got[name].dtype == torch.bfloat16 and torch.equal(got[name], t[name].to(torch.bfloat16)), name
    assert not any(k.endswith((".qweight", ".qzeros", ".scales", ".g_idx")) for k in got)


def test_symmetric_gptq_arrives_as_plain_w4tensor(tmp_path):
    from ssd_amd.quant import W4Tensor, W4ZTensor
    from ssd_amd.weights import load_safetensors
    cfg, _, want = write_int4_ckpt(str(tmp_path), "gptq_sym")
    got = dict(load_safetensors(cfg, str(tmp_path), w4a16=True))
    for packed, parts in PACKS.items():
        w = got[P + packed + ".weight"]
        assert isinstance(w, W4Tensor) and not isinstance(w, W4ZTensor), packed
        assert np.array_equal(w.packed.numpy(), R.pack(_cat(want, parts, 0)))
        assert np.array_equal(bits(w.scale), R.bf16_bits(_cat(want, parts, 1).astype(np.float32)))


def test_fp16_scales_round_to_nearest_even_once(tmp_path):
    from ssd_amd.weights import load_safetensors
    from safetensors.torch import load_file, save_file
    cfg, _, _ = write_int4_ckpt(str(tmp_path), "awq")
    f = os.path.join(str(tmp_path), "model.safetensors")
    t = load_file(f)
    s = t[P + "self_attn.o_proj.scales"]            # [K/128, N]
    s[0, 0], s[0, 1], s[0, 2] = 1.0 + 2 ** -10, 1.0 + 3 * 2 ** -8, 1.0 + 2 ** -8
    save_file(t, f)
    got = dict(load_safetensors(cfg, str(tmp_path), w4a16=True))[P + "self_attn.o_proj.weight"].scale
    assert got[0, 0].item() == 1.0 and got[1, 0].item() == 1.0 + 2 ** -6 and got[2, 0].item() == 1.0


@pytest.mark.parametrize("kind", ["awq", "gptq", "gptq_v2", "gptq_sym"])
def test_bf16_target_reads_dequantized_and_tp_shards(tmp_path, kind):
    from ssd_amd.weights import load_safetensors, shard_param
    cfg, _, want = write_int4_ckpt(str(tmp_path), kind)
    full = dict(load_safetensors(cfg, str(tmp_path)))
    deq = {}
    for packed, parts in PACKS.items():
        w = full[P + packed + ".weight"]
        assert w.dtype == torch.bfloat16
        ref = R.dequant(_cat(want, parts, 0), R.bf16_bits(_cat(want, parts, 1).astype(np.float32)), _cat(want, parts, 2))
        assert np.array_equal(bits(w), ref), packed
        deq[P + packed + ".weight"] = w
    for rank in range(2):
        sh = dict(load_safetensors(cfg, str(tmp_path), rank, 2))
        for name, w in deq.items():
            assert torch.equal(sh[name], shard_param(cfg, name, w, rank, 2)), (name, rank)


def test_unconverted_linear_loads_as_bf16(tmp_path):
    """AWQ modules_to_not_convert: a linear present only as .weight comes as bf16; packed with quantized siblings it is
    concatenated with their dequantized matrices."""
    from ssd_amd.quant import W4ZTensor
    from ssd_amd.weights import load_safetensors
    cfg, t, want = write_int4_ckpt(str(tmp_path), "awq", skip=("self_attn.o_proj", "mlp.up_proj"))
    with pytest.warns(UserWarning, match="gate_up_proj"):       # a packed matrix with only one part quantized: said aloud
        got = dict(load_safetensors(cfg, str(tmp_path), w4a16=True))
    assert torch.equal(got[P + "self_attn.o_proj.weight"], t[P + "self_attn.o_proj.weight"].to(torch.bfloat16))
    assert isinstance(got[P + "mlp.down_proj.weight"], W4ZTensor)
    gu = got[P + "mlp.gate_up_proj.weight"]
    assert gu.dtype == torch.bfloat16 and tuple(gu.shape) == (512, 128)
    u, s, z = want[P + "mlp.gate_proj"]
    assert np.array_equal(bits(gu[:256]), R.dequant(u, R.bf16_bits(s.astype(np.float32)), z))
    assert torch.equal(gu[256:], t[P + "mlp.up_proj.weight"].to(torch.bfloat16))


REFUSALS = [
    ("awq", dict(qc_over={"version": "gemv"}), dict(w4a16=True), "gemv"),
    ("awq", dict(qc_over={"zero_point": False}), dict(w4a16=True), "zero_point"),
    ("gptq", dict(qc_over={"desc_act": True}), dict(w4a16=True), "desc_act"),
    ("gptq", dict(g_idx="shuffled"), dict(w4a16=True), "g_idx"),
    ("awq", dict(qc_over={"bits": 8}), dict(w4a16=True), "bits"),
    ("gptq", dict(qc_over={"bits": 8}), dict(), "bits"),
    ("awq", dict(qc_over={"group_size": 64}), dict(w4a16=True), "group_size"),
    ("gptq", dict(qc_over={"group_size": 64}), dict(), "group_size"),
    ("gptq", dict(qc_over={"checkpoint_format": "marlin"}), dict(w4a16=True), "marlin"),
    ("awq", dict(), dict(fp8=True), "fp8 target"),
    ("awq", dict(), dict(mxfp4=True), "mxfp4 target"),
    ("gptq", dict(), dict(fp8=True), "fp8 target"),
]


@pytest.mark.parametrize("kind,kw,target,match", REFUSALS)
def test_loader_refusals(tmp_path, kind, kw, target, match):
    from ssd_amd.weights import load_safetensors
    kw = dict(kw)
    if kw.get("g_idx") == "shuffled":       # right length, wrong content (trivial, hence accepted, where K is a single group)
        kw["g_idx"] = lambda K: np.roll(np.arange(K) // 128, 1)
    cfg, _, _ = write_int4_ckpt(str(tmp_path), kind, **kw)
    with pytest.raises(ValueError, match=match):
        list(load_safetensors(cfg, str(tmp_path), **target))


def test_other_quant_methods_stay_refused_by_name(tmp_path):
    from ssd_amd.weights import checkpoint_quantization
    json.dump({"quantization_config": {"quant_method": "bitsandbytes"}}, open(os.path.join(str(tmp_path), "config.json"), "w"))
    with pytest.raises(ValueError, match="quant_method"):
        checkpoint_quantization(str(tmp_path))


def test_decoders_other_than_w4a16_and_bf16_refuse_zero_point_tensors():
    from ssd_amd.model import HipDecoder
    from ssd_amd.quant import quantize_w4a16_zp
    cfg = _tiny_cfg()
    w = quantize_w4a16_zp((0.02 * torch.randn(128, 128)).to(torch.bfloat16))
    for q in ("fp8", "mxfp4"):
        dec = HipDecoder.__new__(HipDecoder)
        dec.fp8, dec.mx4, dec.w4, dec.quantized, dec.device = q == "fp8", q == "mxfp4", False, True, torch.device("cpu")
        with pytest.raises(ValueError, match="zero-point"):
            dec.load_weights(iter([(P + "self_attn.o_proj.weight", w)]))
    with pytest.raises(ValueError, match="w4_zero_point"):
        HipDecoder(cfg, max_tokens=16, max_seqs=1, max_blocks=2, block_size=16, max_model_len=64, device=torch.device("cpu"),
                   quantization="fp8", w4_zero_point=True)


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_w4zp_header_symbols_exported_bound_and_documented():
    from ssd_amd.hip.lib import SIGNATURES
    from ssd_amd.hip.quant_ops import QUANT_SIGNATURES
    from ssd_amd.hip.w4_ops import W4_SIGNATURES
    from ssd_amd.hip.mx4_ops import MX4_SIGNATURES
    from ssd_amd.hip.w4zp_ops import W4ZP_SIGNATURES, load_w4zp_library
    _built_lib()
    lib = load_w4zp_library()
    syms = w4zp_header_symbols()
    assert len(syms) == 5
    assert sorted(W4ZP_SIGNATURES) == syms
    for other in (SIGNATURES, QUANT_SIGNATURES, W4_SIGNATURES, MX4_SIGNATURES):
        assert not set(syms) & set(other)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        assert f"`{s}(" in doc, f"{s} has no line in INTEGRATION.md"
    common = open(os.path.join(ROOT, "ssd_amd", "csrc", "common.h")).read()
    assert '#include "ssd_hip_w4zp.h"' in common
    mk = open(os.path.join(ROOT, "ssd_amd", "csrc", "Makefile")).read()
    assert "ssd_hip_w4zp.h" in mk
    from ssd_amd.hip.lib import ABI_VERSION
    assert ABI_VERSION == 3


def test_c_consumer_walks_every_w4zp_validation_path(tmp_path):
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "w4zp_abi_consumer.c")
    body = open(src).read()
    for s in w4zp_header_symbols():
        assert f"{s}(" in body, s
    exe = str(tmp_path / "w4zp_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout
