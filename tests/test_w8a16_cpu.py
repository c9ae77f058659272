"""W8A16 (int8 weight-only, group 128) without a GPU: the quantizer's round trip, compressed-tensors pack-quantized int8 checkpoints
(channel and group-128) bit for bit into a w8a16 target and as the exact dequantized image into a bf16 one, the refusals, Config, and
the C ABI of include/ssd_hip_w8a16.h."""
import json
import os
import re
import subprocess

import pytest
import torch

from tests.conftest import ROOT
from tests.test_w4a16_cpu import _tiny_cfg, SHAPES, PACKS, _built_lib

P = "model.layers.0."
BF = torch.bfloat16


def test_quantizer_round_trip_zero_groups_and_extremes():
    from ssd_amd.quant import quantize_w8a16, dequantize_w8a16, W8Tensor
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(32, 384, generator=g) * 0.02).to(BF)
    w[3, 128:256] = 0                                   # an all-zero group: s = 1, q = 0
    w[5, 0] = 1.0                                       # an outlier sets its group's scale
    codes, s = t = quantize_w8a16(w)
    assert isinstance(t, W8Tensor) and t.shape() == (32, 384) and codes.dtype == torch.uint8 and s.dtype == BF and s.shape == (32, 3)
    q = codes.to(torch.int16) - 128
    assert int(q.min()) >= -128 and int(q.max()) <= 127 and s[3, 1] == 1 and bool((q[3, 128:256] == 0).all())
    sf = s.float().repeat_interleave(128, dim=1)
    assert torch.equal(q.float(), torch.round(w.float() / sf).clamp(-128, 127))
    deq = dequantize_w8a16(codes, s)
    assert torch.equal(deq, t.dequantize()) and torch.equal(deq, (q.float() * sf).to(BF))
    # round to nearest with s within bf16 rounding of amax / 127: half a step of the fp32 scale, plus the bf16 rounding of the result
    assert bool(((deq.float() - w.float()).abs() <= 0.5 * sf * (1 + 2.0 ** -7) + w.float().abs() * 2.0 ** -8).all())


def _write_w8_ckpt(path, *, strategy="group", group_size=128, fmt="pack-quantized", symmetric=True, acts=None, actorder=None,
                   extra=None, scale_dtype=BF):
    """A one-layer pack-quantized int8 checkpoint with unpacked q/k/v and gate/up (HF names); lm_head, embedding and norms bf16.
    Returns the codes q and the scales as stored."""
    from safetensors.torch import save_file
    cfg = _tiny_cfg()
    g = torch.Generator().manual_seed(0)
    h, V = cfg.hidden_size, cfg.vocab_size
    t = {"model.embed_tokens.weight": torch.randn(V, h, generator=g).to(BF), "lm_head.weight": torch.randn(V, h, generator=g).to(BF),
         "model.norm.weight": torch.ones(h, dtype=BF), P + "input_layernorm.weight": torch.ones(h, dtype=BF),
         P + "post_attention_layernorm.weight": torch.ones(h, dtype=BF)}
    want = {}
    for name, (n, k) in SHAPES.items():
        q = torch.randint(-128, 128, (n, k), generator=g, dtype=torch.int16)
        q[0, :4] = torch.tensor([-128, 127, 0, -1])
        s = (torch.rand(n, 1 if strategy == "channel" else k // 128, generator=g, dtype=torch.float64) * 3e-4 + 1e-5).to(scale_dtype)
        u = (q + 128).to(torch.int64).reshape(n, k // 4, 4)
        words = (u << torch.tensor([0, 8, 16, 24])).sum(-1)              # field i of word j = column 4j + i, as q + 128
        t[P + name + ".weight_packed"] = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
        t[P + name + ".weight_scale"] = s
        t[P + name + ".weight_shape"] = torch.tensor([n, k], dtype=torch.int64)
        want[name] = (q, s.to(BF).expand(n, k // 128))
    t.update(extra or {})
    save_file(t, os.path.join(path, "model.safetensors"))
    wq = {"num_bits": 8, "type": "int", "symmetric": symmetric, "strategy": strategy, "group_size": group_size, "dynamic": False}
    if actorder is not None:
        wq["actorder"] = actorder
    qc = {"quant_method": "compressed-tensors", "format": fmt, "ignore": ["lm_head"],
          "config_groups": {"group_0": {"targets": ["Linear"], "weights": wq, "input_activations": acts}}}
    json.dump({"model_type": "llama", "quantization_config": qc}, open(os.path.join(path, "config.json"), "w"))
    return cfg, t, want


@pytest.mark.parametrize("strategy,scale_dtype", [("group", BF), ("channel", BF), ("group", torch.float16)])
def test_pack_quantized_int8_loads_bit_for_bit_and_dequantized_into_bf16(tmp_path, strategy, scale_dtype):
    from ssd_amd.quant import W8Tensor
    from ssd_amd.weights import load_safetensors, checkpoint_quantization
    cfg, t, want = _write_w8_ckpt(str(tmp_path), strategy=strategy, group_size=128 if strategy == "group" else None,
                                  scale_dtype=scale_dtype)
    assert checkpoint_quantization(str(tmp_path)) == "w8a16"
    got = dict(load_safetensors(cfg, str(tmp_path), w8a16=True))
    bf = dict(load_safetensors(cfg, str(tmp_path)))
    for packed, parts in PACKS.items():
        w = got[P + packed + ".weight"]
        q = torch.cat([want[x][0] for x in parts])
        s = torch.cat([want[x][1] for x in parts])
        assert isinstance(w, W8Tensor) and w.codes.dtype == torch.uint8 and w.scale.dtype == BF
        assert torch.equal(w.codes.to(torch.int16) - 128, q) and torch.equal(w.scale.view(torch.int16), s.contiguous().view(torch.int16))
        exact = (q.float() * s.float().repeat_interleave(128, dim=1)).to(BF)
        assert torch.equal(bf[P + packed + ".weight"].view(torch.int16), exact.view(torch.int16)), packed
    assert torch.equal(got["lm_head.weight"], t["lm_head.weight"])
    assert not any(k.endswith(("_packed", "_scale", "_shape")) for k in got)
    for other in ("fp8", "w4a16", "mxfp4"):
        with pytest.raises(ValueError, match=f"{other} target"):
            list(load_safetensors(cfg, str(tmp_path), **{other: True}))


@pytest.mark.parametrize("kw,match", [
    (dict(symmetric=False), "asymmetric int8"),
    (dict(extra={P + "self_attn.o_proj.weight_zero_point": torch.zeros(128, 1, dtype=torch.int32)}), "asymmetric int8"),
    (dict(group_size=64), "group_size"),
    (dict(group_size=32), "group_size"),
    (dict(strategy="tensor", group_size=None), "strategy"),
    (dict(actorder="weight"), "actorder"),
    (dict(fmt="int-quantized"), "int8 activations"),
    (dict(acts={"num_bits": 8, "type": "int", "strategy": "token", "dynamic": True, "symmetric": True}), "int8 activations"),
    (dict(fmt="marlin-24"), "format"),
])
def test_int8_loader_refuses_other_schemes_by_name(tmp_path, kw, match):
    from ssd_amd.weights import load_safetensors
    cfg, _, _ = _write_w8_ckpt(str(tmp_path), **kw)
    for target in (dict(w8a16=True), dict()):
        with pytest.raises(ValueError, match=match):
            list(load_safetensors(cfg, str(tmp_path), **target))


def test_other_checkpoints_refuse_the_w8a16_target_and_gptq_8_bit_is_refused(tmp_path):
    from ssd_amd.weights import load_safetensors, int4_checkpoint_scheme
    from tests.test_fp8_cpu import _write_ckpt
    from tests.test_w4a16_cpu import _write_w4_ckpt
    d1, d2 = tmp_path / "w4", tmp_path / "fp8"
    d1.mkdir()
    d2.mkdir()
    cfg, _, _ = _write_w4_ckpt(str(d1))
    _write_ckpt(str(d2), _tiny_cfg())
    for d in (d1, d2):
        with pytest.raises(ValueError, match="w8a16 target"):
            list(load_safetensors(cfg, str(d), w8a16=True))
    with pytest.raises(ValueError, match="bits"):       # GPTQ / AWQ 8-bit exports are not read (README, "W8A16")
        int4_checkpoint_scheme({"quant_method": "gptq", "bits": 8, "group_size": 128, "sym": True, "desc_act": False})


def test_config_accepts_w8a16_and_keeps_the_refusals():
    from ssd_amd.config import Config
    from ssd_amd.model_config import presets
    kw = dict(max_model_len=512, max_num_batched_tokens=512, kvcache_block_size=16)
    assert Config("llama-3.2-1b", quantization="w8a16", **kw).quantization == "w8a16"
    assert Config("llama-3.2-1b", quantization="w8a16", kv_cache_dtype="fp8", enable_lora=True, **kw).enable_lora
    for bad, match in ((dict(w4_zero_point=True), "w4_zero_point"), (dict(num_gpus=2), "one GPU"), (dict(use_eagle=True), "use_eagle")):
        with pytest.raises(ValueError, match=match):
            Config("llama-3.2-1b", quantization="w8a16", **bad, **kw)
    for spelling in ("int8", "w8a8", "W8A16"):
        with pytest.raises(ValueError, match="quantization must be"):
            Config("llama-3.2-1b", quantization=spelling, **kw)
    moe = next(c for c in presets().values() if c.num_experts > 0)
    with pytest.raises(ValueError, match="quantization='w8a16'"):
        Config("moe", hf_config=moe, quantization="w8a16", **kw)


def test_c_consumer_walks_every_w8_validation_path_and_the_table_is_the_header(tmp_path):
    from ssd_amd.hip.lib import SIGNATURES
    from ssd_amd.hip.w8_ops import W8_SIGNATURES, load_w8_library
    lib = _built_lib()
    syms = sorted(set(re.findall(r"^int (ssd_\w+)\(", open(os.path.join(ROOT, "include", "ssd_hip_w8a16.h")).read(), re.M)))
    assert len(syms) == 5 and sorted(W8_SIGNATURES) == syms and not set(syms) & set(SIGNATURES)
    assert all(hasattr(load_w8_library(), s) for s in syms)
    src = os.path.join(ROOT, "tests", "w8a16_abi_consumer.c")
    assert all(f"{s}(" in open(src).read() for s in syms)
    exe, libdir = str(tmp_path / "w8a16_abi_consumer"), os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "0 failures" in run.stdout, run.stdout + run.stderr
