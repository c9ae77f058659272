"""Block-scaled FP8 (128 x 128 weight_scale_inv), the parts that need no GPU: the checkpoint loader and its refusals, the block
quantizer, the host side of the group-scale table, and the C ABI of include/ssd_hip_fp8b.h (exports, ctypes table, INTEGRATION.md,
a plain-C consumer walking every entry point's argument validation)."""
import json
import os
import re
import subprocess

import pytest
import torch

from tests.conftest import ROOT
from tests.test_fp8_cpu import _tiny_cfg, _built_lib

HEADER = os.path.join(ROOT, "include", "ssd_hip_fp8b.h")
P = "model.layers.0."
PACKS = {"self_attn.qkv_proj": ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"],
         "mlp.gate_up_proj": ["mlp.gate_proj", "mlp.up_proj"], "self_attn.o_proj": ["self_attn.o_proj"],
         "mlp.down_proj": ["mlp.down_proj"]}


def fp8b_header_symbols():
    return sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


def _grid(n, k):
    return -(-n // 128), -(-k // 128)


def write_block_ckpt(path, cfg, *, seed=0, qc_over=None, scale_dtype=torch.float32, scale_edit=None, skip=()):
    """A one-layer checkpoint in the block format with unpacked q/k/v and gate/up (HF names) and the shapes of
    test_fp8_cpu._write_ckpt: h 128, k / v rows 64 (a ragged block row: q | k | v have 1 | 1 | 1 block rows over 128 | 64 | 64
    rows), I 256 (gate | up two block rows each, down_proj two block columns).  Every block has its own scale, none a power of two.
    Linears in `skip` are stored as plain bf16 .weight (modules_to_not_convert); lm_head and the embedding are bf16.  Returns
    (tensors, want) with want[name] = (codes, scales fp32 [grid])."""
    from safetensors.torch import save_file
    g = torch.Generator().manual_seed(seed)
    h, hd, nh, nkv, I, V = cfg.hidden_size, cfg.head_dim, cfg.num_heads, cfg.num_kv_heads, cfg.intermediate_size, cfg.vocab_size
    t = {"model.embed_tokens.weight": torch.randn(V, h, generator=g).to(torch.bfloat16),
         "lm_head.weight": torch.randn(V, h, generator=g).to(torch.bfloat16),
         "model.norm.weight": torch.ones(h, dtype=torch.bfloat16),
         P + "input_layernorm.weight": torch.ones(h, dtype=torch.bfloat16),
         P + "post_attention_layernorm.weight": torch.ones(h, dtype=torch.bfloat16)}
    want = {}
    shapes = {"self_attn.q_proj": (nh * hd, h), "self_attn.k_proj": (nkv * hd, h), "self_attn.v_proj": (nkv * hd, h),
              "self_attn.o_proj": (h, nh * hd), "mlp.gate_proj": (I, h), "mlp.up_proj": (I, h), "mlp.down_proj": (h, I)}
    for name, (n, k) in shapes.items():
        q = (torch.randn(n, k, generator=g) * 100).clamp(-448, 448).to(torch.float8_e4m3fn)
        s = ((1 + torch.rand(_grid(n, k), generator=g)) * 2.0 ** torch.randint(-12, -6, _grid(n, k), generator=g).float()).to(scale_dtype)
        if name in skip:
            t[P + name + ".weight"] = (q.float() * 1e-3).to(torch.bfloat16)
            continue
        t[P + name + ".weight"] = q
        t[P + name + ".weight_scale_inv"] = s
        want[name] = (q, s.float())
    if scale_edit is not None:
        scale_edit(t)
    save_file(t, os.path.join(path, "model.safetensors"))
    qc = {"quant_method": "fp8", "fmt": "e4m3", "weight_block_size": [128, 128], "activation_scheme": "dynamic",
          "modules_to_not_convert": ["lm_head"] + [P + s for s in skip]}
    qc.update(qc_over or {})
    qc = {k: v for k, v in qc.items() if v is not ...}
    json.dump({"model_type": "llama", "quantization_config": qc}, open(os.path.join(path, "config.json"), "w"))
    return t, want


def _rowscale(want, parts):
    """The per-part expansion, written out independently of quant.expand_fp8_block_scales: row n of a part takes block row n // 128."""
    rows = []
    for x in parts:
        q, s = want[x]
        rows.append(torch.stack([s[n // 128] for n in range(q.shape[0])]))
    return torch.cat(rows)


# ---------------------------------------------------------------------------------------------------------------------
# Loader
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_block_checkpoint_loads_codes_bit_for_bit_and_scales_per_part(tmp_path, scale_dtype):
    """Fails on the parent commit, which refuses the directory with a ValueError."""
    from ssd_amd.quant import FP8BTensor, dequantize_fp8_block
    from ssd_amd.weights import load_safetensors, checkpoint_quantization
    cfg = _tiny_cfg()
    t, want = write_block_ckpt(str(tmp_path), cfg, scale_dtype=scale_dtype)
    assert checkpoint_quantization(str(tmp_path)) == "fp8"
    got = dict(load_safetensors(cfg, str(tmp_path), fp8=True))
    bf = dict(load_safetensors(cfg, str(tmp_path)))
    for packed, parts in PACKS.items():
        w = got[P + packed + ".weight"]
        assert isinstance(w, FP8BTensor), packed
        codes = torch.cat([want[x][0] for x in parts])
        assert w.codes.dtype == torch.float8_e4m3fn and torch.equal(w.codes.view(torch.uint8), codes.view(torch.uint8)), packed
        rs = _rowscale(want, parts)
        assert w.rowscale.dtype == torch.float32 and torch.equal(w.rowscale, rs), packed
        # a bf16 target reads bf16(s * q), the product in fp32, element by element
        d = bf[P + packed + ".weight"]
        assert d.dtype == torch.bfloat16
        assert torch.equal(d, dequantize_fp8_block(codes, rs)), packed
        assert torch.equal(d, (codes.float() * rs.repeat_interleave(128, dim=1)[:, :codes.shape[1]]).to(torch.bfloat16)), packed
    # q | k | v have their own block rows: rows 0..127 | 128..191 | 192..255 take three different scales
    s_qkv = got[P + "self_attn.qkv_proj.weight"].rowscale
    assert s_qkv[0, 0] == s_qkv[127, 0] and s_qkv[128, 0] == s_qkv[191, 0] and s_qkv[192, 0] == s_qkv[255, 0]
    assert len({float(s_qkv[r, 0]) for r in (0, 128, 192)}) == 3
    assert tuple(got[P + "mlp.down_proj.weight"].rowscale.shape) == (128, 2)
    for d in (got, bf):
        assert d["lm_head.weight"].dtype == torch.bfloat16 and torch.equal(d["lm_head.weight"], t["lm_head.weight"])
        assert not any(k.endswith(("_scale", "_scale_inv")) for k in d)


def test_unconverted_linears_arrive_as_bf16_and_mixed_packs_dequantize(tmp_path):
    from ssd_amd.quant import FP8BTensor, dequantize_fp8_block, expand_fp8_block_scales
    from ssd_amd.weights import load_safetensors
    cfg = _tiny_cfg()
    t, want = write_block_ckpt(str(tmp_path), cfg, skip=("self_attn.o_proj", "mlp.up_proj"))
    got = dict(load_safetensors(cfg, str(tmp_path), fp8=True))
    assert torch.equal(got[P + "self_attn.o_proj.weight"], t[P + "self_attn.o_proj.weight"])
    assert isinstance(got[P + "mlp.down_proj.weight"], FP8BTensor)
    gu = got[P + "mlp.gate_up_proj.weight"]
    assert gu.dtype == torch.bfloat16 and tuple(gu.shape) == (512, 128)
    q, s = want["mlp.gate_proj"]
    assert torch.equal(gu[:256], dequantize_fp8_block(q, expand_fp8_block_scales(s, 256)))
    assert torch.equal(gu[256:], t[P + "mlp.up_proj.weight"])


def _bad_shape(t):
    t[P + "mlp.down_proj.weight_scale_inv"] = torch.ones(1, 1)


def _non_positive(t):
    t[P + "self_attn.o_proj.weight_scale_inv"][0, 0] = 0.0


def _non_finite(t):
    t[P + "mlp.gate_proj.weight_scale_inv"][1, 0] = float("inf")


REFUSALS = [
    (dict(qc_over={"weight_block_size": [64, 64]}), dict(fp8=True), "weight_block_size"),
    (dict(qc_over={"weight_block_size": [64, 64]}), dict(), "weight_block_size"),
    (dict(qc_over={"weight_block_size": ...}), dict(fp8=True), "weight_block_size"),
    (dict(qc_over={"fmt": "e5m2"}), dict(fp8=True), "e5m2"),
    (dict(scale_edit=_bad_shape), dict(fp8=True), r"mlp\.down_proj\.weight_scale_inv has shape"),
    (dict(scale_edit=_non_positive), dict(fp8=True), r"self_attn\.o_proj\.weight_scale_inv.*positive"),
    (dict(scale_edit=_non_finite), dict(), r"mlp\.gate_proj\.weight_scale_inv.*finite"),
    (dict(), dict(w4a16=True), "w4a16 target"),
    (dict(), dict(mxfp4=True), "mxfp4 target"),
]


@pytest.mark.parametrize("kw,target,match", REFUSALS)
def test_loader_refusals(tmp_path, kw, target, match):
    from ssd_amd.weights import load_safetensors
    cfg = _tiny_cfg()
    write_block_ckpt(str(tmp_path), cfg, **kw)
    with pytest.raises(ValueError, match=match):
        list(load_safetensors(cfg, str(tmp_path), **target))


def test_fmt_may_be_absent_and_activation_scheme_is_ignored(tmp_path):
    from ssd_amd.weights import checkpoint_quantization
    cfg = _tiny_cfg()
    write_block_ckpt(str(tmp_path), cfg, qc_over={"fmt": ..., "activation_scheme": "static"})
    assert checkpoint_quantization(str(tmp_path)) == "fp8"


def test_decoders_of_other_formats_refuse_block_tensors():
    from ssd_amd.model import HipDecoder
    from ssd_amd.quant import quantize_fp8_block
    w = quantize_fp8_block((0.02 * torch.randn(128, 128)).to(torch.bfloat16))
    for q in ("w4a16", "mxfp4"):
        dec = HipDecoder.__new__(HipDecoder)
        dec.fp8, dec.mx4, dec.w4, dec.quantized, dec.device = False, q == "mxfp4", q == "w4a16", True, torch.device("cpu")
        with pytest.raises(ValueError, match="block-scaled fp8"):
            dec.load_weights(iter([(P + "self_attn.o_proj.weight", w)]))


FOREIGN = [(kind, host) for kind, hosts in (("fp8", ("W4Tensor", "W4ZTensor", "MX4Tensor")),
                                            ("w4a16", ("FP8Tensor", "FP8BTensor", "MX4Tensor")),
                                            ("mxfp4", ("FP8Tensor", "FP8BTensor", "W4Tensor", "W4ZTensor"))) for host in hosts]


@pytest.mark.parametrize("kind,host", FOREIGN)
def test_every_quantized_decoder_refuses_every_host_form_of_another_kind(kind, host):
    """The whole matrix, not only the block-scaled column above: a ValueError that names the tensor's format and the decoder's."""
    from ssd_amd import quant
    from ssd_amd.model import HipDecoder
    make = {"FP8Tensor": quant.quantize_fp8, "FP8BTensor": quant.quantize_fp8_block, "W4Tensor": quant.quantize_w4a16,
            "W4ZTensor": quant.quantize_w4a16_zp, "MX4Tensor": quant.quantize_mxfp4}[host]
    phrase = {"FP8Tensor": "per-row fp8", "FP8BTensor": "block-scaled fp8", "W4Tensor": "int4", "W4ZTensor": "zero-point int4",
              "MX4Tensor": "MXFP4"}[host]
    w = make((0.02 * torch.randn(128, 128)).to(torch.bfloat16))
    dec = HipDecoder.__new__(HipDecoder)
    dec.fp8, dec.mx4, dec.w4, dec.quantized, dec.device = kind == "fp8", kind == "mxfp4", kind == "w4a16", True, torch.device("cpu")
    with pytest.raises(ValueError) as e:
        dec.load_weights(iter([(P + "self_attn.o_proj.weight", w)]))
    assert phrase in str(e.value) and kind in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------------------
# The group table
# ---------------------------------------------------------------------------------------------------------------------
def _rand_rowscale(parts, KB, seed=0):
    """[sum(parts), KB]: one independent random row of scales per 128-row block of each part."""
    from ssd_amd.quant import expand_fp8_block_scales
    g = torch.Generator().manual_seed(seed)
    return torch.cat([expand_fp8_block_scales(torch.rand(-(-n // 128), KB, generator=g) + 0.5, n) for n in parts])


def _check_groups(rs, rmap):
    from ssd_amd.quant import fp8_block_group_scales
    got = fp8_block_group_scales(rs, rmap, "x")
    N, KB = rs.shape
    assert got.dtype == torch.float32 and tuple(got.shape) == (N // 16, KB)
    src = torch.arange(N) if rmap is None else rmap.long()
    for d in range(N):                                  # every packed row finds the scales of its source row in its group's entry
        assert torch.equal(got[d // 16], rs[src[d]]), d
    return got


def test_group_scales_identity_gate_up_and_qkv_maps():
    from ssd_amd.quant import gate_up_row_map, qkv_row_map
    _check_groups(_rand_rowscale([320], 3), None)                       # a ragged last block row (320 = 2 * 128 + 64)
    N = 2 * 208                                                         # each half 208 rows: not a multiple of 128
    got = _check_groups(_rand_rowscale([208, 208], 2), gate_up_row_map(N))
    assert len({float(v) for v in got[:, 0]}) == 4                      # gate and up each contribute both of their block rows
    for nh, nkv, hd in ((4, 2, 64), (2, 1, 64), (4, 1, 128), (3, 1, 128)):
        _check_groups(_rand_rowscale([nh * hd, nkv * hd, nkv * hd], 2, seed=hd + nh), qkv_row_map(nh, nkv, hd))


def test_group_scales_refuse_a_group_that_mixes_block_rows():
    from ssd_amd.quant import fp8_block_group_scales, qkv_row_map
    rs = _rand_rowscale([256], 2)
    rmap = torch.arange(256, dtype=torch.int32)
    rmap[5], rmap[133] = 133, 5                                         # packed group 0 now draws one row from block row 1
    with pytest.raises(ValueError, match=r"layers\.3\.o_proj.*rows 0\.\.15"):
        fp8_block_group_scales(rs, rmap, "layers.3.o_proj")
    # head_dim 256: a rotation-paired group takes dims 8j.. and 128 + 8j.. of a head, which straddle two block rows
    with pytest.raises(ValueError, match="qkv"):
        fp8_block_group_scales(_rand_rowscale([256, 256, 256], 1), qkv_row_map(1, 1, 256), "qkv")


# ---------------------------------------------------------------------------------------------------------------------
# Quantizer
# ---------------------------------------------------------------------------------------------------------------------
def test_block_quantizer_round_trip_and_zero_blocks():
    from ssd_amd.quant import FP8_BLOCK, FP8BTensor, quantize_fp8_block, dequantize_fp8_block
    assert FP8_BLOCK == 128
    g = torch.Generator().manual_seed(2)
    w = (torch.randn(200, 320, generator=g) * 0.03).to(torch.bfloat16)       # ragged in both directions: 2 x 3 blocks
    w[:128, 128:256] = 0                                                     # an all-zero block
    w[130, 300] = 2.5                                                        # an outlier in the ragged corner block
    t = quantize_fp8_block(w)
    assert isinstance(t, FP8BTensor) and t.codes.dtype == torch.float8_e4m3fn and tuple(t.codes.shape) == (200, 320)
    assert t.rowscale.dtype == torch.float32 and tuple(t.rowscale.shape) == (200, 3)
    assert bool(torch.isfinite(t.rowscale).all()) and bool((t.rowscale > 0).all())
    assert bool((t.rowscale[:128, 1] == 1).all()) and bool((t.codes[:128, 128:256].float() == 0).all())
    assert bool(torch.isfinite(t.codes.float()).all()) and t.codes.float().abs().max() <= 448
    # the scale of a block is its amax / 448, shared by the rows of the block
    wf = w.float()
    assert torch.equal(t.rowscale[0], t.rowscale[127]) and torch.equal(t.rowscale[128], t.rowscale[199])
    assert t.rowscale[128, 2] == wf[128:, 256:].abs().max() / 448
    # half an e4m3 step at the code's own binade (2^-4 of its magnitude, 2^-10 below the normal range) times the block scale, with
    # the fp32 rounding of w * inv and s * q (2^-22 relative together), plus the bf16 rounding of the product (2^-9 relative)
    s = t.rowscale.repeat_interleave(128, dim=1)[:, :320]
    qa = t.codes.float().abs()
    bound = s * torch.maximum(qa * 2.0 ** -4, torch.full_like(qa, 2.0 ** -10)) * (1 + 2.0 ** -20) + wf.abs() * 2.0 ** -8
    err = (dequantize_fp8_block(*t).float() - wf).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    assert bool((err <= s * 16 * (1 + 2.0 ** -20) + wf.abs() * 2.0 ** -8).all())     # never more than half the top step, 32 / 2


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_fp8b_header_symbols_exported_bound_and_documented():
    from ssd_amd.hip.lib import SIGNATURES
    from ssd_amd.hip.quant_ops import QUANT_SIGNATURES
    from ssd_amd.hip.w4_ops import W4_SIGNATURES
    from ssd_amd.hip.w4zp_ops import W4ZP_SIGNATURES
    from ssd_amd.hip.mx4_ops import MX4_SIGNATURES
    from ssd_amd.hip.fp8b_ops import FP8B_SIGNATURES, load_fp8b_library
    _built_lib()
    lib = load_fp8b_library()
    syms = fp8b_header_symbols()
    assert syms == ["ssd_fp8b_dequant_frag", "ssd_gemm_fp8b", "ssd_gemm_fp8b_cfg"]
    assert sorted(FP8B_SIGNATURES) == syms
    for other in (SIGNATURES, QUANT_SIGNATURES, W4_SIGNATURES, W4ZP_SIGNATURES, MX4_SIGNATURES):
        assert not set(syms) & set(other)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        assert f"`{s}(" in doc, f"{s} has no line in INTEGRATION.md"
    common = open(os.path.join(ROOT, "ssd_amd", "csrc", "common.h")).read()
    assert '#include "ssd_hip_fp8b.h"' in common
    mk = open(os.path.join(ROOT, "ssd_amd", "csrc", "Makefile")).read()
    assert "ssd_hip_fp8b.h" in mk and "gemm_fp8b.hip" in mk and "gemm_fp8b.o" in mk and "gemm_fp8.h" in mk


def test_c_consumer_walks_every_fp8b_validation_path(tmp_path):
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "fp8b_abi_consumer.c")
    body = open(src).read()
    for s in fp8b_header_symbols():
        assert f"{s}(" in body, s
    exe = str(tmp_path / "fp8b_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout
