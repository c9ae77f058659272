"""Qwen3-MoE targets without a GPU: tests/moe_ref.py's float64 forward against transformers' Qwen3MoeForCausalLM, the configuration
(ModelConfig.from_hf, the qwen3-30b-a3b preset, every Config refusal), the safetensors loader in both naming forms, and the tie and
rounding rules of the route reference on hand-made rows."""
import json
import math
import os

import pytest
import torch

from tests import moe_ref as R

BF = torch.bfloat16
TOKENS = [(37 * i + 11) % 512 for i in range(24)]


def _hf_config(**kw):
    from transformers import Qwen3MoeConfig
    base = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=32, num_experts=8,
                num_experts_per_tok=2, moe_intermediate_size=64, intermediate_size=64, vocab_size=512, max_position_embeddings=1024,
                norm_topk_prob=True, tie_word_embeddings=False, decoder_sparse_step=1, mlp_only_layers=[], rms_norm_eps=1e-6)
    base.update(kw)
    return Qwen3MoeConfig(**base)


def _hf_state_dict(cfg, w: dict, dtype) -> dict:
    """Our packed names -> transformers' (q / k / v unpacked; the router and the fused expert tensors keep their names)."""
    nh, nkv, hd = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim
    out = {}
    for name, t in w.items():
        if name.endswith("qkv_proj.weight"):
            q, k, v = t.split([nh * hd, nkv * hd, nkv * hd], 0)
            for x, part in zip("qkv", (q, k, v)):
                out[name.replace("qkv_proj", f"{x}_proj")] = part.to(dtype).contiguous()
        else:
            out[name] = t.to(dtype).contiguous()
    return out


@pytest.fixture(scope="module")
def tiny():
    from ssd_amd import weights as W
    from ssd_amd.model_config import ModelConfig
    hc = _hf_config()
    cfg = ModelConfig.from_hf(hc)
    w = W.synthetic_state_dict(cfg, seed=3, std=0.1, norm_jitter=0.1, recipe={"router_gain": 8.0})
    return hc, cfg, w


def test_truth_forward_equals_transformers_float64(tiny):
    from transformers import Qwen3MoeForCausalLM
    hc, cfg, w = tiny
    hc._experts_implementation = "eager"           # the default grouped-mm path refuses doubles
    model = Qwen3MoeForCausalLM(hc).double().eval()
    missing = model.load_state_dict(_hf_state_dict(cfg, w, torch.float64), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    routes = []
    hooks = [layer.mlp.gate.register_forward_hook(lambda m, i, o: routes.append(o[2])) for layer in model.model.layers]
    with torch.no_grad():
        want = model(torch.tensor([TOKENS])).logits[0]
    for hk in hooks:
        hk.remove()
    # transformers computes three things in float32 whatever the model's dtype (the rotary table, every RMSNorm's normalisation, the
    # router's softmax: moe_ref.forward, hf_float32_points), so its float64 model is matched to 1e-9 by the float64 forward with those
    # three points in float32 too; the truth proper has none of them and must agree to what they can cost
    got, rlogits, ids = R.forward(cfg, w, TOKENS, hf_float32_points=True)
    truth, t_rlogits, t_ids = R.forward(cfg, w, TOKENS)
    # the test's own input condition: no exact tie at the k-th boundary of the float64 router logits
    for li, rl in enumerate(rlogits):
        margin, _ = R.kth_margins(rl, cfg.num_experts_per_tok)
        assert float(margin.min()) > 0.0, f"input problem: layer {li} has an exact tie at the top-k boundary"
    assert len(routes) == cfg.num_layers
    for li in range(cfg.num_layers):
        assert torch.equal(routes[li].sort(-1).values, ids[li].sort(-1).values), f"layer {li}: routes differ"
        assert torch.equal(routes[li], ids[li]), f"layer {li}: order of the chosen experts differs"
        assert torch.equal(t_ids[li], ids[li]), f"layer {li}: the truth proper routes differently"
    rel = float((got - want).abs().max() / want.abs().max())
    rel_truth = float((truth - want).abs().max() / want.abs().max())
    print(f"moe_ref forward vs Qwen3MoeForCausalLM float64: max relative difference {rel:.3e} with transformers' float32 points, "
          f"{rel_truth:.3e} without (the truth proper)")
    assert rel <= 1e-9, rel
    # 9 float32-rounded quantities on a logit's path (2 layers x (2 norms + q / k norm + rotary table) + the final norm), each good
    # to 2^-24 relative and amplified by the few-fold cancellation of a logit: 1e-5 is ~170 float32 roundings
    assert rel_truth <= 1e-5, rel_truth


def test_from_hf_and_its_refusals():
    from ssd_amd.model_config import ModelConfig
    cfg = ModelConfig.from_hf(_hf_config(num_experts=16, num_experts_per_tok=4, moe_intermediate_size=96, norm_topk_prob=False))
    assert cfg.family == "qwen3_moe" and cfg.qk_norm
    assert (cfg.num_experts, cfg.num_experts_per_tok, cfg.moe_intermediate_size, cfg.norm_topk_prob) == (16, 4, 96, False)
    assert (cfg.hidden_size, cfg.num_layers, cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.vocab_size) == (128, 2, 4, 2, 32, 512)
    with pytest.raises(ValueError, match="mlp_only_layers"):
        ModelConfig.from_hf(_hf_config(mlp_only_layers=[1]))
    with pytest.raises(ValueError, match="decoder_sparse_step"):
        ModelConfig.from_hf(_hf_config(decoder_sparse_step=2))


def test_dense_configs_keep_their_fields():
    from transformers import Qwen3Config
    from ssd_amd.model_config import ModelConfig, PRESETS
    for name, c in PRESETS.items():
        if name != "qwen3-30b-a3b":
            assert c.num_experts == 0 and c.num_experts_per_tok == 0 and c.moe_intermediate_size == 0 and not c.norm_topk_prob, name
    d = ModelConfig.from_hf(Qwen3Config(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=32,
                                        intermediate_size=256, vocab_size=512))
    assert d.family == "qwen3" and d.num_experts == 0 and d.qk_norm and d.intermediate_size == 256


def test_preset_parameter_count():
    from ssd_amd import weights as W
    from ssd_amd.model_config import PRESETS
    c = PRESETS["qwen3-30b-a3b"]
    assert (c.hidden_size, c.num_layers, c.num_heads, c.num_kv_heads, c.head_dim) == (2048, 48, 32, 4, 128)
    assert (c.num_experts, c.num_experts_per_tok, c.moe_intermediate_size, c.vocab_size) == (128, 8, 768, 151936)
    assert c.rope_theta == 1e6 and c.max_position_embeddings == 40960 and not c.tie_word_embeddings and c.norm_topk_prob and c.qk_norm
    n = sum(math.prod(s) for _, s in W.param_shapes(c))
    print(f"qwen3-30b-a3b: {n / 1e9:.3f} B parameters")
    assert abs(n / 1e9 - 30.5) <= 0.1


def _assert_loads(cfg, w, path):
    from ssd_amd import weights as W
    got = dict(W.load_safetensors(cfg, path))
    assert set(got) == set(w)
    for name, t in w.items():
        assert got[name].dtype == BF and torch.equal(got[name], t), name


def _index_names(path):
    from safetensors import safe_open
    names = []
    for f in sorted(os.listdir(path)):
        if f.endswith(".safetensors"):
            with safe_open(os.path.join(path, f), "pt", "cpu") as sf:
                names += list(sf.keys())
    return names


def test_loader_reads_both_naming_forms(tiny, tmp_path):
    """A checkpoint save_pretrained wrote (whichever form it emits) and a hand-written one in the other form."""
    from safetensors.torch import save_file
    from transformers import Qwen3MoeForCausalLM
    hc, cfg, w = tiny
    model = Qwen3MoeForCausalLM(hc).to(BF)
    model.load_state_dict(_hf_state_dict(cfg, w, BF), strict=True)
    saved = str(tmp_path / "saved")
    model.save_pretrained(saved, safe_serialization=True)
    names = _index_names(saved)
    fused = any(n.endswith("mlp.experts.gate_up_proj") for n in names)
    per_expert = any(n.endswith("mlp.experts.0.gate_proj.weight") for n in names)
    assert fused != per_expert, names[:20]
    print("save_pretrained wrote the", "fused 3-D" if fused else "per-expert", "names")
    _assert_loads(cfg, w, saved)
    # the other form, written by hand
    other = str(tmp_path / "other")
    os.makedirs(other)
    sd = {}
    for name, t in _hf_state_dict(cfg, w, BF).items():
        if fused and name.endswith("mlp.experts.gate_up_proj"):
            base = name[:-len(".gate_up_proj")]
            for e in range(cfg.num_experts):
                g, u = t[e].chunk(2, 0)
                sd[f"{base}.{e}.gate_proj.weight"], sd[f"{base}.{e}.up_proj.weight"] = g.contiguous(), u.contiguous()
        elif fused and name.endswith("mlp.experts.down_proj"):
            base = name[:-len(".down_proj")]
            for e in range(cfg.num_experts):
                sd[f"{base}.{e}.down_proj.weight"] = t[e].contiguous()
        else:
            sd[name] = t
    if not fused:           # save_pretrained wrote per-expert names: the hand-written form is the fused one
        sd = _hf_state_dict(cfg, w, BF)
    save_file(sd, os.path.join(other, "model.safetensors"))
    with open(os.path.join(other, "config.json"), "w") as f:
        json.dump({"model_type": "qwen3_moe"}, f)
    _assert_loads(cfg, w, other)
    # a checkpoint with neither form of an expert tensor is refused by name
    broken = str(tmp_path / "broken")
    os.makedirs(broken)
    save_file({k: v for k, v in sd.items() if "experts" not in k}, os.path.join(broken, "model.safetensors"))
    from ssd_amd import weights as W
    with pytest.raises(ValueError, match="experts"):
        dict(W.load_safetensors(cfg, broken))


def test_synthetic_router_gain(tiny):
    from ssd_amd import weights as W
    _, cfg, w = tiny
    plain = W.synthetic_state_dict(cfg, seed=3, std=0.1, norm_jitter=0.1)
    for name in w:
        if name.endswith("mlp.gate.weight"):
            assert torch.equal(w[name], (plain[name].float() * 8.0).to(BF)), name
        else:
            assert torch.equal(w[name], plain[name]), name
    shapes = dict(W.param_shapes(cfg))
    assert shapes["model.layers.1.mlp.gate.weight"] == (8, 128)
    assert shapes["model.layers.1.mlp.experts.gate_up_proj"] == (8, 128, 128)
    assert shapes["model.layers.1.mlp.experts.down_proj"] == (8, 128, 64)
    assert not any("mlp.gate_up_proj" in n or "mlp.down_proj.weight" in n for n in shapes)


def test_config_refusals():
    from ssd_amd.config import Config
    from ssd_amd.model_config import ModelConfig
    moe = R.tiny_moe_config()
    dense = ModelConfig("qwen3", 128, 2, 4, 2, 32, 256, 512, 1e-6, 1e6, 1024, True, True)
    kw = dict(hf_config=moe, max_model_len=256, max_num_batched_tokens=256, kvcache_block_size=16)
    Config("moe", **kw)
    Config("moe", draft="d", draft_hf_config=dense, speculate=True, speculate_k=3, **kw)
    for extra, word in ((dict(quantization="fp8"), "quantization"), (dict(quantization="w4a16"), "quantization"),
                        (dict(kv_cache_dtype="fp8"), "kv_cache_dtype"), (dict(enable_lora=True), "enable_lora"),
                        (dict(num_gpus=2), "num_gpus"),
                        (dict(use_eagle=True, speculate=True, draft="d", draft_hf_config=dense, draft_async=True, jit_speculate=True), "use_eagle")):
        with pytest.raises(ValueError, match=word):
            Config("moe", **extra, **kw)
    with pytest.raises(ValueError, match="draft"):
        Config("dense", hf_config=dense, draft="moe", draft_hf_config=moe, speculate=True, speculate_k=3, max_model_len=256,
               max_num_batched_tokens=256, kvcache_block_size=16)
    with pytest.raises(ValueError, match="num_experts"):
        Config("moe", **dict(kw, hf_config=R.tiny_moe_config(num_experts=12)))


def test_runner_without_the_kernels_refuses_a_moe_model():
    """The CPU oracle runners have no expert kernels: the engine refuses the model by name before it builds one."""
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.utils.topology import Topology
    with pytest.raises(ValueError, match="mixture-of-experts"):
        LLMEngine("moe", runner_factory=oracle_runner_factory(None, None), hf_config=R.tiny_moe_config(), max_model_len=256,
                  max_num_batched_tokens=256, kvcache_block_size=16, num_kvcache_blocks=8,
                  topology=Topology(0, 1, torch.device("cpu"), "target", 0, 1))


def test_route_reference_rules():
    # equal logits: ties go to the lower expert index, larger first
    l = torch.tensor([[1.0, 3.0, 3.0, 0.5, 3.0, 1.0, 1.0, -2.0]]).to(BF)
    ids, w, offs, perm = R.route_ref(l, 4, True)
    assert ids.tolist() == [[1, 2, 4, 0]]
    assert abs(float(w.float().sum()) - 1.0) < 2 ** -7
    # an all-equal row: the first k experts, equal weights
    ids, w, _, _ = R.route_ref(torch.zeros(1, 8).to(BF), 3, True)
    assert ids.tolist() == [[0, 1, 2]] and torch.equal(w, torch.full((1, 3), 1 / 3).to(BF))
    # norm off: the softmax itself, rounded to bf16; k == E: every expert, and the weights sum to 1 within the roundings
    l = torch.tensor([[0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], [7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0, 0.0]]).to(BF)
    ids, w, offs, perm = R.route_ref(l, 8, False)
    assert ids.tolist() == [[7, 6, 5, 4, 3, 2, 1, 0], [0, 1, 2, 3, 4, 5, 6, 7]]
    p = torch.softmax(torch.arange(8, dtype=torch.float64), 0).flip(0)
    assert torch.equal(w[0], p.to(BF)) and torch.equal(w[1], p.to(BF))
    ids2, w2, _, _ = R.route_ref(l, 2, False)
    assert torch.equal(w2, w[:, :2]), "without norm a weight does not depend on k"
    # the grouping tables: entries of an expert in ascending entry order
    assert offs.tolist() == [0, 2, 4, 6, 8, 10, 12, 14, 16]
    assert perm.tolist() == [7, 8, 6, 9, 5, 10, 4, 11, 3, 12, 2, 13, 1, 14, 0, 15]


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ssd_hip_moe.h")


def _header_symbols():
    import re
    return sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


def _built_lib():
    from ssd_amd.hip.lib import build_library, lib_path
    if not os.path.exists(lib_path()):
        build_library()
    return lib_path()


def test_moe_header_symbols_exported_and_bound():
    from ssd_amd.hip.lib import SIGNATURES
    from ssd_amd.hip.moe_ops import MOE_SIGNATURES, load_moe_library, EPI_UP, EPI_DOWN, MAX_K, MIN_E, MAX_E
    _built_lib()
    lib = load_moe_library()
    syms = _header_symbols()
    assert syms == ["ssd_moe_combine", "ssd_moe_gemm", "ssd_moe_route"]
    assert sorted(MOE_SIGNATURES) == syms and not set(syms) & set(SIGNATURES)
    assert all(hasattr(lib, s) for s in syms)
    text = open(HEADER).read()
    for name, val in (("SSD_MOE_EPI_UP", EPI_UP), ("SSD_MOE_EPI_DOWN", EPI_DOWN), ("SSD_MOE_MAX_K", MAX_K), ("SSD_MOE_MIN_E", MIN_E),
                      ("SSD_MOE_MAX_E", MAX_E)):
        assert f"#define {name} {val}\n" in text, name
    # the rounding note the combine owes its readers
    assert "index_add_" in text and "rounds LESS often" in text


def test_c_consumer_walks_every_moe_validation_path(tmp_path):
    import subprocess
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "moe_abi_consumer.c")
    body = open(src).read()
    for s in _header_symbols():
        assert f"{s}(" in body, s
    exe = str(tmp_path / "moe_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout
