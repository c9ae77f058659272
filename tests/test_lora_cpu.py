"""LoRA adapters without a GPU: SamplingParams / Config validation, the loader's refusals (each by name), rank padding, the packing
of q | k | v and gate | up adapters into one adapter of the fused linear (exact), the adapter-rooted block hashes of the target's prefix
cache, and the refusals of engines that cannot run an adapter."""
import dataclasses
import json

import pytest
import torch

from tests import lora_ref as LR

BF = torch.bfloat16


def _cfg(name):
    from oracle.io import load_npz
    from tests.conftest import GOLDEN
    from tests.test_model_gpu import mk_cfg
    import os
    g = load_npz(os.path.join(GOLDEN, name + ".npz"))
    return mk_cfg(g, "llama") if name == "tiny_llama" else mk_cfg(g, "qwen3", tie=True, qk_norm=True)


def _adapter(cfg, r=8, alpha=16, seed=0, **kw):
    from ssd_amd.lora import module_shapes
    return LR.make_adapter(module_shapes(cfg), cfg.num_layers, r, alpha, seed, **kw)


# ---- public parameters ----------------------------------------------------------------------------------------------
def test_sampling_params_lora_field():
    from ssd_amd.sampling_params import SamplingParams
    assert SamplingParams().lora is None and SamplingParams(lora="x").lora == "x"
    for bad in ("", 3, ["x"], True):
        with pytest.raises(ValueError, match="lora"):
            SamplingParams(lora=bad)


def test_config_fields_and_refusals():
    from ssd_amd.config import Config
    cfg = _cfg("tiny_llama")
    c = Config("t", hf_config=cfg, max_model_len=256, max_num_batched_tokens=256)
    assert c.enable_lora is False and c.max_loras == 4 and c.max_lora_rank == 64
    c = Config("t", hf_config=cfg, max_model_len=256, max_num_batched_tokens=256, enable_lora=True, max_loras=8, max_lora_rank=16)
    assert c.enable_lora and c.max_loras == 8 and c.max_lora_rank == 16
    for kw, word in ((dict(max_loras=0), "max_loras"), (dict(max_loras=9), "max_loras"), (dict(max_lora_rank=8), "max_lora_rank"),
                     (dict(max_lora_rank=128), "max_lora_rank"), (dict(max_lora_rank=48), "max_lora_rank")):
        with pytest.raises(ValueError, match=word):
            Config("t", hf_config=cfg, max_model_len=256, max_num_batched_tokens=256, enable_lora=True, **kw)
    # with enable_lora off the other two fields are not looked at
    Config("t", hf_config=cfg, max_model_len=256, max_num_batched_tokens=256, max_loras=99)


def test_enable_lora_refuses_tensor_parallel_and_eagle():
    from ssd_amd.engine.llm_engine import LLMEngine
    cfg = _cfg("tiny_llama")
    kw = dict(hf_config=cfg, max_model_len=256, max_num_batched_tokens=256)
    with pytest.raises(ValueError, match="enable_lora.*one GPU"):
        LLMEngine("t", enable_lora=True, num_gpus=2, **kw)
    with pytest.raises(ValueError, match="enable_lora.*use_eagle"):
        LLMEngine("t", enable_lora=True, use_eagle=True, **kw)


# ---- loader ---------------------------------------------------------------------------------------------------------
def test_loader_accepts_the_dict_and_the_directory_form(tmp_path):
    from safetensors.torch import save_file
    from ssd_amd.lora import load_adapter, MODULES
    cfg = _cfg("tiny_llama")
    ad = _adapter(cfg, r=8, alpha=16, seed=3)
    a = load_adapter(ad, cfg, 64)
    assert a.r == 8 and a.scale == 2.0 and a.target_modules == MODULES and len(a.tensors) == 7 * cfg.num_layers
    assert load_adapter(dict(ad, use_rslora=True), cfg, 64).scale == 16 / 8 ** 0.5
    assert load_adapter(ad, cfg, 64, alpha=4).scale == 0.5
    (tmp_path / "adapter_config.json").write_text(json.dumps({k: v for k, v in ad.items() if k != "tensors"} | {
        "peft_type": "LORA", "bias": "none", "use_dora": False, "modules_to_save": None, "rank_pattern": {}, "alpha_pattern": {},
        "fan_in_fan_out": False, "use_rslora": False}))
    save_file({k: v.contiguous() for k, v in ad["tensors"].items()}, str(tmp_path / "adapter_model.safetensors"))
    b = load_adapter(str(tmp_path), cfg, 64)
    assert b.r == a.r and b.scale == a.scale and set(b.tensors) == set(a.tensors)
    assert all(torch.equal(b.tensors[k][i], a.tensors[k][i]) for k in a.tensors for i in (0, 1))
    with pytest.raises(ValueError, match="adapter_config.json"):
        load_adapter(str(tmp_path / "nothing"), cfg, 64)


@pytest.mark.parametrize("change,word", [
    (dict(use_dora=True), "use_dora"), (dict(bias="all"), "bias"), (dict(bias="lora_only"), "bias"),
    (dict(modules_to_save=["lm_head"]), "modules_to_save"), (dict(rank_pattern={"q_proj": 4}), "rank_pattern"),
    (dict(alpha_pattern={"q_proj": 4}), "alpha_pattern"), (dict(fan_in_fan_out=True), "fan_in_fan_out"),
    (dict(peft_type="LOHA"), "peft_type"), (dict(target_modules=["q_proj", "lm_head"]), "lm_head"),
    (dict(target_modules=["embed_tokens"]), "embed_tokens"), (dict(target_modules=[]), "target_modules"),
    (dict(r=0), "r must"), (dict(lora_alpha=None), "lora_alpha"), (dict(r=32), "max_lora_rank")])
def test_loader_refuses_by_name(change, word):
    from ssd_amd.lora import load_adapter
    cfg = _cfg("tiny_llama")
    with pytest.raises(ValueError, match=word):
        load_adapter(dict(_adapter(cfg), **change), cfg, 16)


def test_loader_refuses_tensors_that_do_not_fit():
    from ssd_amd.lora import load_adapter
    cfg = _cfg("tiny_llama")
    ad = _adapter(cfg)
    name = "base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight"

    def with_(**t):
        return dict(ad, tensors={**ad["tensors"], **t})
    with pytest.raises(ValueError, match="shape"):
        load_adapter(with_(**{name: torch.zeros(8, cfg.hidden_size + 1, dtype=BF)}), cfg, 64)
    with pytest.raises(ValueError, match="shape"):
        load_adapter(with_(**{name: torch.zeros(4, cfg.hidden_size, dtype=BF)}), cfg, 64)
    with pytest.raises(ValueError, match="lm_head"):
        load_adapter(with_(**{"base_model.model.lm_head.lora_A.weight": torch.zeros(8, cfg.hidden_size, dtype=BF)}), cfg, 64)
    with pytest.raises(ValueError, match="layers"):
        load_adapter(with_(**{name.replace("layers.0", "layers.9"): torch.zeros(8, cfg.hidden_size, dtype=BF)}), cfg, 64)
    with pytest.raises(ValueError, match="target_modules"):
        load_adapter(dict(ad, target_modules=["k_proj"]), cfg, 64)
    missing = dict(ad["tensors"])
    del missing[name.replace("lora_A", "lora_B")]
    with pytest.raises(ValueError, match="lora_B.weight is missing"):
        load_adapter(dict(ad, tensors=missing), cfg, 64)
    with pytest.raises(ValueError, match="tensors"):
        load_adapter({k: v for k, v in ad.items() if k != "tensors"}, cfg, 64)


# ---- packing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["tiny_llama", "tiny_qwen3"])
@pytest.mark.parametrize("modules", [LR.MODULES, ("q_proj", "v_proj", "up_proj")])
def test_fused_packing_is_exact(model, modules):
    """The packed B . A of a fused linear equals the row-mapped stack of its parts' B . A, exactly (float64 on bf16 inputs: both are
    the same sums of the same products, plus exact zeros), at every slot rank, with the padding zero."""
    from ssd_amd import quant
    from ssd_amd.lora import LINEARS, linear_shape, load_adapter, module_shapes, pack_linear, slot_rank
    cfg = _cfg(model)
    ad = load_adapter(_adapter(cfg, r=8, seed=5, modules=modules), cfg, 64)
    shapes = module_shapes(cfg)
    maps = {"qkv": quant.qkv_row_map(cfg.num_heads, cfg.num_kv_heads, cfg.head_dim).long(),
            "gate_up": quant.gate_up_row_map(2 * cfg.intermediate_size).long()}
    for max_rank in (16, 32, 64):
        for lin, parts in LINEARS.items():
            N, K = linear_shape(lin, cfg)
            R = slot_rank(lin, max_rank)
            assert R % 32 == 0 and len(parts) * max_rank <= R <= 192
            for li in range(cfg.num_layers):
                A, B = pack_linear(ad, li, lin, cfg, R)
                assert A.shape == (R, K) and B.shape == (N, R) and A.dtype == BF and B.dtype == BF
                assert not bool(A[len(parts) * 8:].any()) and not bool(B[:, len(parts) * 8:].any())       # rank padding
                want = torch.cat([(ad.tensors[(li, m)][1].double() @ ad.tensors[(li, m)][0].double()) if (li, m) in ad.tensors
                                  else torch.zeros(shapes[m][0], K, dtype=torch.float64) for m in parts])
                if lin in maps:
                    want = want[maps[lin]]
                assert torch.equal(B.double() @ A.double(), want), (lin, li, max_rank)
                if any((li, m) in ad.tensors for m in parts):
                    assert bool(want.any())


def test_rank_padding_leaves_the_delta_unchanged():
    from ssd_amd.lora import load_adapter, pack_linear
    cfg = _cfg("tiny_llama")
    ad = load_adapter(_adapter(cfg, r=8, seed=2), cfg, 64)
    small = pack_linear(ad, 1, "down", cfg, 32)
    big = pack_linear(ad, 1, "down", cfg, 64)
    assert torch.equal(small[1].double() @ small[0].double(), big[1].double() @ big[0].double())
    assert torch.equal(big[0][:8], ad.tensors[(1, "down_proj")][0]) and torch.equal(big[1][:, :8], ad.tensors[(1, "down_proj")][1])


# ---- registry and block hashes --------------------------------------------------------------------------------------
def test_registry_slots_and_identities():
    from ssd_amd.lora import LoraRegistry
    reg = LoraRegistry(2)
    sx = reg.free_slot("x")
    ix = reg.add("x", sx)
    sy = reg.free_slot("y")
    iy = reg.add("y", sy)
    assert {sx, sy} == {0, 1} and ix != iy and -1 not in (ix, iy) and 0 < ix < 2 ** 64 and reg.names() == ["x", "y"]
    assert reg.resolve("x") == (sx, ix)
    with pytest.raises(ValueError, match="'z'.*max_loras"):
        reg.free_slot("z")
    with pytest.raises(ValueError, match="already registered"):
        reg.free_slot("x")
    with pytest.raises(ValueError, match="lora='z'"):
        reg.resolve("z")
    assert reg.remove("x") == sx
    assert reg.add("x", reg.free_slot("x")) != ix           # registered again: another identity
    with pytest.raises(ValueError, match="not registered"):
        reg.remove("nope")


def _hashes(bm, seq):
    bm.allocate(seq)
    table = seq.draft_block_table if bm.is_draft else seq.block_table
    return [bm.blocks[b].hash for b in table]


def test_block_hashes_start_from_the_adapter_identity():
    from ssd_amd.engine.block_manager import BlockManager
    from ssd_amd.engine.sequence import Sequence
    from ssd_amd.lora import LoraRegistry
    from ssd_amd.sampling_params import SamplingParams
    Sequence.block_size = 4
    reg = LoraRegistry(4)
    X = (reg.free_slot("x"), reg.add("x", 0))
    Y = (reg.free_slot("y"), reg.add("y", 1))
    toks = list(range(1, 11))          # two full blocks and a partial one
    mk = lambda lora, name: Sequence(toks, SamplingParams(lora=name), lora=lora)
    fresh = lambda draft=False: BlockManager(16, 4, is_draft=draft)
    base, x1, x2, y = (_hashes(fresh(), s) for s in (mk(None, None), mk(X, "x"), mk(X, "x"), mk(Y, "y")))
    assert base[:2] == [BlockManager.compute_hash(toks[:4]), BlockManager.compute_hash(toks[4:8], BlockManager.compute_hash(toks[:4]))]
    assert base[2] == -1 and x1[2] == -1
    assert x1 == x2 and x1[:2] != base[:2] and x1[:2] != y[:2] and y[:2] != base[:2]
    assert x1[0] == BlockManager.compute_hash(toks[:4], X[1])
    reg.remove("x")
    X2 = (reg.free_slot("x"), reg.add("x", 0))
    assert X2[0] == X[0] and _hashes(fresh(), mk(X2, "x"))[:2] != x1[:2]
    # the draft's cache is not adapted: its hashes are the base's whatever the request names
    assert _hashes(fresh(True), mk(X, "x")) == _hashes(fresh(True), mk(None, None)) == base
    # sharing inside one manager: X after X hits, base after X and Y after X do not
    bm = fresh()
    first, second, plain, other = mk(X, "x"), mk(X, "x"), mk(None, None), mk(Y, "y")
    for s in (first, second, plain, other):
        bm.allocate(s)
    assert (first.num_cached_tokens, second.num_cached_tokens, plain.num_cached_tokens, other.num_cached_tokens) == (0, 8, 0, 0)
    assert second.block_table[:2] == first.block_table[:2] and not set(plain.block_table) & set(first.block_table)
    # a block that fills during decoding is labelled from the same root
    s = Sequence(toks[:3], SamplingParams(lora="x"), lora=X)
    bm2 = fresh()
    bm2.allocate(s)
    s.token_ids.append(toks[3])
    s.num_tokens += 1
    bm2.finalize_block(s, s.block_table, 0)
    assert bm2.blocks[s.block_table[0]].hash == x1[0]
    Sequence.block_size = 256


def test_sequence_keeps_the_adapter():
    from ssd_amd.engine.sequence import Sequence
    from ssd_amd.sampling_params import SamplingParams
    s = Sequence([1, 2, 3], SamplingParams(lora="x"), lora=(2, 77))
    assert (s.lora, s.lora_slot, s.lora_id) == ("x", 2, 77)
    s = Sequence([1, 2, 3], SamplingParams())
    assert (s.lora, s.lora_slot, s.lora_id) == (None, -1, -1)


# ---- engines that cannot run an adapter -----------------------------------------------------------------------------
def test_oracle_runner_engine_refuses_lora():
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    cfg = dataclasses.replace(_cfg("tiny_llama"))
    kw = dict(hf_config=cfg, max_model_len=256, max_num_batched_tokens=256, kvcache_block_size=16, num_kvcache_blocks=16)
    for enable in (False, True):
        eng = LLMEngine("t", runner_factory=oracle_runner_factory(), enable_lora=enable, **kw)
        with pytest.raises(ValueError, match="lora is not supported by OracleRunner"):
            eng.add_request([1, 2, 3], SamplingParams(lora="x", max_new_tokens=2))
        with pytest.raises(ValueError, match="lora|LoRA"):
            eng.add_lora("x", _adapter(cfg))
        assert eng.list_loras() == []
        out, _ = eng.generate([[1, 2, 3]], SamplingParams(temperature=0, max_new_tokens=2, ignore_eos=True), use_tqdm=False)
        assert len(out[0]["token_ids"]) == 2
