"""Weights: reference parameter names, TP sharding, synthetic generation and safetensors loading.

Parameter names are the reference's packed names (ssd/models/llama3.py:277-283, ssd/utils/loader.py:186-218):
  model.embed_tokens.weight [V,h]; model.layers.{i}.input_layernorm.weight; .self_attn.qkv_proj.weight
  [(nh+2nkv)hd, h] (+ .bias, + q_norm/k_norm for Qwen3); .self_attn.o_proj.weight [h, nh*hd];
  .post_attention_layernorm.weight; .mlp.gate_up_proj.weight [2I, h]; .mlp.down_proj.weight [h, I];
  model.norm.weight; lm_head.weight [V,h] (absent when tied).
A Qwen3-MoE layer (cfg.num_experts > 0) has, in place of the two MLP matrices, .mlp.gate.weight [E,h] (the router),
.mlp.experts.gate_up_proj [E,2I,h] (every expert's [gate ; up] halves) and .mlp.experts.down_proj [E,h,I] -- the fused names
transformers keeps in memory.
Sharding follows the reference weight loaders (ssd/layers/linear.py:90-95,116-122,148-162,188-193;
ssd/layers/embed_head.py:41-47).

No weights exist offline, so the default source is synthetic: every FULL tensor is a deterministic function
of (seed, name) -- independent of rank -- and is sharded afterwards, so TP=N computes the same function as TP=1.
"""
from __future__ import annotations

import glob
import hashlib
import os
from typing import Iterator

import torch

from ssd_amd.model_config import ModelConfig

BF16 = torch.bfloat16


def eagle_param_shapes(cfg: ModelConfig) -> list[tuple[str, tuple[int, ...]]]:
    """Eagle3DraftForCausalLM's parameters under the reference's module names (eagle3_draft_llama3.py:101-140,159-194,
    209-262): QKV reads the 2h-wide [token | conditioning] concatenation, the LM head covers draft_vocab_size tokens and
    ``d2t`` (int64, target id = draft id + d2t[draft id], :325-327) places them in the target vocabulary."""
    h, hd, nh, nkv, I = cfg.hidden_size, cfg.head_dim, cfg.num_heads, cfg.num_kv_heads, cfg.intermediate_size
    p = "model.layer."
    return [("model.embed_tokens.weight", (cfg.vocab_size, h)),
            ("fc.weight", (h, cfg.eagle_taps * cfg.d_model_target)),
            (p + "input_layernorm.weight", (h,)),
            (p + "conditioning_feature_ln.weight", (h,)),
            (p + "self_attn.qkv_proj.weight", ((nh + 2 * nkv) * hd, 2 * h)),
            (p + "self_attn.o_proj.weight", (h, nh * hd)),
            (p + "post_attention_layernorm.weight", (h,)),
            (p + "mlp.gate_up_proj.weight", (2 * I, h)),
            (p + "mlp.down_proj.weight", (h, I)),
            ("final_norm.weight", (h,)),
            ("lm_head.weight", (cfg.draft_vocab_size, h)),
            ("d2t", (cfg.draft_vocab_size,))]


# Qwen3-MoE parameter names below "model.layers.{i}." (transformers' Qwen3MoeSparseMoeBlock: the router, and the experts fused 3-D)
MOE_GATE, MOE_GATE_UP, MOE_DOWN = "mlp.gate.weight", "mlp.experts.gate_up_proj", "mlp.experts.down_proj"


def param_shapes(cfg: ModelConfig) -> list[tuple[str, tuple[int, ...]]]:
    if cfg.family == "eagle3":
        return eagle_param_shapes(cfg)
    h, hd, nh, nkv, I, V = cfg.hidden_size, cfg.head_dim, cfg.num_heads, cfg.num_kv_heads, cfg.intermediate_size, cfg.vocab_size
    out = [("model.embed_tokens.weight", (V, h))]
    for i in range(cfg.num_layers):
        p = f"model.layers.{i}."
        out.append((p + "input_layernorm.weight", (h,)))
        out.append((p + "self_attn.qkv_proj.weight", ((nh + 2 * nkv) * hd, h)))
        if cfg.attention_bias:
            out.append((p + "self_attn.qkv_proj.bias", ((nh + 2 * nkv) * hd,)))
        if cfg.qk_norm:
            out.append((p + "self_attn.q_norm.weight", (hd,)))
            out.append((p + "self_attn.k_norm.weight", (hd,)))
        out.append((p + "self_attn.o_proj.weight", (h, nh * hd)))
        out.append((p + "post_attention_layernorm.weight", (h,)))
        if cfg.num_experts > 0:
            E, Im = cfg.num_experts, cfg.moe_intermediate_size
            out.append((p + MOE_GATE, (E, h)))
            out.append((p + MOE_GATE_UP, (E, 2 * Im, h)))
            out.append((p + MOE_DOWN, (E, h, Im)))
            continue
        out.append((p + "mlp.gate_up_proj.weight", (2 * I, h)))
        out.append((p + "mlp.down_proj.weight", (h, I)))
    out.append(("model.norm.weight", (h,)))
    if not cfg.tie_word_embeddings:
        out.append(("lm_head.weight", (V, h)))
    return out


def _name_seed(seed: int, name: str) -> int:
    return int.from_bytes(hashlib.blake2b(f"{seed}:{name}".encode(), digest_size=7).digest(), "little")


def _pair_tensor(name: str, shape, seed: int, std: float, gen_device: str, recipe: dict) -> torch.Tensor | None:
    """The "correlated pair" recipe: a target and a draft of DIFFERENT shapes that agree on most greedy tokens by
    construction, so that speculation runs at a realistic acceptance rate without trained checkpoints.
      * both models embed a token with the same base vectors E_b[V, ds] (ds = recipe["shared"], the draft's hidden
        size) and read it out with the same base head H_b[V, ds]; a wider model fills its remaining hidden dims with
        independent noise, down-weighted through the gain on the shared dims: logits_target = snr * signal + noise,
        logits_draft = signal (recipe["snr"]; Monte Carlo at V = 128256: snr 4 -> 45 % top-1 agreement, 8 -> ~65 %);
      * o_proj / down_proj are scaled by recipe["layer_gain"], so the decoder layers perturb the residual stream
        (context-dependent, independent between the two models) instead of drowning the embedding.
    Every matrix keeps its real shape and is streamed in full; only the VALUES differ from the plain N(0, std) recipe."""
    ds, snr, lg = int(recipe["shared"]), float(recipe.get("snr", 8.0)), float(recipe.get("layer_gain", 0.005))
    pseed = int(recipe.get("seed", 1234))

    def randn(tag, shp):
        g = torch.Generator(device=gen_device)
        g.manual_seed(_name_seed(pseed, tag))
        return torch.randn(shp, generator=g, device=gen_device, dtype=torch.float32)

    if name in ("model.embed_tokens.weight", "lm_head.weight"):
        V, h = shape
        assert h >= ds
        is_embed = name.startswith("model.embed")
        base = randn("pair.embed" if is_embed else "pair.head", (V, ds))
        if h == ds:
            return (base * (1.0 if is_embed else std)).to(BF16)
        gain = snr * ((h - ds) / ds) ** 0.5 if is_embed else 1.0       # logit SNR = gain * sqrt(ds / (h - ds))
        rest = randn(f"pair.rest.{seed}.{name}", (V, h - ds))
        out = torch.cat([base * gain, rest], dim=1)
        return (out * (1.0 if is_embed else std)).to(BF16)
    if name.endswith("o_proj.weight") or name.endswith("down_proj.weight"):
        g = torch.Generator(device=gen_device)
        g.manual_seed(_name_seed(seed, name))
        return (std * lg * torch.randn(shape, generator=g, device=gen_device, dtype=torch.float32)).to(BF16)
    return None


def eagle_pair_recipe(target: ModelConfig, draft: ModelConfig, draft_seed: int, snr: float = 8.0, layer_gain: float = 0.005,
                      boost: float = 2.0, seed: int = 1234) -> dict:
    """The recipe dict (config.weights_recipe) of the constructed target + EAGLE-3 draft pair: see _eagle_pair_tensor."""
    assert draft.family == "eagle3" and draft.d_model_target == target.hidden_size
    sig = min(draft.num_kv_heads * draft.head_dim, target.hidden_size, draft.hidden_size)
    return {"kind": "eagle_pair", "sig": sig, "snr": snr, "layer_gain": layer_gain, "boost": boost, "seed": seed,
            "draft_seed": draft_seed, "draft_vocab": draft.draft_vocab_size, "target_vocab": target.vocab_size,
            "target_hidden": target.hidden_size, "draft_heads": (draft.num_heads, draft.num_kv_heads, draft.head_dim)}


def eagle_pair_gain(recipe: dict) -> float:
    """Gain of the shared embedding dims inside the TARGET's embedding rows (logit SNR = recipe["snr"], as in _pair_tensor)."""
    ds, ht = int(recipe["sig"]), int(recipe["target_hidden"])
    return float(recipe.get("snr", 8.0)) * ((ht - ds) / ds) ** 0.5 if ht > ds else 1.0


def _eagle_pair_tensor(name: str, shape, seed: int, std: float, gen_device: str, recipe: dict) -> torch.Tensor | None:
    """A target and its EAGLE-3 draft that AGREE by construction (round 3; the "peaky" pair only made both heads favour the same
    three tokens).  The target is the correlated-pair target of _pair_tensor over ds = recipe["sig"] shared dims: it embeds a
    token as [gain * E_b[tok] | noise], reads out with [H_b | noise], its layers perturb the residual stream only slightly
    (layer_gain), so its greedy next token is mostly g(tok) = argmax_v H_b[v] . E_b[tok]; the head rows of the tokens the draft
    vocabulary contains are scaled by recipe["boost"], so that the argmax falls inside that vocabulary.  The one-layer draft is
    wired to compute the same g from the token it is fed, whatever its conditioning row holds:
      * embedding [E_b[tok] | 0]; both input norms carry the weight sqrt(ds / h), so a row [x | ~0] comes out as ~[x | 0];
      * q / k = beta * A_kvhead . E_b[tok] (the conditioning half of the 2h-wide input is ignored): a row's score with ITSELF is
        beta^2 * sqrt(hd), with any other row ~N(0, beta^4) (RoPE leaves same-position dot products unchanged), so the softmax is
        one-hot on the row itself;
      * v = (token half) - (conditioning half) on the ds shared dims (ds = nkv * hd: one 128-wide slice per kv head), o_proj puts
        the slice of the first q head of each group back in place: attention output = E_b[tok] - conditioning, and the residual
        add of the conditioning leaves [E_b[tok] | ~0] whatever the conditioning was (fc(target taps) or the previous prenorm);
      * the MLP is scaled down like the target's, the head is [H_b[d2t] | 0]: logits = H_b . E_b[tok] -> g(tok) within the draft
        vocabulary.  fc copies the shared dims of the first tapped activation (divided by the target's gain), i.e. the first
        conditioning row has the same form as a prenorm.
    Every matrix keeps its real shape and is streamed in full; only the values are constructed."""
    ds = int(recipe["sig"])
    pseed = int(recipe.get("seed", 1234))
    lg = float(recipe.get("layer_gain", 0.005))
    V, Vd, ht = int(recipe["target_vocab"]), int(recipe["draft_vocab"]), int(recipe["target_hidden"])
    is_draft = recipe.get("family") == "eagle3"

    def randn(tag, shp):
        g = torch.Generator(device=gen_device)
        g.manual_seed(_name_seed(pseed, tag))
        return torch.randn(shp, generator=g, device=gen_device, dtype=torch.float32)

    def own(shp):
        g = torch.Generator(device=gen_device)
        g.manual_seed(_name_seed(seed, name))
        return torch.randn(shp, generator=g, device=gen_device, dtype=torch.float32)

    def draft_targets():            # target-vocabulary id of every draft-vocabulary id (d2t of the draft seed)
        gc = torch.Generator()
        gc.manual_seed(_name_seed(int(recipe["draft_seed"]), "d2t"))
        return torch.randperm(V, generator=gc)[:Vd].sort().values

    if (name.endswith("o_proj.weight") and not is_draft) or name.endswith("down_proj.weight"):
        return (std * lg * own(shape)).to(BF16)
    if not is_draft:
        if name == "model.embed_tokens.weight":
            h = shape[1]
            assert shape[0] == V and h == ht and h >= ds
            base = randn("epair.embed", (V, ds)) * eagle_pair_gain(recipe)
            return (base if h == ds else torch.cat([base, own((V, h - ds))], dim=1)).to(BF16)
        if name == "lm_head.weight":
            h = shape[1]
            base = randn("epair.head", (V, ds))
            out = base if h == ds else torch.cat([base, own((V, h - ds))], dim=1)
            out[draft_targets().to(out.device)] *= float(recipe.get("boost", 2.0))
            return (out * std).to(BF16)
        return None
    # ---- the EAGLE-3 draft ----
    nh, nkv, hd = (int(x) for x in recipe["draft_heads"])
    assert ds <= nkv * hd
    if name == "model.embed_tokens.weight":
        h = shape[1]
        out = torch.zeros(shape, dtype=torch.float32, device=gen_device)
        out[:, :ds] = randn("epair.embed", (V, ds))
        return out.to(BF16)
    if name == "lm_head.weight":
        out = torch.zeros(shape, dtype=torch.float32, device=gen_device)
        out[:, :ds] = randn("epair.head", (V, ds))[draft_targets().to(gen_device)]
        return (out * std).to(BF16)
    if name == "fc.weight":
        out = torch.zeros(shape, dtype=torch.float32, device=gen_device)
        idx = torch.arange(ds, device=gen_device)
        out[idx, idx] = 1.0 / eagle_pair_gain(recipe)          # first tap, shared dims
        return out.to(BF16)
    if name.endswith("input_layernorm.weight") or name.endswith("conditioning_feature_ln.weight"):
        return torch.full(shape, (ds / shape[0]) ** 0.5, dtype=torch.float32, device=gen_device).to(BF16)
    if name.endswith("qkv_proj.weight"):
        h = shape[1] // 2
        out = torch.zeros(shape, dtype=torch.float32, device=gen_device)
        beta = (16.0 / max(hd ** 0.5 - 3.5, 1.0)) ** 0.5
        grp = nh // nkv
        for k in range(nkv):
            A = randn(f"epair.A.{k}", (hd, ds)) * (beta / ds ** 0.5)
            for i in range(k * grp, (k + 1) * grp):
                out[i * hd:(i + 1) * hd, :ds] = A                                   # q heads of the group
            out[(nh + k) * hd:(nh + k + 1) * hd, :ds] = A                           # its k head
            r = torch.arange(min(hd, max(ds - k * hd, 0)), device=gen_device)
            rows = (nh + nkv + k) * hd + r                                          # its v head: token half - conditioning half
            out[rows, k * hd + r] = 1.0
            out[rows, h + k * hd + r] = -1.0
        return out.to(BF16)
    if name.endswith("o_proj.weight"):
        out = torch.zeros(shape, dtype=torch.float32, device=gen_device)
        grp = nh // nkv
        for k in range(nkv):
            r = torch.arange(min(hd, max(ds - k * hd, 0)), device=gen_device)
            out[k * hd + r, (k * grp) * hd + r] = 1.0
        return out.to(BF16)
    return None


def peaky_rows(recipe: dict) -> tuple[torch.Tensor, torch.Tensor]:
    """(draft-vocabulary ids, target-vocabulary ids) of the few tokens whose LM-head rows the "peaky" recipe scales in BOTH a
    target and its EAGLE-3 draft.  Random models never agree, and without agreement the speculation-cache hit path, partial
    acceptance and the extend rows of the EAGLE glue never run; with both heads favouring the same few tokens each model picks
    one of them most of the time and the same one about a third of the time (tests/eagle_util.py uses the same construction).
    The target ids are the draft ids pushed through the draft's d2t map, which is a function of (draft seed, vocabularies)."""
    Vd, V = int(recipe["draft_vocab"]), int(recipe["target_vocab"])
    gc = torch.Generator()
    gc.manual_seed(_name_seed(int(recipe["draft_seed"]), "d2t"))
    tgt = torch.randperm(V, generator=gc)[:Vd].sort().values          # = arange(Vd) + d2t of synthetic_tensor("d2t", ...)
    gp = torch.Generator()
    gp.manual_seed(int(recipe.get("seed", 99)))
    picks = torch.randperm(Vd, generator=gp)[:int(recipe.get("peaks", 3))]
    return picks, tgt[picks]


def synthetic_tensor(name: str, shape, seed: int, std: float, gen_device: str, norm_jitter: float = 0.0,
                     recipe: dict | None = None) -> torch.Tensor:
    """Full (unsharded) synthetic parameter.  gen_device="cpu" gives values reproducible on any machine (tests,
    oracle comparisons); "cuda" is for the multi-GB benchmark models."""
    if recipe is not None and recipe.get("kind") == "pair":
        t = _pair_tensor(name, shape, seed, std, gen_device, recipe)
        if t is not None:
            return t
    if recipe is not None and recipe.get("kind") == "eagle_pair":
        t = _eagle_pair_tensor(name, shape, seed, std, gen_device, recipe)
        if t is not None:
            return t
    g = torch.Generator(device=gen_device)
    g.manual_seed(_name_seed(seed, name))
    if name == "d2t":       # an increasing map of the draft vocabulary into the target's (like the frequency-sorted real ones)
        V = int(recipe["target_vocab"]) if recipe and "target_vocab" in recipe else None
        assert V is not None and V >= shape[0], "d2t needs recipe['target_vocab']"
        gc = torch.Generator()
        gc.manual_seed(_name_seed(seed, name))
        idx = torch.randperm(V, generator=gc)[:shape[0]].sort().values
        return (idx - torch.arange(shape[0])).to(torch.int64).to(gen_device)
    if "norm" in name or name.endswith("_ln.weight"):
        if norm_jitter == 0.0:
            return torch.ones(shape, dtype=BF16, device=gen_device)
        return (1.0 + norm_jitter * torch.randn(shape, generator=g, device=gen_device, dtype=torch.float32)).to(BF16)
    t = std * torch.randn(shape, generator=g, device=gen_device, dtype=torch.float32)
    if recipe is not None and name.endswith(MOE_GATE):
        # router_gain (any recipe kind): a multiple of the synthetic router matrix, i.e. of every router logit -- random routers
        # decide by margins of a few bf16 ulps, and a test that compares routes needs them wide
        t = t * float(recipe.get("router_gain", 1.0))
    if recipe is not None and recipe.get("kind") == "peaky" and name == "lm_head.weight":
        dpicks, tpicks = peaky_rows(recipe)
        rows = dpicks if shape[0] == int(recipe["draft_vocab"]) else tpicks
        t[rows.to(t.device)] *= float(recipe.get("gain", 6.0))
    return t.to(BF16)


def shard_param(cfg: ModelConfig, name: str, w: torch.Tensor, rank: int, tp: int) -> torch.Tensor:
    if tp == 1:
        return w
    hd, nh, nkv, I = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads, cfg.intermediate_size
    if name.endswith("qkv_proj.weight") or name.endswith("qkv_proj.bias"):
        q, k, v = w.split([nh * hd, nkv * hd, nkv * hd], dim=0)
        return torch.cat([q.chunk(tp, 0)[rank], k.chunk(tp, 0)[rank], v.chunk(tp, 0)[rank]], 0).contiguous()
    if name.endswith("gate_up_proj.weight"):
        g, u = w.split([I, I], dim=0)
        return torch.cat([g.chunk(tp, 0)[rank], u.chunk(tp, 0)[rank]], 0).contiguous()
    if name.endswith("o_proj.weight") or name.endswith("down_proj.weight"):
        return w.chunk(tp, 1)[rank].contiguous()
    if name.endswith("embed_tokens.weight") or name.endswith("lm_head.weight"):
        return w.chunk(tp, 0)[rank].contiguous()
    return w


def synthetic_weights(cfg: ModelConfig, seed: int, std: float, rank: int = 0, tp: int = 1, gen_device: str = "cpu",
                      out_device: str | None = None, norm_jitter: float = 0.0,
                      recipe: dict | None = None) -> Iterator[tuple[str, torch.Tensor]]:
    """Yields (name, this rank's shard) one tensor at a time (bounded transient memory for 70B)."""
    if cfg.family == "eagle3":          # d2t needs the target vocabulary size; the draft is never tensor-parallel
        assert tp == 1
        recipe = dict(recipe or {}, target_vocab=cfg.vocab_size)
        if recipe.get("kind") == "eagle_pair":
            assert int(recipe["draft_seed"]) == seed and int(recipe["draft_vocab"]) == cfg.draft_vocab_size, "eagle_pair recipe: draft seed / vocabulary mismatch"
        if recipe.get("kind") == "peaky":
            assert int(recipe["draft_seed"]) == seed and int(recipe["draft_vocab"]) == cfg.draft_vocab_size, "peaky recipe: draft seed / vocabulary mismatch"
    if recipe is not None and recipe.get("kind") == "eagle_pair":
        recipe = dict(recipe, family=cfg.family)
    for name, shape in param_shapes(cfg):
        w = shard_param(cfg, name, synthetic_tensor(name, shape, seed, std, gen_device, norm_jitter, recipe), rank, tp)
        yield name, (w.to(out_device) if out_device is not None else w)


def synthetic_state_dict(cfg: ModelConfig, seed: int, std: float, norm_jitter: float = 0.0, recipe: dict | None = None) -> dict:
    return dict(synthetic_weights(cfg, seed, std, gen_device="cpu", norm_jitter=norm_jitter, recipe=recipe))


# --------------------------------------------------------------------------------------------------
# HF safetensors (reference ssd/utils/loader.py:186-218): q/k/v and gate/up are packed by concatenation
# --------------------------------------------------------------------------------------------------


def has_safetensors(model_dir: str) -> bool:
    return os.path.isdir(model_dir) and bool(glob.glob(os.path.join(model_dir, "*.safetensors")))


def load_eagle_safetensors(cfg: ModelConfig, model_dir: str, target_dir: str | None = None,
                           out_device: str | None = None) -> Iterator[tuple[str, torch.Tensor]]:
    """EAGLE-3 checkpoints (reference load_eagle_model, ssd/utils/loader.py:64-183): a flat state dict with
    midlayer.* (q/k/v and gate/up unpacked, hidden_norm = the conditioning-feature norm), norm.weight (final norm),
    fc.weight, lm_head.weight, d2t / t2d, and embed_tokens.weight -- taken from the TARGET checkpoint when the draft
    ships none (:118-125, load_embedding_from_target :9-61)."""
    from safetensors import safe_open
    sd: dict[str, torch.Tensor] = {}
    for f in sorted(glob.glob(os.path.join(model_dir, "*.safetensors"))):
        with safe_open(f, "pt", "cpu") as sf:
            for k in sf.keys():
                sd[k] = sf.get_tensor(k)
    if "embed_tokens.weight" not in sd:
        assert target_dir is not None and has_safetensors(target_dir), "EAGLE-3 draft without embed_tokens needs the target checkpoint"
        for f in sorted(glob.glob(os.path.join(target_dir, "*.safetensors"))):
            with safe_open(f, "pt", "cpu") as sf:
                for k in sf.keys():
                    if k.endswith("embed_tokens.weight"):
                        sd["embed_tokens.weight"] = sf.get_tensor(k)
        assert "embed_tokens.weight" in sd, f"no embed_tokens.weight under {target_dir}"
    ml = "midlayer."
    src = {
        "model.embed_tokens.weight": lambda: sd["embed_tokens.weight"],
        "fc.weight": lambda: sd["fc.weight"],
        "model.layer.input_layernorm.weight": lambda: sd[ml + "input_layernorm.weight"],
        "model.layer.conditioning_feature_ln.weight": lambda: sd[ml + "hidden_norm.weight"],
        "model.layer.self_attn.qkv_proj.weight": lambda: torch.cat([sd[ml + f"self_attn.{x}_proj.weight"] for x in "qkv"], 0),
        "model.layer.self_attn.o_proj.weight": lambda: sd[ml + "self_attn.o_proj.weight"],
        "model.layer.post_attention_layernorm.weight": lambda: sd[ml + "post_attention_layernorm.weight"],
        "model.layer.mlp.gate_up_proj.weight": lambda: torch.cat([sd[ml + "mlp.gate_proj.weight"], sd[ml + "mlp.up_proj.weight"]], 0),
        "model.layer.mlp.down_proj.weight": lambda: sd[ml + "mlp.down_proj.weight"],
        "final_norm.weight": lambda: sd["norm.weight"],
        "lm_head.weight": lambda: sd["lm_head.weight"],
        "d2t": lambda: sd["d2t"],
    }
    for name, shape in eagle_param_shapes(cfg):
        w = src[name]()
        w = w.to(torch.int64) if name == "d2t" else w.to(BF16)
        assert tuple(w.shape) == tuple(shape), f"{name}: {tuple(w.shape)} != {shape}"
        yield name, (w.to(out_device) if out_device is not None else w)


def _quantization_config(model_dir: str) -> dict | None:
    import json
    path = os.path.join(model_dir, "config.json")
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f).get("quantization_config") or None


# AutoAWQ / GPTQ int4 checkpoints: every config field name, tensor suffix, the AWQ nibble order and the GPTQ zero-point convention,
# kept in one place.  They are written from the formats' public descriptions; the config field names were compared with AwqConfig
# and GPTQConfig of transformers (utils/quantization_config.py: bits, group_size, zero_point, version with format as its newer
# name; bits, group_size, desc_act, sym, checkpoint_format with format as its newer name).  No AutoAWQ / auto-gptq / gptqmodel
# package was available, so the tensor layouts have not been checked against a published checkpoint ("W4A16 with zero
# points").
AWQ_METHOD, GPTQ_METHOD = "awq", "gptq"
INT4_BITS_FIELD, INT4_GROUP_FIELD = "bits", "group_size"
AWQ_ZERO_POINT_FIELD, AWQ_VERSION_FIELDS, AWQ_VERSIONS = "zero_point", ("version", "format"), ("gemm",)
GPTQ_DESC_ACT_FIELD, GPTQ_SYM_FIELD, GPTQ_FORMAT_FIELDS = "desc_act", "sym", ("checkpoint_format", "format")
GPTQ_ZERO_OFFSET = {"gptq": 1, "gptq_v2": 0}       # format -> what the stored zero nibble is short of z ("gptq" stores z - 1)
GPTQ_DEFAULT_FORMAT = "gptq"
INT4_QWEIGHT_SUFFIX, INT4_QZEROS_SUFFIX, INT4_SCALES_SUFFIX, GPTQ_G_IDX_SUFFIX = ".qweight", ".qzeros", ".scales", ".g_idx"
# AWQ (gemm): nibble position i (bits 4i .. 4i+3) of word j holds output column 8j + AWQ_ORDER[i], in qweight and in qzeros
AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)


def int4_checkpoint_scheme(qc: dict | None) -> dict | None:
    """{"method": "awq" | "gptq", "zero_offset": 0 | 1} for the AutoAWQ / GPTQ schemes a W4A16 target runs (4 bits, groups of 128
    columns; AWQ: zero points, gemm packing; GPTQ: no activation order, format gptq or gptq_v2, symmetric or not), None for any other
    quant_method; every other AWQ / GPTQ variant is refused here by name."""
    method = (qc or {}).get("quant_method")
    if method not in (AWQ_METHOD, GPTQ_METHOD):
        return None
    if qc.get(INT4_BITS_FIELD) != 4:
        raise ValueError(f"unsupported {method} {INT4_BITS_FIELD} {qc.get(INT4_BITS_FIELD)!r}: only 4-bit weights can be loaded")
    if qc.get(INT4_GROUP_FIELD) != 128:
        raise ValueError(f"unsupported {method} {INT4_GROUP_FIELD} {qc.get(INT4_GROUP_FIELD)!r}: only groups of 128 columns")
    if method == AWQ_METHOD:
        if qc.get(AWQ_ZERO_POINT_FIELD) is not True:
            raise ValueError(f"unsupported awq {AWQ_ZERO_POINT_FIELD} {qc.get(AWQ_ZERO_POINT_FIELD)!r}: only zero_point true")
        version = next((qc[f] for f in AWQ_VERSION_FIELDS if qc.get(f) is not None), None)
        if str(version).lower() not in AWQ_VERSIONS:
            raise ValueError(f"unsupported awq version {version!r}: only the gemm packing (not gemv / gemv_fast / marlin)")
        return {"method": AWQ_METHOD, "zero_offset": 0}
    if qc.get(GPTQ_DESC_ACT_FIELD) is not False:
        raise ValueError(f"unsupported gptq {GPTQ_DESC_ACT_FIELD} {qc.get(GPTQ_DESC_ACT_FIELD)!r}: activation-order checkpoints "
                         "(desc_act true, a g_idx permutation) are not supported")
    if qc.get(GPTQ_SYM_FIELD) not in (True, False):
        raise ValueError(f"gptq {GPTQ_SYM_FIELD} must be true or false, got {qc.get(GPTQ_SYM_FIELD)!r}")
    fmt = next((qc[f] for f in GPTQ_FORMAT_FIELDS if qc.get(f) is not None), GPTQ_DEFAULT_FORMAT)
    if str(fmt).lower() not in GPTQ_ZERO_OFFSET:
        raise ValueError(f"unsupported gptq checkpoint format {fmt!r}: only {sorted(GPTQ_ZERO_OFFSET)} (not marlin / bitblas)")
    return {"method": GPTQ_METHOD, "zero_offset": GPTQ_ZERO_OFFSET[str(fmt).lower()]}


# Block-scaled FP8 checkpoints (the Qwen3-*-FP8 / DeepSeek-style exports): the config field names and the tensor suffix, kept in
# one place.  They are written from memory of the format and have not been checked against a published checkpoint (DESIGN.md,
# "Block-scaled FP8 checkpoints"): quantization_config = {"quant_method": "fp8", "fmt": "e4m3", "weight_block_size": [128, 128],
# "activation_scheme": "dynamic"}, every quantized linear X stored as X.weight (float8_e4m3fn [N, K]) and X.weight_scale_inv
# ([ceil(N / 128), ceil(K / 128)], W = weight_scale_inv[n // 128, k // 128] * code[n, k]); linears listed under
# modules_to_not_convert / ignored_layers are stored as plain bf16 .weight tensors (the tensor's dtype decides here, not the list).
FP8_BLOCK_METHOD = "fp8"
FP8_BLOCK_SIZE_FIELD, FP8_BLOCK_FMT_FIELD, FP8_BLOCK_FMTS = "weight_block_size", "fmt", (None, "e4m3")
FP8_BLOCK_ACTIVATION_FIELD = "activation_scheme"        # read and ignored: activations stay bf16
FP8_BLOCK_SKIP_FIELDS = ("modules_to_not_convert", "ignored_layers")
FP8_BLOCK_SCALE_SUFFIX = "_scale_inv"                   # appended to "<linear>.weight"


def fp8_block_scheme(qc: dict | None) -> bool:
    """True for the block-scaled fp8 scheme an fp8 target runs (quant_method "fp8" without compressed-tensors config_groups, e4m3
    codes, 128 x 128 blocks), False for any other quantization_config; other block sizes, fmt e5m2 and a missing block size
    (AutoFP8-style per-tensor checkpoints) are refused here by name."""
    if not qc or qc.get("quant_method") != FP8_BLOCK_METHOD or "config_groups" in qc:
        return False
    fmt = qc.get(FP8_BLOCK_FMT_FIELD)
    if (fmt.lower() if isinstance(fmt, str) else fmt) not in FP8_BLOCK_FMTS:
        raise ValueError(f"unsupported fp8 {FP8_BLOCK_FMT_FIELD} {fmt!r}: only e4m3 (OCP float8_e4m3fn) codes can be loaded")
    bs = qc.get(FP8_BLOCK_SIZE_FIELD)
    if bs is None:
        raise ValueError(f"unsupported fp8 checkpoint without {FP8_BLOCK_SIZE_FIELD}: per-tensor (AutoFP8-style) quant_method 'fp8' "
                         "checkpoints are not supported, only 128 x 128 block scales")
    from ssd_amd.quant import FP8_BLOCK
    if list(bs) != [FP8_BLOCK, FP8_BLOCK]:
        raise ValueError(f"unsupported fp8 {FP8_BLOCK_SIZE_FIELD} {bs!r}: only [{FP8_BLOCK}, {FP8_BLOCK}]")
    qc.get(FP8_BLOCK_ACTIVATION_FIELD)      # "dynamic" or "static": activations stay bf16 either way
    return True


def checkpoint_quantization(model_dir: str) -> str | None:
    """"fp8" for a compressed-tensors checkpoint with float 8-bit weights and per-channel or per-tensor scales and for a block-scaled
    fp8 one (fp8_block_scheme), "w4a16" for a pack-quantized one with symmetric int4 weights in groups of 128 columns and for an
    AutoAWQ / GPTQ one (int4_checkpoint_scheme), "mxfp4" for an MXFP4 one (config.json quantization_config), None for an
    unquantized one; every other quantization format is refused here, before any tensor is read."""
    return _checkpoint_kind(_quantization_config(model_dir))


def _checkpoint_kind(qc: dict | None) -> str | None:
    """checkpoint_quantization on an already parsed quantization_config."""
    if not qc:
        return None
    method = qc.get("quant_method")
    if int4_checkpoint_scheme(qc) is not None:
        return "w4a16"
    if fp8_block_scheme(qc):
        return "fp8"
    if method != "compressed-tensors":
        raise ValueError(f"unsupported quantization_config.quant_method {method!r}: only compressed-tensors float8 checkpoints "
                         "(per-channel or per-tensor weight scales), pack-quantized int4 ones (group 128), MXFP4 ones, AutoAWQ / "
                         "GPTQ int4 ones (group 128), and block-scaled fp8 ones (quant_method 'fp8', weight_block_size [128, 128]) can "
                         "be loaded")
    groups = qc.get("config_groups") or {}
    if not groups:
        raise ValueError("compressed-tensors checkpoint without config_groups")
    kinds = set()
    for gname, g in groups.items():
        wq = g.get("weights") or {}
        if wq.get("type") == "int" and wq.get("num_bits") == 4:
            kinds.add(_w4a16_scheme(gname, wq, qc.get("format")))
            continue
        if wq.get("type") == "float" and wq.get("num_bits") == 4:
            kinds.add(_mxfp4_scheme(gname, wq, qc.get("format")))
            continue
        if wq.get("type") != "float" or wq.get("num_bits") != 8 or wq.get("strategy") not in ("channel", "tensor"):
            raise ValueError(f"unsupported compressed-tensors weight scheme in {gname}: {wq} (supported: type float, num_bits 8, "
                             "strategy channel or tensor; or type int, num_bits 4, strategy group, group_size 128; or type float, num_bits 4, "
                             "strategy group, group_size 32)")
        kinds.add("fp8")
    if len(kinds) > 1:
        raise ValueError(f"compressed-tensors checkpoint mixes weight schemes {sorted(kinds)}")
    return kinds.pop()


# compressed-tensors names of an MXFP4 checkpoint, kept in one place: they are written from memory of the format and have not been
# checked against a published checkpoint ("MXFP4 weight-only targets")
MXFP4_FORMAT = "mxfp4-pack-quantized"
MXFP4_PACKED_SUFFIX, MXFP4_SCALE_SUFFIX, FP4_GLOBAL_SCALE_SUFFIX = ".weight_packed", ".weight_scale", ".weight_global_scale"


def _mxfp4_scheme(gname: str, wq: dict, fmt) -> str:
    """The float-4 scheme an MXFP4 target runs: e2m1 codes, symmetric, one e8m0 (uint8) scale per 32-column group, mxfp4-pack-quantized.
    NVFP4 (group size 16, fp8-typed scales, a global scale) is refused here by name."""
    if wq.get("group_size") == 16 or fmt == "nvfp4-pack-quantized":
        raise ValueError(f"unsupported float-4 scheme in {gname}: group_size {wq.get('group_size')!r} / format {fmt!r} is NVFP4; only "
                         f"MXFP4 (format {MXFP4_FORMAT}, group_size 32, e8m0 scales) can be loaded")
    if fmt != MXFP4_FORMAT:
        raise ValueError(f"unsupported compressed-tensors format {fmt!r} for float-4 weights in {gname}: only {MXFP4_FORMAT}")
    if wq.get("strategy") != "group":
        raise ValueError(f"unsupported float-4 weight strategy {wq.get('strategy')!r} in {gname}: only strategy group")
    if wq.get("group_size") != 32:
        raise ValueError(f"unsupported float-4 group_size {wq.get('group_size')!r} in {gname}: only 32 (MXFP4)")
    if wq.get("symmetric") is not True:
        raise ValueError(f"asymmetric float-4 weights in {gname} are not supported: symmetric only")
    sd = wq.get("scale_dtype")
    if sd is not None and "uint8" not in str(sd) and "e8m0" not in str(sd):
        raise ValueError(f"unsupported float-4 scale_dtype {sd!r} in {gname}: fp8-typed scales are NVFP4; MXFP4 scales are e8m0 (uint8)")
    return "mxfp4"


def _w4a16_scheme(gname: str, wq: dict, fmt) -> str:
    """The int4 scheme a W4A16 target runs: symmetric, one scale per 128-column group, no activation reordering, pack-quantized."""
    if fmt != "pack-quantized":
        raise ValueError(f"unsupported compressed-tensors format {fmt!r} for int4 weights in {gname}: only pack-quantized")
    if wq.get("symmetric") is not True:
        raise ValueError(f"asymmetric int4 weights (zero points) in {gname} are not supported: symmetric only")
    if wq.get("strategy") != "group":
        raise ValueError(f"unsupported int4 weight strategy {wq.get('strategy')!r} in {gname}: only strategy group")
    if wq.get("group_size") != 128:
        raise ValueError(f"unsupported int4 group_size {wq.get('group_size')!r} in {gname}: only 128")
    if wq.get("actorder") not in (None, False, "static"):
        raise ValueError(f"int4 weights with actorder {wq.get('actorder')!r} in {gname} are not supported (no g_idx reordering)")
    return "w4a16"


def _packed_sources(name: str) -> list[str] | None:
    if "qkv_proj" in name:
        return [name.replace("qkv_proj", s) for s in ("q_proj", "k_proj", "v_proj")]
    if "gate_up_proj" in name:
        return [name.replace("gate_up_proj", s) for s in ("gate_proj", "up_proj")]
    return None


def _unpack_nibbles(words: torch.Tensor, order=None) -> torch.Tensor:
    """int32 [R, C] -> uint8 [R, 8 C]: nibble position i of word j is column 8j + order[i] (order None: 8j + i)."""
    shifts = torch.arange(0, 32, 4, dtype=torch.int64, device=words.device)
    nib = (words.to(torch.int64)[..., None] >> shifts) & 0xF                 # [R, C, 8] by nibble position
    if order is not None:
        out = torch.empty_like(nib)
        out[..., torch.tensor(order, device=words.device)] = nib
        nib = out
    return nib.reshape(words.shape[0], -1).to(torch.uint8)


def _safetensors_index(model_dir: str, device: str | None = None):
    """(index, raw): the file that holds every tensor name under model_dir, and raw(name) = that tensor as stored (on `device`, if
    one is given)."""
    from safetensors import safe_open
    index: dict[str, str] = {}
    for f in sorted(glob.glob(os.path.join(model_dir, "*.safetensors"))):
        with safe_open(f, "pt", "cpu") as sf:
            for k in sf.keys():
                index[k] = f

    def raw(name: str) -> torch.Tensor:
        with safe_open(index[name], "pt", "cpu") as sf:
            t = sf.get_tensor(name)
        return t.to(device) if device is not None else t

    return index, raw


def _assemble(cfg: ModelConfig, name: str, shape, parts: list, target: str | None, rank: int, tp: int, out_device: str | None):
    """One parameter from its parts (q | k | v, gate | up, or the tensor alone), each a bf16 tensor or a host form of ssd_amd/quant.py.
    Parts of one quantized form that the target (its `quantization` value; None: bf16) runs natively stay in that form, packed
    row-wise; for any other target their packed form is dequantized; mixed parts are dequantized one by one and packed as bf16.
    bf16 results are sharded as usual."""
    from ssd_amd import quant
    if quant.is_prequantized(parts[0]) and len({type(p) for p in parts}) == 1:
        w = quant.cat_rows(parts)
        if w.native == target:
            assert w.shape() == tuple(shape), f"{name}: {w.shape()} != {shape}"
            return quant.to_device(w, out_device)
        w = w.dequantize()
    else:
        w = torch.cat([p.dequantize() if quant.is_prequantized(p) else p for p in parts], dim=0)
    assert tuple(w.shape) == tuple(shape), f"{name}: {tuple(w.shape)} != {shape}"
    w = shard_param(cfg, name, w, rank, tp)
    return w.to(out_device) if out_device is not None else w


def _load_awq_gptq(cfg: ModelConfig, model_dir: str, scheme: dict, rank: int, tp: int, out_device: str | None,
                   w4a16: bool) -> Iterator[tuple[str, torch.Tensor]]:
    """The AutoAWQ / GPTQ side of load_safetensors.  A quantized linear is unpacked, transposed to [N, K] and repacked on out_device,
    one tensor at a time; q / k / v and gate / up are concatenated into the packed names.  A w4a16 target gets
    quant.W4ZTensor(packed, scale, zero) (fp16 scales rounded to bf16 once), or the plain symmetric W4Tensor when every zero point
    of the linear is 8; any other target gets bf16(s * (u - z)), sharded as usual.  A linear stored only as an unquantized .weight
    (AWQ modules_to_not_convert, the LM head), norms and embeddings load as bf16."""
    from ssd_amd.quant import W4ZTensor, W4_GROUP, pack_w4u, w4z_as_symmetric
    awq = scheme["method"] == AWQ_METHOD
    index, raw = _safetensors_index(model_dir, out_device)

    def get_q(base: str) -> W4ZTensor:
        qw, qz, sc = raw(base + INT4_QWEIGHT_SUFFIX), raw(base + INT4_QZEROS_SUFFIX), raw(base + INT4_SCALES_SUFFIX)
        if qw.dtype != torch.int32 or qz.dtype != torch.int32:
            raise ValueError(f"{base}: qweight / qzeros are {qw.dtype} / {qz.dtype}, expected int32")
        if sc.dtype not in (BF16, torch.float16, torch.float32):
            raise ValueError(f"{base}{INT4_SCALES_SUFFIX} is {sc.dtype}: expected fp16, bf16 or fp32")
        if awq:
            K, N = qw.shape[0], qw.shape[1] * 8
            packed = pack_w4u(_unpack_nibbles(qw, AWQ_ORDER).t().contiguous())            # [K, N] -> [N, K] -> words
            stored = _unpack_nibbles(qz, AWQ_ORDER)
        else:
            K, N = qw.shape[0] * 8, qw.shape[1]
            packed = qw.t().contiguous()             # word [j, n] = input columns 8j .. 8j+7 of output n: the row form's word [n, j]
            stored = _unpack_nibbles(qz)
            if base + GPTQ_G_IDX_SUFFIX in index:
                g_idx = raw(base + GPTQ_G_IDX_SUFFIX).reshape(-1).to(torch.int64)
                if g_idx.numel() != K or not torch.equal(g_idx, torch.arange(K, device=g_idx.device) // W4_GROUP):
                    raise ValueError(f"{base}{GPTQ_G_IDX_SUFFIX} is not k // {W4_GROUP}: activation-order (g_idx) checkpoints are not "
                                     "supported")
        if K % W4_GROUP or tuple(qz.shape) != (K // W4_GROUP, N // 8) or tuple(sc.shape) != (K // W4_GROUP, N):
            raise ValueError(f"{base}: qweight {tuple(qw.shape)}, qzeros {tuple(qz.shape)}, scales {tuple(sc.shape)} do not describe "
                             f"a [{N}, {K}] matrix in groups of {W4_GROUP}")
        zero = ((stored.to(torch.int16) + scheme["zero_offset"]) & 15).to(torch.uint8).t().contiguous()
        return W4ZTensor(packed, sc.to(BF16).t().contiguous(), zero)

    def get(name: str):
        base = name[:-len(".weight")] if name.endswith(".weight") else None
        if name not in index and base is not None and base + INT4_QWEIGHT_SUFFIX in index:
            return get_q(base)
        t = raw(name)
        if not t.dtype.is_floating_point or t.element_size() == 1:
            raise ValueError(f"{name} is {t.dtype}: expected an unquantized fp16 / bf16 / fp32 tensor")
        return t.to(BF16)

    for name, shape in param_shapes(cfg):
        srcs = _packed_sources(name)
        whole = name in index or name[:-len(".weight")] + INT4_QWEIGHT_SUFFIX in index
        parts = [get(s) for s in srcs] if srcs is not None and not whole else [get(name)]
        quantized = [isinstance(p, W4ZTensor) for p in parts]
        if w4a16 and any(quantized) and not all(quantized):
            import warnings
            warnings.warn(f"{name}: only some of {srcs} are quantized in the checkpoint; the packed matrix is dequantized and the "
                          "w4a16 target quantizes it again on load (lossy for the parts that were int4)")
        w = _assemble(cfg, name, shape, parts, "w4a16" if w4a16 else None, rank, tp, out_device)
        yield name, (w4z_as_symmetric(w) if isinstance(w, W4ZTensor) else w)


def _moe_experts(name: str, shape, index: dict, get) -> torch.Tensor:
    """A layer's fused expert tensor [E, 2I, h] / [E, h, I]: the fused 3-D name as it is (what transformers keeps in memory and
    save_pretrained writes), or stacked from the published per-expert names mlp.experts.{e}.gate_proj / up_proj / down_proj.weight
    ([gate ; up] halves per expert)."""
    if name in index:
        w = get(name)
    else:
        base = name[:name.rindex(".")]              # "...mlp.experts"
        E = shape[0]
        miss = [f"{base}.{e}.down_proj.weight" for e in range(E) if f"{base}.{e}.down_proj.weight" not in index]
        if miss:
            raise ValueError(f"{name}: the checkpoint has neither the fused tensor nor {miss[0]}")
        if name.endswith(MOE_GATE_UP):
            w = torch.stack([torch.cat([get(f"{base}.{e}.gate_proj.weight"), get(f"{base}.{e}.up_proj.weight")], 0) for e in range(E)])
        else:
            w = torch.stack([get(f"{base}.{e}.down_proj.weight") for e in range(E)])
    if not isinstance(w, torch.Tensor) or tuple(w.shape) != tuple(shape):
        raise ValueError(f"{name}: expected a bf16 tensor of shape {tuple(shape)}, got {tuple(w.shape) if isinstance(w, torch.Tensor) else type(w).__name__}")
    return w.contiguous()


def load_safetensors(cfg: ModelConfig, model_dir: str, rank: int = 0, tp: int = 1,
                     out_device: str | None = None, fp8: bool = False, w4a16: bool = False,
                     mxfp4: bool = False) -> Iterator[tuple[str, torch.Tensor]]:
    """Yields (name, bf16 tensor), and for a quantized decoder linear of a quantized checkpoint (checkpoint_quantization) one of
    the host forms of ssd_amd/quant.py instead when the consumer is a target of that kind (``fp8`` / ``w4a16`` / ``mxfp4``: codes and
    scales bit for bit, no re-quantization; _assemble has the rule); a bf16 consumer gets the exact dequantized bf16 matrix, sharded
    as usual, and a quantized target of another kind is refused before any tensor is read.  The forms, by checkpoint:
      * compressed-tensors fp8: quant.FP8Tensor(q float8_e4m3fn [N, K], s fp32 [N]); per-tensor scales of q / k / v and gate / up are
        expanded to one per row before the packing; input_scale tensors (activation quantization) are ignored;
      * block-scaled fp8 (fp8_block_scheme): quant.FP8BTensor(codes, rowscale fp32 [N, ceil(K / 128)]), every source tensor's
        weight_scale_inv expanded to one row of block scales per output row, then concatenated;
      * pack-quantized int4: quant.W4Tensor(packed int32 [N, K/8], scale bf16 [N, K/128]); fp16 / fp32 scales are rounded to bf16 once;
      * AutoAWQ / GPTQ int4 (_load_awq_gptq): quant.W4ZTensor(packed, scale, zero), a plain W4Tensor when all its zero points are 8;
      * MXFP4: quant.MX4Tensor(packed uint8 [N, K/2], scale uint8 [N, K/32]); scale bytes outside 2..252 are refused.
    Unquantized tensors (e.g. the LM head) load as bf16."""
    from ssd_amd.quant import FP8, FP8Tensor, W4Tensor, MX4Tensor, check_mxfp4_scales, FP8_BLOCK, FP8BTensor, expand_fp8_block_scales
    assert fp8 + w4a16 + mxfp4 <= 1
    target = "fp8" if fp8 else "w4a16" if w4a16 else "mxfp4" if mxfp4 else None
    qc = _quantization_config(model_dir)
    kind = _checkpoint_kind(qc)
    scheme = int4_checkpoint_scheme(qc)
    if target is not None and kind is not None and kind != target:
        what = f"{scheme['method']} int4" if scheme is not None else kind
        raise ValueError(f"a checkpoint of the {what} kind cannot load into the {target} target: use quantization={kind!r} or None")
    assert target is None or tp == 1, f"{target} targets are single-rank"
    if scheme is not None:
        yield from _load_awq_gptq(cfg, model_dir, scheme, rank, tp, out_device, w4a16)
        return
    ckpt_fp8 = kind == "fp8"
    block = fp8_block_scheme(qc)
    index, raw = _safetensors_index(model_dir)
    if not block and any(k.endswith("weight_scale_inv") for k in index):
        raise ValueError("block-scaled fp8 checkpoints (weight_scale_inv) are not supported: use per-channel or per-tensor scales")
    for k in index:
        if k.endswith(FP4_GLOBAL_SCALE_SUFFIX):
            raise ValueError(f"{k}: float-4 weights with a global scale tensor (NVFP4) are not supported; only MXFP4")
    for k in index:
        if k.endswith("weight_zero_point"):
            raise ValueError(f"{k}: asymmetric int4 weights (zero points) are not supported")
        if k.endswith("weight_g_idx"):
            raise ValueError(f"{k}: int4 weights with activation reordering (g_idx) are not supported")

    def get_w4(name: str) -> W4Tensor:
        base = name[:-len(".weight")]
        if kind != "w4a16":
            raise ValueError(f"{base}.weight_packed is int4 but config.json declares no pack-quantized int4 scheme")
        packed, s = raw(base + ".weight_packed"), raw(base + ".weight_scale")
        N, KW = packed.shape
        if packed.dtype != torch.int32:
            raise ValueError(f"{base}.weight_packed is {packed.dtype}: expected int32")
        if base + ".weight_shape" in index:
            shp = tuple(int(v) for v in raw(base + ".weight_shape").reshape(-1).tolist())
            if shp != (N, KW * 8):
                raise ValueError(f"{base}.weight_shape {shp} does not match weight_packed {tuple(packed.shape)}")
        if tuple(s.shape) != (N, KW * 8 // 128):
            raise ValueError(f"{base}.weight_scale has shape {tuple(s.shape)}: expected [{N}, {KW * 8 // 128}] (group size 128)")
        if s.dtype not in (BF16, torch.float16, torch.float32):
            raise ValueError(f"{base}.weight_scale is {s.dtype}: expected bf16, fp16 or fp32")
        return W4Tensor(packed.contiguous(), s.to(BF16).contiguous())

    def get_mx4(name: str) -> MX4Tensor:
        base = name[:-len(".weight")]
        packed, s = raw(base + MXFP4_PACKED_SUFFIX), raw(base + MXFP4_SCALE_SUFFIX)
        if packed.dtype != torch.uint8:
            raise ValueError(f"{base}{MXFP4_PACKED_SUFFIX} is {packed.dtype}: expected uint8 (two e2m1 codes per byte)")
        N, KB = packed.shape
        if s.dtype != torch.uint8:
            raise ValueError(f"{base}{MXFP4_SCALE_SUFFIX} is {s.dtype}: expected uint8 (e8m0); fp8-typed scales are NVFP4")
        if tuple(s.shape) != (N, KB * 2 // 32):
            raise ValueError(f"{base}{MXFP4_SCALE_SUFFIX} has shape {tuple(s.shape)}: expected [{N}, {KB * 2 // 32}] (group size 32)")
        check_mxfp4_scales(base + MXFP4_SCALE_SUFFIX, s)
        return MX4Tensor(packed.contiguous(), s.contiguous())

    def get_fp8_block(name: str, q: torch.Tensor) -> FP8BTensor:
        sname = name + FP8_BLOCK_SCALE_SUFFIX
        if sname not in index:
            raise ValueError(f"{name} is float8_e4m3fn but the checkpoint has no {sname}")
        s = raw(sname)
        N, K = q.shape
        grid = (-(-N // FP8_BLOCK), -(-K // FP8_BLOCK))
        if s.dtype not in (BF16, torch.float16, torch.float32):
            raise ValueError(f"{sname} is {s.dtype}: expected fp32, bf16 or fp16")
        if tuple(s.shape) != grid:
            raise ValueError(f"{sname} has shape {tuple(s.shape)}: expected {list(grid)} ({FP8_BLOCK} x {FP8_BLOCK} blocks of a "
                             f"[{N}, {K}] matrix)")
        s = s.float()
        if not bool(torch.isfinite(s).all()) or not bool((s > 0).all()):
            raise ValueError(f"{sname} holds a scale that is not finite or not positive")
        return FP8BTensor(q.contiguous(), expand_fp8_block_scales(s, N))

    def get(name: str):
        if name not in index and name.endswith(".weight") and name[:-len(".weight")] + ".weight_packed" in index:
            return get_mx4(name) if kind == "mxfp4" else get_w4(name)
        t = raw(name)
        if t.dtype == FP8:
            if not ckpt_fp8:
                raise ValueError(f"{name} is float8_e4m3fn but config.json declares no compressed-tensors quantization")
            if block:
                return get_fp8_block(name, t)
            s = raw(name + "_scale").float()
            N = t.shape[0]
            if s.numel() == 1:
                s = s.reshape(1).expand(N).contiguous()
            elif tuple(s.shape) in ((N, 1), (N,)):
                s = s.reshape(N).contiguous()
            else:
                raise ValueError(f"{name}_scale has shape {tuple(s.shape)}: expected a scalar or [{N}, 1]")
            return FP8Tensor(t, s)
        if t.dtype.is_floating_point and t.element_size() == 1:
            raise ValueError(f"{name} is {t.dtype}: only OCP float8_e4m3fn weights are supported (not fnuz / e5m2)")
        if not t.dtype.is_floating_point:
            raise ValueError(f"{name} is {t.dtype}: integer-quantized weights are not supported")
        return t.to(BF16)

    for name, shape in param_shapes(cfg):
        if name.endswith(MOE_GATE_UP) or name.endswith(MOE_DOWN):
            w = _moe_experts(name, shape, index, get)
            yield name, (w.to(out_device) if out_device is not None else w)
            continue
        srcs = _packed_sources(name)
        whole = name in index or name[:-len(".weight")] + ".weight_packed" in index
        parts = [get(s) for s in srcs] if srcs is not None and not whole else [get(name)]
        yield name, _assemble(cfg, name, shape, parts, target, rank, tp, out_device)
