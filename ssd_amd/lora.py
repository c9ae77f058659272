"""LoRA adapters: the loader and the packing of an adapter into the slot tables of the target's four linears per layer.

Pure torch: nothing here touches the GPU library (the CPU tests run it).  The device side is include/ssd_hip_lora.h, which also
holds the normative semantics; HipDecoder.set_lora copies what `pack_linear` returns into a slot.

An adapter comes as a PEFT directory (``adapter_config.json`` + ``adapter_model.safetensors``) or as an in-memory dict
``{"r", "lora_alpha", "target_modules", "tensors": {name: tensor}}`` (any other adapter_config.json field may be given as a key too)
with the same tensor names:
    base_model.model.model.layers.{i}.{self_attn|mlp}.{module}.lora_A.weight   [r, in]
    base_model.model.model.layers.{i}.{self_attn|mlp}.{module}.lora_B.weight   [out, r]
The delta of a module is scale * B . A with scale = lora_alpha / r (lora_alpha / sqrt(r) with use_rslora).  A module or layer the
adapter does not carry contributes zero.  `peft` is not a dependency and was not available when this was written: the field and
tensor names follow the published format from memory and have not been checked against a file PEFT wrote.

q | k | v and gate | up are fused linears here.  Their parts' adapters become ONE adapter of the fused linear: the A matrices are
stacked (part p's ranks at rows p * r ..), B is block-structured (part p's output rows carry part p's rank columns, zeros elsewhere),
and B's rows go through the row maps of the base weight (quant.qkv_row_map, quant.gate_up_row_map), because the rows epilogue of those
GEMMs emits its columns in that packed order.  The packed product B . A equals the row-mapped stack of the parts' B . A exactly.
Ranks below the slot's rank are zero-padded, which is exact as well.
"""
from __future__ import annotations

import json
import math
import os
import re
from dataclasses import dataclass, field

import torch

from ssd_amd import quant

MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
# the target's linears and the modules fused into each, in the fused row order
LINEARS = {"qkv": ("q_proj", "k_proj", "v_proj"), "o": ("o_proj",), "gate_up": ("gate_proj", "up_proj"), "down": ("down_proj",)}
RANKS = (16, 32, 64)            # Config.max_lora_rank
MAX_LORAS = 8                   # Config.max_loras
_BLOCK = {m: ("self_attn" if m in ("q_proj", "k_proj", "v_proj", "o_proj") else "mlp") for m in MODULES}
_NAME = re.compile(r"^base_model\.model\.model\.layers\.(\d+)\.(self_attn|mlp)\.(\w+)\.lora_([AB])\.weight$")


def module_shapes(cfg) -> dict:
    """module -> (out, in) of the model's seven adaptable linears."""
    h, hd = cfg.hidden_size, cfg.head_dim
    q, kv, I = cfg.num_heads * hd, cfg.num_kv_heads * hd, cfg.intermediate_size
    return {"q_proj": (q, h), "k_proj": (kv, h), "v_proj": (kv, h), "o_proj": (h, q), "gate_proj": (I, h), "up_proj": (I, h),
            "down_proj": (h, I)}


def slot_rank(linear: str, max_rank: int) -> int:
    """Rank of a slot of `linear`: its parts' ranks side by side, rounded up to the kernels' 32 (at most 3 * 64 = 192)."""
    return -(-len(LINEARS[linear]) * max_rank // 32) * 32


def linear_shape(linear: str, cfg) -> tuple[int, int]:
    """(N, K) of the fused linear."""
    sh = module_shapes(cfg)
    return sum(sh[m][0] for m in LINEARS[linear]), sh[LINEARS[linear][0]][1]


@dataclass
class LoraAdapter:
    r: int
    lora_alpha: float
    scale: float
    target_modules: tuple
    tensors: dict = field(default_factory=dict)       # (layer, module) -> (A [r, in] bf16, B [out, r] bf16)


def check_config(c: dict, max_rank: int) -> tuple[int, float, float, tuple]:
    """Validate the adapter_config.json fields; returns (r, lora_alpha, scale, target_modules).  Everything this engine does not
    implement is refused by name rather than ignored."""
    pt = c.get("peft_type", "LORA")
    if str(pt).upper() != "LORA":
        raise ValueError(f"peft_type must be 'LORA', got {pt!r}")
    if c.get("use_dora"):
        raise ValueError("use_dora=True (DoRA) adapters are not supported")
    if c.get("bias", "none") not in ("none", None):
        raise ValueError(f"bias={c['bias']!r} adapters are not supported: bias must be 'none'")
    if c.get("modules_to_save"):
        raise ValueError(f"modules_to_save={c['modules_to_save']!r} is not supported: only the LoRA matrices are loaded")
    if c.get("rank_pattern"):
        raise ValueError("a non-empty rank_pattern (per-module ranks) is not supported")
    if c.get("alpha_pattern"):
        raise ValueError("a non-empty alpha_pattern (per-module alphas) is not supported")
    if c.get("fan_in_fan_out"):
        raise ValueError("fan_in_fan_out=True adapters are not supported")
    r = c.get("r")
    if isinstance(r, bool) or not isinstance(r, int) or r < 1:
        raise ValueError(f"r must be a positive integer, got {r!r}")
    if r > max_rank:
        raise ValueError(f"r = {r} exceeds max_lora_rank = {max_rank}")
    alpha = c.get("lora_alpha")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha):
        raise ValueError(f"lora_alpha must be a finite number, got {alpha!r}")
    tm = c.get("target_modules")
    if isinstance(tm, str) or not tm:
        raise ValueError(f"target_modules must be a non-empty list of module names, got {tm!r}")
    bad = [m for m in tm if m not in MODULES]
    if bad:
        raise ValueError(f"target_modules holds {bad[0]!r}: only {', '.join(MODULES)} can be adapted (not lm_head, embed_tokens or "
                         "anything else)")
    scale = alpha / math.sqrt(r) if c.get("use_rslora") else alpha / r
    return r, float(alpha), float(scale), tuple(dict.fromkeys(tm))


def load_adapter(source, cfg, max_rank: int, alpha: float | None = None) -> LoraAdapter:
    """source: a PEFT adapter directory or the in-memory dict; cfg: the target's ModelConfig; alpha: overrides lora_alpha."""
    if isinstance(source, (str, os.PathLike)):
        path = os.fspath(source)
        cfile, tfile = os.path.join(path, "adapter_config.json"), os.path.join(path, "adapter_model.safetensors")
        if not os.path.isfile(cfile) or not os.path.isfile(tfile):
            raise ValueError(f"{path!r} is not a PEFT adapter directory: it needs adapter_config.json and adapter_model.safetensors")
        with open(cfile) as f:
            conf = json.load(f)
        from safetensors.torch import load_file
        tensors = load_file(tfile)
    elif isinstance(source, dict):
        conf = {k: v for k, v in source.items() if k != "tensors"}
        tensors = source.get("tensors")
        if not isinstance(tensors, dict) or not tensors:
            raise ValueError("an in-memory adapter needs a non-empty 'tensors' dict")
    else:
        raise ValueError(f"an adapter source is a directory or a dict, got {type(source).__name__}")
    if alpha is not None:
        conf = dict(conf, lora_alpha=alpha)
    r, a, scale, tm = check_config(conf, max_rank)
    shapes = module_shapes(cfg)
    got: dict = {}
    for name, t in tensors.items():
        m = _NAME.match(name)
        if m is None:
            raise ValueError(f"{name}: not a LoRA tensor of a decoder linear (base_model.model.model.layers.<i>.<block>.<module>."
                             "lora_A|lora_B.weight)")
        li, blk, mod, ab = int(m.group(1)), m.group(2), m.group(3), m.group(4)
        if mod not in MODULES or _BLOCK[mod] != blk:
            raise ValueError(f"{name}: {blk}.{mod} is not one of the adaptable modules ({', '.join(MODULES)})")
        if mod not in tm:
            raise ValueError(f"{name}: {mod} is not in target_modules {list(tm)}")
        if li >= cfg.num_layers:
            raise ValueError(f"{name}: the model has {cfg.num_layers} layers")
        out, K = shapes[mod]
        want = (r, K) if ab == "A" else (out, r)
        if tuple(t.shape) != want:
            raise ValueError(f"{name}: shape {tuple(t.shape)} does not match the model and r = {r}: expected {want}")
        if not torch.is_floating_point(t):
            raise ValueError(f"{name}: dtype {t.dtype} is not a floating-point type")
        got.setdefault((li, mod), {})[ab] = t.detach().to(torch.bfloat16).cpu()
    out_t = {}
    for key, ab in got.items():
        if set(ab) != {"A", "B"}:
            raise ValueError(f"layer {key[0]} {key[1]}: lora_{'B' if 'A' in ab else 'A'}.weight is missing")
        out_t[key] = (ab["A"], ab["B"])
    return LoraAdapter(r, a, scale, tm, out_t)


def pack_linear(adapter: LoraAdapter, layer: int, linear: str, cfg, R: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(A [R, K], B [N, R]) bf16 of the fused linear `linear` of `layer` in the PACKED row order of its base weight: what one slot of
    that linear's tables holds (before the fragment-major re-tiling)."""
    shapes = module_shapes(cfg)
    parts = LINEARS[linear]
    N, K = linear_shape(linear, cfg)
    r = adapter.r
    assert len(parts) * r <= R, (linear, r, R)
    A = torch.zeros(R, K, dtype=torch.bfloat16)
    B = torch.zeros(N, R, dtype=torch.bfloat16)
    n0 = 0
    for p, mod in enumerate(parts):
        out = shapes[mod][0]
        ab = adapter.tensors.get((layer, mod))
        if ab is not None:
            A[p * r:(p + 1) * r] = ab[0]
            B[n0:n0 + out, p * r:(p + 1) * r] = ab[1]
        n0 += out
    if linear == "qkv":
        B = B[quant.qkv_row_map(cfg.num_heads, cfg.num_kv_heads, cfg.head_dim).long()]
    elif linear == "gate_up":
        B = B[quant.gate_up_row_map(N).long()]
    return A.contiguous(), B.contiguous()


class LoraRegistry:
    """The fixed slots of one engine: name -> (slot, identity).  No paging, no LRU: add refuses by name when no slot is free.  The
    identity is a 64-bit number unique per add() call (never -1, the base's), which the target's block hashes start from."""

    def __init__(self, max_loras: int):
        self.max_loras = max_loras
        self.by_name: dict[str, tuple[int, int]] = {}
        self._adds = 0

    def free_slot(self, name: str) -> int:
        if not isinstance(name, str) or not name:
            raise ValueError(f"an adapter name is a non-empty string, got {name!r}")
        if name in self.by_name:
            raise ValueError(f"lora {name!r} is already registered: remove_lora it first")
        used = {s for s, _ in self.by_name.values()}
        free = [s for s in range(self.max_loras) if s not in used]
        if not free:
            raise ValueError(f"lora {name!r} cannot be added: all {self.max_loras} slots (max_loras) are taken by "
                             f"{', '.join(sorted(self.by_name))}")
        return free[0]

    def add(self, name: str, slot: int) -> int:
        import xxhash
        self._adds += 1
        ident = xxhash.xxh64(f"lora:{self._adds}:{name}".encode()).intdigest() | 1 << 63     # (never the base's -1: a positive 64-bit word)
        self.by_name[name] = (slot, ident)
        return ident

    def remove(self, name: str) -> int:
        if name not in self.by_name:
            raise ValueError(f"lora {name!r} is not registered (registered: {', '.join(sorted(self.by_name)) or 'none'})")
        return self.by_name.pop(name)[0]

    def resolve(self, name: str) -> tuple[int, int]:
        if name not in self.by_name:
            raise ValueError(f"lora={name!r} is not a registered adapter (registered: {', '.join(sorted(self.by_name)) or 'none'})")
        return self.by_name[name]

    def names(self) -> list[str]:
        return sorted(self.by_name, key=lambda n: self.by_name[n][0])
