"""float64 reference of the LoRA semantics of include/ssd_hip_lora.h, shared by tests/test_lora_cpu.py, tests/test_hip_lora.py and
tests/test_engine_lora_gpu.py.

For a linear with base output y0 = bf16(x . W^T) and the row's adapter A [r, K], B [N, r], scale:
    t = bf16(x . A^T)                               (fp32 accumulation, one rounding)
    y = bf16(float(y0) + scale * sum_j t[j] B[n][j])  (fp32 sum, one rounding)
Everything here is computed in float64 from the bf16 inputs, so it is the exact value the kernels' roundings are measured against.
"""
import math

import torch

F64 = torch.float64
MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def sane_slots(row_slot: torch.Tensor, slots: int) -> torch.Tensor:
    """A value outside [-1, slots) is treated as -1."""
    rs = row_slot.long()
    return torch.where((rs >= 0) & (rs < slots), rs, torch.full_like(rs, -1))


def shrink_exact(x: torch.Tensor, A: torch.Tensor, row_slot: torch.Tensor):
    """x [M, K], A [slots, R, K] -> (t [M, R] float64 = x . A[slot]^T, mag [M, R] = sum_k |x a|); rows without a slot are 0."""
    rs = sane_slots(row_slot, A.shape[0])
    Ar = A.to(F64)[rs.clamp(min=0)]                       # [M, R, K]
    xd = x.to(F64)
    t = torch.einsum("mk,mrk->mr", xd, Ar)
    mag = torch.einsum("mk,mrk->mr", xd.abs(), Ar.abs())
    on = (rs >= 0).to(F64)[:, None]
    return t * on, mag * on


def expand_exact(y0: torch.Tensor, t: torch.Tensor, B: torch.Tensor, scale: torch.Tensor, row_slot: torch.Tensor):
    """y0 [M, N], t [M, R] (the rounded t the kernel used), B [slots, N, R], scale [slots] -> (y float64 before its rounding, mag)."""
    rs = sane_slots(row_slot, B.shape[0])
    Br = B.to(F64)[rs.clamp(min=0)]                       # [M, N, R]
    sc = scale.to(F64)[rs.clamp(min=0)][:, None]
    td = t.to(F64)
    d = torch.einsum("mr,mnr->mn", td, Br) * sc
    mag = torch.einsum("mr,mnr->mn", td.abs(), Br.abs()) * sc.abs()
    on = (rs >= 0).to(F64)[:, None]
    return y0.to(F64) + d * on, y0.to(F64).abs() + mag * on


def bf16_ulp(v: torch.Tensor) -> torch.Tensor:
    """The spacing of bf16 values at |v| (float64; 8 significand bits, normal range)."""
    a = v.to(F64).abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def assert_within_bar(got: torch.Tensor, want: torch.Tensor, mag: torch.Tensor, what: str = "") -> None:
    """|got - want| <= 1 bf16 ulp of want, differences below 2^-20 * mag exempt: a correctly rounded value is within half an ulp
    of the value the kernel rounded, and that value is within K * 2^-24 * mag <= 2^-20 * mag (fp32 accumulation over K <= 2080
    terms, any order) of the float64 one, which can move the rounding by one step."""
    err = (got.to(F64) - want).abs()
    bar = torch.maximum(bf16_ulp(want), mag * 2.0 ** -20)
    bad = err > bar
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} outside the bar, worst {float((err / bar).max()):.3f} bars"


def scale_of(r: int, alpha: float, rslora: bool = False) -> float:
    return alpha / math.sqrt(r) if rslora else alpha / r


def make_adapter(shapes: dict, layers: int, r: int, alpha: float, seed: int, modules=MODULES, zero_b: bool = False) -> dict:
    """The in-memory adapter dict of the engine tests.  shapes: module -> (out, in).  A ~ N(0, 1/K), B ~ N(0, 0.02^2), drawn from one
    torch.Generator in layer order, then module order (MODULES), A before B, rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    tensors = {}
    for li in range(layers):
        for m in modules:
            out, K = shapes[m]
            blk = "self_attn" if m in ("q_proj", "k_proj", "v_proj", "o_proj") else "mlp"
            base = f"base_model.model.model.layers.{li}.{blk}.{m}"
            A = (torch.randn(r, K, generator=g) / math.sqrt(K)).to(torch.bfloat16)
            B = (torch.randn(out, r, generator=g) * 0.02).to(torch.bfloat16)
            tensors[base + ".lora_A.weight"] = A
            tensors[base + ".lora_B.weight"] = torch.zeros_like(B) if zero_b else B
    return dict(r=r, lora_alpha=alpha, target_modules=list(modules), tensors=tensors)


def merge_state_dict(w: dict, adapter: dict, layers: int, rslora: bool = False) -> tuple[dict, dict]:
    """The fused state dict `w` (qkv_proj = [q | k | v] rows, gate_up_proj = [gate | up] rows, source row order) with the adapter dict
    merged into it: (bf16 weights for the oracle, float64 W + scale * B . A for the truth).  Tensors that are no decoder linear pass
    through.  Parsed here from the tensor names, independently of ssd_amd/lora.py."""
    scale = scale_of(adapter["r"], adapter["lora_alpha"], rslora)
    t = adapter["tensors"]
    fused = {"self_attn.qkv_proj": ("q_proj", "k_proj", "v_proj"), "self_attn.o_proj": ("o_proj",),
             "mlp.gate_up_proj": ("gate_proj", "up_proj"), "mlp.down_proj": ("down_proj",)}
    bf, f64 = dict(w), dict(w)
    for li in range(layers):
        for lin, parts in fused.items():
            name = f"model.layers.{li}.{lin}.weight"
            W, n0 = w[name].to(F64, copy=True), 0           # (merged in place: the 70B cut's matrices are 0.5 G elements)
            blk = lin.split(".")[0]
            for m in parts:
                a = t.get(f"base_model.model.model.layers.{li}.{blk}.{m}.lora_A.weight")
                b = t.get(f"base_model.model.model.layers.{li}.{blk}.{m}.lora_B.weight")
                if a is None or b is None:
                    raise KeyError(f"merge_state_dict needs every module of {name} (missing {m})")
                W[n0:n0 + b.shape[0]].addmm_(b.to(F64), a.to(F64), alpha=scale)
                n0 += b.shape[0]
            assert n0 == W.shape[0], (name, n0, W.shape)
            f64[name] = W
            bf[name] = W.to(torch.bfloat16)
    return bf, f64
