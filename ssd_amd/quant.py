"""FP8 (OCP e4m3fn) weight-only quantization of the decoder linears: W[N, K] ~= s[n] * q[n, k].

The one-time load math is torch on the device; the re-tiling into the kernel layout is csrc/gemm_fp8.hip (ssd_fp8_rows_to_frag).

    amax[n] = max_k |w[n, k]|                       (fp32)
    inv = 448 / amax,  s = amax / 448               (fp32; an all-zero row gets s = 1, q = 0)
    q = e4m3fn(clamp(fp32(w) * inv, -448, 448))     (round to nearest even, saturating)
"""
from __future__ import annotations

import torch

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
LINEAR_SUFFIXES = ("self_attn.qkv_proj.weight", "self_attn.o_proj.weight", "mlp.gate_up_proj.weight", "mlp.down_proj.weight")


def is_quantized_linear(name: str) -> bool:
    """The decoder linears an fp8 target stores quantized (embedding, LM head and norms stay bf16)."""
    return name.startswith("model.layers.") and name.endswith(LINEAR_SUFFIXES)


def quantize_fp8(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """[N, K] bf16 -> (q [N, K] float8_e4m3fn, s [N] fp32), on w's device."""
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    amax = torch.where(amax == 0, torch.full_like(amax, FP8_MAX), amax)
    inv = FP8_MAX / amax
    s = amax / FP8_MAX
    q = (wf * inv[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return q, s


def dequantize_fp8(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """bf16(s[n] * q[n, k]): the weights an fp8 target computes with, as a bf16 matrix (oracles, a bf16 decoder given fp8 tensors)."""
    return (q.float() * s.float().reshape(-1, 1)).to(torch.bfloat16)


def gate_up_row_map(N: int) -> torch.Tensor:
    """Source row of every destination row of the gate/up interleave (ssd_rows_to_frag mode 1): 16-row groups alternate gate, up."""
    d = torch.arange(N, dtype=torch.int64)
    g, i = d // 16, d % 16
    return ((g % 2) * (N // 2) + (g // 2) * 16 + i).to(torch.int32)


def qkv_row_map(nh: int, nkv: int, hd: int) -> torch.Tensor:
    """Source row of every destination row of the rotation-paired QKV order (ssd_rows_to_frag_qkv): in every q / k head, 16-row group
    j = dims [8j .. 8j+7] ++ [hd/2 + 8j .. hd/2 + 8j+7]; v rows keep their order."""
    half, gph = hd // 2, hd // 16
    idx = []
    for head in range(nh + nkv):
        for j in range(gph):
            idx.extend(head * hd + 8 * j + i for i in range(8))
            idx.extend(head * hd + half + 8 * j + i for i in range(8))
    idx.extend(range((nh + nkv) * hd, (nh + 2 * nkv) * hd))
    return torch.tensor(idx, dtype=torch.int32)
