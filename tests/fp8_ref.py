"""Torch restatement of the FP8 weight format (include/ssd_hip_quant.h) for the tests: the quantizer, the packed row orders and the
fp8 fragment layout, written from their definitions and independent of ssd_amd/quant.py."""
from __future__ import annotations

import torch


def quantize(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """amax[n] = max_k |w[n, k]|; inv = 448 / amax, s = amax / 448 (zero row: s = 1, q = 0); q = e4m3fn(clamp(w * inv))."""
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    zero = amax == 0
    inv = torch.where(zero, torch.ones_like(amax), 448.0 / torch.where(zero, torch.ones_like(amax), amax))
    s = torch.where(zero, torch.ones_like(amax), amax / 448.0)
    q = (wf * inv[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    return q, s


def dequant(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    return (q.float() * s.float()[:, None]).to(torch.bfloat16)


def qkv_order(nh: int, nkv: int, hd: int) -> list[int]:
    """Rotation-paired QKV: every q / k head's 16-row group j = dims 8j..8j+7 then hd/2+8j..hd/2+8j+7; v rows unchanged."""
    out = []
    for head in range(nh + nkv):
        base = head * hd
        for j in range(hd // 16):
            out += [base + 8 * j + i for i in range(8)] + [base + hd // 2 + 8 * j + i for i in range(8)]
    return out + list(range((nh + nkv) * hd, (nh + 2 * nkv) * hd))


def gate_up_order(N: int) -> list[int]:
    """16-row groups alternate gate group i, up group i."""
    out = []
    for g in range(N // 32):
        out += list(range(16 * g, 16 * g + 16)) + list(range(N // 2 + 16 * g, N // 2 + 16 * g + 16))
    return out


def to_frag(q_rows: torch.Tensor) -> torch.Tensor:
    """[N, K] one-byte codes -> fp8 frag bytes: unit (g, p) of 64 lanes x 16 bytes, lane l = row g*16 + (l & 15), bytes 0..7 =
    columns 64p + 8(l >> 4) + 0..7, bytes 8..15 = the same + 32."""
    N, K = q_rows.shape
    b = q_rows.view(torch.uint8).reshape(N // 16, 16, K // 64, 2, 4, 8)       # [g][r][p][half][c][8]
    return b.permute(0, 2, 4, 1, 3, 5).contiguous().reshape(-1)                # [g][p][lane = c*16 + r][half][8]
