"""numpy restatement of the W4A16 weight format (include/ssd_hip_w4a16.h) for the tests: the quantizer, the pack-quantized packing and
the w4 fragment layout, written from their definitions and independent of ssd_amd/quant.py."""
from __future__ import annotations

import numpy as np
import torch

GROUP = 128


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def to_np_f32(w: torch.Tensor) -> np.ndarray:
    return w.detach().float().cpu().numpy()


def quantize(w: torch.Tensor) -> tuple[np.ndarray, np.ndarray]:
    """[N, K] -> (q int8 [N, K], s bf16 bits [N, K/128]): amax over the group, s = bf16(amax / 7) (zero group: s = 1),
    q = clamp(rne(w / s), -8, 7), all in fp32."""
    wf = to_np_f32(w)
    N, K = wf.shape
    g = wf.reshape(N, K // GROUP, GROUP)
    amax = np.abs(g).max(-1)
    s_bits = bf16_bits((amax / np.float32(7.0)).astype(np.float32))
    s_bits = np.where(s_bits == 0, np.uint16(0x3F80), s_bits)
    s = bf16_value(s_bits)
    q = np.clip(np.rint((g / s[..., None]).astype(np.float32)), -8, 7).astype(np.int8).reshape(N, K)
    return q, s_bits


def pack(q: np.ndarray) -> np.ndarray:
    """int codes [N, K] -> int32 [N, K/8]: column 8j+i in bits 4i..4i+3 of word j as q + 8."""
    N, K = q.shape
    u = (q.astype(np.int64) + 8).astype(np.uint32).reshape(N, K // 8, 8)
    w = np.zeros((N, K // 8), dtype=np.uint32)
    for i in range(8):
        w |= u[..., i] << np.uint32(4 * i)
    return w.view(np.int32)


def unpack(packed: np.ndarray) -> np.ndarray:
    p = np.ascontiguousarray(packed).view(np.uint32)
    N, KW = p.shape
    out = np.empty((N, KW, 8), dtype=np.int8)
    for i in range(8):
        out[..., i] = ((p >> np.uint32(4 * i)) & 0xF).astype(np.int8) - 8
    return out.reshape(N, KW * 8)


def dequant(q: np.ndarray, s_bits: np.ndarray) -> np.ndarray:
    """bf16 bits of bf16(s * q) [N, K]."""
    s = np.repeat(bf16_value(s_bits), GROUP, axis=1)
    return bf16_bits((q.astype(np.float32) * s).astype(np.float32))


def to_frag(q: np.ndarray) -> np.ndarray:
    """int codes [N, K] -> w4 frag words uint32 [N/16][K/128][64 lanes][4]: lane l = row (l & 15), word j = columns
    32j + 8(l >> 4) + e, e in nibble order 0, 2, 4, 6, 1, 3, 5, 7."""
    N, K = q.shape
    u = (q.astype(np.int64) + 8).astype(np.uint32).reshape(N // 16, 16, K // GROUP, 4, 4, 8)   # [g][r][c][j][l>>4][e]
    order = [0, 2, 4, 6, 1, 3, 5, 7]
    w = np.zeros(u.shape[:-1], dtype=np.uint32)
    for n, e in enumerate(order):
        w |= u[..., e] << np.uint32(4 * n)
    # [g][r][c][j][hi] -> [g][c][hi][r][j]   (lane = hi * 16 + r)
    return np.ascontiguousarray(w.transpose(0, 2, 4, 1, 3)).reshape(-1)


def scale_frag(s_bits: np.ndarray) -> np.ndarray:
    """bf16 bits [N, K/128] -> [N/16][K/128][16]."""
    N, G = s_bits.shape
    return np.ascontiguousarray(s_bits.reshape(N // 16, 16, G).transpose(0, 2, 1)).reshape(-1)
