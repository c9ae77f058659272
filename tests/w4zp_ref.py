"""numpy restatement of the zero-point W4A16 format (include/ssd_hip_w4zp.h) for the tests: W = s * (u - z) with unsigned nibbles u,
one bf16 scale s and one zero point z in 0..15 per row and 128-column group; the min/max quantizer, the row-form packing, the device
tables, and the AutoAWQ (gemm) and GPTQ checkpoint packers.  Written from the format text, independent of ssd_amd/quant.py and
ssd_amd/weights.py."""
from __future__ import annotations

import numpy as np
import torch

GROUP = 128
TINY = np.float32(15.0 * 2.0 ** -126)
AWQ_ORDER = [0, 2, 4, 6, 1, 3, 5, 7]        # nibble position i of a word holds column 8j + AWQ_ORDER[i]


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def quantize(w: torch.Tensor) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """[N, K] -> (u uint8 [N, K], s bf16 bits [N, K/128], z uint8 [N, K/128]), all in fp32: range = max - min over the group (an
    all-equal group of value c: 15 |c|), s = bf16(max(range, TINY) / 15), z = clamp(rne(-min / s), 0, 15),
    u = clamp(rne(w / s) + z, 0, 15)."""
    wf = w.detach().float().cpu().numpy()
    N, K = wf.shape
    g = wf.reshape(N, K // GROUP, GROUP)
    lo, hi = g.min(-1), g.max(-1)
    rng = (hi - lo).astype(np.float32)
    rng = np.where(rng == 0, (np.float32(15.0) * np.abs(lo)).astype(np.float32), rng)
    s_bits = bf16_bits((np.maximum(rng, TINY) / np.float32(15.0)).astype(np.float32))
    s = bf16_value(s_bits)
    z = np.clip(np.rint((-lo / s).astype(np.float32)), 0, 15)
    u = np.clip(np.rint((g / s[..., None]).astype(np.float32)) + z[..., None], 0, 15)
    return u.astype(np.uint8).reshape(N, K), s_bits, z.astype(np.uint8)


def pack(u: np.ndarray) -> np.ndarray:
    """unsigned codes [N, K] -> int32 [N, K/8]: column 8j+i in bits 4i..4i+3 of word j."""
    N, K = u.shape
    v = u.astype(np.uint32).reshape(N, K // 8, 8)
    w = np.zeros((N, K // 8), dtype=np.uint32)
    for i in range(8):
        w |= v[..., i] << np.uint32(4 * i)
    return w.view(np.int32)


def unpack(packed: np.ndarray) -> np.ndarray:
    p = np.ascontiguousarray(packed).view(np.uint32)
    N, KW = p.shape
    out = np.empty((N, KW, 8), dtype=np.uint8)
    for i in range(8):
        out[..., i] = ((p >> np.uint32(4 * i)) & 0xF).astype(np.uint8)
    return out.reshape(N, KW * 8)


def weights_f64(u: np.ndarray, s_bits: np.ndarray, z: np.ndarray) -> np.ndarray:
    """The exact weights s * (u - z) as float64 [N, K]."""
    s = np.repeat(bf16_value(s_bits).astype(np.float64), GROUP, axis=1)
    return s * (u.astype(np.float64) - np.repeat(z.astype(np.float64), GROUP, axis=1))


def dequant(u: np.ndarray, s_bits: np.ndarray, z: np.ndarray) -> np.ndarray:
    """bf16 bits of bf16(s * (u - z)) [N, K], the product in fp32 (u - z is an exact small integer)."""
    s = np.repeat(bf16_value(s_bits), GROUP, axis=1)
    d = u.astype(np.float32) - np.repeat(z.astype(np.float32), GROUP, axis=1)
    return bf16_bits((s * d).astype(np.float32))


def zero_frag(z: np.ndarray) -> np.ndarray:
    """uint8 [N, K/128] -> the device table uint8 [N/16][K/128][16], entry (g, c, r) = z[16g + r][c]."""
    N, G = z.shape
    return np.ascontiguousarray(z.reshape(N // 16, 16, G).transpose(0, 2, 1)).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# Checkpoint packers.  Both formats store a linear W[N, K] (N outputs, K inputs) "input-major".
# ---------------------------------------------------------------------------------------------------------------------
def _pack_cols(v: np.ndarray, order) -> np.ndarray:
    """[R, C] values in 0..15 -> int32 [R, C/8]: nibble position i of word j = column 8j + order[i]."""
    R, C = v.shape
    x = v.astype(np.uint32).reshape(R, C // 8, 8)
    w = np.zeros((R, C // 8), dtype=np.uint32)
    for i in range(8):
        w |= x[..., order[i]] << np.uint32(4 * i)
    return w.view(np.int32)


def awq_pack(u: np.ndarray, s_f16: np.ndarray, z: np.ndarray) -> dict[str, np.ndarray]:
    """AutoAWQ gemm: qweight int32 [K, N/8], qzeros int32 [K/128, N/8] (both along the OUTPUT axis, nibble order AWQ_ORDER),
    scales fp16 [K/128, N]."""
    return {"qweight": _pack_cols(u.T, AWQ_ORDER), "qzeros": _pack_cols(z.T, AWQ_ORDER),
            "scales": np.ascontiguousarray(s_f16.T).astype(np.float16)}


def gptq_pack(u: np.ndarray, s_f16: np.ndarray, z: np.ndarray, v1: bool, g_idx: np.ndarray | None = None) -> dict[str, np.ndarray]:
    """GPTQ: qweight int32 [K/8, N] (word [j, n] = input columns 8j+i of output n, sequential), qzeros int32 [K/128, N/8] (output
    8j+i, sequential; format gptq stores z - 1, gptq_v2 stores z), scales fp16 [K/128, N], g_idx int32 [K] = k // 128."""
    N, K = u.shape
    x = u.T.astype(np.uint32).reshape(K // 8, 8, N)
    qw = np.zeros((K // 8, N), dtype=np.uint32)
    for i in range(8):
        qw |= x[:, i, :] << np.uint32(4 * i)
    stored = ((z.astype(np.int64) - (1 if v1 else 0)) & 15).astype(np.uint8)
    return {"qweight": qw.view(np.int32), "qzeros": _pack_cols(stored.T, list(range(8))),
            "scales": np.ascontiguousarray(s_f16.T).astype(np.float16),
            "g_idx": (np.arange(K) // GROUP).astype(np.int32) if g_idx is None else g_idx.astype(np.int32)}
