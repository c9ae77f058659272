"""numpy restatement of the MXFP4 weight format (include/ssd_hip_mxfp4.h) for the tests: the quantizer, the byte packing, the exact
dequantization and the mx4 fragment layout, written from their definitions and independent of ssd_amd/quant.py."""
from __future__ import annotations

import numpy as np
import torch

BLOCK = 32
MAGS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float64)     # e2m1 magnitudes of codes 0..7; sign in bit 3


def to_np_f32(w: torch.Tensor) -> np.ndarray:
    return w.detach().float().cpu().numpy()


def e2m1_round(a: np.ndarray) -> np.ndarray:
    """Magnitudes (float64, >= 0) -> the nearest e2m1 magnitude code 0..7; a tie goes to the even code; above 6 saturates at 7."""
    d = np.abs(a[..., None] - MAGS)                       # distance to every representable magnitude
    best = d.min(-1, keepdims=True)
    cand = d == best                                      # one candidate, or two at a tie
    codes = np.arange(8)
    even_first = np.where(cand & (codes % 2 == 0), codes, 99).min(-1)
    any_first = np.where(cand, codes, 99).min(-1)
    return np.where(even_first < 99, even_first, any_first).astype(np.uint8)


def quantize(w: torch.Tensor) -> tuple[np.ndarray, np.ndarray]:
    """[N, K] -> (codes uint8 [N, K] in 0..15, scale bytes uint8 [N, K/32]).  Per block: b = max(floor(log2(amax)) + 125, 2) (127 for
    an all-zero block), codes = sign | e2m1_round(|w| / 2^(b - 127)).  float64 throughout: every step is exact there."""
    wf = to_np_f32(w).astype(np.float64)
    N, K = wf.shape
    g = wf.reshape(N, K // BLOCK, BLOCK)
    amax = np.abs(g).max(-1)
    with np.errstate(divide="ignore"):
        # floor(log2) of an fp32 value as its exponent field reads it: subnormals of fp32 (never reached from bf16 normals) count as -127
        _, ex = np.frexp(amax)                            # amax = m * 2^ex, m in [0.5, 1)
    fl = np.maximum(ex - 1, -127)
    b = np.where(amax == 0, 127, np.maximum(fl - 2 + 127, 2)).astype(np.int64)
    scaled = np.abs(g) / np.exp2((b - 127).astype(np.float64))[..., None]
    codes = e2m1_round(scaled) | ((g < 0).astype(np.uint8) << 3)
    return codes.reshape(N, K), b.astype(np.uint8)


def pack(codes: np.ndarray) -> np.ndarray:
    """codes [N, K] -> uint8 [N, K/2]: column 2j in bits 0..3 of byte j, column 2j+1 in bits 4..7."""
    c = codes.astype(np.uint8)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def unpack(packed: np.ndarray) -> np.ndarray:
    N, KB = packed.shape
    out = np.empty((N, KB, 2), dtype=np.uint8)
    out[..., 0] = packed & 0xF
    out[..., 1] = packed >> 4
    return out.reshape(N, KB * 2)


def exact(codes: np.ndarray, b: np.ndarray) -> np.ndarray:
    """float64 [N, K] = (-1)^s * magnitude * 2^(b - 127)."""
    v = MAGS[codes & 7] * np.where(codes & 8, -1.0, 1.0)
    return v * np.repeat(np.exp2(b.astype(np.float64) - 127.0), BLOCK, axis=1)


def bf16_bits_exact(x64: np.ndarray) -> np.ndarray:
    """bf16 bits of values that ARE bf16 numbers (asserted): the top 16 bits of the fp32."""
    f = x64.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), x64)
    u = f.view(np.uint32)
    assert not (u & 0xFFFF).any(), "value is not exact in bf16"
    return (u >> 16).astype(np.uint16)


def to_frag(packed: np.ndarray) -> np.ndarray:
    """packed uint8 [N, K/2] -> mx4 frag words uint32 [N/16][K/128][64 lanes][4]: lane l = row (l & 15), word j = the row-form word of
    columns 128c + 32j + 8(l >> 4) .. +7."""
    N, KB = packed.shape
    w = np.ascontiguousarray(packed).view(np.uint32).reshape(N // 16, 16, KB // 64, 4, 4)     # [g][r][c][j][hi]
    return np.ascontiguousarray(w.transpose(0, 2, 4, 1, 3)).reshape(-1)                        # [g][c][hi][r][j]


def scale_frag(b: np.ndarray) -> np.ndarray:
    """scale bytes [N, K/32] -> uint8 [N/16][K/128][16][4]."""
    N, G = b.shape
    return np.ascontiguousarray(b.reshape(N // 16, 16, G // 4, 4).transpose(0, 2, 1, 3)).reshape(-1)
