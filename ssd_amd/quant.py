"""Weight-only quantization of the decoder linears: FP8 (OCP e4m3fn) with one scale per row, W[N, K] ~= s[n] * q[n, k], and W4A16
(int4 with one scale per row and 128-column group, further down), and MXFP4 (e2m1 codes with one e8m0 scale per row and 32-column
block, at the end).

The one-time load math is torch on the device; the re-tiling into the kernel layout is csrc/gemm_fp8.hip (ssd_fp8_rows_to_frag) and
csrc/gemm_w4a16.hip (ssd_w4_rows_to_frag).  FP8:

    amax[n] = max_k |w[n, k]|                       (fp32)
    inv = 448 / amax,  s = amax / 448               (fp32; an all-zero row gets s = 1, q = 0)
    q = e4m3fn(clamp(fp32(w) * inv, -448, 448))     (round to nearest even, saturating)
"""
from __future__ import annotations

from typing import NamedTuple

import torch

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
LINEAR_SUFFIXES = ("self_attn.qkv_proj.weight", "self_attn.o_proj.weight", "mlp.gate_up_proj.weight", "mlp.down_proj.weight")


def is_quantized_linear(name: str) -> bool:
    """The decoder linears an fp8 target stores quantized (embedding, LM head and norms stay bf16)."""
    return name.startswith("model.layers.") and name.endswith(LINEAR_SUFFIXES)


# Host forms.  A pre-quantized decoder linear travels from a checkpoint (or a host quantizer) to the decoder as one of five
# NamedTuples: FP8Tensor, FP8BTensor, W4Tensor, W4ZTensor, MX4Tensor.  Each answers, here and nowhere else: `native`, the
# `quantization` value of the target that runs it as it is; `phrase`, what refusals call it; shape(), the logical (N, K); and
# dequantize(), the bf16 matrix such a target computes with (what a bf16 target loads instead).  Every field of every type has one
# row per output row, so packing q | k | v or gate | up (cat_rows) and moving (to_device) are generic.
class FP8Tensor(NamedTuple):
    """An FP8 decoder linear with one scale per row on the host: codes float8_e4m3fn [N, K], scale fp32 [N]."""
    codes: torch.Tensor
    scale: torch.Tensor
    native, phrase = "fp8", "per-row fp8"

    def shape(self) -> tuple[int, int]:
        return tuple(self.codes.shape)

    def dequantize(self) -> torch.Tensor:
        return dequantize_fp8(*self)


def quantize_fp8(w: torch.Tensor) -> FP8Tensor:
    """[N, K] bf16 -> FP8Tensor(q [N, K] float8_e4m3fn, s [N] fp32), on w's device."""
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    amax = torch.where(amax == 0, torch.full_like(amax, FP8_MAX), amax)
    inv = FP8_MAX / amax
    s = amax / FP8_MAX
    q = (wf * inv[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return FP8Tensor(q, s)


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


# ---------------------------------------------------------------------------------------------------------------------
# Block-scaled FP8 (include/ssd_hip_fp8b.h): e4m3fn codes with one fp32 scale per block of FP8_BLOCK rows and FP8_BLOCK columns,
# W = s[n // 128, k // 128] * q[n, k]: the form of `quant_method: "fp8"` checkpoints with weight_block_size [128, 128] (their
# weight_scale_inv tensor is s).  Grids are ceil: the last block row / column may be ragged.  The quantizer, fp32 on the tensor's
# device, per block:
#
#     amax = max |w| over the block
#     s = amax / 448,  inv = 448 / amax               (an all-zero block gets s = 1, q = 0)
#     q = e4m3fn(clamp(fp32(w) * inv, -448, 448))     (round to nearest even, saturating)
#
# On the host a linear carries its scales expanded to one ROW of block scales per output row, [N, ceil(K / 128)]: that form
# survives torch.cat of q | k | v and gate | up (whose sources have their own block grids) and any row permutation.  The device
# keeps one scale per 16-row group of the packed order and column block (fp8_block_group_scales).
# ---------------------------------------------------------------------------------------------------------------------
FP8_BLOCK = 128


class FP8BTensor(NamedTuple):
    """A block-scaled FP8 decoder linear on the host: codes float8_e4m3fn [N, K], rowscale fp32 [N, ceil(K / 128)] (row n holds
    the scales of the block row its source tensor put row n in)."""
    codes: torch.Tensor
    rowscale: torch.Tensor
    native, phrase = "fp8", "block-scaled fp8"

    def shape(self) -> tuple[int, int]:
        return tuple(self.codes.shape)

    def dequantize(self) -> torch.Tensor:
        return dequantize_fp8_block(*self)


def expand_fp8_block_scales(s: torch.Tensor, N: int) -> torch.Tensor:
    """Block scales [ceil(N / 128), KB] -> one row of scales per output row, fp32 [N, KB]."""
    assert s.dim() == 2 and s.shape[0] == -(-N // FP8_BLOCK), (tuple(s.shape), N)
    return s.float().repeat_interleave(FP8_BLOCK, dim=0)[:N].contiguous()


def _fp8_block_elem_scales(rowscale: torch.Tensor, K: int) -> torch.Tensor:
    return rowscale.float().repeat_interleave(FP8_BLOCK, dim=1)[:, :K]


def quantize_fp8_block(w: torch.Tensor) -> FP8BTensor:
    """[N, K] bf16 -> FP8BTensor(codes [N, K], rowscale [N, ceil(K / 128)]), on w's device (ragged last blocks allowed)."""
    N, K = w.shape
    NB, KB = -(-N // FP8_BLOCK), -(-K // FP8_BLOCK)
    wf = w.float()
    pad = torch.zeros(NB * FP8_BLOCK, KB * FP8_BLOCK, dtype=torch.float32, device=w.device)
    pad[:N, :K] = wf.abs()
    amax = pad.reshape(NB, FP8_BLOCK, KB, FP8_BLOCK).amax(dim=(1, 3))
    amax = torch.where(amax == 0, torch.full_like(amax, FP8_MAX), amax)
    inv = _fp8_block_elem_scales(expand_fp8_block_scales(FP8_MAX / amax, N), K)
    q = (wf * inv).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return FP8BTensor(q, expand_fp8_block_scales(amax / FP8_MAX, N))


def dequantize_fp8_block(codes: torch.Tensor, rowscale: torch.Tensor) -> torch.Tensor:
    """bf16(s * q), the product in fp32: the weights a block-scaled fp8 target computes with, as a bf16 matrix."""
    return (codes.float() * _fp8_block_elem_scales(rowscale, codes.shape[1])).to(torch.bfloat16)


def fp8_block_group_scales(rowscale: torch.Tensor, row_map: torch.Tensor | None, name: str = "") -> torch.Tensor:
    """rowscale fp32 [N, KB] in source row order -> the device table fp32 [N / 16, KB]: one scale per 16-row group of the PACKED row
    order (row_map names the source row of every packed row; None = in order) and column block.  Raises ValueError if the rows of
    some packed group do not share their scales (the shipped row maps keep every group inside one 128-row block for head_dim 64
    and 128; head_dim 256 would not)."""
    N, KB = rowscale.shape
    assert N % 16 == 0, N
    s = rowscale.float()
    if row_map is not None:
        s = s[row_map.to(s.device).long()]
    g = s.reshape(N // 16, 16, KB)
    mixed = (g != g[:, :1]).any(dim=2).any(dim=1)
    if bool(mixed.any()):
        bad = int(mixed.nonzero()[0])
        raise ValueError(f"{name or 'linear'}: packed rows {16 * bad}..{16 * bad + 15} draw from source rows with different block scales; "
                         "the block-scaled fp8 GEMM needs one scale per 16-row group")
    return g[:, 0].contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# W4A16: signed int4 codes q in [-8, 7] with one bf16 scale per output row and 128-column group, W ~= s[n, k // 128] * q[n, k]
# (csrc/gemm_w4a16.hip).  Round to nearest, fp32 on the tensor's device:
#
#     amax = max |w| over the group
#     s = bf16_rne(amax / 7)                          (an all-zero group gets s = 1, q = 0)
#     q = clamp(rne(w / float(s)), -8, 7)
#
# The host form is compressed-tensors "pack-quantized": codes int32 [N, K / 8], word j = columns 8j .. 8j+7, column 8j+i in bits
# 4i .. 4i+3 as the unsigned nibble q + 8; scales bf16 [N, K / 128].
# ---------------------------------------------------------------------------------------------------------------------
W4_GROUP = 128


class W4Tensor(NamedTuple):
    """A W4A16 decoder linear in the pack-quantized host form: packed int32 [N, K / 8], scale bf16 [N, K / 128]."""
    packed: torch.Tensor
    scale: torch.Tensor
    native, phrase = "w4a16", "int4 (w4a16)"

    def shape(self) -> tuple[int, int]:
        return self.packed.shape[0], self.packed.shape[1] * 8

    def dequantize(self) -> torch.Tensor:
        return dequantize_w4a16(*self)


def pack_w4(q: torch.Tensor) -> torch.Tensor:
    """int codes [N, K] in [-8, 7] -> int32 [N, K / 8] (column 8j+i in bits 4i .. 4i+3 of word j, as q + 8)."""
    N, K = q.shape
    u = (q.to(torch.int64) + 8).reshape(N, K // 8, 8)
    shifts = torch.arange(0, 32, 4, dtype=torch.int64, device=q.device)
    w = (u << shifts).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_w4(packed: torch.Tensor) -> torch.Tensor:
    """int32 [N, K / 8] -> int8 codes [N, K] in [-8, 7]."""
    N, KW = packed.shape
    shifts = torch.arange(0, 32, 4, dtype=torch.int64, device=packed.device)
    u = (packed.to(torch.int64)[..., None] >> shifts) & 0xF
    return (u - 8).to(torch.int8).reshape(N, KW * 8)


def quantize_w4a16(w: torch.Tensor) -> W4Tensor:
    """[N, K] bf16 (K % 128 == 0) -> W4Tensor(packed int32 [N, K / 8], scale bf16 [N, K / 128]), on w's device."""
    N, K = w.shape
    assert K % W4_GROUP == 0, f"W4A16 needs K % {W4_GROUP} == 0, got {K}"
    wf = w.float().reshape(N, K // W4_GROUP, W4_GROUP)
    s = (wf.abs().amax(-1) / 7.0).to(torch.bfloat16)
    s = torch.where(s == 0, torch.ones_like(s), s)
    q = torch.round(wf / s.float()[..., None]).clamp(-8, 7).reshape(N, K)
    return W4Tensor(pack_w4(q), s)


def dequantize_w4a16(packed: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """bf16(s * q): the weights a W4A16 target computes with, as a bf16 matrix (oracles, a bf16 decoder given int4 tensors)."""
    q = unpack_w4(packed).float()
    s = scale.float().repeat_interleave(W4_GROUP, dim=1)
    return (q * s).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------
# W4A16 with zero points (include/ssd_hip_w4zp.h): unsigned codes u in [0, 15], one bf16 scale s and one integer zero point z in
# [0, 15] per output row and 128-column group, W = s[n, k // 128] * (u[n, k] - z[n, k // 128]): the form of AWQ and asymmetric GPTQ
# checkpoints.  The symmetric W4Tensor above is the special case z = 8 (its nibble is u = q + 8), and the packing is pack_w4's with
# the nibble u itself.  The min/max quantizer, round to nearest even, fp32 on the tensor's device, per group:
#
#     lo = min w, hi = max w, range = hi - lo          (an all-equal group, range == 0: range = 15 * |lo|, see below)
#     s = bf16_rne(max(range, W4ZP_TINY) / 15)
#     z = clamp(rne(-lo / s), 0, 15)
#     u = clamp(rne(w / s) + z, 0, 15)
#
# An all-equal group of value c takes the range 15 |c|, so s = |c| exactly (c is bf16) and the group is reproduced exactly:
# c > 0 gives z = 0 (rne(-1) clamped), u = 1; c < 0 gives z = 1, u = 0; c = 0 gives s = W4ZP_TINY / 15, z = 0, u = 0.  (With the
# plain range 0 the scale would be the tiny floor and z, u would both saturate; with range |c| the scale bf16(|c| / 15) is
# inexact and 15 s != c.)  W4ZP_TINY = 15 * 2^-126 keeps s a normal, non-zero bf16 number.
# ---------------------------------------------------------------------------------------------------------------------
W4ZP_TINY = 15.0 * 2.0 ** -126


class W4ZTensor(NamedTuple):
    """A W4A16 decoder linear with zero points in the host row form: packed int32 [N, K / 8] (column 8j+i in bits 4i .. 4i+3 of word
    j, the nibble is u), scale bf16 [N, K / 128], zero uint8 [N, K / 128] in 0..15."""
    packed: torch.Tensor
    scale: torch.Tensor
    zero: torch.Tensor
    native, phrase = "w4a16", "zero-point int4"

    def shape(self) -> tuple[int, int]:
        return self.packed.shape[0], self.packed.shape[1] * 8

    def dequantize(self) -> torch.Tensor:
        return dequantize_w4zp(*self)


def pack_w4u(u: torch.Tensor) -> torch.Tensor:
    """unsigned codes [N, K] in [0, 15] -> int32 [N, K / 8] (pack_w4's layout with the nibble u)."""
    return pack_w4(u.to(torch.int64) - 8)


def unpack_w4u(packed: torch.Tensor) -> torch.Tensor:
    """int32 [N, K / 8] -> uint8 codes [N, K] in [0, 15]."""
    return (unpack_w4(packed).to(torch.int16) + 8).to(torch.uint8)


def quantize_w4a16_zp(w: torch.Tensor) -> W4ZTensor:
    """[N, K] bf16 (K % 128 == 0) -> W4ZTensor, on w's device: the min/max quantizer described above."""
    N, K = w.shape
    assert K % W4_GROUP == 0, f"W4A16 needs K % {W4_GROUP} == 0, got {K}"
    wf = w.float().reshape(N, K // W4_GROUP, W4_GROUP)
    lo, hi = wf.amin(-1), wf.amax(-1)
    rng = hi - lo
    rng = torch.where(rng == 0, 15.0 * lo.abs(), rng)
    s = (rng.clamp_min(W4ZP_TINY) / 15.0).to(torch.bfloat16)
    sf = s.float()
    z = torch.round(-lo / sf).clamp(0, 15)
    u = (torch.round(wf / sf[..., None]) + z[..., None]).clamp(0, 15).reshape(N, K)
    return W4ZTensor(pack_w4u(u), s, z.to(torch.uint8))


def dequantize_w4zp(packed: torch.Tensor, scale: torch.Tensor, zero: torch.Tensor) -> torch.Tensor:
    """bf16(s * (u - z)), the product in fp32: the weights a zero-point W4A16 linear computes with (oracles, a bf16 decoder given
    such tensors)."""
    u = unpack_w4u(packed).float()
    s = scale.float().repeat_interleave(W4_GROUP, dim=1)
    z = zero.float().repeat_interleave(W4_GROUP, dim=1)
    return (s * (u - z)).to(torch.bfloat16)


def w4z_as_symmetric(w: W4ZTensor) -> "W4Tensor | W4ZTensor":
    """A linear whose zero points all equal 8 is the symmetric format bit for bit: hand it on as a W4Tensor (no zero table, the
    symmetric kernel)."""
    return W4Tensor(w.packed, w.scale) if bool((w.zero == 8).all()) else w


# ---------------------------------------------------------------------------------------------------------------------
# MXFP4 (OCP microscaling FP4): e2m1 codes (4 bits s e e m: magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 for codes 0..7, sign in bit 3) with
# one e8m0 scale byte b per output row and block of 32 consecutive columns, W = 2^(b - 127) * e2m1(q) (csrc/gemm_mxfp4.hip).
# Supported scale bytes are 2 <= b <= 252: there 0.5 * 2^(b - 127) is a normal bf16 number and 6 * 2^(b - 127) is finite, so every
# weight is exact in bf16 and the device never has to agree with the host about flushing or overflow.
#
# The host form: codes uint8 [N, K / 2], byte j of a row = column 2j in bits 0..3 and column 2j+1 in bits 4..7; scales uint8
# [N, K / 32].  Widths must be multiples of MX4_GROUP = 128 (one 1 KiB device unit covers 16 rows x 128 columns = four blocks).
# ---------------------------------------------------------------------------------------------------------------------
MX4_BLOCK = 32
MX4_GROUP = 128
MX4_SCALE_MIN, MX4_SCALE_MAX = 2, 252
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)


class MX4Tensor(NamedTuple):
    """An MXFP4 decoder linear in the host form: packed uint8 [N, K / 2], scale uint8 [N, K / 32]."""
    packed: torch.Tensor
    scale: torch.Tensor
    native, phrase = "mxfp4", "MXFP4"

    def shape(self) -> tuple[int, int]:
        return self.packed.shape[0], self.packed.shape[1] * 2

    def dequantize(self) -> torch.Tensor:
        return dequantize_mxfp4(*self)


def check_mxfp4_scales(name: str, scale: torch.Tensor) -> None:
    """Refuses e8m0 scale bytes outside 2..252 (0, 1: weights that are bf16 subnormals; 253, 254: overflow; 255: NaN)."""
    if scale.dtype != torch.uint8:
        raise ValueError(f"{name}: MXFP4 scales are {scale.dtype}, expected uint8 (e8m0)")
    lo, hi = int(scale.min()), int(scale.max())
    if lo < MX4_SCALE_MIN or hi > MX4_SCALE_MAX:
        bad = lo if lo < MX4_SCALE_MIN else hi
        raise ValueError(f"{name}: MXFP4 scale byte {bad} is outside the supported range {MX4_SCALE_MIN}..{MX4_SCALE_MAX} "
                         "(2^(b - 127) with every weight a normal, finite bf16 number; 255 is NaN)")


def pack_mxfp4(codes: torch.Tensor) -> torch.Tensor:
    """e2m1 codes [N, K] in 0..15 -> uint8 [N, K / 2] (column 2j in bits 0..3 of byte j, column 2j+1 in bits 4..7)."""
    c = codes.to(torch.int32)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8)


def unpack_mxfp4(packed: torch.Tensor) -> torch.Tensor:
    """uint8 [N, K / 2] -> e2m1 codes uint8 [N, K] in 0..15."""
    p = packed.to(torch.int32)
    return torch.stack((p & 0xF, p >> 4), dim=-1).reshape(packed.shape[0], -1).to(torch.uint8)


def quantize_mxfp4(w: torch.Tensor) -> MX4Tensor:
    """[N, K] bf16 (K % 128 == 0) -> MX4Tensor(packed uint8 [N, K / 2], scale uint8 [N, K / 32]), on w's device: the OCP MX v1.0
    conversion, in fp32.  Per block of 32 columns

        amax = max |w|
        b = max(floor(log2(amax)) - 2 + 127, 2)         (the floor is the fp32 exponent field; an all-zero block gets b = 127, q = 0;
                                                         finite bf16 inputs never exceed 252)
        q = e2m1(w / 2^(b - 127))                       (round to nearest, ties to the even code, saturating at +-6)

    so amax / 2^(b - 127) lies in [4, 8) unless the clamp at 2 took hold.  The ties and the saturation, on magnitudes: 0.25 -> 0,
    0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4, anything above 6 -> 6.  The sign bit is that of w (a negative value
    that rounds to zero keeps it: code 8 = -0; -0.0 itself gives code 0)."""
    N, K = w.shape
    assert K % MX4_GROUP == 0, f"MXFP4 needs K % {MX4_GROUP} == 0, got {K}"
    wf = w.float().reshape(N, K // MX4_BLOCK, MX4_BLOCK)
    amax = wf.abs().amax(-1)
    e = (amax.view(torch.int32) >> 23) & 0xFF
    b = torch.where(amax == 0, torch.full_like(e, 127), (e - 2).clamp_min(MX4_SCALE_MIN))
    a = (wf / (b << 23).view(torch.float32)[..., None]).abs()
    q = (a > 0.25).to(torch.int32) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0)
    q = q | ((wf < 0).to(torch.int32) << 3)
    return MX4Tensor(pack_mxfp4(q.reshape(N, K)), b.to(torch.uint8))


def dequantize_mxfp4(packed: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """bf16 [N, K] = 2^(b - 127) * e2m1(q), exact for 2 <= b <= 252: the weights an MXFP4 target computes with (oracles, a bf16 decoder
    given MXFP4 tensors)."""
    lut = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=packed.device)
    v = lut[unpack_mxfp4(packed).long()]
    s = (scale.to(torch.int32) << 23).view(torch.float32).repeat_interleave(MX4_BLOCK, dim=1)
    return (v * s).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------
# What the loaders and the decoder ask of a host form without knowing which of the five it is.
# ---------------------------------------------------------------------------------------------------------------------
def is_prequantized(w) -> bool:
    """Whether w is a pre-quantized decoder linear in one of the host forms (anything else is a plain tensor)."""
    return isinstance(w, (FP8Tensor, FP8BTensor, W4Tensor, W4ZTensor, MX4Tensor))


def cat_rows(parts: list):
    """q | k | v or gate | up of ONE host form packed into the form of the whole matrix: every field is concatenated along the rows."""
    assert len({type(p) for p in parts}) == 1 and is_prequantized(parts[0]), [type(p).__name__ for p in parts]
    return type(parts[0])(*(torch.cat(field, dim=0) for field in zip(*parts)))


def to_device(w, device):
    """A host form with every field on `device` (None: where it is)."""
    return w if device is None else type(w)(*(t.to(device) for t in w))


# ---------------------------------------------------------------------------------------------------------------------
# FP8 KV cache (kv_cache_dtype="fp8", include/ssd_hip_kv8.h): e4m3fn codes, one byte per element, one fp32 scale per layer, K or V,
# and kv head.  The definition the kernels are tested against, in torch, on any device.
# ---------------------------------------------------------------------------------------------------------------------
def kv_fp8_encode(x_bf16: torch.Tensor, inv_scale) -> torch.Tensor:
    """uint8 codes of bf16 values [..., hd]: e4m3fn_rne(clamp(fp32(x) * inv_scale, -448, 448)).  inv_scale is an fp32 scalar or a
    tensor that broadcasts against x (per kv head: shape [..., nkv, 1, 1] for the cache layout [..., nkv, block_size, hd]).  The clamp
    comes first: torch's float8_e4m3fn cast rounds to nearest even and keeps -0.0 but does not saturate (500.0 becomes NaN)."""
    assert x_bf16.dtype == torch.bfloat16, x_bf16.dtype
    inv = torch.as_tensor(inv_scale, dtype=torch.float32, device=x_bf16.device)
    y = (x_bf16.float() * inv).clamp(-FP8_MAX, FP8_MAX)
    return y.to(FP8).view(torch.uint8)


def kv_fp8_decode(codes: torch.Tensor, scale) -> torch.Tensor:
    """fp32 values scale * fp32(code) of uint8 codes (the widening is exact; codes 0x7F and 0xFF are NaN)."""
    assert codes.dtype == torch.uint8, codes.dtype
    s = torch.as_tensor(scale, dtype=torch.float32, device=codes.device)
    return s * codes.view(FP8).float()
