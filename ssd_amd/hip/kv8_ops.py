"""ctypes table and torch front end of the FP8 KV cache entry points (include/ssd_hip_kv8.h).

Kept apart from ``lib.SIGNATURES`` and the weight-format tables (``quant_ops``, ``w4_ops``, ``w4zp_ops``, ``mx4_ops``): these bind on
the same libssdhip.so.  As in ops.py, nothing here computes in torch; the calls enqueue on the current stream and are
hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind
from .ops import _p, _stream, _check, MODE_CAUSAL

c_void_p, c_int, c_float = C.c_void_p, C.c_int, C.c_float

# name -> argtypes, exactly include/ssd_hip_kv8.h
KV8_SIGNATURES = {
    "ssd_rope_store_kv_fp8": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_float, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "ssd_attn_paged_fp8": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                           c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int,
                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ssd_attn_prefill_varlen_fp8": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                                    c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p],
    "ssd_kv_fp8_dequant": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
}


def load_kv8_library():
    return bind(KV8_SIGNATURES)


def rope_store_kv_fp8(qkv_rows, positions, cos_sin, slot_mapping, q_out, k_cache, v_cache, T, nh, nkv, hd, block_size,
                      k_inv_scale=None, v_inv_scale=None, q_norm_w=None, k_norm_w=None, eps: float = 0.0, qkv_perm: int = 0):
    """ops.rope_store_kv with uint8 caches; k_inv_scale / v_inv_scale: fp32 [nkv] (None = 1.0)."""
    _check(load_kv8_library().ssd_rope_store_kv_fp8(_p(qkv_rows), _p(positions), _p(cos_sin), _p(slot_mapping), _p(q_out), _p(k_cache),
                                                    _p(v_cache), _p(k_inv_scale), _p(v_inv_scale), _p(q_norm_w), _p(k_norm_w), eps, T, nh,
                                                    nkv, hd, block_size, qkv_perm, _stream()), "ssd_rope_store_kv_fp8")


def attn_paged_fp8(q_rows, k_cache, v_cache, block_tables, max_blocks, context_lens, B, T, max_q, nh, nkv, hd, block_size, scale,
                   k_scale=None, v_scale=None, cu_q=None, q_per_seq=0, mode=MODE_CAUSAL, splits=1, flags=0, ws_o=None, ws_ml=None,
                   out_rows=None, out_frag=None, waves=1):
    """ops.attn_paged over uint8 caches (causal mode only); k_scale / v_scale: fp32 [nkv] (None = 1.0)."""
    flags = (flags & 0xff) | ((waves & 0xf) << 8)
    _check(load_kv8_library().ssd_attn_paged_fp8(_p(q_rows), _p(k_cache), _p(v_cache), _p(k_scale), _p(v_scale), _p(block_tables),
                                                 max_blocks, _p(context_lens), _p(cu_q), q_per_seq, B, T, max_q, nh, nkv, hd, block_size,
                                                 scale, mode, 0, 0, 0, 1, 0, splits, flags, _p(ws_o), _p(ws_ml), _p(out_rows),
                                                 _p(out_frag), _stream()), "ssd_attn_paged_fp8")


def attn_prefill_varlen_fp8(q_rows, k_cache, v_cache, block_tables, max_blocks, context_lens, cu_q, B, T, max_q, nh, nkv, hd, block_size,
                            scale, k_scale=None, v_scale=None, out_rows=None, out_frag=None):
    _check(load_kv8_library().ssd_attn_prefill_varlen_fp8(_p(q_rows), _p(k_cache), _p(v_cache), _p(k_scale), _p(v_scale),
                                                          _p(block_tables), max_blocks, _p(context_lens), _p(cu_q), B, T, max_q, nh, nkv,
                                                          hd, block_size, scale, _p(out_rows), _p(out_frag), _stream()),
           "ssd_attn_prefill_varlen_fp8")


def kv_fp8_dequant(cache8, scale, cache_bf16, pages: int, nkv: int, block_size: int, hd: int):
    """cache_bf16 [pages, nkv, block_size, hd] = bf16(scale[h] * code); scale: fp32 [nkv] (None = 1.0)."""
    _check(load_kv8_library().ssd_kv_fp8_dequant(_p(cache8), _p(scale), _p(cache_bf16), pages, nkv, block_size, hd, _stream()),
           "ssd_kv_fp8_dequant")
