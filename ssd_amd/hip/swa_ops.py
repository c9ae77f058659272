"""ctypes table and torch front end of the sliding-window attention entry points (include/ssd_hip_swa.h).

Kept apart from ``lib.SIGNATURES`` and ``kv8_ops.KV8_SIGNATURES``: these bind on the same libssdhip.so.  The wrappers take the
keywords of ``ops.attn_paged`` / ``kv8_ops.attn_paged_fp8`` plus ``window``, enqueue on the current stream and are
hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind
from .ops import _p, _stream, _check, MODE_CAUSAL

c_void_p, c_int, c_float = C.c_void_p, C.c_int, C.c_float

# name -> argtypes, exactly include/ssd_hip_swa.h
SWA_SIGNATURES = {
    "ssd_attn_paged_window": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                              c_int, c_int, c_float, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_int, c_void_p],
    "ssd_attn_paged_fp8_window": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                                  c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                  c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
}


def load_swa_library():
    return bind(SWA_SIGNATURES)


def attn_paged_window(q_rows, k_cache, v_cache, block_tables, max_blocks, context_lens, B, T, max_q, nh, nkv, hd, block_size, scale,
                      cu_q=None, q_per_seq=0, mode=MODE_CAUSAL, tree_K=0, tree_mq=0, tree_step=0, tree_F=1, tree_jidx=None, splits=1,
                      flags=0, ws_o=None, ws_ml=None, out_rows=None, out_frag=None, waves=1, window=0):
    """ops.attn_paged where a row with causal limit lim sees the keys [max(0, lim - window), lim); window 0 = ops.attn_paged."""
    flags = (flags & 0xff) | ((waves & 0xf) << 8)
    _check(load_swa_library().ssd_attn_paged_window(_p(q_rows), _p(k_cache), _p(v_cache), _p(block_tables), max_blocks, _p(context_lens),
                                                    _p(cu_q), q_per_seq, B, T, max_q, nh, nkv, hd, block_size, scale, mode, tree_K,
                                                    tree_mq, tree_step, tree_F, _p(tree_jidx), splits, flags, _p(ws_o), _p(ws_ml),
                                                    _p(out_rows), _p(out_frag), window, _stream()), "ssd_attn_paged_window")


def attn_paged_fp8_window(q_rows, k_cache, v_cache, block_tables, max_blocks, context_lens, B, T, max_q, nh, nkv, hd, block_size, scale,
                          k_scale=None, v_scale=None, cu_q=None, q_per_seq=0, mode=MODE_CAUSAL, splits=1, flags=0, ws_o=None,
                          ws_ml=None, out_rows=None, out_frag=None, waves=1, window=0):
    """kv8_ops.attn_paged_fp8 under the same window."""
    flags = (flags & 0xff) | ((waves & 0xf) << 8)
    _check(load_swa_library().ssd_attn_paged_fp8_window(_p(q_rows), _p(k_cache), _p(v_cache), _p(k_scale), _p(v_scale), _p(block_tables),
                                                        max_blocks, _p(context_lens), _p(cu_q), q_per_seq, B, T, max_q, nh, nkv, hd,
                                                        block_size, scale, mode, 0, 0, 0, 1, 0, splits, flags, _p(ws_o), _p(ws_ml),
                                                        _p(out_rows), _p(out_frag), window, _stream()), "ssd_attn_paged_fp8_window")
