"""ctypes table and torch front end of the W4A16 weight entry points (include/ssd_hip_w4a16.h).

Kept apart from ``lib.SIGNATURES`` (exactly ssd_hip.h + ssd_hip_tune.h) and from ``quant_ops.QUANT_SIGNATURES`` (fp8): these bind on
the same libssdhip.so.  As in ops.py, nothing here computes in torch; the calls enqueue on the current stream and are
hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind
from .ops import _p, _stream, _check, EPI_ROWS

c_void_p, c_int = C.c_void_p, C.c_int

# name -> argtypes, exactly include/ssd_hip_w4a16.h
W4_SIGNATURES = {
    "ssd_w4_rows_to_frag": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "ssd_w4_frag_to_rows": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "ssd_w4_dequant_frag": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "ssd_gemm_w4a16": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "ssd_gemm_w4a16_cfg": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
}


def load_w4_library():
    return bind(W4_SIGNATURES)


def w4_rows_to_frag(packed, scale, q_frag, s_frag, N: int, K: int, row_map=None):
    """packed: int32 [N, K/8]; scale: bf16 [N, K/128]; q_frag: N*K/2 bytes; s_frag: bf16 N*K/128; row_map: int32 [N] source row of
    every destination row (None = identity)."""
    _check(load_w4_library().ssd_w4_rows_to_frag(_p(packed), _p(scale), _p(q_frag), _p(s_frag), _p(row_map), N, K, _stream()),
           "ssd_w4_rows_to_frag")


def w4_frag_to_rows(q_frag, s_frag, packed, scale, N: int, K: int):
    _check(load_w4_library().ssd_w4_frag_to_rows(_p(q_frag), _p(s_frag), _p(packed), _p(scale), N, K, _stream()), "ssd_w4_frag_to_rows")


def w4_dequant_frag(q_frag, s_frag, w_frag, N: int, K: int):
    """bf16 frag [N, K] = bf16(s * q) for the bf16 prefill GEMMs."""
    _check(load_w4_library().ssd_w4_dequant_frag(_p(q_frag), _p(s_frag), _p(w_frag), N, K, _stream()), "ssd_w4_dequant_frag")


def gemm_w4a16(x_frag, q_frag, s_frag, y, M: int, N: int, K: int, ldy: int, epilogue: int = EPI_ROWS, bias=None, cfg=None):
    lib = load_w4_library()
    if cfg is None:
        rc = lib.ssd_gemm_w4a16(_p(x_frag), _p(q_frag), _p(s_frag), _p(bias), _p(y), M, N, K, ldy, epilogue, _stream())
    else:
        rc = lib.ssd_gemm_w4a16_cfg(_p(x_frag), _p(q_frag), _p(s_frag), _p(bias), _p(y), M, N, K, ldy, epilogue, cfg[0], cfg[1],
                                    _stream())
    _check(rc, "ssd_gemm_w4a16")
