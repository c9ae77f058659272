"""ctypes table and torch front end of the W8A16 weight entry points (include/ssd_hip_w8a16.h).

Kept apart from ``lib.SIGNATURES`` (exactly ssd_hip.h + ssd_hip_tune.h) and from the other weight-format tables (``quant_ops``,
``w4_ops``, ``w4zp_ops``, ``mx4_ops``): these bind on the same libssdhip.so.  As in ops.py, nothing here computes in torch; the calls
enqueue on the current stream and are hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind
from .ops import _p, _stream, _check, EPI_ROWS

c_void_p, c_int = C.c_void_p, C.c_int

# name -> argtypes, exactly include/ssd_hip_w8a16.h
W8_SIGNATURES = {
    "ssd_w8_rows_to_frag": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "ssd_w8_frag_to_rows": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "ssd_w8_dequant_frag": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "ssd_gemm_w8a16": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "ssd_gemm_w8a16_cfg": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
}


def load_w8_library():
    return bind(W8_SIGNATURES)


def w8_rows_to_frag(codes, scale, q_frag, s_frag, N: int, K: int, row_map=None):
    """codes: uint8 [N, K] (u = q + 128); scale: bf16 [N, K/128]; q_frag: N*K bytes; s_frag: bf16 N*K/128; row_map: int32 [N] source
    row of every destination row (None = identity)."""
    _check(load_w8_library().ssd_w8_rows_to_frag(_p(codes), _p(scale), _p(q_frag), _p(s_frag), _p(row_map), N, K, _stream()),
           "ssd_w8_rows_to_frag")


def w8_frag_to_rows(q_frag, s_frag, codes, scale, N: int, K: int):
    _check(load_w8_library().ssd_w8_frag_to_rows(_p(q_frag), _p(s_frag), _p(codes), _p(scale), N, K, _stream()), "ssd_w8_frag_to_rows")


def w8_dequant_frag(q_frag, s_frag, w_frag, N: int, K: int):
    """bf16 frag [N, K] = bf16(s * q) for the bf16 prefill GEMMs."""
    _check(load_w8_library().ssd_w8_dequant_frag(_p(q_frag), _p(s_frag), _p(w_frag), N, K, _stream()), "ssd_w8_dequant_frag")


def gemm_w8a16(x_frag, q_frag, s_frag, y, M: int, N: int, K: int, ldy: int, epilogue: int = EPI_ROWS, bias=None, cfg=None):
    lib = load_w8_library()
    if cfg is None:
        rc = lib.ssd_gemm_w8a16(_p(x_frag), _p(q_frag), _p(s_frag), _p(bias), _p(y), M, N, K, ldy, epilogue, _stream())
    else:
        rc = lib.ssd_gemm_w8a16_cfg(_p(x_frag), _p(q_frag), _p(s_frag), _p(bias), _p(y), M, N, K, ldy, epilogue, cfg[0], cfg[1],
                                    _stream())
    _check(rc, "ssd_gemm_w8a16")
