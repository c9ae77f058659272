"""ctypes table and torch front end of the zero-point W4A16 entry points (include/ssd_hip_w4zp.h).

Kept apart from ``lib.SIGNATURES``, ``quant_ops.QUANT_SIGNATURES``, ``w4_ops.W4_SIGNATURES`` and ``mx4_ops``' table: these bind on
the same libssdhip.so.  As in ops.py, nothing here computes in torch; the calls enqueue on the current stream and are
hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind
from .ops import _p, _stream, _check, EPI_ROWS

c_void_p, c_int = C.c_void_p, C.c_int

# name -> argtypes, exactly include/ssd_hip_w4zp.h
W4ZP_SIGNATURES = {
    "ssd_w4zp_rows_to_frag": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "ssd_w4zp_frag_to_rows": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "ssd_w4zp_dequant_frag": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "ssd_gemm_w4a16_zp": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "ssd_gemm_w4a16_zp_cfg": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                              c_void_p],
}


def load_w4zp_library():
    return bind(W4ZP_SIGNATURES)


def w4zp_rows_to_frag(packed, scale, zero, q_frag, s_frag, z_frag, N: int, K: int, row_map=None):
    """packed: int32 [N, K/8]; scale: bf16 [N, K/128]; zero: uint8 [N, K/128]; q_frag: N*K/2 bytes; s_frag: bf16 N*K/128; z_frag:
    uint8 N*K/128; row_map: int32 [N] source row of every destination row (None = identity)."""
    _check(load_w4zp_library().ssd_w4zp_rows_to_frag(_p(packed), _p(scale), _p(zero), _p(q_frag), _p(s_frag), _p(z_frag), _p(row_map),
                                                     N, K, _stream()), "ssd_w4zp_rows_to_frag")


def w4zp_frag_to_rows(q_frag, s_frag, z_frag, packed, scale, zero, N: int, K: int):
    _check(load_w4zp_library().ssd_w4zp_frag_to_rows(_p(q_frag), _p(s_frag), _p(z_frag), _p(packed), _p(scale), _p(zero), N, K,
                                                     _stream()), "ssd_w4zp_frag_to_rows")


def w4zp_dequant_frag(q_frag, s_frag, z_frag, w_frag, N: int, K: int):
    """bf16 frag [N, K] = bf16(s * (u - z)) for the bf16 prefill GEMMs."""
    _check(load_w4zp_library().ssd_w4zp_dequant_frag(_p(q_frag), _p(s_frag), _p(z_frag), _p(w_frag), N, K, _stream()),
           "ssd_w4zp_dequant_frag")


def gemm_w4a16_zp(x_frag, q_frag, s_frag, z_frag, y, M: int, N: int, K: int, ldy: int, epilogue: int = EPI_ROWS, bias=None, cfg=None):
    lib = load_w4zp_library()
    if cfg is None:
        rc = lib.ssd_gemm_w4a16_zp(_p(x_frag), _p(q_frag), _p(s_frag), _p(z_frag), _p(bias), _p(y), M, N, K, ldy, epilogue, _stream())
    else:
        rc = lib.ssd_gemm_w4a16_zp_cfg(_p(x_frag), _p(q_frag), _p(s_frag), _p(z_frag), _p(bias), _p(y), M, N, K, ldy, epilogue, cfg[0],
                                       cfg[1], _stream())
    _check(rc, "ssd_gemm_w4a16_zp")
