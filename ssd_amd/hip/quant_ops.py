"""ctypes table and torch front end of the FP8 weight entry points (include/ssd_hip_quant.h).

Kept apart from ``lib.SIGNATURES``, which is exactly ssd_hip.h + ssd_hip_tune.h: these bind on the same libssdhip.so.  As in
ops.py, nothing here computes in torch; the calls enqueue on the current stream and are hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind
from .ops import _p, _stream, _check, EPI_ROWS

c_void_p, c_int = C.c_void_p, C.c_int

# name -> argtypes, exactly include/ssd_hip_quant.h
QUANT_SIGNATURES = {
    "ssd_fp8_rows_to_frag": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "ssd_fp8_frag_to_rows": [c_void_p, c_void_p, c_int, c_int, c_void_p],
    "ssd_fp8_dequant_frag": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "ssd_gemm_fp8": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "ssd_gemm_fp8_cfg": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
}


def load_quant_library():
    return bind(QUANT_SIGNATURES)


def fp8_rows_to_frag(q_rows, q_frag, N: int, K: int, row_map=None):
    """q_rows: [N, K] float8_e4m3fn (or its uint8 view); row_map: int32 [N] source row of every destination row (None = identity)."""
    _check(load_quant_library().ssd_fp8_rows_to_frag(_p(q_rows), _p(q_frag), _p(row_map), N, K, _stream()), "ssd_fp8_rows_to_frag")


def fp8_frag_to_rows(q_frag, q_rows, N: int, K: int):
    _check(load_quant_library().ssd_fp8_frag_to_rows(_p(q_frag), _p(q_rows), N, K, _stream()), "ssd_fp8_frag_to_rows")


def fp8_dequant_frag(q_frag, scale, w_frag, N: int, K: int):
    """bf16 frag [N, K] = bf16(scale[n] * q[n, k]) for the bf16 prefill GEMMs."""
    _check(load_quant_library().ssd_fp8_dequant_frag(_p(q_frag), _p(scale), _p(w_frag), N, K, _stream()), "ssd_fp8_dequant_frag")


def gemm_fp8(x_frag, q_frag, scale, y, M: int, N: int, K: int, ldy: int, epilogue: int = EPI_ROWS, bias=None, cfg=None):
    lib = load_quant_library()
    if cfg is None:
        rc = lib.ssd_gemm_fp8(_p(x_frag), _p(q_frag), _p(scale), _p(bias), _p(y), M, N, K, ldy, epilogue, _stream())
    else:
        rc = lib.ssd_gemm_fp8_cfg(_p(x_frag), _p(q_frag), _p(scale), _p(bias), _p(y), M, N, K, ldy, epilogue, cfg[0], cfg[1], _stream())
    _check(rc, "ssd_gemm_fp8")
