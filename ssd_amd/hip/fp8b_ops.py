"""ctypes table and torch front end of the block-scaled FP8 entry points (include/ssd_hip_fp8b.h).

Kept apart from ``lib.SIGNATURES``, ``quant_ops.QUANT_SIGNATURES`` and the int4 / mxfp4 tables: these bind on the same
libssdhip.so.  As in ops.py, nothing here computes in torch; the calls enqueue on the current stream and are hipGraph-capturable.
The codes are laid out by ``quant_ops.fp8_rows_to_frag``; the group table (fp32 [N/16, ceil(K/128)], packed row order) is built on
the host by ``quant.fp8_block_group_scales``.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind
from .ops import _p, _stream, _check, EPI_ROWS

c_void_p, c_int = C.c_void_p, C.c_int

# name -> argtypes, exactly include/ssd_hip_fp8b.h
FP8B_SIGNATURES = {
    "ssd_fp8b_dequant_frag": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "ssd_gemm_fp8b": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "ssd_gemm_fp8b_cfg": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
}


def load_fp8b_library():
    return bind(FP8B_SIGNATURES)


def fp8b_dequant_frag(q_frag, s_grp, w_frag, N: int, K: int):
    """bf16 frag [N, K] = bf16(s_grp[n / 16, k / 128] * q) for the bf16 prefill GEMMs."""
    _check(load_fp8b_library().ssd_fp8b_dequant_frag(_p(q_frag), _p(s_grp), _p(w_frag), N, K, _stream()), "ssd_fp8b_dequant_frag")


def gemm_fp8b(x_frag, q_frag, s_grp, y, M: int, N: int, K: int, ldy: int, epilogue: int = EPI_ROWS, bias=None, cfg=None):
    lib = load_fp8b_library()
    if cfg is None:
        rc = lib.ssd_gemm_fp8b(_p(x_frag), _p(q_frag), _p(s_grp), _p(bias), _p(y), M, N, K, ldy, epilogue, _stream())
    else:
        rc = lib.ssd_gemm_fp8b_cfg(_p(x_frag), _p(q_frag), _p(s_grp), _p(bias), _p(y), M, N, K, ldy, epilogue, cfg[0], cfg[1], _stream())
    _check(rc, "ssd_gemm_fp8b")
