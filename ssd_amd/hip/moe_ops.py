"""ctypes table and torch front end of the mixture-of-experts entry points (include/ssd_hip_moe.h).

Kept apart from ``lib.SIGNATURES`` and the other additive tables: these bind on the same libssdhip.so.  As in ops.py, nothing here
computes in torch; the calls enqueue on the current stream and are hipGraph-capturable.  The expert tables are laid out by
``ops.rows_to_frag`` (mode 1 for gate_up, mode 0 for down), one expert after the other.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind
from .ops import _p, _stream, _check

c_void_p, c_int, c_long = C.c_void_p, C.c_int, C.c_long

EPI_UP, EPI_DOWN = 0, 1
MAX_K, MIN_E, MAX_E = 8, 8, 256

# name -> argtypes, exactly include/ssd_hip_moe.h
MOE_SIGNATURES = {
    "ssd_moe_route": [c_void_p, c_long, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ssd_moe_gemm": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "ssd_moe_combine": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p],
}


def load_moe_library():
    return bind(MOE_SIGNATURES)


def moe_route(logits, ld: int, T: int, E: int, k: int, norm: bool, topk_ids, topk_w, offs, perm):
    """Top-k experts and routing weights of the bf16 router-logit rows [T][ld], and the grouping tables offs [E + 1] / perm [T k]."""
    _check(load_moe_library().ssd_moe_route(_p(logits), ld, T, E, k, 1 if norm else 0, _p(topk_ids), _p(topk_w), _p(offs), _p(perm),
                                            _stream()), "ssd_moe_route")


def moe_gemm(rows_in, w_frag, offs, perm, out, T: int, k: int, E: int, N: int, K: int, epilogue: int):
    """The grouped skinny GEMM over E fragment-major tables [N][K]: EPI_UP x [T][K] -> act [T k][N / 2] = silu(g) * u, EPI_DOWN
    act [T k][K] -> d [T k][N]."""
    _check(load_moe_library().ssd_moe_gemm(_p(rows_in), _p(w_frag), _p(offs), _p(perm), _p(out), T, k, E, N, K, epilogue, _stream()),
           "ssd_moe_gemm")


def moe_combine(d_rows, topk_w, h_rows, T: int, k: int, H: int):
    """h [T][H] = bf16(sum_j topk_w[t][j] * d[t k + j])."""
    _check(load_moe_library().ssd_moe_combine(_p(d_rows), _p(topk_w), _p(h_rows), T, k, H, _stream()), "ssd_moe_combine")
