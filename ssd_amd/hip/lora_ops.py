"""ctypes table and torch front end of the LoRA adapter entry points (include/ssd_hip_lora.h).

Kept apart from ``lib.SIGNATURES`` and the other additive tables: these bind on the same libssdhip.so.  As in ops.py, nothing here
computes in torch; the calls enqueue on the current stream and are hipGraph-capturable.  The slot tables are laid out by
``ops.rows_to_frag`` (mode 0), one matrix after the other.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind
from .ops import _p, _stream, _check

c_void_p, c_int, c_long = C.c_void_p, C.c_int, C.c_long

EPI_ADD, EPI_SILU = 0, 1
MAX_R, MAX_SPLITS = 192, 16

# name -> argtypes, exactly include/ssd_hip_lora.h
LORA_SIGNATURES = {
    "ssd_lora_default_splits": [c_int],
    "ssd_lora_workspace_bytes": [c_int, c_int, c_int],
    "ssd_lora_shrink": [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "ssd_lora_expand": [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                        c_int, c_int, c_void_p],
}
_RESTYPES = {"ssd_lora_workspace_bytes": c_long}


def load_lora_library():
    return bind(LORA_SIGNATURES, _RESTYPES)


def lora_default_splits(K: int) -> int:
    return load_lora_library().ssd_lora_default_splits(K)


def lora_workspace_bytes(M: int, K: int, R: int) -> int:
    return load_lora_library().ssd_lora_workspace_bytes(M, K, R)


def _nbytes(t) -> int:
    return 0 if t is None else t.numel() * t.element_size()


def lora_shrink(x_frag, a_frag, row_slot, ws, M: int, K: int, R: int, slots: int, splits: int = 0):
    """fp32 slabs ws[splits][M][R] = x . A[row_slot]^T for the rows that name a slot (splits 0: the default)."""
    _check(load_lora_library().ssd_lora_shrink(_p(x_frag), _p(a_frag), _p(row_slot), _p(ws), _nbytes(ws), M, K, R, slots, splits,
                                               _stream()), "ssd_lora_shrink")


def lora_expand(ws, b_frag, scale, row_slot, y, ldy: int, M: int, N: int, K: int, R: int, slots: int, splits: int = 0,
                epilogue: int = EPI_ADD, act_frag=None):
    """y rows += scale[slot] * t . B[slot]^T in place (EPI_ADD), or act_frag = silu(gate) * up of the updated packed rows (EPI_SILU)."""
    _check(load_lora_library().ssd_lora_expand(_p(ws), _nbytes(ws), _p(b_frag), _p(scale), _p(row_slot), _p(y), ldy, _p(act_frag), M, N, K,
                                               R, slots, splits, epilogue, _stream()), "ssd_lora_expand")
