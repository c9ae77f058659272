"""ctypes table and torch front end of the log-probability kernels (include/ssd_hip_logprob.h): log-sum-exp and the N most probable
entries of raw logit rows, and the log-probability of the token each row produced.

Kept apart from ``lib.SIGNATURES`` like the other additive headers (``filter_ops``, ``penalty_ops``, ...): it binds on the same
libssdhip.so.  Nothing here computes in torch; every call enqueues on the current stream and is hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind, SsdHipError
from .ops import _p, _stream, _check

c_void_p, c_int, c_long = C.c_void_p, C.c_int, C.c_long

MAX_N = 20          # SSD_LOGPROB_MAX_N: the largest logprobs=N, and the row stride of top_val / top_id
MAX_V = 196608      # SSD_LOGPROB_MAX_V

# name -> argtypes, exactly include/ssd_hip_logprob.h
LOGPROB_SIGNATURES = {
    "ssd_logprob_rows_ws_bytes": [c_int, c_int],
    "ssd_logprob_rows": [c_void_p, c_long, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p,
                         c_void_p],
    "ssd_logprob_pick": [c_void_p, c_long, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p],
    "ssd_logprob_pick_verify": [c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p],
}

LAUNCHES = 0        # kernel-launching calls of this process (eager launches and graph captures; a replay launches without Python)


def load_logprob_library():
    return bind(LOGPROB_SIGNATURES)


def logprob_rows_ws_bytes(T: int, V: int) -> int:
    n = load_logprob_library().ssd_logprob_rows_ws_bytes(T, V)
    if n < 0:
        raise SsdHipError(f"ssd_logprob_rows_ws_bytes({T}, {V}) failed with code {n}")
    return n


def logprob_rows(logits, ld: int, T: int, V: int, n_top, rows_per_param: int, lse, top_val, top_id, ws, raw_copy=None,
                 raw_ld: int = 0) -> None:
    """Raw bf16 logits [T][ld], read only -> lse fp32 [T], top_val fp32 / top_id int32 [T][MAX_N], and (raw_copy) a bit-exact copy of
    the rows.  n_top: int32 on the device, one entry per rows_per_param rows; -1 skips the row."""
    global LAUNCHES
    LAUNCHES += 1
    _check(load_logprob_library().ssd_logprob_rows(_p(logits), ld, T, V, _p(n_top), rows_per_param, _p(lse), _p(top_val), _p(top_id),
                                                   _p(raw_copy), raw_ld, _p(ws), _stream()), "ssd_logprob_rows")


def logprob_pick(rows, ld: int, T: int, V: int, tokens, lse, n_top, rows_per_param: int, out) -> None:
    """out[t] = rows[t][tokens[t]] - lse[t]; tokens int64 [T]."""
    global LAUNCHES
    LAUNCHES += 1
    _check(load_logprob_library().ssd_logprob_pick(_p(rows), ld, T, V, _p(tokens), _p(lse), _p(n_top), rows_per_param, _p(out),
                                                   _stream()), "ssd_logprob_pick")


def logprob_pick_verify(rows, ld: int, B: int, K: int, V: int, ids, accept, recovery, lse, n_top, out) -> None:
    """The pick over the B * (K+1) rows of a verify: accepted inputs, the recovery token, NaN past it."""
    global LAUNCHES
    LAUNCHES += 1
    _check(load_logprob_library().ssd_logprob_pick_verify(_p(rows), ld, B, K, V, _p(ids), _p(accept), _p(recovery), _p(lse), _p(n_top),
                                                          _p(out), _stream()), "ssd_logprob_pick_verify")
