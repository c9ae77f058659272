"""ctypes table and torch front end of the prompt log-probability kernel (include/ssd_hip_prompt_logprob.h): log-sum-exp, the N most
probable entries, and the log-probability and rank of a token that is known before its row is read, in one pass over the row.

Kept apart from ``lib.SIGNATURES`` like the other additive headers (``logprob_ops``, ``filter_ops``, ...): it binds on the same
libssdhip.so.  Nothing here computes in torch; every call enqueues on the current stream and is hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind, SsdHipError
from .logprob_ops import MAX_N, MAX_V  # noqa: F401  (the limits are ssd_hip_logprob.h's)
from .ops import _p, _stream, _check

c_void_p, c_int, c_long = C.c_void_p, C.c_int, C.c_long

# name -> argtypes, exactly include/ssd_hip_prompt_logprob.h
PROMPT_LOGPROB_SIGNATURES = {
    "ssd_logprob_known_ws_bytes": [c_int, c_int],
    "ssd_logprob_rows_known": [c_void_p, c_long, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p],
}

LAUNCHES = 0        # kernel-launching calls of this process


def load_prompt_logprob_library():
    return bind(PROMPT_LOGPROB_SIGNATURES)


def logprob_known_ws_bytes(T: int, V: int) -> int:
    n = load_prompt_logprob_library().ssd_logprob_known_ws_bytes(T, V)
    if n < 0:
        raise SsdHipError(f"ssd_logprob_known_ws_bytes({T}, {V}) failed with code {n}")
    return n


def logprob_rows_known(logits, ld: int, T: int, V: int, n_top, tokens, lse, top_val, top_id, out, rank, ws) -> None:
    """Raw bf16 logits [T][ld], read only, and the token each row must score (int64 [T]) -> lse fp32 [T], top_val fp32 / top_id int32
    [T][MAX_N], out fp32 [T] (the token's log-probability) and rank int32 [T].  n_top: int32 [T] on the device, one entry per row; -1
    skips the row and its token is not read."""
    global LAUNCHES
    LAUNCHES += 1
    _check(load_prompt_logprob_library().ssd_logprob_rows_known(_p(logits), ld, T, V, _p(n_top), _p(tokens), _p(lse), _p(top_val),
                                                                _p(top_id), _p(out), _p(rank), _p(ws), _stream()),
           "ssd_logprob_rows_known")
