"""ctypes table and torch front end of the logit filter (include/ssd_hip_filter.h): top-k / top-p / min-p truncation of sampled rows.

Kept apart from ``lib.SIGNATURES`` like the other additive headers (``kv8_ops``, ``quant_ops``, ...): it binds on the same
libssdhip.so.  Nothing here computes in torch; the call enqueues on the current stream and is hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind
from .ops import _p, _stream, _check

c_void_p, c_int, c_long = C.c_void_p, C.c_int, C.c_long

MAX_V = 196608      # SSD_FILTER_MAX_V

# name -> argtypes, exactly include/ssd_hip_filter.h
FILTER_SIGNATURES = {
    "ssd_filter_rows": [c_void_p, c_long, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p],
}

LAUNCHES = 0        # filter_rows calls of this process (eager launches and graph captures; a replay launches without Python)


def load_filter_library():
    return bind(FILTER_SIGNATURES)


def filter_rows(logits, ld: int, T: int, V: int, temps, top_k, top_p, min_p, rows_per_param: int, kept=None) -> None:
    """In place on bf16 logits [T][ld]: entries outside the top-k / top-p / min-p set of their row become -inf.  temps, top_p, min_p:
    fp32, top_k: int32, one entry per rows_per_param rows, on the device; kept: optional int32 [T] (survivors per row)."""
    global LAUNCHES
    LAUNCHES += 1
    _check(load_filter_library().ssd_filter_rows(_p(logits), ld, T, V, _p(temps), _p(top_k), _p(top_p), _p(min_p), rows_per_param,
                                                 _p(kept), _stream()), "ssd_filter_rows")
