"""ctypes table and torch front end of the logit penalties (include/ssd_hip_penalty.h): repetition / presence / frequency penalties and
logit bias on raw logit rows.

Kept apart from ``lib.SIGNATURES`` like the other additive headers (``filter_ops``, ``kv8_ops``, ...): it binds on the same
libssdhip.so.  Nothing here computes in torch; the call enqueues on the current stream and is hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind
from .ops import _p, _stream, _check

c_void_p, c_int, c_long = C.c_void_p, C.c_int, C.c_long

MAX_EXTRA = 64      # SSD_PENALTY_MAX_EXTRA

# name -> argtypes, exactly include/ssd_hip_penalty.h
PENALTY_SIGNATURES = {
    "ssd_penalize_rows": [c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                          c_void_p, c_void_p, c_int, c_void_p, c_void_p],
}

LAUNCHES = 0        # penalize_rows calls of this process (eager launches and graph captures; a replay launches without Python)


def load_penalty_library():
    return bind(PENALTY_SIGNATURES)


def pack_count(count: int, in_prompt: bool) -> int:
    """One tab_cnt entry: (output count << 1) | in-prompt flag."""
    return (int(count) << 1) | (1 if in_prompt else 0)


def penalize_rows(logits, ld: int, T: int, V: int, rows_per_seq: int, tab_ids, tab_cnt, tab_bias, tab_ld: int, tab_len, rep, pres, freq,
                  extra=None, extra_ld: int = 0, extra_n=None) -> None:
    """In place on bf16 logits [T][ld]: logit bias, repetition, frequency and presence penalty at the ids of each sequence's history
    table (int32 tab_ids / tab_cnt, fp32 tab_bias: [B][tab_ld]; int32 tab_len [B]; all four None = no history) and at the extra
    tokens of the round (int64 extra [B][extra_ld]; extra_n None: row j sees extra[b][1..j]; int32 device scalar: every row sees
    extra[b][1..*extra_n]).  rep / pres / freq: fp32 [B] on the device."""
    global LAUNCHES
    LAUNCHES += 1
    _check(load_penalty_library().ssd_penalize_rows(_p(logits), ld, T, V, rows_per_seq, _p(tab_ids), _p(tab_cnt), _p(tab_bias), tab_ld,
                                                    _p(tab_len), _p(rep), _p(pres), _p(freq), _p(extra), extra_ld, _p(extra_n),
                                                    _stream()), "ssd_penalize_rows")
