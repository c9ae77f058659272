"""ctypes table and torch front end of the token constraints (include/ssd_hip_constrain.h): allow mask, minimum length and bad words on
raw logit rows.

Kept apart from ``lib.SIGNATURES`` like the other additive headers (``penalty_ops``, ``logprob_ops``, ...): it binds on the same
libssdhip.so.  Nothing here computes in torch; the call enqueues on the current stream and is hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind
from .ops import _p, _stream, _check

c_void_p, c_int, c_long = C.c_void_p, C.c_int, C.c_long

MAX_EXTRA = 64              # SSD_CONSTRAIN_MAX_EXTRA
MAX_STOP = 64               # SSD_CONSTRAIN_MAX_STOP
MAX_WORDS = 128             # SSD_CONSTRAIN_MAX_WORDS
MAX_WORD_TOKENS = 1024      # SSD_CONSTRAIN_MAX_WORD_TOKENS
MAX_WORD_LEN = 16           # SSD_CONSTRAIN_MAX_WORD_LEN
TAIL_LD = MAX_WORD_LEN - 1  # the host tail: what the longest word's prefix can need
SLICE = 4096                # SSD_CONSTRAIN_SLICE

# name -> argtypes, exactly include/ssd_hip_constrain.h
CONSTRAIN_SIGNATURES = {
    "ssd_constrain_rows": [c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p],
}

LAUNCHES = 0        # constrain_rows calls of this process (eager launches and graph captures; a replay launches without Python)


def load_constrain_library():
    return bind(CONSTRAIN_SIGNATURES)


def mask_words(V: int) -> int:
    """uint32 words of one sequence's allow mask."""
    return (V + 31) // 32


def constrain_rows(logits, ld: int, T: int, V: int, rows_per_seq: int, allow_on=None, allow_bits=None, min_left=None, stop_ids=None,
                   stop_len=None, bw_tok=None, bw_off=None, bw_n=None, tail=None, tail_ld: int = 0, tail_len=None, extra=None,
                   extra_ld: int = 0, extra_n=None) -> None:
    """In place on bf16 logits [T][ld]: banned entries become -inf.  Groups (each whole or None): allow mask (int32 allow_on [B], 32-bit
    allow_bits [B][mask_words(V)]); stop list (int32 min_left [B], stop_ids [B][MAX_STOP], stop_len [B]); bad words (int32 bw_tok
    [B][MAX_WORD_TOKENS], bw_off [B][MAX_WORDS + 1], bw_n [B], tail [B][tail_ld], tail_len [B]); extras (int64 extra [B][extra_ld];
    extra_n None: row j sees extra[b][1..j]; int32 device scalar: every row sees extra[b][1..*extra_n])."""
    global LAUNCHES
    LAUNCHES += 1
    _check(load_constrain_library().ssd_constrain_rows(_p(logits), ld, T, V, rows_per_seq, _p(allow_on), _p(allow_bits), _p(min_left),
                                                       _p(stop_ids), _p(stop_len), _p(bw_tok), _p(bw_off), _p(bw_n), _p(tail), tail_ld,
                                                       _p(tail_len), _p(extra), extra_ld, _p(extra_n), _stream()), "ssd_constrain_rows")
