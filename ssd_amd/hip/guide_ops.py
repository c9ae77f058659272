"""ctypes table and torch front end of guided decoding (include/ssd_hip_guide.h): the walk of every sequence's token automaton through
the round's tokens, and the allow set of every row's state written over the raw logit rows.

Kept apart from ``lib.SIGNATURES`` like the other additive headers (``penalty_ops``, ``constrain_ops``, ...): it binds on the same
libssdhip.so.  Nothing here computes in torch; the calls enqueue on the current stream and are hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind
from .ops import _p, _stream, _check

c_void_p, c_int, c_long = C.c_void_p, C.c_int, C.c_long

MAX_STATES = 16384          # SSD_GUIDE_MAX_STATES
MAX_EDGES = 262144          # SSD_GUIDE_MAX_EDGES (also the largest edges_ld the calls take)
MAX_EXTRA = 64              # SSD_GUIDE_MAX_EXTRA
SLICE = 4096                # SSD_GUIDE_SLICE

# name -> argtypes, exactly include/ssd_hip_guide.h
GUIDE_SIGNATURES = {
    "ssd_guide_walk": [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                       c_int, c_void_p, c_void_p],
    "ssd_guide_rows": [c_void_p, c_long, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                       c_void_p],
}

LAUNCHES = 0        # guide_walk + guide_rows calls of this process (eager launches and graph captures; a replay launches without Python)


def load_guide_library():
    return bind(GUIDE_SIGNATURES)


def guide_walk(state_rows, T: int, rows_per_seq: int, guide_on, state0, n_states, edge_off, dflt, edge_tok, edge_next, states_ld: int,
               edges_ld: int, extra=None, extra_ld: int = 0, extra_n=None) -> None:
    """int32 state_rows [T] = the automaton state in front of every row: int32 state0 [B] (-1 where int32 guide_on [B] is 0) advanced
    through the extras the row sees (int64 extra [B][extra_ld]; extra_n None: row j sees extra[b][1..j]; int32 device scalar: every
    row sees extra[b][1..*extra_n]).  Tables: int32 n_states [B], edge_off [B][states_ld + 1], dflt [B][states_ld], edge_tok and
    edge_next [B][edges_ld]."""
    global LAUNCHES
    LAUNCHES += 1
    _check(load_guide_library().ssd_guide_walk(_p(state_rows), T, rows_per_seq, _p(guide_on), _p(state0), _p(n_states), _p(edge_off),
                                               _p(dflt), _p(edge_tok), _p(edge_next), states_ld, edges_ld, _p(extra), extra_ld,
                                               _p(extra_n), _stream()), "ssd_guide_walk")


def guide_rows(logits, ld: int, T: int, V: int, state_rows, rows_per_seq: int, n_states, edge_off, dflt, edge_tok, edge_next,
               states_ld: int, edges_ld: int) -> None:
    """In place on bf16 logits [T][ld]: entries the state of their row (int32 state_rows [T]; -1 = no guide) does not allow become
    -inf.  The tables are those of guide_walk."""
    global LAUNCHES
    LAUNCHES += 1
    _check(load_guide_library().ssd_guide_rows(_p(logits), ld, T, V, _p(state_rows), rows_per_seq, _p(n_states), _p(edge_off), _p(dflt),
                                               _p(edge_tok), _p(edge_next), states_ld, edges_ld, _stream()), "ssd_guide_rows")
