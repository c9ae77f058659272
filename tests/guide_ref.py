"""numpy restatement of include/ssd_hip_guide.h, written from the header: delta over the flattened tables of one batch row, the walk of
every row's state through the extras it sees, and the rows whose banned entries become -inf.  Rows are uint16 arrays of bf16 bit
patterns, so that comparisons are on bits (NaN payloads, signed zeros, pad columns).

An automaton here is a dict of the five per-row tables: "n" (number of states) and the int arrays "off" [>= n + 1], "dflt" [>= n],
"tok" and "next" [edges], exactly what one slot of the device tables holds (unused parts may hold anything)."""
from __future__ import annotations

import numpy as np

NINF = 0xFF80
MAX_STATES, MAX_EDGES, MAX_EXTRA, SLICE = 16384, 262144, 64, 4096


def tables_of(automaton) -> dict:
    """The tables of a ssd_amd.guide.TokenAutomaton."""
    return dict(n=automaton.num_states, off=np.asarray(automaton.edge_off), dflt=np.asarray(automaton.dflt),
                tok=np.asarray(automaton.edge_tok), next=np.asarray(automaton.edge_next))


def tables_from(n: int, states: dict, dflt: dict | None = None) -> dict:
    """Tables from {state: [(token, next), ...]} (sorted here by token) and {state: default}; nothing is validated, so a test can write
    next states outside [-1, n)."""
    off, tok, nxt = [0], [], []
    for s in range(n):
        for t, x in sorted(states.get(s, ())):
            tok.append(t)
            nxt.append(x)
        off.append(len(tok))
    d = [-1] * n
    for s, x in (dflt or {}).items():
        d[s] = x
    return dict(n=n, off=np.array(off, np.int64), dflt=np.array(d, np.int64), tok=np.array(tok, np.int64), next=np.array(nxt, np.int64))


def _next(a: dict, x: int) -> int:
    return int(x) if -1 <= int(x) < a["n"] else -1          # a next state outside [-1, n) reads as -1


def edge_range(a: dict, s: int, edges_ld: int | None = None) -> tuple[int, int]:
    o0, o1 = int(a["off"][s]), int(a["off"][s + 1])
    ld = len(a["tok"]) if edges_ld is None else edges_ld
    return (0, 0) if (o0 < 0 or o1 > ld or o1 < o0) else (o0, o1)          # offsets that leave the table or run backwards: no edges


def delta(a: dict, s: int, t: int, edges_ld: int | None = None) -> int:
    if not 0 <= s < a["n"]:
        return -1
    o0, o1 = edge_range(a, s, edges_ld)
    hit = np.nonzero(np.asarray(a["tok"][o0:o1]) == t)[0]
    if len(hit):
        return _next(a, a["next"][o0 + int(hit[0])])
    return _next(a, a["dflt"][s])


def extras_seen(extra_row, j: int, extra_n) -> list[int]:
    """The extras row j of a sequence sees: prefix form (extra_n None) entries 1..j, chain form entries 1..clamp(extra_n)."""
    if extra_row is None:
        return []
    m = j if extra_n is None else min(max(int(extra_n), 0), len(extra_row) - 1)
    return [int(t) for t in extra_row[1:1 + m]]


def walk(T: int, rows_per_seq: int, autos, guide_on, state0, extra=None, extra_n=None, edges_ld: int | None = None) -> np.ndarray:
    """int32 [T]: the state in front of every row.  autos: one tables dict per sequence (None where guide_on is 0 is fine)."""
    out = np.full(T, -1, dtype=np.int32)
    for row in range(T):
        b, j = divmod(row, rows_per_seq)
        a = autos[b]
        if not guide_on[b] or a is None or not 0 <= int(state0[b]) < a["n"]:
            continue
        s = int(state0[b])
        for t in extras_seen(extra[b] if extra is not None else None, j, extra_n):
            s = -1 if (t < 0 or t > 2 ** 31 - 1) else delta(a, s, t, edges_ld)
        out[row] = s
    return out


def allowed_set(a: dict, s: int, V: int, edges_ld: int | None = None) -> np.ndarray:
    """bool [V]: the tokens allowed at state s (0 <= s < n)."""
    ok = np.full(V, _next(a, a["dflt"][s]) != -1)
    o0, o1 = edge_range(a, s, edges_ld)
    for t, x in zip(a["tok"][o0:o1], a["next"][o0:o1]):
        if 0 <= t < V:
            ok[int(t)] = _next(a, x) != -1
    return ok


def guide_rows(bits: np.ndarray, V: int, rows_per_seq: int, autos, state_rows, edges_ld: int | None = None) -> np.ndarray:
    """bits: uint16 [T][ld].  Returns the guided copy: entries below V that the row's state does not allow become -inf; rows whose
    state is -1 or not a state, and columns >= V, keep their bits."""
    out = np.array(bits, dtype=np.uint16, copy=True)
    for row in range(out.shape[0]):
        a, s = autos[row // rows_per_seq], int(state_rows[row])
        if a is None or not 0 <= s < a["n"]:
            continue
        out[row, :V][~allowed_set(a, s, V, edges_ld)] = NINF
    return out
