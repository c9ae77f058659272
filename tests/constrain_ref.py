"""numpy restatement of include/ssd_hip_constrain.h, written from the header: which entries of a logits row are banned by the allow mask,
the minimum length and the bad words, given the host tail and the extras the row sees.  Rows are uint16 arrays of bf16 bit patterns, so
that comparisons are on bits (NaN payloads, signed zeros, pad columns)."""
from __future__ import annotations

import numpy as np

NINF = 0xFF80
MAX_EXTRA, MAX_STOP, MAX_WORDS, MAX_WORD_TOKENS, MAX_WORD_LEN = 64, 64, 128, 1024, 16


def mask_words(V: int) -> int:
    return (V + 31) // 32


def mask_of(ids, V: int) -> np.ndarray:
    """uint32 [ceil(V / 32)] with the bits of `ids` set; ids outside [0, V) set nothing."""
    m = np.zeros(mask_words(V), dtype=np.uint32)
    for t in ids:
        if 0 <= t < V:
            m[t >> 5] |= np.uint32(1 << (t & 31))
    return m


def extras_seen(extra_row, j: int, extra_n) -> list[int]:
    """The extras row j of a sequence sees: prefix form (extra_n None) entries 1..j, chain form entries 1..clamp(extra_n)."""
    if extra_row is None:
        return []
    m = j if extra_n is None else min(max(int(extra_n), 0), len(extra_row) - 1)
    return [int(t) for t in extra_row[1:1 + m]]


def banned(V: int, context, e: int, allow=None, min_left: int = 0, stops=(), words=()) -> set[int]:
    """Banned ids of one row.  context: the tail followed by the row's e extras; allow: None (off) or the uint32 mask words."""
    out = set()
    if allow is not None:           # (a)
        t = np.arange(V)
        out |= {int(i) for i in np.nonzero(((np.asarray(allow, dtype=np.uint32)[t >> 5] >> (t & 31).astype(np.uint32)) & 1) == 0)[0]}
    if e < min_left:                # (b)
        out |= {int(t) for t in stops if 0 <= t < V}
    for w in words:                 # (c)
        L = len(w)
        if not 1 <= L <= MAX_WORD_LEN:
            continue
        t = int(w[-1])
        if not 0 <= t < V:
            continue
        if L == 1 or (len(context) >= L - 1 and [int(c) for c in context[len(context) - (L - 1):]] == [int(x) for x in w[:-1]]):
            out.add(t)
    return out


def constrain_rows(bits: np.ndarray, V: int, rows_per_seq: int, seqs, extra=None, extra_n=None, tail_ld: int = MAX_WORD_LEN - 1) -> np.ndarray:
    """bits: uint16 [T][ld].  seqs: per sequence a dict with the optional keys "allow" (uint32 mask words; absent or None = off),
    "min_left" and "stops", "words" (lists of ids) and "tail" (the tokens the host knows, oldest first; the last tail_ld count).
    extra: int [B][extra_ld] or None; extra_n as in extras_seen.  Returns the constrained copy; columns >= V are never written."""
    out = np.array(bits, dtype=np.uint16, copy=True)
    for row in range(out.shape[0]):
        b, j = divmod(row, rows_per_seq)
        s = seqs[b]
        ex = extras_seen(extra[b] if extra is not None else None, j, extra_n)
        tail = [int(t) for t in s.get("tail", [])][-tail_ld:] if tail_ld > 0 else []
        for t in banned(V, tail + ex, len(ex), s.get("allow"), int(s.get("min_left", 0)), s.get("stops", ()), s.get("words", ())):
            out[row, t] = NINF
    return out


def flatten_words(words):
    """(tokens, offsets) of a word list, as bw_tok / bw_off rows hold them."""
    tok, off = [], [0]
    for w in words:
        tok.extend(int(t) for t in w)
        off.append(len(tok))
    return tok, off
