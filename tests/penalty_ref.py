"""numpy restatement of include/ssd_hip_penalty.h: logit bias, repetition, frequency and presence penalty on rows of bf16 logits, every
step in fp32 and rounded on its own, the result rounded to bf16 (nearest even).  Rows are uint16 arrays of bf16 bit patterns, so that
comparisons are on bits (NaN payloads, signed zeros, pad columns)."""
from __future__ import annotations

from collections import Counter

import numpy as np

F32 = np.float32


def bf16_to_f32(bits) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16(x) -> np.ndarray:
    """Round to nearest even; a NaN becomes the quiet NaN 0x7FC0 (the header's rule for a NaN the arithmetic produced)."""
    x = np.asarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def is_nan_bits(b: int) -> bool:
    return (int(b) & 0x7FFF) > 0x7F80


def adjust(bits: int, bias: float, in_prompt: bool, c: int, r: float, p: float, f: float) -> int:
    """One entry: steps 1-5 of the header.  bias 0 = none."""
    if is_nan_bits(bits):
        return int(bits)
    with np.errstate(all="ignore"):
        x = bf16_to_f32(np.uint16(bits))[()]
        if F32(bias) != 0:
            x = F32(x + F32(bias))
        if in_prompt or c > 0:
            x = F32(x * F32(r)) if x < 0 else F32(x / F32(r))
        if c > 0:
            x = F32(x - F32(F32(f) * F32(c)))
            x = F32(x - F32(p))
    return int(f32_to_bf16(x)[()])


def history(table, extras, V: int):
    """token -> [c, in_prompt, bias] of one row: the table's entries (id, count, in_prompt, bias) plus the extra tokens (output tokens);
    ids outside [0, V) are ignored."""
    h = {}
    for t, c, ip, b in table:
        if 0 <= t < V:
            assert t not in h, "table ids are unique"
            h[t] = [int(c), bool(ip), float(b)]
    for t, n in Counter(int(t) for t in extras).items():
        if 0 <= t < V:
            h.setdefault(t, [0, False, 0.0])[0] += n
    return h


def penalize_rows(bits: np.ndarray, V: int, rows_per_seq: int, tables, rep, pres, freq, extra=None, extra_n=None) -> np.ndarray:
    """bits: uint16 [T][ld].  tables: per sequence a list of (id, count, in_prompt, bias), or None (no table at all).  extra: int
    [B][extra_ld] or None; extra_n None: prefix form (row j sees extra[b][1..j]), an int: chain form (every row sees extra[b][1..n],
    n clamped to [0, extra_ld - 1]).  Returns the adjusted copy; columns >= V are never written."""
    out = np.array(bits, dtype=np.uint16, copy=True)
    T = out.shape[0]
    for row in range(T):
        b, j = divmod(row, rows_per_seq)
        r, p, f = float(rep[b]), float(pres[b]), float(freq[b])
        pen = not (F32(r) == 1 and F32(p) == 0 and F32(f) == 0)
        ex = []
        if extra is not None and pen:
            m = j if extra_n is None else min(max(int(extra_n), 0), len(extra[b]) - 1)
            ex = list(extra[b][1:1 + m])
        tab = tables[b] if tables is not None else []
        for t, (c, ip, bias) in history(tab, ex, V).items():
            out[row, t] = adjust(out[row, t], bias, ip, c, r, p, f)
    return out


def table_of(prompt, output, bias=None):
    """The table a recount from scratch gives: unique ids of prompt, output and bias, as {id: [count, in_prompt, bias]}; negative
    ids (placeholders) are no history."""
    tab = {int(t): [0, False, float(v)] for t, v in (bias or {}).items()}
    for t in prompt:
        if t >= 0:
            tab.setdefault(int(t), [0, False, 0.0])[1] = True
    for t in output:
        if t >= 0:
            tab.setdefault(int(t), [0, False, 0.0])[0] += 1
    return tab
