"""float64 numpy restatement of include/ssd_hip_logprob.h: what ssd_logprob_rows, ssd_logprob_pick and ssd_logprob_pick_verify compute
for one row (the tests' reference; nothing here is on a product path).

A row is an array of values as float (the bf16 logits widened exactly).  NaN is not comparable; -0.0 and +0.0 are one value; a row whose
maximum is not finite has all of its mass on the maximum's class; a row with nothing comparable has lse = NaN and an empty top list."""
from typing import NamedTuple

import numpy as np

MAX_N = 20      # SSD_LOGPROB_MAX_N


class Row(NamedTuple):
    lse: float                  # NaN for a row with nothing comparable
    logprob: np.ndarray         # float64 [V]: log-probability of every entry (NaN entries: NaN)
    top_id: list                # the n largest comparable entries, descending value, ties by lowest index; padded with -1 to n_top
    top_val: list               # their log-probabilities; padded with -inf


def logprob_row(x, n_top: int = 0) -> Row:
    x = np.asarray(x, dtype=np.float64)
    ok = ~np.isnan(x)
    lp = np.full(x.shape, np.nan)
    if not ok.any():
        return Row(float("nan"), lp, [-1] * n_top, [-np.inf] * n_top)
    m = x[ok].max()
    if np.isinf(m):
        cls = ok & (x == m)
        lse = float(m)
        lp[ok] = -np.inf
        lp[cls] = -np.log(cls.sum())
    else:
        with np.errstate(under="ignore"):
            lse = float(m + np.log(np.exp(x[ok] - m).sum()))
        lp[ok] = x[ok] - lse
    idx = np.flatnonzero(ok)
    # descending value, ties by lowest index: a stable sort of the negated values (-0.0 and +0.0 compare equal)
    order = idx[np.argsort(-x[idx], kind="stable")][:n_top]
    pad = n_top - len(order)
    return Row(lse, lp, order.tolist() + [-1] * pad, lp[order].tolist() + [-np.inf] * pad)


def pick(x, token: int, lse: float) -> float:
    """ssd_logprob_pick for one row: float(x[token]) - lse, NaN for a token outside [0, V)."""
    if token < 0 or token >= len(x):
        return float("nan")
    with np.errstate(invalid="ignore"):
        return float(np.float64(x[token]) - lse)


def verify_tokens(ids, accept: int, recovery: int) -> list:
    """The token of each of the K+1 verify rows of one sequence, or None past the recovery row.  ids: the round's K+1 inputs."""
    K = len(ids) - 1
    return [int(ids[j + 1]) if (j < accept and j < K) else int(recovery) if j == accept else None for j in range(K + 1)]
