"""float64 numpy restatement of the logit filter's semantics (include/ssd_hip_filter.h), the reference of tests/test_hip_filter.py and
tests/test_engine_filter_gpu.py.  Nothing here is shared with the kernel: values are compared as float64 numbers, k-th largest comes
from a sort, masses are float64 sums per distinct value.

For one row x[0..V) and temperature T > 0:  s = x / T,  m = max s,  e = exp(s - m);  kept = K & P & M with
  K  x >= (k-th largest value)                       top_k = 0 or >= V: off
  P  x >= t_p, t_p = the largest value v with  mass(K, x >= v) >= top_p * mass(K)        top_p = 1: off
  M  e >= min_p                                      min_p = 0: off
NaN is not comparable (not counted, no mass, never kept); a row with temperature 0, with all parameters off or with nothing
comparable is untouched; a row whose maximum is not finite has all its mass on the maximum's class."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class RowResult:
    keep: np.ndarray            # bool [V]: the kept set (all True for an untouched row)
    touched: bool               # False: the kernel must leave the row bit for bit
    e: np.ndarray | None        # float64 [V] exp(s - m) (0 for NaN entries), None for an untouched row
    in_k: np.ndarray | None     # bool [V] the top-k set K
    p_margin: float             # top_p: relative distance of top_p * mass(K) from the two masses that decide t_p (inf: top_p off)


def f32(v) -> float:
    return float(np.float32(v))


def exp_row(x: np.ndarray, T: float):
    """(e, comparable): e = exp(x / T - max) in float64 over the comparable entries, 0 elsewhere."""
    x = np.asarray(x, dtype=np.float64)
    comp = ~np.isnan(x)
    e = np.zeros_like(x)
    if not comp.any():
        return e, comp
    mx = x[comp].max()
    if np.isfinite(mx):
        with np.errstate(over="ignore", under="ignore"):
            e[comp] = np.exp(x[comp] / f32(T) - mx / f32(T))
    else:
        e[comp & (x == mx)] = 1.0
    return e, comp


def filter_row(x, T: float, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0) -> RowResult:
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[0]
    T, top_p, min_p = f32(T), f32(top_p), f32(min_p)          # the kernel reads fp32 parameters
    k_on, p_on, m_on = 0 < top_k < V, top_p < 1.0, min_p > 0.0
    e, comp = exp_row(x, T if T > 0 else 1.0)
    if T == 0 or not (k_on or p_on or m_on) or not comp.any():
        return RowResult(np.ones(V, dtype=bool), False, None, None, float("inf"))
    in_k = comp.copy()
    if k_on and top_k < comp.sum():
        t_k = np.sort(x[comp])[::-1][top_k - 1]
        in_k &= x >= t_k
    keep = in_k.copy()
    margin = float("inf")
    if p_on:
        vals = np.unique(x[in_k])[::-1]                        # distinct values, largest first
        per = _class_masses(x, e, in_k)                        # mass of each distinct value, same order
        cum = np.cumsum(per)                                   # cum[j] = mass(K, x >= vals[j])
        want = top_p * cum[-1]
        j = int(np.argmax(cum >= want))                        # first (= largest value) that reaches the target
        keep &= x >= vals[j]
        below = cum[j - 1] if j > 0 else 0.0
        margin = min(cum[j] - want, want - below) / want if want > 0 else float("inf")
    if m_on:
        keep &= e >= min_p
    keep &= comp
    return RowResult(keep, True, e, in_k, margin)


def _class_masses(x, e, in_k):
    order = np.argsort(-x[in_k], kind="stable")
    xs, es = x[in_k][order], e[in_k][order]
    starts = np.concatenate([[0], np.nonzero(xs[1:] != xs[:-1])[0] + 1])
    return np.add.reduceat(es, starts)


def renormalised(res: RowResult) -> np.ndarray:
    """The distribution a sampler draws from after the filter."""
    p = np.where(res.keep, res.e, 0.0)
    return p / p.sum()
