"""float64 numpy restatement of include/ssd_hip_prompt_logprob.h: what ssd_logprob_rows_known computes for one row and its known token
(the tests' reference; nothing here is on a product path).  lse, the top list and the token's log-probability are tests/logprob_ref.py's;
this adds the rank."""
from typing import NamedTuple

import numpy as np

from tests import logprob_ref as R

MAX_N = R.MAX_N


def rank(x, token: int) -> int:
    """The number of comparable (non-NaN) entries i with x_i >= x_token, the token itself included: a unique maximum has rank 1, two
    tied maxima both 2, a -inf token the number of comparable entries; -0.0 == +0.0.  0 for a token outside [0, V) or a NaN entry."""
    x = np.asarray(x, dtype=np.float64)
    if token < 0 or token >= len(x) or np.isnan(x[token]):
        return 0
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(x >= x[token]))         # NaN >= anything is False


class Known(NamedTuple):
    row: R.Row
    logprob: float      # NaN for a token outside [0, V)
    rank: int


def known_row(x, token: int, n_top: int = 0) -> Known:
    row = R.logprob_row(x, n_top)
    return Known(row, R.pick(x, token, row.lse), rank(x, token))


# The prompts of tests/test_engine_prompt_logprob_gpu.py, (a, b, n) -> [(a * j + b) % 128 for j in range(n)]: the family of
# tests/test_engine_logprob_gpu.py, chosen as that file chose its six.  `profiles/prompt_logprob_probe.py rows --grid` prefills 64
# prompts of the family in the engine's batches (8 prompts, 108 rows: a batch's row count decides which GEMMs run) on the decoder
# alone, none of the log-probability code running: the top-5 list of its logits, sorted on the host, is not the oracle's at 14 of
# 800 prompt positions (1.75 %; prompt by prompt instead of batched, over another 40: 25 of 856), with logit errors up to 0.125
# (0.31 on one 33-token prompt of the unbatched grid, which is not used).  These ten are prompts at which the decoder ranks the
# oracle's top 5 alike at every prompt position; the last two are the 21- and 13-token prompts of the chunking test, ENGINE_LONG spans
# two full KV blocks of 16.
ENGINE_PROMPTS_ABN = [(3, 1, 9), (5, 5, 9), (9, 3, 9), (3, 2, 13), (9, 4, 13), (5, 2, 13), (5, 7, 21), (5, 4, 21), (9, 4, 21), (9, 2, 13)]
ENGINE_PROMPTS = [[(a * j + b) % 128 for j in range(n)] for a, b, n in ENGINE_PROMPTS_ABN]
ENGINE_LONG_ABN = (3, 6, 36)
ENGINE_LONG = [(3 * j + 6) % 128 for j in range(36)]
