"""ctypes table and torch front end of the per-request seed kernels (include/ssd_hip_seed.h): the Gumbel-max sampler and the ratio
verification drawing from a stream keyed by (seed, purpose, absolute position, index), and the hook that exposes that stream.

Kept apart from ``lib.SIGNATURES`` like the other additive headers (``filter_ops``, ``logprob_ops``, ...): it binds on the same
libssdhip.so.  Nothing here computes in torch; every call enqueues on the current stream and is hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

from .lib import bind, SsdHipError
from .ops import _p, _stream, _check

c_void_p, c_int, c_long, c_uint, c_float = C.c_void_p, C.c_int, C.c_long, C.c_uint, C.c_float

DRAFT, TARGET, ACCEPT = 1, 2, 3     # SSD_SEED_DRAFT / SSD_SEED_TARGET / SSD_SEED_ACCEPT
SLICE = 4096                        # SSD_SEED_SLICE

# name -> argtypes, exactly include/ssd_hip_seed.h
SEED_SIGNATURES = {
    "ssd_sample_seeded_ws_bytes": [c_int, c_int],
    "ssd_sample_rows_seeded": [c_void_p, c_long, c_int, c_int, c_void_p, c_int, c_void_p, c_uint, c_void_p, c_void_p, c_void_p, c_int,
                               c_float, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p],
    "ssd_verify_ratio_seeded": [c_void_p, c_long, c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_uint, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                c_void_p, c_void_p, c_void_p],
    "ssd_seeded_uniforms": [c_void_p, c_void_p, c_int, c_int, c_uint, c_int, c_void_p, c_void_p],
}

LAUNCHES = 0        # kernel-launching calls of this process (eager launches and graph captures; a replay launches without Python)


def load_seed_library():
    return bind(SEED_SIGNATURES, {"ssd_sample_seeded_ws_bytes": c_long})


def sample_seeded_ws_bytes(T: int, V: int) -> int:
    n = load_seed_library().ssd_sample_seeded_ws_bytes(T, V)
    if n < 0:
        raise SsdHipError(f"ssd_sample_seeded_ws_bytes({T}, {V}) failed with code {n}")
    return n


def sample_rows_seeded(logits, ld: int, T: int, V: int, temps, rows_per_temp: int, rng_state, salt: int, out, row_seed,
                       rows_per_seed: int, positions, purpose: int, ws, out2=None, boost_idx=None, boost_k: int = 0,
                       boost_x: float = 1.0) -> None:
    """ops.sample_rows with row_seed (int64, one per rows_per_seed rows, -1 = the engine's stream) and positions (int64 [T], of the
    rows' input tokens); ws: sample_seeded_ws_bytes(T, V) bytes."""
    global LAUNCHES
    LAUNCHES += 1
    _check(load_seed_library().ssd_sample_rows_seeded(_p(logits), ld, T, V, _p(temps), rows_per_temp, _p(rng_state), salt, _p(out),
                                                      _p(out2), _p(boost_idx), boost_k, boost_x, _stream(), _p(row_seed), rows_per_seed,
                                                      _p(positions), purpose, _p(ws)), "ssd_sample_rows_seeded")


def verify_ratio_seeded(logits_p, ld_p: int, logits_q, ld_q: int, V: int, B: int, K: int, spec, preds_p, lse_p, lse_q, temps_t, temps_q,
                        ratio_rows, rng_state, salt: int, accept_len, recovery, row_seed, positions, packed=None, accept_prob=None,
                        boost_idx_q=None, boost_k: int = 0, boost_x: float = 1.0) -> None:
    """ops.verify_ratio with row_seed (int64 [B], -1 = the engine's stream) and positions (int64 [B][K+1], of the verify's inputs)."""
    global LAUNCHES
    LAUNCHES += 1
    _check(load_seed_library().ssd_verify_ratio_seeded(_p(logits_p), ld_p, _p(logits_q), ld_q, V, B, K, _p(spec), _p(preds_p), _p(lse_p),
                                                       _p(lse_q), _p(temps_t), _p(temps_q), _p(ratio_rows), _p(rng_state), salt,
                                                       _p(accept_len), _p(recovery), _p(packed), _p(accept_prob), _p(boost_idx_q),
                                                       boost_k, boost_x, _stream(), _p(row_seed), _p(positions)),
           "ssd_verify_ratio_seeded")


def seeded_uniforms(row_seed, positions, rows: int, purpose: int, idx0: int, n: int, out) -> None:
    """out fp32 [rows][n] = u(row_seed[r], purpose, positions[r] + 1, idx0 + j); NaN rows for negative seeds."""
    global LAUNCHES
    LAUNCHES += 1
    _check(load_seed_library().ssd_seeded_uniforms(_p(row_seed), _p(positions), rows, purpose, idx0, n, _p(out), _stream()),
           "ssd_seeded_uniforms")
