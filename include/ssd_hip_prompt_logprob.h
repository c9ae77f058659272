/*
 * libssdhip -- log-probabilities of rows whose token is known before the row is read (the prompt rows of a prefill): log-sum-exp, the N
 * most probable entries, the known token's log-probability and its rank, in one pass over the row.
 *
 * Additive to ssd_hip.h and ssd_hip_logprob.h (same conventions, error codes and ABI version; SSD_LOGPROB_MAX_N, SSD_LOGPROB_SLICE and
 * SSD_LOGPROB_MAX_V are that header's).  A decode row's token is chosen after the row is read, so ssd_logprob_rows is followed by
 * ssd_logprob_pick; a prompt row's token is the next prompt token, so the slice that reads the row can also count the entries that
 * are at least as large as the token's, and the row is read once.
 *
 * For one row x[0..V) of bf16 logits and its token k, over the row's comparable (non-NaN) entries:
 *   lse, top     as ssd_logprob_rows defines them, edge rules included (NaN is not comparable, [V, ld) is never read into a result, rows
 *                with an infinite maximum and rows with nothing comparable), and bit-identical to what ssd_logprob_rows writes
 *   out          float(x_k) - lse, bit-identical to ssd_logprob_pick; NaN for k outside [0, V)
 *   rank         the number of comparable entries i in [0, V) with x_i >= x_k, the token itself included (vLLM's definition): a unique
 *                maximum has rank 1, two tied maxima both have rank 2, a -inf token has the number of comparable entries;
 *                -0.0 == +0.0; 0 when k is outside [0, V) or x_k is NaN
 * The rank is a sum of integer counts, one per slice, so it is exact; like the sums of ssd_logprob_rows it uses no atomics and is the
 * same on every run, inside and outside a hipGraph, whatever the row's alignment.
 */
#ifndef SSD_HIP_PROMPT_LOGPROB_H
#define SSD_HIP_PROMPT_LOGPROB_H
#include "ssd_hip_logprob.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace ssd_logprob_rows_known needs for T rows of V entries (one record per slice, as ssd_logprob_rows_ws_bytes), or
 * SSD_ERR_SHAPE for T or V <= 0, V > SSD_LOGPROB_MAX_V, or a size that does not fit an int. */
int ssd_logprob_known_ws_bytes(int T, int V);

/* logits_rows: bf16 [T][ld], read only.  n_top: device int32 [T], one entry per ROW, read by the kernel: -1 (or anything outside
 * 0..SSD_LOGPROB_MAX_N) = the row is skipped and nothing of its outputs is written, 0..SSD_LOGPROB_MAX_N = the number of top entries.
 * tokens: device int64 [T], the token row t must score; the entry of a skipped row is NOT read.  Per row that is not skipped:
 *   lse[t], top_id[t][0..n_top), top_val[t][0..n_top)   as ssd_logprob_rows (row stride SSD_LOGPROB_MAX_N; slots past n_top untouched)
 *   out[t]                      fp32, the token's log-probability as above
 *   rank[t]                     int32, the token's rank as above
 * top_val and top_id may be null only together (then lse, out and rank are produced).  ws: ssd_logprob_known_ws_bytes(T, V) bytes,
 * 4-byte aligned.  SSD_ERR_SHAPE for T or V <= 0, T > 65535, ld < V or V > SSD_LOGPROB_MAX_V; SSD_ERR_ARG for a null logits_rows, n_top,
 * tokens, lse, out, rank or ws, or for exactly one of top_val / top_id null. */
int ssd_logprob_rows_known(const void* logits_rows, long ld, int T, int V, const int32_t* n_top, const int64_t* tokens, float* lse,
                           float* top_val, int32_t* top_id, float* out, int32_t* rank, void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_PROMPT_LOGPROB_H */
