/*
 * libssdhip -- per-token log-probabilities of the target's logit rows: log-sum-exp, the N most probable entries, and the
 * log-probability of the token a row produced.
 *
 * Additive to ssd_hip.h (same conventions, error codes and ABI version).  The log-probabilities are of the RAW distribution of a
 * row: log_softmax of the LM head's bf16 logits as they are, before penalties, logit bias, temperature and truncation (the
 * "raw logprobs" default of the vLLM / OpenAI interfaces).  ssd_logprob_rows therefore runs in front of ssd_penalize_rows and
 * ssd_filter_rows, which rewrite the rows in place, and can leave a bit-exact copy of the rows for the pick that follows them.
 *
 * For one row x[0..V) of bf16 logits, over its comparable (non-NaN) entries:
 *   m   = max x_i                         lse = m + log(sum_i exp(float(x_i) - m))                logprob_i = float(x_i) - lse
 *   top = the n = min(n_top, number of comparable entries) largest entries, in descending order of value, ties by lowest index
 * Edge rules (the family of ssd_hip_filter.h):
 *   - NaN is not comparable: it carries no mass and never appears in the top list; -0.0 and +0.0 are one value;
 *   - entries in [V, ld) are never read into a result;
 *   - a row whose maximum is not finite (+inf, or -inf: every comparable entry is -inf) has all of its mass on the maximum's class:
 *     lse = the maximum, every member of the class gets -log(count of the class), every other entry -inf;
 *   - a row with nothing comparable: lse = NaN and all top slots are -1 / -inf.
 * Sums are fp32.  A row is cut into slices of SSD_LOGPROB_SLICE entries; every thread of a slice adds its at most 16 terms in index
 * order, the 256 partials of a slice meet in a shuffle tree and a fixed-order sum over its 4 waves, and the slices of a row meet in a
 * shuffle tree of one wave.  No float atomics: the same row gives the same bits on every run, inside and outside a hipGraph, whatever
 * its alignment (16-byte loads when the row start allows them, 2-byte loads otherwise, with the same entries in the same threads).
 */
#ifndef SSD_HIP_LOGPROB_H
#define SSD_HIP_LOGPROB_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Largest count of most probable entries one row can return, and the row stride of top_val / top_id. */
#define SSD_LOGPROB_MAX_N 20
/* Entries per slice (one workgroup of 256 threads x 2 chunks of 8), and the largest vocabulary: 48 slices, one lane each in the merge. */
#define SSD_LOGPROB_SLICE 4096
#define SSD_LOGPROB_MAX_V 196608

/* Bytes of workspace ssd_logprob_rows needs for T rows of V entries (the per-slice maxima, sums and candidates), or SSD_ERR_SHAPE
 * for T or V <= 0, V > SSD_LOGPROB_MAX_V, or a size that does not fit an int. */
int ssd_logprob_rows_ws_bytes(int T, int V);

/* logits_rows: bf16 [T][ld], read only.  n_top: device int32 array with one entry per rows_per_param consecutive rows (1 for decode
 * rows, K+1 for verify rows), read by the kernel, so a captured graph replays with fresh values: -1 = the row is skipped and nothing of
 * its outputs is written, 0..SSD_LOGPROB_MAX_N = the number of top entries asked for (any other value is treated as -1).
 * Per row that is not skipped:
 *   lse[t]                      fp32, as above
 *   top_id[t][0..n), top_val[t][0..n)   int32 / fp32, row stride SSD_LOGPROB_MAX_N: index and log-probability of the n largest
 *                               entries; slots [n, n_top) get id -1 and value -inf; slots past n_top are untouched
 *   raw_copy[t][0..V)           (optional, bf16, row stride raw_ld) a bit-exact copy of the row; entries [V, raw_ld) are never written
 * top_val and top_id may be null only together (then only lse and the copy are produced).  ws: ssd_logprob_rows_ws_bytes(T, V) bytes,
 * 4-byte aligned.  SSD_ERR_SHAPE for T, V or rows_per_param <= 0, T > 65535, ld < V, V > SSD_LOGPROB_MAX_V, or raw_ld < V with a copy requested;
 * SSD_ERR_ARG for a null logits_rows, n_top, lse or ws, or for exactly one of top_val / top_id null. */
int ssd_logprob_rows(const void* logits_rows, long ld, int T, int V, const int32_t* n_top, int rows_per_param, float* lse,
                     float* top_val, int32_t* top_id, void* raw_copy, long raw_ld, void* ws, void* stream);

/* out[t] = float(rows[t][tokens[t]]) - lse[t], fp32 (an infinite row's maximum class gives inf - inf = NaN here; top_val has the
 * class's -log(count)).  rows: the raw rows -- the live ones, or the copy ssd_logprob_rows left.  tokens: int64 [T].  A token outside
 * [0, V) gives NaN; a row skipped by n_top (as above) is not written.  SSD_ERR_SHAPE for T, V or rows_per_param <= 0 or ld < V;
 * SSD_ERR_ARG for a null rows, tokens, lse, n_top or out. */
int ssd_logprob_pick(const void* rows, long ld, int T, int V, const int64_t* tokens, const float* lse, const int32_t* n_top,
                     int rows_per_param, float* out, void* stream);

/* The same over the B * (K+1) rows of a verify.  Row (b, j) holds the distribution that predicts position j + 1 of the round, so with
 * a = accept[b], the number of accepted draft tokens as ssd_verify_greedy / ssd_argmax_parts_verify / ssd_verify_ratio leave it (0..K;
 * the recovery token is not counted), its token is ids[b][j + 1] for j < a, recovery[b] for j == a, and none (out = NaN) for j > a.
 * ids: int64 [B][K+1] (the round's inputs), accept: int32 [B], recovery: int64 [B], n_top: one entry per sequence, out: fp32 [B][K+1].
 * SSD_ERR_SHAPE for B or V <= 0, K < 0 or ld < V; SSD_ERR_ARG for a null rows, ids, accept, recovery, lse, n_top or out. */
int ssd_logprob_pick_verify(const void* rows, long ld, int B, int K, int V, const int64_t* ids, const int32_t* accept,
                            const int64_t* recovery, const float* lse, const int32_t* n_top, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_LOGPROB_H */
