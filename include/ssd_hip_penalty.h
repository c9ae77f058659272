/*
 * libssdhip -- repetition / presence / frequency penalties and logit bias on raw logit rows, in place, in front of ssd_filter_rows,
 * the samplers, ssd_row_lse, ssd_verify_ratio and argmax.
 *
 * Additive to ssd_hip.h (same conventions, error codes and ABI version).  This comment is the normative text.
 *
 * History of one logits row (the row predicts the token that follows everything the sequence has seen so far):
 *   in_prompt(t)   token t occurs in the prompt
 *   c(t)           how often t occurs among the tokens after the prompt that precede this row's prediction, the tokens speculated
 *                  earlier in the same round included
 *   seen(t)        in_prompt(t) or c(t) > 0
 * Per entry t of the row, with the sequence's r = repetition penalty (1 = off), p = presence penalty (0 = off), f = frequency
 * penalty (0 = off) and bias(t) (0 = none), every step in fp32 and rounded on its own (no fused multiply-add, IEEE division):
 *   1. x = float(bf16 logit)
 *   2. bias(t) != 0:   x = x + bias(t)
 *   3. seen(t):        x = (x < 0) ? x * r : x / r          (Hugging Face / vLLM: prompt and output tokens)
 *   4. c(t) > 0:       x = x - f * float(c(t)),  then  x = x - p          (OpenAI / vLLM: output tokens only)
 *   5. the result is stored as bf16, round to nearest even.
 * Entries that are neither seen nor biased keep their bits; entries in [V, ld) are never touched; history and bias ids outside
 * [0, V) are ignored.  A NaN logit keeps its bits; -inf stays -inf (r > 0; p, f and the biases are finite); should the arithmetic
 * itself produce a NaN (+inf minus an overflowed f * c) it is stored as the quiet NaN 0x7FC0.  A sequence with r = 1, p = 0, f = 0 and no
 * bias leaves its rows untouched bit for bit.  The order of the pipeline is penalties, temperature, truncation, draw.
 *
 * The history arrives sparse.  Sequence b has a table of tab_len[b] <= tab_ld entries with UNIQUE token ids (tab_len is clamped to
 * [0, tab_ld]):
 *   tab_ids [b][i]    token id
 *   tab_cnt [b][i]    (c << 1) | in_prompt       c counts the output tokens the host knows of
 *   tab_bias[b][i]    bias (0 = none)
 * and the tokens of the current round are read from device memory, so that a captured graph replays with fresh values:
 *   extra [b][0 .. extra_ld)   int64; entry 0 is the token fed to the sequence's first row of the round and is already in the table
 *   prefix form (extra_n == NULL)   row j of sequence b (j = row % rows_per_seq) also sees extra[b][1 .. j]: the K+1 input ids of a
 *                                   verify; row 0 sees none
 *   chain form  (extra_n != NULL)   every row of sequence b also sees extra[b][1 .. n], n = min(max(*extra_n, 0), extra_ld - 1): the
 *                                   speculation buffer and the step counter that ssd_draft_advance maintains
 * The extra tokens may repeat each other and may or may not be in the table: every distinct token is adjusted exactly once, with
 * c = table count + occurrences among the extras (an extra token is an output token).  Unique ids mean that no two threads write
 * the same entry; there are no atomics, and the same input gives the same bits on every run, inside and outside a hipGraph.
 */
#ifndef SSD_HIP_PENALTY_H
#define SSD_HIP_PENALTY_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Most extra tokens one row can see (extra_ld - 1). */
#define SSD_PENALTY_MAX_EXTRA 64

/* logits_rows: bf16 [T][ld], adjusted in place, one workgroup per row; rows_per_seq consecutive rows belong to one sequence (1 for
 * decode rows, K+1 for verify rows).  rep / pres / freq: fp32 device arrays with one entry per sequence.  The table (tab_ids,
 * tab_cnt, tab_bias, tab_len) is either given whole or null whole: a null table means "no history and no bias" (rows that only see
 * extra tokens).  extra may be null (no extra tokens; then extra_n must be null and extra_ld is ignored).
 * SSD_ERR_SHAPE for T, V or rows_per_seq <= 0, ld < V, a table with tab_ld <= 0, extra with extra_ld < 1 or
 * extra_ld - 1 > SSD_PENALTY_MAX_EXTRA, or the prefix form with extra_ld < rows_per_seq; SSD_ERR_ARG for a null logits_rows, rep,
 * pres or freq, a table given in part, or extra_n without extra. */
int ssd_penalize_rows(void* logits_rows, long ld, int T, int V, int rows_per_seq, const int32_t* tab_ids, const int32_t* tab_cnt,
                      const float* tab_bias, int tab_ld, const int32_t* tab_len, const float* rep, const float* pres,
                      const float* freq, const int64_t* extra, int extra_ld, const int32_t* extra_n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_PENALTY_H */
