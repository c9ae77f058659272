/*
 * libssdhip -- hard token constraints on raw logit rows, in place, beside ssd_penalize_rows and in front of the temperature,
 * ssd_filter_rows, the samplers, ssd_row_lse, ssd_verify_ratio and argmax: an allow mask over the vocabulary, a minimum length (stop
 * tokens that cannot be generated yet) and banned words (the Hugging Face NoBadWordsLogitsProcessor rule).
 *
 * Additive to ssd_hip.h (same conventions, error codes and ABI version).  This comment is the normative text.
 *
 * logits_rows is bf16 [T][ld]; rows_per_seq consecutive rows belong to one sequence b = row / rows_per_seq (1 for decode rows, K+1 for
 * verify rows).  A BANNED entry t in [0, V) becomes -inf (bits 0xFF80) whatever it held, a NaN included.  Every other entry keeps its
 * bits: all of [V, ld), NaNs, and every row of a sequence with nothing switched on.  Ids outside [0, V) in any list ban nothing.
 *
 * The context of a row (the row predicts the token that follows it) is the host tail followed by the extras the row sees:
 *   tail [b][0 .. tail_len[b])      int32, oldest first: the last tail_len[b] tokens the host knows of the sequence (prompt and
 *                                   output), ENDING with the token fed to the sequence's first row of the round; tail_len is clamped
 *                                   to [0, tail_ld]
 *   extra[b][0 .. extra_ld)         int64, exactly the buffer of ssd_penalize_rows: entry 0 is the token fed to the first row (it is
 *                                   already the tail's last token) and
 *     prefix form (extra_n == NULL)   row j of sequence b (j = row % rows_per_seq) also sees extra[b][1 .. j]; row 0 sees none
 *     chain form  (extra_n != NULL)   every row of sequence b also sees extra[b][1 .. n], n = min(max(*extra_n, 0), extra_ld - 1)
 *   Without extra no row sees any.  With e the number of extras a row sees (they are output tokens), entry t of the row is banned
 *   if (a), (b) or (c) holds:
 *
 *   (a) allow mask      allow_on[b] != 0 and bit (t & 31) of allow_bits[b][t >> 5] is 0.  allow_bits is uint32 [B][ceil(V / 32)]; bits
 *                       at or past V in the last word are ignored.
 *   (b) minimum length  e < min_left[b] and t is one of stop_ids[b][0 .. stop_len[b]).  min_left is max(0, min_tokens - output tokens
 *                       in front of the sequence's first row); stop_ids is int32 [B][SSD_CONSTRAIN_MAX_STOP] and holds the stop
 *                       tokens of the sequence, the EOS among them unless the sequence ignores it; stop_len is clamped to
 *                       [0, SSD_CONSTRAIN_MAX_STOP].
 *   (c) bad words       t is the LAST token of a bad word of length L, and either L == 1, or the context has at least L - 1 tokens
 *                       and its last L - 1 tokens equal the word's first L - 1 (compared as integers; the match may lie wholly in
 *                       the tail, wholly in the extras, or across the boundary).  Words arrive flattened: word w of sequence b is
 *                       bw_tok[b][bw_off[b][w] .. bw_off[b][w + 1]), w < bw_n[b]; bw_tok is int32 [B][SSD_CONSTRAIN_MAX_WORD_TOKENS],
 *                       bw_off int32 [B][SSD_CONSTRAIN_MAX_WORDS + 1], bw_n is clamped to [0, SSD_CONSTRAIN_MAX_WORDS].  A word
 *                       whose offsets leave [0, SSD_CONSTRAIN_MAX_WORD_TOKENS] or whose length is outside
 *                       [1, SSD_CONSTRAIN_MAX_WORD_LEN] bans nothing.  A word longer than tail_ld + 1 can only match through extras:
 *                       the host keeps tail_ld = SSD_CONSTRAIN_MAX_WORD_LEN - 1.
 *
 * Nothing guards a row whose every entry ends up banned (bad words can exhaust a small allow set dynamically): that is the caller's
 * error.  All per-round values -- masks, lists, tail, extras, *extra_n -- are read from device memory when the kernel runs, so a
 * captured graph replays with fresh data.  Every entry has exactly one writing thread and there are no atomics: the same input gives
 * the same bits on every run, inside and outside a hipGraph.  -inf stays -inf under ssd_penalize_rows (finite penalties and biases),
 * so the order of the two calls does not matter.
 */
#ifndef SSD_HIP_CONSTRAIN_H
#define SSD_HIP_CONSTRAIN_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Most extra tokens one row can see (extra_ld - 1); the bound of SSD_PENALTY_MAX_EXTRA. */
#define SSD_CONSTRAIN_MAX_EXTRA 64
/* Stop ids per sequence (the EOS included), and the row stride of stop_ids. */
#define SSD_CONSTRAIN_MAX_STOP 64
/* Bad words per sequence (bw_off has one more entry per row). */
#define SSD_CONSTRAIN_MAX_WORDS 128
/* Tokens of all bad words of one sequence, and the row stride of bw_tok. */
#define SSD_CONSTRAIN_MAX_WORD_TOKENS 1024
/* Longest bad word; tail_ld is at most one less. */
#define SSD_CONSTRAIN_MAX_WORD_LEN 16
/* Entries of a row one workgroup handles (grid: slices x rows). */
#define SSD_CONSTRAIN_SLICE 4096

/* Four optional groups, each given whole or null whole:
 *   allow mask   allow_on, allow_bits
 *   stop list    min_left, stop_ids, stop_len
 *   bad words    bw_tok, bw_off, bw_n, tail, tail_len (with tail_ld)
 *   extras       extra (with extra_ld) and, for the chain form, extra_n
 * A null group is switched off for every sequence; with all of them null the call launches and changes nothing.
 * SSD_ERR_SHAPE for T, V or rows_per_seq <= 0, T > 65535, ld < V, bad words with tail_ld < 1 or
 * tail_ld > SSD_CONSTRAIN_MAX_WORD_LEN - 1, extra with extra_ld < 1 or extra_ld - 1 > SSD_CONSTRAIN_MAX_EXTRA, or the prefix form
 * with extra_ld < rows_per_seq; SSD_ERR_ARG for a null logits_rows, a group given in part, or extra_n without extra. */
int ssd_constrain_rows(void* logits_rows, long ld, int T, int V, int rows_per_seq, const int32_t* allow_on, const uint32_t* allow_bits,
                       const int32_t* min_left, const int32_t* stop_ids, const int32_t* stop_len, const int32_t* bw_tok,
                       const int32_t* bw_off, const int32_t* bw_n, const int32_t* tail, int tail_ld, const int32_t* tail_len,
                       const int64_t* extra, int extra_ld, const int32_t* extra_n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_CONSTRAIN_H */
