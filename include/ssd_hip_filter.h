/*
 * libssdhip -- top-k / top-p / min-p truncation of sampled logit rows, in place, in front of ssd_sample_rows, ssd_row_lse and
 * ssd_verify_ratio.
 *
 * Additive to ssd_hip.h (same conventions, error codes and ABI version).  For one row x[0..V) of bf16 logits with temperature
 * T > 0 (Hugging Face order: after the temperature):  s_i = float(x_i) / T,  m = max s_i,  e_i = exp(s_i - m).  The kept set is
 * K & P & M with
 *   K (top_k; 0 or >= V = off)   {i : x_i >= t_k},  t_k = the k-th largest value of the row (ties at t_k are all kept)
 *   P (top_p; 1.0 = off)         {i : x_i >= t_p},  t_p = the largest value v with sum_{i in K, x_i >= v} e_i >= top_p * sum_{i in K} e_i
 *   M (min_p; 0.0 = off)         {i : e_i >= min_p}
 * All three are "value >= threshold", so the result is an upper set of the row's values, and the class of the maximum is always in it.
 * Dropped entries are overwritten with -inf (bf16 0xFF80); kept entries keep their bits; entries in [V, ld) are never touched.
 * -inf needs nothing downstream: ssd_sample_rows never picks it, ssd_row_lse adds exp(-inf) = 0, ssd_verify_ratio sees p = 0.
 *   - a row whose temperature is 0, or whose three parameters are all off, is left untouched bit for bit (kept = V);
 *   - NaN is not comparable: it is not counted, carries no mass and is dropped; a row with nothing comparable is left as it is
 *     (kept = V); -0.0 and +0.0 are one value;
 *   - a row whose maximum is not finite has all of its mass on the maximum's class: P and M keep exactly that class.
 * top_k uses integer counts and is exact.  The masses are fp32: every thread sums at most 192 terms, the 1024 partials meet in a
 * fixed-order tree, so the result is the same bits on every run, inside and outside a hipGraph, whatever the row's alignment.
 */
#ifndef SSD_HIP_FILTER_H
#define SSD_HIP_FILTER_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Largest vocabulary ssd_filter_rows accepts: 1024 threads x 24 chunks of 8 logits (the 192 terms per thread above). */
#define SSD_FILTER_MAX_V 196608

/* logits_rows: bf16 [T][ld], filtered in place, one workgroup per row.  temps / top_k / top_p / min_p: device arrays with one entry
 * per rows_per_param consecutive rows (the convention of rows_per_temp: 1 for decode rows, K+1 for verify rows, MQ_LEN for tree
 * rows), read by the kernel, so a captured graph replays with fresh values.  kept (optional, int32 [T]): number of entries of the
 * kept set per row.  SSD_ERR_SHAPE for T, V or rows_per_param <= 0, ld < V or V > SSD_FILTER_MAX_V; SSD_ERR_ARG for a null
 * logits_rows, temps, top_k, top_p or min_p. */
int ssd_filter_rows(void* logits_rows, long ld, int T, int V, const float* temps, const int32_t* top_k, const float* top_p,
                    const float* min_p, int rows_per_param, int32_t* kept, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_FILTER_H */
