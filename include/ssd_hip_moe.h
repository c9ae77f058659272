/*
 * libssdhip -- routed mixture-of-experts MLP (Qwen3-MoE): top-k routing, the grouped skinny GEMM over the experts' tables, and the
 * weighted combine.
 *
 * Additive to ssd_hip.h (same conventions, error codes and ABI version).  Every call takes raw device pointers and a stream, never
 * allocates and never synchronises; no grid depends on device data, so every launch is hipGraph-capturable and a captured graph
 * replays with other logits -- other routes -- in the same buffers.  No float atomics anywhere: the same input gives the same bits
 * on every run.
 *
 * The block (Qwen3MoeSparseMoeBlock of transformers).  For a token row x [K = hidden] with router logits l [E] (the router GEMM is
 * ssd_gemm_wf / ssd_gemm_pf with SSD_EPI_ROWS on mlp.gate.weight, bf16 rows):
 *   ids      = the k largest logits, larger first, ties to the lower expert index
 *   w[j]     = bf16(softmax(l)[ids[j]] / (norm ? sum_j softmax(l)[ids[j]] : 1)), widened to fp32
 *   act[j]   = bf16(silu(g) * u),  g = bf16(x . Wg[ids[j]]^T), u = bf16(x . Wu[ids[j]]^T)      (the arithmetic of ssd_silu_mul)
 *   d[j]     = bf16(act[j] . Wd[ids[j]]^T)
 *   h        = bf16(sum_j w[j] * float(d[j]))                                                   j ascending, fp32, one rounding
 * The residual add stays with the ssd_rmsnorm that follows, as after a dense down_proj.  This rounds LESS often than the bf16 module
 * of transformers, which multiplies every expert's output by its weight in bf16 and accumulates the k products into the bf16 result
 * with index_add_ (one rounding per product and one per addition); here the k products are summed in fp32 and rounded once.
 *
 * "Entry" p = t * k + j names choice j of token row t.  topk_ids, topk_w, act and d are indexed by entry.
 *
 * ssd_moe_route.  logits bf16 rows [T][ld], ld >= E; columns past E are never read.  Outputs:
 *   topk_ids int32 [T][k]; a NaN logit never wins against a number (a row of NaNs yields experts 0 .. k-1).
 *   topk_w   fp32  [T][k]: softmax over all E logits in fp32 (maximum subtracted, expf, the E terms summed lane-wise then by a
 *            butterfly -- a fixed order), the chosen probabilities divided by their sum (j ascending) when `norm`, rounded to bf16
 *            (transformers casts the routing weights to the hidden dtype) and widened.  Against the float64-exact value this
 *            differs by at most one bf16 ulp, and only where the exact value lies within ~1e-6 relative of a rounding boundary.
 *   offs     int32 [E + 1]: offs[e] = number of entries whose expert is below e; offs[E] = T * k.
 *   perm     int32 [T * k]: the entries grouped by expert, perm[offs[e] .. offs[e+1]) = the entries of expert e in ascending
 *            entry order.  The order comes from a scan (one workgroup per expert walks the T * k ids), never from atomics.
 *
 * ssd_moe_gemm.  w_frag holds E matrices [N][K], one after the other, each fragment-major (ssd_rows_to_frag); rows_in row-major.
 *   epilogue SSD_MOE_EPI_UP:   N = 2 I, tables from ssd_rows_to_frag mode 1 (16-row groups alternate gate / up), rows_in = x [T][K]
 *       read at row perm[i] / k, out = act rows [T * k][I = N / 2] at row perm[i].
 *   epilogue SSD_MOE_EPI_DOWN: N = H, tables mode 0, rows_in = act [T * k][K = I] read at row perm[i], out = d rows [T * k][N] at
 *       row perm[i], every element rounded to bf16 once.
 * A workgroup belongs to ONE expert and one span of output features (one gate / up pair of 16-row groups, or up to four 16-row
 * groups of the down table); it walks that expert's perm range 16 rows (one MFMA tile) at a time, so a tile never mixes experts and
 * only an expert's last tile is ragged.  An expert without entries costs one workgroup that exits.  Accumulation order (fixed):
 * the K / 32 k-tiles are dealt round-robin to the workgroup's 4 waves (wave v takes k-tiles v, v + 4, ...), each wave accumulates
 * its k-tiles in ascending order in fp32 on v_mfma_f32_16x16x32_bf16, and the 4 partial sums are added in wave order.  Every
 * output element has exactly one writer; rows of rows_in that no entry names are never read; tables of experts without entries are
 * never read; output rows are written for every entry (perm is a permutation of the entries), nothing else is.  offs / perm values
 * outside their ranges are clamped / skipped, so a bad table never addresses outside the buffers.
 *
 * ssd_moe_combine.  h rows [T][H] = bf16(sum_j topk_w[t][j] * float(d[t * k + j][:])), j ascending, every product and every sum
 * rounded to fp32 (no fused multiply-add), one final rounding.
 *
 * Shapes: 1 <= k <= 8 <= E <= 256, E % 8 == 0, k <= E; K % 32 == 0; epilogue UP: N % 64 == 0 (I % 32 == 0); epilogue DOWN:
 * N % 16 == 0; T >= 1 and T * k <= 2^24.
 * Refusals, before any launch: SSD_ERR_ARG for a null pointer the kernel would dereference or an unknown epilogue; SSD_ERR_SHAPE
 * for every shape outside the list above, and for ld < E.
 */
#ifndef SSD_HIP_MOE_H
#define SSD_HIP_MOE_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define SSD_MOE_EPI_UP 0
#define SSD_MOE_EPI_DOWN 1
#define SSD_MOE_MAX_K 8
#define SSD_MOE_MIN_E 8
#define SSD_MOE_MAX_E 256

int ssd_moe_route(const void* logits_rows, long ld, int T, int E, int k, int norm, int32_t* topk_ids, float* topk_w, int32_t* offs,
                  int32_t* perm, void* stream);

int ssd_moe_gemm(const void* rows_in, const void* w_frag, const int32_t* offs, const int32_t* perm, void* out, int T, int k, int E,
                 int N, int K, int epilogue, void* stream);

int ssd_moe_combine(const void* d_rows, const float* topk_w, void* h_rows, int T, int k, int H, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_MOE_H */
