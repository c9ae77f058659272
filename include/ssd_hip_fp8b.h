/*
 * libssdhip -- block-scaled FP8 (OCP e4m3fn codes, one fp32 scale per block of rows and 128 columns): the form of the
 * `quant_method: "fp8"` checkpoints with `weight_block_size: [128, 128]` and a `weight_scale_inv` tensor per linear.
 *
 * Additive to ssd_hip.h and ssd_hip_quant.h (same conventions, error codes and ABI version).  A quantized matrix W[N][K]
 * (K % 64 == 0, N % 16 == 0) is
 *   q[N][K]         e4m3fn codes, and
 *   s[N/16][KB]     one fp32 scale per 16-row group and 128-column block, KB = ceil(K / 128),
 *                                                                    W = s[n / 16][k / 128] * q[n][k].
 * The last column block is half a block where K % 128 == 64.
 *
 * Device layout.  Codes: the "fp8 frag" layout of ssd_hip_quant.h, unchanged, written by ssd_fp8_rows_to_frag (with its row_map).
 * Scales: fp32 [N/16][KB], row-major, in the PACKED row order of the codes: entry (g, b) scales rows 16g .. 16g+15 of the frag and
 * columns 128b .. 128b+127.  All 16 rows of an MFMA tile share one scale, so a scale is uniform over a wave.  The granularity is
 * finer than the checkpoint's 128 rows on purpose: q | k | v and gate | up are concatenated from tensors with their own block
 * grids, the row maps move rows around, and grids may be ragged (ceil(N / 128) block rows); all of these reduce to "expand to one
 * scale row per output row, permute, take one per 16-row group" on the host.  The table is 4 bytes per 2 KiB of codes.
 *
 * Semantics of the GEMM (normative):
 *   y[m][n] = bf16(bias[n] + sum_b s[n / 16][b] * sum_{k in block b} q[n][k] * x[m][k]).
 * The inner sums are taken by the bf16 MFMA in fp32 from exactly converted codes (every e4m3 value is a bf16 value; the convert
 * instruction runs at scale 1.0).  The scale is an arbitrary positive fp32 and is multiplied in fp32: it is applied once per
 * 64-COLUMN UNIT (two MFMA k-steps into a zeroed fp32 temporary, then acc = fma(s, temporary, acc)), i.e. twice per full block with
 * the same scale, not once per 128-column block.  It is never folded into the convert instruction's scale operand.  The K order
 * is fixed by (K, nt's deep flag, waves) alone: the same input gives the same bits on every run and for every tiles-per-workgroup
 * value.
 */
#ifndef SSD_HIP_FP8B_H
#define SSD_HIP_FP8B_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bf16 frag [N][K] (ssd_hip.h layout, same row order) = bf16(s * q), the product in fp32: the weights of the bf16 prefill GEMMs
 * for prompts longer than the direct limit.  w_frag needs N*K*2 bytes. */
int ssd_fp8b_dequant_frag(const void* q_frag, const float* s_grp, void* w_frag, int N, int K, void* stream);

/* y = x . (s (.) q)^T for M <= 128 token rows, N % 16 == 0, K % 64 == 0: the contract of ssd_gemm_fp8 (epilogues SSD_EPI_ROWS and
 * SSD_EPI_SILU_FRAG, bias bf16 [N] or NULL, the same error codes) with s_grp the group table above.  Never allocates or
 * synchronises. */
int ssd_gemm_fp8b(const void* x_frag, const void* q_frag, const float* s_grp, const void* bias, void* y, int M, int N, int K, int ldy,
                  int epilogue, void* stream);
/* The same with an explicit decomposition; nt and waves are encoded as for ssd_gemm_fp8_cfg. */
int ssd_gemm_fp8b_cfg(const void* x_frag, const void* q_frag, const float* s_grp, const void* bias, void* y, int M, int N, int K,
                      int ldy, int epilogue, int nt, int waves, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_FP8B_H */
