/*
 * libssdhip -- the compute-bound, LDS-tiled grouped expert GEMM over MXFP4 expert tables: the long-prefill sibling of
 * ssd_moe_gemm_mxfp4 (ssd_hip_moe_mxfp4.h), and ssd_moe_gemm_tiled (ssd_hip_moe_tiled.h) with other tables.
 *
 * Additive to ssd_hip_moe_tiled.h (the work unit, the grid, the token gather, both epilogues and every clamp are defined there) and to
 * ssd_hip_moe_mxfp4.h (the arguments and the "mx4 frag" tables are defined there).  Same conventions, error codes and ABI version as
 * ssd_hip.h.  ssd_moe_gemm_tiled_mxfp4 takes the arguments of ssd_moe_gemm_mxfp4 unchanged: q_frag E code tables [N/16][K/128][64][16 B],
 * s_frag E scale tables [N/16][K/128][16][4], both from ssd_mx4_rows_to_frag (gate_up with the row map that alternates gate / up
 * groups); offs / perm from ssd_moe_route; SSD_MOE_EPI_UP x [T][K] -> act [T k][N / 2], SSD_MOE_EPI_DOWN act [T k][K] -> d [T k][N].
 * Nothing about loaders or layouts changes, and there is still no dequantized copy of a table in memory.
 *
 * The launch is ssd_moe_gemm_tiled's: a workgroup owns one expert, a block of SSD_MOE_TILED_BM = 128 of its entries and a span of
 * SSD_MOE_TILED_BN = 128 table rows, and walks all of K in 64-deep stages through two LDS buffers (64 KiB, two workgroups per CU);
 * 2 x 2 waves; grid (floor(T k / 128) + E) * ceil(N / 128); surplus workgroups exit before any table access.  Only the weight operand
 * is staged differently.  The LDS-DMA cannot widen, so per 128-column unit each wave loads, for its two row groups, one 16-byte code
 * chunk and one 4-byte scale quad per lane (the A-operand loads of ssd_moe_gemm_mxfp4), widens them with v_cvt_scalef32_pk_bf16_fp4
 * ONCE PER WORKGROUP -- code words 0, 1 for the unit's first stage, words 2, 3 for its second -- and writes the k-tiles lane-linear
 * into the LDS slots that ssd_moe_gemm_tiled's DMA fills.  The next unit's codes are loaded ahead of the current stage's MFMAs.  A
 * weight byte is fetched and converted once per 128 entries (ssd_moe_gemm_mxfp4: once per 64 rows).
 *
 * ACCUMULATION ORDER (normative).  An output element is accumulated by ONE wave over the K / 32 k-tiles in ascending order, from +0 in
 * fp32, one v_mfma_f32_16x16x32_bf16 per k-tile on the exactly widened weights W = 2^(b - 127) * e2m1(q), and rounded once
 * (SSD_MOE_EPI_UP: g and u each, then silu(g) * u once, the arithmetic of ssd_silu_mul).  There is no K split and there are no
 * partial sums.  Two consequences:
 *   1. an entry's result depends on its own row of rows_in and its expert's table only: not on T, not on its place in a block, not on
 *      other tokens' routes;
 *   2. the output is bit-identical to ssd_moe_gemm_tiled over the bf16 image of the same tables (ssd_rows_to_frag of W, mode 1 for
 *      SSD_MOE_EPI_UP and mode 0 for SSD_MOE_EPI_DOWN).
 * It differs from ssd_moe_gemm_mxfp4's result, whose waves split K and add partial sums, by fp32 rounding.
 *
 * The contract of ssd_moe_gemm_tiled holds: no allocation, no synchronisation, a grid that depends on no device data
 * (hipGraph-capturable: a captured launch replays with other routes in the same buffers), one writer per output element, no atomics,
 * the same bits on every run.  Tables of experts without entries and rows of rows_in that no entry names are never read; nothing is
 * written past the T k entries; offs / perm values outside their ranges are clamped / skipped.
 *
 * Shapes: those of ssd_moe_gemm_mxfp4 -- 1 <= k <= 8 <= E <= 256, E % 8 == 0, k <= E; K % 128 == 0; SSD_MOE_EPI_UP: N % 64 == 0;
 * SSD_MOE_EPI_DOWN: N % 16 == 0; T >= 1 and T * k <= 2^24 -- and (floor(T k / 128) + E) * ceil(N / 128) < 2^31.
 * Refusals, before any launch: SSD_ERR_ARG for a null pointer the kernel would dereference or an unknown epilogue; SSD_ERR_SHAPE for
 * every shape outside the list above.
 */
#ifndef SSD_HIP_MOE_TILED_MXFP4_H
#define SSD_HIP_MOE_TILED_MXFP4_H
#include "ssd_hip_moe_tiled.h"
#include "ssd_hip_moe_mxfp4.h"
#ifdef __cplusplus
extern "C" {
#endif

int ssd_moe_gemm_tiled_mxfp4(const void* rows_in, const void* q_frag, const void* s_frag, const int32_t* offs, const int32_t* perm,
                             void* out, int T, int k, int E, int N, int K, int epilogue, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_MOE_TILED_MXFP4_H */
