/*
 * libssdhip -- the compute-bound, LDS-tiled grouped expert GEMM over block-scaled FP8 expert tables: the long-prefill sibling of
 * ssd_moe_gemm_fp8b (ssd_hip_moe_fp8b.h), and ssd_moe_gemm_tiled (ssd_hip_moe_tiled.h) with other tables.
 *
 * Additive to ssd_hip_moe_tiled.h (the work unit, the grid, the token gather, both epilogues and every clamp are defined there) and to
 * ssd_hip_moe_fp8b.h (the arguments, the "fp8 frag" code tables and the per-group scale tables are defined there).  Same conventions,
 * error codes and ABI version as ssd_hip.h.  ssd_moe_gemm_tiled_fp8b takes the arguments of ssd_moe_gemm_fp8b unchanged: q_frag E
 * code tables [N/16][K/64][64 lanes][16 B], s_grp fp32 [E][N/16][K/128] in the packed row order of the codes; offs / perm from
 * ssd_moe_route; SSD_MOE_EPI_UP x [T][K] -> act [T k][N / 2], SSD_MOE_EPI_DOWN act [T k][K] -> d [T k][N].
 * W = s[n / 16][k / 128] * e4m3(q[n][k]) with s an arbitrary positive fp32.  Nothing about loaders or layouts changes, and there is
 * still no dequantized copy of a table in memory.
 *
 * The launch is ssd_moe_gemm_tiled's: a workgroup owns one expert, a block of SSD_MOE_TILED_BM = 128 of its entries and a span of
 * SSD_MOE_TILED_BN = 128 table rows, and walks all of K in 64-deep stages through two LDS buffers (64 KiB, two workgroups per CU);
 * 2 x 2 waves; grid (floor(T k / 128) + E) * ceil(N / 128); surplus workgroups exit before any table access.  Two things differ.
 * The weight stage: the LDS-DMA cannot widen, and one 1 KiB code tile (16 rows x 64 columns) is exactly one stage of one row group,
 * so per stage each wave loads ONE 16-byte code chunk per lane for each of its two row groups, widens it exactly (the convert
 * instruction runs at scale 1.0) ONCE PER WORKGROUP -- code words 0, 1 are the stage's first k-tile, words 2, 3 its second -- and
 * writes the two k-tiles lane-linear into the LDS slots that ssd_moe_gemm_tiled's DMA fills.  The next stage's codes are in flight
 * while the current one multiplies.  A weight byte is fetched and converted once per 128 entries (ssd_moe_gemm_fp8b: once per 64
 * rows).  The scale: one fp32 per (16-row group, block), uniform over the wave that owns the group, read as such one block ahead and
 * applied to a partial sum in fp32 -- never to the weights, never through the convert instruction's scale operand.
 *
 * ACCUMULATION ORDER (normative).  An output element is accumulated by ONE wave over all of K; there is no K split.  With the stages
 * j = 0 .. K / 64 - 1 in ascending order and an fp32 accumulator that starts at +0:
 *   1. an fp32 temporary starts at +0;
 *   2. it takes the k-tiles 2 j, then 2 j + 1, one v_mfma_f32_16x16x32_bf16 each (the instruction's own order over the 32 columns)
 *      from the exactly converted codes;
 *   3. accumulator = fma(s[n / 16][j / 2], temporary, accumulator), one fused multiply-add in fp32: both stages of a block take the
 *      block's scale;
 *   4. after the last stage the accumulator is rounded to bf16 once (SSD_MOE_EPI_DOWN), or g and u are and silu(g) * u is rounded
 *      once more (SSD_MOE_EPI_UP, the arithmetic of ssd_silu_mul).
 * An output element depends on its own rows_in row, its own table row and scales and K only: never on T, on the routes, on its place
 * in a block or on its neighbours.  The same entry row gives the same bits alone (T = 1) and inside a prefill of any length.
 * This is the per-64-column partial-sum order of the dense block-scaled GEMM, not the per-128-column, K-split order of
 * ssd_moe_gemm_fp8b: the two expert kernels agree to fp32 rounding, not by bits.
 *
 * The contract of ssd_moe_gemm_tiled holds: no allocation, no synchronisation, a grid that depends on no device data
 * (hipGraph-capturable: a captured launch replays with other routes in the same buffers), one writer per output element, no atomics,
 * the same bits on every run.  Tables of experts without entries and rows of rows_in that no entry names are never read; nothing is
 * written past the T k entries; offs / perm values outside their ranges are clamped / skipped.  Row groups past the table in the
 * last span read the last group's codes and scales and are never stored.
 *
 * Shapes: those of ssd_moe_gemm_fp8b -- 1 <= k <= 8 <= E <= 256, E % 8 == 0, k <= E; K % 128 == 0; SSD_MOE_EPI_UP: N % 64 == 0;
 * SSD_MOE_EPI_DOWN: N % 16 == 0; T >= 1 and T * k <= 2^24 -- and (floor(T k / 128) + E) * ceil(N / 128) < 2^31.
 * Refusals, before any launch: SSD_ERR_ARG for a null pointer the kernel would dereference or an unknown epilogue; SSD_ERR_SHAPE for
 * every shape outside the list above.
 */
#ifndef SSD_HIP_MOE_TILED_FP8B_H
#define SSD_HIP_MOE_TILED_FP8B_H
#include "ssd_hip_moe_tiled.h"
#include "ssd_hip_moe_fp8b.h"
#ifdef __cplusplus
extern "C" {
#endif

int ssd_moe_gemm_tiled_fp8b(const void* rows_in, const void* q_frag, const float* s_grp, const int32_t* offs, const int32_t* perm,
                            void* out, int T, int k, int E, int N, int K, int epilogue, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_MOE_TILED_FP8B_H */
