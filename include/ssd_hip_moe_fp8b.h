/*
 * libssdhip -- the grouped skinny GEMM of the routed mixture-of-experts MLP over block-scaled FP8 expert tables.
 *
 * Additive to ssd_hip_moe.h (the block, the entries, offs / perm and the two epilogues are defined there) and to ssd_hip_fp8b.h
 * (the format, its "fp8 frag" code layout and its per-group scale table are defined there).  Same conventions, error codes and ABI
 * version as ssd_hip.h.
 *
 * ssd_moe_gemm_fp8b is ssd_moe_gemm with other tables.  q_frag holds E code tables one after the other, expert e at byte
 * e * N * K, each [N/16][K/64][64 lanes][16 B] (fp8 frag, from ssd_fp8_rows_to_frag, one call per expert; for SSD_MOE_EPI_UP the
 * call carries the row map that makes the 16-row groups alternate gate / up).  s_grp holds E scale tables one after the other,
 * expert e at float e * (N/16) * (K/128), each fp32 [N/16][K/128] in the packed row order of the codes: the per-group table of
 * ssd_hip_fp8b.h.  W = s[n / 16][k / 128] * e4m3(q[n][k]) with s an arbitrary positive fp32, and
 *   SSD_MOE_EPI_UP:   N = 2 I, rows_in = x [T][K] read at row perm[i] / k, out = act rows [T * k][I] at row perm[i],
 *                     act = bf16(silu(g) * u), g and u rounded to bf16 first (the arithmetic of ssd_silu_mul);
 *   SSD_MOE_EPI_DOWN: N = H, rows_in = act [T * k][K = I] read at row perm[i], out = d rows [T * k][N] at row perm[i], every element
 *                     rounded to bf16 once.
 * There is no dequantized copy of a table anywhere: every T, long prefills included, reads the codes and the scales.
 *
 * The launch.  A workgroup belongs to ONE expert and one span of output features (one gate / up pair of 16-row groups, or up to
 * four 16-row groups of a down table); it walks that expert's perm range 16 rows (one MFMA tile) at a time, up to four tiles per pass,
 * so a tile never mixes experts and only an expert's last tile is ragged.  An expert without entries costs one workgroup that exits
 * before it reads anything of its tables.  A lane's A operand of a 128-column block is two 16-byte loads of codes, widened exactly
 * (the convert instruction runs at scale 1.0) into four v_mfma_f32_16x16x32_bf16 k-steps; the block's scale is uniform over the wave
 * and is read as such; the B operand is gathered from the row-major activations.  An expert with more than 64 rows takes one pass
 * per 64 rows and reads and converts its codes once per pass.
 *
 * ACCUMULATION ORDER (normative).  Let B = K / 128 blocks and W = 4 waves if B >= 8, else W = 2.  W depends on K alone.
 *   1. Wave v (0 <= v < W) owns the blocks v, v + W, v + 2 W, ... below B.
 *   2. Its fp32 accumulator starts at +0 and takes its blocks in ascending order.  Block c: an fp32 temporary starts at +0 and
 *      takes the four k-tiles 4c, 4c + 1, 4c + 2, 4c + 3 in that order, one v_mfma_f32_16x16x32_bf16 each (the instruction's own
 *      order over the 32 columns) from the exactly converted codes; then accumulator = fma(s[n / 16][c], temporary, accumulator),
 *      one fused multiply-add in fp32.  The scale is never folded into the convert instruction's scale operand.
 *   3. The W partial sums are added in fp32 in wave order, ((p0 + p1) + p2) + p3; a wave without a block contributes +0.
 *   4. The sum is rounded to bf16 once (DOWN), or g and u are and silu(g) * u is rounded once more (UP).
 * An output element depends on its own rows_in row, its own table row and scales and K only: never on T, on the routes, on the other
 * rows of its tile, on the number of tiles per pass or on the span width.  The same entry row gives the same bits alone (T = 1) and
 * inside a prefill of any length.
 *
 * Every output element has exactly one writer and there are no atomics; nothing is allocated or synchronised; no grid depends on
 * device data (grid = spans x E), so the launch is hipGraph-capturable and a captured graph replays with other routes in the same
 * buffers.  Rows of rows_in that no entry names are never read; tables of experts without entries are never read; output rows are
 * written for every entry and nothing else is.  offs / perm values outside their ranges are clamped / skipped, so a bad table never
 * addresses outside the buffers.
 *
 * Shapes: those of ssd_moe_gemm_mxfp4 (1 <= k <= 8 <= E <= 256, E % 8 == 0, k <= E, T >= 1, T * k <= 2^24; K % 128 == 0;
 * UP: N % 64 == 0; DOWN: N % 16 == 0).
 * Refusals, before any launch: SSD_ERR_ARG for a null pointer the kernel would dereference or an unknown epilogue; SSD_ERR_SHAPE for
 * every shape outside the list above.
 */
#ifndef SSD_HIP_MOE_FP8B_H
#define SSD_HIP_MOE_FP8B_H
#include "ssd_hip_moe.h"
#include "ssd_hip_fp8b.h"
#ifdef __cplusplus
extern "C" {
#endif

int ssd_moe_gemm_fp8b(const void* rows_in, const void* q_frag, const float* s_grp, const int32_t* offs, const int32_t* perm,
                      void* out, int T, int k, int E, int N, int K, int epilogue, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_MOE_FP8B_H */
