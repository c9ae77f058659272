/*
 * libssdhip -- the grouped expert GEMM of a routed mixture-of-experts MLP in its compute-bound, LDS-tiled form: the long-prefill
 * sibling of ssd_moe_gemm (ssd_hip_moe.h).
 *
 * Additive to ssd_hip_moe.h (same conventions, error codes, ABI version, epilogue constants and shape limits).  ssd_moe_gemm_tiled
 * takes the arguments of ssd_moe_gemm unchanged and computes the same thing from the same tables:
 *   w_frag    E matrices [N][K], one after the other, each fragment-major (ssd_rows_to_frag; mode 1 for SSD_MOE_EPI_UP: 16-row groups
 *             alternate gate / up; mode 0 for SSD_MOE_EPI_DOWN)
 *   offs/perm the grouping tables of ssd_moe_route
 *   SSD_MOE_EPI_UP    rows_in = x [T][K] read at row perm[i] / k, out = act rows [T * k][N / 2] at row perm[i]:
 *                     bf16(silu(g) * u) on the bf16-rounded g and u, with the arithmetic of ssd_silu_mul
 *   SSD_MOE_EPI_DOWN  rows_in = act [T * k][K] read at row perm[i], out = d rows [T * k][N] at row perm[i], every element rounded to
 *                     bf16 once
 * It never allocates and never synchronises; its grid depends on no device data (hipGraph-capturable: a captured launch replays
 * with other routes in the same buffers); one writer per output element, no atomics, the same bits on every run.
 *
 * Where ssd_moe_gemm streams an expert's weights once per 64 rows and splits K over its waves, this kernel is an LDS-tiled MFMA GEMM
 * per (expert, block of BM entries, span of BN table rows):
 *   work unit   a workgroup owns one expert e, entries perm[offs[e] + b BM .. + BM) of it (only an expert's last block is ragged) and
 *               BN consecutive table rows -- whole gate / up pairs for SSD_MOE_EPI_UP, so the epilogue finishes in the workgroup.
 *               It walks ALL of K in stages of 64 (two k-tiles; the last stage of an odd K / 32 holds one).
 *   operands    per stage every 1 KiB fragment tile of the span and every 16-row token tile of the block is copied ONCE into LDS by
 *               LDS-DMA (16 bytes per lane) in MFMA operand order, double-buffered, one barrier per stage; every wave reads its
 *               operands from LDS.  The token tile is a gather: lane l copies 16 bytes of its entry's row (column 32 kt + 8 (l >> 4)).
 *               The weight copy is a step of its own (a later format can widen codes there).  Token tiles without an entry are
 *               neither copied nor multiplied; in an expert's ragged last tile the columns past the last entry repeat that entry's
 *               row (a token row only ever influences its own column of the MFMA result, and those columns are never stored).
 *               So a weight byte serves BM token rows per fetch and a token byte BN table rows (ssd_moe_gemm: 64 and 32).
 *   grid        floor(T k / BM) + E blocks (an upper bound of sum_e ceil(n_e / BM) that the host can compute) times ceil(N / BN)
 *               spans, one dimension.  Every wave finds its (e, b) from offs (E + 1 <= 257 integers, one wave-wide prefix sum);
 *               surplus workgroups exit before they touch a table.  Workgroup ids are remapped so that consecutive (block, span)
 *               ids -- blocks fastest: the blocks that share an expert's span -- run on one XCD and share its L2.
 *
 * Accumulation order (normative).  An output element is accumulated by ONE wave on v_mfma_f32_16x16x32_bf16 over the K / 32 k-tiles
 * in ascending order from +0 in fp32 and rounded once (SSD_MOE_EPI_UP: g and u each, then the product once).  There is no K split and
 * no partial sum.  An entry's result therefore depends only on its own row of rows_in and its expert's table: not on T, not on the
 * entry's place in a block, not on other tokens' routes.  (It differs from ssd_moe_gemm's result, whose four
 * waves each sum every fourth k-tile, by fp32 rounding.)
 *
 * Every T >= 1 is correct; the kernel is meant for prefills of hundreds of rows and more.  Tables of experts without entries are
 * never read; rows of rows_in that no entry names are never read; output rows are written for every entry, nothing else is.  offs /
 * perm values outside their ranges are clamped / skipped (an entry index outside [0, T k) reads row 0 and stores nothing), so a bad
 * table never addresses outside the buffers.
 *
 * BM = SSD_MOE_TILED_BM = 128 and BN = SSD_MOE_TILED_BN = 128: four waves, 64 KiB of LDS, two workgroups per CU.
 *
 * Shapes: those of ssd_moe_gemm -- 1 <= k <= 8 <= E <= 256, E % 8 == 0, k <= E; K % 32 == 0; SSD_MOE_EPI_UP: N % 64 == 0;
 * SSD_MOE_EPI_DOWN: N % 16 == 0; T >= 1 and T * k <= 2^24 -- and (floor(T k / BM) + E) * ceil(N / BN) < 2^31.
 * Refusals, before any launch: SSD_ERR_ARG for a null pointer the kernel would dereference, or an unknown epilogue;
 * SSD_ERR_SHAPE for every shape outside the list above.
 */
#ifndef SSD_HIP_MOE_TILED_H
#define SSD_HIP_MOE_TILED_H
#include "ssd_hip_moe.h"
#ifdef __cplusplus
extern "C" {
#endif

#define SSD_MOE_TILED_BM 128
#define SSD_MOE_TILED_BN 128

int ssd_moe_gemm_tiled(const void* rows_in, const void* w_frag, const int32_t* offs, const int32_t* perm, void* out, int T, int k,
                       int E, int N, int K, int epilogue, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_MOE_TILED_H */
