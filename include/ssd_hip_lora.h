/*
 * libssdhip -- LoRA adapters: per-row low-rank deltas on the rows a linear's GEMM has just produced.
 *
 * Additive to ssd_hip.h (same conventions, error codes and ABI version).  Every call takes raw device pointers and a stream, never
 * allocates and never synchronises: both launches are hipGraph-capturable.  An adapter is data: another adapter in the same slot
 * table runs the same launches.
 *
 * Semantics (normative).  For a linear with base output y0 = bf16(x . W^T [+ bias]) (the rows its GEMM stored) and, for the row's
 * adapter, A [r][K], B [N][r] and scale = lora_alpha / r (lora_alpha / sqrt(r) with use_rslora):
 *   t[j] = bf16(sum_k x[k] * A[j][k])                       fp32 accumulation in a fixed order (below), one rounding
 *   y[n] = bf16(float(y0[n]) + scale * sum_j t[j] * B[n][j]) fp32 sum, the scale multiplied in fp32, one rounding
 * This rounds once more than the exact sum (y0) and less often than bf16 PEFT modules, which round t, the delta, the scaled delta
 * and the sum.  A rank below the slot's rank R is zero-padded (exact: the padded terms are +0).  q | k | v and gate | up are fused
 * linears here: the parts' adapters are packed as ONE adapter of the fused linear -- the A matrices stacked ([sum of ranks][K],
 * padded to R), B block-structured (part p's rows carry part p's columns, zero elsewhere), B's rows carried through the same row
 * maps as the base weight (rotation-paired QKV, interleaved gate / up: the column order the rows epilogue of those GEMMs emits).
 *
 * Tables.  `slots` adapters of one linear share one geometry:
 *   a_frag   slots matrices [R][K], each fragment-major (ssd_rows_to_frag mode 0), R % 32 == 0, R <= 192, K % 32 == 0
 *   b_frag   slots matrices [N][R], each fragment-major (mode 0), N % 16 == 0
 *   scale    fp32 [slots]
 *   row_slot int32 [M]: the slot of every token row, -1 = no adapter.  A value outside [-1, slots) is treated as -1, so a bad
 *            index never addresses outside the tables.
 * A 16-row tile may mix slots and -1 rows in any pattern; every (row, column) of every output has exactly one writer.
 *
 * ssd_lora_shrink.  x_frag is the fragment-major activation the base GEMM has just read ([ceil(M/16)][K/32] tiles of 1 KiB); its
 * padding rows past M may hold anything (NaN included) and influence nothing.  K is split over S workgroups per (slot, 16 ranks,
 * 32 token rows): split s owns k-tiles [s*KT/S, (s+1)*KT/S) (integer division, KT = K/32), dealt to the workgroup's 4 waves round-robin,
 * each wave accumulating its k-tiles in ascending order on v_mfma_f32_16x16x32_bf16, the 4 waves summed in wave order.  The result is
 * the fp32 slab ws[s][m][0..R) for every row m with a slot; rows without one are not written.  No float atomics: the kernel boundary
 * is the only synchronisation, and the consumer sums the slabs in slab order.
 *
 * ssd_lora_expand.  Per row with a slot: t = bf16(ws[0][m] + ws[1][m] + ... + ws[S-1][m]) (left to right), multiplied with the
 * slot's B on the MFMA in ascending rank order, scaled in fp32, then
 *   epilogue 0 (SSD_LORA_EPI_ADD):  y rows [M][ldy] updated in place; rows without a slot keep their bits (they are not written).
 *   epilogue 1 (SSD_LORA_EPI_SILU): gate_up only.  y holds the packed gate / up column order (alternating 16-column groups: gate
 *       features 16p.., up features 16p..), N % 64 == 0.  act_frag [M][N/2], fragment-major, receives silu(g) * u of the UPDATED
 *       values for ALL M rows, with the arithmetic of ssd_silu_mul (fp32 on the bf16-rounded values, one rounding).  y itself is
 *       not rewritten.
 * A workgroup serves 32 token rows; at M <= 32 every table byte is read once per launch.
 *
 * Refusals, before any launch: SSD_ERR_ARG for a null pointer the kernel would dereference, an unknown epilogue, slots < 1, splits
 * outside 1..16 or above K/32, a workspace smaller than splits * M * R * 4 bytes; SSD_ERR_SHAPE for M <= 0, K % 32, R % 32, R > 192,
 * N % 16, ldy < N, epilogue 1 with N % 64.
 */
#ifndef SSD_HIP_LORA_H
#define SSD_HIP_LORA_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define SSD_LORA_EPI_ADD 0
#define SSD_LORA_EPI_SILU 1
#define SSD_LORA_MAX_R 192
#define SSD_LORA_MAX_SPLITS 16

/* The K split both launches use when `splits` is 0: between 1 and 16, never above K/32.  0 for a K the kernels refuse. */
int ssd_lora_default_splits(int K);
/* Bytes of a workspace that serves every legal split of an M-row launch: min(16, K/32) * M * R * 4.  0 for refused shapes. */
long ssd_lora_workspace_bytes(int M, int K, int R);

/* fp32 slabs ws[splits][M][R] of x . A^T for the rows that name a slot.  splits 0 = the default. */
int ssd_lora_shrink(const void* x_frag, const void* a_frag, const int32_t* row_slot, float* ws, long ws_bytes, int M, int K, int R,
                    int slots, int splits, void* stream);

/* y += scale * t . B^T (epilogue 0) or act_frag = silu_mul of the updated rows (epilogue 1); K is the K of the shrink that filled ws
 * (it names the default split when splits is 0), act_frag is NULL for epilogue 0. */
int ssd_lora_expand(const float* ws, long ws_bytes, const void* b_frag, const float* scale, const int32_t* row_slot, void* y, int ldy,
                    void* act_frag, int M, int N, int K, int R, int slots, int splits, int epilogue, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_LORA_H */
