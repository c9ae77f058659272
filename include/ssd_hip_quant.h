/*
 * libssdhip -- FP8 (OCP e4m3fn) weight-only quantization of the target's decoder linears.
 *
 * Additive to ssd_hip.h (same conventions, error codes and ABI version): the reference has no call site for these, so they live in a
 * header of their own.  A quantized matrix W[N][K] is stored as
 *   q[N][K]  e4m3fn codes, one byte each, and
 *   s[N]     one fp32 scale per output row,          W ~= s[n] * q[n][k].
 *
 * "fp8 frag" layout of q (K % 64 == 0): [N/16][K/64][64 lanes][16 bytes].  Lane l of the 1 KiB unit (row group g, k-pair p) holds row
 * g*16 + (l & 15): bytes 0..7 are columns 64p + 8*(l >> 4) + 0..7 (its slice of bf16 k-tile 2p) and bytes 8..15 are columns
 * 64p + 32 + 8*(l >> 4) + 0..7 (its slice of k-tile 2p+1).  One contiguous 1 KiB wave load therefore feeds two
 * v_mfma_f32_16x16x32_bf16 k-steps of a 16-row group after an exact fp8 -> bf16 conversion in registers.
 */
#ifndef SSD_HIP_QUANT_H
#define SSD_HIP_QUANT_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Row-major e4m3fn codes [N][K] -> fp8 frag.  row_map (int32 [N], device; NULL = identity) names the SOURCE row of every destination
 * row, which is how the packed orders of the bf16 path (rotation-paired QKV, gate/up interleave) are applied. */
int ssd_fp8_rows_to_frag(const void* q_rows, void* q_frag, const int32_t* row_map, int N, int K, void* stream);
/* fp8 frag -> row-major codes [N][K] in destination row order (tests / inspection). */
int ssd_fp8_frag_to_rows(const void* q_frag, void* q_rows, int N, int K, void* stream);
/* bf16 frag [N][K] (ssd_hip.h layout, same row order) = bf16(s[n] * q[n][k]): the weights of the bf16 prefill GEMMs for prompts
 * longer than 128 rows.  w_frag needs N*K*2 bytes. */
int ssd_fp8_dequant_frag(const void* q_frag, const float* scale, void* w_frag, int N, int K, void* stream);

/* y = x . (s (.) q)^T for M <= 128 token rows.  x: bf16 frag [M][K]; scale: fp32 [N] in the packed row order; bias: bf16 [N] or NULL.
 * epilogue SSD_EPI_ROWS: y rows bf16 [M][ldy] = bf16(s[n]*acc + bias[n]);
 *          SSD_EPI_SILU_FRAG: row groups alternate gate / up, each scaled by its own row scale, y = bf16 frag [M][N/2] of silu(g)*u. */
int ssd_gemm_fp8(const void* x_frag, const void* q_frag, const float* scale, const void* bias, void* y, int M, int N, int K, int ldy,
                 int epilogue, void* stream);
/* The same with an explicit decomposition (sweeps): nt = row groups per workgroup (1, 2, 4; bit 8 = twice the k-pairs in flight per
 * wave), waves = waves per workgroup (1..8; bits 8..15 = consecutive tiles per workgroup, 0 = 1). */
int ssd_gemm_fp8_cfg(const void* x_frag, const void* q_frag, const float* scale, const void* bias, void* y, int M, int N, int K, int ldy,
                     int epilogue, int nt, int waves, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_QUANT_H */
