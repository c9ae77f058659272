/*
 * libssdhip -- W4A16 (signed int4 codes, one bf16 scale per row and 128-column group) weight-only quantization of the target's
 * decoder linears.
 *
 * Additive to ssd_hip.h (same conventions, error codes and ABI version): the reference has no call site for these, so they live in a
 * header of their own, next to ssd_hip_quant.h (fp8).  A quantized matrix W[N][K] (K % 128 == 0) is
 *   q[N][K]      signed int4 codes in [-8, 7], and
 *   s[N][K/128]  one bf16 scale per output row and 128-column group,          W ~= s[n][k/128] * q[n][k].
 *
 * Row form (the compressed-tensors "pack-quantized" form): codes int32 [N][K/8], word j of a row holds columns 8j .. 8j+7, column
 * 8j+i in bits 4i .. 4i+3 as the unsigned nibble u = q + 8; scales bf16 [N][K/128].
 *
 * "w4 frag" layout of the codes: [N/16][K/128][64 lanes][4 words] (16 bytes per lane, 1 KiB per unit).  Lane l of unit (row group
 * g, column group c) holds row g*16 + (l & 15); its word j (0..3) holds the 8 columns 128c + 32j + 8*(l >> 4) + e, e = 0..7 (its slice
 * of bf16 k-tile 4c + j), as nibbles u = q + 8 in the order e = 0, 2, 4, 6, 1, 3, 5, 7 (nibble i in bits 4i .. 4i+3).  So
 * ((word >> 4p) & 0x000F000F) | 0x43004300 is the bf16 pair (128 + u of column e = 2p, 128 + u of column 2p+1): one contiguous
 * 1 KiB wave load feeds four v_mfma_f32_16x16x32_bf16 k-steps of a 16-row group, exactly, offset by 136.
 * "w4 frag" layout of the scales: bf16 [N/16][K/128][16], entry (g, c, r) = s[g*16 + r][c] (32 bytes per unit).
 */
#ifndef SSD_HIP_W4A16_H
#define SSD_HIP_W4A16_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Row form (codes int32 [N][K/8], scales bf16 [N][K/128]) -> w4 frag codes and scales.  row_map (int32 [N], device; NULL =
 * identity) names the SOURCE row of every destination row, which is how the packed orders of the bf16 path (rotation-paired QKV,
 * gate/up interleave) are applied; the scales follow their rows. */
int ssd_w4_rows_to_frag(const void* q_rows, const void* s_rows, void* q_frag, void* s_frag, const int32_t* row_map, int N, int K,
                        void* stream);
/* w4 frag -> row form in destination row order (tests / inspection). */
int ssd_w4_frag_to_rows(const void* q_frag, const void* s_frag, void* q_rows, void* s_rows, int N, int K, void* stream);
/* bf16 frag [N][K] (ssd_hip.h layout, same row order) = bf16(s * q): the weights of the bf16 prefill GEMMs for prompts longer than
 * the direct limit.  w_frag needs N*K*2 bytes. */
int ssd_w4_dequant_frag(const void* q_frag, const void* s_frag, void* w_frag, int N, int K, void* stream);

/* y = x . (s (.) q)^T for M <= 128 token rows.  x: bf16 frag [M][K]; q, s: w4 frag; bias: bf16 [N] or NULL.
 * epilogue SSD_EPI_ROWS: y rows bf16 [M][ldy] = bf16(acc + bias[n]);
 *          SSD_EPI_SILU_FRAG: row groups alternate gate / up, y = bf16 frag [M][N/2] of silu(g)*u.
 * acc is the fp32 sum over column groups of s * (the group's fp32 partial dot product). */
int ssd_gemm_w4a16(const void* x_frag, const void* q_frag, const void* s_frag, const void* bias, void* y, int M, int N, int K, int ldy,
                   int epilogue, void* stream);
/* The same with an explicit decomposition (sweeps): nt = row groups per workgroup (1, 2, 4; bit 8 = twice the column groups in
 * flight per wave), waves = waves per workgroup (1..8; bits 8..15 = consecutive tiles per workgroup, 0 = 1). */
int ssd_gemm_w4a16_cfg(const void* x_frag, const void* q_frag, const void* s_frag, const void* bias, void* y, int M, int N, int K,
                       int ldy, int epilogue, int nt, int waves, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_W4A16_H */
