/*
 * libssdhip -- W4A16 with zero points (unsigned int4 codes, one bf16 scale and one 4-bit zero point per row and 128-column group):
 * the form of AWQ and asymmetric GPTQ checkpoints, and of the min/max on-load quantizer.
 *
 * Additive to ssd_hip.h and ssd_hip_w4a16.h (same conventions, error codes and ABI version).  A quantized matrix W[N][K]
 * (K % 128 == 0, N % 16 == 0) is
 *   u[N][K]      unsigned int4 codes in [0, 15],
 *   s[N][K/128]  one bf16 scale per output row and 128-column group, and
 *   z[N][K/128]  one integer zero point in [0, 15] per output row and group,     W = s[n][k/128] * (u[n][k] - z[n][k/128]).
 * The symmetric format of ssd_hip_w4a16.h is the special case z = 8 everywhere (its nibble is u = q + 8).
 *
 * Row form: codes int32 [N][K/8], word j of a row holds columns 8j .. 8j+7, column 8j+i in bits 4i .. 4i+3 as the nibble u;
 * scales bf16 [N][K/128]; zero points uint8 [N][K/128], one per byte, value 0..15 (the high nibble is zero).
 *
 * Device layout.  Codes and scales: the "w4 frag" layout of ssd_hip_w4a16.h, unchanged (1 KiB of codes and 32 bytes of scales per
 * unit of 16 rows x 128 columns).  Zero points: uint8 [N/16][K/128][16], one byte per entry, 16 bytes per unit:
 *   byte 16 * (g * (K/128) + c) + r  =  z[16g + r][c]          (g = row group, c = column group, r = 0..15, value 0..15).
 * An MFMA lane l owns the four accumulator rows 16g + 4 * (l >> 4) + {0, 1, 2, 3}; their zero points are the four consecutive
 * bytes at offset 4 * (l >> 4) of the unit, which the GEMM reads as one aligned 4-byte load (byte i of the little-endian word is
 * row 4 * (l >> 4) + i).  One byte per zero point rather than a nibble: v_cvt_f32_ubyte0..3 turn the word into four floats with
 * no shift or mask, and the table is 16 of a unit's 1072 bytes either way.
 */
#ifndef SSD_HIP_W4ZP_H
#define SSD_HIP_W4ZP_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Row form -> device layout (w4 frag codes and scales, zero-point table).  row_map (int32 [N], device; NULL = identity) names the
 * SOURCE row of every destination row, as in ssd_w4_rows_to_frag; scales and zero points follow their rows. */
int ssd_w4zp_rows_to_frag(const void* q_rows, const void* s_rows, const void* z_rows, void* q_frag, void* s_frag, void* z_frag,
                          const int32_t* row_map, int N, int K, void* stream);
/* Device layout -> row form in destination row order (tests / inspection). */
int ssd_w4zp_frag_to_rows(const void* q_frag, const void* s_frag, const void* z_frag, void* q_rows, void* s_rows, void* z_rows, int N,
                          int K, void* stream);
/* bf16 frag [N][K] (ssd_hip.h layout, same row order) = bf16(s * (u - z)), the product in fp32: the weights of the bf16 prefill
 * GEMMs for prompts longer than the direct limit.  w_frag needs N*K*2 bytes. */
int ssd_w4zp_dequant_frag(const void* q_frag, const void* s_frag, const void* z_frag, void* w_frag, int N, int K, void* stream);

/* y = x . (s (.) (u - z))^T for M <= 128 token rows: the contract of ssd_gemm_w4a16 (epilogues SSD_EPI_ROWS and
 * SSD_EPI_SILU_FRAG, bias bf16 [N] or NULL) with z_frag the zero-point table above.  Never allocates or synchronises. */
int ssd_gemm_w4a16_zp(const void* x_frag, const void* q_frag, const void* s_frag, const void* z_frag, const void* bias, void* y,
                      int M, int N, int K, int ldy, int epilogue, void* stream);
/* The same with an explicit decomposition; nt and waves are encoded as for ssd_gemm_w4a16_cfg. */
int ssd_gemm_w4a16_zp_cfg(const void* x_frag, const void* q_frag, const void* s_frag, const void* z_frag, const void* bias, void* y,
                          int M, int N, int K, int ldy, int epilogue, int nt, int waves, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_W4ZP_H */
