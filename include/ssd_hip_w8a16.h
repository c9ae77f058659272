/*
 * libssdhip -- W8A16 (signed int8 codes, one bf16 scale per row and 128-column group) weight-only quantization of the target's
 * decoder linears.
 *
 * Additive to ssd_hip.h (same conventions, error codes and ABI version): the reference has no call site for these, so they live in a
 * header of their own, next to ssd_hip_quant.h (fp8) and ssd_hip_w4a16.h (int4).  A quantized matrix W[N][K] (K % 128 == 0,
 * N % 16 == 0) is
 *   q[N][K]      signed int8 codes in [-128, 127], and
 *   s[N][K/128]  one bf16 scale per output row and 128-column group,          W = s[n][k/128] * q[n][k].
 * A per-channel checkpoint repeats its one scale across the groups of a row.
 *
 * Row form: codes uint8 [N][K], the byte of column k is u = q + 128 (read as little-endian int32 words these are the four 8-bit
 * fields per word of compressed-tensors "pack-quantized" with num_bits 8); scales bf16 [N][K/128].
 *
 * "w8 frag" layout of the codes: [N/16][K/64][64 lanes][16 bytes] -- the byte ORDER of the "fp8 frag" layout of ssd_hip_quant.h:
 * lane l of the 1 KiB unit (row group g, k-pair p) holds row g*16 + (l & 15), bytes 0..7 are columns 64p + 8*(l >> 4) + 0..7 (its
 * slice of bf16 k-tile 2p), bytes 8..15 are columns 64p + 32 + 8*(l >> 4) + 0..7 (k-tile 2p+1).  The byte VALUE in device memory is
 * the two's-complement q = u ^ 0x80, not u: a sign-extending byte select converts it to fp32 in one instruction
 * (v_cvt_f32_i32 with an SDWA byte operand) and the top halves of two such floats are the bf16 pair (one v_perm_b32), 1.5 vector
 * instructions per weight and no offset to remove afterwards; from u the same path needs a subtract per weight or a correction
 * MFMA chain per k-tile.  Because the value differs from the row form, ssd_fp8_rows_to_frag is NOT reused: ssd_w8_rows_to_frag moves
 * the bytes in the same order and flips bit 7 on the way.  Every int8 value is a bf16 value (|q| <= 128 has at most 8 significant
 * bits), so one contiguous 1 KiB wave load feeds two v_mfma_f32_16x16x32_bf16 k-steps of a 16-row group on the exact integers; the
 * two units of a 128-column group share one scale.
 * "w8 frag" layout of the scales: the w4 frag scale table, bf16 [N/16][K/128][16], entry (g, c, r) = s[g*16 + r][c].
 */
#ifndef SSD_HIP_W8A16_H
#define SSD_HIP_W8A16_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Row form (codes uint8 [N][K] as u = q + 128, scales bf16 [N][K/128]) -> w8 frag codes (N*K bytes) and scales.  row_map (int32 [N],
 * device; NULL = identity) names the SOURCE row of every destination row, which is how the packed orders of the bf16 path
 * (rotation-paired QKV, gate/up interleave) are applied; the scales follow their rows. */
int ssd_w8_rows_to_frag(const void* q_rows, const void* s_rows, void* q_frag, void* s_frag, const int32_t* row_map, int N, int K,
                        void* stream);
/* w8 frag -> row form in destination row order (tests / inspection). */
int ssd_w8_frag_to_rows(const void* q_frag, const void* s_frag, void* q_rows, void* s_rows, int N, int K, void* stream);
/* bf16 frag [N][K] (ssd_hip.h layout, same row order) = bf16(s * q), the product taken in fp32: the weights of the bf16 prefill
 * GEMMs for prompts longer than the direct limit.  w_frag needs N*K*2 bytes. */
int ssd_w8_dequant_frag(const void* q_frag, const void* s_frag, void* w_frag, int N, int K, void* stream);

/* y = x . (s (.) q)^T for M <= 128 token rows.  x: bf16 frag [M][K]; q, s: w8 frag; bias: bf16 [N] or NULL.
 * epilogue SSD_EPI_ROWS: y rows bf16 [M][ldy] = bf16(acc + bias[n]);
 *          SSD_EPI_SILU_FRAG: row groups alternate gate / up, y = bf16 frag [M][N/2] of silu(g)*u.
 * acc is the fp32 sum over column groups of s * (the group's fp32 partial dot product); a 128-column group contributes its two
 * 64-column code units one after the other, each as s * (the unit's fp32 partial).  Never allocates or synchronises;
 * hipGraph-capturable. */
int ssd_gemm_w8a16(const void* x_frag, const void* q_frag, const void* s_frag, const void* bias, void* y, int M, int N, int K, int ldy,
                   int epilogue, void* stream);
/* The same with an explicit decomposition (sweeps): nt = row groups per workgroup (1, 2, 4; bit 8 = twice the code units in flight
 * per wave), waves = waves per workgroup (1..8; bits 8..15 = consecutive tiles per workgroup, 0 = 1). */
int ssd_gemm_w8a16_cfg(const void* x_frag, const void* q_frag, const void* s_frag, const void* bias, void* y, int M, int N, int K,
                       int ldy, int epilogue, int nt, int waves, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_W8A16_H */
