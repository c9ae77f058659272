/*
 * libssdhip -- MXFP4 (OCP microscaling FP4: e2m1 element codes, one e8m0 power-of-two scale per row and 32-column block) weight-only
 * quantization of the target's decoder linears.
 *
 * Additive to ssd_hip.h (same conventions, error codes and ABI version): the reference has no call site for these, so they live in a
 * header of their own, next to ssd_hip_quant.h (fp8) and ssd_hip_w4a16.h (int4).  A quantized matrix W[N][K] (K % 128 == 0) is
 *   q[N][K]     e2m1 codes, 4 bits s e e m: magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 for codes 0..7, sign in bit 3, and
 *   b[N][K/32]  one scale byte per output row and 32-column block, 2 <= b <= 252,      W = 2^(b[n][k/32] - 127) * e2m1(q[n][k]).
 * In that range of b every weight is a normal (or zero), finite bf16 number, so W is an exact bf16 matrix.  Scale bytes outside it are
 * the caller's to refuse: the kernels widen a byte with one shift (float bits b << 23) and do not look at it.
 *
 * Row form: codes uint8 [N][K/2], byte j of a row holds column 2j in bits 0..3 and column 2j+1 in bits 4..7 (so the little-endian
 * 32-bit word w of a row holds columns 8w .. 8w+7, column 8w+i in bits 4i .. 4i+3); scales uint8 [N][K/32].
 *
 * "mx4 frag" layout of the codes: [N/16][K/128][64 lanes][4 words] (16 bytes per lane, 1 KiB per unit).  Lane l of unit (row group
 * g, column group c) holds row g*16 + (l & 15); its word j (0..3) is the row-form word of the 8 columns 128c + 32j + 8*(l >> 4) + e,
 * e = 0..7 (its slice of bf16 k-tile 4c + j), unpermuted: byte p of the word = columns e = 2p (bits 0..3) and 2p+1 (bits 4..7).
 * v_cvt_scalef32_pk_bf16_fp4 with byte select p turns that byte into the bf16 pair (column 2p, column 2p+1) times the block scale:
 * one contiguous 1 KiB wave load feeds four v_mfma_f32_16x16x32_bf16 k-steps of a 16-row group.
 * "mx4 frag" layout of the scales: uint8 [N/16][K/128][16][4], entry (g, c, r, j) = b[g*16 + r][4c + j] (64 bytes per unit): the
 * four scale bytes of a lane's row for the unit's four k-tiles are one aligned 4-byte load.
 */
#ifndef SSD_HIP_MXFP4_H
#define SSD_HIP_MXFP4_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Row form (codes uint8 [N][K/2], scales uint8 [N][K/32]) -> mx4 frag codes and scales.  row_map (int32 [N], device; NULL =
 * identity) names the SOURCE row of every destination row, which is how the packed orders of the bf16 path (rotation-paired QKV,
 * gate/up interleave) are applied; the scales follow their rows. */
int ssd_mx4_rows_to_frag(const void* q_rows, const void* s_rows, void* q_frag, void* s_frag, const int32_t* row_map, int N, int K,
                         void* stream);
/* mx4 frag -> row form in destination row order (tests / inspection). */
int ssd_mx4_frag_to_rows(const void* q_frag, const void* s_frag, void* q_rows, void* s_rows, int N, int K, void* stream);
/* bf16 frag [N][K] (ssd_hip.h layout, same row order) = 2^(b - 127) * e2m1(q), exact: the weights of the bf16 prefill GEMMs for
 * prompts longer than the direct limit.  w_frag needs N*K*2 bytes. */
int ssd_mx4_dequant_frag(const void* q_frag, const void* s_frag, void* w_frag, int N, int K, void* stream);

/* y = x . W^T for M <= 128 token rows.  x: bf16 frag [M][K]; q, s: mx4 frag; bias: bf16 [N] or NULL.
 * epilogue SSD_EPI_ROWS: y rows bf16 [M][ldy] = bf16(acc + bias[n]);
 *          SSD_EPI_SILU_FRAG: row groups alternate gate / up, y = bf16 frag [M][N/2] of silu(g)*u.
 * acc is the fp32 MFMA sum over K of x times the exact bf16 weights. */
int ssd_gemm_mxfp4(const void* x_frag, const void* q_frag, const void* s_frag, const void* bias, void* y, int M, int N, int K, int ldy,
                   int epilogue, void* stream);
/* The same with an explicit decomposition (sweeps): nt = row groups per workgroup (1, 2, 4; bit 8 = twice the column groups in
 * flight per wave), waves = waves per workgroup (1..8; bits 8..15 = consecutive tiles per workgroup, 0 = 1). */
int ssd_gemm_mxfp4_cfg(const void* x_frag, const void* q_frag, const void* s_frag, const void* bias, void* y, int M, int N, int K,
                       int ldy, int epilogue, int nt, int waves, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_MXFP4_H */
