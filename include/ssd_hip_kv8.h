/*
 * libssdhip -- FP8 (OCP e4m3fn) paged KV cache: the RoPE / KV store and the paged attention over a cache of one byte per element.
 *
 * Additive to ssd_hip.h (same conventions, error codes and ABI version).  The cache layout is the bf16 one with a 1-byte element:
 * per layer and per K / V, uint8 [num_blocks][n_kv_heads][block_size][head_dim]; one (page, kv head) is a contiguous run of
 * block_size * head_dim bytes.  There is one fp32 scale per kv head (per layer and per K / V: the caller passes that layer's row):
 *   store:  code = e4m3fn_rne(clamp(fp32(x) * inv_scale[h], -448, 448))     x = the bf16 value the bf16 cache would have held,
 *                                                                            inv_scale[h] = 1 / scale[h] computed by the host in fp32
 *   load:   value = scale[h] * fp32(code)                                    (every e4m3 code is an exact bf16 value)
 * One fp32 multiply, then the clamp, then round-to-nearest-even; -0.0 is kept; codes 0x7F / 0xFF (NaN) come from a NaN input only.
 * q, the attention output and every activation stay bf16.  head_dim is 64 or 128.
 */
#ifndef SSD_HIP_KV8_H
#define SSD_HIP_KV8_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ssd_rope_store_kv with byte caches: (optional per-head RMSNorm) + neox RoPE + KV store of T rows [q | k | v].  q_out_rows is the bf16
 * output of ssd_rope_store_kv, bit for bit; K (after norm and RoPE, rounded to bf16) and V are encoded as above.
 * k_inv_scale / v_inv_scale: fp32 [nkv] on the device, NULL = 1.0.  SSD_ERR_ARG for a null row / cache pointer, SSD_ERR_SHAPE for a
 * head_dim other than 64 / 128. */
int ssd_rope_store_kv_fp8(const void* qkv_rows, const int64_t* positions, const float* cos_sin, const int32_t* slot_mapping,
                          void* q_out_rows, void* k_cache, void* v_cache, const float* k_inv_scale, const float* v_inv_scale,
                          const void* q_norm_w, const void* k_norm_w, float eps, int T, int nh, int nkv, int hd, int block_size,
                          int qkv_perm, void* stream);

/* ssd_attn_paged over byte caches, causal mode only (mode 1, the draft's tree mask, returns SSD_ERR_ARG: the draft's cache is bf16;
 * the tree_* arguments are ignored).  k_scale / v_scale: fp32 [nkv] on the device, NULL = 1.0.  cu_q, splits + the merge kernel,
 * flags (bit 0 plain LDS read, bit 1 single-bf16 P, bit 2 one row tile per workgroup, bits 8..11 waves 1..8), out_rows / out_frag:
 * as ssd_attn_paged.  With power-of-two scales the result is bit-identical to ssd_attn_paged over the bf16 cache scale * code. */
int ssd_attn_paged_fp8(const void* q_rows, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale,
                       const int32_t* block_tables, int max_blocks, const int32_t* context_lens, const int32_t* cu_q, int q_per_seq,
                       int B, int T, int max_q, int nh, int nkv, int hd, int block_size, float scale, int mode, int tree_K,
                       int tree_mq, int tree_step, int tree_F, const int32_t* tree_jidx, int splits, int flags, void* ws_o,
                       void* ws_ml, void* out_rows, void* out_frag, void* stream);

/* ssd_attn_prefill_varlen over byte caches (cu_q int32 [B + 1] required). */
int ssd_attn_prefill_varlen_fp8(const void* q_rows, const void* k_cache, const void* v_cache, const float* k_scale,
                                const float* v_scale, const int32_t* block_tables, int max_blocks, const int32_t* context_lens,
                                const int32_t* cu_q, int B, int T, int max_q, int nh, int nkv, int hd, int block_size, float scale,
                                void* out_rows, void* out_frag, void* stream);

/* cache_bf16 [pages][nkv][block_size][hd] = bf16(scale[h] * code) over whole pages (tests / inspection).  scale: fp32 [nkv], NULL = 1.0. */
int ssd_kv_fp8_dequant(const void* cache8, const float* scale, void* cache_bf16, int pages, int nkv, int block_size, int hd,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_KV8_H */
