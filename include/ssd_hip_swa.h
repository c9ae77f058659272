/*
 * libssdhip -- sliding-window attention: the paged attention of ssd_hip.h / ssd_hip_kv8.h under a per-layer key window.
 *
 * Additive to ssd_hip.h and ssd_hip_kv8.h (same conventions, error codes and ABI version).
 *
 * Semantics.  With window W >= 1, the query at absolute position i sees the keys j with i - W < j <= i: W keys, itself included.
 * This is the Hugging Face rule kv_idx > q_idx - sliding_window, and vLLM's rule.  In the terms of the kernel (mode 0, bottom-right
 * aligned): a row with causal limit lim sees the keys [max(0, lim - W), lim).
 *   - W = 0 means no window: the call launches exactly what the unwindowed entry launches.
 *   - Every row of a verify or a prefill has its own window: row r of an 8-row verify is cut off at lim_r - W, not at the first
 *     row's edge.
 *   - If W is at least every row's lim, no key is cut off and the output is bit-identical to the unwindowed entry with the same
 *     splits, flags and waves: the tile dealing then starts at key 0, so the accumulation order is the old one.
 *   - The window is measured in cache positions.  Windowed launches are causal (mode 0) only, so cache positions are absolute
 *     positions.
 *
 * Cost and the never-read guarantee.  A workgroup scans the 32-key tiles of [kmin, kmax) only, kmin = its first row's left edge
 * rounded down to a tile: a windowed decode at a 32k context streams what a W-key context streams.  For sequence b let
 * lo_b = max(0, lim of its first query row - W).  No K or V row with key < lo_b is addressed, and no block-table entry of a page
 * that lies wholly in front of lo_b is used to form an address: such pages may be recycled or hold anything.
 *
 * head_dim is 64 or 128, as for the unwindowed entries.  Workspaces are as for the unwindowed entries.
 */
#ifndef SSD_HIP_SWA_H
#define SSD_HIP_SWA_H
#include "ssd_hip.h"
#include "ssd_hip_kv8.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ssd_attn_paged with a window.  window == 0 forwards to ssd_attn_paged (every mode).  window < 0, or window > 0 with mode != 0 (the
 * draft-tree mask is not windowed), returns SSD_ERR_ARG before any launch; so does a null q / cache / table / output pointer when
 * window > 0.  The tree_* arguments are ignored when window > 0. */
int ssd_attn_paged_window(const void* q_rows, const void* k_cache, const void* v_cache, const int32_t* block_tables,
                          int max_blocks, const int32_t* context_lens, const int32_t* cu_q, int q_per_seq, int B, int T,
                          int max_q, int nh, int nkv, int hd, int block_size, float scale, int mode, int tree_K,
                          int tree_mq, int tree_step, int tree_F, const int32_t* tree_jidx, int splits, int flags,
                          void* ws_o, void* ws_ml, void* out_rows, void* out_frag, int window, void* stream);

/* ssd_attn_paged_fp8 with a window: byte caches, k_scale / v_scale fp32 [nkv] or NULL = 1.0.  window == 0 forwards to
 * ssd_attn_paged_fp8; the refusals are those above. */
int ssd_attn_paged_fp8_window(const void* q_rows, const void* k_cache, const void* v_cache, const float* k_scale,
                              const float* v_scale, const int32_t* block_tables, int max_blocks, const int32_t* context_lens,
                              const int32_t* cu_q, int q_per_seq, int B, int T, int max_q, int nh, int nkv, int hd,
                              int block_size, float scale, int mode, int tree_K, int tree_mq, int tree_step, int tree_F,
                              const int32_t* tree_jidx, int splits, int flags, void* ws_o, void* ws_ml, void* out_rows,
                              void* out_frag, int window, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_SWA_H */
