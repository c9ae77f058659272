/*
 * libssdhip -- per-request seeds: a random stream keyed by what belongs to the request, and the sampling and ratio-verification
 * launches that draw from it.
 *
 * Additive to ssd_hip.h (same conventions, error codes and ABI version).  The engine's own stream (csrc/stochastic.hip) is a function
 * of (rng word in device memory, launch salt, row of the batch, index): the same prompt draws other numbers depending on what the
 * engine sampled before, which batch slot the request landed in and whether it was preempted.  A request with a seed draws from
 *
 *   key(seed, purpose, pos)    = mix64( mix64(seed) ^ ((uint64)purpose << 56) ^ (uint64)pos )              0 <= pos < 2^48
 *   u(seed, purpose, pos, idx) = ((float)(mix64(key ^ idx) >> 40) + 0.5f) * 2^-24                          idx < 2^32
 *
 * with mix64 the finaliser of csrc/stochastic.h (splitmix64: z += 0x9e3779b97f4a7c15; z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9;
 * z = (z ^ z >> 27) * 0x94d049bb133111eb; z ^ z >> 31), 64-bit wrap-around arithmetic.  u lies in (0, 1) and has 24 bits.
 *   seed     0 <= seed < 2^63; a negative entry of a seed array means "no seed: the engine's stream"
 *   purpose  what the number is used for (below)
 *   pos      the ABSOLUTE position of the token being decided = the position of the row's input token + 1.  The kernels take the
 *            input positions (the arrays the forward pass already has on the device) and add the 1 themselves.
 *   idx      for a token draw the vocabulary index (the Gumbel noise of entry v is -log(-log(u(.., v)))); 0 for the acceptance uniform
 * Batch slot, launch count, rng word, salt and batch-mates play no part.
 *
 * Known answers (seed, purpose, pos, idx) -> mix64(key ^ idx) >> 40:
 *   (0, 1, 0, 0) -> 2331386 (key 0x9c8c1ca9370e13af, u = 0x1.1c97d4p-3)      (0, 2, 0, 0) -> 10258722 (key 0xc83312cb7bd81b65)
 *   (42, 2, 9, 5) -> 9468248      (2^63 - 1, 3, 8191, 0) -> 11556502      (1234567890123, 1, 300, 128255) -> 9889909
 */
#ifndef SSD_HIP_SEED_H
#define SSD_HIP_SEED_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Purposes.  The draft's draw, the acceptance uniform and the target's draw at one position are independent up to the hash. */
#define SSD_SEED_DRAFT 1   /* a draft model draws a token: synchronous chain, JIT chain, tree step */
#define SSD_SEED_TARGET 2  /* the target draws a token: decode, the prefill's first token, recovery from the residual, bonus draw from p */
#define SSD_SEED_ACCEPT 3  /* the uniform of the ratio test, idx = 0 */

/* Entries per slice of ssd_sample_rows_seeded (one workgroup of 256 threads x 2 chunks of 8). */
#define SSD_SEED_SLICE 4096

/* Bytes of workspace ssd_sample_rows_seeded needs for T rows of V entries: one (score, index) candidate of 8 bytes per row and slice.
 * SSD_ERR_SHAPE (negative) for T or V <= 0; every other shape has an answer. */
long ssd_sample_seeded_ws_bytes(int T, int V);

/* ssd_sample_rows (ssd_hip.h) with a seed per rows_per_seed consecutive rows.  The first fourteen arguments are ssd_sample_rows's.
 *   row_seed   int64, one entry per rows_per_seed rows, on the device (data, not a launch constant: a captured graph replays with
 *              other seeds).  < 0: the row draws from (rng word, salt, row, idx) and gets the token ssd_sample_rows gives it, bit
 *              for bit.  >= 0: the noise of entry v is u(seed, purpose, positions[row] + 1, v); rng word, salt and row are ignored.
 *   positions  int64 [T]: the position of each row's input token
 *   purpose    SSD_SEED_DRAFT or SSD_SEED_TARGET (SSD_SEED_ACCEPT is accepted too)
 *   workspace  ssd_sample_seeded_ws_bytes(T, V) bytes, 8-byte aligned
 * Rows of temperature 0 take the argmax whatever their seed.  Every row is cut into slices of SSD_SEED_SLICE entries, one workgroup per
 * (row, slice), with 16-byte loads where the row's address allows them; each leaves the slice's best (score, index) in the workspace and
 * a second launch merges a row's candidates with one wave.  The order "larger score, then lower index" is total (NaN scores are not
 * comparable and never win; a row with nothing comparable gives 0), so the token does not depend on the slicing.  No float atomics, no
 * host visit, hipGraph-capturable.
 * SSD_ERR_SHAPE for T, V, rows_per_temp or rows_per_seed <= 0; SSD_ERR_ARG for a null logits, temps, rng_state, out, row_seed,
 * positions or workspace, a purpose outside 1..3, or boost arguments ssd_sample_rows refuses. */
int ssd_sample_rows_seeded(const void* logits, long ld, int T, int V, const float* temps, int rows_per_temp, const void* rng_state,
                           unsigned salt, int64_t* out, int64_t* out2, const int32_t* boost_idx, int boost_k, float boost_x,
                           void* stream, const int64_t* row_seed, int rows_per_seed, const int64_t* positions, int purpose,
                           void* workspace);

/* ssd_verify_ratio (ssd_hip.h) with a seed per sequence.  The first twenty-four arguments are ssd_verify_ratio's.
 *   row_seed   int64 [B] on the device; < 0: the sequence draws from (rng word, salt, b) exactly as ssd_verify_ratio
 *   positions  int64 [B][K+1]: the positions of the verify's input tokens
 * A seeded sequence tests draft token x_{i+1} against u(seed, SSD_SEED_ACCEPT, positions[b][i] + 1, 0) and draws its recovery token at
 * row n (residual, or p after K acceptances or for a non-ratio row) with the noise u(seed, SSD_SEED_TARGET, positions[b][n] + 1, v).
 * accept_prob, greedy sequences' outputs and unseeded sequences are the bits ssd_verify_ratio writes.
 * Errors as ssd_verify_ratio, and SSD_ERR_ARG for a null row_seed or positions. */
int ssd_verify_ratio_seeded(const void* logits_p, long ld_p, const void* logits_q, long ld_q, int V, int B, int K,
                            const int64_t* spec, const int64_t* preds_p, const float* lse_p, const float* lse_q,
                            const float* temps_t, const float* temps_q, const int32_t* ratio_rows, const void* rng_state,
                            unsigned salt, int32_t* accept_len, int64_t* recovery, int64_t* packed, float* accept_prob,
                            const int32_t* boost_idx_q, int boost_k, float boost_x, void* stream, const int64_t* row_seed,
                            const int64_t* positions);

/* out[r][j] = u(row_seed[r], purpose, positions[r] + 1, idx0 + j), fp32 [rows][n]; a row whose seed is negative gets NaN.  The hook
 * that lets a test compare the device stream with the definition above by bits.
 * SSD_ERR_SHAPE for rows or n <= 0 or idx0 + n > 2^32; SSD_ERR_ARG for a null row_seed, positions or out or a purpose outside 1..3. */
int ssd_seeded_uniforms(const int64_t* row_seed, const int64_t* positions, int rows, int purpose, unsigned idx0, int n, float* out,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_SEED_H */
