// Log-probabilities of rows whose token is known before the row is read (include/ssd_hip_prompt_logprob.h): the prompt rows of a
// prefill.  The kernels are the KNOWN instantiations of logprob.h: the slice pass also counts the entries >= the token's, the merge adds
// the counts into the rank and writes the token's log-probability, so a row is read once and no pick launch follows.
#include "common.h"
#include "logprob.h"

extern "C" int ssd_logprob_known_ws_bytes(int T, int V) { return ssd_logprob_rows_ws_bytes(T, V); }

extern "C" int ssd_logprob_rows_known(const void* logits_rows, long ld, int T, int V, const int32_t* n_top, const int64_t* tokens, float* lse,
                                      float* top_val, int32_t* top_id, float* out, int32_t* rank, void* ws, void* stream) {
  if (T <= 0 || V <= 0 || ld < V || V > SSD_LOGPROB_MAX_V || T > 65535) return SSD_ERR_SHAPE;
  if (!logits_rows || !n_top || !tokens || !lse || !out || !rank || !ws || (!top_val) != (!top_id)) return SSD_ERR_ARG;
  const int S = lp_slices(V);
  hipLaunchKernelGGL(logprob_slice_kernel<true>, dim3(S, T), dim3(LP_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits_rows, ld, V, n_top,
                     1, S, (bf16_t*)nullptr, 0L, tokens, (float*)ws);
  hipLaunchKernelGGL(logprob_merge_kernel<true>, dim3(T), dim3(64), 0, (hipStream_t)stream, (const float*)ws, n_top, 1, S, lse, top_val,
                     top_id, (const bf16_t*)logits_rows, ld, V, tokens, out, rank);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}
