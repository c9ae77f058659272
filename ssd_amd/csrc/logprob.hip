// Per-token log-probabilities of raw logit rows (include/ssd_hip_logprob.h): log-sum-exp, the n most probable entries, an optional
// bit-exact copy of the row, and the log-probability of the token the row produced.  The slice and merge kernels live in logprob.h,
// which prompt_logprob.hip shares; the picks that follow a decode or verify step are here.
#include "common.h"
#include "logprob.h"

// token < 0: none
__device__ __forceinline__ float lp_pick(const bf16_t* __restrict__ rows, long ld, int V, int t, long token, const float* __restrict__ lse) {
  if (token < 0 || token >= V) return __builtin_nanf("");
  return lp_logprob(rows + (size_t)t * ld, V, token, lse[t]);
}

__global__ void __launch_bounds__(LP_THREADS)
logprob_pick_kernel(const bf16_t* __restrict__ rows, long ld, int T, int V, const int64_t* __restrict__ tokens, const float* __restrict__ lse,
                    const int32_t* __restrict__ n_top, int rows_per_param, float* __restrict__ out) {
  const int t = blockIdx.x * LP_THREADS + threadIdx.x;
  if (t >= T || lp_count(n_top, t / rows_per_param) < 0) return;
  out[t] = lp_pick(rows, ld, V, t, tokens[t], lse);
}

__global__ void __launch_bounds__(LP_THREADS)
logprob_pick_verify_kernel(const bf16_t* __restrict__ rows, long ld, int B, int K, int V, const int64_t* __restrict__ ids,
                           const int32_t* __restrict__ accept, const int64_t* __restrict__ recovery, const float* __restrict__ lse,
                           const int32_t* __restrict__ n_top, float* __restrict__ out) {
  const int t = blockIdx.x * LP_THREADS + threadIdx.x;
  if (t >= B * (K + 1)) return;
  const int b = t / (K + 1), j = t % (K + 1);
  if (lp_count(n_top, b) < 0) return;
  const int a = accept[b];
  const long token = (j < a && j < K) ? ids[(size_t)b * (K + 1) + j + 1] : j == a ? recovery[b] : -1;
  out[t] = lp_pick(rows, ld, V, t, token, lse);
}

extern "C" int ssd_logprob_rows_ws_bytes(int T, int V) {
  if (T <= 0 || V <= 0 || V > SSD_LOGPROB_MAX_V) return SSD_ERR_SHAPE;
  const long bytes = (long)T * lp_slices(V) * LP_REC * 4;
  return bytes > 0x7fffffffL ? SSD_ERR_SHAPE : (int)bytes;
}

extern "C" int ssd_logprob_rows(const void* logits_rows, long ld, int T, int V, const int32_t* n_top, int rows_per_param, float* lse,
                                float* top_val, int32_t* top_id, void* raw_copy, long raw_ld, void* ws, void* stream) {
  if (T <= 0 || V <= 0 || rows_per_param <= 0 || ld < V || V > SSD_LOGPROB_MAX_V || (raw_copy && raw_ld < V) || T > 65535)
    return SSD_ERR_SHAPE;
  if (!logits_rows || !n_top || !lse || !ws || (!top_val) != (!top_id)) return SSD_ERR_ARG;
  const int S = lp_slices(V);
  hipLaunchKernelGGL(logprob_slice_kernel<false>, dim3(S, T), dim3(LP_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits_rows, ld, V, n_top,
                     rows_per_param, S, (bf16_t*)raw_copy, raw_ld, (const int64_t*)nullptr, (float*)ws);
  hipLaunchKernelGGL(logprob_merge_kernel<false>, dim3(T), dim3(64), 0, (hipStream_t)stream, (const float*)ws, n_top, rows_per_param, S, lse,
                     top_val, top_id, (const bf16_t*)nullptr, 0L, V, (const int64_t*)nullptr, (float*)nullptr, (int32_t*)nullptr);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_logprob_pick(const void* rows, long ld, int T, int V, const int64_t* tokens, const float* lse, const int32_t* n_top,
                                int rows_per_param, float* out, void* stream) {
  if (T <= 0 || V <= 0 || rows_per_param <= 0 || ld < V) return SSD_ERR_SHAPE;
  if (!rows || !tokens || !lse || !n_top || !out) return SSD_ERR_ARG;
  hipLaunchKernelGGL(logprob_pick_kernel, dim3((T + LP_THREADS - 1) / LP_THREADS), dim3(LP_THREADS), 0, (hipStream_t)stream,
                     (const bf16_t*)rows, ld, T, V, tokens, lse, n_top, rows_per_param, out);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_logprob_pick_verify(const void* rows, long ld, int B, int K, int V, const int64_t* ids, const int32_t* accept,
                                       const int64_t* recovery, const float* lse, const int32_t* n_top, float* out, void* stream) {
  if (B <= 0 || K < 0 || V <= 0 || ld < V) return SSD_ERR_SHAPE;
  if (!rows || !ids || !accept || !recovery || !lse || !n_top || !out) return SSD_ERR_ARG;
  const int T = B * (K + 1);
  hipLaunchKernelGGL(logprob_pick_verify_kernel, dim3((T + LP_THREADS - 1) / LP_THREADS), dim3(LP_THREADS), 0, (hipStream_t)stream,
                     (const bf16_t*)rows, ld, B, K, V, ids, accept, recovery, lse, n_top, out);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}
