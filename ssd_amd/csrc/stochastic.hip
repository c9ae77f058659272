// Temperature > 0: sampling and ratio-based speculative verification.
//  * ssd_sample_rows    Sampler.forward (reference ssd/layers/sampler.py:15-36): temperature 0 -> argmax, else a draw
//                       from softmax(logits / T).  The reference draws argmax(p / Exp(1)); that is the Gumbel-max trick,
//                       so here it is argmax(logit / T + Gumbel) in ONE pass, no softmax, no V-sized temporaries.
//  * ssd_row_lse        log-sum-exp of logits / T per row (the softmax normaliser verify() needs, verify.py:76-99).
//  * ssd_verify_ratio   verify() for rows with temperature > 0 (reference ssd/utils/verify.py:50-167):
//                       accept x_i with probability min(1, p_i(x_i) / q_i(x_i)); at the first rejection n draw the
//                       recovery token from normalise(max(0, p_n - q_n)); if everything was accepted (or the row is not
//                       a "ratio row": cache miss without JIT) draw it from p_n; temperature-0 rows take the greedy branch.
// Randomness is a counter-based hash of (seed word in device memory, stream salt, row, index): launches inside a
// hipGraph stay fresh because the seed word is advanced on the device (ssd_rng_advance) after every use.
#include "common.h"
#include "stochastic.h"     // the hash, the streams, Best / Boost, the block reductions, verify_ratio_kernel

// out[row][0..k) = indices of the k largest logits of the row, largest first, lowest index on ties
__global__ void __launch_bounds__(ST_THREADS)
topk_rows_kernel(const bf16_t* __restrict__ logits, long ld, int V, int k, int32_t* __restrict__ out) {
  __shared__ Best sm[ST_THREADS / 64];
  __shared__ int chosen[ST_MAXBOOST];
  const int row = blockIdx.x;
  const bf16_t* x = logits + (size_t)row * ld;
  for (int r = 0; r < k; ++r) {
    Best best = {-INFINITY, 0x7fffffff};
    for (int i = threadIdx.x; i < V; i += ST_THREADS) {
      bool taken = false;
      for (int j = 0; j < r; ++j) taken = taken || chosen[j] == i;
      if (!taken) best = bmax(best, Best{bf2f(x[i]), i});
    }
    best = block_best<ST_THREADS>(best, sm);
    if (threadIdx.x == 0) { chosen[r] = best.i; out[(size_t)row * k + r] = best.i; }
    __syncthreads();
  }
}

extern "C" int ssd_topk_rows(const void* logits, long ld, int T, int V, int k, int32_t* out, void* stream) {
  if (T <= 0 || V <= 0 || k < 1 || k > ST_MAXBOOST || k > V) return SSD_ERR_SHAPE;
  hipLaunchKernelGGL(topk_rows_kernel, dim3(T), dim3(ST_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits, ld, V, k, out);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

__global__ void __launch_bounds__(ST_THREADS)
sample_rows_kernel(const bf16_t* __restrict__ logits, long ld, int V, const float* __restrict__ temps, int rows_per_temp,
                   const uint64_t* __restrict__ rng, uint32_t salt, int64_t* __restrict__ out, int64_t* __restrict__ out2,
                   const int32_t* __restrict__ boost_idx, int boost_k, float log_x) {
  __shared__ Best sm[ST_THREADS / 64];
  const int row = blockIdx.x;
  const float T = temps[row / rows_per_temp];
  const Boost bo = load_boost(boost_idx, row, boost_k, log_x);
  const bf16_t* x = logits + (size_t)row * ld;
  const uint64_t seed = *rng;
  Best best = {-INFINITY, 0x7fffffff};
  if (T == 0.f) {
    for (int i = threadIdx.x; i < V; i += ST_THREADS) best = bmax(best, Best{bf2f(x[i]), i});
  } else {
    const float inv = 1.0f / fmaxf(T, 1e-8f);
    for (int i = threadIdx.x; i < V; i += ST_THREADS)
      best = bmax(best, Best{bf2f(x[i]) * inv + bo.of(i) + gumbel(u01(seed, salt, row, i)), i});
  }
  best = block_best<ST_THREADS>(best, sm);
  if (threadIdx.x == 0) { out[row] = best.i; if (out2) out2[row] = best.i; }
}

extern "C" int ssd_sample_rows(const void* logits, long ld, int T, int V, const float* temps, int rows_per_temp,
                               const void* rng_state, unsigned salt, int64_t* out, int64_t* out2, const int32_t* boost_idx,
                               int boost_k, float boost_x, void* stream) {
  if (T <= 0 || V <= 0 || rows_per_temp <= 0) return SSD_ERR_SHAPE;
  if (boost_idx && (boost_k < 1 || boost_k > ST_MAXBOOST || !(boost_x > 0.f))) return SSD_ERR_ARG;
  hipLaunchKernelGGL(sample_rows_kernel, dim3(T), dim3(ST_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits, ld, V,
                     temps, rows_per_temp, (const uint64_t*)rng_state, salt, out, out2, boost_idx, boost_k,
                     boost_idx ? logf(boost_x) : 0.f);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

__global__ void rng_advance_kernel(uint64_t* rng) { *rng = mix64(*rng + 0x632be59bd9b4e019ull); }
extern "C" int ssd_rng_advance(void* rng_state, void* stream) {
  if (!rng_state) return SSD_ERR_ARG;
  hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (uint64_t*)rng_state);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// lse[row] = log(sum_v exp(logit_v / T - m)) + m with m = max_v logit_v / T  (rows with T == 0 get lse = +inf marker 0)
__global__ void __launch_bounds__(ST_THREADS)
row_lse_kernel(const bf16_t* __restrict__ logits, long ld, int V, const float* __restrict__ temps, int rows_per_temp,
               float* __restrict__ lse, const int32_t* __restrict__ boost_idx, int boost_k, float log_x) {
  __shared__ float sm[ST_THREADS / 64];
  const int row = blockIdx.x;
  const float T = temps[row / rows_per_temp];
  if (T == 0.f) { if (threadIdx.x == 0) lse[row] = 0.f; return; }
  const float inv = 1.0f / fmaxf(T, 1e-8f);
  const bf16_t* x = logits + (size_t)row * ld;
  const Boost bo = load_boost(boost_idx, row, boost_k, log_x);
  float m = -INFINITY;
  for (int i = threadIdx.x; i < V; i += ST_THREADS) m = fmaxf(m, bf2f(x[i]) * inv + bo.of(i));
  m = block_max<ST_THREADS>(m, sm);
  float s = 0.f;
  for (int i = threadIdx.x; i < V; i += ST_THREADS) s += __expf(bf2f(x[i]) * inv + bo.of(i) - m);
  s = block_sum<ST_THREADS>(s, sm);
  if (threadIdx.x == 0) lse[row] = __logf(s) + m;
}

extern "C" int ssd_row_lse(const void* logits, long ld, int T, int V, const float* temps, int rows_per_temp, float* lse,
                           const int32_t* boost_idx, int boost_k, float boost_x, void* stream) {
  if (T <= 0 || V <= 0 || rows_per_temp <= 0) return SSD_ERR_SHAPE;
  if (boost_idx && (boost_k < 1 || boost_k > ST_MAXBOOST || !(boost_x > 0.f))) return SSD_ERR_ARG;
  hipLaunchKernelGGL(row_lse_kernel, dim3(T), dim3(ST_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits, ld, V, temps,
                     rows_per_temp, lse, boost_idx, boost_k, boost_idx ? logf(boost_x) : 0.f);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_verify_ratio(const void* logits_p, long ld_p, const void* logits_q, long ld_q, int V, int B, int K,
                                const int64_t* spec, const int64_t* preds_p, const float* lse_p, const float* lse_q,
                                const float* temps_t, const float* temps_q, const int32_t* ratio_rows, const void* rng_state,
                                unsigned salt, int32_t* accept_len, int64_t* recovery, int64_t* packed, float* accept_prob,
                                const int32_t* boost_idx_q, int boost_k, float boost_x, void* stream) {
  if (B <= 0 || K < 1 || K > 62 || V <= 0) return SSD_ERR_SHAPE;
  if (boost_idx_q && (boost_k < 1 || boost_k > ST_MAXBOOST || !(boost_x > 0.f))) return SSD_ERR_ARG;
  hipLaunchKernelGGL(verify_ratio_kernel<false>, dim3(B), dim3(ST_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits_p, ld_p,
                     (const bf16_t*)logits_q, ld_q, V, K, spec, preds_p, lse_p, lse_q, temps_t, temps_q, ratio_rows,
                     (const uint64_t*)rng_state, salt, accept_len, recovery, packed, accept_prob, boost_idx_q, boost_k,
                     boost_idx_q ? logf(boost_x) : 0.f, (const int64_t*)nullptr, (const int64_t*)nullptr);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}
