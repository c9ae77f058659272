// Per-request seeds (include/ssd_hip_seed.h): the Gumbel-max sampler and the ratio verification drawing from a stream keyed by
// (seed, purpose, absolute position, index) instead of (rng word, salt, row, index), and the hook that exposes that stream.
//
// The sampler has the shape of logprob_slice_kernel + logprob_merge_kernel (logprob.hip), for the same reason: one workgroup per
// 128 K-entry row is a latency-bound launch on a few of the 256 CUs.  A row is cut into slices of 4096 entries; workgroup (row, slice)
// scores its 16 entries per thread -- logit / T + boost + Gumbel noise, the very expression of sample_rows_kernel -- and leaves the
// slice's best (score, index) in the workspace; one wave per row merges the candidates.  bmax (larger score, then lower index; a NaN
// score never wins) is a total order on what is comparable, so the winner is the one sample_rows_kernel finds, whatever the slicing.
// A seeded row computes its key once per workgroup from workgroup-uniform values and pays one mix64 per entry; an unseeded row pays
// the three of u01 and reproduces ssd_sample_rows bit for bit.
#include "common.h"
#include "stochastic.h"

constexpr int SD_THREADS = 256;
constexpr int SD_WAVES = SD_THREADS / 64;
constexpr int SD_PER = 2;                   // 8-entry chunks per thread
constexpr int SD_NONE = 0x7fffffff;         // index of "no candidate"
static_assert(SSD_SEED_SLICE == SD_THREADS * SD_PER * 8, "one slice = one workgroup's registers");

__global__ void __launch_bounds__(SD_THREADS)
sample_slice_kernel(const bf16_t* __restrict__ logits, long ld, int V, int S, int row0, const float* __restrict__ temps, int rows_per_temp,
                    const uint64_t* __restrict__ rng, uint32_t salt, const int32_t* __restrict__ boost_idx, int boost_k, float log_x,
                    const int64_t* __restrict__ row_seed, int rows_per_seed, const int64_t* __restrict__ positions, int purpose,
                    Best* __restrict__ ws) {
  __shared__ Best sm[SD_WAVES];
  const int row = row0 + (int)(blockIdx.x / (unsigned)S), sl = (int)(blockIdx.x % (unsigned)S), tid = threadIdx.x;
  const float T = temps[row / rows_per_temp];
  const int64_t own = row_seed[row / rows_per_seed];
  const bool seeded = own >= 0;
  const uint64_t word = *rng;
  const uint64_t key = seeded ? seed_key((uint64_t)own, purpose, (uint64_t)positions[row] + 1) : 0;
  const Boost bo = load_boost(boost_idx, row, boost_k, log_x);
  const bf16_t* x = logits + (size_t)row * ld;
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const float inv = 1.0f / fmaxf(T, 1e-8f);
  Best best = {-INFINITY, SD_NONE};
#pragma unroll
  for (int u = 0; u < SD_PER; ++u) {
    const long base = (((long)sl * SD_PER + u) * SD_THREADS + tid) * 8;
    if (base >= V) continue;
    uint32_t b[8];
    int n = 8;
    if (vec && base + 8 <= V) {
      const u32x4_t q = *reinterpret_cast<const u32x4_t*>(x + base);
#pragma unroll
      for (int e = 0; e < 4; ++e) { b[2 * e] = q[e] & 0xffffu; b[2 * e + 1] = q[e] >> 16; }
    } else {
      n = (int)(V - base < 8 ? V - base : 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) b[e] = e < n ? x[base + e] : 0;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (e >= n) break;
      const int i = (int)base + e;
      float s = bf2f(b[e]);
      if (T != 0.f) s = s * inv + bo.of(i) + gumbel(seeded ? seed_u(key, i) : u01(word, salt, row, i));
      best = bmax(best, Best{s, i});
    }
  }
  best = wave_best(best);
  if ((tid & 63) == 0) sm[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    Best r = sm[0];
#pragma unroll
    for (int w = 1; w < SD_WAVES; ++w) r = bmax(r, sm[w]);
    ws[(size_t)row * S + sl] = r;
  }
}

// one wave per row: the row's S candidates, lane by lane, then the shuffle tree
__global__ void __launch_bounds__(64)
sample_merge_kernel(const Best* __restrict__ ws, int S, int64_t* __restrict__ out, int64_t* __restrict__ out2) {
  const int row = blockIdx.x;
  const Best* c = ws + (size_t)row * S;
  Best best = {-INFINITY, SD_NONE};
  for (int s = threadIdx.x; s < S; s += 64) best = bmax(best, c[s]);
  best = wave_best(best);
  if (best.i == SD_NONE) best.i = 0;        // nothing comparable in the row (all NaN): as block_best
  if (threadIdx.x == 0) { out[row] = best.i; if (out2) out2[row] = best.i; }
}

static int sd_slices(int V) { return (int)(((long)V + SSD_SEED_SLICE - 1) / SSD_SEED_SLICE); }

extern "C" long ssd_sample_seeded_ws_bytes(int T, int V) {
  if (T <= 0 || V <= 0) return SSD_ERR_SHAPE;
  return (long)T * sd_slices(V) * (long)sizeof(Best);
}

extern "C" int ssd_sample_rows_seeded(const void* logits, long ld, int T, int V, const float* temps, int rows_per_temp,
                                      const void* rng_state, unsigned salt, int64_t* out, int64_t* out2, const int32_t* boost_idx,
                                      int boost_k, float boost_x, void* stream, const int64_t* row_seed, int rows_per_seed,
                                      const int64_t* positions, int purpose, void* workspace) {
  if (T <= 0 || V <= 0 || rows_per_temp <= 0 || rows_per_seed <= 0) return SSD_ERR_SHAPE;
  if (!logits || !temps || !rng_state || !out || !row_seed || !positions || !workspace) return SSD_ERR_ARG;
  if (purpose < SSD_SEED_DRAFT || purpose > SSD_SEED_ACCEPT) return SSD_ERR_ARG;
  if (boost_idx && (boost_k < 1 || boost_k > ST_MAXBOOST || !(boost_x > 0.f))) return SSD_ERR_ARG;
  const int S = sd_slices(V);
  const int per = 0x7fffffff / S;           // rows one launch's grid can hold (everything real is one launch)
  for (int row0 = 0; row0 < T; row0 += per) {
    const int rows = T - row0 < per ? T - row0 : per;
    hipLaunchKernelGGL(sample_slice_kernel, dim3((unsigned)rows * (unsigned)S), dim3(SD_THREADS), 0, (hipStream_t)stream,
                       (const bf16_t*)logits, ld, V, S, row0, temps, rows_per_temp, (const uint64_t*)rng_state, salt, boost_idx, boost_k,
                       boost_idx ? logf(boost_x) : 0.f, row_seed, rows_per_seed, positions, purpose, (Best*)workspace);
  }
  hipLaunchKernelGGL(sample_merge_kernel, dim3(T), dim3(64), 0, (hipStream_t)stream, (const Best*)workspace, S, out, out2);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_verify_ratio_seeded(const void* logits_p, long ld_p, const void* logits_q, long ld_q, int V, int B, int K,
                                       const int64_t* spec, const int64_t* preds_p, const float* lse_p, const float* lse_q,
                                       const float* temps_t, const float* temps_q, const int32_t* ratio_rows, const void* rng_state,
                                       unsigned salt, int32_t* accept_len, int64_t* recovery, int64_t* packed, float* accept_prob,
                                       const int32_t* boost_idx_q, int boost_k, float boost_x, void* stream, const int64_t* row_seed,
                                       const int64_t* positions) {
  if (B <= 0 || K < 1 || K > 62 || V <= 0) return SSD_ERR_SHAPE;
  if (boost_idx_q && (boost_k < 1 || boost_k > ST_MAXBOOST || !(boost_x > 0.f))) return SSD_ERR_ARG;
  if (!row_seed || !positions) return SSD_ERR_ARG;
  hipLaunchKernelGGL(verify_ratio_kernel<true>, dim3(B), dim3(ST_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits_p, ld_p,
                     (const bf16_t*)logits_q, ld_q, V, K, spec, preds_p, lse_p, lse_q, temps_t, temps_q, ratio_rows,
                     (const uint64_t*)rng_state, salt, accept_len, recovery, packed, accept_prob, boost_idx_q, boost_k,
                     boost_idx_q ? logf(boost_x) : 0.f, row_seed, positions);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

__global__ void __launch_bounds__(SD_THREADS)
seeded_uniforms_kernel(const int64_t* __restrict__ row_seed, const int64_t* __restrict__ positions, int purpose, uint32_t idx0, int n,
                       float* __restrict__ out) {
  const int r = blockIdx.y;
  const int j = blockIdx.x * SD_THREADS + threadIdx.x;
  if (j >= n) return;
  const int64_t own = row_seed[r];
  out[(size_t)r * n + j] = own >= 0 ? seed_u(seed_key((uint64_t)own, purpose, (uint64_t)positions[r] + 1), idx0 + (uint32_t)j)
                                    : __builtin_nanf("");
}

extern "C" int ssd_seeded_uniforms(const int64_t* row_seed, const int64_t* positions, int rows, int purpose, unsigned idx0, int n,
                                   float* out, void* stream) {
  if (rows <= 0 || n <= 0 || (unsigned long long)idx0 + (unsigned long long)n > (1ull << 32)) return SSD_ERR_SHAPE;
  if (!row_seed || !positions || !out) return SSD_ERR_ARG;
  if (purpose < SSD_SEED_DRAFT || purpose > SSD_SEED_ACCEPT) return SSD_ERR_ARG;
  const int nx = (n + SD_THREADS - 1) / SD_THREADS;
  for (int r0 = 0; r0 < rows; r0 += 65535) {        // grid.y holds 65535 rows
    const int part = rows - r0 < 65535 ? rows - r0 : 65535;
    hipLaunchKernelGGL(seeded_uniforms_kernel, dim3(nx, part), dim3(SD_THREADS), 0, (hipStream_t)stream, row_seed + r0, positions + r0,
                       purpose, idx0, n, out + (size_t)r0 * n);
  }
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}
