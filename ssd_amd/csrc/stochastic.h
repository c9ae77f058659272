// Device helpers of the temperature > 0 kernels, shared by stochastic.hip (one workgroup per row, the engine's rng word) and seeded.hip
// (per-request seeds, rows cut into slices): the hash, both random streams, the (score, index) order, the sampler_x boost and the
// ratio verification, which exists once and is instantiated with and without per-sequence seeds.
#pragma once
#include "common.h"
#include "ssd_hip_seed.h"

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// uniform in (0, 1), 24 bits.  The key word holds salt[0:24) | row[0:8) | idx, one field per bit range; whatever of salt and row does
// not fit (row >= 256: the tree step samples B * mq rows; salt >= 2^24) goes through a mix64 round of its own, so (salt, row, idx)
// -> stream is injective up to the hash and row 256 under salt s is no longer row 0 under salt s + 1.  Rows < 256 under salts
// < 2^24 (everything the engine drew before) keep their streams bit for bit.
__device__ __forceinline__ float u01(uint64_t seed, uint32_t salt, uint32_t row, uint32_t idx) {
  uint64_t z = mix64(((uint64_t)(salt & 0xffffffu) << 40) ^ ((uint64_t)(row & 0xffu) << 32) ^ idx);
  const uint64_t hi = ((uint64_t)(salt >> 24) << 24) | (row >> 8);
  if (hi) z = mix64(z ^ hi);
  const uint64_t h = mix64(seed ^ z);
  return ((float)(h >> 40) + 0.5f) * (1.0f / 16777216.0f);
}
// The stream of a request with a seed (include/ssd_hip_seed.h): one key per (seed, purpose, absolute position of the token being
// decided), one mix64 per number.  Nothing of the launch (rng word, salt, row) enters.
__device__ __forceinline__ uint64_t seed_key(uint64_t seed, int purpose, uint64_t pos) {
  return mix64(mix64(seed) ^ ((uint64_t)purpose << 56) ^ pos);
}
__device__ __forceinline__ float seed_u(uint64_t key, uint32_t idx) {
  return ((float)(mix64(key ^ idx) >> 40) + 0.5f) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ float gumbel(float u) { return -__logf(-__logf(u)); }

struct Best { float v; int i; };
__device__ __forceinline__ Best bmax(Best a, Best b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ Best wave_best(Best best) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = bmax(best, Best{__shfl_xor(best.v, o, 64), __shfl_xor(best.i, o, 64)});
  return best;
}

template <int THREADS>
__device__ Best block_best(Best best, Best* sm) {
  best = wave_best(best);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = best;
  __syncthreads();
  Best r = sm[0];
  for (int w = 1; w < THREADS / 64; ++w) r = bmax(r, sm[w]);
  if (r.i == 0x7fffffff) r.i = 0;   // nothing comparable in the row (all NaN): never emit the sentinel as a token id (as block_row_argmax)
  return r;
}
template <int THREADS>
__device__ float block_sum(float v, float* sm) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  for (int w = 0; w < THREADS / 64; ++w) r += sm[w];
  return r;
}
template <int THREADS>
__device__ float block_max(float v, float* sm) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sm[0];
  for (int w = 1; w < THREADS / 64; ++w) r = fmaxf(r, sm[w]);
  return r;
}

constexpr int ST_THREADS = 1024;
constexpr int ST_MAXBOOST = 8;      // sampler_x rescales the F+1 largest probabilities; F+1 <= 8

// sampler_x (reference apply_sampler_x_rescaling, async_spec_helpers.py:79-105): the F+1 most probable tokens of a row
// get their probability multiplied by x before renormalisation.  In log space that is "+ log x" on those logits: a Gumbel
// draw and a log-sum-exp over the boosted logits are exactly the rescaled, renormalised distribution.
struct Boost {
  int idx[ST_MAXBOOST];
  int k;
  float log_x;
  __device__ __forceinline__ float of(int i) const {
    float b = 0.f;
#pragma unroll
    for (int j = 0; j < ST_MAXBOOST; ++j) b = (j < k && idx[j] == i) ? log_x : b;
    return b;
  }
};
__device__ __forceinline__ Boost load_boost(const int32_t* __restrict__ boost_idx, int row, int k, float log_x) {
  Boost b;
  b.k = boost_idx ? k : 0;
  b.log_x = log_x;
#pragma unroll
  for (int j = 0; j < ST_MAXBOOST; ++j) b.idx[j] = (boost_idx && j < k) ? boost_idx[(size_t)row * k + j] : -1;
  return b;
}

// One workgroup per sequence.
//   logits_p [B][K+1][ld_p], logits_q [B][K][ld_q]; spec [B][K+1] = (recovery, x_1..x_K); preds_p [B][K+1] = argmax rows of p;
//   lse_p [B][K+1], lse_q [B][K] from ssd_row_lse; temps_t / temps_q [B]; ratio_rows int32[B] (1: the draft tokens really
//   were sampled from q -- cache hit, or JIT speculation; 0: fall back to greedy acceptance and draw the recovery from p).
// Outputs as ssd_verify_greedy (+ accept_prob [B][K] for inspection when not null).
// SEEDED (ssd_verify_ratio_seeded): a sequence with row_seed[b] >= 0 takes the acceptance uniform of draft token x_{i+1} from
// (seed, SSD_SEED_ACCEPT, positions[b][i] + 1) at index 0 and the Gumbel noise of the recovery token at row n from
// (seed, SSD_SEED_TARGET, positions[b][n] + 1); every other sequence, and the whole instantiation without SEEDED, draws from
// (rng word, salt, b) as ever.  Nothing else differs, so whatever is deterministic is the same bits in both.
template <bool SEEDED>
__global__ void __launch_bounds__(ST_THREADS)
verify_ratio_kernel(const bf16_t* __restrict__ lp, long ld_p, const bf16_t* __restrict__ lq, long ld_q, int V, int K,
                    const int64_t* __restrict__ spec, const int64_t* __restrict__ preds_p, const float* __restrict__ lse_p,
                    const float* __restrict__ lse_q, const float* __restrict__ temps_t, const float* __restrict__ temps_q,
                    const int32_t* __restrict__ ratio_rows, const uint64_t* __restrict__ rng, uint32_t salt,
                    int32_t* __restrict__ accept_len, int64_t* __restrict__ recovery, int64_t* __restrict__ packed,
                    float* __restrict__ accept_prob, const int32_t* __restrict__ boost_idx_q, int boost_k, float log_x,
                    const int64_t* __restrict__ row_seed, const int64_t* __restrict__ positions) {
  __shared__ Best smb[ST_THREADS / 64];
  __shared__ float smf[ST_THREADS / 64];
  __shared__ int s_n;
  const int b = blockIdx.x;
  const float Tt = temps_t[b], Tq = temps_q[b];
  const uint64_t seed = *rng;
  int64_t own = -1;                                 // the sequence's own seed, or < 0: the engine's stream
  if (SEEDED) own = row_seed[b];
  const int64_t* sp = spec + (size_t)b * (K + 1);
  const int64_t* pr = preds_p + (size_t)b * (K + 1);
  const bool ratio = (Tt > 0.f || Tq > 0.f) && ratio_rows[b] != 0;
  const float inv_t = 1.0f / fmaxf(Tt, 1e-8f), inv_q = 1.0f / fmaxf(Tq, 1e-8f);
  // ---- acceptance: one lane per draft position, first rejection by ballot ----
  if (threadIdx.x < 64) {
    const int i = threadIdx.x;
    bool reject = false;
    if (i < K) {
      const int x = (int)sp[i + 1];
      if (ratio) {
        // p_i(x): softmax(logits_p / Tt) (one-hot at the argmax when Tt == 0); q_i(x) likewise
        const float pv = Tt > 0.f ? __expf(bf2f(lp[((size_t)b * (K + 1) + i) * ld_p + x]) * inv_t - lse_p[b * (K + 1) + i])
                                  : (pr[i] == x ? 1.f : 0.f);
        float qv;
        if (Tq > 0.f) {   // lse_q already carries the sampler_x boost (ssd_row_lse with the same boost rows)
          const Boost bo = load_boost(boost_idx_q, b * K + i, boost_k, log_x);
          qv = __expf(bf2f(lq[((size_t)b * K + i) * ld_q + x]) * inv_q + bo.of(x) - lse_q[b * K + i]);
        }
        else qv = 1.f;   // a greedy draft proposed its own argmax: q is one-hot at x
        const float a = fminf(pv / (qv + 1e-10f), 1.0f);
        if (accept_prob) accept_prob[b * K + i] = a;
        const float u = (SEEDED && own >= 0)
                            ? seed_u(seed_key((uint64_t)own, SSD_SEED_ACCEPT, (uint64_t)positions[(size_t)b * (K + 1) + i] + 1), 0)
                            : u01(seed, salt, b, 1000 + i);
        reject = !(u <= a);
      } else {
        if (accept_prob) accept_prob[b * K + i] = (pr[i] == x) ? 1.f : 0.f;
        reject = pr[i] != x;
      }
    }
    const unsigned long long mask = __ballot(reject);
    if (i == 0) s_n = mask ? (int)__builtin_ctzll(mask) : K;
  }
  __syncthreads();
  const int n = s_n;
  // ---- recovery token ----
  int64_t rec;
  if (Tt == 0.f) {
    rec = pr[n];                                    // greedy target: argmax of row n
  } else {
    const bf16_t* prow = lp + ((size_t)b * (K + 1) + n) * ld_p;
    const float lsep = lse_p[b * (K + 1) + n];
    const bool adjust = ratio && n < K;
    const uint64_t tkey = (SEEDED && own >= 0) ? seed_key((uint64_t)own, SSD_SEED_TARGET, (uint64_t)positions[(size_t)b * (K + 1) + n] + 1) : 0;
    auto noise = [&](int v) { return gumbel((SEEDED && own >= 0) ? seed_u(tkey, v) : u01(seed, salt, b, 5000 + v)); };
    Best best = {-INFINITY, 0x7fffffff};
    bool use_p = !adjust;
    if (adjust) {
      // residual r_v = max(0, p_v - q_v); if it vanishes everywhere fall back to p (verify.py:153-155)
      const bf16_t* qrow = lq + ((size_t)b * K + n) * ld_q;
      const float lseq = lse_q[b * K + n];
      const int xq = (int)sp[n + 1];
      const Boost bo = load_boost(boost_idx_q, b * K + n, boost_k, log_x);
      float tot = 0.f;
      for (int v = threadIdx.x; v < V; v += ST_THREADS) {
        const float pv = __expf(bf2f(prow[v]) * inv_t - lsep);
        const float qv = Tq > 0.f ? __expf(bf2f(qrow[v]) * inv_q + bo.of(v) - lseq) : (v == xq ? 1.f : 0.f);
        const float r = fmaxf(pv - qv, 0.f);
        tot += r;
        if (r > 0.f) best = bmax(best, Best{__logf(r) + noise(v), v});
      }
      tot = block_sum<ST_THREADS>(tot, smf);
      if (!(tot > 0.f)) use_p = true;
    }
    if (use_p) {
      best = Best{-INFINITY, 0x7fffffff};
      for (int v = threadIdx.x; v < V; v += ST_THREADS)
        best = bmax(best, Best{bf2f(prow[v]) * inv_t + noise(v), v});
    }
    best = block_best<ST_THREADS>(best, smb);
    rec = best.i;
  }
  if (threadIdx.x == 0) {
    accept_len[b] = n;
    recovery[b] = rec;
  }
  if (packed) {
    int64_t* row = packed + (size_t)b * (K + 3);
    if (threadIdx.x == 0) { row[0] = n; row[1] = rec; }
    if (threadIdx.x <= K) row[2 + threadIdx.x] = sp[threadIdx.x];
  }
}
