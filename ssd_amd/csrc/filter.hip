// Top-k / top-p / min-p truncation of sampled logit rows (include/ssd_hip_filter.h): the rows are filtered in place, dropped entries
// become -inf, and the samplers of stochastic.hip run on them unchanged.
//
// One workgroup of 1024 threads per row, as ssd_sample_rows / ssd_row_lse.  Every filter is "value >= threshold", and a bf16 value
// has an order-preserving 16-bit key, so the kernel only has to find one key:
//   pass A       largest key and number of comparable (non-NaN) entries
//   top_k        t_k = the largest key v with count(key >= v) >= k: interval search, FT_PROBES - 1 new probes per pass over the
//                row (each pass quarters the interval: at most 8 passes for 65536 keys), integer counts
//   top_p        t_p = the largest key v >= t_k with mass(key >= v) >= top_p * mass(key >= t_k): the same search over
//                [t_k, max]; the first pass also yields the mass of K; entries below the interval's lower end skip the exp
//   min_p        t_m = the smallest key whose e = exp(s - m) reaches min_p: e depends on the value alone, so this is a search over
//                keys in registers, without a pass over the row
//   last pass    entries with key < max(t_k, t_p, t_m) and NaNs are overwritten with -inf; the survivors are counted
// The row (256 KB at V = 128256) stays in L2 between the passes.  A thread always owns the same 8-entry chunks, whether the row is
// 16-byte aligned (one 16-byte load per chunk) or not (eight 2-byte loads), and adds its entries in index order; the 1024 partial
// sums meet in a shuffle tree and a fixed-order sum over the 16 waves.  No atomics: the result is the same bits on every run.
#include "common.h"

constexpr int FT_THREADS = 1024;
constexpr int FT_WAVES = FT_THREADS / 64;
constexpr int FT_PROBES = 4;                    // thresholds per pass: the interval's lower end + 3 new ones
constexpr uint32_t FT_NEG_INF = 0xff80u;        // bf16 -inf
constexpr int FT_KEY_NEG_INF = 0x007f;          // the smallest and the largest key of a comparable value
constexpr int FT_KEY_POS_INF = 0xff80;
static_assert(SSD_FILTER_MAX_V == FT_THREADS * 8 * 24, "192 terms per thread");

__device__ __forceinline__ bool ft_nan(uint32_t b) { return (b & 0x7fffu) > 0x7f80u; }
// a < b as values <=> key(a) < key(b); -0.0 and +0.0 share a key (they are one value)
__device__ __forceinline__ int ft_key(uint32_t b) {
  if (b == 0x8000u) b = 0;
  return (int)((b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u));
}
__device__ __forceinline__ uint32_t ft_bits(int key) { return (key & 0x8000) ? (uint32_t)(key & 0x7fff) : (~(uint32_t)key & 0xffffu); }

// f(bits) for every entry of the row; WRITE: f returns the entry's new bits.  Chunk c = entries [8c, 8c + 8) belongs to thread c % 1024.
template <bool WRITE, class F>
__device__ __forceinline__ void ft_each(bf16_t* x, int V, bool vec, F f) {
  const int nchunks = (V + 7) >> 3;
  for (int c = threadIdx.x; c < nchunks; c += FT_THREADS) {
    const int base = c << 3;
    if (vec && base + 8 <= V) {
      const u32x4_t v = *reinterpret_cast<const u32x4_t*>(x + base);
      u32x4_t o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t lo = f(v[j] & 0xffffu);
        const uint32_t hi = f(v[j] >> 16);
        o[j] = lo | (hi << 16);
      }
      if (WRITE && (o[0] != v[0] || o[1] != v[1] || o[2] != v[2] || o[3] != v[3])) *reinterpret_cast<u32x4_t*>(x + base) = o;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (base + j < V) {
          const uint32_t b = x[base + j];
          const uint32_t n = f(b);
          if (WRITE && n != b) x[base + j] = (bf16_t)n;
        }
      }
    }
  }
}

// a[p] = sum over the workgroup, the same bits in every thread: shuffle tree inside a wave, then the 16 waves in order
template <class TV>
__device__ __forceinline__ void ft_sum(TV (&a)[FT_PROBES], TV* sm) {
#pragma unroll
  for (int p = 0; p < FT_PROBES; ++p) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a[p] += __shfl_xor(a[p], o, 64);
  }
  __syncthreads();          // the readers of the previous sum are done with sm
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int p = 0; p < FT_PROBES; ++p) sm[p * FT_WAVES + (threadIdx.x >> 6)] = a[p];
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < FT_PROBES; ++p) {
    TV r = sm[p * FT_WAVES];
    for (int w = 1; w < FT_WAVES; ++w) r += sm[p * FT_WAVES + w];
    a[p] = r;
  }
}

// The largest key v in [lo, hi) for which the predicate holds; it holds at lo, fails at hi and is monotone in v (a count, or an fp32
// sum of non-negative terms added in a fixed order, never grows when terms leave it).
//   MASS = false: count(key >= v) >= k          MASS = true: mass(key >= v) >= top_p * mass(key >= lo)
template <bool MASS>
__device__ int ft_search(bf16_t* x, int V, bool vec, int lo, int hi, int k, float top_p, float inv, float m, float* smf, int* smi) {
  float target = 0.f;
  bool first = true;
  while (hi - lo > 1) {
    const int q = (hi - lo + 3) >> 2;
    const int t[FT_PROBES] = {lo, min(lo + q, hi), min(lo + 2 * q, hi), min(lo + 3 * q, hi)};
    bool ok[FT_PROBES];
    if (MASS) {
      float a[FT_PROBES] = {0.f, 0.f, 0.f, 0.f};
      ft_each<false>(x, V, vec, [&](uint32_t b) {
        const int key = ft_key(b);
        if (!ft_nan(b) && key >= lo) {
          const float e = __expf(bf2f(b) * inv - m);
#pragma unroll
          for (int p = 0; p < FT_PROBES; ++p) a[p] += key >= t[p] ? e : 0.f;
        }
        return b;
      });
      ft_sum(a, smf);
      if (first) target = top_p * a[0];
      first = false;
#pragma unroll
      for (int p = 0; p < FT_PROBES; ++p) ok[p] = a[p] >= target;
    } else {
      int a[FT_PROBES] = {0, 0, 0, 0};
      ft_each<false>(x, V, vec, [&](uint32_t b) {
        const int key = ft_key(b);
        if (!ft_nan(b)) {
#pragma unroll
          for (int p = 0; p < FT_PROBES; ++p) a[p] += key >= t[p] ? 1 : 0;
        }
        return b;
      });
      ft_sum(a, smi);
#pragma unroll
      for (int p = 0; p < FT_PROBES; ++p) ok[p] = a[p] >= k;
    }
    int nlo = lo, nhi = hi;
    for (int p = 1; p < FT_PROBES; ++p) {
      if (ok[p]) nlo = t[p];
      else { nhi = t[p]; break; }
    }
    lo = nlo;
    hi = nhi;
  }
  return lo;
}

__global__ void __launch_bounds__(FT_THREADS)
filter_rows_kernel(bf16_t* __restrict__ logits, long ld, int V, const float* __restrict__ temps, const int32_t* __restrict__ top_k,
                   const float* __restrict__ top_p, const float* __restrict__ min_p, int rows_per_param, int32_t* __restrict__ kept) {
  __shared__ float smf[FT_PROBES * FT_WAVES];
  __shared__ int smi[FT_PROBES * FT_WAVES];
  const int row = blockIdx.x;
  const int pi = row / rows_per_param;
  const float T = temps[pi];
  const int k = top_k[pi];
  const float tp = top_p[pi], mp = min_p[pi];
  const bool k_on = k > 0 && k < V, p_on = tp < 1.0f, m_on = mp > 0.0f;
  if (T == 0.f || !(k_on || p_on || m_on)) {
    if (kept && threadIdx.x == 0) kept[row] = V;
    return;
  }
  bf16_t* x = logits + (size_t)row * ld;
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;

  // ---- pass A: the largest key, the number of comparable entries ----
  int maxkey = -1;
  int cnt[FT_PROBES] = {0, 0, 0, 0};
  ft_each<false>(x, V, vec, [&](uint32_t b) {
    if (!ft_nan(b)) { maxkey = max(maxkey, ft_key(b)); ++cnt[0]; }
    return b;
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) maxkey = max(maxkey, __shfl_xor(maxkey, o, 64));
  if ((threadIdx.x & 63) == 0) smi[threadIdx.x >> 6] = maxkey;
  __syncthreads();
  for (int w = 0; w < FT_WAVES; ++w) maxkey = max(maxkey, smi[w]);
  ft_sum(cnt, smi);         // (its first barrier also ends the reads of smi above)
  const int nc = cnt[0];
  if (nc == 0) {            // nothing comparable: the row is left as it is
    if (kept && threadIdx.x == 0) kept[row] = V;
    return;
  }
  const float inv = 1.0f / fmaxf(T, 1e-8f);
  const float m = bf2f(ft_bits(maxkey)) * inv;
  const bool finite = maxkey != FT_KEY_POS_INF && maxkey != FT_KEY_NEG_INF;

  int thr = FT_KEY_NEG_INF;
  if (k_on && k < nc) thr = ft_search<false>(x, V, vec, thr, maxkey + 1, k, 0.f, inv, m, smf, smi);
  if (p_on) thr = finite ? ft_search<true>(x, V, vec, thr, maxkey + 1, 0, tp, inv, m, smf, smi) : maxkey;
  if (m_on) {
    int lo = FT_KEY_NEG_INF - 1, hi = maxkey;      // e(lo) < min_p (sentinel), e(max) = 1 >= min_p
    while (finite && hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (__expf(bf2f(ft_bits(mid)) * inv - m) >= mp) hi = mid;
      else lo = mid;
    }
    thr = max(thr, hi);
  }
  thr = min(thr, maxkey);   // the class of the maximum always stays

  // ---- last pass: drop what lies below the threshold, count what stays ----
  int n[FT_PROBES] = {0, 0, 0, 0};
  ft_each<true>(x, V, vec, [&](uint32_t b) {
    const bool keep = !ft_nan(b) && ft_key(b) >= thr;
    n[0] += keep ? 1 : 0;
    return keep ? b : FT_NEG_INF;
  });
  if (kept) {
    ft_sum(n, smi);
    if (threadIdx.x == 0) kept[row] = n[0];
  }
}

extern "C" int ssd_filter_rows(void* logits_rows, long ld, int T, int V, const float* temps, const int32_t* top_k, const float* top_p,
                               const float* min_p, int rows_per_param, int32_t* kept, void* stream) {
  if (T <= 0 || V <= 0 || rows_per_param <= 0 || ld < V || V > SSD_FILTER_MAX_V) return SSD_ERR_SHAPE;
  if (!logits_rows || !temps || !top_k || !top_p || !min_p) return SSD_ERR_ARG;
  hipLaunchKernelGGL(filter_rows_kernel, dim3(T), dim3(FT_THREADS), 0, (hipStream_t)stream, (bf16_t*)logits_rows, ld, V, temps, top_k,
                     top_p, min_p, rows_per_param, kept);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}
