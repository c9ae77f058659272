// The slice and merge kernels of the log-probability family, shared by logprob.hip (include/ssd_hip_logprob.h: the rows of a decode or
// verify step, whose token is chosen after the row is read) and prompt_logprob.hip (include/ssd_hip_prompt_logprob.h: prompt rows, whose
// token is known before).  Each exists once and is instantiated with and without the known token (KNOWN).
//
// The shape of fork_slice_kernel + fork_merge_kernel (sample.hip), for the same reason: one workgroup per 128 K-entry row is a
// latency-bound launch on a few of the 256 CUs.  A row is cut into S slices of 4096 entries; workgroup (slice, row) loads its slice
// once (16 values per thread) and leaves
//   (max, sum exp(x - max), number of comparable entries)   and   the slice's top-n candidates (larger value, then lower index)
// in the workspace, and stores the copy from the registers it already holds.  One wave per row then merges the S triples (one lane per
// slice, shuffle trees) and the S sorted candidate lists (every lane holds the head of its slice's list; the winner's lane moves on).
// The top-n of a union is the top-n of the per-slice top-ns, and ties resolve by index in both stages, also across slice borders.
// A thread always owns the same two 8-entry chunks, whether the row is 16-byte aligned (one 16-byte load per chunk) or not (eight
// 2-byte loads), and adds its entries in index order.  No atomics: the result is the same bits on every run.
//
// KNOWN adds, in the same pass over the same registers: every thread of a slice reads x[token] (one uniform address) and counts its own
// comparable entries >= it; the slice's count travels in word 3 of its record, and the merge adds the counts (integers: the rank is
// exact) and writes the token's log-probability from the lse it has just computed.  Nothing of the KNOWN = false instantiation changes.
#pragma once
#include "common.h"

constexpr int LP_THREADS = 256;
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr int LP_PER = 2;                                           // 8-entry chunks per thread
constexpr int LP_MAXN = SSD_LOGPROB_MAX_N;
constexpr int LP_MAXS = SSD_LOGPROB_MAX_V / SSD_LOGPROB_SLICE;      // 48 slices: one lane each in the merge
// words per (row, slice): max, sum, count, the count of entries >= the known token (a pad without one), values, indices
constexpr int LP_REC = 4 + 2 * LP_MAXN;
constexpr int LP_NONE = 0x7fffffff;                                 // index of "no candidate"
static_assert(SSD_LOGPROB_SLICE == LP_THREADS * LP_PER * 8, "one slice = one workgroup's registers");
static_assert(LP_MAXS * SSD_LOGPROB_SLICE == SSD_LOGPROB_MAX_V && LP_MAXS <= 64, "one lane per slice");

struct LpBest { float v; int i; };
// larger value, then lower index; {-inf, LP_NONE} loses against every entry, a -inf one included
__device__ __forceinline__ LpBest lp_better(LpBest a, LpBest b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ LpBest lp_wave_best(LpBest a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = lp_better(a, LpBest{__shfl_xor(a.v, o, 64), __shfl_xor(a.i, o, 64)});
  return a;
}
__device__ __forceinline__ bool lp_nan(uint32_t b) { return (b & 0x7fffu) > 0x7f80u; }
// the count of row group `pi`, or -1 (skip) for anything outside 0..SSD_LOGPROB_MAX_N
__device__ __forceinline__ int lp_count(const int32_t* __restrict__ n_top, int pi) {
  const int n = n_top[pi];
  return (n < 0 || n > LP_MAXN) ? -1 : n;
}

// the token's entry as the rank sees it: comparable only inside [0, V) and not NaN
__device__ __forceinline__ bool lp_token_value(const bf16_t* __restrict__ x, int V, long token, float* v) {
  if (token < 0 || token >= V) return false;
  const uint32_t b = x[token];
  *v = bf2f(b);
  return !lp_nan(b);
}
// float(x[token]) - l; a token outside [0, V) gives NaN
__device__ __forceinline__ float lp_logprob(const bf16_t* __restrict__ x, int V, long token, float l) {
  if (token < 0 || token >= V) return __builtin_nanf("");
  return bf2f(x[token]) - l;
}

template <bool KNOWN>
__global__ void __launch_bounds__(LP_THREADS)
logprob_slice_kernel(const bf16_t* __restrict__ logits, long ld, int V, const int32_t* __restrict__ n_top, int rows_per_param, int S,
                     bf16_t* __restrict__ raw, long raw_ld, const int64_t* __restrict__ tokens, float* __restrict__ ws) {
  __shared__ LpBest smb[LP_MAXN + 1][LP_WAVES];
  __shared__ float sms[LP_WAVES];
  __shared__ int smc[LP_WAVES];
  __shared__ int smg[LP_WAVES];
  const int row = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x;
  const int n = lp_count(n_top, row / rows_per_param);
  if (n < 0) return;
  const bf16_t* x = logits + (size_t)row * ld;
  bf16_t* cp = raw ? raw + (size_t)row * raw_ld : nullptr;
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const bool cvec = (reinterpret_cast<uintptr_t>(cp) & 15) == 0;
  // the known token's entry: one uniform address, asked for ahead of the slice's own loads
  float xt = 0.f;
  bool tok = false;
  if constexpr (KNOWN) tok = lp_token_value(x, V, tokens[row], &xt);

  // ---- the slice, once: values, validity (inside [0, V) and not NaN), the copy ----
  float v[LP_PER * 8];
  int base[LP_PER];
  unsigned ok = 0;
#pragma unroll
  for (int u = 0; u < LP_PER; ++u) {
    base[u] = ((sl * LP_PER + u) * LP_THREADS + tid) * 8;
    uint32_t b[8];
    unsigned in = 0;
    if (vec && base[u] + 8 <= V) {
      const u32x4_t q = *reinterpret_cast<const u32x4_t*>(x + base[u]);
#pragma unroll
      for (int e = 0; e < 4; ++e) { b[2 * e] = q[e] & 0xffffu; b[2 * e + 1] = q[e] >> 16; }
      in = 0xffu;
      if (cp && cvec) *reinterpret_cast<u32x4_t*>(cp + base[u]) = q;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        b[e] = 0xff80u;
        if (base[u] + e < V) { b[e] = x[base[u] + e]; in |= 1u << e; }
      }
    }
    if (cp && !(cvec && vec && base[u] + 8 <= V)) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if ((in >> e) & 1u) cp[base[u] + e] = (bf16_t)b[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool good = ((in >> e) & 1u) && !lp_nan(b[e]);
      v[u * 8 + e] = good ? bf2f(b[e]) : -INFINITY;
      ok |= good ? 1u << (u * 8 + e) : 0u;
    }
  }

  // ---- round 0: the slice's maximum (its first candidate) and the number of comparable entries ----
  unsigned taken = ~ok;
  LpBest best = {-INFINITY, LP_NONE};
#pragma unroll
  for (int u = 0; u < LP_PER; ++u)
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if ((ok >> (u * 8 + e)) & 1u) best = lp_better(best, LpBest{v[u * 8 + e], base[u] + e});
  best = lp_wave_best(best);
  int cnt = __popc(ok);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((tid & 63) == 0) { smb[0][tid >> 6] = best; smc[tid >> 6] = cnt; }
  if constexpr (KNOWN) {
    // ---- the comparable entries of this slice that are >= the token's (-0.0 == +0.0; a token that is not comparable counts nothing) ----
    int ge = 0;
#pragma unroll
    for (int q = 0; q < LP_PER * 8; ++q) ge += (tok && ((ok >> q) & 1u) && v[q] >= xt) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ge += __shfl_xor(ge, o, 64);
    if ((tid & 63) == 0) smg[tid >> 6] = ge;
  }
  __syncthreads();
  LpBest r = smb[0][0];
  int nc = smc[0];
#pragma unroll
  for (int w = 1; w < LP_WAVES; ++w) { r = lp_better(r, smb[0][w]); nc += smc[w]; }
  const float m = r.v;

  // ---- sum exp(x - m): the class of the maximum counts 1 each, which also covers a maximum that is not finite ----
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < LP_PER * 8; ++q)
    if ((ok >> q) & 1u) s += v[q] == m ? 1.f : __expf(v[q] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((tid & 63) == 0) sms[tid >> 6] = s;
  __syncthreads();
  float* rec = ws + ((size_t)row * S + sl) * LP_REC;
  if (tid == 0) {
    rec[0] = m;
    rec[1] = ((sms[0] + sms[1]) + sms[2]) + sms[3];
    rec[2] = __int_as_float(nc);
    if constexpr (KNOWN) rec[3] = __int_as_float(((smg[0] + smg[1]) + smg[2]) + smg[3]);
    if (n > 0) { rec[4] = r.v; rec[4 + LP_MAXN] = __int_as_float(r.i); }
  }

  // ---- rounds 1 .. n-1: the next candidates; an exhausted slice leaves {-inf, LP_NONE} ----
  for (int f = 1; f < n; ++f) {
#pragma unroll
    for (int u = 0; u < LP_PER; ++u)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (base[u] + e == r.i) taken |= 1u << (u * 8 + e);
    best = LpBest{-INFINITY, LP_NONE};
#pragma unroll
    for (int u = 0; u < LP_PER; ++u)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (!((taken >> (u * 8 + e)) & 1u)) best = lp_better(best, LpBest{v[u * 8 + e], base[u] + e});
    best = lp_wave_best(best);
    if ((tid & 63) == 0) smb[f][tid >> 6] = best;
    __syncthreads();
    r = smb[f][0];
#pragma unroll
    for (int w = 1; w < LP_WAVES; ++w) r = lp_better(r, smb[f][w]);
    if (tid == 0) { rec[4 + f] = r.v; rec[4 + LP_MAXN + f] = __int_as_float(r.i); }
  }
}

template <bool KNOWN>
__global__ void __launch_bounds__(64)
logprob_merge_kernel(const float* __restrict__ ws, const int32_t* __restrict__ n_top, int rows_per_param, int S, float* __restrict__ lse,
                     float* __restrict__ top_val, int32_t* __restrict__ top_id, const bf16_t* __restrict__ logits, long ld, int V,
                     const int64_t* __restrict__ tokens, float* __restrict__ out, int32_t* __restrict__ rank) {
  __shared__ float cv[LP_MAXS * LP_MAXN];
  __shared__ int ci[LP_MAXS * LP_MAXN];
  const int row = blockIdx.x, lane = threadIdx.x;
  const int n = lp_count(n_top, row / rows_per_param);
  if (n < 0) return;
  const float* rec = ws + (size_t)row * S * LP_REC;
  if (top_id) {
    for (int q = lane; q < S * n; q += 64) {
      const int sl = q / n, f = q % n;
      cv[sl * LP_MAXN + f] = rec[(size_t)sl * LP_REC + 4 + f];
      ci[sl * LP_MAXN + f] = __float_as_int(rec[(size_t)sl * LP_REC + 4 + LP_MAXN + f]);
    }
  }
  // ---- the S (max, sum, count) triples, lane = slice: the row's maximum, then the sums rescaled to it ----
  float m_s = -INFINITY, sum_s = 0.f;
  int nc = 0;
  if (lane < S) {
    m_s = rec[(size_t)lane * LP_REC];
    sum_s = rec[(size_t)lane * LP_REC + 1];
    nc = __float_as_int(rec[(size_t)lane * LP_REC + 2]);
  }
  float M = m_s;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { M = fmaxf(M, __shfl_xor(M, o, 64)); }
  float total = nc > 0 ? sum_s * (m_s == M ? 1.f : __expf(m_s - M)) : 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { total += __shfl_xor(total, o, 64); nc += __shfl_xor(nc, o, 64); }
  const float l = nc > 0 ? M + logf(total) : __builtin_nanf("");
  const bool infinite = nc > 0 && (M == INFINITY || M == -INFINITY);
  if (lane == 0) lse[row] = l;
  if constexpr (KNOWN) {
    int ge = lane < S ? __float_as_int(rec[(size_t)lane * LP_REC + 3]) : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ge += __shfl_xor(ge, o, 64);
    if (lane == 0) {
      const bf16_t* x = logits + (size_t)row * ld;
      const long token = tokens[row];
      float xt;
      out[row] = lp_logprob(x, V, token, l);
      rank[row] = lp_token_value(x, V, token, &xt) ? ge : 0;
    }
  }
  if (!top_id) return;
  __syncthreads();

  // ---- the S sorted candidate lists: every lane offers the head of its slice's list ----
  int head = 0;
  for (int f = 0; f < n; ++f) {
    LpBest c = {-INFINITY, LP_NONE};
    if (lane < S && head < n) c = LpBest{cv[lane * LP_MAXN + head], ci[lane * LP_MAXN + head]};
    const LpBest best = lp_wave_best(c);
    if (best.i != LP_NONE && c.i == best.i) ++head;
    if (lane == 0) {
      const size_t o = (size_t)row * LP_MAXN + f;
      if (best.i == LP_NONE) {
        top_id[o] = -1;
        top_val[o] = -INFINITY;
      } else {
        top_id[o] = best.i;
        top_val[o] = infinite ? (best.v == M ? -logf(total) : -INFINITY) : best.v - l;
      }
    }
  }
}

static inline int lp_slices(int V) { return (V + SSD_LOGPROB_SLICE - 1) / SSD_LOGPROB_SLICE; }
