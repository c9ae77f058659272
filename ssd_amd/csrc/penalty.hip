// Repetition / presence / frequency penalties and logit bias on raw logit rows (include/ssd_hip_penalty.h has the semantics): the rows
// are adjusted in place before ssd_filter_rows, the samplers, ssd_row_lse, ssd_verify_ratio and argmax read them.
//
// The work is sparse: a row of V logits is touched only at the ids of its sequence's history table and at the few tokens of the
// current round.  One workgroup of 256 threads per row:
//   1. the row's extra tokens (prefix form: the first j of the sequence's inputs; chain form: the first *extra_n of its speculation
//      row) go into LDS as int32, ids outside [0, V) as -1;
//   2. thread i walks table entries i, i + 256, ...: total count = table count + matches among the extras (which it marks as "in
//      the table"), one load, the fp32 arithmetic of the header, one 2-byte store if the bits changed;
//   3. after a barrier, thread k < m takes extra k if it is the first occurrence of its token and nobody marked it: count =
//      occurrences among the extras, not in the prompt, no bias.
// Table ids are unique and step 3 handles each remaining distinct token once, so no two threads write the same entry: no atomics,
// the same bits on every run.  Every fp32 operation is an explicit round-to-nearest intrinsic: nothing is contracted into an FMA and
// the division is the IEEE one, whatever the compiler flags.
#include "common.h"
#include "rows.h"

constexpr int PN_THREADS = 256;

__device__ __forceinline__ uint32_t pn_apply(uint32_t b, float bias, bool seen, int c, float r, float p, float f) {
  if ((b & 0x7fffu) > 0x7f80u) return b;          // a NaN logit keeps its bits
  float x = bf2f(b);
  if (bias != 0.f) x = __fadd_rn(x, bias);
  if (seen) x = x < 0.f ? __fmul_rn(x, r) : __fdiv_rn(x, r);
  if (c > 0) {
    x = __fsub_rn(x, __fmul_rn(f, (float)c));
    x = __fsub_rn(x, p);
  }
  return x != x ? 0x7fc0u : f2bf(x);
}

__global__ void __launch_bounds__(PN_THREADS)
penalize_rows_kernel(bf16_t* __restrict__ logits, long ld, int V, int rows_per_seq, const int32_t* __restrict__ tab_ids,
                     const int32_t* __restrict__ tab_cnt, const float* __restrict__ tab_bias, int tab_ld,
                     const int32_t* __restrict__ tab_len, const float* __restrict__ rep, const float* __restrict__ pres,
                     const float* __restrict__ freq, const int64_t* __restrict__ extra, int extra_ld,
                     const int32_t* __restrict__ extra_n) {
  __shared__ int ex[SSD_PENALTY_MAX_EXTRA];
  __shared__ int in_tab[SSD_PENALTY_MAX_EXTRA];
  const int row = blockIdx.x;
  const int b = row / rows_per_seq;
  const float r = rep[b], p = pres[b], f = freq[b];
  const bool pen = !(r == 1.f && p == 0.f && f == 0.f);
  const int n = tab_ids ? min(max(tab_len[b], 0), tab_ld) : 0;
  const int m = pen ? rows_seen(extra, extra_ld, extra_n, row, b, rows_per_seq) : 0;     // they only matter to r, p and f
  if (n == 0 && m == 0) return;
  bf16_t* x = logits + (size_t)row * ld;

  if ((int)threadIdx.x < m) {
    const int64_t t = extra[(size_t)b * extra_ld + 1 + threadIdx.x];
    ex[threadIdx.x] = (t >= 0 && t < V) ? (int)t : -1;
    in_tab[threadIdx.x] = 0;
  }
  __syncthreads();

  const size_t tb = (size_t)b * tab_ld;
  for (int i = threadIdx.x; i < n; i += PN_THREADS) {
    const int t = tab_ids[tb + i];
    if (t < 0 || t >= V) continue;
    const int packed = tab_cnt[tb + i];
    int c = packed >> 1;
    for (int k = 0; k < m; ++k) {
      if (ex[k] == t) { ++c; in_tab[k] = 1; }
    }
    const uint32_t old = x[t];
    const uint32_t nw = pn_apply(old, tab_bias[tb + i], (packed & 1) || c > 0, c, r, p, f);
    if (nw != old) x[t] = (bf16_t)nw;
  }
  if (m == 0) return;
  __syncthreads();

  const int k = threadIdx.x;
  if (k < m && ex[k] >= 0 && !in_tab[k]) {
    const int t = ex[k];
    int c = 0;
    bool first = true;
    for (int q = 0; q < m; ++q) {
      if (ex[q] == t) { ++c; if (q < k) first = false; }
    }
    if (first) {
      const uint32_t old = x[t];
      const uint32_t nw = pn_apply(old, 0.f, true, c, r, p, f);
      if (nw != old) x[t] = (bf16_t)nw;
    }
  }
}

extern "C" int ssd_penalize_rows(void* logits_rows, long ld, int T, int V, int rows_per_seq, const int32_t* tab_ids,
                                 const int32_t* tab_cnt, const float* tab_bias, int tab_ld, const int32_t* tab_len, const float* rep,
                                 const float* pres, const float* freq, const int64_t* extra, int extra_ld, const int32_t* extra_n,
                                 void* stream) {
  const bool tab_any = tab_ids || tab_cnt || tab_bias || tab_len;
  const bool tab_all = tab_ids && tab_cnt && tab_bias && tab_len;
  if (T <= 0 || V <= 0 || rows_per_seq <= 0 || ld < V) return SSD_ERR_SHAPE;
  if (tab_all && tab_ld <= 0) return SSD_ERR_SHAPE;
  if (extra && (extra_ld < 1 || extra_ld - 1 > SSD_PENALTY_MAX_EXTRA || (!extra_n && extra_ld < rows_per_seq))) return SSD_ERR_SHAPE;
  if (!logits_rows || !rep || !pres || !freq || (tab_any && !tab_all) || (extra_n && !extra)) return SSD_ERR_ARG;
  hipLaunchKernelGGL(penalize_rows_kernel, dim3(T), dim3(PN_THREADS), 0, (hipStream_t)stream, (bf16_t*)logits_rows, ld, V, rows_per_seq,
                     tab_ids, tab_cnt, tab_bias, tab_ld, tab_len, rep, pres, freq, extra, extra_ld, extra_n);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}
