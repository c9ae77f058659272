// Hard token constraints on raw logit rows (include/ssd_hip_constrain.h has the semantics): an allow mask over the vocabulary, stop
// tokens that cannot be generated before min_tokens, and banned words matched against the host tail + the round's tokens.  Banned
// entries become -inf in place, before anything reads the rows.
//
// The shape of logprob_slice_kernel (logprob.hip) and seeded.hip: a row is cut into slices of 4096 entries and workgroup (slice, row)
// owns its slice, so a 128 K-entry row is spread over 32 CUs instead of one.  Every workgroup
//   1. puts the row's context (tail, then the extras the row sees) into LDS;
//   2. resolves the sparse lists into 192 LDS slots: thread i < 64 the i-th stop id (if the minimum length still holds), thread
//      64 + w bad word w (its last token if the word has one token or its prefix ends the context), -1 for "bans nothing";
//   3. wave 0 compacts the slots that fall into this slice (ballot + prefix count, slot order: no atomics);
//   4. every thread builds an 8-bit ban mask for each of its two 8-entry chunks -- from one 4-byte load of the allow word that covers
//      the chunk and from the compacted list -- and then: nothing banned: the chunk is neither read nor written; all banned: one
//      16-byte store; otherwise one 16-byte load, the banned halves replaced, one 16-byte store.  A chunk that crosses V or a row that
//      is not 16-byte aligned takes 2-byte stores of its banned entries instead (ban_chunk, rows.h).
// A chunk belongs to one thread whatever the path, so every entry has exactly one writer: a sparse ban is never a separate store that
// could race a neighbour's read-modify-write.  The same input gives the same bits on every run.
#include "common.h"
#include "rows.h"

constexpr int CN_THREADS = 256;
constexpr int CN_PER = 2;                                               // 8-entry chunks per thread
constexpr int CN_SLOTS = SSD_CONSTRAIN_MAX_STOP + SSD_CONSTRAIN_MAX_WORDS;
constexpr int CN_CTX = SSD_CONSTRAIN_MAX_WORD_LEN - 1 + SSD_CONSTRAIN_MAX_EXTRA;
static_assert(SSD_CONSTRAIN_SLICE == CN_THREADS * CN_PER * 8, "one slice = two chunks per thread");
static_assert(CN_SLOTS % 64 == 0 && CN_SLOTS <= CN_THREADS, "one thread per slot, whole waves in the compaction");
static_assert(SSD_CONSTRAIN_MAX_WORD_LEN - 1 <= 64 && SSD_CONSTRAIN_MAX_EXTRA + 64 <= CN_THREADS, "one thread per context token");

__global__ void __launch_bounds__(CN_THREADS)
constrain_rows_kernel(bf16_t* __restrict__ logits, long ld, int V, int rows_per_seq, const int32_t* __restrict__ allow_on,
                      const uint32_t* __restrict__ allow_bits, const int32_t* __restrict__ min_left, const int32_t* __restrict__ stop_ids,
                      const int32_t* __restrict__ stop_len, const int32_t* __restrict__ bw_tok, const int32_t* __restrict__ bw_off,
                      const int32_t* __restrict__ bw_n, const int32_t* __restrict__ tail, int tail_ld, const int32_t* __restrict__ tail_len,
                      const int64_t* __restrict__ extra, int extra_ld, const int32_t* __restrict__ extra_n) {
  __shared__ long long ctx[CN_CTX];
  __shared__ int slot[CN_SLOTS];
  __shared__ int hit[CN_SLOTS];         // offsets into this slice of the ids that fall into it
  __shared__ int nhit;
  const int row = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x;
  const int b = row / rows_per_seq;
  const int e = rows_seen(extra, extra_ld, extra_n, row, b, rows_per_seq);
  const bool on = allow_on && allow_on[b] != 0;
  const int ns = (stop_ids && e < min_left[b]) ? min(max(stop_len[b], 0), SSD_CONSTRAIN_MAX_STOP) : 0;
  const int nw = bw_tok ? min(max(bw_n[b], 0), SSD_CONSTRAIN_MAX_WORDS) : 0;
  if (!on && ns == 0 && nw == 0) return;        // (uniform over the workgroup)
  const int lo = sl * SSD_CONSTRAIN_SLICE;

  int n = 0;
  if (ns > 0 || nw > 0) {
    const int tl = nw > 0 ? min(max(tail_len[b], 0), tail_ld) : 0;
    if (nw > 0) {
      if (tid < tl) ctx[tid] = tail[(size_t)b * tail_ld + tid];
      if (tid >= 64 && tid - 64 < e) ctx[tl + tid - 64] = extra[(size_t)b * extra_ld + 1 + (tid - 64)];
      __syncthreads();
    }
    if (tid < SSD_CONSTRAIN_MAX_STOP) {
      slot[tid] = tid < ns ? stop_ids[(size_t)b * SSD_CONSTRAIN_MAX_STOP + tid] : -1;
    } else if (tid < CN_SLOTS) {
      const int w = tid - SSD_CONSTRAIN_MAX_STOP;
      int id = -1;
      if (w < nw) {
        const int32_t* off = bw_off + (size_t)b * (SSD_CONSTRAIN_MAX_WORDS + 1);
        const int o0 = off[w], o1 = off[w + 1], L = o1 - o0, nc = tl + e;
        if (o0 >= 0 && o1 <= SSD_CONSTRAIN_MAX_WORD_TOKENS && L >= 1 && L <= SSD_CONSTRAIN_MAX_WORD_LEN && nc >= L - 1) {
          const int32_t* tok = bw_tok + (size_t)b * SSD_CONSTRAIN_MAX_WORD_TOKENS + o0;
          bool match = true;
          for (int k = 0; k < L - 1; ++k) match = match && ctx[nc - (L - 1) + k] == (long long)tok[k];
          if (match) id = tok[L - 1];
        }
      }
      slot[tid] = id;
    }
    __syncthreads();
    if (tid < 64) {
      const int hi = min(lo + SSD_CONSTRAIN_SLICE, V);
      int m = 0;
#pragma unroll
      for (int r = 0; r < CN_SLOTS / 64; ++r) {
        const int id = slot[r * 64 + tid];
        const bool in = id >= lo && id < hi;
        const unsigned long long bal = __ballot(in);
        if (in) hit[m + __popcll(bal & ((1ull << tid) - 1ull))] = id - lo;
        m += __popcll(bal);
      }
      if (tid == 0) nhit = m;
    }
    __syncthreads();
    n = nhit;
    if (!on && n == 0) return;
  }

  bf16_t* x = logits + (size_t)row * ld;
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const uint32_t* bits = on ? allow_bits + (size_t)b * ((V + 31) >> 5) : nullptr;
#pragma unroll
  for (int u = 0; u < CN_PER; ++u) {
    const int c = u * CN_THREADS + tid;         // chunk of the slice
    const int base = lo + c * 8;
    if (base >= V) continue;
    uint32_t ban = 0;
    if (on) ban = ~(bits[base >> 5] >> (base & 31)) & 0xffu;
    for (int i = 0; i < n; ++i) {
      const int d = hit[i];
      if ((d >> 3) == c) ban |= 1u << (d & 7);
    }
    ban_chunk(x, base, V, vec, ban);
  }
}

extern "C" int ssd_constrain_rows(void* logits_rows, long ld, int T, int V, int rows_per_seq, const int32_t* allow_on,
                                  const uint32_t* allow_bits, const int32_t* min_left, const int32_t* stop_ids, const int32_t* stop_len,
                                  const int32_t* bw_tok, const int32_t* bw_off, const int32_t* bw_n, const int32_t* tail, int tail_ld,
                                  const int32_t* tail_len, const int64_t* extra, int extra_ld, const int32_t* extra_n, void* stream) {
  const bool allow_any = allow_on || allow_bits, allow_all = allow_on && allow_bits;
  const bool stop_any = min_left || stop_ids || stop_len, stop_all = min_left && stop_ids && stop_len;
  const bool bw_any = bw_tok || bw_off || bw_n || tail || tail_len, bw_all = bw_tok && bw_off && bw_n && tail && tail_len;
  if (T <= 0 || V <= 0 || rows_per_seq <= 0 || ld < V || T > 65535) return SSD_ERR_SHAPE;
  if (bw_all && (tail_ld < 1 || tail_ld > SSD_CONSTRAIN_MAX_WORD_LEN - 1)) return SSD_ERR_SHAPE;
  if (extra && (extra_ld < 1 || extra_ld - 1 > SSD_CONSTRAIN_MAX_EXTRA || (!extra_n && extra_ld < rows_per_seq))) return SSD_ERR_SHAPE;
  if (!logits_rows || (allow_any && !allow_all) || (stop_any && !stop_all) || (bw_any && !bw_all) || (extra_n && !extra))
    return SSD_ERR_ARG;
  const int S = (V + SSD_CONSTRAIN_SLICE - 1) / SSD_CONSTRAIN_SLICE;
  hipLaunchKernelGGL(constrain_rows_kernel, dim3(S, T), dim3(CN_THREADS), 0, (hipStream_t)stream, (bf16_t*)logits_rows, ld, V,
                     rows_per_seq, allow_on, allow_bits, min_left, stop_ids, stop_len, bw_tok, bw_off, bw_n, tail, tail_ld, tail_len,
                     extra, extra_ld, extra_n);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}
