// Device helpers of the kernels that rewrite raw logit rows per request, shared by penalty.hip, constrain.hip and guide.hip: which of the
// round's extra tokens a row sees, and the write of one 8-entry chunk of bans.
#pragma once
#include "common.h"

constexpr uint32_t ROWS_NINF = 0xff80u;         // bf16 -inf

// Extras row `row` of sequence b sees (the headers' two forms): none without `extra`; extra_n null -- row j of a sequence sees
// extra[b][1..j]; extra_n a device scalar -- every row sees extra[b][1..*extra_n], clamped to what a row of extra_ld entries holds.
__device__ __forceinline__ int rows_seen(const int64_t* __restrict__ extra, int extra_ld, const int32_t* __restrict__ extra_n, int row,
                                         int b, int rows_per_seq) {
  return extra ? (extra_n ? min(max(*extra_n, 0), extra_ld - 1) : row - b * rows_per_seq) : 0;
}

// -inf over the entries x[base + k] of one chunk whose bit k of `ban` is set (base < V, a multiple of 8; bits at or past V are
// dropped).  Nothing banned: the chunk is neither read nor written; all banned: one 16-byte store; otherwise one 16-byte load, the
// banned halves replaced, one 16-byte store.  A chunk that crosses V or a row that is not 16-byte aligned (vec false) takes 2-byte
// stores of its banned entries instead.  The caller gives every chunk to one thread, so every entry has exactly one writer.
__device__ __forceinline__ void ban_chunk(bf16_t* x, int base, int V, bool vec, uint32_t ban) {
  if (base + 8 > V) ban &= (1u << (V - base)) - 1u;
  if (ban == 0) return;
  bf16_t* c = x + base;
  if (vec && base + 8 <= V) {
    u32x4_t q;
    if (ban == 0xffu) {
      q = u32x4_t{ROWS_NINF | (ROWS_NINF << 16), ROWS_NINF | (ROWS_NINF << 16), ROWS_NINF | (ROWS_NINF << 16), ROWS_NINF | (ROWS_NINF << 16)};
    } else {
      q = *reinterpret_cast<const u32x4_t*>(c);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uint32_t w = q[k];
        if ((ban >> (2 * k)) & 1u) w = (w & 0xffff0000u) | ROWS_NINF;
        if ((ban >> (2 * k + 1)) & 1u) w = (w & 0x0000ffffu) | (ROWS_NINF << 16);
        q[k] = w;
      }
    }
    *reinterpret_cast<u32x4_t*>(c) = q;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if ((ban >> k) & 1u) c[k] = (bf16_t)ROWS_NINF;
  }
}
