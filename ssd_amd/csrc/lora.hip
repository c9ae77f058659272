// LoRA adapters (include/ssd_hip_lora.h): shrink (x . A^T into fp32 split-K slabs) and expand (t . B^T added to the rows a linear's
// GEMM has just stored, or finished as SiLU(gate) * up), with a slot per token row.
//
// Both launches are latency-bound at decode sizes (M <= 24: the tables are <= 2 % of the base weight's bytes), so each is ONE round
// trip to memory per wave: every load of a wave is independent of every other, the cross-wave combine goes through LDS, and the K
// split of the shrink is summed by the expand's prologue (the project's slab idiom: the kernel boundary is the only synchronisation).
// The MFMA operand roles are those of the GEMMs: the A operand is the table (16 table rows -> D rows), the B operand is the token
// tile (16 token rows -> D columns), so a token row only ever influences its own D column: rows of another slot, rows without one
// and the padding rows past M compute values that are never stored.
#include "common.h"
#include "ssd_hip_lora.h"

constexpr int LORA_WAVES = 4;       // waves per workgroup, both kernels
constexpr int LORA_ROWS = 32;       // token rows per workgroup: two 16-row tiles share every table fragment a wave loads

// the slot of token row m: -1 past M and for every value outside [0, slots)
__device__ __forceinline__ int lora_slot(const int32_t* __restrict__ row_slot, int m, int M, int slots) {
  if (m >= M) return -1;
  const int s = row_slot[m];
  return (s >= 0 && s < slots) ? s : -1;
}

// four consecutive bf16 of a row as fp32: one 8-byte load where the row pitch keeps them aligned
__device__ __forceinline__ void lora_load4(const bf16_t* __restrict__ p, bool vec, float (&o)[4]) {
  if (vec) {
    const u32x2_t v = *reinterpret_cast<const u32x2_t*>(p);
    o[0] = bf2f(v[0] & 0xffffu); o[1] = bf2f(v[0] >> 16); o[2] = bf2f(v[1] & 0xffffu); o[3] = bf2f(v[1] >> 16);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = bf2f(p[r]);
  }
}

// grid (S, ceil(M / 32), slots * R / 16): workgroup (s, c, z) multiplies rank group z % (R / 16) of slot z / (R / 16) with token rows
// 32c .. 32c + 31 over the k-tiles of split s, and stores the columns of the rows that name that slot.
__global__ void __launch_bounds__(LORA_WAVES * 64)
lora_shrink_kernel(const u32x4_t* __restrict__ Xf, const u32x4_t* __restrict__ Af, const int32_t* __restrict__ row_slot,
                   float* __restrict__ ws, int M, int K, int R, int slots, int S) {
  __shared__ f32x4_t red[LORA_WAVES][2][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int RG = R >> 4, KT = K >> 5;
  const int s = blockIdx.x, slot = blockIdx.z / RG, rg = blockIdx.z % RG;
  const int m0 = blockIdx.y * LORA_ROWS;
  const int mcol = lane & 15;
  const int cs0 = lora_slot(row_slot, m0 + mcol, M, slots), cs1 = lora_slot(row_slot, m0 + 16 + mcol, M, slots);
  if (__ballot(cs0 == slot || cs1 == slot) == 0) return;       // no row of this chunk names the slot (uniform over the workgroup)
  const int mtiles = (M + 15) >> 4;
  const bool two = blockIdx.y * 2 + 1 < mtiles;                 // x_frag holds ceil(M / 16) row tiles: the second may not exist
  const int kb = (int)((long)s * KT / S), ke = (int)((long)(s + 1) * KT / S);
  const u32x4_t* ap = Af + (((size_t)slot * RG + rg) * KT << 6) + lane;
  const u32x4_t* xp0 = Xf + ((size_t)(blockIdx.y * 2) * KT << 6) + lane;
  const u32x4_t* xp1 = two ? xp0 + ((size_t)KT << 6) : xp0;     // (no second tile: the first again, its products are never stored)
  f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
  // four k-tiles per step: all twelve loads of a step are in flight before the first MFMA waits (a wave's share is 4 .. 14 k-tiles at
  // the 70B shapes: one to four dependent round trips instead of one per k-tile)
  constexpr int U = 4;
  int kt = kb + wave;
  for (; kt + (U - 1) * LORA_WAVES < ke; kt += U * LORA_WAVES) {
    u32x4_t a[U], b0[U], b1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t o = (size_t)(kt + u * LORA_WAVES) << 6;
      a[u] = ap[o]; b0[u] = xp0[o]; b1[u] = xp1[o];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc0 = mfma16(a[u], b0[u], acc0);
      acc1 = mfma16(a[u], b1[u], acc1);
    }
  }
  for (; kt < ke; kt += LORA_WAVES) {
    const u32x4_t a = ap[(size_t)kt << 6], b0 = xp0[(size_t)kt << 6], b1 = xp1[(size_t)kt << 6];
    acc0 = mfma16(a, b0, acc0);
    acc1 = mfma16(a, b1, acc1);
  }
  red[wave][0][lane] = acc0;
  red[wave][1][lane] = acc1;
  __syncthreads();
  if (wave >= 2) return;
  const int cs = wave == 0 ? cs0 : cs1;
  if (cs != slot) return;                                      // (covers m >= M and the missing second tile)
  f32x4_t v = red[0][wave][lane];
#pragma unroll
  for (int w = 1; w < LORA_WAVES; ++w) v += red[w][wave][lane];
  const int m = m0 + wave * 16 + mcol;
  const int j = rg * 16 + (lane >> 4) * 4;                     // D rows -> ranks j .. j + 3
  *reinterpret_cast<f32x4_t*>(ws + ((size_t)s * M + m) * R + j) = v;
}

// grid (workgroups over the units of N, ceil(M / 32)).  A unit is one 16-column group of y (epilogue 0) or a (gate, up) pair of them
// (epilogue 1); wave w of workgroup b takes units (b * 4 + w) * upw .. + upw - 1.
template <int EPI, int RT>
__global__ void __launch_bounds__(LORA_WAVES * 64)
lora_expand_kernel(const float* __restrict__ ws, const u32x4_t* __restrict__ Bf, const float* __restrict__ scale,
                   const int32_t* __restrict__ row_slot, bf16_t* __restrict__ y, int ldy, u32x2_t* __restrict__ act, int M, int N, int R,
                   int slots, int S, int upw) {
  __shared__ u32x4_t tl[2][RT][64];                            // t of the chunk's two row tiles as MFMA B operands, per rank tile (RT = R / 32)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int NG = N >> 4;
  const int m0 = blockIdx.y * LORA_ROWS;
  // ---- t = bf16(sum of the slabs in slab order): chunk (tile, rank tile, lane) holds row (lane & 15), ranks 8 (lane >> 4) .. + 7 ----
  for (int c = threadIdx.x; c < 2 * RT * 64; c += LORA_WAVES * 64) {
    const int l = c & 63, kt = (c >> 6) % RT, mt = (c >> 6) / RT;
    const int m = m0 + mt * 16 + (l & 15);
    u32x4_t t = {0u, 0u, 0u, 0u};
    if (lora_slot(row_slot, m, M, slots) >= 0) {
      const float* p = ws + (size_t)m * R + kt * 32 + (l >> 4) * 8;
      f32x4_t lo = *reinterpret_cast<const f32x4_t*>(p), hi = *reinterpret_cast<const f32x4_t*>(p + 4);
#pragma unroll 4
      for (int s = 1; s < S; ++s) {
        const float* q = p + (size_t)s * M * R;
        lo += *reinterpret_cast<const f32x4_t*>(q);
        hi += *reinterpret_cast<const f32x4_t*>(q + 4);
      }
      t = u32x4_t{pack_bf2(lo[0], lo[1]), pack_bf2(lo[2], lo[3]), pack_bf2(hi[0], hi[1]), pack_bf2(hi[2], hi[3])};
    }
    tl[mt][kt][l] = t;
  }
  __syncthreads();
  const int mcol = lane & 15, nrow = (lane >> 4) * 4;
  const int cs0 = lora_slot(row_slot, m0 + mcol, M, slots), cs1 = lora_slot(row_slot, m0 + 16 + mcol, M, slots);
  const bool vec = (ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 7) == 0;
  constexpr int G = EPI == SSD_LORA_EPI_SILU ? 2 : 1;           // 16-column groups per unit
  const int units = NG / G;
  const int u0 = (blockIdx.x * LORA_WAVES + wave) * upw;
  for (int u = u0; u < min(units, u0 + upw); ++u) {
    f32x4_t d[G][2];                                           // scale * (t . B^T) of this lane's row, 0 without a slot
#pragma unroll
    for (int g = 0; g < G; ++g) d[g][0] = d[g][1] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int sl = 0; sl < slots; ++sl) {
      if (__ballot(cs0 == sl || cs1 == sl) == 0) continue;     // a slot no row of the chunk names: its table is not read
      const float sc = scale[sl];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const u32x4_t* bp = Bf + (((size_t)sl * NG + (size_t)u * G + g) * RT << 6) + lane;
        f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
        u32x4_t b[RT];
#pragma unroll
        for (int kt = 0; kt < RT; ++kt) b[kt] = bp[(size_t)kt << 6];
#pragma unroll
        for (int kt = 0; kt < RT; ++kt) {
          a0 = mfma16(b[kt], tl[0][kt][lane], a0);
          a1 = mfma16(b[kt], tl[1][kt][lane], a1);
        }
        if (cs0 == sl) d[g][0] = a0 * sc;
        if (cs1 == sl) d[g][1] = a1 * sc;
      }
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int m = m0 + mt * 16 + mcol;
      const int cs = mt == 0 ? cs0 : cs1;
      if (m >= M) continue;
      if (EPI == SSD_LORA_EPI_ADD) {
        if (cs < 0) continue;                                   // rows without a slot keep their bits: never written
        bf16_t* yp = y + (size_t)m * ldy + u * 16 + nrow;
        float o[4];
        lora_load4(yp, vec, o);
        if (vec) {
          *reinterpret_cast<u32x2_t*>(yp) = u32x2_t{pack_bf2(o[0] + d[0][mt][0], o[1] + d[0][mt][1]), pack_bf2(o[2] + d[0][mt][2], o[3] + d[0][mt][3])};
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) yp[r] = (bf16_t)f2bf(o[r] + d[0][mt][r]);
        }
      } else {
        // y: group 2u = gate features 16u .., group 2u + 1 = up features 16u ..; the activation is fragment-major [M][N / 2]
        const bf16_t* gp = y + (size_t)m * ldy + (2 * u) * 16 + nrow;
        const bf16_t* up = gp + 16;
        float o[4], g4[4], u4[4];
        lora_load4(gp, vec, g4);
        lora_load4(up, vec, u4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float gb = g4[r], ub = u4[r];
          if (cs >= 0) { gb = round_bf(gb + d[0][mt][r]); ub = round_bf(ub + d[G - 1][mt][r]); }
          o[r] = (gb / (1.0f + __expf(-gb))) * ub;
        }
        const int n = u * 16 + nrow;                            // feature in [0, N / 2)
        act[frag_chunk(m, n >> 3, (N >> 1) >> 5) * 2 + ((n >> 2) & 1)] = u32x2_t{pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
      }
    }
  }
}

extern "C" int ssd_lora_default_splits(int K) {
  if (K <= 0 || (K & 31)) return 0;
  const int KT = K >> 5;
  int S = KT / 8;                     // >= 8 k-tiles per workgroup, two per wave
  if (S < 1) S = 1;
  if (S > SSD_LORA_MAX_SPLITS) S = SSD_LORA_MAX_SPLITS;
  return S;
}

extern "C" long ssd_lora_workspace_bytes(int M, int K, int R) {
  if (M <= 0 || K <= 0 || (K & 31) || R <= 0 || (R & 31) || R > SSD_LORA_MAX_R) return 0;
  const int KT = K >> 5;
  return (long)(KT < SSD_LORA_MAX_SPLITS ? KT : SSD_LORA_MAX_SPLITS) * M * R * 4;
}

static int lora_check(int M, int K, int R, int slots, int* splits, long ws_bytes) {
  if (M <= 0 || K <= 0 || (K & 31) || R <= 0 || (R & 31) || R > SSD_LORA_MAX_R) return SSD_ERR_SHAPE;
  if (slots < 1) return SSD_ERR_ARG;
  if (*splits == 0) *splits = ssd_lora_default_splits(K);
  if (*splits < 1 || *splits > SSD_LORA_MAX_SPLITS || *splits > (K >> 5)) return SSD_ERR_ARG;
  if (ws_bytes < (long)*splits * M * R * 4) return SSD_ERR_ARG;
  return SSD_OK;
}

extern "C" int ssd_lora_shrink(const void* x_frag, const void* a_frag, const int32_t* row_slot, float* ws, long ws_bytes, int M, int K,
                               int R, int slots, int splits, void* stream) {
  if (!x_frag || !a_frag || !row_slot || !ws) return SSD_ERR_ARG;
  const int rc = lora_check(M, K, R, slots, &splits, ws_bytes);
  if (rc != SSD_OK) return rc;
  const long z = (long)slots * (R >> 4);
  if (z > 65535) return SSD_ERR_SHAPE;
  const dim3 grid((unsigned)splits, (unsigned)((M + LORA_ROWS - 1) / LORA_ROWS), (unsigned)z);
  hipLaunchKernelGGL(lora_shrink_kernel, grid, dim3(LORA_WAVES * 64), 0, (hipStream_t)stream, (const u32x4_t*)x_frag,
                     (const u32x4_t*)a_frag, row_slot, ws, M, K, R, slots, splits);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_lora_expand(const float* ws, long ws_bytes, const void* b_frag, const float* scale, const int32_t* row_slot, void* y,
                               int ldy, void* act_frag, int M, int N, int K, int R, int slots, int splits, int epilogue, void* stream) {
  if (!ws || !b_frag || !scale || !row_slot || !y) return SSD_ERR_ARG;
  if (epilogue != SSD_LORA_EPI_ADD && epilogue != SSD_LORA_EPI_SILU) return SSD_ERR_ARG;
  if (epilogue == SSD_LORA_EPI_SILU && !act_frag) return SSD_ERR_ARG;
  if (N <= 0 || (N & 15) || ldy < N) return SSD_ERR_SHAPE;
  if (epilogue == SSD_LORA_EPI_SILU && (N & 63)) return SSD_ERR_SHAPE;
  const int rc = lora_check(M, K, R, slots, &splits, ws_bytes);
  if (rc != SSD_OK) return rc;
  const int units = (N >> 4) / (epilogue == SSD_LORA_EPI_SILU ? 2 : 1);
  // at most 256 workgroups per 32 token rows: every workgroup sums the slabs of its rows itself
  const int upw = (units + LORA_WAVES * 256 - 1) / (LORA_WAVES * 256);
  const int per = LORA_WAVES * upw;
  const long chunks = (M + LORA_ROWS - 1) / LORA_ROWS;
  if (chunks > 65535) return SSD_ERR_SHAPE;
  const dim3 grid((unsigned)((units + per - 1) / per), (unsigned)chunks);
#define LORA_EXPAND(EPI, RT)                                                                                                     \
  hipLaunchKernelGGL((lora_expand_kernel<EPI, RT>), grid, dim3(LORA_WAVES * 64), 0, (hipStream_t)stream, ws, (const u32x4_t*)b_frag, \
                     scale, row_slot, (bf16_t*)y, ldy, (u32x2_t*)act_frag, M, N, R, slots, splits, upw)
#define LORA_EXPAND_RT(RT)                                                                                                       \
  case RT:                                                                                                                       \
    if (epilogue == SSD_LORA_EPI_SILU) LORA_EXPAND(SSD_LORA_EPI_SILU, RT); else LORA_EXPAND(SSD_LORA_EPI_ADD, RT);                \
    break;
  switch (R >> 5) {
    LORA_EXPAND_RT(1) LORA_EXPAND_RT(2) LORA_EXPAND_RT(3) LORA_EXPAND_RT(4) LORA_EXPAND_RT(5) LORA_EXPAND_RT(6)
    default: return SSD_ERR_SHAPE;
  }
#undef LORA_EXPAND_RT
#undef LORA_EXPAND
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}
