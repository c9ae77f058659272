// FP8 (OCP e4m3fn) weight-only GEMMs for the quantized target: y = x . (s (.) q)^T with bf16 activations, e4m3 weight codes and one
// fp32 scale per output row (include/ssd_hip_quant.h).  Same structure as gemm_wf_kernel (gemm.hip), which this mirrors:
//  * q is stored "fp8 frag": one 1 KiB unit per (16-row group, 64-column k-pair), lane l holding its 8-byte slices of k-tiles 2p and
//    2p+1 side by side -- one 16-byte lane load, one contiguous 1 KiB wave load, two MFMA k-steps.
//  * codes go straight to VGPRs with non-temporal loads and are widened with v_cvt_scalef32_pk_bf16_fp8 at scale 1.0: every e4m3
//    value is a bf16 value, so the conversion is exact and the MFMA is the bf16 one with fp32 accumulation.
//  * one workgroup owns NT row groups for the whole K; its waves split K and combine through LDS in a fixed order (deterministic).
//  * the row scale (and the bias) are applied to the fp32 sums in the epilogue.
#include "common.h"

enum { F8_ROWS = SSD_EPI_ROWS, F8_SILU_FRAG = SSD_EPI_SILU_FRAG };

// 8 e4m3 codes (two 32-bit words) -> the 8 bf16 of one MFMA operand slice
__device__ __forceinline__ u32x4_t fp8x8_to_bf16(uint32_t w0, uint32_t w1) {
  u32x4_t r;
  r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false));
  r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true));
  r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false));
  r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true));
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// Layout: row-major codes -> fp8 frag (with an optional destination -> source row map), and back.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void fp8_rows_to_frag_kernel(const uint8_t* __restrict__ src, u32x4_t* __restrict__ dst, const int32_t* __restrict__ row_map,
                                        int N, int K, long total) {
  const int KP = K >> 6;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
    const long unit = c >> 6;
    const int lane = (int)(c & 63);
    const int g = (int)(unit / KP), p = (int)(unit % KP);
    const int r = g * 16 + (lane & 15);
    const int sr = row_map ? row_map[r] : r;
    const uint8_t* row = src + (size_t)sr * K + (size_t)p * 64 + 8 * (lane >> 4);
    const u32x2_t lo = *reinterpret_cast<const u32x2_t*>(row);
    const u32x2_t hi = *reinterpret_cast<const u32x2_t*>(row + 32);
    dst[c] = u32x4_t{lo[0], lo[1], hi[0], hi[1]};
  }
}

__global__ void fp8_frag_to_rows_kernel(const u32x4_t* __restrict__ src, uint8_t* __restrict__ dst, int N, int K, long total) {
  const int KP = K >> 6;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
    const long unit = c >> 6;
    const int lane = (int)(c & 63);
    const int g = (int)(unit / KP), p = (int)(unit % KP);
    const int r = g * 16 + (lane & 15);
    uint8_t* row = dst + (size_t)r * K + (size_t)p * 64 + 8 * (lane >> 4);
    const u32x4_t v = src[c];
    *reinterpret_cast<u32x2_t*>(row) = u32x2_t{v[0], v[1]};
    *reinterpret_cast<u32x2_t*>(row + 32) = u32x2_t{v[2], v[3]};
  }
}

// fp8 frag unit (g, p) -> the bf16 frag chunks of k-tiles 2p and 2p+1 of the same lane, bf16(s[r] * q)
__global__ void fp8_dequant_frag_kernel(const u32x4_t* __restrict__ src, const float* __restrict__ scale, u32x4_t* __restrict__ dst,
                                        int N, int K, long total) {
  const int KP = K >> 6, KT = K >> 5;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
    const long unit = c >> 6;
    const int lane = (int)(c & 63);
    const int g = (int)(unit / KP), p = (int)(unit % KP);
    const float s = scale[g * 16 + (lane & 15)];
    const u32x4_t v = src[c];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const u32x4_t b = fp8x8_to_bf16(v[2 * h], v[2 * h + 1]);
      u32x4_t o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = pack_bf2(s * bf2f(b[i] & 0xffffu), s * bf2f(b[i] >> 16));
      dst[((size_t)g * KT + 2 * p + h) * 64 + lane] = o;
    }
  }
}

static int grid_for(long total) {
  long blocks = (total + 255) / 256;
  return (int)(blocks > 65536 ? 65536 : blocks);
}

extern "C" int ssd_fp8_rows_to_frag(const void* q_rows, void* q_frag, const int32_t* row_map, int N, int K, void* stream) {
  if (N <= 0 || K <= 0 || (N & 15) || (K & 63)) return SSD_ERR_SHAPE;
  if (!q_rows || !q_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 64) * 64;
  hipLaunchKernelGGL(fp8_rows_to_frag_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)q_rows,
                     (u32x4_t*)q_frag, row_map, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_fp8_frag_to_rows(const void* q_frag, void* q_rows, int N, int K, void* stream) {
  if (N <= 0 || K <= 0 || (N & 15) || (K & 63)) return SSD_ERR_SHAPE;
  if (!q_rows || !q_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 64) * 64;
  hipLaunchKernelGGL(fp8_frag_to_rows_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (uint8_t*)q_rows, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_fp8_dequant_frag(const void* q_frag, const float* scale, void* w_frag, int N, int K, void* stream) {
  if (N <= 0 || K <= 0 || (N & 15) || (K & 63)) return SSD_ERR_SHAPE;
  if (!q_frag || !scale || !w_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 64) * 64;
  hipLaunchKernelGGL(fp8_dequant_frag_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag, scale,
                     (u32x4_t*)w_frag, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------
// The GEMM.  U = k-pairs per stage and wave (the bytes in flight per wave are U * NT KiB of codes); K is dealt to the waves in
// groups of U k-pairs round-robin, the < U left-over pairs go to the last wave (gemm_wf_kernel's walk).
// ---------------------------------------------------------------------------------------------------------------------
template <int MT, int NT>
struct F8Stage {
  u32x4_t a[NT];          // 16 codes per lane: k-tiles 2p, 2p+1
  u32x4_t b[MT][2];       // x operands of the two k-tiles
};

template <int MT, int NT, int EPI, int U>
__global__ void __launch_bounds__(512)
gemm_fp8_kernel(const u32x4_t* __restrict__ Qf, const u32x4_t* __restrict__ Xf, const float* __restrict__ scale,
                const bf16_t* __restrict__ bias, void* __restrict__ Yv, int M, int N, int K, int ldy, int tpw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = blockDim.x >> 6;
  const int KP = K >> 6, KT = K >> 5;
  const int ntiles = (N / 16) / NT;
  const int t_begin = blockIdx.x * tpw, t_end = min(ntiles, t_begin + tpw);
  const u32x4_t* xp = Xf + lane;
  const size_t wstride = (size_t)KP << 6;   // 16-byte chunks between adjacent row groups of q
  const size_t xstride = (size_t)KT << 6;   // ... of x
  const int kstep = nw * U;
  const int kp0 = wave * U;
  const int kmain = (KP / U) * U;
  const u32x4_t* wp = Qf + ((size_t)t_begin * NT * KP << 6) + lane;
  const int mt_last = (M - 1) >> 4;
  auto xload = [&](int mt, int kt) -> u32x4_t {
    // token rows >= M of the last 16-row tile are padding: their lanes do not load; m-tiles past the last one re-read it
    u32x4_t b = {0u, 0u, 0u, 0u};
    if (NT > 1 || mt * 16 + (lane & 15) < M) b = xp[(mt < mt_last ? mt : mt_last) * xstride + ((size_t)kt << 6)];
    return b;
  };
  auto load = [&](F8Stage<MT, NT>(&s)[U], int kp) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) s[u].a[nt] = __builtin_nontemporal_load(wp + nt * wstride + ((size_t)(kp + u) << 6));
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        s[u].b[mt][0] = xload(mt, 2 * (kp + u));
        s[u].b[mt][1] = xload(mt, 2 * (kp + u) + 1);
      }
    }
  };
  F8Stage<MT, NT> cur[U], nxt[U];
  if (t_begin < t_end && kp0 < kmain) load(cur, kp0);

  for (int tile = t_begin; tile < t_end; ++tile) {
    const int tile0 = tile * NT;
    f32x4_t acc[NT][MT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    auto step = [&](const u32x4_t& a, const u32x4_t (&b)[MT][2], int nt) {
      const u32x4_t a0 = fp8x8_to_bf16(a[0], a[1]), a1 = fp8x8_to_bf16(a[2], a[3]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        acc[nt][mt] = mfma16(a0, b[mt][0], acc[nt][mt]);
        acc[nt][mt] = mfma16(a1, b[mt][1], acc[nt][mt]);
      }
    };
    auto compute = [&](F8Stage<MT, NT>(&s)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) step(s[u].a[nt], s[u].b, nt);
    };

    int kp = kp0;
    if (kp < kmain) {
      for (; kp + kstep < kmain; kp += kstep) {
        load(nxt, kp + kstep);
        compute(cur);
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
      }
      compute(cur);
    }
    for (kp = (wave == nw - 1) ? kmain : KP; kp < KP; ++kp) {   // K remainder (< U pairs): last wave
      u32x4_t b[MT][2];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        b[mt][0] = xload(mt, 2 * kp);
        b[mt][1] = xload(mt, 2 * kp + 1);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) step(__builtin_nontemporal_load(wp + nt * wstride + ((size_t)kp << 6)), b, nt);
    }

    // next tile: advance the weight pointer and put its first loads in flight before the combine
    wp += (size_t)NT * wstride;
    if (tile + 1 < t_end && kp0 < kmain) load(cur, kp0);

    // ---- cross-wave split-K combine through LDS, fixed order ----
    f32x4_t* red = reinterpret_cast<f32x4_t*>(smem);  // [nw][NT*MT][64]
    constexpr int ITEMS = NT * MT;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) red[((wave * ITEMS) + nt * MT + mt) * 64 + lane] = acc[nt][mt];
    __syncthreads();

    const int mcol = lane & 15;        // D column j -> token row m
    const int nrow = (lane >> 4) * 4;  // D rows nrow + r -> output feature n
    if (EPI == F8_SILU_FRAG) {
      constexpr int PAIRS = NT / 2;
      const int KT2 = (N >> 1) >> 5;
      u32x2_t* out = reinterpret_cast<u32x2_t*>(Yv);
      for (int item = wave; item < PAIRS * MT; item += nw) {
        const int pr = item / MT, mt = item % MT;
        f32x4_t g = f32x4_t{0.f, 0.f, 0.f, 0.f}, u = g;
        for (int w = 0; w < nw; ++w) {
          g += red[((w * ITEMS) + (2 * pr) * MT + mt) * 64 + lane];
          u += red[((w * ITEMS) + (2 * pr + 1) * MT + mt) * 64 + lane];
        }
        const int m = mt * 16 + mcol;
        const int ng = (tile0 + 2 * pr) * 16 + nrow, nu = (tile0 + 2 * pr + 1) * 16 + nrow;   // packed rows of gate / up
        const int n = ((tile0 >> 1) + pr) * 16 + nrow;                                       // feature index in [0, N/2)
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float gb = scale[ng + r] * g[r], ub = scale[nu + r] * u[r];
          if (bias) { gb += bf2f(bias[ng + r]); ub += bf2f(bias[nu + r]); }
          gb = round_bf(gb); ub = round_bf(ub);
          o[r] = (gb / (1.0f + __expf(-gb))) * ub;
        }
        if (m < M) out[frag_chunk(m, n >> 3, KT2) * 2 + ((n >> 2) & 1)] = u32x2_t{pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
      }
    } else {
      for (int item = wave; item < ITEMS; item += nw) {
        const int nt = item / MT, mt = item % MT;
        f32x4_t s = f32x4_t{0.f, 0.f, 0.f, 0.f};
        for (int w = 0; w < nw; ++w) s += red[((w * ITEMS) + item) * 64 + lane];
        const int m = mt * 16 + mcol;
        const int n = (tile0 + nt) * 16 + nrow;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[r] = scale[n + r] * s[r];
          if (bias) s[r] += bf2f(bias[n + r]);
        }
        if (m < M)
          *reinterpret_cast<u32x2_t*>(reinterpret_cast<bf16_t*>(Yv) + (size_t)m * ldy + n) = u32x2_t{pack_bf2(s[0], s[1]), pack_bf2(s[2], s[3])};
      }
    }
    __syncthreads();   // the combine area is reused by the next tile
  }
}

template <int MT, int NT, int EPI, int U>
static int f8_launch(const void* x, const void* q, const float* scale, const void* bias, void* y, int M, int N, int K, int ldy,
                     int waves, int tpw, hipStream_t st) {
  const int ntiles = (N / 16) / NT;
  if (tpw < 1) tpw = 1;
  const int blocks = (ntiles + tpw - 1) / tpw;
  const size_t lds = (size_t)waves * NT * MT * 64 * sizeof(f32x4_t);
  if (lds > 64 * 1024) return SSD_ERR_ARG;
  hipLaunchKernelGGL((gemm_fp8_kernel<MT, NT, EPI, U>), dim3(blocks), dim3(waves * 64), lds, st, (const u32x4_t*)q,
                     (const u32x4_t*)x, scale, (const bf16_t*)bias, y, M, N, K, ldy, tpw);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// U per (MT, NT, deep): 4-8 KiB of codes in flight per wave in the plain form, twice that in the deep one, within the VGPR budget
// of a <= 8-wave workgroup (256 per lane: the double-buffered stage is 2 * U * (4 NT + 8 MT) VGPRs)
template <int MT, int EPI>
static int f8_dispatch_nt(const void* x, const void* q, const float* scale, const void* bias, void* y, int M, int N, int K, int ldy,
                          int nt, bool deep, int waves, int tpw, hipStream_t st) {
#define F8L(NTV, UV) return f8_launch<MT, NTV, EPI, UV>(x, q, scale, bias, y, M, N, K, ldy, waves, tpw, st)
  if constexpr (MT == 1) {
    if (nt == 1) { if constexpr (EPI == F8_SILU_FRAG) return SSD_ERR_ARG; else { if (deep) F8L(1, 6); F8L(1, 4); } }
    if (nt == 2) { if (deep) F8L(2, 4); F8L(2, 2); }
    if (nt == 4) { if (deep) F8L(4, 2); F8L(4, 1); }
  } else if constexpr (MT == 2) {
    if (deep) return SSD_ERR_ARG;
    if (nt == 1) { if constexpr (EPI == F8_SILU_FRAG) return SSD_ERR_ARG; else F8L(1, 2); }
    if (nt == 2) F8L(2, 2);
  } else {
    if (deep) return SSD_ERR_ARG;
    if (nt == 1) { if constexpr (EPI == F8_SILU_FRAG) return SSD_ERR_ARG; else F8L(1, 1); }
    if (nt == 2) F8L(2, 1);
  }
#undef F8L
  return SSD_ERR_ARG;
}

extern "C" int ssd_gemm_fp8_cfg(const void* x_frag, const void* q_frag, const float* scale, const void* bias, void* y, int M, int N, int K,
                                int ldy, int epilogue, int nt, int waves, void* stream) {
  if (M <= 0 || M > 128 || N <= 0 || K <= 0 || (N & 15) || (K & 63)) return SSD_ERR_SHAPE;
  if (!x_frag || !q_frag || !scale || !y) return SSD_ERR_ARG;
  if (epilogue == F8_ROWS && ldy < N) return SSD_ERR_SHAPE;
  const int tpw = (waves >> 8) & 0xff;
  const bool deep = (nt >> 8) & 1;
  waves &= 0xff;
  nt &= 0xff;
  if (waves < 1 || waves > 8 || (nt != 1 && nt != 2 && nt != 4) || ((N / 16) % nt) != 0) return SSD_ERR_ARG;
  if (epilogue == F8_SILU_FRAG && ((nt & 1) || (N & 63))) return SSD_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int mt = (M + 15) / 16;
#define F8_MT(MTV)                                                                                                               \
  switch (epilogue) {                                                                                                            \
    case F8_ROWS: return f8_dispatch_nt<MTV, F8_ROWS>(x_frag, q_frag, scale, bias, y, M, N, K, ldy, nt, deep, waves, tpw, st);       \
    case F8_SILU_FRAG: return f8_dispatch_nt<MTV, F8_SILU_FRAG>(x_frag, q_frag, scale, bias, y, M, N, K, ldy, nt, deep, waves, tpw, st); \
    default: return SSD_ERR_ARG;                                                                                                 \
  }
  if (mt == 1) { F8_MT(1) }
  if (mt == 2) { F8_MT(2) }
  if (mt <= 4) { F8_MT(4) }
  { F8_MT(8) }
#undef F8_MT
}

// Default decomposition.  One token tile: the bf16 skinny table at the k-pair count (a 1 KiB unit covers 64 columns here, 32 in
// bf16, so a matrix streams like a bf16 one of half its K), in the plain form, re-tuned where the 70B verify shapes were swept at
// M = 8 (profiles/fp8_sweep.jsonl, every nt / deep / waves / tpw): gate_up 81.3 -> 75.9 us with 4 consecutive tiles per workgroup,
// o_proj 16.1 -> 13.4 and down_proj 43.3 -> 41.1 with 2 row groups x 8 waves, qkv 22.1 -> 18.7 with 4 waves.  More token tiles: one
// or two row groups per workgroup, waves sized so that every wave has a few k-pairs, LDS for the combine <= 64 KiB.
extern "C" int ssd_gemm_fp8(const void* x_frag, const void* q_frag, const float* scale, const void* bias, void* y, int M, int N, int K,
                            int ldy, int epilogue, void* stream) {
  if (M <= 0 || M > 128 || N <= 0 || K <= 0 || (N & 15) || (K & 63)) return SSD_ERR_SHAPE;
  const int groups = N / 16, KP = K / 64, mt = (M + 15) / 16;
  const bool silu = epilogue == F8_SILU_FRAG;
  int nt, waves, tpw = 1;
  if (mt == 1) {
    ssd_pick_skinny_cfg(groups, KP, silu, &nt, &waves, &tpw);
    if (silu && nt == 4) {
      const int cand[] = {4, 3, 2, 1};
      tpw = ssd_pick_tpw(groups / 4, cand, 4);
      waves = 8;
    } else if (!silu && groups == 512 && KP >= 128) {        // 70B-class o_proj / down_proj
      nt = 2; waves = 8; tpw = 1;
    } else if (!silu && nt == 1 && tpw == 1 && waves > 4 && KP <= 128) {
      waves = 4;                                             // 70B-class qkv
    }
    if (waves > 8) waves = 8;
    return ssd_gemm_fp8_cfg(x_frag, q_frag, scale, bias, y, M, N, K, ldy, epilogue, nt, waves | (tpw << 8), stream);
  }
  nt = (epilogue == F8_SILU_FRAG || (groups >= 2048 && groups % 2 == 0)) ? 2 : 1;
  waves = 8;
  while (waves > 1 && KP / waves < 4) waves >>= 1;
  const int mtr = mt == 2 ? 2 : (mt <= 4 ? 4 : 8);
  while (waves > 1 && (size_t)waves * nt * mtr * 1024 > 64 * 1024) waves >>= 1;
  return ssd_gemm_fp8_cfg(x_frag, q_frag, scale, bias, y, M, N, K, ldy, epilogue, nt, waves, stream);
}
