// MXFP4 weight-only GEMMs for the quantized target: y = x . W^T with bf16 activations and W = 2^(b - 127) * e2m1(q), e2m1 weight codes
// with one e8m0 scale byte per output row and 32-column block (include/ssd_hip_mxfp4.h).  Same skeleton as gemm_w4a16_kernel
// (gemm_w4a16.hip):
//  * q is stored "mx4 frag": one 1 KiB unit per (16-row group, 128-column group), lane l holding its 8-column slices of the group's
//    four k-tiles -- one 16-byte lane load, one contiguous 1 KiB wave load, four MFMA k-steps; the four scale bytes of the lane's row
//    for those k-tiles are one 4-byte load.
//  * codes go straight to VGPRs with non-temporal loads.  What differs is the inner step: v_cvt_scalef32_pk_bf16_fp4 turns one byte
//    (two codes) into two bf16 already multiplied by the block scale, four conversions per 8 weights.  An MX block is one k-tile of
//    v_mfma_f32_16x16x32_bf16, so a lane's operand slice has ONE scale; 2^e * {0, .5, 1, 1.5, 2, 3, 4, 6} is exact in bf16, so the
//    operand is the exact weight and the MFMA goes straight into the row accumulator: no offset, no per-group partial, no scale fma.
//  * one workgroup owns NT row groups for the whole K; its waves split K and combine through LDS in a fixed order (deterministic).
#include "common.h"

enum { MX4_ROWS = SSD_EPI_ROWS, MX4_SILU_FRAG = SSD_EPI_SILU_FRAG };

typedef __attribute__((ext_vector_type(2))) __bf16 mx4_bf16x2_t;

// scale byte b (2 <= b <= 252) -> the fp32 2^(b - 127)
__device__ __forceinline__ float mx4_scale(uint32_t quad, int j) { return __uint_as_float(((quad >> (8 * j)) & 0xffu) << 23); }

// one frag word (8 codes, column e in bits 4e .. 4e+3) -> the 8 bf16 of one MFMA operand slice, each scale * e2m1 (exact)
__device__ __forceinline__ u32x4_t mx4_to_bf16(uint32_t w, float scale) {
  u32x4_t r;
  r[0] = __builtin_bit_cast(uint32_t, (mx4_bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0));
  r[1] = __builtin_bit_cast(uint32_t, (mx4_bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1));
  r[2] = __builtin_bit_cast(uint32_t, (mx4_bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2));
  r[3] = __builtin_bit_cast(uint32_t, (mx4_bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3));
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// Layout: row form -> mx4 frag (with an optional destination -> source row map), and back; dequantize into a bf16 frag.
// One thread per 16-byte lane chunk of a unit; lanes 0..15 of a unit also move the four scale bytes of their row.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void mx4_rows_to_frag_kernel(const uint32_t* __restrict__ q_src, const uint32_t* __restrict__ s_src,
                                        u32x4_t* __restrict__ q_dst, uint32_t* __restrict__ s_dst, const int32_t* __restrict__ row_map,
                                        int N, int K, long total) {
  const int KG = K >> 7, KW = K >> 3;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
    const long unit = c >> 6;
    const int lane = (int)(c & 63);
    const int g = (int)(unit / KG), cg = (int)(unit % KG);
    const int r = g * 16 + (lane & 15);
    const int sr = row_map ? row_map[r] : r;
    const uint32_t* row = q_src + (size_t)sr * KW + (size_t)cg * 16 + (lane >> 4);
    u32x4_t v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = row[4 * j];
    q_dst[c] = v;
    if (lane < 16) s_dst[unit * 16 + lane] = s_src[(size_t)sr * KG + cg];   // K/32 scale bytes per row = KG aligned quads
  }
}

__global__ void mx4_frag_to_rows_kernel(const u32x4_t* __restrict__ q_src, const uint32_t* __restrict__ s_src,
                                        uint32_t* __restrict__ q_dst, uint32_t* __restrict__ s_dst, int N, int K, long total) {
  const int KG = K >> 7, KW = K >> 3;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
    const long unit = c >> 6;
    const int lane = (int)(c & 63);
    const int g = (int)(unit / KG), cg = (int)(unit % KG);
    const int r = g * 16 + (lane & 15);
    uint32_t* row = q_dst + (size_t)r * KW + (size_t)cg * 16 + (lane >> 4);
    const u32x4_t v = q_src[c];
#pragma unroll
    for (int j = 0; j < 4; ++j) row[4 * j] = v[j];
    if (lane < 16) s_dst[(size_t)r * KG + cg] = s_src[unit * 16 + lane];
  }
}

// mx4 frag unit (g, cg), lane l -> the bf16 frag chunks of k-tiles 4cg .. 4cg+3 of the same lane, 2^(b - 127) * e2m1(q)
__global__ void mx4_dequant_frag_kernel(const u32x4_t* __restrict__ q_src, const uint32_t* __restrict__ s_src, u32x4_t* __restrict__ dst,
                                        int N, int K, long total) {
  const int KG = K >> 7, KT = K >> 5;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
    const long unit = c >> 6;
    const int lane = (int)(c & 63);
    const int g = (int)(unit / KG), cg = (int)(unit % KG);
    const uint32_t quad = s_src[unit * 16 + (lane & 15)];
    const u32x4_t v = q_src[c];
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[((size_t)g * KT + 4 * cg + j) * 64 + lane] = mx4_to_bf16(v[j], mx4_scale(quad, j));
  }
}

static int grid_for(long total) {
  long blocks = (total + 255) / 256;
  return (int)(blocks > 65536 ? 65536 : blocks);
}

static bool mx4_shape_ok(int N, int K) { return N > 0 && K > 0 && (N & 15) == 0 && (K & 127) == 0; }

extern "C" int ssd_mx4_rows_to_frag(const void* q_rows, const void* s_rows, void* q_frag, void* s_frag, const int32_t* row_map, int N,
                                    int K, void* stream) {
  if (!mx4_shape_ok(N, K)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !q_frag || !s_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(mx4_rows_to_frag_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)q_rows,
                     (const uint32_t*)s_rows, (u32x4_t*)q_frag, (uint32_t*)s_frag, row_map, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_mx4_frag_to_rows(const void* q_frag, const void* s_frag, void* q_rows, void* s_rows, int N, int K, void* stream) {
  if (!mx4_shape_ok(N, K)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !q_frag || !s_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(mx4_frag_to_rows_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const uint32_t*)s_frag, (uint32_t*)q_rows, (uint32_t*)s_rows, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_mx4_dequant_frag(const void* q_frag, const void* s_frag, void* w_frag, int N, int K, void* stream) {
  if (!mx4_shape_ok(N, K)) return SSD_ERR_SHAPE;
  if (!q_frag || !s_frag || !w_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(mx4_dequant_frag_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const uint32_t*)s_frag, (u32x4_t*)w_frag, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------
// The GEMM.  U = column groups per stage and wave (the code bytes in flight per wave are U * NT KiB); K is dealt to the waves in
// runs of U column groups round-robin, the < U left-over groups go to the last wave (gemm_fp8_kernel's walk).  XS: the x operands
// ride in the double-buffered stage (MT <= 4); at MT = 8 they would not fit the VGPR budget and are loaded per group instead.
// ---------------------------------------------------------------------------------------------------------------------
template <int MT, int NT, bool XS>
struct Mx4Stage {
  u32x4_t a[NT];                  // 32 codes per lane: k-tiles 4c .. 4c+3
  uint32_t s[NT];                 // the 4 scale bytes of the lane's weight row for those k-tiles
  u32x4_t b[XS ? MT : 1][4];      // x operands of the four k-tiles
};

template <int MT, int NT, int EPI, int U, bool XS>
__global__ void __launch_bounds__(512)
gemm_mxfp4_kernel(const u32x4_t* __restrict__ Qf, const uint32_t* __restrict__ Sf, const u32x4_t* __restrict__ Xf,
                  const bf16_t* __restrict__ bias, void* __restrict__ Yv, int M, int N, int K, int ldy, int tpw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = blockDim.x >> 6;
  const int KG = K >> 7, KT = K >> 5;
  const int ntiles = (N / 16) / NT;
  const int t_begin = blockIdx.x * tpw, t_end = min(ntiles, t_begin + tpw);
  const u32x4_t* xp = Xf + lane;
  const size_t wstride = (size_t)KG << 6;   // 16-byte chunks between adjacent row groups of q
  const size_t sstride = (size_t)KG << 4;   // 4-byte scale quads between adjacent row groups of s
  const size_t xstride = (size_t)KT << 6;   // 16-byte chunks between adjacent token tiles of x
  const int kstep = nw * U;
  const int kg0 = wave * U;
  const int kmain = (KG / U) * U;
  const u32x4_t* wp = Qf + ((size_t)t_begin * NT * wstride) + lane;
  const uint32_t* sp = Sf + ((size_t)t_begin * NT * sstride) + (lane & 15);
  const int mt_last = (M - 1) >> 4;
  auto xload = [&](int mt, int kt) -> u32x4_t {
    // token rows >= M of the last 16-row tile are padding: their lanes do not load; m-tiles past the last one re-read it
    u32x4_t b = {0u, 0u, 0u, 0u};
    if (NT > 1 || mt * 16 + (lane & 15) < M) b = xp[(mt < mt_last ? mt : mt_last) * xstride + ((size_t)kt << 6)];
    return b;
  };
  auto xgroup = [&](u32x4_t (&b)[XS ? MT : 1][4], int kg) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < 4; ++j) b[mt][j] = xload(mt, 4 * kg + j);
  };
  auto load = [&](Mx4Stage<MT, NT, XS>(&s)[U], int kg) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        s[u].a[nt] = __builtin_nontemporal_load(wp + nt * wstride + ((size_t)(kg + u) << 6));
        s[u].s[nt] = __builtin_nontemporal_load(sp + nt * sstride + ((size_t)(kg + u) << 4));
      }
      if constexpr (XS) xgroup(s[u].b, kg + u);
    }
  };
  Mx4Stage<MT, NT, XS> cur[U], nxt[U];
  if (t_begin < t_end && kg0 < kmain) load(cur, kg0);

  for (int tile = t_begin; tile < t_end; ++tile) {
    const int tile0 = tile * NT;
    f32x4_t acc[NT][MT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // one column group: convert each row group's four k-tile slices with their block scales, then MFMA straight into the row
    // accumulators.  With XS the x operands come from the stage; without, each token tile's four are loaded here (from L2: x is
    // shared by every workgroup).
    auto group = [&](const u32x4_t (&a)[NT], const uint32_t (&sc)[NT], const u32x4_t (&bs)[XS ? MT : 1][4], int kg) {
      u32x4_t w[NT][4];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) w[nt][j] = mx4_to_bf16(a[nt][j], mx4_scale(sc[nt], j));
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        u32x4_t b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = XS ? bs[XS ? mt : 0][j] : xload(mt, 4 * kg + j);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[nt][mt] = mfma16(w[nt][j], b[j], acc[nt][mt]);
      }
    };
    auto compute = [&](Mx4Stage<MT, NT, XS>(&s)[U], int kg) {
#pragma unroll
      for (int u = 0; u < U; ++u) group(s[u].a, s[u].s, s[u].b, kg + u);
    };

    int kg = kg0;
    if (kg < kmain) {
      for (; kg + kstep < kmain; kg += kstep) {
        load(nxt, kg + kstep);
        compute(cur, kg);
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
      }
      compute(cur, kg);
    }
    for (kg = (wave == nw - 1) ? kmain : KG; kg < KG; ++kg) {   // K remainder (< U groups): last wave
      u32x4_t a[NT], b[XS ? MT : 1][4];
      uint32_t sc[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        a[nt] = __builtin_nontemporal_load(wp + nt * wstride + ((size_t)kg << 6));
        sc[nt] = __builtin_nontemporal_load(sp + nt * sstride + ((size_t)kg << 4));
      }
      if constexpr (XS) xgroup(b, kg);
      group(a, sc, b, kg);
    }

    // next tile: advance the weight pointers and put its first loads in flight before the combine
    wp += (size_t)NT * wstride;
    sp += (size_t)NT * sstride;
    if (tile + 1 < t_end && kg0 < kmain) load(cur, kg0);

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
    if (EPI == MX4_SILU_FRAG) {
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
          float gb = g[r], ub = u[r];
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
        if (bias) {
#pragma unroll
          for (int r = 0; r < 4; ++r) s[r] += bf2f(bias[n + r]);
        }
        if (m < M)
          *reinterpret_cast<u32x2_t*>(reinterpret_cast<bf16_t*>(Yv) + (size_t)m * ldy + n) = u32x2_t{pack_bf2(s[0], s[1]), pack_bf2(s[2], s[3])};
      }
    }
    __syncthreads();   // the combine area is reused by the next tile
  }
}

template <int MT, int NT, int EPI, int U, bool XS>
static int mx4_launch(const void* x, const void* q, const void* s, const void* bias, void* y, int M, int N, int K, int ldy, int waves,
                      int tpw, hipStream_t st) {
  const int ntiles = (N / 16) / NT;
  if (tpw < 1) tpw = 1;
  const int blocks = (ntiles + tpw - 1) / tpw;
  const size_t lds = (size_t)waves * NT * MT * 64 * sizeof(f32x4_t);
  if (lds > 64 * 1024) return SSD_ERR_ARG;
  hipLaunchKernelGGL((gemm_mxfp4_kernel<MT, NT, EPI, U, XS>), dim3(blocks), dim3(waves * 64), lds, st, (const u32x4_t*)q,
                     (const uint32_t*)s, (const u32x4_t*)x, (const bf16_t*)bias, y, M, N, K, ldy, tpw);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// U per (MT, NT, deep): as gemm_w4a16.hip -- 2-4 KiB of codes in flight per wave in the plain form (x staged with them), twice that
// in the deep one (x loaded per group), within the VGPR budget of a <= 8-wave workgroup without spills (the double-buffered stage is
// 2 U (5 NT + 16 MT) VGPRs with x in it, 10 U NT without)
template <int MT, int EPI>
static int mx4_dispatch_nt(const void* x, const void* q, const void* s, const void* bias, void* y, int M, int N, int K, int ldy, int nt,
                           bool deep, int waves, int tpw, hipStream_t st) {
#define MX4L(NTV, UV, XSV) return mx4_launch<MT, NTV, EPI, UV, XSV>(x, q, s, bias, y, M, N, K, ldy, waves, tpw, st)
  if constexpr (MT == 1) {
    if (nt == 1) { if constexpr (EPI == MX4_SILU_FRAG) return SSD_ERR_ARG; else { if (deep) MX4L(1, 8, false); MX4L(1, 2, true); } }
    if (nt == 2) { if (deep) MX4L(2, 4, false); MX4L(2, 1, true); }
    if (nt == 4) { if (deep) MX4L(4, 2, false); MX4L(4, 1, true); }
  } else if constexpr (MT == 2) {
    if (deep) return SSD_ERR_ARG;
    if (nt == 1) { if constexpr (EPI == MX4_SILU_FRAG) return SSD_ERR_ARG; else MX4L(1, 2, true); }
    if (nt == 2) MX4L(2, 1, true);
  } else if constexpr (MT == 4) {
    if (deep) return SSD_ERR_ARG;
    if (nt == 1) { if constexpr (EPI == MX4_SILU_FRAG) return SSD_ERR_ARG; else MX4L(1, 1, true); }
    if (nt == 2) MX4L(2, 1, true);
  } else {
    if (deep) return SSD_ERR_ARG;
    if (nt == 1) { if constexpr (EPI == MX4_SILU_FRAG) return SSD_ERR_ARG; else MX4L(1, 1, false); }
    if (nt == 2) MX4L(2, 1, false);
  }
#undef MX4L
  return SSD_ERR_ARG;
}

extern "C" int ssd_gemm_mxfp4_cfg(const void* x_frag, const void* q_frag, const void* s_frag, const void* bias, void* y, int M, int N,
                                  int K, int ldy, int epilogue, int nt, int waves, void* stream) {
  if (M <= 0 || M > 128 || !mx4_shape_ok(N, K)) return SSD_ERR_SHAPE;
  if (!x_frag || !q_frag || !s_frag || !y) return SSD_ERR_ARG;
  if (epilogue == MX4_ROWS && ldy < N) return SSD_ERR_SHAPE;
  const int tpw = (waves >> 8) & 0xff;
  const bool deep = (nt >> 8) & 1;
  waves &= 0xff;
  nt &= 0xff;
  if (waves < 1 || waves > 8 || (nt != 1 && nt != 2 && nt != 4) || ((N / 16) % nt) != 0) return SSD_ERR_ARG;
  if (epilogue == MX4_SILU_FRAG && ((nt & 1) || (N & 63))) return SSD_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int mt = (M + 15) / 16;
#define MX4_MT(MTV)                                                                                                                      \
  switch (epilogue) {                                                                                                                    \
    case MX4_ROWS: return mx4_dispatch_nt<MTV, MX4_ROWS>(x_frag, q_frag, s_frag, bias, y, M, N, K, ldy, nt, deep, waves, tpw, st);        \
    case MX4_SILU_FRAG: return mx4_dispatch_nt<MTV, MX4_SILU_FRAG>(x_frag, q_frag, s_frag, bias, y, M, N, K, ldy, nt, deep, waves, tpw, st); \
    default: return SSD_ERR_ARG;                                                                                                         \
  }
  if (mt == 1) { MX4_MT(1) }
  if (mt == 2) { MX4_MT(2) }
  if (mt <= 4) { MX4_MT(4) }
  { MX4_MT(8) }
#undef MX4_MT
}

// Default decomposition.  One token tile: the classes of ssd_gemm_w4a16 (same unit size, same bytes per row group within 3 %), checked
// against the M = 8 sweep of every explicit decomposition at the 1B / 8B / 70B / Qwen3-32B shapes (profiles/mxfp4_sweep.jsonl):
//   gate_up: 4 row groups per workgroup, 2 waves once there are >= 768 such tiles, else 4;
//   qkv-class (>= 640 row groups, K <= 8192): 4 row groups x 8 waves;
//   o / down-class (>= 320 row groups, K >= 8192): 2 row groups x 8 waves;
//   anything smaller: 1 row group x 8 waves.
// More token tiles: one or two row groups per workgroup, waves sized so that every wave has a few column groups, LDS for the
// combine <= 64 KiB.
extern "C" int ssd_gemm_mxfp4(const void* x_frag, const void* q_frag, const void* s_frag, const void* bias, void* y, int M, int N, int K,
                              int ldy, int epilogue, void* stream) {
  if (M <= 0 || M > 128 || !mx4_shape_ok(N, K)) return SSD_ERR_SHAPE;
  const int groups = N / 16, KG = K / 128, mt = (M + 15) / 16;
  const bool silu = epilogue == MX4_SILU_FRAG;
  int nt, waves;
  if (mt == 1) {
    if (silu) {
      nt = groups % 4 == 0 ? 4 : 2;
      waves = groups / nt >= 768 ? 2 : 4;
    } else {
      waves = 8;
      if (groups >= 640 && KG <= 64 && groups % 4 == 0) nt = 4;
      else if (groups >= 320 && KG >= 64 && groups % 2 == 0) nt = 2;
      else nt = 1;
    }
    while (waves > 1 && KG / waves < 2) waves >>= 1;
    return ssd_gemm_mxfp4_cfg(x_frag, q_frag, s_frag, bias, y, M, N, K, ldy, epilogue, nt, waves, stream);
  }
  nt = (silu || (groups >= 2048 && groups % 2 == 0)) ? 2 : 1;
  waves = 8;
  while (waves > 1 && KG / waves < 2) waves >>= 1;
  const int mtr = mt == 2 ? 2 : (mt <= 4 ? 4 : 8);
  while (waves > 1 && (size_t)waves * nt * mtr * 1024 > 64 * 1024) waves >>= 1;
  return ssd_gemm_mxfp4_cfg(x_frag, q_frag, s_frag, bias, y, M, N, K, ldy, epilogue, nt, waves, stream);
}
