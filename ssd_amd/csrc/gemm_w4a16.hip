// W4A16 weight-only GEMMs for the quantized target: y = x . (s (.) q)^T with bf16 activations, signed int4 weight codes and one bf16
// scale per output row and 128-column group (include/ssd_hip_w4a16.h).  Same skeleton as gemm_fp8_kernel (gemm_fp8.hip):
//  * q is stored "w4 frag": one 1 KiB unit per (16-row group, 128-column group), lane l holding its 8-column slices of the group's
//    four k-tiles -- one 16-byte lane load, one contiguous 1 KiB wave load, four MFMA k-steps.
//  * codes go straight to VGPRs with non-temporal loads and are widened exactly, a mask and an or per two weights (plus a shift per
//    nibble position): (word >> 4p) & 0x000F000F | 0x43004300 is the bf16 pair 128 + u = q + 136 (bf16 has one ulp = 1 in [128, 256)).
//  * each column group accumulates into a fresh fp32 partial that starts at -136 * sum(x over the group) (four MFMAs against a
//    constant -136 operand, shared by the workgroup's row groups), so the partial is sum(q * x); the row accumulator takes
//    s * partial in fp32.
//  * one workgroup owns NT row groups for the whole K; its waves split K and combine through LDS in a fixed order (deterministic).
// With zero points (include/ssd_hip_w4zp.h, template parameter ZP) the weight is s * (u - z), z per (row, group): the same walk and
// the same partial p = sum((u - 8) * x).  The constant-operand chain already holds corr = -136 * sum(x) for every row, so per
// accumulator register t = fma((z - 8) / 136, corr, p) = sum((u - z) * x), then acc = fma(s, t, acc): no further MFMA and no
// further live accumulator (a second chain against a constant -1 operand spilled at MT >= 4).  (z - 8) / 136 is rounded to fp32
// (relative 2^-24 on a term no larger than 8 |sum(x)|, below the rounding of p itself, which passes through 136 |sum(x)|); z = 8
// gives t = p, the symmetric kernel's value.  Every difference is under `if constexpr (ZP)`; the ZP = false instantiations are
// the symmetric kernels, unchanged.
#include "common.h"

enum { W4_ROWS = SSD_EPI_ROWS, W4_SILU_FRAG = SSD_EPI_SILU_FRAG };

// row-form word (column i in nibble i) <-> frag word (columns 0, 2, 4, 6, 1, 3, 5, 7 in nibbles 0..7)
__device__ __forceinline__ int w4_nibble_of_col(int e) { return (e & 1) ? 4 + (e >> 1) : (e >> 1); }

__device__ __forceinline__ uint32_t w4_row_to_frag_word(uint32_t w) {
  uint32_t o = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) o |= ((w >> (4 * e)) & 0xfu) << (4 * w4_nibble_of_col(e));
  return o;
}

__device__ __forceinline__ uint32_t w4_frag_to_row_word(uint32_t w) {
  uint32_t o = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) o |= ((w >> (4 * w4_nibble_of_col(e))) & 0xfu) << (4 * e);
  return o;
}

// one frag word -> the 8 bf16 of one MFMA operand slice, each 136 + q (exact)
__device__ __forceinline__ u32x4_t w4_to_bf16_off(uint32_t w) {
  u32x4_t r;
  r[0] = (w & 0x000F000Fu) | 0x43004300u;
  r[1] = ((w >> 4) & 0x000F000Fu) | 0x43004300u;
  r[2] = ((w >> 8) & 0x000F000Fu) | 0x43004300u;
  r[3] = ((w >> 12) & 0x000F000Fu) | 0x43004300u;
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// Layout: row form -> w4 frag (with an optional destination -> source row map), and back; dequantize into a bf16 frag.
// One thread per 16-byte lane chunk of a unit; lanes 0..15 of a unit also move the unit's 16 scales.
// ---------------------------------------------------------------------------------------------------------------------
// ZP: lanes 0..15 also move the unit's 16 zero-point bytes (z_src rows uint8 [N][K/128] <-> z_dst uint8 [N/16][K/128][16]).
template <bool ZP>
__global__ void w4_rows_to_frag_kernel(const uint32_t* __restrict__ q_src, const bf16_t* __restrict__ s_src,
                                       const uint8_t* __restrict__ z_src, u32x4_t* __restrict__ q_dst, bf16_t* __restrict__ s_dst,
                                       uint8_t* __restrict__ z_dst, const int32_t* __restrict__ row_map, int N, int K, long total) {
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
    for (int j = 0; j < 4; ++j) v[j] = w4_row_to_frag_word(row[4 * j]);
    q_dst[c] = v;
    if (lane < 16) {
      s_dst[unit * 16 + lane] = s_src[(size_t)sr * KG + cg];
      if constexpr (ZP) z_dst[unit * 16 + lane] = z_src[(size_t)sr * KG + cg];
    }
  }
}

template <bool ZP>
__global__ void w4_frag_to_rows_kernel(const u32x4_t* __restrict__ q_src, const bf16_t* __restrict__ s_src,
                                       const uint8_t* __restrict__ z_src, uint32_t* __restrict__ q_dst, bf16_t* __restrict__ s_dst,
                                       uint8_t* __restrict__ z_dst, int N, int K, long total) {
  const int KG = K >> 7, KW = K >> 3;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
    const long unit = c >> 6;
    const int lane = (int)(c & 63);
    const int g = (int)(unit / KG), cg = (int)(unit % KG);
    const int r = g * 16 + (lane & 15);
    uint32_t* row = q_dst + (size_t)r * KW + (size_t)cg * 16 + (lane >> 4);
    const u32x4_t v = q_src[c];
#pragma unroll
    for (int j = 0; j < 4; ++j) row[4 * j] = w4_frag_to_row_word(v[j]);
    if (lane < 16) {
      s_dst[(size_t)r * KG + cg] = s_src[unit * 16 + lane];
      if constexpr (ZP) z_dst[(size_t)r * KG + cg] = z_src[unit * 16 + lane];
    }
  }
}

// w4 frag unit (g, cg), lane l -> the bf16 frag chunks of k-tiles 4cg .. 4cg+3 of the same lane, bf16(s * q); ZP: bf16(s * (u - z))
template <bool ZP>
__global__ void w4_dequant_frag_kernel(const u32x4_t* __restrict__ q_src, const bf16_t* __restrict__ s_src,
                                       const uint8_t* __restrict__ z_src, u32x4_t* __restrict__ dst, int N, int K, long total) {
  const int KG = K >> 7, KT = K >> 5;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
    const long unit = c >> 6;
    const int lane = (int)(c & 63);
    const int g = (int)(unit / KG), cg = (int)(unit % KG);
    const float s = bf2f(s_src[unit * 16 + (lane & 15)]);
    int z = 8;
    if constexpr (ZP) z = z_src[unit * 16 + (lane & 15)];
    const u32x4_t v = q_src[c];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      u32x4_t o;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const float lo = (float)((int)((v[j] >> (4 * p)) & 0xfu) - z), hi = (float)((int)((v[j] >> (4 * p + 16)) & 0xfu) - z);
        o[p] = pack_bf2(s * lo, s * hi);
      }
      dst[((size_t)g * KT + 4 * cg + j) * 64 + lane] = o;
    }
  }
}

static int grid_for(long total) {
  long blocks = (total + 255) / 256;
  return (int)(blocks > 65536 ? 65536 : blocks);
}

static bool w4_shape_ok(int N, int K) { return N > 0 && K > 0 && (N & 15) == 0 && (K & 127) == 0; }

extern "C" int ssd_w4_rows_to_frag(const void* q_rows, const void* s_rows, void* q_frag, void* s_frag, const int32_t* row_map, int N,
                                   int K, void* stream) {
  if (!w4_shape_ok(N, K)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !q_frag || !s_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(w4_rows_to_frag_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)q_rows,
                     (const bf16_t*)s_rows, (const uint8_t*)nullptr, (u32x4_t*)q_frag, (bf16_t*)s_frag, (uint8_t*)nullptr, row_map, N, K,
                     total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_w4_frag_to_rows(const void* q_frag, const void* s_frag, void* q_rows, void* s_rows, int N, int K, void* stream) {
  if (!w4_shape_ok(N, K)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !q_frag || !s_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(w4_frag_to_rows_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const bf16_t*)s_frag, (const uint8_t*)nullptr, (uint32_t*)q_rows, (bf16_t*)s_rows, (uint8_t*)nullptr, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_w4_dequant_frag(const void* q_frag, const void* s_frag, void* w_frag, int N, int K, void* stream) {
  if (!w4_shape_ok(N, K)) return SSD_ERR_SHAPE;
  if (!q_frag || !s_frag || !w_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(w4_dequant_frag_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const bf16_t*)s_frag, (const uint8_t*)nullptr, (u32x4_t*)w_frag, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_w4zp_rows_to_frag(const void* q_rows, const void* s_rows, const void* z_rows, void* q_frag, void* s_frag,
                                     void* z_frag, const int32_t* row_map, int N, int K, void* stream) {
  if (!w4_shape_ok(N, K)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !z_rows || !q_frag || !s_frag || !z_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(w4_rows_to_frag_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)q_rows,
                     (const bf16_t*)s_rows, (const uint8_t*)z_rows, (u32x4_t*)q_frag, (bf16_t*)s_frag, (uint8_t*)z_frag, row_map, N, K,
                     total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_w4zp_frag_to_rows(const void* q_frag, const void* s_frag, const void* z_frag, void* q_rows, void* s_rows,
                                     void* z_rows, int N, int K, void* stream) {
  if (!w4_shape_ok(N, K)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !z_rows || !q_frag || !s_frag || !z_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(w4_frag_to_rows_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const bf16_t*)s_frag, (const uint8_t*)z_frag, (uint32_t*)q_rows, (bf16_t*)s_rows, (uint8_t*)z_rows, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_w4zp_dequant_frag(const void* q_frag, const void* s_frag, const void* z_frag, void* w_frag, int N, int K,
                                     void* stream) {
  if (!w4_shape_ok(N, K)) return SSD_ERR_SHAPE;
  if (!q_frag || !s_frag || !z_frag || !w_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(w4_dequant_frag_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const bf16_t*)s_frag, (const uint8_t*)z_frag, (u32x4_t*)w_frag, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------
// The GEMM.  U = column groups per stage and wave (the code bytes in flight per wave are U * NT KiB); K is dealt to the waves in
// runs of U column groups round-robin, the < U left-over groups go to the last wave (gemm_fp8_kernel's walk).  XS: the x operands
// ride in the double-buffered stage (MT <= 4); at MT = 8 they would not fit the VGPR budget and are loaded per group instead.
// ---------------------------------------------------------------------------------------------------------------------
// the zero points of a lane's four output rows per row group, one byte each (ZP only: the symmetric stage has no such member)
template <int NT, bool ZP>
struct W4Zero {
  uint32_t z[NT];
};
template <int NT>
struct W4Zero<NT, false> {};

template <int MT, int NT, bool XS, bool ZS>
struct W4Stage : W4Zero<NT, ZS> {
  u32x4_t a[NT];                  // 32 codes per lane: k-tiles 4c .. 4c+3
  u32x2_t s[NT];                  // the 4 bf16 group scales of the lane's output rows
  u32x4_t b[XS ? MT : 1][4];      // x operands of the four k-tiles
};

template <int MT, int NT, int EPI, int U, bool XS, bool ZP>
__global__ void __launch_bounds__(512)
gemm_w4a16_kernel(const u32x4_t* __restrict__ Qf, const u32x2_t* __restrict__ Sf, const uint32_t* __restrict__ Zf,
                  const u32x4_t* __restrict__ Xf, const bf16_t* __restrict__ bias, void* __restrict__ Yv, int M, int N, int K, int ldy,
                  int tpw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool ZS = ZP && MT < 8;         // the zero points ride in the stage; at MT = 8 they are loaded per group, as x is
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = blockDim.x >> 6;
  const int KG = K >> 7, KT = K >> 5;
  const int ntiles = (N / 16) / NT;
  const int t_begin = blockIdx.x * tpw, t_end = min(ntiles, t_begin + tpw);
  const u32x4_t* xp = Xf + lane;
  const size_t wstride = (size_t)KG << 6;   // 16-byte chunks between adjacent row groups of q
  const size_t sstride = (size_t)KG << 2;   // 8-byte scale quads between adjacent row groups of s
  const size_t xstride = (size_t)KT << 6;   // 16-byte chunks between adjacent token tiles of x
  const int kstep = nw * U;
  const int kg0 = wave * U;
  const int kmain = (KG / U) * U;
  const u32x4_t* wp = Qf + ((size_t)t_begin * NT * wstride) + lane;
  const u32x2_t* sp = Sf + ((size_t)t_begin * NT * sstride) + (lane >> 4);
  const uint32_t* zp = nullptr;             // 4-byte zero-point quads: same stride and lane offset as the scale quads
  if constexpr (ZP) zp = Zf + ((size_t)t_begin * NT * sstride) + (lane >> 4);
  const int mt_last = (M - 1) >> 4;
  const u32x4_t NEG136 = {0xC308C308u, 0xC308C308u, 0xC308C308u, 0xC308C308u};   // bf16 -136 in every element
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
  auto load = [&](W4Stage<MT, NT, XS, ZS>(&s)[U], int kg) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        s[u].a[nt] = __builtin_nontemporal_load(wp + nt * wstride + ((size_t)(kg + u) << 6));
        s[u].s[nt] = __builtin_nontemporal_load(sp + nt * sstride + ((size_t)(kg + u) << 2));
        if constexpr (ZS) s[u].z[nt] = __builtin_nontemporal_load(zp + nt * sstride + ((size_t)(kg + u) << 2));
      }
      if constexpr (XS) xgroup(s[u].b, kg + u);
    }
  };
  W4Stage<MT, NT, XS, ZS> cur[U], nxt[U];
  if (t_begin < t_end && kg0 < kmain) load(cur, kg0);

  for (int tile = t_begin; tile < t_end; ++tile) {
    const int tile0 = tile * NT;
    f32x4_t acc[NT][MT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // one column group: partial = -136 * sum(x) + sum((q + 136) * x) per (row, token), then acc += s * partial.  With XS the x
    // operands come from the stage; without, each token tile's four are loaded here (from L2: x is shared by every workgroup).
    // ZP: zq holds the zero-point bytes; t = ((z - 8) / 136) * corr + partial = sum((u - z) * x) before the scale.
    auto group = [&](const u32x4_t (&a)[NT], const u32x2_t (&sc)[NT], const W4Zero<NT, ZS>& zs, const u32x4_t (&bs)[XS ? MT : 1][4],
                     int kg) {
      u32x4_t w[NT][4];
      float s[NT][4];
      float zf[ZP ? NT : 1][4];
      W4Zero<NT, ZP> zq;
      if constexpr (ZS) zq = zs;
      else if constexpr (ZP) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) zq.z[nt] = __builtin_nontemporal_load(zp + nt * sstride + ((size_t)kg << 2));
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[nt][j] = w4_to_bf16_off(a[nt][j]);
        s[nt][0] = bf2f(sc[nt][0] & 0xffffu); s[nt][1] = bf2f(sc[nt][0] >> 16);
        s[nt][2] = bf2f(sc[nt][1] & 0xffffu); s[nt][3] = bf2f(sc[nt][1] >> 16);
        if constexpr (ZP) {
#pragma unroll
          for (int r = 0; r < 4; ++r) zf[nt][r] = __builtin_fmaf((float)((zq.z[nt] >> (8 * r)) & 0xffu), 1.0f / 136.0f, -8.0f / 136.0f);
        }
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        u32x4_t b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = XS ? bs[XS ? mt : 0][j] : xload(mt, 4 * kg + j);
        f32x4_t corr = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) corr = mfma16(NEG136, b[j], corr);
        // MT = 8 with zero points: without this fence the scheduler hoists the x loads of later token tiles over the MFMA chains and
        // the 8 extra zero-point registers tip NT = 2 into scratch (16 / 36 bytes per lane); with it 199 / 203 VGPRs, none.
        if constexpr (ZP && MT == 8) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          f32x4_t p = corr;
#pragma unroll
          for (int j = 0; j < 4; ++j) p = mfma16(w[nt][j], b[j], p);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float t = p[r];
            if constexpr (ZP) t = __builtin_fmaf(zf[nt][r], corr[r], t);
            acc[nt][mt][r] = __builtin_fmaf(s[nt][r], t, acc[nt][mt][r]);
          }
        }
      }
    };
    auto compute = [&](W4Stage<MT, NT, XS, ZS>(&s)[U], int kg) {
#pragma unroll
      for (int u = 0; u < U; ++u) group(s[u].a, s[u].s, s[u], s[u].b, kg + u);
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
      u32x2_t sc[NT];
      W4Zero<NT, ZS> zq;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        a[nt] = __builtin_nontemporal_load(wp + nt * wstride + ((size_t)kg << 6));
        sc[nt] = __builtin_nontemporal_load(sp + nt * sstride + ((size_t)kg << 2));
        if constexpr (ZS) zq.z[nt] = __builtin_nontemporal_load(zp + nt * sstride + ((size_t)kg << 2));
      }
      if constexpr (XS) xgroup(b, kg);
      group(a, sc, zq, b, kg);
    }

    // next tile: advance the weight pointers and put its first loads in flight before the combine
    wp += (size_t)NT * wstride;
    sp += (size_t)NT * sstride;
    if constexpr (ZP) zp += (size_t)NT * sstride;
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
    if (EPI == W4_SILU_FRAG) {
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

template <int MT, int NT, int EPI, int U, bool XS, bool ZP>
static int w4_launch(const void* x, const void* q, const void* s, const void* z, const void* bias, void* y, int M, int N, int K, int ldy,
                     int waves, int tpw, hipStream_t st) {
  const int ntiles = (N / 16) / NT;
  if (tpw < 1) tpw = 1;
  const int blocks = (ntiles + tpw - 1) / tpw;
  const size_t lds = (size_t)waves * NT * MT * 64 * sizeof(f32x4_t);
  if (lds > 64 * 1024) return SSD_ERR_ARG;
  hipLaunchKernelGGL((gemm_w4a16_kernel<MT, NT, EPI, U, XS, ZP>), dim3(blocks), dim3(waves * 64), lds, st, (const u32x4_t*)q,
                     (const u32x2_t*)s, (const uint32_t*)z, (const u32x4_t*)x, (const bf16_t*)bias, y, M, N, K, ldy, tpw);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// U per (MT, NT, deep): 2-4 KiB of codes in flight per wave in the plain form (x staged with them), twice that in the deep one (x
// loaded per group), within the VGPR budget of a <= 8-wave workgroup without spills (the double-buffered stage is 2 U (6 NT + 16 MT)
// VGPRs with x in it, 12 U NT without; the zero points add 2 U NT)
template <int MT, int EPI, bool ZP>
static int w4_dispatch_nt(const void* x, const void* q, const void* s, const void* z, const void* bias, void* y, int M, int N, int K,
                          int ldy, int nt, bool deep, int waves, int tpw, hipStream_t st) {
#define W4L(NTV, UV, XSV) return w4_launch<MT, NTV, EPI, UV, XSV, ZP>(x, q, s, z, bias, y, M, N, K, ldy, waves, tpw, st)
  if constexpr (MT == 1) {
    if (nt == 1) { if constexpr (EPI == W4_SILU_FRAG) return SSD_ERR_ARG; else { if (deep) W4L(1, 8, false); W4L(1, 2, true); } }
    if (nt == 2) { if (deep) W4L(2, 4, false); W4L(2, 1, true); }
    if (nt == 4) { if (deep) W4L(4, 2, false); W4L(4, 1, true); }
  } else if constexpr (MT == 2) {
    if (deep) return SSD_ERR_ARG;
    if (nt == 1) { if constexpr (EPI == W4_SILU_FRAG) return SSD_ERR_ARG; else W4L(1, 2, true); }
    if (nt == 2) W4L(2, 1, true);
  } else if constexpr (MT == 4) {
    if (deep) return SSD_ERR_ARG;
    if (nt == 1) { if constexpr (EPI == W4_SILU_FRAG) return SSD_ERR_ARG; else W4L(1, 1, true); }
    if (nt == 2) W4L(2, 1, !ZP);      // with zero points the staged x no longer fits beside them: x per group, as at MT = 8
  } else {
    if (deep) return SSD_ERR_ARG;
    if (nt == 1) { if constexpr (EPI == W4_SILU_FRAG) return SSD_ERR_ARG; else W4L(1, 1, false); }
    if (nt == 2) W4L(2, 1, false);
  }
#undef W4L
  return SSD_ERR_ARG;
}

template <bool ZP>
static int w4_gemm_cfg(const void* x_frag, const void* q_frag, const void* s_frag, const void* z_frag, const void* bias, void* y, int M,
                       int N, int K, int ldy, int epilogue, int nt, int waves, void* stream) {
  if (M <= 0 || M > 128 || !w4_shape_ok(N, K)) return SSD_ERR_SHAPE;
  if (!x_frag || !q_frag || !s_frag || !y || (ZP && !z_frag)) return SSD_ERR_ARG;
  if (epilogue == W4_ROWS && ldy < N) return SSD_ERR_SHAPE;
  const int tpw = (waves >> 8) & 0xff;
  const bool deep = (nt >> 8) & 1;
  waves &= 0xff;
  nt &= 0xff;
  if (waves < 1 || waves > 8 || (nt != 1 && nt != 2 && nt != 4) || ((N / 16) % nt) != 0) return SSD_ERR_ARG;
  if (epilogue == W4_SILU_FRAG && ((nt & 1) || (N & 63))) return SSD_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int mt = (M + 15) / 16;
#define W4_MT(MTV)                                                                                                                    \
  switch (epilogue) {                                                                                                                 \
    case W4_ROWS:                                                                                                                     \
      return w4_dispatch_nt<MTV, W4_ROWS, ZP>(x_frag, q_frag, s_frag, z_frag, bias, y, M, N, K, ldy, nt, deep, waves, tpw, st);        \
    case W4_SILU_FRAG:                                                                                                                \
      return w4_dispatch_nt<MTV, W4_SILU_FRAG, ZP>(x_frag, q_frag, s_frag, z_frag, bias, y, M, N, K, ldy, nt, deep, waves, tpw, st);   \
    default: return SSD_ERR_ARG;                                                                                                      \
  }
  if (mt == 1) { W4_MT(1) }
  if (mt == 2) { W4_MT(2) }
  if (mt <= 4) { W4_MT(4) }
  { W4_MT(8) }
#undef W4_MT
}

extern "C" int ssd_gemm_w4a16_cfg(const void* x_frag, const void* q_frag, const void* s_frag, const void* bias, void* y, int M, int N,
                                  int K, int ldy, int epilogue, int nt, int waves, void* stream) {
  return w4_gemm_cfg<false>(x_frag, q_frag, s_frag, nullptr, bias, y, M, N, K, ldy, epilogue, nt, waves, stream);
}

extern "C" int ssd_gemm_w4a16_zp_cfg(const void* x_frag, const void* q_frag, const void* s_frag, const void* z_frag, const void* bias,
                                     void* y, int M, int N, int K, int ldy, int epilogue, int nt, int waves, void* stream) {
  return w4_gemm_cfg<true>(x_frag, q_frag, s_frag, z_frag, bias, y, M, N, K, ldy, epilogue, nt, waves, stream);
}

// Default decomposition.  One token tile: from the M = 8 sweep of every explicit decomposition at the 1B / 8B / 70B / Qwen3-32B shapes
// (profiles/w4a16_sweep.jsonl; the 1B and the small 8B matrices sit at the ~7.6 us launch floor in any form).  The plain form won
// every matrix above that floor:
//   gate_up: 4 row groups per workgroup, 2 waves once there are >= 768 such tiles (70B 49.5 us, Qwen3-32B 30.3), else 4 (8B 15.2);
//   qkv-class (>= 640 row groups, K <= 8192): 4 row groups x 8 waves (70B 14.6 us, Qwen3-32B 10.3);
//   o / down-class (>= 320 row groups, K >= 8192): 2 row groups x 8 waves (70B o 10.7 us, down 30.8; Qwen3-32B 10.2, 26.2);
//   anything smaller: 1 row group x 8 waves.
// More token tiles: one or two row groups per workgroup, waves sized so that every wave has a few column groups, LDS for the
// combine <= 64 KiB.
// The zero-point GEMM starts from the same classes (the walk and the bytes per unit differ by 16 in 1056).
template <bool ZP>
static int w4_gemm_default(const void* x_frag, const void* q_frag, const void* s_frag, const void* z_frag, const void* bias, void* y,
                           int M, int N, int K, int ldy, int epilogue, void* stream) {
  if (M <= 0 || M > 128 || !w4_shape_ok(N, K)) return SSD_ERR_SHAPE;
  const int groups = N / 16, KG = K / 128, mt = (M + 15) / 16;
  const bool silu = epilogue == W4_SILU_FRAG;
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
    return w4_gemm_cfg<ZP>(x_frag, q_frag, s_frag, z_frag, bias, y, M, N, K, ldy, epilogue, nt, waves, stream);
  }
  nt = (silu || (groups >= 2048 && groups % 2 == 0)) ? 2 : 1;
  waves = 8;
  while (waves > 1 && KG / waves < 2) waves >>= 1;
  const int mtr = mt == 2 ? 2 : (mt <= 4 ? 4 : 8);
  while (waves > 1 && (size_t)waves * nt * mtr * 1024 > 64 * 1024) waves >>= 1;
  return w4_gemm_cfg<ZP>(x_frag, q_frag, s_frag, z_frag, bias, y, M, N, K, ldy, epilogue, nt, waves, stream);
}

extern "C" int ssd_gemm_w4a16(const void* x_frag, const void* q_frag, const void* s_frag, const void* bias, void* y, int M, int N, int K,
                              int ldy, int epilogue, void* stream) {
  return w4_gemm_default<false>(x_frag, q_frag, s_frag, nullptr, bias, y, M, N, K, ldy, epilogue, stream);
}

extern "C" int ssd_gemm_w4a16_zp(const void* x_frag, const void* q_frag, const void* s_frag, const void* z_frag, const void* bias, void* y,
                                 int M, int N, int K, int ldy, int epilogue, void* stream) {
  return w4_gemm_default<true>(x_frag, q_frag, s_frag, z_frag, bias, y, M, N, K, ldy, epilogue, stream);
}
