// W4A16 weight-only GEMMs for the quantized target: y = x . (s (.) q)^T with bf16 activations, signed int4 weight codes and one bf16
// scale per output row and 128-column group (include/ssd_hip_w4a16.h).  The walk is wq_gemm_kernel's (gemm_wq.h); w4's own:
//  * q is stored "w4 frag": one 1 KiB unit per (16-row group, 128-column group), lane l holding its 8-column slices of the group's
//    four k-tiles -- one 16-byte lane load, one contiguous 1 KiB wave load, four MFMA k-steps.
//  * codes go straight to VGPRs with non-temporal loads and are widened exactly, a mask and an or per two weights (plus a shift per
//    nibble position): (word >> 4p) & 0x000F000F | 0x43004300 is the bf16 pair 128 + u = q + 136 (bf16 has one ulp = 1 in [128, 256)).
//  * each column group accumulates into a fresh fp32 partial that starts at -136 * sum(x over the group) (four MFMAs against a
//    constant -136 operand, shared by the workgroup's row groups), so the partial is sum(q * x); the row accumulator takes
//    s * partial in fp32.
// With zero points (include/ssd_hip_w4zp.h, template parameter ZP) the weight is s * (u - z), z per (row, group): the same walk and
// the same partial p = sum((u - 8) * x).  The constant-operand chain already holds corr = -136 * sum(x) for every row, so per
// accumulator register t = fma((z - 8) / 136, corr, p) = sum((u - z) * x), then acc = fma(s, t, acc): no further MFMA and no
// further live accumulator (a second chain against a constant -1 operand spilled at MT >= 4).  (z - 8) / 136 is rounded to fp32
// (relative 2^-24 on a term no larger than 8 |sum(x)|, below the rounding of p itself, which passes through 136 |sum(x)|); z = 8
// gives t = p, the symmetric kernel's value.  Every difference is under `if constexpr (ZP)`; the ZP = false instantiations are
// the symmetric kernels, unchanged.
#include "common.h"
#include "gemm_wq.h"

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

extern "C" int ssd_w4_rows_to_frag(const void* q_rows, const void* s_rows, void* q_frag, void* s_frag, const int32_t* row_map, int N,
                                   int K, void* stream) {
  if (!wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !q_frag || !s_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(w4_rows_to_frag_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)q_rows,
                     (const bf16_t*)s_rows, (const uint8_t*)nullptr, (u32x4_t*)q_frag, (bf16_t*)s_frag, (uint8_t*)nullptr, row_map, N, K,
                     total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_w4_frag_to_rows(const void* q_frag, const void* s_frag, void* q_rows, void* s_rows, int N, int K, void* stream) {
  if (!wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !q_frag || !s_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(w4_frag_to_rows_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const bf16_t*)s_frag, (const uint8_t*)nullptr, (uint32_t*)q_rows, (bf16_t*)s_rows, (uint8_t*)nullptr, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_w4_dequant_frag(const void* q_frag, const void* s_frag, void* w_frag, int N, int K, void* stream) {
  if (!wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  if (!q_frag || !s_frag || !w_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(w4_dequant_frag_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const bf16_t*)s_frag, (const uint8_t*)nullptr, (u32x4_t*)w_frag, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_w4zp_rows_to_frag(const void* q_rows, const void* s_rows, const void* z_rows, void* q_frag, void* s_frag,
                                     void* z_frag, const int32_t* row_map, int N, int K, void* stream) {
  if (!wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !z_rows || !q_frag || !s_frag || !z_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(w4_rows_to_frag_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)q_rows,
                     (const bf16_t*)s_rows, (const uint8_t*)z_rows, (u32x4_t*)q_frag, (bf16_t*)s_frag, (uint8_t*)z_frag, row_map, N, K,
                     total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_w4zp_frag_to_rows(const void* q_frag, const void* s_frag, const void* z_frag, void* q_rows, void* s_rows,
                                     void* z_rows, int N, int K, void* stream) {
  if (!wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !z_rows || !q_frag || !s_frag || !z_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(w4_frag_to_rows_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const bf16_t*)s_frag, (const uint8_t*)z_frag, (uint32_t*)q_rows, (bf16_t*)s_rows, (uint8_t*)z_rows, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_w4zp_dequant_frag(const void* q_frag, const void* s_frag, const void* z_frag, void* w_frag, int N, int K,
                                     void* stream) {
  if (!wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  if (!q_frag || !s_frag || !z_frag || !w_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(w4_dequant_frag_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const bf16_t*)s_frag, (const uint8_t*)z_frag, (u32x4_t*)w_frag, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------
// The GEMM: wq_gemm_kernel with a K unit of one column group (128 columns, four k-tiles) and the group's scale quads (and, with
// ZP, zero-point quads) as the stage's side-band.  XS: the x operands ride in the double-buffered stage (MT <= 4); at MT = 8 they
// would not fit the VGPR budget and are loaded per group instead.
// ---------------------------------------------------------------------------------------------------------------------
// the zero points of a lane's four output rows per row group, one byte each (ZP only: the symmetric stage has no such member)
template <int NT, bool ZP>
struct W4Zero {
  uint32_t z[NT];
};
template <int NT>
struct W4Zero<NT, false> {};

template <bool ZP>
struct W4 {
  static constexpr int KSHIFT = 7, KT = 4;
  static constexpr bool ROW_SCALE = false, HAS_Z = ZP;
  template <int MT, int NT>
  struct Side : W4Zero<NT, ZP && MT < 8> {
    static constexpr bool ZS = ZP && MT < 8;   // the zero points ride in the stage; at MT = 8 they are loaded per group, as x is
    u32x2_t s[NT];                             // the 4 bf16 group scales of the lane's output rows
  };
  struct Band {
    const size_t sstride;   // 8-byte scale quads between adjacent row groups of s
    const u32x2_t* sp;
    const uint32_t* zp;     // 4-byte zero-point quads: same stride and lane offset as the scale quads
    __device__ Band(const void* Sf, const void* Zf, size_t g0, int KG, int lane)
        : sstride((size_t)KG << 2), sp((const u32x2_t*)Sf + g0 * sstride + (lane >> 4)),
          zp(ZP ? (const uint32_t*)Zf + g0 * sstride + (lane >> 4) : nullptr) {}
    template <class S>
    __device__ void load(S& s, int nt, int kg) const {
      s.s[nt] = __builtin_nontemporal_load(sp + nt * sstride + ((size_t)kg << 2));
      if constexpr (S::ZS) s.z[nt] = __builtin_nontemporal_load(zp + nt * sstride + ((size_t)kg << 2));
    }
    __device__ void advance(int nt) {
      sp += (size_t)nt * sstride;
      if constexpr (ZP) zp += (size_t)nt * sstride;
    }
  };

  // one column group: partial = -136 * sum(x) + sum((q + 136) * x) per (row, token), then acc += s * partial.  With XS the x
  // operands come from the stage; without, each token tile's four are loaded here (from L2: x is shared by every workgroup).
  // ZP: zq holds the zero-point bytes; t = ((z - 8) / 136) * corr + partial = sum((u - z) * x) before the scale.
  template <int MT, int NT, bool XS, class S, class XL>
  static __device__ __forceinline__ void group(f32x4_t (&acc)[NT][MT], const S& st, int kg, const XL& xload, const Band& band) {
    const u32x4_t NEG136 = {0xC308C308u, 0xC308C308u, 0xC308C308u, 0xC308C308u};   // bf16 -136 in every element
    u32x4_t w[NT][4];
    float s[NT][4];
    float zf[ZP ? NT : 1][4];
    W4Zero<NT, ZP> zq;
    if constexpr (S::ZS) zq = st;
    else if constexpr (ZP) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) zq.z[nt] = __builtin_nontemporal_load(band.zp + nt * band.sstride + ((size_t)kg << 2));
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) w[nt][j] = w4_to_bf16_off(st.a[nt][j]);
      s[nt][0] = bf2f(st.s[nt][0] & 0xffffu); s[nt][1] = bf2f(st.s[nt][0] >> 16);
      s[nt][2] = bf2f(st.s[nt][1] & 0xffffu); s[nt][3] = bf2f(st.s[nt][1] >> 16);
      if constexpr (ZP) {
#pragma unroll
        for (int r = 0; r < 4; ++r) zf[nt][r] = __builtin_fmaf((float)((zq.z[nt] >> (8 * r)) & 0xffu), 1.0f / 136.0f, -8.0f / 136.0f);
      }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      u32x4_t b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = XS ? st.b[XS ? mt : 0][j] : xload(mt, 4 * kg + j);
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
  }

  // U per (MT, NT, deep): 2-4 KiB of codes in flight per wave in the plain form (x staged with them), twice that in the deep one (x
  // loaded per group), within the VGPR budget of a <= 8-wave workgroup without spills (the double-buffered stage is 2 U (6 NT + 16 MT)
  // VGPRs with x in it, 12 U NT without; the zero points add 2 U NT)
  static constexpr WqForm FORMS[4][3][2] = {
      /* MT 1 */ {{{2, true}, {8, false}}, {{1, true}, {4, false}}, {{1, true}, {2, false}}},
      /* MT 2 */ {{{2, true}, {}}, {{1, true}, {}}, {}},
      // MT 4, nt 2: with zero points the staged x no longer fits beside them: x per group, as at MT = 8
      /* MT 4 */ {{{1, true}, {}}, {{1, !ZP}, {}}, {}},
      /* MT 8 */ {{{1, false}, {}}, {{1, false}, {}}, {}},
  };
};

template <bool ZP>
static int w4_gemm_cfg(const void* x_frag, const void* q_frag, const void* s_frag, const void* z_frag, const void* bias, void* y, int M,
                       int N, int K, int ldy, int epilogue, int nt, int waves, void* stream) {
  return wq_gemm_cfg<W4<ZP>>(WqArgs{x_frag, q_frag, s_frag, z_frag, bias, y, M, N, K, ldy}, epilogue, nt, waves, stream);
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
  if (M <= 0 || M > 128 || !wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  const int groups = N / 16, KG = K / 128, mt = (M + 15) / 16;
  const bool silu = epilogue == WQ_SILU_FRAG;
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
