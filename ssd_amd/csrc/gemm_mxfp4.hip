// MXFP4 weight-only GEMMs for the quantized target: y = x . W^T with bf16 activations and W = 2^(b - 127) * e2m1(q), e2m1 weight codes
// with one e8m0 scale byte per output row and 32-column block (include/ssd_hip_mxfp4.h).  The walk is wq_gemm_kernel's
// (gemm_wq.h); mxfp4's own:
//  * q is stored "mx4 frag": one 1 KiB unit per (16-row group, 128-column group), lane l holding its 8-column slices of the group's
//    four k-tiles -- one 16-byte lane load, one contiguous 1 KiB wave load, four MFMA k-steps; the four scale bytes of the lane's row
//    for those k-tiles are one 4-byte load.
//  * codes go straight to VGPRs with non-temporal loads.  What differs is the inner step: v_cvt_scalef32_pk_bf16_fp4 turns one byte
//    (two codes) into two bf16 already multiplied by the block scale, four conversions per 8 weights.  An MX block is one k-tile of
//    v_mfma_f32_16x16x32_bf16, so a lane's operand slice has ONE scale; 2^e * {0, .5, 1, 1.5, 2, 3, 4, 6} is exact in bf16, so the
//    operand is the exact weight and the MFMA goes straight into the row accumulator: no offset, no per-group partial, no scale fma.
#include "common.h"
#include "gemm_wq.h"

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

extern "C" int ssd_mx4_rows_to_frag(const void* q_rows, const void* s_rows, void* q_frag, void* s_frag, const int32_t* row_map, int N,
                                    int K, void* stream) {
  if (!wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !q_frag || !s_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(mx4_rows_to_frag_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)q_rows,
                     (const uint32_t*)s_rows, (u32x4_t*)q_frag, (uint32_t*)s_frag, row_map, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_mx4_frag_to_rows(const void* q_frag, const void* s_frag, void* q_rows, void* s_rows, int N, int K, void* stream) {
  if (!wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !q_frag || !s_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(mx4_frag_to_rows_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const uint32_t*)s_frag, (uint32_t*)q_rows, (uint32_t*)s_rows, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_mx4_dequant_frag(const void* q_frag, const void* s_frag, void* w_frag, int N, int K, void* stream) {
  if (!wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  if (!q_frag || !s_frag || !w_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(mx4_dequant_frag_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const uint32_t*)s_frag, (u32x4_t*)w_frag, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------
// The GEMM: wq_gemm_kernel with a K unit of one column group (128 columns, four k-tiles) and the lane's scale quad as the stage's
// side-band.  XS: the x operands ride in the double-buffered stage (MT <= 4); at MT = 8 they would not fit the VGPR budget and are
// loaded per group instead.
// ---------------------------------------------------------------------------------------------------------------------
struct Mx4 {
  static constexpr int KSHIFT = 7, KT = 4;
  static constexpr bool ROW_SCALE = false, HAS_Z = false;
  template <int MT, int NT>
  struct Side {
    uint32_t s[NT];   // the 4 scale bytes of the lane's weight row for the unit's k-tiles
  };
  struct Band {
    const size_t sstride;   // 4-byte scale quads between adjacent row groups of s
    const uint32_t* sp;
    __device__ Band(const void* Sf, const void*, size_t g0, int KG, int lane)
        : sstride((size_t)KG << 4), sp((const uint32_t*)Sf + g0 * sstride + (lane & 15)) {}
    template <class S>
    __device__ void load(S& s, int nt, int kg) const {
      s.s[nt] = __builtin_nontemporal_load(sp + nt * sstride + ((size_t)kg << 4));
    }
    __device__ void advance(int nt) { sp += (size_t)nt * sstride; }
  };

  // one column group: convert each row group's four k-tile slices with their block scales, then MFMA straight into the row
  // accumulators.  With XS the x operands come from the stage; without, each token tile's four are loaded here (from L2: x is
  // shared by every workgroup).
  template <int MT, int NT, bool XS, class S, class XL>
  static __device__ __forceinline__ void group(f32x4_t (&acc)[NT][MT], const S& st, int kg, const XL& xload, const Band&) {
    u32x4_t w[NT][4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j) w[nt][j] = mx4_to_bf16(st.a[nt][j], mx4_scale(st.s[nt], j));
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      u32x4_t b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = XS ? st.b[XS ? mt : 0][j] : xload(mt, 4 * kg + j);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[nt][mt] = mfma16(w[nt][j], b[j], acc[nt][mt]);
    }
  }

  // U per (MT, NT, deep): as gemm_w4a16.hip -- 2-4 KiB of codes in flight per wave in the plain form (x staged with them), twice that
  // in the deep one (x loaded per group), within the VGPR budget of a <= 8-wave workgroup without spills (the double-buffered stage is
  // 2 U (5 NT + 16 MT) VGPRs with x in it, 10 U NT without)
  static constexpr WqForm FORMS[4][3][2] = {
      /* MT 1 */ {{{2, true}, {8, false}}, {{1, true}, {4, false}}, {{1, true}, {2, false}}},
      /* MT 2 */ {{{2, true}, {}}, {{1, true}, {}}, {}},
      /* MT 4 */ {{{1, true}, {}}, {{1, true}, {}}, {}},
      /* MT 8 */ {{{1, false}, {}}, {{1, false}, {}}, {}},
  };
};

extern "C" int ssd_gemm_mxfp4_cfg(const void* x_frag, const void* q_frag, const void* s_frag, const void* bias, void* y, int M, int N,
                                  int K, int ldy, int epilogue, int nt, int waves, void* stream) {
  return wq_gemm_cfg<Mx4>(WqArgs{x_frag, q_frag, s_frag, nullptr, bias, y, M, N, K, ldy}, epilogue, nt, waves, stream);
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
    return ssd_gemm_mxfp4_cfg(x_frag, q_frag, s_frag, bias, y, M, N, K, ldy, epilogue, nt, waves, stream);
  }
  nt = (silu || (groups >= 2048 && groups % 2 == 0)) ? 2 : 1;
  waves = 8;
  while (waves > 1 && KG / waves < 2) waves >>= 1;
  const int mtr = mt == 2 ? 2 : (mt <= 4 ? 4 : 8);
  while (waves > 1 && (size_t)waves * nt * mtr * 1024 > 64 * 1024) waves >>= 1;
  return ssd_gemm_mxfp4_cfg(x_frag, q_frag, s_frag, bias, y, M, N, K, ldy, epilogue, nt, waves, stream);
}
