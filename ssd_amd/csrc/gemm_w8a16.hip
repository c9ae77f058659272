// W8A16 weight-only GEMMs for the quantized target: y = x . (s (.) q)^T with bf16 activations, signed int8 weight codes and one bf16
// scale per output row and 128-column group (include/ssd_hip_w8a16.h).  The walk is wq_gemm_kernel's (gemm_wq.h); w8's own:
//  * q is stored "w8 frag": the byte order of the fp8 frag layout (one 1 KiB unit per 16-row group and 64-column k-pair, lane l
//    holding its 8-byte slices of k-tiles 2p and 2p+1 side by side), the byte itself the two's-complement code.
//  * codes go straight to VGPRs with non-temporal loads and are widened exactly: v_cvt_f32_i32 with a sign-extending SDWA byte
//    select per weight, then one v_perm_b32 takes the top halves of two floats as a bf16 pair (|q| <= 128 has <= 8 significant
//    bits, so nothing is cut off).  1.5 VALU instructions per weight where fp8's v_cvt_scalef32_pk_bf16_fp8 spends 0.5; the
//    alternatives from the unsigned byte cost more: v_cvt_f32_ubyteN + subtract + pack is 2 (with v_pk_add_f32) or 2.5, the
//    0x4B000000 | u splice (one v_perm_b32 per weight) + subtract + pack is 2.5, and leaving the 128 in and removing it with a
//    constant-operand MFMA chain, as w4 does, doubles the MFMAs of a 64-column unit at one row group.
//  * the K unit of the walk is the 64-column code unit; the scale group is two of them.  Each unit accumulates into a fresh fp32
//    partial (two MFMAs) and the row accumulator takes s * partial in fp32, the group's scale quad riding in the stage beside the
//    codes (8 bytes per lane and unit, from a 32-byte table entry per group: L2 traffic, not HBM).
#include "common.h"
#include "gemm_wq.h"
#include "ssd_hip_w8a16.h"

// the top halves of two fp32 as a bf16 pair (exact for the integers here)
__device__ __forceinline__ uint32_t w8_top_halves(float lo, float hi) {
  return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
}

// 8 two's-complement bytes (one lane's slice of a k-tile: w0 = columns 0..3, w1 = columns 4..7) -> the 8 bf16 of one MFMA operand
__device__ __forceinline__ u32x4_t w8x8_to_bf16(uint32_t w0, uint32_t w1) {
  u32x4_t r;
  r[0] = w8_top_halves((float)(int8_t)w0, (float)(int8_t)(w0 >> 8));
  r[1] = w8_top_halves((float)(int8_t)(w0 >> 16), (float)(int8_t)(w0 >> 24));
  r[2] = w8_top_halves((float)(int8_t)w1, (float)(int8_t)(w1 >> 8));
  r[3] = w8_top_halves((float)(int8_t)(w1 >> 16), (float)(int8_t)(w1 >> 24));
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// Layout: row form -> w8 frag (with an optional destination -> source row map), and back; dequantize into a bf16 frag.
// One thread per 16-byte lane chunk of a code unit; lanes 0..15 of a group's first unit also move the group's 16 scales.
// ---------------------------------------------------------------------------------------------------------------------
constexpr uint32_t W8_FLIP = 0x80808080u;   // u = q + 128 <-> two's-complement q, four bytes at a time

__global__ void w8_rows_to_frag_kernel(const uint8_t* __restrict__ q_src, const bf16_t* __restrict__ s_src, u32x4_t* __restrict__ q_dst,
                                       bf16_t* __restrict__ s_dst, const int32_t* __restrict__ row_map, int N, int K, long total) {
  const int KP = K >> 6, KG = K >> 7;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
    const long unit = c >> 6;
    const int lane = (int)(c & 63);
    const int g = (int)(unit / KP), p = (int)(unit % KP);
    const int r = g * 16 + (lane & 15);
    const int sr = row_map ? row_map[r] : r;
    const uint8_t* row = q_src + (size_t)sr * K + (size_t)p * 64 + 8 * (lane >> 4);
    const u32x2_t lo = *reinterpret_cast<const u32x2_t*>(row);
    const u32x2_t hi = *reinterpret_cast<const u32x2_t*>(row + 32);
    q_dst[c] = u32x4_t{lo[0] ^ W8_FLIP, lo[1] ^ W8_FLIP, hi[0] ^ W8_FLIP, hi[1] ^ W8_FLIP};
    if (lane < 16 && !(p & 1)) s_dst[((size_t)g * KG + (p >> 1)) * 16 + lane] = s_src[(size_t)sr * KG + (p >> 1)];
  }
}

__global__ void w8_frag_to_rows_kernel(const u32x4_t* __restrict__ q_src, const bf16_t* __restrict__ s_src, uint8_t* __restrict__ q_dst,
                                       bf16_t* __restrict__ s_dst, int N, int K, long total) {
  const int KP = K >> 6, KG = K >> 7;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
    const long unit = c >> 6;
    const int lane = (int)(c & 63);
    const int g = (int)(unit / KP), p = (int)(unit % KP);
    const int r = g * 16 + (lane & 15);
    uint8_t* row = q_dst + (size_t)r * K + (size_t)p * 64 + 8 * (lane >> 4);
    const u32x4_t v = q_src[c];
    *reinterpret_cast<u32x2_t*>(row) = u32x2_t{v[0] ^ W8_FLIP, v[1] ^ W8_FLIP};
    *reinterpret_cast<u32x2_t*>(row + 32) = u32x2_t{v[2] ^ W8_FLIP, v[3] ^ W8_FLIP};
    if (lane < 16 && !(p & 1)) s_dst[(size_t)r * KG + (p >> 1)] = s_src[((size_t)g * KG + (p >> 1)) * 16 + lane];
  }
}

// w8 frag unit (g, p), lane l -> the bf16 frag chunks of k-tiles 2p and 2p+1 of the same lane, bf16(s * q)
__global__ void w8_dequant_frag_kernel(const u32x4_t* __restrict__ q_src, const bf16_t* __restrict__ s_src, u32x4_t* __restrict__ dst,
                                       int N, int K, long total) {
  const int KP = K >> 6, KG = K >> 7, KT = K >> 5;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
    const long unit = c >> 6;
    const int lane = (int)(c & 63);
    const int g = (int)(unit / KP), p = (int)(unit % KP);
    const float s = bf2f(s_src[((size_t)g * KG + (p >> 1)) * 16 + (lane & 15)]);
    const u32x4_t v = q_src[c];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      u32x4_t o;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t w = v[2 * h + (i >> 1)] >> (16 * (i & 1));
        o[i] = pack_bf2(s * (float)(int8_t)w, s * (float)(int8_t)(w >> 8));
      }
      dst[((size_t)g * KT + 2 * p + h) * 64 + lane] = o;
    }
  }
}

extern "C" int ssd_w8_rows_to_frag(const void* q_rows, const void* s_rows, void* q_frag, void* s_frag, const int32_t* row_map, int N,
                                   int K, void* stream) {
  if (!wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !q_frag || !s_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 64) * 64;
  hipLaunchKernelGGL(w8_rows_to_frag_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)q_rows,
                     (const bf16_t*)s_rows, (u32x4_t*)q_frag, (bf16_t*)s_frag, row_map, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_w8_frag_to_rows(const void* q_frag, const void* s_frag, void* q_rows, void* s_rows, int N, int K, void* stream) {
  if (!wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  if (!q_rows || !s_rows || !q_frag || !s_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 64) * 64;
  hipLaunchKernelGGL(w8_frag_to_rows_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const bf16_t*)s_frag, (uint8_t*)q_rows, (bf16_t*)s_rows, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_w8_dequant_frag(const void* q_frag, const void* s_frag, void* w_frag, int N, int K, void* stream) {
  if (!wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  if (!q_frag || !s_frag || !w_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 64) * 64;
  hipLaunchKernelGGL(w8_dequant_frag_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (const bf16_t*)s_frag, (u32x4_t*)w_frag, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------
// The GEMM: wq_gemm_kernel with a K unit of one k-pair (64 columns, two k-tiles, fp8's), the scale quad of the unit's column group
// as the stage's side-band (w4's table, read at half the unit index).  XS: the x operands ride in the double-buffered stage; at
// MT = 8 with two row groups they would not fit the VGPR budget (172 / 192 bytes of scratch per lane) and are loaded per unit
// instead (from L2: x is shared by every workgroup), as the block-scaled fp8 policy does there.
// ---------------------------------------------------------------------------------------------------------------------
struct W8 {
  static constexpr int KSHIFT = 6, KT = 2;
  static constexpr bool ROW_SCALE = false, HAS_Z = false;
  template <int MT, int NT>
  struct Side {
    u32x2_t s[NT];          // the 4 bf16 group scales of the lane's output rows
  };
  struct Band {
    const size_t sstride;   // 8-byte scale quads between adjacent row groups of s: 4 per column group, K / 128 groups
    const u32x2_t* sp;
    __device__ Band(const void* Sf, const void*, size_t g0, int KP, int lane)
        : sstride((size_t)(KP >> 1) << 2), sp((const u32x2_t*)Sf + g0 * sstride + (lane >> 4)) {}
    template <class S>
    __device__ void load(S& s, int nt, int kp) const {
      s.s[nt] = __builtin_nontemporal_load(sp + nt * sstride + ((size_t)(kp >> 1) << 2));
    }
    __device__ void advance(int nt) { sp += (size_t)nt * sstride; }
  };

  // one k-pair: convert every row group's two k-tile slices and its scales, then per token tile and row group a fresh partial of two
  // MFMAs and acc += s * partial.  With XS the x operands come from the stage; without, each token tile's two are loaded here.
  template <int MT, int NT, bool XS, class S, class XL>
  static __device__ __forceinline__ void group(f32x4_t (&acc)[NT][MT], const S& st, int kp, const XL& xload, const Band&) {
    u32x4_t w[NT][2];
    float s[NT][4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      w[nt][0] = w8x8_to_bf16(st.a[nt][0], st.a[nt][1]);
      w[nt][1] = w8x8_to_bf16(st.a[nt][2], st.a[nt][3]);
      s[nt][0] = bf2f(st.s[nt][0] & 0xffffu); s[nt][1] = bf2f(st.s[nt][0] >> 16);
      s[nt][2] = bf2f(st.s[nt][1] & 0xffffu); s[nt][3] = bf2f(st.s[nt][1] >> 16);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      u32x4_t b[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = XS ? st.b[XS ? mt : 0][j] : xload(mt, 2 * kp + j);
      // without this fence the scheduler hoists the x loads of later token tiles over the MFMAs and MT = 8, NT = 2 goes to scratch
      // (32 / 56 bytes per lane)
      if constexpr (!XS) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        f32x4_t p = mfma16(w[nt][0], b[0], f32x4_t{0.f, 0.f, 0.f, 0.f});
        p = mfma16(w[nt][1], b[1], p);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[nt][mt][r] = __builtin_fmaf(s[nt][r], p[r], acc[nt][mt][r]);
      }
    }
  }

  // U per (MT, NT, deep): the fp8 policy's table (the same code bytes per unit; the scale quads add 4 U NT VGPRs to the
  // double-buffered stage, 2 U (6 NT + 8 MT) in all), within the VGPR budget of a <= 8-wave workgroup without spills
  // (profiles/w8a16_resources.txt)
  static constexpr WqForm FORMS[4][3][2] = {
      /* MT 1 */ {{{4, true}, {6, true}}, {{2, true}, {4, true}}, {{1, true}, {2, true}}},
      /* MT 2 */ {{{2, true}, {}}, {{2, true}, {}}, {}},
      /* MT 4 */ {{{1, true}, {}}, {{1, true}, {}}, {}},
      /* MT 8 */ {{{1, true}, {}}, {{1, false}, {}}, {}},
  };
};

extern "C" int ssd_gemm_w8a16_cfg(const void* x_frag, const void* q_frag, const void* s_frag, const void* bias, void* y, int M, int N,
                                  int K, int ldy, int epilogue, int nt, int waves, void* stream) {
  if (M <= 0 || M > 128 || !wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;   // whole scale groups: two code units each
  return wq_gemm_cfg<W8>(WqArgs{x_frag, q_frag, s_frag, nullptr, bias, y, M, N, K, ldy}, epilogue, nt, waves, stream);
}

// Default decomposition: the fp8 GEMM's (gemm_fp8.hip; the same 1 KiB code units per row group, so a matrix streams like the fp8
// one), not re-tuned.
extern "C" int ssd_gemm_w8a16(const void* x_frag, const void* q_frag, const void* s_frag, const void* bias, void* y, int M, int N, int K,
                              int ldy, int epilogue, void* stream) {
  if (M <= 0 || M > 128 || !wq_shape_ok(N, K, 128)) return SSD_ERR_SHAPE;
  const int groups = N / 16, KP = K / 64, mt = (M + 15) / 16;
  const bool silu = epilogue == WQ_SILU_FRAG;
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
    return ssd_gemm_w8a16_cfg(x_frag, q_frag, s_frag, bias, y, M, N, K, ldy, epilogue, nt, waves | (tpw << 8), stream);
  }
  nt = (silu || (groups >= 2048 && groups % 2 == 0)) ? 2 : 1;
  waves = 8;
  while (waves > 1 && KP / waves < 4) waves >>= 1;
  const int mtr = mt == 2 ? 2 : (mt <= 4 ? 4 : 8);
  while (waves > 1 && (size_t)waves * nt * mtr * 1024 > 64 * 1024) waves >>= 1;
  return ssd_gemm_w8a16_cfg(x_frag, q_frag, s_frag, bias, y, M, N, K, ldy, epilogue, nt, waves, stream);
}
