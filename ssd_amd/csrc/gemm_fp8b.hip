// Block-scaled FP8 weight-only GEMMs (include/ssd_hip_fp8b.h): y = x . (s (.) q)^T with bf16 activations, e4m3 codes in the fp8 frag
// layout of gemm_fp8.hip and one fp32 scale per (16-row group, 128-column block).  The walk is wq_gemm_kernel's (gemm_wq.h) and the
// conversion is fp8's (gemm_fp8.h); what is this format's own:
//  * the side-band of a stage is the unit's scale, one float per row group.  It is uniform over the wave (every row of an MFMA tile
//    shares it), read from a [N/16][KB] table with the block index ku >> 1: two 64-column units share a block, and where
//    K % 128 == 64 the last block holds one unit.
//  * a unit's two MFMA k-steps go into a zeroed fp32 temporary and acc = fma(s, temporary, acc) in fp32: the scale is an arbitrary
//    positive number, so it never rides in the convert instruction's (power-of-two) scale operand.
//  * the epilogue has no scale left to apply (ROW_SCALE false): bias, rounding and SiLU only.
#include "common.h"
#include "gemm_wq.h"
#include "gemm_fp8.h"

// fp8 frag unit (g, p) -> the bf16 frag chunks of k-tiles 2p and 2p+1 of the same lane, bf16(s[g][p / 2] * q)
__global__ void fp8b_dequant_frag_kernel(const u32x4_t* __restrict__ src, const float* __restrict__ sgrp, u32x4_t* __restrict__ dst,
                                         int N, int K, long total) {
  const int KP = K >> 6, KT = K >> 5, KB = (K + 127) >> 7;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
    const long unit = c >> 6;
    const int lane = (int)(c & 63);
    const int g = (int)(unit / KP), p = (int)(unit % KP);
    const float s = sgrp[(size_t)g * KB + (p >> 1)];
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

extern "C" int ssd_fp8b_dequant_frag(const void* q_frag, const float* s_grp, void* w_frag, int N, int K, void* stream) {
  if (!wq_shape_ok(N, K, 64)) return SSD_ERR_SHAPE;
  if (!q_frag || !s_grp || !w_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 64) * 64;
  hipLaunchKernelGGL(fp8b_dequant_frag_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag, s_grp,
                     (u32x4_t*)w_frag, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------
// The GEMM: wq_gemm_kernel with fp8's K unit (one k-pair: 64 columns, two k-tiles) and the unit's block scale as the side-band.
// ---------------------------------------------------------------------------------------------------------------------
struct Fp8B {
  static constexpr int KSHIFT = 6, KT = 2;
  static constexpr bool ROW_SCALE = false, HAS_Z = false;
  template <int MT, int NT>
  struct Side {
    float s[NT];   // the unit's block scale per row group
  };
  struct Band {
    const int KB;      // scales between adjacent row groups: column blocks, ceil(KU / 2)
    const float* sp;   // the table row of the workgroup's current first row group
    __device__ Band(const void* Sf, const void*, size_t g0, int KU, int) : KB((KU + 1) >> 1), sp((const float*)Sf + g0 * (size_t)KB) {}
    template <class S>
    __device__ void load(S& s, int nt, int ku) const {
      s.s[nt] = sp[(size_t)nt * KB + (ku >> 1)];
    }
    __device__ void advance(int nt) { sp += (size_t)nt * KB; }
  };

  // one k-pair: convert a row group's two k-tile slices; per token tile two MFMAs into a zeroed temporary, then acc += s * temporary.
  // With XS the x operands come from the stage; without, each token tile's two are loaded here (from L2: x is shared by every
  // workgroup).
  template <int MT, int NT, bool XS, class S, class XL>
  static __device__ __forceinline__ void group(f32x4_t (&acc)[NT][MT], const S& st, int ku, const XL& xload, const Band&) {
    u32x4_t a[NT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      a[nt][0] = fp8x8_to_bf16(st.a[nt][0], st.a[nt][1]);
      a[nt][1] = fp8x8_to_bf16(st.a[nt][2], st.a[nt][3]);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      u32x4_t b[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = XS ? st.b[XS ? mt : 0][j] : xload(mt, 2 * ku + j);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        f32x4_t t = f32x4_t{0.f, 0.f, 0.f, 0.f};
        t = mfma16(a[nt][0], b[0], t);
        t = mfma16(a[nt][1], b[1], t);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[nt][mt][r] = __builtin_fmaf(st.s[nt], t[r], acc[nt][mt][r]);
      }
    }
  }

  // U per (MT, NT, deep): fp8's table (the stage grows by NT floats), except that at MT = 8 with two row groups the staged x no
  // longer fits beside the temporaries (256 VGPRs and 12 / 24 bytes of scratch per lane): x per unit there, as w4a16 does at
  // MT = 8.  profiles/fp8b_resources.txt: every instantiation without scratch.
  static constexpr WqForm FORMS[4][3][2] = {
      /* MT 1 */ {{{4, true}, {6, true}}, {{2, true}, {4, true}}, {{1, true}, {2, true}}},
      /* MT 2 */ {{{2, true}, {}}, {{2, true}, {}}, {}},
      /* MT 4 */ {{{1, true}, {}}, {{1, true}, {}}, {}},
      /* MT 8 */ {{{1, true}, {}}, {{1, false}, {}}, {}},
  };
};

extern "C" int ssd_gemm_fp8b_cfg(const void* x_frag, const void* q_frag, const float* s_grp, const void* bias, void* y, int M, int N,
                                 int K, int ldy, int epilogue, int nt, int waves, void* stream) {
  return wq_gemm_cfg<Fp8B>(WqArgs{x_frag, q_frag, s_grp, nullptr, bias, y, M, N, K, ldy}, epilogue, nt, waves, stream);
}

// Default decomposition: ssd_gemm_fp8's classes (the codes, their layout and the walk are the same; the side-band adds 4 bytes per
// KiB unit).  M = 8 sweep of every nt / deep / waves / tpw at the 70B and Qwen3-32B shapes (profiles/fp8b_sweep.jsonl, default /
// best in us): 70B o_proj 13.50 / 13.49, gate_up 75.09 / 75.00, down_proj 41.08 / 40.62, qkv 19.12 / 18.44; Qwen3-32B down_proj
// 32.41 / 32.42, gate_up 46.50 / 45.65, qkv 12.99 / 12.13 (4 row groups x 8 waves), o_proj 12.80 / 12.15 (2 row groups x 8 waves).
// The last two and 70B qkv are open: a class for them wants a second sweep to confirm it, which has not been run.
extern "C" int ssd_gemm_fp8b(const void* x_frag, const void* q_frag, const float* s_grp, const void* bias, void* y, int M, int N, int K,
                             int ldy, int epilogue, void* stream) {
  if (M <= 0 || M > 128 || !wq_shape_ok(N, K, 64)) return SSD_ERR_SHAPE;
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
    return ssd_gemm_fp8b_cfg(x_frag, q_frag, s_grp, bias, y, M, N, K, ldy, epilogue, nt, waves | (tpw << 8), stream);
  }
  nt = (silu || (groups >= 2048 && groups % 2 == 0)) ? 2 : 1;
  waves = 8;
  while (waves > 1 && KP / waves < 4) waves >>= 1;
  const int mtr = mt == 2 ? 2 : (mt <= 4 ? 4 : 8);
  while (waves > 1 && (size_t)waves * nt * mtr * 1024 > 64 * 1024) waves >>= 1;
  return ssd_gemm_fp8b_cfg(x_frag, q_frag, s_grp, bias, y, M, N, K, ldy, epilogue, nt, waves, stream);
}
