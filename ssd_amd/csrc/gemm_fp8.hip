// FP8 (OCP e4m3fn) weight-only GEMMs for the quantized target: y = x . (s (.) q)^T with bf16 activations, e4m3 weight codes and one
// fp32 scale per output row (include/ssd_hip_quant.h).  The walk is wq_gemm_kernel's (gemm_wq.h); what is fp8's own:
//  * q is stored "fp8 frag": one 1 KiB unit per (16-row group, 64-column k-pair), lane l holding its 8-byte slices of k-tiles 2p and
//    2p+1 side by side -- one 16-byte lane load, one contiguous 1 KiB wave load, two MFMA k-steps.
//  * codes go straight to VGPRs with non-temporal loads and are widened with v_cvt_scalef32_pk_bf16_fp8 at scale 1.0: every e4m3
//    value is a bf16 value, so the conversion is exact and the MFMA is the bf16 one with fp32 accumulation.
//  * the row scale (and the bias) are applied to the fp32 sums in the epilogue.
#include "common.h"
#include "gemm_wq.h"
#include "gemm_fp8.h"   // fp8x8_to_bf16, shared with gemm_fp8b.hip

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

extern "C" int ssd_fp8_rows_to_frag(const void* q_rows, void* q_frag, const int32_t* row_map, int N, int K, void* stream) {
  if (!wq_shape_ok(N, K, 64)) return SSD_ERR_SHAPE;
  if (!q_rows || !q_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 64) * 64;
  hipLaunchKernelGGL(fp8_rows_to_frag_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)q_rows,
                     (u32x4_t*)q_frag, row_map, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_fp8_frag_to_rows(const void* q_frag, void* q_rows, int N, int K, void* stream) {
  if (!wq_shape_ok(N, K, 64)) return SSD_ERR_SHAPE;
  if (!q_rows || !q_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 64) * 64;
  hipLaunchKernelGGL(fp8_frag_to_rows_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag,
                     (uint8_t*)q_rows, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_fp8_dequant_frag(const void* q_frag, const float* scale, void* w_frag, int N, int K, void* stream) {
  if (!wq_shape_ok(N, K, 64)) return SSD_ERR_SHAPE;
  if (!q_frag || !scale || !w_frag) return SSD_ERR_ARG;
  const long total = (long)(N / 16) * (K / 64) * 64;
  hipLaunchKernelGGL(fp8_dequant_frag_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)q_frag, scale,
                     (u32x4_t*)w_frag, N, K, total);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------
// The GEMM: wq_gemm_kernel with a K unit of one k-pair (64 columns, two k-tiles), no side-band in the stage (the scale is per row
// and waits for the epilogue) and x always staged with the codes.
// ---------------------------------------------------------------------------------------------------------------------
struct Fp8 {
  static constexpr int KSHIFT = 6, KT = 2;
  static constexpr bool ROW_SCALE = true, HAS_Z = false;
  template <int MT, int NT>
  struct Side {};
  struct Band {
    __device__ Band(const void*, const void*, size_t, int, int) {}
    template <class S>
    __device__ void load(S&, int, int) const {}
    __device__ void advance(int) {}
  };

  // one k-pair: convert a row group's two k-tile slices, then its MFMAs against every token tile
  template <int MT, int NT, bool XS, class S, class XL>
  static __device__ __forceinline__ void group(f32x4_t (&acc)[NT][MT], const S& s, int, const XL&, const Band&) {
    static_assert(XS, "fp8 stages x at every MT");
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const u32x4_t a0 = fp8x8_to_bf16(s.a[nt][0], s.a[nt][1]), a1 = fp8x8_to_bf16(s.a[nt][2], s.a[nt][3]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        acc[nt][mt] = mfma16(a0, s.b[mt][0], acc[nt][mt]);
        acc[nt][mt] = mfma16(a1, s.b[mt][1], acc[nt][mt]);
      }
    }
  }

  // U per (MT, NT, deep): 4-8 KiB of codes in flight per wave in the plain form, twice that in the deep one, within the VGPR budget
  // of a <= 8-wave workgroup (256 per lane: the double-buffered stage is 2 * U * (4 NT + 8 MT) VGPRs)
  static constexpr WqForm FORMS[4][3][2] = {
      /* MT 1 */ {{{4, true}, {6, true}}, {{2, true}, {4, true}}, {{1, true}, {2, true}}},
      /* MT 2 */ {{{2, true}, {}}, {{2, true}, {}}, {}},
      /* MT 4 */ {{{1, true}, {}}, {{1, true}, {}}, {}},
      /* MT 8 */ {{{1, true}, {}}, {{1, true}, {}}, {}},
  };
};

extern "C" int ssd_gemm_fp8_cfg(const void* x_frag, const void* q_frag, const float* scale, const void* bias, void* y, int M, int N, int K,
                                int ldy, int epilogue, int nt, int waves, void* stream) {
  return wq_gemm_cfg<Fp8>(WqArgs{x_frag, q_frag, scale, nullptr, bias, y, M, N, K, ldy}, epilogue, nt, waves, stream);
}


// Default decomposition.  One token tile: the bf16 skinny table at the k-pair count (a 1 KiB unit covers 64 columns here, 32 in
// bf16, so a matrix streams like a bf16 one of half its K), in the plain form, re-tuned where the 70B verify shapes were swept at
// M = 8 (profiles/fp8_sweep.jsonl, every nt / deep / waves / tpw): gate_up 81.3 -> 75.9 us with 4 consecutive tiles per workgroup,
// o_proj 16.1 -> 13.4 and down_proj 43.3 -> 41.1 with 2 row groups x 8 waves, qkv 22.1 -> 18.7 with 4 waves.  More token tiles: one
// or two row groups per workgroup, waves sized so that every wave has a few k-pairs, LDS for the combine <= 64 KiB.
extern "C" int ssd_gemm_fp8(const void* x_frag, const void* q_frag, const float* scale, const void* bias, void* y, int M, int N, int K,
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
    return ssd_gemm_fp8_cfg(x_frag, q_frag, scale, bias, y, M, N, K, ldy, epilogue, nt, waves | (tpw << 8), stream);
  }
  nt = (epilogue == WQ_SILU_FRAG || (groups >= 2048 && groups % 2 == 0)) ? 2 : 1;
  waves = 8;
  while (waves > 1 && KP / waves < 4) waves >>= 1;
  const int mtr = mt == 2 ? 2 : (mt <= 4 ? 4 : 8);
  while (waves > 1 && (size_t)waves * nt * mtr * 1024 > 64 * 1024) waves >>= 1;
  return ssd_gemm_fp8_cfg(x_frag, q_frag, scale, bias, y, M, N, K, ldy, epilogue, nt, waves, stream);
}
