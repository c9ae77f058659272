// What the dense (gemm_mxfp4.hip) and the grouped expert (moe_mxfp4.hip) MXFP4 GEMMs share: the widening of e2m1 codes with their
// e8m0 block scale to the exact bf16 weights of one MFMA operand slice (include/ssd_hip_mxfp4.h).
#pragma once
#include "common.h"

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
