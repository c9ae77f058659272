// What the per-row (gemm_fp8.hip) and the block-scaled (gemm_fp8b.hip) fp8 GEMMs share: the widening of e4m3 codes to bf16.
#pragma once
#include "common.h"

// 8 e4m3 codes (two 32-bit words) -> the 8 bf16 of one MFMA operand slice
__device__ __forceinline__ u32x4_t fp8x8_to_bf16(uint32_t w0, uint32_t w1) {
  u32x4_t r;
  r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false));
  r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true));
  r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false));
  r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true));
  return r;
}
