/* Plain-C consumer of include/ssd_hip_quant.h (tests/test_fp8_cpu.py builds it with cc -std=c99 -Wall -Werror and links libssdhip.so):
 * every FP8 entry point called with null pointers or zero / misaligned sizes must return SSD_ERR_SHAPE or SSD_ERR_ARG from its
 * argument validation, before any launch (no GPU is needed for that). */
#include <stdio.h>
#include "ssd_hip_quant.h"

static int failures = 0;

static void expect(const char* what, int rc) {
  if (rc != SSD_ERR_SHAPE && rc != SSD_ERR_ARG) {
    printf("FAIL %s returned %d\n", what, rc);
    ++failures;
  } else {
    printf("ok   %s -> %d\n", what, rc);
  }
}

int main(void) {
  char buf[64];
  void* p = buf;
  const float* f = (const float*)buf;
  const int32_t* m = (const int32_t*)buf;
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION) {
    printf("FAIL abi version %d != %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  expect("ssd_fp8_rows_to_frag zero N", ssd_fp8_rows_to_frag(p, p, m, 0, 64, NULL));
  expect("ssd_fp8_rows_to_frag K % 64", ssd_fp8_rows_to_frag(p, p, m, 16, 32, NULL));
  expect("ssd_fp8_rows_to_frag null src", ssd_fp8_rows_to_frag(NULL, p, NULL, 16, 64, NULL));
  expect("ssd_fp8_rows_to_frag null dst", ssd_fp8_rows_to_frag(p, NULL, NULL, 16, 64, NULL));
  expect("ssd_fp8_frag_to_rows zero K", ssd_fp8_frag_to_rows(p, p, 16, 0, NULL));
  expect("ssd_fp8_frag_to_rows N % 16", ssd_fp8_frag_to_rows(p, p, 8, 64, NULL));
  expect("ssd_fp8_frag_to_rows null", ssd_fp8_frag_to_rows(NULL, NULL, 16, 64, NULL));
  expect("ssd_fp8_dequant_frag zero N", ssd_fp8_dequant_frag(p, f, p, 0, 64, NULL));
  expect("ssd_fp8_dequant_frag null scale", ssd_fp8_dequant_frag(p, NULL, p, 16, 64, NULL));
  expect("ssd_fp8_dequant_frag null dst", ssd_fp8_dequant_frag(p, f, NULL, 16, 64, NULL));
  expect("ssd_gemm_fp8 zero M", ssd_gemm_fp8(p, p, f, NULL, p, 0, 16, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8 M > 128", ssd_gemm_fp8(p, p, f, NULL, p, 129, 16, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8 K % 64", ssd_gemm_fp8(p, p, f, NULL, p, 1, 16, 96, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8 null x", ssd_gemm_fp8(NULL, p, f, NULL, p, 1, 16, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8 null scale", ssd_gemm_fp8(p, p, NULL, NULL, p, 1, 16, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8 ldy < N", ssd_gemm_fp8(p, p, f, NULL, p, 1, 32, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8 bad epilogue", ssd_gemm_fp8(p, p, f, NULL, p, 1, 64, 64, 64, 7, NULL));
  expect("ssd_gemm_fp8_cfg zero N", ssd_gemm_fp8_cfg(p, p, f, NULL, p, 1, 0, 64, 16, SSD_EPI_ROWS, 1, 1, NULL));
  expect("ssd_gemm_fp8_cfg null y", ssd_gemm_fp8_cfg(p, p, f, NULL, NULL, 1, 16, 64, 16, SSD_EPI_ROWS, 1, 1, NULL));
  expect("ssd_gemm_fp8_cfg waves 0", ssd_gemm_fp8_cfg(p, p, f, NULL, p, 1, 16, 64, 16, SSD_EPI_ROWS, 1, 0, NULL));
  expect("ssd_gemm_fp8_cfg waves 9", ssd_gemm_fp8_cfg(p, p, f, NULL, p, 1, 16, 64, 16, SSD_EPI_ROWS, 1, 9, NULL));
  expect("ssd_gemm_fp8_cfg nt 3", ssd_gemm_fp8_cfg(p, p, f, NULL, p, 1, 48, 64, 48, SSD_EPI_ROWS, 3, 1, NULL));
  expect("ssd_gemm_fp8_cfg silu odd nt", ssd_gemm_fp8_cfg(p, p, f, NULL, p, 1, 64, 64, 0, SSD_EPI_SILU_FRAG, 1, 1, NULL));
  printf("%d failures\n", failures);
  return failures != 0;
}
