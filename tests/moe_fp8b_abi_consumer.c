/* Plain-C consumer of include/ssd_hip_moe_fp8b.h (tests/test_moe_fp8b_cpu.py builds it with cc -std=c99 -Wall -Werror and links
 * libssdhip.so): the grouped block-scaled FP8 expert GEMM called with a null pointer, an unknown epilogue or a shape outside the header's list
 * must return SSD_ERR_ARG or SSD_ERR_SHAPE from its argument validation, before any launch (no GPU is needed for that). */
#include <stdio.h>
#include "ssd_hip_moe_fp8b.h"

static int failures = 0;

static void expect(const char* what, int rc, int want) {
  if (rc != want) {
    printf("FAIL %s returned %d, expected %d\n", what, rc, want);
    ++failures;
  } else {
    printf("ok   %s -> %d\n", what, rc);
  }
}

int main(void) {
  char buf[64];
  void* p = buf;
  int32_t* m = (int32_t*)buf;
  const float* s = (const float*)buf;
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION) {
    printf("FAIL abi version %d != %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  expect("null rows", ssd_moe_gemm_fp8b(NULL, p, s, m, m, p, 1, 2, 8, 64, 128, SSD_MOE_EPI_UP, NULL), SSD_ERR_ARG);
  expect("null codes", ssd_moe_gemm_fp8b(p, NULL, s, m, m, p, 1, 2, 8, 64, 128, SSD_MOE_EPI_UP, NULL), SSD_ERR_ARG);
  expect("null scales", ssd_moe_gemm_fp8b(p, p, NULL, m, m, p, 1, 2, 8, 64, 128, SSD_MOE_EPI_UP, NULL), SSD_ERR_ARG);
  expect("null out", ssd_moe_gemm_fp8b(p, p, s, m, m, NULL, 1, 2, 8, 64, 128, SSD_MOE_EPI_UP, NULL), SSD_ERR_ARG);
  expect("epilogue 2", ssd_moe_gemm_fp8b(p, p, s, m, m, p, 1, 2, 8, 64, 128, 2, NULL), SSD_ERR_ARG);
  expect("zero T", ssd_moe_gemm_fp8b(p, p, s, m, m, p, 0, 2, 8, 64, 128, SSD_MOE_EPI_UP, NULL), SSD_ERR_SHAPE);
  expect("k above E", ssd_moe_gemm_fp8b(p, p, s, m, m, p, 1, SSD_MOE_MAX_K + 1, 8, 64, 128, SSD_MOE_EPI_UP, NULL), SSD_ERR_SHAPE);
  expect("E 4", ssd_moe_gemm_fp8b(p, p, s, m, m, p, 1, 2, SSD_MOE_MIN_E - 4, 64, 128, SSD_MOE_EPI_UP, NULL), SSD_ERR_SHAPE);
  expect("K 64", ssd_moe_gemm_fp8b(p, p, s, m, m, p, 1, 2, 8, 64, 64, SSD_MOE_EPI_UP, NULL), SSD_ERR_SHAPE);
  expect("up N 96", ssd_moe_gemm_fp8b(p, p, s, m, m, p, 1, 2, 8, 96, 128, SSD_MOE_EPI_UP, NULL), SSD_ERR_SHAPE);
  expect("down N 24", ssd_moe_gemm_fp8b(p, p, s, m, m, p, 1, 2, 8, 24, 128, SSD_MOE_EPI_DOWN, NULL), SSD_ERR_SHAPE);
  printf("%d failures\n", failures);
  return failures != 0;
}
