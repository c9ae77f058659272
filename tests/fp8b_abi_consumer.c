/* Plain-C consumer of include/ssd_hip_fp8b.h (tests/test_fp8b_cpu.py builds it with cc -std=c99 -Wall -Werror and links
 * libssdhip.so): every block-scaled fp8 entry point called with null pointers or zero / misaligned sizes must return SSD_ERR_SHAPE or
 * SSD_ERR_ARG from its argument validation, before any launch (no GPU is needed for that). */
#include <stdio.h>
#include "ssd_hip_fp8b.h"

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
  float buf[16];
  void* p = buf;
  const float* s = buf;
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION) {
    printf("FAIL abi version %d != %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  expect("ssd_fp8b_dequant_frag zero N", ssd_fp8b_dequant_frag(p, s, p, 0, 64, NULL));
  expect("ssd_fp8b_dequant_frag K % 64", ssd_fp8b_dequant_frag(p, s, p, 16, 96, NULL));
  expect("ssd_fp8b_dequant_frag N % 16", ssd_fp8b_dequant_frag(p, s, p, 24, 64, NULL));
  expect("ssd_fp8b_dequant_frag null codes", ssd_fp8b_dequant_frag(NULL, s, p, 16, 64, NULL));
  expect("ssd_fp8b_dequant_frag null scales", ssd_fp8b_dequant_frag(p, NULL, p, 16, 64, NULL));
  expect("ssd_fp8b_dequant_frag null dst", ssd_fp8b_dequant_frag(p, s, NULL, 16, 64, NULL));
  expect("ssd_gemm_fp8b zero M", ssd_gemm_fp8b(p, p, s, NULL, p, 0, 16, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8b M > 128", ssd_gemm_fp8b(p, p, s, NULL, p, 129, 16, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8b K % 64", ssd_gemm_fp8b(p, p, s, NULL, p, 1, 16, 32, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8b N % 16", ssd_gemm_fp8b(p, p, s, NULL, p, 1, 24, 64, 24, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8b null x", ssd_gemm_fp8b(NULL, p, s, NULL, p, 1, 16, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8b null codes", ssd_gemm_fp8b(p, NULL, s, NULL, p, 1, 16, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8b null scales", ssd_gemm_fp8b(p, p, NULL, NULL, p, 1, 16, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8b null y", ssd_gemm_fp8b(p, p, s, NULL, NULL, 1, 16, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8b ldy < N", ssd_gemm_fp8b(p, p, s, NULL, p, 1, 32, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_fp8b bad epilogue", ssd_gemm_fp8b(p, p, s, NULL, p, 1, 64, 64, 64, 7, NULL));
  expect("ssd_gemm_fp8b_cfg zero N", ssd_gemm_fp8b_cfg(p, p, s, NULL, p, 1, 0, 64, 16, SSD_EPI_ROWS, 1, 1, NULL));
  expect("ssd_gemm_fp8b_cfg null q", ssd_gemm_fp8b_cfg(p, NULL, s, NULL, p, 1, 16, 64, 16, SSD_EPI_ROWS, 1, 1, NULL));
  expect("ssd_gemm_fp8b_cfg null scales", ssd_gemm_fp8b_cfg(p, p, NULL, NULL, p, 1, 16, 64, 16, SSD_EPI_ROWS, 1, 1, NULL));
  expect("ssd_gemm_fp8b_cfg waves 0", ssd_gemm_fp8b_cfg(p, p, s, NULL, p, 1, 16, 64, 16, SSD_EPI_ROWS, 1, 0, NULL));
  expect("ssd_gemm_fp8b_cfg waves 9", ssd_gemm_fp8b_cfg(p, p, s, NULL, p, 1, 16, 64, 16, SSD_EPI_ROWS, 1, 9, NULL));
  expect("ssd_gemm_fp8b_cfg nt 3", ssd_gemm_fp8b_cfg(p, p, s, NULL, p, 1, 48, 64, 48, SSD_EPI_ROWS, 3, 1, NULL));
  expect("ssd_gemm_fp8b_cfg nt not dividing", ssd_gemm_fp8b_cfg(p, p, s, NULL, p, 1, 48, 64, 48, SSD_EPI_ROWS, 2, 1, NULL));
  expect("ssd_gemm_fp8b_cfg silu odd nt", ssd_gemm_fp8b_cfg(p, p, s, NULL, p, 1, 64, 64, 0, SSD_EPI_SILU_FRAG, 1, 1, NULL));
  expect("ssd_gemm_fp8b_cfg silu N % 64", ssd_gemm_fp8b_cfg(p, p, s, NULL, p, 1, 32, 64, 0, SSD_EPI_SILU_FRAG, 2, 1, NULL));
  expect("ssd_gemm_fp8b_cfg deep at M = 64", ssd_gemm_fp8b_cfg(p, p, s, NULL, p, 64, 32, 64, 32, SSD_EPI_ROWS, 2 | 256, 1, NULL));
  printf("%d failures\n", failures);
  return failures != 0;
}
