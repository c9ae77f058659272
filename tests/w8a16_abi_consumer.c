/* Plain-C consumer of include/ssd_hip_w8a16.h (tests/test_w8a16_cpu.py builds it with cc -std=c99 -Wall -Werror and links
 * libssdhip.so): every W8A16 entry point called with null pointers or zero / misaligned sizes must return SSD_ERR_SHAPE or SSD_ERR_ARG
 * from its argument validation, before any launch (no GPU is needed for that). */
#include <stdio.h>
#include "ssd_hip_w8a16.h"

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
  const int32_t* m = (const int32_t*)buf;
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION) {
    printf("FAIL abi version %d != %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  expect("ssd_w8_rows_to_frag zero N", ssd_w8_rows_to_frag(p, p, p, p, m, 0, 128, NULL));
  expect("ssd_w8_rows_to_frag K % 128", ssd_w8_rows_to_frag(p, p, p, p, m, 16, 64, NULL));
  expect("ssd_w8_rows_to_frag null scales", ssd_w8_rows_to_frag(p, NULL, p, p, NULL, 16, 128, NULL));
  expect("ssd_w8_frag_to_rows K % 128", ssd_w8_frag_to_rows(p, p, p, p, 16, 192, NULL));
  expect("ssd_w8_frag_to_rows null", ssd_w8_frag_to_rows(NULL, NULL, p, p, 16, 128, NULL));
  expect("ssd_w8_dequant_frag K % 128", ssd_w8_dequant_frag(p, p, p, 16, 64, NULL));
  expect("ssd_w8_dequant_frag null scales", ssd_w8_dequant_frag(p, NULL, p, 16, 128, NULL));
  expect("ssd_gemm_w8a16 M > 128", ssd_gemm_w8a16(p, p, p, NULL, p, 129, 16, 128, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_w8a16 K % 128", ssd_gemm_w8a16(p, p, p, NULL, p, 1, 16, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_w8a16 ldy < N", ssd_gemm_w8a16(p, p, p, NULL, p, 1, 32, 128, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_w8a16 bad epilogue", ssd_gemm_w8a16(p, p, p, NULL, p, 1, 64, 128, 64, 7, NULL));
  expect("ssd_gemm_w8a16_cfg K % 128", ssd_gemm_w8a16_cfg(p, p, p, NULL, p, 1, 16, 192, 16, SSD_EPI_ROWS, 1, 1, NULL));
  expect("ssd_gemm_w8a16_cfg waves 9", ssd_gemm_w8a16_cfg(p, p, p, NULL, p, 1, 16, 128, 16, SSD_EPI_ROWS, 1, 9, NULL));
  expect("ssd_gemm_w8a16_cfg nt 3", ssd_gemm_w8a16_cfg(p, p, p, NULL, p, 1, 48, 128, 48, SSD_EPI_ROWS, 3, 1, NULL));
  expect("ssd_gemm_w8a16_cfg silu odd nt", ssd_gemm_w8a16_cfg(p, p, p, NULL, p, 1, 64, 128, 0, SSD_EPI_SILU_FRAG, 1, 1, NULL));
  expect("ssd_gemm_w8a16_cfg deep at M = 64", ssd_gemm_w8a16_cfg(p, p, p, NULL, p, 64, 32, 128, 32, SSD_EPI_ROWS, 2 | 256, 1, NULL));
  printf("%d failures\n", failures);
  return failures != 0;
}
