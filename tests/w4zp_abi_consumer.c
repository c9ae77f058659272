/* Plain-C consumer of include/ssd_hip_w4zp.h (tests/test_w4zp_cpu.py builds it with cc -std=c99 -Wall -Werror and links
 * libssdhip.so): every zero-point W4A16 entry point called with null pointers or zero / misaligned sizes must return SSD_ERR_SHAPE or
 * SSD_ERR_ARG from its argument validation, before any launch (no GPU is needed for that). */
#include <stdio.h>
#include "ssd_hip_w4zp.h"

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
  expect("ssd_w4zp_rows_to_frag zero N", ssd_w4zp_rows_to_frag(p, p, p, p, p, p, m, 0, 128, NULL));
  expect("ssd_w4zp_rows_to_frag K % 128", ssd_w4zp_rows_to_frag(p, p, p, p, p, p, m, 16, 64, NULL));
  expect("ssd_w4zp_rows_to_frag N % 16", ssd_w4zp_rows_to_frag(p, p, p, p, p, p, m, 8, 128, NULL));
  expect("ssd_w4zp_rows_to_frag null codes", ssd_w4zp_rows_to_frag(NULL, p, p, p, p, p, NULL, 16, 128, NULL));
  expect("ssd_w4zp_rows_to_frag null scales", ssd_w4zp_rows_to_frag(p, NULL, p, p, p, p, NULL, 16, 128, NULL));
  expect("ssd_w4zp_rows_to_frag null zeros", ssd_w4zp_rows_to_frag(p, p, NULL, p, p, p, NULL, 16, 128, NULL));
  expect("ssd_w4zp_rows_to_frag null frag", ssd_w4zp_rows_to_frag(p, p, p, NULL, p, p, NULL, 16, 128, NULL));
  expect("ssd_w4zp_rows_to_frag null scale frag", ssd_w4zp_rows_to_frag(p, p, p, p, NULL, p, NULL, 16, 128, NULL));
  expect("ssd_w4zp_rows_to_frag null zero frag", ssd_w4zp_rows_to_frag(p, p, p, p, p, NULL, NULL, 16, 128, NULL));
  expect("ssd_w4zp_frag_to_rows zero K", ssd_w4zp_frag_to_rows(p, p, p, p, p, p, 16, 0, NULL));
  expect("ssd_w4zp_frag_to_rows K % 128", ssd_w4zp_frag_to_rows(p, p, p, p, p, p, 16, 192, NULL));
  expect("ssd_w4zp_frag_to_rows null frags", ssd_w4zp_frag_to_rows(NULL, NULL, NULL, p, p, p, 16, 128, NULL));
  expect("ssd_w4zp_frag_to_rows null zero frag", ssd_w4zp_frag_to_rows(p, p, NULL, p, p, p, 16, 128, NULL));
  expect("ssd_w4zp_frag_to_rows null rows", ssd_w4zp_frag_to_rows(p, p, p, NULL, p, p, 16, 128, NULL));
  expect("ssd_w4zp_frag_to_rows null zero rows", ssd_w4zp_frag_to_rows(p, p, p, p, p, NULL, 16, 128, NULL));
  expect("ssd_w4zp_dequant_frag zero N", ssd_w4zp_dequant_frag(p, p, p, p, 0, 128, NULL));
  expect("ssd_w4zp_dequant_frag K % 128", ssd_w4zp_dequant_frag(p, p, p, p, 16, 96, NULL));
  expect("ssd_w4zp_dequant_frag null scales", ssd_w4zp_dequant_frag(p, NULL, p, p, 16, 128, NULL));
  expect("ssd_w4zp_dequant_frag null zeros", ssd_w4zp_dequant_frag(p, p, NULL, p, 16, 128, NULL));
  expect("ssd_w4zp_dequant_frag null dst", ssd_w4zp_dequant_frag(p, p, p, NULL, 16, 128, NULL));
  expect("ssd_gemm_w4a16_zp zero M", ssd_gemm_w4a16_zp(p, p, p, p, NULL, p, 0, 16, 128, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_w4a16_zp M > 128", ssd_gemm_w4a16_zp(p, p, p, p, NULL, p, 129, 16, 128, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_w4a16_zp K % 128", ssd_gemm_w4a16_zp(p, p, p, p, NULL, p, 1, 16, 64, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_w4a16_zp N % 16", ssd_gemm_w4a16_zp(p, p, p, p, NULL, p, 1, 24, 128, 24, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_w4a16_zp null x", ssd_gemm_w4a16_zp(NULL, p, p, p, NULL, p, 1, 16, 128, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_w4a16_zp null scales", ssd_gemm_w4a16_zp(p, p, NULL, p, NULL, p, 1, 16, 128, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_w4a16_zp null zeros", ssd_gemm_w4a16_zp(p, p, p, NULL, NULL, p, 1, 16, 128, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_w4a16_zp null y", ssd_gemm_w4a16_zp(p, p, p, p, NULL, NULL, 1, 16, 128, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_w4a16_zp ldy < N", ssd_gemm_w4a16_zp(p, p, p, p, NULL, p, 1, 32, 128, 16, SSD_EPI_ROWS, NULL));
  expect("ssd_gemm_w4a16_zp bad epilogue", ssd_gemm_w4a16_zp(p, p, p, p, NULL, p, 1, 64, 128, 64, 7, NULL));
  expect("ssd_gemm_w4a16_zp_cfg zero N", ssd_gemm_w4a16_zp_cfg(p, p, p, p, NULL, p, 1, 0, 128, 16, SSD_EPI_ROWS, 1, 1, NULL));
  expect("ssd_gemm_w4a16_zp_cfg null q", ssd_gemm_w4a16_zp_cfg(p, NULL, p, p, NULL, p, 1, 16, 128, 16, SSD_EPI_ROWS, 1, 1, NULL));
  expect("ssd_gemm_w4a16_zp_cfg null zeros", ssd_gemm_w4a16_zp_cfg(p, p, p, NULL, NULL, p, 1, 16, 128, 16, SSD_EPI_ROWS, 1, 1, NULL));
  expect("ssd_gemm_w4a16_zp_cfg waves 0", ssd_gemm_w4a16_zp_cfg(p, p, p, p, NULL, p, 1, 16, 128, 16, SSD_EPI_ROWS, 1, 0, NULL));
  expect("ssd_gemm_w4a16_zp_cfg waves 9", ssd_gemm_w4a16_zp_cfg(p, p, p, p, NULL, p, 1, 16, 128, 16, SSD_EPI_ROWS, 1, 9, NULL));
  expect("ssd_gemm_w4a16_zp_cfg nt 3", ssd_gemm_w4a16_zp_cfg(p, p, p, p, NULL, p, 1, 48, 128, 48, SSD_EPI_ROWS, 3, 1, NULL));
  expect("ssd_gemm_w4a16_zp_cfg nt not dividing", ssd_gemm_w4a16_zp_cfg(p, p, p, p, NULL, p, 1, 48, 128, 48, SSD_EPI_ROWS, 2, 1, NULL));
  expect("ssd_gemm_w4a16_zp_cfg silu odd nt", ssd_gemm_w4a16_zp_cfg(p, p, p, p, NULL, p, 1, 64, 128, 0, SSD_EPI_SILU_FRAG, 1, 1, NULL));
  expect("ssd_gemm_w4a16_zp_cfg silu N % 64", ssd_gemm_w4a16_zp_cfg(p, p, p, p, NULL, p, 1, 32, 128, 0, SSD_EPI_SILU_FRAG, 2, 1, NULL));
  expect("ssd_gemm_w4a16_zp_cfg deep at M = 64", ssd_gemm_w4a16_zp_cfg(p, p, p, p, NULL, p, 64, 32, 128, 32, SSD_EPI_ROWS, 2 | 256, 1, NULL));
  printf("%d failures\n", failures);
  return failures != 0;
}
