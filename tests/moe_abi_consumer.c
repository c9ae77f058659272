/* Plain-C consumer of include/ssd_hip_moe.h (tests/test_moe_cpu.py builds it with cc -std=c99 -Wall -Werror and links libssdhip.so):
 * every mixture-of-experts entry point called with a null pointer, an unknown epilogue or a shape outside the header's list must
 * return SSD_ERR_ARG or SSD_ERR_SHAPE from its argument validation, before any launch (no GPU is needed for that). */
#include <stdio.h>
#include "ssd_hip_moe.h"

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
  float* f = (float*)buf;
  int32_t* m = (int32_t*)buf;
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION) {
    printf("FAIL abi version %d != %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  expect("ssd_moe_route null logits", ssd_moe_route(NULL, 8, 1, 8, 2, 1, m, f, m, m, NULL), SSD_ERR_ARG);
  expect("ssd_moe_route null topk_ids", ssd_moe_route(p, 8, 1, 8, 2, 1, NULL, f, m, m, NULL), SSD_ERR_ARG);
  expect("ssd_moe_route null topk_w", ssd_moe_route(p, 8, 1, 8, 2, 1, m, NULL, m, m, NULL), SSD_ERR_ARG);
  expect("ssd_moe_route null offs", ssd_moe_route(p, 8, 1, 8, 2, 1, m, f, NULL, m, NULL), SSD_ERR_ARG);
  expect("ssd_moe_route null perm", ssd_moe_route(p, 8, 1, 8, 2, 1, m, f, m, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_moe_route zero T", ssd_moe_route(p, 8, 0, 8, 2, 1, m, f, m, m, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_route k 0", ssd_moe_route(p, 8, 1, 8, 0, 1, m, f, m, m, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_route k 9", ssd_moe_route(p, 16, 1, 16, SSD_MOE_MAX_K + 1, 1, m, f, m, m, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_route E 4", ssd_moe_route(p, 4, 1, SSD_MOE_MIN_E - 4, 2, 1, m, f, m, m, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_route E 12", ssd_moe_route(p, 12, 1, 12, 2, 1, m, f, m, m, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_route E 264", ssd_moe_route(p, 264, 1, SSD_MOE_MAX_E + 8, 2, 1, m, f, m, m, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_route ld below E", ssd_moe_route(p, 7, 1, 8, 2, 1, m, f, m, m, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_route T k above 2^24", ssd_moe_route(p, 8, (1 << 24) / 2 + 1, 8, 2, 1, m, f, m, m, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_gemm null rows", ssd_moe_gemm(NULL, p, m, m, p, 1, 2, 8, 64, 64, SSD_MOE_EPI_UP, NULL), SSD_ERR_ARG);
  expect("ssd_moe_gemm null tables", ssd_moe_gemm(p, NULL, m, m, p, 1, 2, 8, 64, 64, SSD_MOE_EPI_UP, NULL), SSD_ERR_ARG);
  expect("ssd_moe_gemm null offs", ssd_moe_gemm(p, p, NULL, m, p, 1, 2, 8, 64, 64, SSD_MOE_EPI_UP, NULL), SSD_ERR_ARG);
  expect("ssd_moe_gemm null perm", ssd_moe_gemm(p, p, m, NULL, p, 1, 2, 8, 64, 64, SSD_MOE_EPI_UP, NULL), SSD_ERR_ARG);
  expect("ssd_moe_gemm null out", ssd_moe_gemm(p, p, m, m, NULL, 1, 2, 8, 64, 64, SSD_MOE_EPI_UP, NULL), SSD_ERR_ARG);
  expect("ssd_moe_gemm epilogue 2", ssd_moe_gemm(p, p, m, m, p, 1, 2, 8, 64, 64, 2, NULL), SSD_ERR_ARG);
  expect("ssd_moe_gemm zero T", ssd_moe_gemm(p, p, m, m, p, 0, 2, 8, 64, 64, SSD_MOE_EPI_UP, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_gemm k above E", ssd_moe_gemm(p, p, m, m, p, 1, 9, 8, 64, 64, SSD_MOE_EPI_UP, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_gemm E 20", ssd_moe_gemm(p, p, m, m, p, 1, 2, 20, 64, 64, SSD_MOE_EPI_UP, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_gemm K 48", ssd_moe_gemm(p, p, m, m, p, 1, 2, 8, 64, 48, SSD_MOE_EPI_UP, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_gemm up N 96", ssd_moe_gemm(p, p, m, m, p, 1, 2, 8, 96, 64, SSD_MOE_EPI_UP, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_gemm down N 24", ssd_moe_gemm(p, p, m, m, p, 1, 2, 8, 24, 64, SSD_MOE_EPI_DOWN, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_combine null d", ssd_moe_combine(NULL, f, p, 1, 2, 64, NULL), SSD_ERR_ARG);
  expect("ssd_moe_combine null topk_w", ssd_moe_combine(p, NULL, p, 1, 2, 64, NULL), SSD_ERR_ARG);
  expect("ssd_moe_combine null h", ssd_moe_combine(p, f, NULL, 1, 2, 64, NULL), SSD_ERR_ARG);
  expect("ssd_moe_combine zero T", ssd_moe_combine(p, f, p, 0, 2, 64, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_combine k 9", ssd_moe_combine(p, f, p, 1, 9, 64, NULL), SSD_ERR_SHAPE);
  expect("ssd_moe_combine H 24", ssd_moe_combine(p, f, p, 1, 2, 24, NULL), SSD_ERR_SHAPE);
  printf("%d failures\n", failures);
  return failures != 0;
}
