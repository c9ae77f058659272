/* Plain-C consumer of include/ssd_hip_swa.h (tests/test_swa_cpu.py builds it with cc -std=c99 -Wall -Werror and links libssdhip.so):
 * both sliding-window entry points called with a negative window, a window in the tree mode, null pointers, head_dim 256 or key
 * splits without workspaces must return SSD_ERR_SHAPE or SSD_ERR_ARG from their argument validation, before any launch (no GPU is
 * needed for that); window 0 forwards, so the unwindowed entry's refusals come back through it. */
#include <stdio.h>
#include "ssd_hip_swa.h"

static int failures = 0;

static void expect(const char* what, int rc, int want) {
  if (rc != want) {
    printf("FAIL %s returned %d, not %d\n", what, rc, want);
    ++failures;
  } else {
    printf("ok   %s -> %d\n", what, rc);
  }
}

#define BF16(q, k, hd, mode, splits, window) \
  ssd_attn_paged_window(q, k, p, m, 1, m, NULL, 1, 1, 1, 1, 4, 2, hd, 16, 0.125f, mode, 0, 1, 0, 1, NULL, splits, 0, NULL, NULL, p, NULL, window, NULL)
#define FP8(q, k, hd, mode, splits, window) \
  ssd_attn_paged_fp8_window(q, k, p, f, f, m, 1, m, NULL, 1, 1, 1, 1, 4, 2, hd, 16, 0.125f, mode, 0, 1, 0, 1, NULL, splits, 0, NULL, NULL, p, NULL, window, NULL)

int main(void) {
  char buf[64];
  void* p = buf;
  const float* f = (const float*)buf;
  const int32_t* m = (const int32_t*)buf;
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION) {
    printf("FAIL abi version %d != %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  expect("ssd_attn_paged_window window -1", BF16(p, p, 64, 0, 1, -1), SSD_ERR_ARG);
  expect("ssd_attn_paged_window mode 1 with a window", BF16(p, p, 64, 1, 1, 8), SSD_ERR_ARG);
  expect("ssd_attn_paged_window null q", BF16(NULL, p, 64, 0, 1, 8), SSD_ERR_ARG);
  expect("ssd_attn_paged_window null k cache", BF16(p, NULL, 64, 0, 1, 8), SSD_ERR_ARG);
  expect("ssd_attn_paged_window hd 256", BF16(p, p, 256, 0, 1, 8), SSD_ERR_SHAPE);
  expect("ssd_attn_paged_window splits without workspaces", BF16(p, p, 64, 0, 2, 8), SSD_ERR_ARG);
  expect("ssd_attn_paged_window window 0 forwards: hd 256", BF16(p, p, 256, 0, 1, 0), SSD_ERR_SHAPE);
  expect("ssd_attn_paged_fp8_window window -1", FP8(p, p, 64, 0, 1, -1), SSD_ERR_ARG);
  expect("ssd_attn_paged_fp8_window mode 1 with a window", FP8(p, p, 64, 1, 1, 8), SSD_ERR_ARG);
  expect("ssd_attn_paged_fp8_window null q", FP8(NULL, p, 64, 0, 1, 8), SSD_ERR_ARG);
  expect("ssd_attn_paged_fp8_window null k cache", FP8(p, NULL, 64, 0, 1, 8), SSD_ERR_ARG);
  expect("ssd_attn_paged_fp8_window hd 256", FP8(p, p, 256, 0, 1, 8), SSD_ERR_SHAPE);
  expect("ssd_attn_paged_fp8_window splits without workspaces", FP8(p, p, 64, 0, 2, 8), SSD_ERR_ARG);
  expect("ssd_attn_paged_fp8_window window 0 forwards: mode 1", FP8(p, p, 64, 1, 1, 0), SSD_ERR_ARG);
  printf("%d failures\n", failures);
  return failures != 0;
}
