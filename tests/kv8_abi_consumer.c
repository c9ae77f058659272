/* Plain-C consumer of include/ssd_hip_kv8.h (tests/test_kv8_cpu.py builds it with cc -std=c99 -Wall -Werror and links libssdhip.so):
 * every FP8 KV cache entry point called with null pointers, head_dim 256, the tree mode or key splits without workspaces must return
 * SSD_ERR_SHAPE or SSD_ERR_ARG from its argument validation, before any launch (no GPU is needed for that). */
#include <stdio.h>
#include "ssd_hip_kv8.h"

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
  const int64_t* l = (const int64_t*)buf;
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION) {
    printf("FAIL abi version %d != %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  expect("ssd_rope_store_kv_fp8 null rows", ssd_rope_store_kv_fp8(NULL, l, f, m, p, p, p, f, f, NULL, NULL, 0.f, 1, 4, 2, 64, 16, 0, NULL));
  expect("ssd_rope_store_kv_fp8 null positions", ssd_rope_store_kv_fp8(p, NULL, f, m, p, p, p, f, f, NULL, NULL, 0.f, 1, 4, 2, 64, 16, 0, NULL));
  expect("ssd_rope_store_kv_fp8 null q_out", ssd_rope_store_kv_fp8(p, l, f, m, NULL, p, p, f, f, NULL, NULL, 0.f, 1, 4, 2, 64, 16, 0, NULL));
  expect("ssd_rope_store_kv_fp8 null k cache", ssd_rope_store_kv_fp8(p, l, f, m, p, NULL, p, f, f, NULL, NULL, 0.f, 1, 4, 2, 64, 16, 0, NULL));
  expect("ssd_rope_store_kv_fp8 null v cache", ssd_rope_store_kv_fp8(p, l, f, m, p, p, NULL, f, f, NULL, NULL, 0.f, 1, 4, 2, 64, 16, 0, NULL));
  expect("ssd_rope_store_kv_fp8 hd 256", ssd_rope_store_kv_fp8(p, l, f, m, p, p, p, f, f, NULL, NULL, 0.f, 1, 4, 2, 256, 16, 0, NULL));
  expect("ssd_rope_store_kv_fp8 zero T", ssd_rope_store_kv_fp8(p, l, f, m, p, p, p, f, f, NULL, NULL, 0.f, 0, 4, 2, 64, 16, 0, NULL));
  expect("ssd_attn_paged_fp8 null q", ssd_attn_paged_fp8(NULL, p, p, f, f, m, 1, m, NULL, 1, 1, 1, 1, 4, 2, 64, 16, 0.125f, 0, 0, 0, 0, 1, NULL,
                                                         1, 0, NULL, NULL, p, NULL, NULL));
  expect("ssd_attn_paged_fp8 null k cache", ssd_attn_paged_fp8(p, NULL, p, f, f, m, 1, m, NULL, 1, 1, 1, 1, 4, 2, 64, 16, 0.125f, 0, 0, 0, 0, 1,
                                                               NULL, 1, 0, NULL, NULL, p, NULL, NULL));
  expect("ssd_attn_paged_fp8 null tables", ssd_attn_paged_fp8(p, p, p, f, f, NULL, 1, m, NULL, 1, 1, 1, 1, 4, 2, 64, 16, 0.125f, 0, 0, 0, 0, 1,
                                                              NULL, 1, 0, NULL, NULL, p, NULL, NULL));
  expect("ssd_attn_paged_fp8 no output", ssd_attn_paged_fp8(p, p, p, f, f, m, 1, m, NULL, 1, 1, 1, 1, 4, 2, 64, 16, 0.125f, 0, 0, 0, 0, 1, NULL,
                                                            1, 0, NULL, NULL, NULL, NULL, NULL));
  expect("ssd_attn_paged_fp8 hd 256", ssd_attn_paged_fp8(p, p, p, f, f, m, 1, m, NULL, 1, 1, 1, 1, 4, 2, 256, 16, 0.0625f, 0, 0, 0, 0, 1, NULL,
                                                         1, 0, NULL, NULL, p, NULL, NULL));
  expect("ssd_attn_paged_fp8 mode 1", ssd_attn_paged_fp8(p, p, p, f, f, m, 1, m, NULL, 1, 1, 1, 1, 4, 2, 64, 16, 0.125f, 1, 3, 6, 0, 2, NULL, 1, 0,
                                                         NULL, NULL, p, NULL, NULL));
  expect("ssd_attn_paged_fp8 splits without workspaces", ssd_attn_paged_fp8(p, p, p, f, f, m, 1, m, NULL, 1, 1, 1, 1, 4, 2, 64, 16, 0.125f, 0, 0, 0,
                                                                            0, 1, NULL, 2, 0, NULL, NULL, p, NULL, NULL));
  expect("ssd_attn_paged_fp8 block size 24", ssd_attn_paged_fp8(p, p, p, f, f, m, 1, m, NULL, 1, 1, 1, 1, 4, 2, 64, 24, 0.125f, 0, 0, 0, 0, 1, NULL,
                                                                1, 0, NULL, NULL, p, NULL, NULL));
  expect("ssd_attn_prefill_varlen_fp8 null cu_q", ssd_attn_prefill_varlen_fp8(p, p, p, f, f, m, 1, m, NULL, 1, 1, 1, 4, 2, 64, 16, 0.125f, p, NULL,
                                                                              NULL));
  expect("ssd_attn_prefill_varlen_fp8 null v cache", ssd_attn_prefill_varlen_fp8(p, p, NULL, f, f, m, 1, m, m, 1, 1, 1, 4, 2, 64, 16, 0.125f, p,
                                                                                 NULL, NULL));
  expect("ssd_attn_prefill_varlen_fp8 hd 256", ssd_attn_prefill_varlen_fp8(p, p, p, f, f, m, 1, m, m, 1, 1, 1, 4, 2, 256, 16, 0.0625f, p, NULL,
                                                                           NULL));
  expect("ssd_kv_fp8_dequant null codes", ssd_kv_fp8_dequant(NULL, f, p, 1, 2, 16, 64, NULL));
  expect("ssd_kv_fp8_dequant null dst", ssd_kv_fp8_dequant(p, f, NULL, 1, 2, 16, 64, NULL));
  expect("ssd_kv_fp8_dequant hd 256", ssd_kv_fp8_dequant(p, f, p, 1, 2, 16, 256, NULL));
  expect("ssd_kv_fp8_dequant zero pages", ssd_kv_fp8_dequant(p, f, p, 0, 2, 16, 64, NULL));
  printf("%d failures\n", failures);
  return failures != 0;
}
