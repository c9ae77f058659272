/* Plain-C consumer of include/ssd_hip_penalty.h (tests/test_penalty_cpu.py builds it with cc -std=c99 -Wall -Werror and links
 * libssdhip.so): ssd_penalize_rows called with zero or negative sizes, ld < V, a bad table or extra geometry or null required
 * pointers must return SSD_ERR_SHAPE or SSD_ERR_ARG from its argument validation, before any launch (no GPU is needed for that). */
#include <stdio.h>
#include "ssd_hip_penalty.h"

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
  const float* f = (const float*)buf;
  const int32_t* i = (const int32_t*)buf;
  const int64_t* e = (const int64_t*)buf;
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION) {
    printf("FAIL abi version %d != %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  if (SSD_PENALTY_MAX_EXTRA < 16) {
    printf("FAIL SSD_PENALTY_MAX_EXTRA %d is below a 16-token lookahead\n", SSD_PENALTY_MAX_EXTRA);
    ++failures;
  }
  expect("ssd_penalize_rows zero T", ssd_penalize_rows(p, 16, 0, 16, 1, i, i, f, 4, i, f, f, f, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_penalize_rows negative T", ssd_penalize_rows(p, 16, -1, 16, 1, i, i, f, 4, i, f, f, f, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_penalize_rows zero V", ssd_penalize_rows(p, 16, 1, 0, 1, i, i, f, 4, i, f, f, f, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_penalize_rows zero rows_per_seq", ssd_penalize_rows(p, 16, 1, 16, 0, i, i, f, 4, i, f, f, f, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_penalize_rows ld below V", ssd_penalize_rows(p, 8, 1, 16, 1, i, i, f, 4, i, f, f, f, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_penalize_rows zero tab_ld", ssd_penalize_rows(p, 16, 1, 16, 1, i, i, f, 0, i, f, f, f, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_penalize_rows zero extra_ld", ssd_penalize_rows(p, 16, 1, 16, 1, i, i, f, 4, i, f, f, f, e, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_penalize_rows extra_ld above SSD_PENALTY_MAX_EXTRA + 1",
         ssd_penalize_rows(p, 16, 1, 16, 1, i, i, f, 4, i, f, f, f, e, SSD_PENALTY_MAX_EXTRA + 2, i, NULL), SSD_ERR_SHAPE);
  expect("ssd_penalize_rows prefix form with extra_ld below rows_per_seq",
         ssd_penalize_rows(p, 16, 4, 16, 4, i, i, f, 4, i, f, f, f, e, 3, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_penalize_rows null rows", ssd_penalize_rows(NULL, 16, 1, 16, 1, i, i, f, 4, i, f, f, f, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_penalize_rows null rep", ssd_penalize_rows(p, 16, 1, 16, 1, i, i, f, 4, i, NULL, f, f, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_penalize_rows null pres", ssd_penalize_rows(p, 16, 1, 16, 1, i, i, f, 4, i, f, NULL, f, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_penalize_rows null freq", ssd_penalize_rows(p, 16, 1, 16, 1, i, i, f, 4, i, f, f, NULL, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_penalize_rows table without tab_len", ssd_penalize_rows(p, 16, 1, 16, 1, i, i, f, 4, NULL, f, f, f, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_penalize_rows table without tab_bias", ssd_penalize_rows(p, 16, 1, 16, 1, i, i, NULL, 4, i, f, f, f, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_penalize_rows extra_n without extra", ssd_penalize_rows(p, 16, 1, 16, 1, i, i, f, 4, i, f, f, f, NULL, 0, i, NULL), SSD_ERR_ARG);
  printf("%d failures\n", failures);
  return failures != 0;
}
