/* Plain-C consumer of include/ssd_hip_filter.h (tests/test_filter_cpu.py builds it with cc -std=c99 -Wall -Werror and links
 * libssdhip.so): ssd_filter_rows called with zero or negative sizes, ld < V, a vocabulary above SSD_FILTER_MAX_V or null required
 * pointers must return SSD_ERR_SHAPE or SSD_ERR_ARG from its argument validation, before any launch (no GPU is needed for that). */
#include <stdio.h>
#include "ssd_hip_filter.h"

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
  const int32_t* k = (const int32_t*)buf;
  int32_t* kept = (int32_t*)buf;
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION) {
    printf("FAIL abi version %d != %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  if (SSD_FILTER_MAX_V < 196608) {
    printf("FAIL SSD_FILTER_MAX_V %d is below the split fork's 196608\n", SSD_FILTER_MAX_V);
    ++failures;
  }
  expect("ssd_filter_rows zero T", ssd_filter_rows(p, 16, 0, 16, f, k, f, f, 1, kept, NULL), SSD_ERR_SHAPE);
  expect("ssd_filter_rows negative T", ssd_filter_rows(p, 16, -1, 16, f, k, f, f, 1, kept, NULL), SSD_ERR_SHAPE);
  expect("ssd_filter_rows zero V", ssd_filter_rows(p, 16, 1, 0, f, k, f, f, 1, kept, NULL), SSD_ERR_SHAPE);
  expect("ssd_filter_rows zero rows_per_param", ssd_filter_rows(p, 16, 1, 16, f, k, f, f, 0, kept, NULL), SSD_ERR_SHAPE);
  expect("ssd_filter_rows ld below V", ssd_filter_rows(p, 8, 1, 16, f, k, f, f, 1, kept, NULL), SSD_ERR_SHAPE);
  expect("ssd_filter_rows V above SSD_FILTER_MAX_V", ssd_filter_rows(p, SSD_FILTER_MAX_V + 8, 1, SSD_FILTER_MAX_V + 8, f, k, f, f, 1,
                                                                      kept, NULL), SSD_ERR_SHAPE);
  expect("ssd_filter_rows null rows", ssd_filter_rows(NULL, 16, 1, 16, f, k, f, f, 1, kept, NULL), SSD_ERR_ARG);
  expect("ssd_filter_rows null temps", ssd_filter_rows(p, 16, 1, 16, NULL, k, f, f, 1, kept, NULL), SSD_ERR_ARG);
  expect("ssd_filter_rows null top_k", ssd_filter_rows(p, 16, 1, 16, f, NULL, f, f, 1, kept, NULL), SSD_ERR_ARG);
  expect("ssd_filter_rows null top_p", ssd_filter_rows(p, 16, 1, 16, f, k, NULL, f, 1, kept, NULL), SSD_ERR_ARG);
  expect("ssd_filter_rows null min_p", ssd_filter_rows(p, 16, 1, 16, f, k, f, NULL, 1, kept, NULL), SSD_ERR_ARG);
  printf("%d failures\n", failures);
  return failures != 0;
}
