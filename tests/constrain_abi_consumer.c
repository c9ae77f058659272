/* Plain-C consumer of include/ssd_hip_constrain.h (tests/test_constrain_cpu.py builds it with cc -std=c99 -Wall -Werror and links
 * libssdhip.so): ssd_constrain_rows called with zero or negative sizes, ld < V, a bad tail or extra geometry, a null row pointer or a
 * group given in part must return SSD_ERR_SHAPE or SSD_ERR_ARG from its argument validation, before any launch (no GPU is needed
 * for that). */
#include <stdio.h>
#include "ssd_hip_constrain.h"

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
  const int32_t* i = (const int32_t*)buf;
  const uint32_t* u = (const uint32_t*)buf;
  const int64_t* e = (const int64_t*)buf;
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION) {
    printf("FAIL abi version %d != %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  if (SSD_CONSTRAIN_MAX_EXTRA < 16 || SSD_CONSTRAIN_MAX_STOP != 64 || SSD_CONSTRAIN_MAX_WORDS != 128 ||
      SSD_CONSTRAIN_MAX_WORD_TOKENS != 1024 || SSD_CONSTRAIN_MAX_WORD_LEN != 16 || SSD_CONSTRAIN_SLICE != 4096) {
    printf("FAIL the limits of ssd_hip_constrain.h moved\n");
    ++failures;
  }
#define ALL i, u, i, i, i, i, i, i, i, 15, i
  expect("ssd_constrain_rows zero T", ssd_constrain_rows(p, 16, 0, 16, 1, ALL, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_constrain_rows negative T", ssd_constrain_rows(p, 16, -1, 16, 1, ALL, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_constrain_rows T above 65535", ssd_constrain_rows(p, 16, 65536, 16, 1, ALL, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_constrain_rows zero V", ssd_constrain_rows(p, 16, 1, 0, 1, ALL, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_constrain_rows zero rows_per_seq", ssd_constrain_rows(p, 16, 1, 16, 0, ALL, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_constrain_rows ld below V", ssd_constrain_rows(p, 8, 1, 16, 1, ALL, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_constrain_rows zero tail_ld", ssd_constrain_rows(p, 16, 1, 16, 1, i, u, i, i, i, i, i, i, i, 0, i, NULL, 0, NULL, NULL),
         SSD_ERR_SHAPE);
  expect("ssd_constrain_rows tail_ld above SSD_CONSTRAIN_MAX_WORD_LEN - 1",
         ssd_constrain_rows(p, 16, 1, 16, 1, i, u, i, i, i, i, i, i, i, SSD_CONSTRAIN_MAX_WORD_LEN, i, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_constrain_rows zero extra_ld", ssd_constrain_rows(p, 16, 1, 16, 1, ALL, e, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_constrain_rows extra_ld above SSD_CONSTRAIN_MAX_EXTRA + 1",
         ssd_constrain_rows(p, 16, 1, 16, 1, ALL, e, SSD_CONSTRAIN_MAX_EXTRA + 2, i, NULL), SSD_ERR_SHAPE);
  expect("ssd_constrain_rows prefix form with extra_ld below rows_per_seq", ssd_constrain_rows(p, 16, 4, 16, 4, ALL, e, 3, NULL, NULL),
         SSD_ERR_SHAPE);
  expect("ssd_constrain_rows null rows", ssd_constrain_rows(NULL, 16, 1, 16, 1, ALL, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_constrain_rows allow_on without allow_bits",
         ssd_constrain_rows(p, 16, 1, 16, 1, i, NULL, i, i, i, i, i, i, i, 15, i, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_constrain_rows allow_bits without allow_on",
         ssd_constrain_rows(p, 16, 1, 16, 1, NULL, u, i, i, i, i, i, i, i, 15, i, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_constrain_rows stop list without min_left",
         ssd_constrain_rows(p, 16, 1, 16, 1, i, u, NULL, i, i, i, i, i, i, 15, i, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_constrain_rows stop list without stop_len",
         ssd_constrain_rows(p, 16, 1, 16, 1, i, u, i, i, NULL, i, i, i, i, 15, i, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_constrain_rows bad words without bw_off",
         ssd_constrain_rows(p, 16, 1, 16, 1, i, u, i, i, i, i, NULL, i, i, 15, i, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_constrain_rows bad words without tail",
         ssd_constrain_rows(p, 16, 1, 16, 1, i, u, i, i, i, i, i, i, NULL, 15, i, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_constrain_rows bad words without tail_len",
         ssd_constrain_rows(p, 16, 1, 16, 1, i, u, i, i, i, i, i, i, i, 15, NULL, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_constrain_rows extra_n without extra", ssd_constrain_rows(p, 16, 1, 16, 1, ALL, NULL, 0, i, NULL), SSD_ERR_ARG);
  printf("%d failures\n", failures);
  return failures != 0;
}
