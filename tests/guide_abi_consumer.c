/* Plain-C consumer of include/ssd_hip_guide.h (tests/test_guide_cpu.py builds it with cc -std=c99 -Wall -Werror and links
 * libssdhip.so): ssd_guide_walk and ssd_guide_rows called with zero or negative sizes, ld < V, strides below 1, a bad extra geometry,
 * a null pointer or a table given in part must return SSD_ERR_SHAPE or SSD_ERR_ARG from their argument validation, before any launch
 * (no GPU is needed for that). */
#include <stdio.h>
#include "ssd_hip_guide.h"

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
  int32_t* w = (int32_t*)buf;
  const int32_t* i = (const int32_t*)buf;
  const int64_t* e = (const int64_t*)buf;
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION) {
    printf("FAIL abi version %d != %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  if (SSD_GUIDE_MAX_STATES != 16384 || SSD_GUIDE_MAX_EDGES != 262144 || SSD_GUIDE_MAX_EXTRA < 16 ||
      SSD_GUIDE_SLICE != 4096) {
    printf("FAIL the limits of ssd_hip_guide.h moved\n");
    ++failures;
  }
#define TAB i, i, i, i, i, 4, 8
  expect("ssd_guide_walk zero T", ssd_guide_walk(w, 0, 1, i, i, TAB, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_walk negative T", ssd_guide_walk(w, -1, 1, i, i, TAB, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_walk T above 65535", ssd_guide_walk(w, 65536, 1, i, i, TAB, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_walk zero rows_per_seq", ssd_guide_walk(w, 1, 0, i, i, TAB, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_walk zero states_ld", ssd_guide_walk(w, 1, 1, i, i, i, i, i, i, i, 0, 8, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_walk zero edges_ld", ssd_guide_walk(w, 1, 1, i, i, i, i, i, i, i, 4, 0, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_walk edges_ld above SSD_GUIDE_MAX_EDGES",
         ssd_guide_walk(w, 1, 1, i, i, i, i, i, i, i, 4, SSD_GUIDE_MAX_EDGES + 1, NULL, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_walk zero extra_ld", ssd_guide_walk(w, 1, 1, i, i, TAB, e, 0, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_walk extra_ld above SSD_GUIDE_MAX_EXTRA + 1", ssd_guide_walk(w, 1, 1, i, i, TAB, e, SSD_GUIDE_MAX_EXTRA + 2, i, NULL),
         SSD_ERR_SHAPE);
  expect("ssd_guide_walk prefix form with extra_ld below rows_per_seq", ssd_guide_walk(w, 4, 4, i, i, TAB, e, 3, NULL, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_walk null state_rows", ssd_guide_walk(NULL, 1, 1, i, i, TAB, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_guide_walk null guide_on", ssd_guide_walk(w, 1, 1, NULL, i, TAB, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_guide_walk null state0", ssd_guide_walk(w, 1, 1, i, NULL, TAB, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_guide_walk tables without n_states", ssd_guide_walk(w, 1, 1, i, i, NULL, i, i, i, i, 4, 8, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_guide_walk tables without edge_off", ssd_guide_walk(w, 1, 1, i, i, i, NULL, i, i, i, 4, 8, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_guide_walk tables without dflt", ssd_guide_walk(w, 1, 1, i, i, i, i, NULL, i, i, 4, 8, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_guide_walk tables without edge_tok", ssd_guide_walk(w, 1, 1, i, i, i, i, i, NULL, i, 4, 8, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_guide_walk tables without edge_next", ssd_guide_walk(w, 1, 1, i, i, i, i, i, i, NULL, 4, 8, NULL, 0, NULL, NULL), SSD_ERR_ARG);
  expect("ssd_guide_walk extra_n without extra", ssd_guide_walk(w, 1, 1, i, i, TAB, NULL, 0, i, NULL), SSD_ERR_ARG);

  expect("ssd_guide_rows zero T", ssd_guide_rows(p, 16, 0, 16, i, 1, TAB, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_rows T above 65535", ssd_guide_rows(p, 16, 65536, 16, i, 1, TAB, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_rows zero V", ssd_guide_rows(p, 16, 1, 0, i, 1, TAB, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_rows zero rows_per_seq", ssd_guide_rows(p, 16, 1, 16, i, 0, TAB, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_rows ld below V", ssd_guide_rows(p, 8, 1, 16, i, 1, TAB, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_rows zero states_ld", ssd_guide_rows(p, 16, 1, 16, i, 1, i, i, i, i, i, 0, 8, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_rows zero edges_ld", ssd_guide_rows(p, 16, 1, 16, i, 1, i, i, i, i, i, 4, 0, NULL), SSD_ERR_SHAPE);
  expect("ssd_guide_rows null rows", ssd_guide_rows(NULL, 16, 1, 16, i, 1, TAB, NULL), SSD_ERR_ARG);
  expect("ssd_guide_rows null state_rows", ssd_guide_rows(p, 16, 1, 16, NULL, 1, TAB, NULL), SSD_ERR_ARG);
  expect("ssd_guide_rows tables without n_states", ssd_guide_rows(p, 16, 1, 16, i, 1, NULL, i, i, i, i, 4, 8, NULL), SSD_ERR_ARG);
  expect("ssd_guide_rows tables without edge_off", ssd_guide_rows(p, 16, 1, 16, i, 1, i, NULL, i, i, i, 4, 8, NULL), SSD_ERR_ARG);
  expect("ssd_guide_rows tables without dflt", ssd_guide_rows(p, 16, 1, 16, i, 1, i, i, NULL, i, i, 4, 8, NULL), SSD_ERR_ARG);
  expect("ssd_guide_rows tables without edge_tok", ssd_guide_rows(p, 16, 1, 16, i, 1, i, i, i, NULL, i, 4, 8, NULL), SSD_ERR_ARG);
  expect("ssd_guide_rows tables without edge_next", ssd_guide_rows(p, 16, 1, 16, i, 1, i, i, i, i, NULL, 4, 8, NULL), SSD_ERR_ARG);
  printf("%d failures\n", failures);
  return failures != 0;
}
