/* Plain-C consumer of include/ssd_hip_logprob.h (tests/test_logprob_cpu.py builds it with cc -std=c99 -Wall -Werror and links
 * libssdhip.so): every entry point called with zero or negative sizes, ld < V, a vocabulary above SSD_LOGPROB_MAX_V, a copy narrower
 * than V or null required pointers must return SSD_ERR_SHAPE or SSD_ERR_ARG from its argument validation, before any launch (no GPU
 * is needed for that); the workspace query answers on the host. */
#include <stdio.h>
#include "ssd_hip_logprob.h"

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
  int32_t* k = (int32_t*)buf;
  int64_t* t = (int64_t*)buf;
  const int big = SSD_LOGPROB_MAX_V + 8;
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION) {
    printf("FAIL abi version %d != %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  if (SSD_LOGPROB_MAX_V < 196608 || SSD_LOGPROB_MAX_N != 20 || SSD_LOGPROB_MAX_V % SSD_LOGPROB_SLICE) {
    printf("FAIL SSD_LOGPROB_MAX_V %d / SSD_LOGPROB_MAX_N %d / SSD_LOGPROB_SLICE %d\n", SSD_LOGPROB_MAX_V, SSD_LOGPROB_MAX_N,
           SSD_LOGPROB_SLICE);
    ++failures;
  }
  /* the workspace query: positive, growing with T and with the number of slices, refusing what ssd_logprob_rows refuses */
  expect("ssd_logprob_rows_ws_bytes zero T", ssd_logprob_rows_ws_bytes(0, 16), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows_ws_bytes zero V", ssd_logprob_rows_ws_bytes(1, 0), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows_ws_bytes V above SSD_LOGPROB_MAX_V", ssd_logprob_rows_ws_bytes(1, big), SSD_ERR_SHAPE);
  {
    const int one = ssd_logprob_rows_ws_bytes(1, 1), slice = ssd_logprob_rows_ws_bytes(1, SSD_LOGPROB_SLICE);
    expect("ssd_logprob_rows_ws_bytes workspace query: one slice up to SSD_LOGPROB_SLICE", one > 0 && one == slice, 1);
    expect("ssd_logprob_rows_ws_bytes workspace query: a second slice", ssd_logprob_rows_ws_bytes(1, SSD_LOGPROB_SLICE + 1), 2 * one);
    expect("ssd_logprob_rows_ws_bytes workspace query: rows", ssd_logprob_rows_ws_bytes(24, SSD_LOGPROB_MAX_V),
           24 * (SSD_LOGPROB_MAX_V / SSD_LOGPROB_SLICE) * one);
  }

  expect("ssd_logprob_rows zero T", ssd_logprob_rows(p, 16, 0, 16, k, 1, f, f, k, NULL, 0, p, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows negative T", ssd_logprob_rows(p, 16, -1, 16, k, 1, f, f, k, NULL, 0, p, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows zero V", ssd_logprob_rows(p, 16, 1, 0, k, 1, f, f, k, NULL, 0, p, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows zero rows_per_param", ssd_logprob_rows(p, 16, 1, 16, k, 0, f, f, k, NULL, 0, p, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows ld below V", ssd_logprob_rows(p, 8, 1, 16, k, 1, f, f, k, NULL, 0, p, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows V above SSD_LOGPROB_MAX_V", ssd_logprob_rows(p, big, 1, big, k, 1, f, f, k, NULL, 0, p, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows raw_ld below V", ssd_logprob_rows(p, 16, 1, 16, k, 1, f, f, k, p, 8, p, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows null rows", ssd_logprob_rows(NULL, 16, 1, 16, k, 1, f, f, k, NULL, 0, p, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_rows null n_top", ssd_logprob_rows(p, 16, 1, 16, NULL, 1, f, f, k, NULL, 0, p, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_rows null lse", ssd_logprob_rows(p, 16, 1, 16, k, 1, NULL, f, k, NULL, 0, p, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_rows null top_val alone", ssd_logprob_rows(p, 16, 1, 16, k, 1, f, NULL, k, NULL, 0, p, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_rows null top_id alone", ssd_logprob_rows(p, 16, 1, 16, k, 1, f, f, NULL, NULL, 0, p, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_rows null ws", ssd_logprob_rows(p, 16, 1, 16, k, 1, f, f, k, NULL, 0, NULL, NULL), SSD_ERR_ARG);

  expect("ssd_logprob_pick zero T", ssd_logprob_pick(p, 16, 0, 16, t, f, k, 1, f, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_pick zero V", ssd_logprob_pick(p, 16, 1, 0, t, f, k, 1, f, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_pick zero rows_per_param", ssd_logprob_pick(p, 16, 1, 16, t, f, k, 0, f, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_pick ld below V", ssd_logprob_pick(p, 8, 1, 16, t, f, k, 1, f, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_pick null rows", ssd_logprob_pick(NULL, 16, 1, 16, t, f, k, 1, f, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_pick null tokens", ssd_logprob_pick(p, 16, 1, 16, NULL, f, k, 1, f, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_pick null lse", ssd_logprob_pick(p, 16, 1, 16, t, NULL, k, 1, f, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_pick null n_top", ssd_logprob_pick(p, 16, 1, 16, t, f, NULL, 1, f, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_pick null out", ssd_logprob_pick(p, 16, 1, 16, t, f, k, 1, NULL, NULL), SSD_ERR_ARG);

  expect("ssd_logprob_pick_verify zero B", ssd_logprob_pick_verify(p, 16, 0, 3, 16, t, k, t, f, k, f, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_pick_verify negative K", ssd_logprob_pick_verify(p, 16, 1, -1, 16, t, k, t, f, k, f, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_pick_verify zero V", ssd_logprob_pick_verify(p, 16, 1, 3, 0, t, k, t, f, k, f, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_pick_verify ld below V", ssd_logprob_pick_verify(p, 8, 1, 3, 16, t, k, t, f, k, f, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_pick_verify null rows", ssd_logprob_pick_verify(NULL, 16, 1, 3, 16, t, k, t, f, k, f, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_pick_verify null ids", ssd_logprob_pick_verify(p, 16, 1, 3, 16, NULL, k, t, f, k, f, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_pick_verify null accept", ssd_logprob_pick_verify(p, 16, 1, 3, 16, t, NULL, t, f, k, f, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_pick_verify null recovery", ssd_logprob_pick_verify(p, 16, 1, 3, 16, t, k, NULL, f, k, f, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_pick_verify null lse", ssd_logprob_pick_verify(p, 16, 1, 3, 16, t, k, t, NULL, k, f, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_pick_verify null n_top", ssd_logprob_pick_verify(p, 16, 1, 3, 16, t, k, t, f, NULL, f, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_pick_verify null out", ssd_logprob_pick_verify(p, 16, 1, 3, 16, t, k, t, f, k, NULL, NULL), SSD_ERR_ARG);
  printf("%d failures\n", failures);
  return failures != 0;
}
