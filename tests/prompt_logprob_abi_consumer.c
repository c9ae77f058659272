/* Plain-C consumer of include/ssd_hip_prompt_logprob.h (tests/test_prompt_logprob_cpu.py builds it with cc -std=c99 -Wall -Werror and
 * links libssdhip.so): ssd_logprob_rows_known called with zero or negative sizes, more than 65535 rows, ld < V, a vocabulary above
 * SSD_LOGPROB_MAX_V or null required pointers must return SSD_ERR_SHAPE or SSD_ERR_ARG from its argument validation, before any launch
 * (no GPU is needed for that); the workspace query answers on the host. */
#include <stdio.h>
#include "ssd_hip_prompt_logprob.h"

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
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION || SSD_HIP_ABI_VERSION != 3) {
    printf("FAIL abi version %d / %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  /* the workspace query: the records of ssd_logprob_rows, refusing what ssd_logprob_rows_known refuses */
  expect("ssd_logprob_known_ws_bytes zero T", ssd_logprob_known_ws_bytes(0, 16), SSD_ERR_SHAPE);
  expect("ssd_logprob_known_ws_bytes zero V", ssd_logprob_known_ws_bytes(1, 0), SSD_ERR_SHAPE);
  expect("ssd_logprob_known_ws_bytes V above SSD_LOGPROB_MAX_V", ssd_logprob_known_ws_bytes(1, big), SSD_ERR_SHAPE);
  {
    const int one = ssd_logprob_known_ws_bytes(1, 1), slice = ssd_logprob_known_ws_bytes(1, SSD_LOGPROB_SLICE);
    expect("ssd_logprob_known_ws_bytes workspace query: one slice up to SSD_LOGPROB_SLICE", one > 0 && one == slice, 1);
    expect("ssd_logprob_known_ws_bytes workspace query: a second slice", ssd_logprob_known_ws_bytes(1, SSD_LOGPROB_SLICE + 1), 2 * one);
    expect("ssd_logprob_known_ws_bytes workspace query: rows", ssd_logprob_known_ws_bytes(512, SSD_LOGPROB_MAX_V),
           512 * (SSD_LOGPROB_MAX_V / SSD_LOGPROB_SLICE) * one);
    expect("ssd_logprob_known_ws_bytes workspace query: as ssd_logprob_rows_ws_bytes", ssd_logprob_known_ws_bytes(7, 128256),
           ssd_logprob_rows_ws_bytes(7, 128256));
  }

  expect("ssd_logprob_rows_known zero T", ssd_logprob_rows_known(p, 16, 0, 16, k, t, f, f, k, f, k, p, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows_known negative T", ssd_logprob_rows_known(p, 16, -1, 16, k, t, f, f, k, f, k, p, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows_known T above 65535", ssd_logprob_rows_known(p, 16, 65536, 16, k, t, f, f, k, f, k, p, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows_known zero V", ssd_logprob_rows_known(p, 16, 1, 0, k, t, f, f, k, f, k, p, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows_known negative V", ssd_logprob_rows_known(p, 16, 1, -4, k, t, f, f, k, f, k, p, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows_known ld below V", ssd_logprob_rows_known(p, 8, 1, 16, k, t, f, f, k, f, k, p, NULL), SSD_ERR_SHAPE);
  expect("ssd_logprob_rows_known V above SSD_LOGPROB_MAX_V", ssd_logprob_rows_known(p, big, 1, big, k, t, f, f, k, f, k, p, NULL),
         SSD_ERR_SHAPE);
  expect("ssd_logprob_rows_known null rows", ssd_logprob_rows_known(NULL, 16, 1, 16, k, t, f, f, k, f, k, p, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_rows_known null n_top", ssd_logprob_rows_known(p, 16, 1, 16, NULL, t, f, f, k, f, k, p, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_rows_known null tokens", ssd_logprob_rows_known(p, 16, 1, 16, k, NULL, f, f, k, f, k, p, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_rows_known null lse", ssd_logprob_rows_known(p, 16, 1, 16, k, t, NULL, f, k, f, k, p, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_rows_known null top_val alone", ssd_logprob_rows_known(p, 16, 1, 16, k, t, f, NULL, k, f, k, p, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_rows_known null top_id alone", ssd_logprob_rows_known(p, 16, 1, 16, k, t, f, f, NULL, f, k, p, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_rows_known null out", ssd_logprob_rows_known(p, 16, 1, 16, k, t, f, f, k, NULL, k, p, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_rows_known null rank", ssd_logprob_rows_known(p, 16, 1, 16, k, t, f, f, k, f, NULL, p, NULL), SSD_ERR_ARG);
  expect("ssd_logprob_rows_known null ws", ssd_logprob_rows_known(p, 16, 1, 16, k, t, f, f, k, f, k, NULL, NULL), SSD_ERR_ARG);
  /* a shape error wins over a null pointer, as in ssd_logprob_rows */
  expect("ssd_logprob_rows_known zero T and null rows", ssd_logprob_rows_known(NULL, 16, 0, 16, k, t, f, f, k, f, k, p, NULL), SSD_ERR_SHAPE);
  printf("%d failures\n", failures);
  return failures != 0;
}
