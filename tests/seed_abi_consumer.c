/* Plain-C consumer of include/ssd_hip_seed.h (tests/test_seed_cpu.py builds it with cc -std=c99 -Wall -Werror and links libssdhip.so):
 * ssd_sample_rows_seeded, ssd_verify_ratio_seeded and ssd_seeded_uniforms called with zero or negative sizes, null required pointers
 * or a purpose that does not exist must return SSD_ERR_SHAPE or SSD_ERR_ARG from their argument validation, before any launch (no
 * GPU is needed for that), and the workspace query answers on the host. */
#include <stdio.h>
#include "ssd_hip_seed.h"

static int failures = 0;

static void expect(const char* what, long rc, long want) {
  if (rc != want) {
    printf("FAIL %s returned %ld, expected %ld\n", what, rc, want);
    ++failures;
  } else {
    printf("ok   %s -> %ld\n", what, rc);
  }
}

static int sample(const void* lg, int T, int V, const float* temps, int rpt, const void* rng, int64_t* out, const int32_t* boost,
                  int boost_k, float boost_x, const int64_t* seed, int rps, const int64_t* pos, int purpose, void* ws) {
  return ssd_sample_rows_seeded(lg, 16, T, V, temps, rpt, rng, 1u, out, NULL, boost, boost_k, boost_x, NULL, seed, rps, pos, purpose, ws);
}

static int verify(int V, int B, int K, const void* p, const int32_t* boost, int boost_k, const int64_t* seed, const int64_t* pos) {
  return ssd_verify_ratio_seeded(p, 16, p, 16, V, B, K, (const int64_t*)p, (const int64_t*)p, (const float*)p, (const float*)p,
                                 (const float*)p, (const float*)p, (const int32_t*)p, p, 2u, (int32_t*)p, (int64_t*)p, NULL, NULL,
                                 boost, boost_k, 2.0f, NULL, seed, pos);
}

int main(void) {
  int64_t buf[16];
  void* p = buf;
  const float* f = (const float*)buf;
  const int32_t* k = (const int32_t*)buf;
  const int64_t* q = buf;
  if (ssd_abi_version() != SSD_HIP_ABI_VERSION) {
    printf("FAIL abi version %d != %d\n", ssd_abi_version(), SSD_HIP_ABI_VERSION);
    ++failures;
  }
  if (SSD_SEED_DRAFT != 1 || SSD_SEED_TARGET != 2 || SSD_SEED_ACCEPT != 3 || SSD_SEED_SLICE != 4096) {
    printf("FAIL purposes / slice moved\n");
    ++failures;
  }
  expect("workspace query one slice", ssd_sample_seeded_ws_bytes(1, 4096), 8);
  expect("workspace query ragged", ssd_sample_seeded_ws_bytes(3, 4097), 48);
  expect("workspace query largest shape", ssd_sample_seeded_ws_bytes(2147483647, 2147483647), 2147483647L * 524288L * 8L);
  expect("workspace query zero T", ssd_sample_seeded_ws_bytes(0, 16), SSD_ERR_SHAPE);
  expect("workspace query zero V", ssd_sample_seeded_ws_bytes(1, 0), SSD_ERR_SHAPE);

  expect("sample zero T", sample(p, 0, 16, f, 1, p, buf, NULL, 0, 1.f, q, 1, q, SSD_SEED_TARGET, p), SSD_ERR_SHAPE);
  expect("sample negative T", sample(p, -1, 16, f, 1, p, buf, NULL, 0, 1.f, q, 1, q, SSD_SEED_TARGET, p), SSD_ERR_SHAPE);
  expect("sample zero V", sample(p, 1, 0, f, 1, p, buf, NULL, 0, 1.f, q, 1, q, SSD_SEED_TARGET, p), SSD_ERR_SHAPE);
  expect("sample zero rows_per_temp", sample(p, 1, 16, f, 0, p, buf, NULL, 0, 1.f, q, 1, q, SSD_SEED_TARGET, p), SSD_ERR_SHAPE);
  expect("sample zero rows_per_seed", sample(p, 1, 16, f, 1, p, buf, NULL, 0, 1.f, q, 0, q, SSD_SEED_TARGET, p), SSD_ERR_SHAPE);
  expect("sample null rows", sample(NULL, 1, 16, f, 1, p, buf, NULL, 0, 1.f, q, 1, q, SSD_SEED_TARGET, p), SSD_ERR_ARG);
  expect("sample null temps", sample(p, 1, 16, NULL, 1, p, buf, NULL, 0, 1.f, q, 1, q, SSD_SEED_TARGET, p), SSD_ERR_ARG);
  expect("sample null rng", sample(p, 1, 16, f, 1, NULL, buf, NULL, 0, 1.f, q, 1, q, SSD_SEED_TARGET, p), SSD_ERR_ARG);
  expect("sample null out", sample(p, 1, 16, f, 1, p, NULL, NULL, 0, 1.f, q, 1, q, SSD_SEED_TARGET, p), SSD_ERR_ARG);
  expect("sample null row_seed", sample(p, 1, 16, f, 1, p, buf, NULL, 0, 1.f, NULL, 1, q, SSD_SEED_TARGET, p), SSD_ERR_ARG);
  expect("sample null positions", sample(p, 1, 16, f, 1, p, buf, NULL, 0, 1.f, q, 1, NULL, SSD_SEED_TARGET, p), SSD_ERR_ARG);
  expect("sample null workspace", sample(p, 1, 16, f, 1, p, buf, NULL, 0, 1.f, q, 1, q, SSD_SEED_TARGET, NULL), SSD_ERR_ARG);
  expect("sample purpose 0", sample(p, 1, 16, f, 1, p, buf, NULL, 0, 1.f, q, 1, q, 0, p), SSD_ERR_ARG);
  expect("sample purpose 4", sample(p, 1, 16, f, 1, p, buf, NULL, 0, 1.f, q, 1, q, 4, p), SSD_ERR_ARG);
  expect("sample boost_k 0", sample(p, 1, 16, f, 1, p, buf, k, 0, 2.f, q, 1, q, SSD_SEED_DRAFT, p), SSD_ERR_ARG);
  expect("sample boost_k 9", sample(p, 1, 16, f, 1, p, buf, k, 9, 2.f, q, 1, q, SSD_SEED_DRAFT, p), SSD_ERR_ARG);
  expect("sample boost_x 0", sample(p, 1, 16, f, 1, p, buf, k, 2, 0.f, q, 1, q, SSD_SEED_DRAFT, p), SSD_ERR_ARG);

  expect("verify zero B", verify(16, 0, 2, p, NULL, 0, q, q), SSD_ERR_SHAPE);
  expect("verify zero K", verify(16, 1, 0, p, NULL, 0, q, q), SSD_ERR_SHAPE);
  expect("verify K 63", verify(16, 1, 63, p, NULL, 0, q, q), SSD_ERR_SHAPE);
  expect("verify zero V", verify(0, 1, 2, p, NULL, 0, q, q), SSD_ERR_SHAPE);
  expect("verify boost_k 9", verify(16, 1, 2, p, k, 9, q, q), SSD_ERR_ARG);
  expect("verify null row_seed", verify(16, 1, 2, p, NULL, 0, NULL, q), SSD_ERR_ARG);
  expect("verify null positions", verify(16, 1, 2, p, NULL, 0, q, NULL), SSD_ERR_ARG);

  expect("uniforms zero rows", ssd_seeded_uniforms(q, q, 0, 1, 0u, 4, (float*)p, NULL), SSD_ERR_SHAPE);
  expect("uniforms zero n", ssd_seeded_uniforms(q, q, 1, 1, 0u, 0, (float*)p, NULL), SSD_ERR_SHAPE);
  expect("uniforms index past 2^32", ssd_seeded_uniforms(q, q, 1, 1, 4294967295u, 2, (float*)p, NULL), SSD_ERR_SHAPE);
  expect("uniforms null row_seed", ssd_seeded_uniforms(NULL, q, 1, 1, 0u, 4, (float*)p, NULL), SSD_ERR_ARG);
  expect("uniforms null positions", ssd_seeded_uniforms(q, NULL, 1, 1, 0u, 4, (float*)p, NULL), SSD_ERR_ARG);
  expect("uniforms null out", ssd_seeded_uniforms(q, q, 1, 1, 0u, 4, NULL, NULL), SSD_ERR_ARG);
  expect("uniforms purpose 0", ssd_seeded_uniforms(q, q, 1, 0, 0u, 4, (float*)p, NULL), SSD_ERR_ARG);
  expect("uniforms purpose 4", ssd_seeded_uniforms(q, q, 1, 4, 0u, 4, (float*)p, NULL), SSD_ERR_ARG);
  printf("%d failures\n", failures);
  return failures != 0;
}
