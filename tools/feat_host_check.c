/*
 * feat_host_check.c -- the host side of the calls beside synthesis that runs
 * without a device: argument checks, the snapshot sizes and the snapshot
 * validation of include/lpcnet_mi355x.h's lpcnet_batch_*features*,
 * _burg_cepstrum*, _plc_rows_device, _plc_update* and _encode* calls, in the
 * order the contract gives them: value arguments, pointers, the null batch.
 * `make hostcheck` builds it against the in-tree library and `make check`
 * runs it.  It is also a stand-alone program for a sanitizer build of the
 * library's host code:
 *
 *   make lib BUILD=build_san LIB=build_san/liblpcnet_mi355x.so \
 *        EXTRA="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
 *   /opt/rocm/llvm/bin/clang -std=c99 -g -fsanitize=address,undefined -Iinclude -o build_san/feat_host_check \
 *        tools/feat_host_check.c -Lbuild_san -llpcnet_mi355x -Wl,-rpath,'$ORIGIN'
 *   (the compiler hipcc drives: the library's sanitizer calls need its runtime)
 *   build_san/feat_host_check
 *
 * Exit status 0 and "feat_host_check ok" when every check holds.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lpcnet_mi355x.h"

static int fails;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "line %d: %s (last error: %s)\n", __LINE__, #cond, lpcnet_mi355x_last_error()); \
      fails++;                                                           \
    }                                                                    \
  } while (0)

static int err_has(const char *s) { return strstr(lpcnet_mi355x_last_error(), s) != NULL; }

int main(void)
{
  const int n = lpcnet_batch_features_state_size(NULL);
  CHECK(n > 0 && n % 16 == 0 && n == lpcnet_batch_features_state_size(NULL));
  short *pcm = calloc(160, sizeof(short));
  float *feat = calloc(36, sizeof(float));
  unsigned char *st = calloc((size_t)n, 1);
  if (!pcm || !feat || !st) return 2;

  /* rows other than NB_FEATURES / NB_TOTAL_FEATURES, before anything else */
  static const int rows[] = {0, 18, 19, 21, 35, 37, 57, -20};
  for (size_t i = 0; i < sizeof(rows) / sizeof(rows[0]); i++) {
    CHECK(lpcnet_batch_compute_features_device(NULL, pcm, feat, rows[i], NULL, 1) == -1);
    CHECK(err_has("row"));
  }
  CHECK(lpcnet_batch_compute_features_device(NULL, pcm, feat, 20, NULL, -1) == -1 && err_has("nframes"));
  CHECK(lpcnet_batch_compute_features_device(NULL, NULL, feat, 20, NULL, 1) == -1);
  CHECK(lpcnet_batch_compute_features_device(NULL, pcm, feat, 20, NULL, 1) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_compute_features_device(NULL, pcm, feat, 36, NULL, 1) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_compute_features(NULL, pcm, feat, NULL) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_compute_features(NULL, NULL, feat, NULL) == -1);
  CHECK(lpcnet_batch_compute_features_float(NULL, (const float *)feat, NULL, NULL) == -1);

  /* stream indices */
  CHECK(lpcnet_batch_features_reset(NULL, -2) == -1 && err_has("no such stream"));
  CHECK(lpcnet_batch_features_reset(NULL, -1) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_features_save_state(NULL, -1, st) == -1 && err_has("no such stream"));
  CHECK(lpcnet_batch_features_save_state(NULL, 0, NULL) == -1);
  CHECK(lpcnet_batch_features_restore_state(NULL, -1, st) == -1 && err_has("no such stream"));
  CHECK(lpcnet_batch_features_restore_state(NULL, 0, NULL) == -1);

  /* a snapshot whose best_i (the last int) lies outside the Viterbi search is refused unread past its size */
  static const int bad[] = {-1, 224, 1 << 20};
  for (size_t i = 0; i < sizeof(bad) / sizeof(bad[0]); i++) {
    memcpy(st + n - 4, &bad[i], 4);
    CHECK(lpcnet_batch_features_restore_state(NULL, 0, st) == -1 && err_has("best_i"));
  }
  const int good = 223;
  memcpy(st + n - 4, &good, 4);
  CHECK(lpcnet_batch_features_restore_state(NULL, 0, st) == -1 && err_has("null batch"));

  /* Burg analysis: host calls, then the device call's col / row / nframes */
  CHECK(lpcnet_batch_burg_cepstrum(NULL, pcm, feat, NULL) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_burg_cepstrum(NULL, NULL, feat, NULL) == -1 && !err_has("null batch"));
  CHECK(lpcnet_batch_burg_cepstrum(NULL, pcm, NULL, NULL) == -1 && !err_has("null batch"));
  CHECK(lpcnet_batch_burg_cepstrum_float(NULL, (const float *)feat, feat, NULL) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_burg_cepstrum_float(NULL, NULL, feat, NULL) == -1 && !err_has("null batch"));
  CHECK(lpcnet_batch_burg_cepstrum_device(NULL, pcm, feat, 36, -1, NULL, 1) == -1 && err_has("col"));
  static const int brows[][2] = {{0, 0}, {35, 0}, {-36, 0}, {36, 1}, {56, 21}};
  for (size_t i = 0; i < sizeof(brows) / sizeof(brows[0]); i++)
    CHECK(lpcnet_batch_burg_cepstrum_device(NULL, pcm, feat, brows[i][0], brows[i][1], NULL, 1) == -1 && err_has("row"));
  CHECK(lpcnet_batch_burg_cepstrum_device(NULL, pcm, feat, 36, 0, NULL, -1) == -1 && err_has("nframes"));
  CHECK(lpcnet_batch_burg_cepstrum_device(NULL, NULL, feat, 36, 0, NULL, 1) == -1 && !err_has("null batch"));
  CHECK(lpcnet_batch_burg_cepstrum_device(NULL, pcm, NULL, 36, 0, NULL, 1) == -1 && !err_has("null batch"));
  CHECK(lpcnet_batch_burg_cepstrum_device(NULL, pcm, feat, 36, 0, NULL, 1) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_burg_cepstrum_device(NULL, pcm, feat, 57, 21, NULL, 1) == -1 && err_has("null batch"));

  /* the predictor's input rows: parts, then pointers, then the batch */
  static const int parts[] = {0, 4, -1, 7};
  for (size_t i = 0; i < sizeof(parts) / sizeof(parts[0]); i++)
    CHECK(lpcnet_batch_plc_rows_device(NULL, pcm, feat, parts[i], 1.f, NULL) == -1 && err_has("parts"));
  CHECK(lpcnet_batch_plc_rows_device(NULL, NULL, feat, 3, 1.f, NULL) == -1 && !err_has("null batch"));
  CHECK(lpcnet_batch_plc_rows_device(NULL, pcm, NULL, 3, 1.f, NULL) == -1 && !err_has("null batch"));
  for (int p = 1; p <= 3; p++) CHECK(lpcnet_batch_plc_rows_device(NULL, pcm, feat, p, 1.f, NULL) == -1 && err_has("null batch"));

  /* the good-packet step asks for a batch with PLC records before anything else */
  CHECK(lpcnet_batch_plc_update(NULL, pcm, feat, NULL) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_plc_update(NULL, NULL, NULL, NULL) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_plc_update_device(NULL, pcm, feat, NULL) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_plc_update_device(NULL, NULL, NULL, NULL) == -1 && err_has("null batch"));

  /* 1.6 kb/s encoder */
  unsigned char pk[8];
  CHECK(lpcnet_batch_encode(NULL, pcm, pk, feat, NULL) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_encode(NULL, pcm, pk, NULL, NULL) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_encode(NULL, NULL, pk, feat, NULL) == -1 && !err_has("null batch"));
  CHECK(lpcnet_batch_encode(NULL, pcm, NULL, feat, NULL) == -1 && !err_has("null batch"));
  CHECK(lpcnet_batch_compute_features4(NULL, pcm, feat, NULL) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_compute_features4(NULL, NULL, feat, NULL) == -1 && !err_has("null batch"));
  CHECK(lpcnet_batch_compute_features4(NULL, pcm, NULL, NULL) == -1 && !err_has("null batch"));
  for (size_t i = 0; i < sizeof(rows) / sizeof(rows[0]); i++)
    CHECK(lpcnet_batch_encode_device(NULL, pcm, pk, feat, rows[i], NULL, 1) == -1 && err_has("row"));
  CHECK(lpcnet_batch_encode_device(NULL, pcm, pk, feat, 20, NULL, -1) == -1 && err_has("npackets"));
  CHECK(lpcnet_batch_encode_device(NULL, NULL, pk, feat, 20, NULL, 1) == -1 && !err_has("null batch"));
  CHECK(lpcnet_batch_encode_device(NULL, pcm, NULL, feat, 20, NULL, 1) == -1 && !err_has("null batch"));
  CHECK(lpcnet_batch_encode_device(NULL, pcm, pk, NULL, 20, NULL, 1) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_encode_device(NULL, pcm, pk, feat, 36, NULL, 0) == -1 && err_has("null batch"));

  /* the encoder snapshot: the features snapshot, then vq_mem[18] */
  const int ne = lpcnet_batch_encode_state_size(NULL);
  CHECK(ne == n + 18 * 4);
  unsigned char *est = calloc((size_t)ne, 1);
  if (!est) return 2;
  CHECK(lpcnet_batch_encode_save_state(NULL, -1, est) == -1 && err_has("no such stream"));
  CHECK(lpcnet_batch_encode_save_state(NULL, 0, NULL) == -1 && !err_has("null batch"));
  CHECK(lpcnet_batch_encode_save_state(NULL, 0, est) == -1 && err_has("null batch"));
  CHECK(lpcnet_batch_encode_restore_state(NULL, -1, est) == -1 && err_has("no such stream"));
  CHECK(lpcnet_batch_encode_restore_state(NULL, 0, NULL) == -1 && !err_has("null batch"));
  for (size_t i = 0; i < sizeof(bad) / sizeof(bad[0]); i++) {
    memcpy(est + n - 4, &bad[i], 4);
    CHECK(lpcnet_batch_encode_restore_state(NULL, 0, est) == -1 && err_has("best_i"));
  }
  memcpy(est + n - 4, &good, 4);
  CHECK(lpcnet_batch_encode_restore_state(NULL, 0, est) == -1 && err_has("null batch"));
  free(est);

  /* a batch cannot exist without a device: creation fails cleanly */
  if (lpcnet_mi355x_device_count() == 0) CHECK(lpcnet_batch_create(4, 0) == NULL);

  free(pcm);
  free(feat);
  free(st);
  if (fails) return 1;
  printf("feat_host_check ok (snapshot %d bytes)\n", n);
  return 0;
}
