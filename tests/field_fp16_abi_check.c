/* AVR_FIELD_FP16's argument checks (include/avr.h, an addition within ABI 18) under a host AddressSanitizer build of
 * the library (`make -C adaptive-volume-rendering_amd asan-field-fp16`). Every call below is refused, or is a no-op,
 * BEFORE any HIP call, so the program runs without a GPU; ASan watches the reads of the host structs (dims, view
 * descriptors: heap-allocated at their exact size) and the formatting of the error strings. Exit status: number of
 * failed checks. Run by tests/test_field_fp16_ref_cpu.py.                                                        */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "abi_check_common.h"

int main(void) {
  /* stands in for device memory: never dereferenced by a refused call */
  double host[8] __attribute__((aligned(16))) = {0};
  float* f = (float*)host;
  int64_t* cnt = (int64_t*)host;
  avr_field_dims* d = (avr_field_dims*)malloc(sizeof(avr_field_dims));
  avr_view_desc* v = (avr_view_desc*)malloc(3 * sizeof(avr_view_desc));
  avr_resnetfc_weights* w = (avr_resnetfc_weights*)malloc(sizeof(avr_resnetfc_weights));
  if (!d || !v || !w) return 99;
  memset(d, 0, sizeof *d);
  memset(v, 0, 3 * sizeof *v);
  memset(w, 0, sizeof *w);
  d->d_in = 42; d->d_latent = 512; d->d_hidden = 512; d->n_blocks = 5; d->n_lin_z = 3; d->num_freqs = 6;
  d->freq_factor = 1.5f; d->precision = AVR_FIELD_FP16;
  for (int s = 0; s < 3; ++s) v[s].latent_h = v[s].latent_w = 8;

  if (avr_version() != AVR_ABI_VERSION || AVR_ABI_VERSION != 18 || AVR_FIELD_FP16 != 2 || AVR_FIELD_X3 != 1 ||
      AVR_FIELD_FP32 != 0) {
    fprintf(stderr, "FAIL version %d / precision constants\n", avr_version());
    ++failures;
  }

  /* the blob is the x3 blob: same size, and the pack refuses what it refuses for x3 */
  int64_t n16 = -1, n3 = -2;
  expect("packed_floats fp16", avr_field_packed_floats(d, &n16), AVR_OK, NULL);
  d->precision = AVR_FIELD_X3;
  expect("packed_floats x3", avr_field_packed_floats(d, &n3), AVR_OK, NULL);
  d->precision = AVR_FIELD_FP16;
  if (n16 != n3 || n16 <= 0) {
    fprintf(stderr, "FAIL blob sizes fp16 %lld x3 %lld\n", (long long)n16, (long long)n3);
    ++failures;
  }
  expect("pack: null weights", avr_field_pack(d, NULL, f, NULL), AVR_E_INVALID, "null");
  expect("pack: null blob", avr_field_pack(d, w, NULL, NULL), AVR_E_INVALID, "null");

  /* the single-scene entries */
  expect("rays: null view", avr_field_fwd_rays(d, NULL, f, f, f, f, f, 4, 8, f, NULL), AVR_E_INVALID, "null");
  expect("rays: null packed", avr_field_fwd_rays(d, v, NULL, f, f, f, f, 4, 8, f, NULL), AVR_E_INVALID, "null");
  expect("rays: null table", avr_field_fwd_rays(d, v, f, NULL, f, f, f, 4, 8, f, NULL), AVR_E_INVALID, "table");
  expect("rays: null z", avr_field_fwd_rays(d, v, f, f, f, f, NULL, 4, 8, f, NULL), AVR_E_INVALID, "null");
  expect("rays: n_samples 0", avr_field_fwd_rays(d, v, f, f, f, f, f, 4, 0, f, NULL), AVR_E_INVALID, "sizes");
  expect("rays: n_rays < 0", avr_field_fwd_rays(d, v, f, f, f, f, f, -1, 8, f, NULL), AVR_E_INVALID, "sizes");
  expect("rays: n_rays 0", avr_field_fwd_rays(d, v, f, f, NULL, NULL, NULL, 0, 8, NULL, NULL), AVR_OK, NULL);
  expect("points: null out", avr_field_fwd_points(d, v, f, f, f, f, 4, NULL, NULL), AVR_E_INVALID, "null");
  expect("points: n < 0", avr_field_fwd_points(d, v, f, f, f, f, -1, f, NULL), AVR_E_INVALID, "size");
  expect("points: n 0", avr_field_fwd_points(d, v, f, f, NULL, NULL, 0, NULL, NULL), AVR_OK, NULL);
  d->d_hidden = 384;
  expect("points: d_hidden 384", avr_field_fwd_points(d, v, f, f, f, f, 4, f, NULL), AVR_E_INVALID, NULL);
  d->d_hidden = 512;
  v[0].latent_h = 0;
  expect("points: latent size", avr_field_fwd_points(d, v, f, f, f, f, 4, f, NULL), AVR_E_INVALID, "latent");
  v[0].latent_h = 8;

  /* nets without a single-product kernel: AVR_E_UNSUPPORTED, never another path */
  d->bn = 1;
  expect("rays: BatchNorm", avr_field_fwd_rays(d, v, f, f, f, f, f, 4, 8, f, NULL), AVR_E_UNSUPPORTED, "fp16");
  expect("points: BatchNorm", avr_field_fwd_points(d, v, f, f, f, f, 4, f, NULL), AVR_E_UNSUPPORTED, "fp16");
  expect("points_batch: BatchNorm", avr_field_fwd_points_batch(d, v, 3, f, f, f, f, 4, f, NULL), AVR_E_UNSUPPORTED,
         "fp16");
  expect("rays_batch: BatchNorm", avr_field_fwd_rays_batch(d, v, 3, f, f, f, f, f, 4, 8, f, NULL), AVR_E_UNSUPPORTED,
         "fp16");
  expect("counted: BatchNorm", avr_field_fwd_points_counted(d, v, f, f, f, f, 4, cnt, f, NULL), AVR_E_UNSUPPORTED,
         "counted");
  d->bn = 0;
  d->spade = 1;
  expect("points: use_spade", avr_field_fwd_points(d, v, f, f, f, f, 4, f, NULL), AVR_E_UNSUPPORTED, "fp16");
  expect("counted: use_spade", avr_field_fwd_points_counted(d, v, f, f, f, f, 4, cnt, f, NULL), AVR_E_UNSUPPORTED,
         "counted");
  d->spade = 0;
  d->beta = 1.f;
  expect("points: Softplus", avr_field_fwd_points(d, v, f, f, f, f, 4, f, NULL), AVR_E_UNSUPPORTED, "fp16");
  expect("rays: Softplus", avr_field_fwd_rays(d, v, f, f, f, f, f, 4, 8, f, NULL), AVR_E_UNSUPPORTED, "fp16");
  expect("counted: Softplus", avr_field_fwd_points_counted(d, v, f, f, f, f, 4, cnt, f, NULL), AVR_E_UNSUPPORTED,
         "counted");
  d->beta = 0.f;

  /* the split (NS > 1) launch */
  expect("split: first half", avr_field_fwd_points_split(d, v, 2, f, f, f, f, 4, 0, 3, NULL, f, NULL, NULL),
         AVR_E_UNSUPPORTED, "split");
  expect("split: second half", avr_field_fwd_points_split(d, v, 1, f, f, NULL, NULL, 4, 3, 5, f, NULL, f, NULL),
         AVR_E_UNSUPPORTED, "split");

  /* the multi-scene entries */
  expect("points_batch: 17 scenes", avr_field_fwd_points_batch(d, v, 17, f, f, f, f, 4, f, NULL), AVR_E_INVALID,
         "scenes");
  expect("points_batch: 0 scenes", avr_field_fwd_points_batch(d, v, 0, f, f, f, f, 4, f, NULL), AVR_E_INVALID,
         "scenes");
  expect("points_batch: null views", avr_field_fwd_points_batch(d, NULL, 3, f, f, f, f, 4, f, NULL), AVR_E_INVALID,
         "scenes");
  expect("points_batch: null out", avr_field_fwd_points_batch(d, v, 3, f, f, f, f, 4, NULL, NULL), AVR_E_INVALID,
         "null");
  expect("points_batch: n < 0", avr_field_fwd_points_batch(d, v, 3, f, f, f, f, -1, f, NULL), AVR_E_INVALID, "size");
  expect("points_batch: n 0", avr_field_fwd_points_batch(d, v, 3, f, f, NULL, NULL, 0, NULL, NULL), AVR_OK, NULL);
  v[2].latent_w = 4;
  expect("points_batch: map sizes", avr_field_fwd_points_batch(d, v, 3, f, f, f, f, 4, f, NULL), AVR_E_INVALID,
         "one size");
  v[2].latent_w = 8;
  expect("rays_batch: null rd", avr_field_fwd_rays_batch(d, v, 3, f, f, f, NULL, f, 4, 8, f, NULL), AVR_E_INVALID,
         "null");
  expect("rays_batch: n_samples 0", avr_field_fwd_rays_batch(d, v, 3, f, f, f, f, f, 4, 0, f, NULL), AVR_E_INVALID,
         "sizes");
  expect("rays_batch: n_rays 0", avr_field_fwd_rays_batch(d, v, 3, f, f, NULL, NULL, NULL, 0, 8, NULL, NULL), AVR_OK,
         NULL);

  /* the counted entry */
  expect("counted: capacity < 0", avr_field_fwd_points_counted(d, v, f, f, f, f, -1, cnt, f, NULL), AVR_E_INVALID,
         "capacity");
  expect("counted: null count", avr_field_fwd_points_counted(d, v, f, f, f, f, 4, NULL, f, NULL), AVR_E_INVALID,
         "null");
  expect("counted: misaligned out", avr_field_fwd_points_counted(d, v, f, f, f, f, 4, cnt, f + 1, NULL), AVR_E_INVALID,
         "aligned");
  expect("counted: misaligned count", avr_field_fwd_points_counted(d, v, f, f, f, f, 4, (int64_t*)(f + 1), f, NULL),
         AVR_E_INVALID, "aligned");
  expect("counted: capacity 0", avr_field_fwd_points_counted(d, v, f, f, NULL, NULL, 0, NULL, NULL, NULL), AVR_OK,
         NULL);

  /* the training, backward and table entries take what they took before AVR_FIELD_FP16 existed */
  expect("train: fp16", avr_field_fwd_points_train(d, v, 1, f, f, f, f, 4, f, f, 4, (uint32_t*)f, NULL, NULL, 0, NULL,
                                                   NULL), AVR_E_INVALID, "x3 only");
  expect("bwd: fp16", avr_field_bwd(d, f, f, 1, 4, f, f, (const uint32_t*)f, f, 4, f, 4, NULL, NULL), AVR_E_INVALID,
         "x3 only");
  expect("table: null latent", avr_field_latent_table(d, f, NULL, 8, 8, f, NULL), AVR_E_INVALID, "null");
  expect("table_batch: 0 scenes", avr_field_latent_table_batch(d, f, f, 0, 8, 8, f, NULL), AVR_E_INVALID, "n_scenes");

  /* 7 is still no precision */
  d->precision = 7;
  expect("points: precision 7", avr_field_fwd_points(d, v, f, f, f, f, 4, f, NULL), AVR_E_INVALID, "precision 7");
  expect("rays: precision 7", avr_field_fwd_rays(d, v, f, f, f, f, f, 4, 8, f, NULL), AVR_E_INVALID, "precision 7");
  expect("counted: precision 7", avr_field_fwd_points_counted(d, v, f, f, f, f, 4, cnt, f, NULL), AVR_E_INVALID,
         "precision 7");
  expect("points_batch: precision 7", avr_field_fwd_points_batch(d, v, 3, f, f, f, f, 4, f, NULL), AVR_E_INVALID,
         "x3 or fp16");
  expect("split: precision 7", avr_field_fwd_points_split(d, v, 2, f, f, f, f, 4, 0, 3, NULL, f, NULL, NULL),
         AVR_E_INVALID, "x3 only");
  d->precision = AVR_FIELD_FP32;
  expect("points_batch: fp32", avr_field_fwd_points_batch(d, v, 3, f, f, f, f, 4, f, NULL), AVR_E_INVALID,
         "x3 or fp16");

  for (int k = 0; k < 8; ++k)
    if (host[k] != 0.0) {   /* no refused or empty call wrote anything */
      fprintf(stderr, "FAIL host buffer written\n");
      ++failures;
      break;
    }
  free(d);
  free(v);
  free(w);
  printf("field_fp16_abi_check: %d failure(s)\n", failures);
  return failures;
}
