/* The occupancy-grid entries' argument checks (include/avr.h, additions within ABI 18) under a host
 * AddressSanitizer build of the library (`make -C adaptive-volume-rendering_amd asan-occupancy`, the build
 * tests/abi_check.c uses). Every call below is rejected with AVR_E_INVALID, or is a no-op, BEFORE any HIP call, so
 * the program runs without a GPU; ASan watches the reads of the host descriptor and res array (heap-allocated at
 * their exact size) and the formatting of the error strings. Exit status: number of failed checks. Run by
 * tests/test_cpu_occupancy.py.                                                                               */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "abi_check_common.h"

int main(void) {
  float host[16] = {0};      /* stands in for device memory: never dereferenced by a refused call */
  float* f = host;
  uint32_t* bits = (uint32_t*)host;
  uint64_t* mask = (uint64_t*)host;
  int64_t* offs = (int64_t*)host;
  int32_t* counts = (int32_t*)host;
  int* res = (int*)malloc(3 * sizeof(int));
  avr_occ_grid* g = (avr_occ_grid*)malloc(sizeof(avr_occ_grid));
  if (!res || !g) return 99;
  res[0] = 32; res[1] = 16; res[2] = 8;
  for (int a = 0; a < 3; ++a) { g->lo[a] = -1.f; g->inv[a] = 1.f; g->res[a] = res[a]; }
  g->bits = bits;

  if (avr_version() != AVR_ABI_VERSION || AVR_ABI_VERSION != 18) {
    fprintf(stderr, "FAIL version %d\n", avr_version());
    ++failures;
  }

  /* avr_occ_build */
  expect("build: null res", avr_occ_build(f, 1, NULL, 0.f, 1, bits, NULL), AVR_E_INVALID, "null");
  expect("build: null sigma", avr_occ_build(NULL, 1, res, 0.f, 1, bits, NULL), AVR_E_INVALID, "null");
  expect("build: null bits", avr_occ_build(f, 1, res, 0.f, 1, NULL, NULL), AVR_E_INVALID, "null");
  expect("build: no planes", avr_occ_build(f, 0, res, 0.f, 1, bits, NULL), AVR_E_INVALID, "n_planes");
  expect("build: dilate 3", avr_occ_build(f, 1, res, 0.f, 3, bits, NULL), AVR_E_INVALID, "dilate");
  expect("build: dilate -1", avr_occ_build(f, 1, res, 0.f, -1, bits, NULL), AVR_E_INVALID, "dilate");
  res[0] = 48;
  expect("build: rx % 32", avr_occ_build(f, 1, res, 0.f, 1, bits, NULL), AVR_E_INVALID, "multiple of 32");
  res[0] = 32;
  for (int a = 0; a < 3; ++a) {
    const int keep = res[a];
    res[a] = 0;
    expect("build: res 0", avr_occ_build(f, 1, res, 0.f, 1, bits, NULL), AVR_E_INVALID, "res[");
    res[a] = a == 0 ? 288 : 257;
    expect("build: res above 256", avr_occ_build(f, 1, res, 0.f, 1, bits, NULL), AVR_E_INVALID, "res[");
    res[a] = keep;
  }

  /* avr_occ_classify */
  expect("classify: null grid", avr_occ_classify(NULL, f, f, f, 4, 8, mask, counts, NULL), AVR_E_INVALID, "null");
  g->bits = NULL;
  expect("classify: null bits", avr_occ_classify(g, f, f, f, 4, 8, mask, counts, NULL), AVR_E_INVALID, "null");
  g->bits = bits;
  expect("classify: null ro", avr_occ_classify(g, NULL, f, f, 4, 8, mask, counts, NULL), AVR_E_INVALID, "null");
  expect("classify: null rd", avr_occ_classify(g, f, NULL, f, 4, 8, mask, counts, NULL), AVR_E_INVALID, "null");
  expect("classify: null z", avr_occ_classify(g, f, f, NULL, 4, 8, mask, counts, NULL), AVR_E_INVALID, "null");
  expect("classify: null mask", avr_occ_classify(g, f, f, f, 4, 8, NULL, counts, NULL), AVR_E_INVALID, "null");
  expect("classify: null counts", avr_occ_classify(g, f, f, f, 4, 8, mask, NULL, NULL), AVR_E_INVALID, "null");
  expect("classify: N = 0", avr_occ_classify(g, f, f, f, 4, 0, mask, counts, NULL), AVR_E_INVALID, "n_samples");
  expect("classify: N = 257", avr_occ_classify(g, f, f, f, 4, 257, mask, counts, NULL), AVR_E_INVALID, "n_samples");
  expect("classify: R < 0", avr_occ_classify(g, f, f, f, -1, 8, mask, counts, NULL), AVR_E_INVALID, "n_rays");
  expect("classify: R = 0", avr_occ_classify(g, NULL, NULL, NULL, 0, 8, NULL, NULL, NULL), AVR_OK, NULL);
  g->res[0] = 40;
  expect("classify: rx % 32", avr_occ_classify(g, f, f, f, 4, 8, mask, counts, NULL), AVR_E_INVALID, "multiple of 32");
  g->res[0] = 32;
  g->res[2] = 0;
  expect("classify: res 0", avr_occ_classify(g, f, f, f, 4, 8, mask, counts, NULL), AVR_E_INVALID, "res[");
  g->res[2] = 300;
  expect("classify: res 300", avr_occ_classify(g, f, f, f, 4, 8, mask, counts, NULL), AVR_E_INVALID, "res[");
  g->res[2] = 8;

  /* avr_occ_compact */
  expect("compact: null ro", avr_occ_compact(NULL, f, f, mask, offs, 4, 8, 5, f, f, NULL), AVR_E_INVALID, "null");
  expect("compact: null mask", avr_occ_compact(f, f, f, NULL, offs, 4, 8, 5, f, f, NULL), AVR_E_INVALID, "null");
  expect("compact: null offsets", avr_occ_compact(f, f, f, mask, NULL, 4, 8, 5, f, f, NULL), AVR_E_INVALID, "null");
  expect("compact: null xyz", avr_occ_compact(f, f, f, mask, offs, 4, 8, 5, NULL, f, NULL), AVR_E_INVALID, "null");
  expect("compact: null viewdirs", avr_occ_compact(f, f, f, mask, offs, 4, 8, 5, f, NULL, NULL), AVR_E_INVALID, "null");
  expect("compact: N = 0", avr_occ_compact(f, f, f, mask, offs, 4, 0, 0, f, f, NULL), AVR_E_INVALID, "n_samples");
  expect("compact: N = 257", avr_occ_compact(f, f, f, mask, offs, 4, 257, 5, f, f, NULL), AVR_E_INVALID, "n_samples");
  expect("compact: R < 0", avr_occ_compact(f, f, f, mask, offs, -4, 8, 0, f, f, NULL), AVR_E_INVALID, "n_rays");
  expect("compact: M < 0", avr_occ_compact(f, f, f, mask, offs, 4, 8, -1, f, f, NULL), AVR_E_INVALID, "n_live");
  expect("compact: M > R N", avr_occ_compact(f, f, f, mask, offs, 4, 8, 33, f, f, NULL), AVR_E_INVALID, "n_live");
  expect("compact: M = 0", avr_occ_compact(NULL, NULL, NULL, NULL, NULL, 4, 8, 0, NULL, NULL, NULL), AVR_OK, NULL);
  expect("compact: R = 0", avr_occ_compact(NULL, NULL, NULL, NULL, NULL, 0, 8, 0, NULL, NULL, NULL), AVR_OK, NULL);

  /* avr_occ_expand */
  expect("expand: null field", avr_occ_expand(f, mask, offs, 4, 8, 5, NULL, NULL), AVR_E_INVALID, "null");
  expect("expand: null field_c", avr_occ_expand(NULL, mask, offs, 4, 8, 5, f, NULL), AVR_E_INVALID, "null");
  expect("expand: null mask", avr_occ_expand(f, NULL, offs, 4, 8, 5, f, NULL), AVR_E_INVALID, "null");
  expect("expand: null offsets", avr_occ_expand(f, mask, NULL, 4, 8, 5, f, NULL), AVR_E_INVALID, "null");
  expect("expand: N = 0", avr_occ_expand(f, mask, offs, 4, 0, 0, f, NULL), AVR_E_INVALID, "n_samples");
  expect("expand: N = 257", avr_occ_expand(f, mask, offs, 4, 257, 5, f, NULL), AVR_E_INVALID, "n_samples");
  expect("expand: R < 0", avr_occ_expand(f, mask, offs, -1, 8, 0, f, NULL), AVR_E_INVALID, "n_rays");
  expect("expand: M > R N", avr_occ_expand(f, mask, offs, 4, 8, 33, f, NULL), AVR_E_INVALID, "n_live");
  expect("expand: misaligned", avr_occ_expand(f, mask, offs, 4, 8, 5, f + 1, NULL), AVR_E_INVALID, "aligned");
  expect("expand: R = 0", avr_occ_expand(NULL, NULL, NULL, 0, 8, 0, NULL, NULL), AVR_OK, NULL);

  for (int k = 0; k < 16; ++k)
    if (host[k] != 0.f) {   /* no refused or empty call wrote anything */
      fprintf(stderr, "FAIL host buffer written\n");
      ++failures;
      break;
    }
  free(res);
  free(g);
  printf("occupancy_abi_check: %d failure(s)\n", failures);
  return failures;
}
