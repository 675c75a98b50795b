/* The device-side early-termination entries' argument checks (include/avr.h "fine pass, early termination on the
 * device", additions within ABI 18) under a host AddressSanitizer build of the library (`make -C
 * adaptive-volume-rendering_amd asan-march-device`, the build tests/abi_check.c uses). Every call below is rejected
 * with AVR_E_INVALID, or is a no-op, BEFORE any HIP call, so the program runs without a GPU; ASan watches the reads of
 * the host descriptor (heap-allocated at its exact size) and the formatting of the error strings. Exit status: number
 * of failed checks. Run by tests/test_cpu_march_device.py.                                                        */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "abi_check_common.h"

int main(void) {
  _Alignas(16) float host[16] = {0};   /* stands in for device memory: never dereferenced by a refused call */
  float* f = host;
  void* st = host;
  uint64_t* mask = (uint64_t*)host;
  int64_t* offs = (int64_t*)host;
  int64_t* cnt = (int64_t*)host;
  int32_t* counts = (int32_t*)host;
  void* odd8 = (char*)host + 4;        /* not 8-B aligned */
  avr_occ_grid* g = (avr_occ_grid*)malloc(sizeof(avr_occ_grid));
  if (!g) return 99;
  memset(g, 0, sizeof *g);
  g->res[0] = g->res[1] = g->res[2] = 32;
  g->bits = (const uint32_t*)host;

  if (avr_version() != AVR_ABI_VERSION || AVR_ABI_VERSION != 18) {
    fprintf(stderr, "FAIL version %d\n", avr_version());
    ++failures;
  }

  /* avr_march_classify(grid, ro, rd, z, state, R, N, c0, chunk, t_stop, mask, counts, stream) */
  expect("classify: R < 0", avr_march_classify(NULL, f, f, f, st, -1, 100, 0, 64, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "n_rays");
  expect("classify: chunk 0", avr_march_classify(NULL, f, f, f, st, 4, 100, 0, 0, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "chunk");
  expect("classify: chunk 65", avr_march_classify(NULL, f, f, f, st, 4, 100, 0, 65, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "chunk");
  expect("classify: window past N", avr_march_classify(NULL, f, f, f, st, 4, 100, 64, 37, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "n_samples");
  expect("classify: c0 < 0", avr_march_classify(NULL, f, f, f, st, 4, 100, -1, 16, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "n_samples");
  expect("classify: N = 0", avr_march_classify(NULL, f, f, f, st, 4, 0, 0, 1, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "n_samples");
  expect("classify: c0 + chunk overflow",
         avr_march_classify(NULL, f, f, f, st, 4, 100, 2147483647, 64, 0.f, mask, counts, NULL), AVR_E_INVALID,
         "n_samples");
  expect("classify: null ro", avr_march_classify(NULL, NULL, f, f, st, 4, 100, 0, 64, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "null");
  expect("classify: null rd", avr_march_classify(NULL, f, NULL, f, st, 4, 100, 0, 64, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "null");
  expect("classify: null z", avr_march_classify(NULL, f, f, NULL, st, 4, 100, 0, 64, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "null");
  expect("classify: null state", avr_march_classify(NULL, f, f, f, NULL, 4, 100, 0, 64, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "null");
  expect("classify: null mask", avr_march_classify(NULL, f, f, f, st, 4, 100, 0, 64, 0.f, NULL, counts, NULL),
         AVR_E_INVALID, "null");
  expect("classify: null counts", avr_march_classify(NULL, f, f, f, st, 4, 100, 0, 64, 0.f, mask, NULL, NULL),
         AVR_E_INVALID, "null");
  expect("classify: misaligned mask",
         avr_march_classify(NULL, f, f, f, st, 4, 100, 0, 64, 0.f, (uint64_t*)odd8, counts, NULL), AVR_E_INVALID,
         "aligned");
  expect("classify: misaligned state", avr_march_classify(NULL, f, f, f, odd8, 4, 100, 0, 64, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "aligned");
  g->res[0] = 48;
  expect("classify: grid rx % 32", avr_march_classify(g, f, f, f, st, 4, 100, 0, 64, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "multiple of 32");
  g->res[0] = 32;
  g->res[2] = 257;
  expect("classify: grid rz 257", avr_march_classify(g, f, f, f, st, 4, 100, 0, 64, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "res[2]");
  g->res[2] = 32;
  g->bits = NULL;
  expect("classify: null grid bits", avr_march_classify(g, f, f, f, st, 4, 100, 0, 64, 0.f, mask, counts, NULL),
         AVR_E_INVALID, "null");
  g->bits = (const uint32_t*)host;
  expect("classify: R = 0", avr_march_classify(NULL, NULL, NULL, NULL, NULL, 0, 100, 64, 36, 0.f, NULL, NULL, NULL),
         AVR_OK, NULL);
  expect("classify: R = 0, grid", avr_march_classify(g, NULL, NULL, NULL, NULL, 0, 100, 0, 64, 0.f, NULL, NULL, NULL),
         AVR_OK, NULL);

  /* avr_march_compact_counted(ro, rd, z, mask, offsets, R, N, c0, chunk, n_live, capacity, xyz, viewdirs, stream) */
  expect("compact: R < 0", avr_march_compact_counted(f, f, f, mask, offs, -1, 100, 0, 64, cnt, 0, f, f, NULL),
         AVR_E_INVALID, "n_rays");
  expect("compact: chunk 0", avr_march_compact_counted(f, f, f, mask, offs, 4, 100, 0, 0, cnt, 0, f, f, NULL),
         AVR_E_INVALID, "chunk");
  expect("compact: chunk 65", avr_march_compact_counted(f, f, f, mask, offs, 4, 100, 0, 65, cnt, 4, f, f, NULL),
         AVR_E_INVALID, "chunk");
  expect("compact: window past N", avr_march_compact_counted(f, f, f, mask, offs, 4, 100, 90, 11, cnt, 4, f, f, NULL),
         AVR_E_INVALID, "n_samples");
  expect("compact: capacity < 0", avr_march_compact_counted(f, f, f, mask, offs, 4, 100, 0, 64, cnt, -1, f, f, NULL),
         AVR_E_INVALID, "capacity");
  expect("compact: capacity > R chunk",
         avr_march_compact_counted(f, f, f, mask, offs, 4, 100, 0, 16, cnt, 65, f, f, NULL), AVR_E_INVALID, "capacity");
  expect("compact: null ro", avr_march_compact_counted(NULL, f, f, mask, offs, 4, 100, 0, 16, cnt, 64, f, f, NULL),
         AVR_E_INVALID, "null");
  expect("compact: null rd", avr_march_compact_counted(f, NULL, f, mask, offs, 4, 100, 0, 16, cnt, 64, f, f, NULL),
         AVR_E_INVALID, "null");
  expect("compact: null z", avr_march_compact_counted(f, f, NULL, mask, offs, 4, 100, 0, 16, cnt, 64, f, f, NULL),
         AVR_E_INVALID, "null");
  expect("compact: null mask", avr_march_compact_counted(f, f, f, NULL, offs, 4, 100, 0, 16, cnt, 64, f, f, NULL),
         AVR_E_INVALID, "null");
  expect("compact: null offsets", avr_march_compact_counted(f, f, f, mask, NULL, 4, 100, 0, 16, cnt, 64, f, f, NULL),
         AVR_E_INVALID, "null");
  expect("compact: null n_live", avr_march_compact_counted(f, f, f, mask, offs, 4, 100, 0, 16, NULL, 64, f, f, NULL),
         AVR_E_INVALID, "null");
  expect("compact: null xyz", avr_march_compact_counted(f, f, f, mask, offs, 4, 100, 0, 16, cnt, 64, NULL, f, NULL),
         AVR_E_INVALID, "null");
  expect("compact: null viewdirs",
         avr_march_compact_counted(f, f, f, mask, offs, 4, 100, 0, 16, cnt, 64, f, NULL, NULL), AVR_E_INVALID, "null");
  expect("compact: misaligned n_live",
         avr_march_compact_counted(f, f, f, mask, offs, 4, 100, 0, 16, (int64_t*)odd8, 64, f, f, NULL), AVR_E_INVALID,
         "aligned");
  expect("compact: misaligned offsets",
         avr_march_compact_counted(f, f, f, mask, (int64_t*)odd8, 4, 100, 0, 16, cnt, 64, f, f, NULL), AVR_E_INVALID,
         "aligned");
  expect("compact: capacity = 0",
         avr_march_compact_counted(NULL, NULL, NULL, NULL, NULL, 4, 100, 0, 16, NULL, 0, NULL, NULL, NULL), AVR_OK,
         NULL);
  expect("compact: R = 0",
         avr_march_compact_counted(NULL, NULL, NULL, NULL, NULL, 0, 100, 0, 16, NULL, 0, NULL, NULL, NULL), AVR_OK,
         NULL);

  /* avr_march_composite_masked(z, field_c, mask, offsets, n_live, capacity, R, N, c0, chunk, infinity, t_stop,
   *                            state, evaluated, accumulate, stream) */
  expect("composite: R < 0",
         avr_march_composite_masked(f, f, mask, offs, cnt, 0, -1, 100, 0, 64, 1.8f, 0.f, st, cnt, 0, NULL),
         AVR_E_INVALID, "n_rays");
  expect("composite: chunk 0",
         avr_march_composite_masked(f, f, mask, offs, cnt, 0, 4, 100, 0, 0, 1.8f, 0.f, st, cnt, 0, NULL),
         AVR_E_INVALID, "chunk");
  expect("composite: chunk 65",
         avr_march_composite_masked(f, f, mask, offs, cnt, 4, 4, 100, 0, 65, 1.8f, 0.f, st, cnt, 0, NULL),
         AVR_E_INVALID, "chunk");
  expect("composite: window past N",
         avr_march_composite_masked(f, f, mask, offs, cnt, 4, 4, 100, 64, 37, 1.8f, 0.f, st, cnt, 0, NULL),
         AVR_E_INVALID, "n_samples");
  expect("composite: capacity < 0",
         avr_march_composite_masked(f, f, mask, offs, cnt, -1, 4, 100, 0, 64, 1.8f, 0.f, st, cnt, 0, NULL),
         AVR_E_INVALID, "capacity");
  expect("composite: capacity > R chunk",
         avr_march_composite_masked(f, f, mask, offs, cnt, 257, 4, 100, 0, 64, 1.8f, 0.f, st, cnt, 0, NULL),
         AVR_E_INVALID, "capacity");
  expect("composite: null z",
         avr_march_composite_masked(NULL, f, mask, offs, cnt, 256, 4, 100, 0, 64, 1.8f, 0.f, st, cnt, 0, NULL),
         AVR_E_INVALID, "null");
  expect("composite: null field_c",
         avr_march_composite_masked(f, NULL, mask, offs, cnt, 256, 4, 100, 0, 64, 1.8f, 0.f, st, cnt, 0, NULL),
         AVR_E_INVALID, "null");
  expect("composite: null mask",
         avr_march_composite_masked(f, f, NULL, offs, cnt, 256, 4, 100, 0, 64, 1.8f, 0.f, st, cnt, 0, NULL),
         AVR_E_INVALID, "null");
  expect("composite: null offsets",
         avr_march_composite_masked(f, f, mask, NULL, cnt, 256, 4, 100, 0, 64, 1.8f, 0.f, st, cnt, 0, NULL),
         AVR_E_INVALID, "null");
  expect("composite: null n_live",
         avr_march_composite_masked(f, f, mask, offs, NULL, 256, 4, 100, 0, 64, 1.8f, 0.f, st, cnt, 0, NULL),
         AVR_E_INVALID, "null");
  expect("composite: null state",
         avr_march_composite_masked(f, f, mask, offs, cnt, 256, 4, 100, 0, 64, 1.8f, 0.f, NULL, cnt, 0, NULL),
         AVR_E_INVALID, "null");
  expect("composite: null evaluated",
         avr_march_composite_masked(f, f, mask, offs, cnt, 256, 4, 100, 0, 64, 1.8f, 0.f, st, NULL, 0, NULL),
         AVR_E_INVALID, "null");
  expect("composite: misaligned n_live",
         avr_march_composite_masked(f, f, mask, offs, (int64_t*)odd8, 256, 4, 100, 0, 64, 1.8f, 0.f, st, cnt, 0, NULL),
         AVR_E_INVALID, "aligned");
  expect("composite: misaligned evaluated",
         avr_march_composite_masked(f, f, mask, offs, cnt, 256, 4, 100, 0, 64, 1.8f, 0.f, st, (int64_t*)odd8, 1, NULL),
         AVR_E_INVALID, "aligned");
  expect("composite: misaligned field_c",
         avr_march_composite_masked(f, f + 2, mask, offs, cnt, 256, 4, 100, 0, 64, 1.8f, 0.f, st, cnt, 0, NULL),
         AVR_E_INVALID, "16-B");
  expect("composite: R = 0",
         avr_march_composite_masked(NULL, NULL, NULL, NULL, NULL, 0, 0, 100, 0, 64, 1.8f, 0.f, NULL, NULL, 0, NULL),
         AVR_OK, NULL);

  for (int k = 0; k < 16; ++k)
    if (host[k] != 0.f) {   /* no refused or empty call wrote anything */
      fprintf(stderr, "FAIL host buffer written\n");
      ++failures;
      break;
    }
  free(g);
  printf("march_device_abi_check: %d failure(s)\n", failures);
  return failures;
}
