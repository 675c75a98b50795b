/* avr_adaptive_front's argument checks (include/avr.h) under a host AddressSanitizer build of the library
 * (`make -C adaptive-volume-rendering_amd asan-adaptive`, the build tests/abi_check.c uses). Every call below is
 * rejected with AVR_E_INVALID, or is a no-op, BEFORE any HIP call, so the program runs without a GPU; ASan watches
 * the reads of the host view array (heap-allocated at its exact size) and the formatting of the error strings.
 * Exit status: number of failed checks. Run by tests/test_cpu_adaptive_abi.py.                                  */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "abi_check_common.h"

/* the call's arguments, so that each check changes one of them */
typedef struct {
  const avr_view_desc* views;
  int n_scenes;
  const float *tables, *w_hh, *b_ih, *b_hh, *w_out, *b_out, *ro, *rd, *init, *noise;
  const int64_t* ids;
  int64_t n_per_scene;
  int steps, n_band;
  float *world, *z, *init_out, *noise_out;
} args_t;

static int run(const args_t* a) {
  return avr_adaptive_front(a->views, a->n_scenes, a->tables, a->w_hh, a->b_ih, a->b_hh, a->w_out, a->b_out, a->ro,
                            a->rd, a->init, a->noise, 99u, 1000u, a->ids, a->n_per_scene, a->steps, 0.05f, a->n_band,
                            a->world, a->z, a->init_out, a->noise_out, NULL);
}

int main(void) {
  enum { NS = 3 };
  float host[8] = {0};   /* stands in for device memory: never dereferenced by a refused call */
  int64_t ids[8] = {0};
  avr_view_desc* views = (avr_view_desc*)calloc(NS, sizeof(avr_view_desc));
  if (!views) return 99;
  for (int s = 0; s < NS; ++s) {
    views[s].latent_h = views[s].latent_w = 8;
    views[s].image_shape[0] = views[s].image_shape[1] = 128.f;
    views[s].latent_scaling[0] = views[s].latent_scaling[1] = 2.f;
  }
  const args_t ok = {views, NS, host, host, host, host, host, host, host, host, host, host, ids, 5, 10, 20,
                     host, host, host, host};
  args_t a;

  if (avr_version() != AVR_ABI_VERSION || AVR_ABI_VERSION != 18) {   /* the entry is an addition within ABI 18 */
    fprintf(stderr, "FAIL version %d\n", avr_version());
    ++failures;
  }
  a = ok; a.n_per_scene = 0;
  expect("no rays", run(&a), AVR_OK, NULL);
  a = ok; a.n_per_scene = 0; a.n_band = 0; a.z = NULL; a.init = NULL; a.noise = NULL; a.ids = NULL;
  expect("no rays, optional arrays absent", run(&a), AVR_OK, NULL);

  a = ok; a.n_scenes = 0;
  expect("n_scenes = 0", run(&a), AVR_E_INVALID, "n_scenes");
  a = ok; a.n_scenes = AVR_MAX_SCENES + 1;   /* refused before views[NS] would be read */
  expect("n_scenes too large", run(&a), AVR_E_INVALID, "n_scenes");
  a = ok; a.n_band = -1;
  expect("n_band < 0", run(&a), AVR_E_INVALID, "n_band");
  a = ok; a.n_band = 65;
  expect("n_band > 64", run(&a), AVR_E_INVALID, "n_band");
  a = ok; a.z = NULL;
  expect("n_band > 0 without z_sorted", run(&a), AVR_E_INVALID, "z_sorted");
  a = ok; a.steps = -1;
  expect("steps < 0", run(&a), AVR_E_INVALID, "steps");
  a = ok; a.n_per_scene = -1;
  expect("n_per_scene < 0", run(&a), AVR_E_INVALID, "n_per_scene");
  a = ok; a.n_per_scene = 0; a.n_band = 65;   /* sizes are checked before the empty call returns */
  expect("no rays, bad n_band", run(&a), AVR_E_INVALID, "n_band");

  /* every required pointer in turn */
  const void** slots[10];
  a = ok;
  slots[0] = (const void**)&a.views; slots[1] = (const void**)&a.tables; slots[2] = (const void**)&a.w_hh;
  slots[3] = (const void**)&a.b_ih; slots[4] = (const void**)&a.b_hh; slots[5] = (const void**)&a.w_out;
  slots[6] = (const void**)&a.b_out; slots[7] = (const void**)&a.ro; slots[8] = (const void**)&a.rd;
  slots[9] = (const void**)&a.world;
  for (int s = 0; s < 10; ++s) {
    const void* keep = *slots[s];
    *slots[s] = NULL;
    expect("null pointer", run(&a), AVR_E_INVALID, "null");
    *slots[s] = keep;
  }
  /* scenes whose latent maps differ in size: the check walks all NS views and not one more */
  views[NS - 1].latent_w = 4;
  a = ok;
  expect("latent sizes differ", run(&a), AVR_E_INVALID, "latent");
  views[NS - 1].latent_w = 8;

  free(views);
  printf("adaptive_abi_check: %d failure(s)\n", failures);
  return failures;
}
