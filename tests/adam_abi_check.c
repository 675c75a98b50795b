/* avr_adam_step's argument checks (include/avr.h, ABI 18) under a host AddressSanitizer build of the library
 * (`make -C adaptive-volume-rendering_amd asan-adam`, the build tests/abi_check.c uses). Every call below is
 * rejected with AVR_E_INVALID, or is a no-op, BEFORE any HIP call, so the program runs without a GPU; ASan
 * watches the reads of the host tensor array (heap-allocated at its exact size, the invalid entry last) and the
 * formatting of the error strings. Exit status: number of failed checks. Run by tests/test_cpu_adam.py.      */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "abi_check_common.h"

int main(void) {
  enum { N = 5 };
  float host[8] = {0};   /* stands in for device memory: never dereferenced by a refused call */
  float step = 3.f;
  avr_adam_tensor* t = (avr_adam_tensor*)malloc(N * sizeof(avr_adam_tensor));
  if (!t) return 99;
  for (int k = 0; k < N; ++k) t[k] = (avr_adam_tensor){host, host, host, host, 8};
  t[1].numel = 0;                                                /* an empty entry is skipped ...          */
  t[1].param = NULL;                                             /* ... whatever its pointers              */
  const double lr = 1e-3, b1 = 0.9, b2 = 0.999, eps = 1e-8, wd = 0.0;

  if (avr_version() != AVR_ABI_VERSION || AVR_ABI_VERSION < 18) {
    fprintf(stderr, "FAIL version %d\n", avr_version());
    ++failures;
  }
  expect("no tensors", avr_adam_step(NULL, 0, lr, b1, b2, eps, wd, NULL, NULL), AVR_OK, NULL);
  expect("no tensors, list given", avr_adam_step(t, 0, lr, b1, b2, eps, wd, &step, NULL), AVR_OK, NULL);
  expect("negative count", avr_adam_step(t, -1, lr, b1, b2, eps, wd, &step, NULL), AVR_E_INVALID, "n_tensors");
  expect("null list", avr_adam_step(NULL, N, lr, b1, b2, eps, wd, &step, NULL), AVR_E_INVALID, "null");
  expect("null step", avr_adam_step(t, N, lr, b1, b2, eps, wd, NULL, NULL), AVR_E_INVALID, "null");

  expect("lr", avr_adam_step(t, N, -1e-3, b1, b2, eps, wd, &step, NULL), AVR_E_INVALID, "lr");
  expect("beta1 = 1", avr_adam_step(t, N, lr, 1.0, b2, eps, wd, &step, NULL), AVR_E_INVALID, "beta1");
  expect("beta1 < 0", avr_adam_step(t, N, lr, -0.1, b2, eps, wd, &step, NULL), AVR_E_INVALID, "beta1");
  expect("beta2 = 1", avr_adam_step(t, N, lr, b1, 1.0, eps, wd, &step, NULL), AVR_E_INVALID, "beta2");
  expect("beta2 < 0", avr_adam_step(t, N, lr, b1, -0.5, eps, wd, &step, NULL), AVR_E_INVALID, "beta2");
  expect("eps", avr_adam_step(t, N, lr, b1, b2, -1e-8, wd, &step, NULL), AVR_E_INVALID, "eps");
  expect("weight_decay", avr_adam_step(t, N, lr, b1, b2, eps, -1e-2, &step, NULL), AVR_E_INVALID, "weight_decay");

  /* the invalid entry is the last one of the array: the check walks all N entries and not one more */
  t[N - 1].numel = -4;
  expect("negative numel", avr_adam_step(t, N, lr, b1, b2, eps, wd, &step, NULL), AVR_E_INVALID, "numel");
  t[N - 1].numel = 8;
  float** slots[4] = {&t[N - 1].param, (float**)&t[N - 1].grad, &t[N - 1].exp_avg, &t[N - 1].exp_avg_sq};
  for (int s = 0; s < 4; ++s) {
    *slots[s] = NULL;
    expect("null pointer in the last entry", avr_adam_step(t, N, lr, b1, b2, eps, wd, &step, NULL), AVR_E_INVALID,
           "null");
    *slots[s] = host;
  }
  if (step != 3.f) {   /* no refused or empty call touched the counter */
    fprintf(stderr, "FAIL step counter changed to %g\n", step);
    ++failures;
  }
  free(t);
  printf("adam_abi_check: %d failure(s)\n", failures);
  return failures;
}
