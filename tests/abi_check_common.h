/* What the *_abi_check.c programs share: the failure counter and the check of one refused (or accepted) call --
 * its return code and, for a refusal, that the error string is set and names `needle` (NULL: any text). */
#ifndef AVR_ABI_CHECK_COMMON_H
#define AVR_ABI_CHECK_COMMON_H
#include <stdio.h>
#include <string.h>

#include "avr.h"

static int failures = 0;

static void expect(const char* what, int got, int want, const char* needle) {
  const char* msg = avr_last_error_string();
  if (got != want) {
    fprintf(stderr, "FAIL %s: got %d want %d (%s)\n", what, got, want, msg);
    ++failures;
  } else if (want != AVR_OK && (strlen(msg) == 0 || (needle && !strstr(msg, needle)))) {
    fprintf(stderr, "FAIL %s: error string '%s' lacks '%s'\n", what, msg, needle ? needle : "any text");
    ++failures;
  }
}

#endif
