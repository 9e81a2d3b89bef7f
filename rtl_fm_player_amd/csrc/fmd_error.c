/* fmd_error.c - fmd_last_error's thread-local text and fmd_fail, which sets it: the resolver, the receivers' checks and their check programs all link it. */
#define _GNU_SOURCE
#include <stdarg.h>
#include <stdio.h>

#include "fmd_internal.h"

static __thread char g_err[256];

int fmd_fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

const char *fmd_last_error(void) { return g_err; }
