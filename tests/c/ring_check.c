/* The ingest ring's accounting without a device (run by tests/test_ring_cpu.py).  Compiled together with csrc/fmd_ring.c and nothing else of the
 * library, with no ROCm include path or library: that it builds this way is the proof that the unit is device-free.  The ring's memory is a
 * malloc of exactly its capacity, and every transfer a malloc of exactly its length, so a sanitised build sees any byte written or read beside them.
 *
 * Reads one command per line from stdin and answers each with one line, `rpos wpos size inflight debt dropped` and then what the command returns:
 *   new <cap> <mode>          an empty ring of cap bytes, mode = FMD_OVERFLOW_DROP_OLDEST (0) or FMD_OVERFLOW_REFERENCE (1)
 *   push <n> <seed>           fmd_ingest_callback with n bytes: x = seed, then per byte x = 1664525 x + 1013904223 (mod 2^32), byte = x >> 24
 *   take <n>                  fmdk_ring_take            -> from
 *   release <n>               fmdk_ring_release
 *   untake <n> <old>          fmdk_ring_untake
 *   pop <n>                   fmd_ingest_pop            -> the count returned, and the bytes in hex
 *   peek <from> <n>           the n bytes at `from` (fmdk_ring_split), no change           -> the bytes in hex */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fmd_ring.h"

int fmd_fail(int code, const char *fmt, ...) { (void)fmt; return code; }

static struct fmd_ingest g;

static void put_hex(const uint8_t *p, uint32_t n) {
  putchar(' ');
  for (uint32_t i = 0; i < n; i++) printf("%02x", p[i]);
}

int main(void) {
  char line[128], cmd[16];
  int live = 0;
  while (fgets(line, sizeof line, stdin)) {
    unsigned a = 0, b = 0;
    const int n = sscanf(line, "%15s %u %u", cmd, &a, &b);
    if (n < 2 || (!live && strcmp(cmd, "new") != 0)) return 2;
    uint8_t *buf = NULL;
    uint32_t ret = 0, shown = 0, first = 0;
    if (!strcmp(cmd, "new") && n == 3 && a > 0) {
      if (live) { fmdk_ring_fini(&g); free(g.ring); }
      memset(&g, 0, sizeof g);
      uint8_t *mem = (uint8_t *)calloc(a, 1);
      if (!mem) return 3;
      fmdk_ring_init(&g, mem, a);
      g.unbound = 1;
      g.stream = -1;
      if (fmd_ingest_set_overflow(&g, (int)b)) return 2;
      live = 1;
    } else if (!strcmp(cmd, "push") && n == 3 && a > 0) {
      if (!(buf = (uint8_t *)malloc(a))) return 3;
      uint32_t x = b;
      for (unsigned i = 0; i < a; i++) buf[i] = (uint8_t)((x = 1664525u * x + 1013904223u) >> 24);
      fmd_ingest_callback(buf, a, &g);
    } else if (!strcmp(cmd, "take") && n == 2) {
      ret = fmdk_ring_take(&g, a);
    } else if (!strcmp(cmd, "release") && n == 2) {
      fmdk_ring_release(&g, a);
    } else if (!strcmp(cmd, "untake") && n == 3) {
      fmdk_ring_untake(&g, a, b);
    } else if (!strcmp(cmd, "pop") && n == 2 && a > 0) {
      if (!(buf = (uint8_t *)malloc(a))) return 3;
      ret = shown = fmd_ingest_pop(&g, buf, a);
    } else if (!strcmp(cmd, "peek") && n == 3 && a < g.cap && b <= g.cap) {
      if (!(buf = (uint8_t *)malloc(b ? b : 1))) return 3;
      const uint8_t *ring = fmdk_ring_split(&g, a, b, &first);
      memcpy(buf, ring + a, first);
      memcpy(buf + first, ring, b - first);
      shown = b;
    } else {
      return 2;
    }
    printf("%u %u %u %u %u %llu", g.rpos, g.wpos, g.size, g.inflight, g.debt, (unsigned long long)g.dropped);
    if (!strcmp(cmd, "take") || !strcmp(cmd, "pop")) printf(" %u", ret);
    if (!strcmp(cmd, "pop") || !strcmp(cmd, "peek")) put_hex(buf, shown);
    putchar('\n');
    fflush(stdout);
    free(buf);
  }
  if (live) { fmdk_ring_fini(&g); free(g.ring); }
  return 0;
}
