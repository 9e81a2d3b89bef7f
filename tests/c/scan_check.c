/* The station finder's device-free part (run by tests/test_scan_cpu.py).  Built from this file, csrc/fmd_recv.c and csrc/fmd_error.c as sources, with
 * no device library, under the sanitizers: fmdk_scan_plan_make is private and not exported from the library.
 *
 * Reads lines from stdin and answers each with one line:
 *   p <rate> <n_bins> <raster_hz> <bw> <min_sep> <floor_permille> <dc_guard> <max_stations> <threshold as a hex float word> <r0> <r1> <r2>
 *       -> ok <C> <cmax> <rank> <n_used> <nb as a hex double word> then per candidate " <first> <count> <w_first> <w_last>" (hex double words)
 *          (or "refused <rc> <message>") */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fmd_internal.h"

static char line[512];
static fmdk_scan_cand cand[FMD_SCAN_MAX_CANDIDATES];

static unsigned long long bits(double x) {
  unsigned long long w;
  memcpy(&w, &x, 8);
  return w;
}

int main(void) {
  while (fgets(line, sizeof line, stdin)) {
    if (line[0] != 'p') return 2;
    fmd_scan_config c;
    fmdk_scan_plan p;
    uint32_t tw = 0;
    memset(&c, 0, sizeof c);
    if (sscanf(line + 1, "%d %d %d %d %d %d %d %d %x %d %d %d", &c.rate, &c.n_bins, &c.raster_hz, &c.bw, &c.min_sep, &c.floor_permille, &c.dc_guard,
               &c.max_stations, &tw, &c.reserved[0], &c.reserved[1], &c.reserved[2]) != 12)
      return 2;
    memcpy(&c.threshold, &tw, 4);
    const int rc = fmdk_scan_plan_make(&c, &p, cand);
    if (rc) {
      printf("refused %d %s\n", rc, fmd_last_error());
      continue;
    }
    if (fmd_scan_candidates(&c) != p.n_cand) return 3;
    printf("ok %d %d %d %d %016llx", p.n_cand, p.cmax, p.rank, p.n_used, bits(p.nb));
    for (int i = 0; i < p.n_cand; i++) printf(" %d %d %016llx %016llx", cand[i].first, cand[i].count, bits(cand[i].w_first), bits(cand[i].w_last));
    puts("");
  }
  return 0;
}
