/* The channel tuner's device-free helpers (run by tests/test_tuner_cpu.py).  Built from this file, csrc/fmd_recv.c and csrc/fmd_error.c as sources, with
 * no device library, under the sanitizers: fmdk_tuner_table and fmdk_tuner_channel are private and not exported from the library.
 *
 * Reads lines from stdin and answers each with one line:
 *   t <P>                                              -> the carrier table, 2 P floats as hex words (re, im, re, im ...)
 *   c <rate> <step_hz> <n_sources> <source> <shift> <gain as a hex float word>
 *                                                      -> source sh sh8 sh2k <g as a hex word>      (or "refused <rc> <message>") */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fmd_internal.h"

static char line[256];
static float tab[2 * FMD_TUNER_MAX_PERIOD];

int main(void) {
  while (fgets(line, sizeof line, stdin)) {
    if (line[0] == 't') {
      int P = 0;
      if (sscanf(line + 1, "%d", &P) != 1 || P < 4 || P > FMD_TUNER_MAX_PERIOD || (P & 3)) return 2;
      fmdk_tuner_table(P, tab);
      for (int i = 0; i < 2 * P; i++) {
        uint32_t w;
        memcpy(&w, &tab[i], 4);
        printf("%08x", w);
      }
      puts("");
    } else if (line[0] == 'c') {
      fmd_tuner_config c;
      fmd_tuner_channel ch;
      fmdk_tuner_chan out;
      int ns = 0;
      uint32_t gw = 0;
      memset(&c, 0, sizeof c);
      memset(&ch, 0, sizeof ch);
      if (sscanf(line + 1, "%d %d %d %d %d %x", &c.rate, &c.step_hz, &ns, &ch.source, &ch.shift, &gw) != 6) return 2;
      memcpy(&ch.gain, &gw, 4);
      const int rc = fmdk_tuner_channel(&c, ns, &ch, &out);
      if (rc) {
        printf("refused %d %s\n", rc, fmd_last_error());
      } else {
        memcpy(&gw, &out.g, 4);
        printf("%d %d %d %d %08x\n", out.source, out.sh, out.sh8, out.sh2k, gw);
      }
    } else {
      return 2;
    }
  }
  return 0;
}
