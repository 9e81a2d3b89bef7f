/* The stereo control's device-free part (run by tests/test_stereo_cpu.py).  Built from this file, csrc/fmd_recv.c and csrc/fmd_error.c as sources, with
 * no device library, under the sanitizers: fmdk_stereo_plan is private and not exported from the library.
 *
 * Reads lines from stdin and answers each with one line:
 *   p <pcm_stride> <pilot_per_block> <hold_blocks> <reserved0> <pilot_on> <pilot_off> <blend_lo> <blend_hi> <slew> <r0> <r1> <r2>
 *     (the five floats as hex words)                   -> ok <thr_on> <thr_off> <inv_mz> <inv_span> as hex words   (or "refused <rc> <message>")
 *   s                                                  -> sizeof of config, state, info, meter */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fmd_internal.h"

static char line[512];

static uint32_t word_of(float f) {
  uint32_t w;
  memcpy(&w, &f, 4);
  return w;
}

int main(void) {
  while (fgets(line, sizeof line, stdin)) {
    if (line[0] == 'p') {
      fmd_stereo_config c;
      fmdk_stereo_k k;
      uint32_t w[5];
      memset(&c, 0, sizeof c);
      if (sscanf(line + 1, "%d %d %d %d %x %x %x %x %x %d %d %d", &c.pcm_stride, &c.pilot_per_block, &c.hold_blocks, &c.reserved0, &w[0], &w[1], &w[2],
                 &w[3], &w[4], &c.reserved[0], &c.reserved[1], &c.reserved[2]) != 12)
        return 2;
      memcpy(&c.pilot_on, &w[0], 4);
      memcpy(&c.pilot_off, &w[1], 4);
      memcpy(&c.blend_lo, &w[2], 4);
      memcpy(&c.blend_hi, &w[3], 4);
      memcpy(&c.slew, &w[4], 4);
      const int rc = fmdk_stereo_plan(&c, &k);
      if (rc) printf("refused %d %s\n", rc, fmd_last_error());
      else printf("ok %08x %08x %08x %08x\n", word_of(k.thr_on), word_of(k.thr_off), word_of(k.inv_mz), word_of(k.inv_span));
    } else if (line[0] == 's') {
      printf("%zu %zu %zu %zu\n", sizeof(fmd_stereo_config), sizeof(fmd_stereo_state), sizeof(fmd_stereo_info), sizeof(fmd_stereo_meter));
    } else {
      return 2;
    }
  }
  return 0;
}
