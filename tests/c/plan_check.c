/* The launch plan without a device (run by tests/test_launch_plan.py).  Linked against the host layer and kernel objects directly
 * (csrc/fmd_host.o, fmd_kernels_*.o): fmdk_plan_launch and fmdk_workers_per_cu are private and not exported from the library.
 *
 * Reads lines from stdin and answers each with one line:
 *   c <fmd_config as hex bytes> <n_streams> <n_blocks> <n_cus> <dbg>
 *       -> family ex mode half mx kernel_per_simd workers_per_cu warm_tiles n_chunks     (or "refused <rc>")
 *   v <ex> <mode> <half> <mx> <dbg>
 *       -> kernel_per_simd workers_per_cu                                                 (the budgets of one instantiation) */
#include <stdio.h>
#include <string.h>

#include "fmd_internal.h"

int main(void) {
  char kind[2], hex[2 * sizeof(fmd_config) + 1];
  while (scanf("%1s", kind) == 1) {
    if (kind[0] == 'c') {
      int ns, nb, cus, dbg;
      if (scanf("%s %d %d %d %d", hex, &ns, &nb, &cus, &dbg) != 5 || strlen(hex) != 2 * sizeof(fmd_config)) return 2;
      fmd_config c;
      unsigned char *p = (unsigned char *)&c;
      for (size_t i = 0; i < sizeof c; i++) {
        unsigned x;
        if (sscanf(hex + 2 * i, "%2x", &x) != 1) return 2;
        p[i] = (unsigned char)x;
      }
      fmdk_plan r;
      const int rc = fmdk_plan_launch(&c, NULL, ns, nb, cus, dbg, &r);
      if (rc) printf("refused %d\n", rc);
      else
        printf("%d %d %d %d %d %d %d %d %d\n", r.family, r.v.ex, r.v.mode, r.v.half, r.v.mx, r.kernel_per_simd, r.workers_per_cu, r.warm_tiles,
               r.n_chunks);
    } else if (kind[0] == 'v') {
      int ex, mode, half, mx, dbg, k = 0;
      if (scanf("%d %d %d %d %d", &ex, &mode, &half, &mx, &dbg) != 5) return 2;
      const fmdk_variant v = {(int8_t)ex, (int8_t)mode, (int8_t)half, (int8_t)mx};
      const int w = fmdk_workers_per_cu(&v, dbg, &k);
      printf("%d %d\n", k, w);
    } else {
      return 2;
    }
  }
  return 0;
}
