/* The launch plan and the resolved kernel arguments without a device (run by tests/test_launch_plan.py and tests/test_resolve_cpu.py).  Linked against
 * the resolver and the fused kernel objects directly (csrc/fmd_resolve.o, fmd_error.o, fmd_kernels_exact / _fast / _mfma.o): fmdk_plan_launch, fmdk_resolve and fmdk_workers_per_cu are private and
 * not exported from the library.
 *
 * Reads lines from stdin and answers each with one line:
 *   c <fmd_config as hex bytes> <n_streams> <n_blocks> <n_cus> <dbg>
 *       -> family ex mode half mx kernel_per_simd workers_per_cu warm_tiles n_chunks     (or "refused <rc>")
 *   v <ex> <mode> <half> <mx> <dbg>
 *       -> kernel_per_simd workers_per_cu                                                 (the budgets of one instantiation)
 *   k <fmd_config as hex bytes> <n_streams> <n_blocks> <n_cus> <dbg> [<fmd_taps as hex bytes>]
 *       -> 64-bit FNV-1a of the launch's fmdk_params (dec_tables NULL), and of the decimating tables or "-"         (or "refused <rc>")
 *   t <fmd_config as hex bytes> [<fmd_taps as hex bytes>]
 *       -> family dec_p dec_wide ci_qf[0] ci_qf[1] ci_qf[2] g_qf gq[0] .. gq[89] <the decimating tables as hex bytes, or "-">   (or "refused <rc>") */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fmd_internal.h"

static int unhex(const char *hex, void *out, size_t n) {
  if (strlen(hex) != 2 * n) return -1;
  for (size_t i = 0; i < n; i++) {
    unsigned x;
    if (sscanf(hex + 2 * i, "%2x", &x) != 1) return -1;
    ((unsigned char *)out)[i] = (unsigned char)x;
  }
  return 0;
}

static unsigned long long fnv1a(const void *p, size_t n) {
  unsigned long long h = 0xcbf29ce484222325ULL;
  for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char *)p)[i]) * 0x100000001b3ULL;
  return h;
}

static char line[8192], hex[2 * sizeof(fmd_config) + 2], thex[2 * sizeof(fmd_taps) + 2];
static fmdk_resolved r;

int main(void) {
  while (fgets(line, sizeof line, stdin)) {
    const char kind = line[0];
    fmd_config c;
    fmd_taps t, *taps = NULL;
    int ns = 1, nb = 1, cus = 1, dbg = 0, n = 0;
    thex[0] = 0;
    if (kind == 'c' || kind == 'k') {
      n = sscanf(line + 1, "%89s %d %d %d %d %3217s", hex, &ns, &nb, &cus, &dbg, thex);
      if (n < 5 || (n == 6 && kind == 'c')) return 2;
    } else if (kind == 't') {
      if (sscanf(line + 1, "%89s %3217s", hex, thex) < 1) return 2;
    }
    if (kind == 'c' || kind == 'k' || kind == 't') {
      if (unhex(hex, &c, sizeof c)) return 2;
      if (thex[0]) {
        if (unhex(thex, &t, sizeof t)) return 2;
        taps = &t;
      }
    }
    if (kind == 'c') {
      fmdk_plan p;
      const int rc = fmdk_plan_launch(&c, NULL, ns, nb, cus, dbg, &p);
      if (rc) printf("refused %d\n", rc);
      else
        printf("%d %d %d %d %d %d %d %d %d\n", p.family, p.v.ex, p.v.mode, p.v.half, p.v.mx, p.kernel_per_simd, p.workers_per_cu, p.warm_tiles,
               p.n_chunks);
    } else if (kind == 'k' || kind == 't') {
      const int rc = fmdk_resolve(&c, taps, &r);
      if (rc) {
        printf("refused %d\n", rc);
        continue;
      }
      size_t bytes = 0;
      uint8_t *tab = r.var.mx == 2 ? fmdk_dec_tables(&r, &bytes) : NULL;        /* (the variant that reads them) */
      if (r.var.mx == 2 && !tab) return 3;
      if (kind == 'k') {
        const fmdk_params kp = fmdk_launch_params(&r, ns, cus, 0, nb, dbg);
        printf("%016llx ", fnv1a(&kp, sizeof kp));
        if (tab) printf("%016llx\n", fnv1a(tab, bytes));
        else printf("-\n");
      } else {
        printf("%d %d %d %d %d %d %d", r.cfg.math, r.kp.dec_p, r.kp.dec_wide, r.kp.ci_qf[0], r.kp.ci_qf[1], r.kp.ci_qf[2], r.kp.g_qf);
        for (int u = 0; u < 90; u++) printf(" %d", r.kp.gq[u]);
        printf(" ");
        for (size_t i = 0; i < bytes; i++) printf("%02x", tab[i]);
        puts(tab ? "" : "-");
      }
      free(tab);
    } else if (kind == 'v') {
      int ex, mode, half, mx, k = 0;
      if (sscanf(line + 1, "%d %d %d %d %d", &ex, &mode, &half, &mx, &dbg) != 5) return 2;
      const fmdk_variant v = {(int8_t)ex, (int8_t)mode, (int8_t)half, (int8_t)mx};
      const int w = fmdk_workers_per_cu(&v, dbg, &k);
      printf("%d %d\n", k, w);
    } else {
      return 2;
    }
  }
  return 0;
}
