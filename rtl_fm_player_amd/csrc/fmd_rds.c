/*
 * fmd_rds.c - what the RDS receiver needs no device for (include/fmdemod_mi355x.h, "RDS receiver"): the range check, the
 * integer geometry of the bit ownership, the matched filter's default taps, the timing table - used by fmd_objects.c - and the block / group
 * decoder with the PI / PTY / PS collector.  No GPU header, no GPU call, no allocation: tests/c/rds_check.c links this unit alone.
 */
#define _GNU_SOURCE
#include <math.h>
#include <string.h>

#include "fmd_internal.h"

/* ---- geometry: integers only ------------------------------------------------------------------------------------------------------------ */

static int64_t gcd64(int64_t a, int64_t b) {
  while (b) { const int64_t t = a % b; a = b; b = t; }
  return a;
}

void fmdk_rds_geometry(int rate_z, int block_z, fmdk_rds_geom *g) {
  g->two_rz = 2 * rate_z;
  g->pw = (int32_t)(g->two_rz / gcd64(FMDK_RDS_Q, g->two_rz));
  g->hh = (rate_z + FMDK_RDS_Q - 1) / FMDK_RDS_Q;               /* ceil(S / 2) */
  g->lb = g->hh + 2;                                            /* L */
  g->hb = (g->two_rz + FMDK_RDS_Q - 1) / FMDK_RDS_Q;            /* ceil(S) */
  g->hy = g->lb + g->hb + g->hh;
  /* the largest count of a block: the bits with e + j 2 rate_z < 2375 Bz for the smallest e = 0 */
  const int32_t most = (int32_t)(((int64_t)FMDK_RDS_Q * block_z + g->two_rz - 1) / g->two_rz);
  g->slot = (most + 3) & ~3;
}

int fmdk_rds_check(const fmd_rds_config *c) {
  if (!c) return fmd_fail(FMD_E_ARG, "RDS config is NULL");
  if (c->rate_z <= 0 || c->rate_z % 125) return fmd_fail(FMD_E_UNSUPPORTED, "rate_z must be a positive multiple of 125 (got %d)", c->rate_z);
  if (2LL * c->rate_z < 10LL * FMDK_RDS_Q || 2LL * c->rate_z > 32LL * FMDK_RDS_Q)
    return fmd_fail(FMD_E_UNSUPPORTED, "rate_z %d gives %.2f samples per bit: 10 .. 32 are supported", c->rate_z, 2.0 * c->rate_z / FMDK_RDS_Q);
  if (c->n_taps < 16 || c->n_taps > FMD_RDS_MAX_TAPS || (c->n_taps & 3))
    return fmd_fail(FMD_E_UNSUPPORTED, "n_taps must be a multiple of 4 in 16 .. %d (got %d)", FMD_RDS_MAX_TAPS, c->n_taps);
  fmdk_rds_geom g;
  fmdk_rds_geometry(c->rate_z, c->block_z > 0 ? c->block_z : 4, &g);
  if (c->block_z <= 0 || (c->block_z & 3) || c->block_z < c->n_taps || c->block_z < g.hy || c->block_z > FMDK_RDS_MAX_BLOCK)
    return fmd_fail(FMD_E_UNSUPPORTED, "block_z must be a multiple of 4 in max(n_taps %d, lookback %d) .. %d (got %d)", c->n_taps, g.hy, FMDK_RDS_MAX_BLOCK, c->block_z);
  if (g.pw > FMD_RDS_MAX_PERIOD || g.hy > FMD_RDS_MAX_YHIST) return fmd_fail(FMD_E_UNSUPPORTED, "timing period %d or lookback %d beyond the built range", g.pw, g.hy);
  if (c->avg_blocks < 1) return fmd_fail(FMD_E_UNSUPPORTED, "avg_blocks must be at least 1 (got %d)", c->avg_blocks);
  if (c->max_blocks < 1) return fmd_fail(FMD_E_UNSUPPORTED, "max_blocks must be at least 1 (got %d)", c->max_blocks);
  return FMD_OK;
}

/* ---- taps and table: in double, rounded once ------------------------------------------------------------------------------------------- */

static double sinc_pi(double x) {
  const double pi = 3.14159265358979323846;
  return x == 0.0 ? 1.0 : sin(pi * x) / (pi * x);
}

/* the shaped impulse, t in units of Td: the inverse transform of cos(pi f Td / 4) on |f| <= 2 / Td, up to a constant factor */
static double rds_h(double t) { return sinc_pi(4.0 * t + 0.5) + sinc_pi(4.0 * t - 0.5); }

int fmd_rds_design(const fmd_rds_config *cfg, float *taps) {
  if (!taps) return fmd_fail(FMD_E_ARG, "taps is NULL");
  const int rc = fmdk_rds_check(cfg);
  if (rc) return rc;
  const int T = cfg->n_taps;
  double p[FMD_RDS_MAX_TAPS], e = 0.0;
  for (int k = 0; k < T; k++) {
    const double t = (0.5 * (double)(T - 1) - (double)k) * 1187.5 / (double)cfg->rate_z;      /* in bit periods */
    p[k] = rds_h(t + 0.25) - rds_h(t - 0.25);
    e += p[k] * p[k];
  }
  for (int k = 0; k < T; k++) taps[k] = (float)(p[k] / e);
  return FMD_OK;
}

void fmdk_rds_table(const fmd_rds_config *c, float *tab) {
  const double two_pi = 6.283185307179586476925286766559;
  fmdk_rds_geom g;
  fmdk_rds_geometry(c->rate_z, c->block_z, &g);
  for (int i = 0; i < g.pw; i++) {
    const double a = two_pi * (double)(((int64_t)i * FMDK_RDS_Q) % g.two_rz) / (double)g.two_rz;
    tab[2 * i] = (float)cos(a);
    tab[2 * i + 1] = (float)(-sin(a));
  }
}

/* ---- block and group decoder ------------------------------------------------------------------------------------------------------------ */

#define RDS_POLY 0x5B9u                              /* x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1 */
static const uint16_t rds_offset[5] = {0x0FC, 0x198, 0x168, 0x1B4, 0x350};      /* A, B, C, D, C' */

/* remainder of the 26-bit word mod g(x): for a block (information x^10 + checkword + offset word) it is the offset word */
static uint32_t rds_rem(uint32_t w) {
  for (int i = 25; i >= 10; i--)
    if (w & (1u << i)) w ^= RDS_POLY << (i - 10);
  return w & 0x3FFu;
}

/* the position 0..3 whose offset word r is (C' reads 2 with *cprime set), -1: none */
static int rds_position(uint32_t r, int *cprime) {
  *cprime = 0;
  for (int i = 0; i < 4; i++)
    if (r == rds_offset[i]) return i;
  if (r == rds_offset[4]) { *cprime = 1; return 2; }
  return -1;
}

void fmd_rds_decoder_init(fmd_rds_decoder *dec) {
  if (!dec) return;
  memset(dec, 0, sizeof(*dec));
  memset(dec->hpos, -1, sizeof(dec->hpos));
}

static void rds_store(fmd_rds_decoder *d, int pos, uint16_t word) {
  d->blk[pos] = word;
  d->ok_mask |= (uint8_t)(1u << pos);
}

int fmd_rds_decoder_push(fmd_rds_decoder *dec, const float *soft, int n, fmd_rds_group *out, int max_out) {
  if (!dec || (!soft && n > 0) || n < 0 || max_out < 0 || (!out && max_out > 0)) return fmd_fail(FMD_E_ARG, "bad argument");
  int ng = 0, i = 0;
  for (; i < n; i++) {
    if (ng == max_out && (!dec->synced || (dec->pos == 3 && dec->cnt == 25))) break;      /* the next bit could complete a group with no room for it */
    dec->reg = ((dec->reg << 1) | (soft[i] < 0.0f ? 1u : 0u)) & 0x3FFFFFFu;
    if (dec->fill < 26) dec->fill++;
    dec->bits++;
    if (!dec->synced) {
      const int h = dec->hidx;                                           /* this slot still holds what was seen 26 bits ago */
      dec->hidx = h == 25 ? 0 : h + 1;
      const int before = dec->hpos[h];
      const uint16_t before_word = dec->hword[h];
      int cp;
      const int pos = dec->fill < 26 ? -1 : rds_position(rds_rem(dec->reg), &cp);
      dec->hpos[h] = (int8_t)pos;
      dec->hword[h] = (uint16_t)(dec->reg >> 10);
      if (pos < 0 || before < 0 || ((before + 1) & 3) != pos) continue;
      /* two valid blocks 26 bits apart, in cyclic order: in sync */
      dec->synced = 1;
      dec->n_sync++;
      dec->bad_run = 0;
      dec->ok_mask = 0;
      memset(dec->blk, 0, sizeof(dec->blk));
      if (pos > 0) rds_store(dec, pos - 1, before_word);                 /* (pos 0: the block before closed a group that was never begun) */
      dec->pos = pos;
      dec->cnt = 26;
      memset(dec->hpos, -1, sizeof(dec->hpos));
    } else if (++dec->cnt < 26) {
      continue;
    }
    /* in sync, a whole block in the register */
    int cp;
    const int pos = rds_position(rds_rem(dec->reg), &cp);
    int ok = pos == dec->pos;
    if (ok && pos == 2 && (dec->ok_mask & 2) && cp != ((dec->blk[1] >> 11) & 1)) ok = 0;       /* C in a version-A group, C' in a version-B group */
    if (ok) {
      rds_store(dec, dec->pos, (uint16_t)(dec->reg >> 10));
      dec->bad_run = 0;
    } else {
      dec->bad_run++;
    }
    dec->cnt = 0;
    if (dec->pos == 3) {
      if (dec->ok_mask) {
        fmd_rds_group *g = &out[ng++];
        memcpy(g->blk, dec->blk, sizeof(g->blk));
        g->ok_mask = dec->ok_mask;
        g->version = (dec->ok_mask & 2) ? (uint8_t)((dec->blk[1] >> 11) & 1) : 255;
      }
      dec->ok_mask = 0;
      memset(dec->blk, 0, sizeof(dec->blk));
    }
    dec->pos = (dec->pos + 1) & 3;
    if (dec->bad_run >= FMD_RDS_SYNC_LOSS) {
      dec->synced = 0;
      dec->n_loss++;
      dec->ok_mask = 0;
    }
  }
  dec->consumed = i;
  return ng;
}

void fmd_rds_info_init(fmd_rds_info *info) {
  if (info) memset(info, 0, sizeof(*info));
}

int fmd_rds_info_update(fmd_rds_info *info, const fmd_rds_group *g) {
  if (!info || !g) return 0;
  int changed = 0;
  if (g->ok_mask & 1) {
    changed |= !info->have_pi || info->pi != g->blk[0];
    info->pi = g->blk[0];
    info->have_pi = 1;
  }
  if (!(g->ok_mask & 2)) return changed;
  const uint16_t b = g->blk[1];
  const uint8_t pty = (uint8_t)((b >> 5) & 31);
  changed |= info->pty != pty;
  info->pty = pty;
  if ((b >> 12) != 0 || !(g->ok_mask & 8)) return changed;             /* group type 0 (A or B): block D carries two characters of the PS name */
  const int seg = b & 3;
  const char c0 = (char)(g->blk[3] >> 8), c1 = (char)(g->blk[3] & 0xFF);
  changed |= info->ps[2 * seg] != c0 || info->ps[2 * seg + 1] != c1 || !(info->ps_mask & (1u << seg));
  info->ps[2 * seg] = c0;
  info->ps[2 * seg + 1] = c1;
  info->ps_mask |= (uint8_t)(1u << seg);
  return changed;
}
