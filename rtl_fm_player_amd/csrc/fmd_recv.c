/* fmd_recv.c - the device-free part of the receivers beside the batch (subcarrier, tuner, scan, stereo control; the RDS receiver's is fmd_rds.c):
 * range checks with their messages, tap design, carrier and rotation tables, the scan's candidates and the stereo tracker's constants.  No device
 * header, no device call, nothing of a kernel unit: tests/c/scan_check.c, tuner_check.c and stereo_check.c compile this file and fmd_error.c alone. */
#define _GNU_SOURCE
#include <math.h>
#include <string.h>

#include "fmd_internal.h"

static const double pi = 3.14159265358979323846, two_pi = 6.283185307179586476925286766559;
static int64_t gcd64(int64_t a, int64_t b) {
  while (b) { const int64_t t = a % b; a = b; b = t; }
  return a;
}

/* THE low-pass of the receivers (fmd_subc_design, fmd_tuner_design): n_taps taps of a Blackman-windowed sinc with its -6 dB point at bw Hz at a
 * sample rate of `rate`, unit DC gain: in double, rounded once.  The models repeat this order of operations bit for bit. */
static void blackman_sinc(int bw, int rate, int n_taps, float *taps) {
  double s[FMD_SUBC_MAX_TAPS > FMD_TUNER_MAX_TAPS ? FMD_SUBC_MAX_TAPS : FMD_TUNER_MAX_TAPS], sum = 0.0;
  for (int k = 0; k < n_taps; k++) {
    const double x = 2.0 * (double)bw * ((double)k - 0.5 * (double)(n_taps - 1)) / (double)rate;
    const double snc = x == 0.0 ? 1.0 : sin(pi * x) / (pi * x);
    const double a = 2.0 * pi * (double)(k + 1) / (double)(n_taps + 1);
    s[k] = snc * (0.42 - 0.5 * cos(a) + 0.08 * cos(2.0 * a));
    sum += s[k];
  }
  for (int k = 0; k < n_taps; k++) taps[k] = (float)(s[k] / sum);
}

/* ---- MPX subcarrier receiver: what needs no device (include/fmdemod_mi355x.h, "MPX subcarrier receiver"; csrc/subcarrier.inc) ---- */

/* the carrier's period in samples, R / gcd(fc, R) (0 < fc < R assumed) */
int fmdk_subc_period(const fmd_subc_config *c) { return (int)((int64_t)c->rate_in / gcd64(c->fc, c->rate_in)); }

int fmdk_subc_check(const fmd_subc_config *c) {
  if (!c) return fmd_fail(FMD_E_ARG, "subcarrier config is NULL");
  if (c->rate_in <= 0) return fmd_fail(FMD_E_ARG, "rate_in must be positive");
  if (c->fc <= 0 || 2LL * c->fc >= c->rate_in) return fmd_fail(FMD_E_ARG, "fc must lie in 0 < fc < rate_in / 2 (got %d at %d)", c->fc, c->rate_in);
  if (c->bw <= 0 || 2LL * c->bw >= c->rate_in) return fmd_fail(FMD_E_ARG, "bw must lie in 0 < bw < rate_in / 2 (got %d at %d)", c->bw, c->rate_in);
  if (c->n_taps < 16 || c->n_taps > FMD_SUBC_MAX_TAPS || (c->n_taps & 3))
    return fmd_fail(FMD_E_UNSUPPORTED, "n_taps must be a multiple of 4 in 16 .. %d (got %d)", FMD_SUBC_MAX_TAPS, c->n_taps);
  if (c->decim != 4 && c->decim != 8 && c->decim != 16 && c->decim != 32) return fmd_fail(FMD_E_UNSUPPORTED, "decim must be 4, 8, 16 or 32 (got %d)", c->decim);
  if (c->block_samples <= 0 || c->block_samples % c->decim) return fmd_fail(FMD_E_ARG, "block_samples must be a positive multiple of decim (got %d, decim %d)", c->block_samples, c->decim);
  if (c->block_samples < c->n_taps)
    return fmd_fail(FMD_E_UNSUPPORTED, "block_samples %d is shorter than the filter (%d taps): a block's history would reach past the block before it", c->block_samples, c->n_taps);
  if (fmdk_subc_period(c) > FMD_SUBC_MAX_PERIOD)
    return fmd_fail(FMD_E_UNSUPPORTED, "the carrier's period rate_in / gcd(fc, rate_in) = %d samples exceeds %d", fmdk_subc_period(c), FMD_SUBC_MAX_PERIOD);
  return FMD_OK;
}

int fmd_subc_design(const fmd_subc_config *cfg, float *taps) {
  if (!taps) return fmd_fail(FMD_E_ARG, "taps is NULL");
  const int rc = fmdk_subc_check(cfg);
  if (rc == FMD_OK) blackman_sinc(cfg->bw, cfg->rate_in, cfg->n_taps, taps);
  return rc;
}

/* the carrier table 2 exp(-2 pi i ((p fc) mod R) / R), p = 0 .. Pd - 1, {re, im} pairs: in double, rounded once */
void fmdk_subc_carrier(const fmd_subc_config *c, float *tab) {
  const int pd = fmdk_subc_period(c);
  for (int p = 0; p < pd; p++) {
    const double a = two_pi * (double)(((int64_t)p * c->fc) % c->rate_in) / (double)c->rate_in;
    tab[2 * p] = (float)(2.0 * cos(a));
    tab[2 * p + 1] = (float)(-2.0 * sin(a));
  }
}

/* ---- channel tuner: what needs no device (include/fmdemod_mi355x.h, "Channel tuner"; csrc/tuner.inc) ---- */

int fmdk_tuner_check(const fmd_tuner_config *c) {
  if (!c) return fmd_fail(FMD_E_ARG, "tuner config is NULL");
  if (c->rate <= 0) return fmd_fail(FMD_E_ARG, "rate must be positive");
  if (c->step_hz <= 0 || c->rate % c->step_hz) return fmd_fail(FMD_E_ARG, "step_hz must be positive and divide rate (got %d at %d)", c->step_hz, c->rate);
  const int P = c->rate / c->step_hz;
  if (P < 4 || P > FMD_TUNER_MAX_PERIOD || (P & 3))
    return fmd_fail(FMD_E_UNSUPPORTED, "the table's period rate / step_hz = %d must be a multiple of 4 in 4 .. %d", P, FMD_TUNER_MAX_PERIOD);
  if (c->n_taps < 16 || c->n_taps > FMD_TUNER_MAX_TAPS || (c->n_taps & 3))
    return fmd_fail(FMD_E_UNSUPPORTED, "n_taps must be a multiple of 4 in 16 .. %d (got %d)", FMD_TUNER_MAX_TAPS, c->n_taps);
  if (c->bw <= 0 || 2LL * c->bw >= c->rate) return fmd_fail(FMD_E_ARG, "bw must lie in 0 < bw < rate / 2 (got %d at %d)", c->bw, c->rate);
  if (c->block_len < 64 || (c->block_len & 15)) return fmd_fail(FMD_E_ARG, "block_len must be a multiple of 16, at least 64 (got %d)", c->block_len);
  if (c->block_len / 2 < c->n_taps)
    return fmd_fail(FMD_E_UNSUPPORTED, "a block of %d samples is shorter than the filter (%d taps): its history would reach past the block before it",
                    c->block_len / 2, c->n_taps);
  return FMD_OK;
}

int fmd_tuner_design(const fmd_tuner_config *cfg, float *taps) {
  if (!taps) return fmd_fail(FMD_E_ARG, "taps is NULL");
  const int rc = fmdk_tuner_check(cfg);
  if (rc == FMD_OK) blackman_sinc(cfg->bw, cfg->rate, cfg->n_taps, taps);
  return rc;
}

int fmd_tuner_shift(const fmd_tuner_config *cfg, int offset_hz, int offset_tuning, int32_t *shift) {
  if (!shift) return fmd_fail(FMD_E_ARG, "shift is NULL");
  const int rc = fmdk_tuner_check(cfg);
  if (rc) return rc;
  if (2LL * offset_hz > cfg->rate || 2LL * offset_hz < -(long long)cfg->rate)
    return fmd_fail(FMD_E_ARG, "offset_hz %d lies outside the capture (+-%d Hz)", offset_hz, cfg->rate / 2);
  if (!offset_tuning && (cfg->rate & 3)) return fmd_fail(FMD_E_ARG, "rate %d is no multiple of 4: -rate / 4 is not on the grid", cfg->rate);
  const long long hz = (offset_tuning ? 0LL : -(long long)(cfg->rate / 4)) - (long long)offset_hz;
  if (hz % cfg->step_hz) return fmd_fail(FMD_E_ARG, "a shift of %lld Hz is not on the grid of %d Hz", hz, cfg->step_hz);
  *shift = (int32_t)(hz / cfg->step_hz);
  return FMD_OK;
}

/* c[p] = exp(+2 pi i p / P), P a multiple of 4: every entry from an angle of the first octant (0 .. pi/4) by symmetry, so that the quarter periods are
 * exactly 1, i, -1, -i and the table has the symmetries of the circle; in double, rounded once */
void fmdk_tuner_table(int period, float *tab) {
  const int q = period / 4;
  for (int p = 0; p < period; p++) {
    const int quad = p / q, r = p % q;                  /* angle = quad pi/2 + 2 pi r / P, r < q */
    double c, s;
    if (2 * r <= q) {
      c = cos(two_pi * (double)r / (double)period);
      s = sin(two_pi * (double)r / (double)period);
    } else {                                            /* past pi/4: the mirror image of the angle 2 pi (q - r) / P */
      c = sin(two_pi * (double)(q - r) / (double)period);
      s = cos(two_pi * (double)(q - r) / (double)period);
    }
    const float cf = (float)c, sf = (float)s;
    float re, im;
    switch (quad) {
      case 0: re = cf; im = sf; break;
      case 1: re = -sf; im = cf; break;
      case 2: re = -cf; im = -sf; break;
      default: re = sf; im = -cf; break;
    }
    tab[2 * p] = re + 0.0f;                             /* (+0, not -0, where an entry is zero) */
    tab[2 * p + 1] = im + 0.0f;
  }
}

int fmdk_tuner_channel(const fmd_tuner_config *c, int n_sources, const fmd_tuner_channel *ch, fmdk_tuner_chan *out) {
  if (!c || !ch || !out) return fmd_fail(FMD_E_ARG, "NULL argument");
  const int P = c->rate / c->step_hz;
  if (ch->source < 0 || ch->source >= n_sources) return fmd_fail(FMD_E_ARG, "source %d out of range (%d sources)", ch->source, n_sources);
  if (ch->shift <= -P || ch->shift >= P) return fmd_fail(FMD_E_ARG, "shift %d outside -%d < shift < %d (the table's period)", ch->shift, P, P);
  if (!isfinite(ch->gain) || !(ch->gain > 0.0f) || ch->gain > 64.0f) return fmd_fail(FMD_E_ARG, "gain must be finite with 0 < gain <= 64 (got %g)", (double)ch->gain);
  memset(out, 0, sizeof(*out));
  out->source = ch->source;
  out->sh = ch->shift < 0 ? ch->shift + P : ch->shift;
  out->sh8 = (int32_t)((8LL * out->sh) % P);
  out->sh2k = (int32_t)((2048LL * out->sh) % P);
  out->g = 128.0f * ch->gain;                           /* exact: a power of two */
  return FMD_OK;
}

/* ---- station finder: what needs no device (include/fmdemod_mi355x.h, "Station finder"; csrc/scan.inc) ---- */

static long long floor_div(long long a, long long b) {   /* b > 0 */
  const long long q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

int fmdk_scan_plan_make(const fmd_scan_config *c, fmdk_scan_plan *p, fmdk_scan_cand *cand) {
  if (!c || !p) return fmd_fail(FMD_E_ARG, "scan config is NULL");
  if (c->reserved[0] || c->reserved[1] || c->reserved[2]) return fmd_fail(FMD_E_ARG, "reserved words of the scan config must be zero");
  if (c->rate <= 0) return fmd_fail(FMD_E_ARG, "rate must be positive (got %d)", c->rate);
  if (c->n_bins < 64 || c->n_bins > FMD_SCAN_MAX_BINS || (c->n_bins & (c->n_bins - 1)))
    return fmd_fail(FMD_E_UNSUPPORTED, "n_bins must be a power of two in 64 .. %d (got %d)", FMD_SCAN_MAX_BINS, c->n_bins);
  if (c->raster_hz <= 0) return fmd_fail(FMD_E_ARG, "raster_hz must be positive (got %d)", c->raster_hz);
  const long long R = c->rate, N = c->n_bins, bw = c->bw, ras = c->raster_hz;
  if (bw <= 0 || R > 2 * bw * N)
    return fmd_fail(FMD_E_ARG, "bw must be positive and a channel at least one bin wide: rate / n_bins <= 2 bw (got bw %d at %d Hz, %d bins)", c->bw,
                    c->rate, c->n_bins);
  const long long room = (R - 2 * bw) * N - R;           /* 2 N (rate/2 - D/2 - bw) */
  if (room < 0) return fmd_fail(FMD_E_ARG, "no channel of +-%d Hz fits inside the capture's +-(rate/2 - half a bin) at %d Hz, %d bins (cmax < 0)", c->bw, c->rate, c->n_bins);
  const long long cmax = room / (2 * N * ras), C = 2 * cmax + 1;
  if (C > FMD_SCAN_MAX_CANDIDATES)
    return fmd_fail(FMD_E_UNSUPPORTED, "%lld candidates on a raster of %d Hz: at most %d", C, c->raster_hz, FMD_SCAN_MAX_CANDIDATES);
  if (c->min_sep < 1 || c->min_sep > C) return fmd_fail(FMD_E_ARG, "min_sep must lie in 1 .. C = %lld (got %d)", C, c->min_sep);
  if (c->floor_permille < 0 || c->floor_permille > 1000) return fmd_fail(FMD_E_ARG, "floor_permille must lie in 0 .. 1000 (got %d)", c->floor_permille);
  if (c->dc_guard < 0 || c->dc_guard > c->n_bins / 4) return fmd_fail(FMD_E_ARG, "dc_guard must lie in 0 .. n_bins / 4 = %d (got %d)", c->n_bins / 4, c->dc_guard);
  if (c->max_stations < 1 || c->max_stations > FMD_SCAN_MAX_STATIONS)
    return fmd_fail(FMD_E_ARG, "max_stations must lie in 1 .. %d (got %d)", FMD_SCAN_MAX_STATIONS, c->max_stations);
  if (!isfinite(c->threshold) || !(c->threshold > 0.0f)) return fmd_fail(FMD_E_ARG, "threshold must be finite and positive (got %g)", (double)c->threshold);

  memset(p, 0, sizeof(*p));
  p->n_cand = (int32_t)C;
  p->cmax = (int32_t)cmax;
  p->n_used = (int32_t)(N - (c->dc_guard > 0 ? 2 * c->dc_guard - 1 : 0));
  p->rank = (int32_t)(((long long)c->floor_permille * (p->n_used - 1)) / 1000);
  p->nb = (double)(2 * bw * N) / (double)R;
  if (!cand) return FMD_OK;
  /* in units of 1 / (2 N) Hz: bin s covers [(2 s - 1) R, (2 s + 1) R), the band [2 N lo, 2 N hi] */
  for (long long i = 0; i < C; i++) {
    const long long ctr = (i - cmax) * ras, lo2 = 2 * N * (ctr - bw), hi2 = 2 * N * (ctr + bw);
    const long long s0 = floor_div(lo2 + R, 2 * R);                    /* the bin that holds lo */
    const long long s1 = -floor_div(-(hi2 + R), 2 * R) - 1;            /* the last bin that begins below hi */
    cand[i].first = (int32_t)s0;
    cand[i].count = (int32_t)(s1 - s0 + 1);
    cand[i].w_first = (double)((2 * s0 + 1) * R - lo2) / (double)(2 * R);
    cand[i].w_last = (double)(hi2 - (2 * s1 - 1) * R) / (double)(2 * R);
  }
  return FMD_OK;
}

int fmd_scan_candidates(const fmd_scan_config *cfg) {
  fmdk_scan_plan p;
  const int rc = fmdk_scan_plan_make(cfg, &p, NULL);
  return rc ? rc : p.n_cand;
}

/* ---- stereo control: what needs no device (include/fmdemod_mi355x.h, "Stereo control"; csrc/stereo.inc) ---- */

int fmdk_stereo_plan(const fmd_stereo_config *c, fmdk_stereo_k *k) {
  if (!c) return fmd_fail(FMD_E_ARG, "stereo config is NULL");
  if (c->reserved0 || c->reserved[0] || c->reserved[1] || c->reserved[2]) return fmd_fail(FMD_E_ARG, "reserved words of the stereo config must be zero");
  if (c->pcm_stride < 8 || c->pcm_stride > 65536 || (c->pcm_stride & 7))
    return fmd_fail(FMD_E_UNSUPPORTED, "pcm_stride must be a multiple of 8 in 8 .. 65536 (got %d)", c->pcm_stride);
  if (c->pilot_per_block < 0 || c->pilot_per_block > 65536) return fmd_fail(FMD_E_UNSUPPORTED, "pilot_per_block must lie in 0 .. 65536 (got %d)", c->pilot_per_block);
  if (c->hold_blocks < 1 || c->hold_blocks > (1 << 20)) return fmd_fail(FMD_E_ARG, "hold_blocks must lie in 1 .. 2^20 (got %d)", c->hold_blocks);
  if (!isfinite(c->pilot_on) || !isfinite(c->pilot_off) || !(c->pilot_off > 0.0f) || !(c->pilot_off <= c->pilot_on))
    return fmd_fail(FMD_E_ARG, "the pilot thresholds must be finite with 0 < pilot_off <= pilot_on (got off %g, on %g)", (double)c->pilot_off, (double)c->pilot_on);
  if (!isfinite(c->blend_lo) || !isfinite(c->blend_hi) || !(c->blend_lo < c->blend_hi))
    return fmd_fail(FMD_E_ARG, "the blend range must be finite with blend_lo < blend_hi (got %g, %g)", (double)c->blend_lo, (double)c->blend_hi);
  if (!(c->slew > 0.0f) || !(c->slew <= 1.0f)) return fmd_fail(FMD_E_ARG, "slew must lie in 0 < slew <= 1 (got %g)", (double)c->slew);
  if (!k) return FMD_OK;
  k->thr_on = (float)((double)c->pilot_on * (double)c->pilot_on);
  k->thr_off = (float)((double)c->pilot_off * (double)c->pilot_off);
  k->inv_mz = c->pilot_per_block > 0 ? (float)(1.0 / (double)c->pilot_per_block) : 0.0f;
  k->inv_span = (float)(1.0 / ((double)c->blend_hi - (double)c->blend_lo));
  return FMD_OK;
}
