/*
 * fmd_resolve.c - the fused chain's resolver, device-free (tests/c/plan_check.c): configuration checks and filter design, the kernel family a configuration
 * resolves to, the kernel arguments (fmdk_params), the fixed-point forms of the filters and their error estimate, the decimating second stage's tap tables and
 * the time chunks of a launch, with the tiling helpers of the fused kernels' unit.  The receivers' checks and designs: fmd_recv.c, fmd_rds.c; fmd_fail: fmd_error.c.
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "fmd_internal.h"

#define FMD_PI 3.14159265f   /* PI_F  include/rtl_fm_player.h:40 */
#define FMD_2PI 6.28318531f  /* PI2_F include/rtl_fm_player.h:39 */

/* ---- filter design: init_lp_f32 / init_lp_real_f32 restated ------------- */

float fmd_deemph_lambda(int output_rate, double tau) {
  return (float)exp(-1.0 / ((double)output_rate * tau));   /* src/rtl_fm_player.c:1577 */
}

void fmdk_design_fb(float *fb) {   /* src/rtl_fm_player.c:241-251 */
  for (int i = 0; i < 16; i++) {
    float j = (float)i - 15.5f;
    fb[i] = (sinf(0.125f * FMD_PI * j) / (FMD_PI * j)) * (0.54f - 0.46f * cosf(FMD_PI * (float)i / 15.5f));
  }
}

void fmdk_design_mpx(int size, int rate_in, float *fm, float *fp, float *fs, float *swf, float *cwf) {
  /* src/rtl_fm_player.c:420-452 */
  const float rate = (float)rate_in;
  const float wf = FMD_2PI * 19000.0f / rate;
  *swf = sinf(wf);
  *cwf = cosf(wf);
  const float fmh = 16000.0f / rate, fpl = 18000.0f / rate, fph = 20000.0f / rate;
  const float fsl = 21000.0f / rate, fsh = 55000.0f / rate;
  for (int i = 0; i < (size >> 1); i++) {
    const float fi = (float)i - (float)(size - 1) / 2.0f;
    const float fh = 0.54f - 0.46f * cosf(FMD_2PI * (float)i / (float)(size - 1));
    float fv;
    fv = (fi == 0) ? 2.0f * fmh : sinf(FMD_2PI * fmh * fi) / (FMD_PI * fi);
    fm[i] = fv * fh;
    fv = (fi == 0) ? 2.0f * (fph - fpl) : (sinf(FMD_2PI * fph * fi) - sinf(FMD_2PI * fpl * fi)) / (FMD_PI * fi);
    fp[i] = fv * fh;
    fv = (fi == 0) ? 2.0f * (fsh - fsl) : (sinf(FMD_2PI * fsh * fi) - sinf(FMD_2PI * fsl * fi)) / (FMD_PI * fi);
    fs[i] = fv * fh;
  }
}

int fmdk_check_config(const fmd_config *c) {
  if (!c) return fmd_fail(FMD_E_ARG, "config is NULL");
  if (c->rate_in <= 0) return fmd_fail(FMD_E_ARG, "rate_in must be positive");
  if (c->mode < 0 || c->mode > 2) return fmd_fail(FMD_E_ARG, "lpr.mode must be 0, 1 or 2");
  if (c->size < 2 || c->size > 256 || (c->size & 1)) return fmd_fail(FMD_E_ARG, "lpr.size must be even, 2..256");
  if (c->block_len < 64 || (c->block_len & 15)) return fmd_fail(FMD_E_ARG, "block_len must be a multiple of 16, >= 64");
  if (c->math < FMD_MATH_EXACT || c->math > FMD_MATH_FAST_MFMA_F)
    return fmd_fail(FMD_E_ARG, "math must be FMD_MATH_EXACT, _FAST, _FAST_VALU, _FAST_MFMA or _FAST_MFMA_F (4 - 6, the retired family names, mean _FAST)");
  /* the +-1 LSB kernels evaluate the de-emphasis blockwise with powers of lambda (scan weights, restarts from zero):
   * a contraction is assumed.  lambda outside (0, 1) - never produced by fmd_deemph_lambda - belongs to the exact kernels */
  if (c->math != FMD_MATH_EXACT && c->deemph && !(c->deemph_lambda > 0.f && c->deemph_lambda < 1.f))
    return fmd_fail(FMD_E_UNSUPPORTED, "the fast kernels need 0 < deemph_lambda < 1 (got %g): use FMD_MATH_EXACT", (double)c->deemph_lambda);
  if (c->rate_out2 > 0) {
    if (c->rate_out <= 0 || c->rate_out > 2000000) return fmd_fail(FMD_E_UNSUPPORTED, "rate_out must be 1..2000000");
    if (c->rate_out2 > c->rate_out)
      return fmd_fail(FMD_E_UNSUPPORTED, "rate_out2 > rate_out overflows the reference's accumulator");
    /* stereo writes two outputs per emit over its own input; beyond 1/3 the
     * in-place overwrite reaches more than the block's second sample */
    if (c->mode == 2 && 3LL * c->rate_out2 > c->rate_out)
      return fmd_fail(FMD_E_UNSUPPORTED, "stereo needs rate_out2 <= rate_out / 3");
  } else if (c->mode == 2) {
    return fmd_fail(FMD_E_UNSUPPORTED, "stereo without the resampler is not supported");
  }
  return FMD_OK;
}

int fmd_design_taps(const fmd_config *cfg, fmd_taps *out) {
  if (!out) return fmd_fail(FMD_E_ARG, "taps is NULL");
  int rc = fmdk_check_config(cfg);
  if (rc) return rc;
  memset(out, 0, sizeof(*out));
  fmdk_design_fb(out->fb);
  fmdk_design_mpx(cfg->size, cfg->rate_in, out->fm, out->fp, out->fs, &out->swf, &out->cwf);
  return FMD_OK;
}

static int max_result_len(const fmd_config *c) {
  const long m = c->block_len / 16;
  long n;
  if (c->rate_out2 > 0) n = (m * (long)c->rate_out2) / c->rate_out + 1;
  else n = m;
  if (c->mode == 2) n *= 2;
  return (int)n;
}

/* The sign the j^n rotation gives tap j in the sum of component comp (0 = I, 1 = Q), and *sel = the byte of the sample it multiplies. */
static int rotation_sign(int j, int comp, int offset_tuning, int *sel) {
  const int p = j & 3;
  *sel = comp;
  if (offset_tuning) return 1;
  *sel = comp ? ((p & 1) ^ 1) : (p & 1);                   /* j^p: I = (+I, -Q, -I, +Q), Q = (+Q, +I, -Q, -I) */
  return comp ? ((p == 0 || p == 1) ? 1 : -1) : ((p == 0 || p == 3) ? 1 : -1);
}

/* Stage A on the matrix pipe (FMD_MATH_FAST_MFMA): the A operand of v_mfma_i32_16x16x64_i8.
 * Output m of the /8 low-pass (src/rtl_fm_player.c:253-411, rotation :206-226 folded in) is
 *   y_c[m] = sum_{j<32} sgn_c(j) fb[min(j, 31-j)] x[8m - 24 + j][sel_c(j)],   x = (u - 127.5) / 128,
 * a dot product of the 64 window bytes with a vector that has 32 non-zero entries.  With E = sgn round(fb 2^26)
 * (|E| < 2^23, three balanced int8 limbs) and s = u - 128 the sum  S = sum E s  is EXACT integer arithmetic and
 *   y = 2^-33 (S + sum E / 2) = 2^-17 S0 + 2^-25 S1 + 2^-33 S2 + bias.
 * Tap quantisation moves y by at most 32 x 2^-27 |x| <= 2.4e-7 (rms 2.4e-8): the size of the fp32 rounding of the
 * reference's own sum, inside the +-1 LSB contract like the fused sums of FMD_MATH_FAST_VALU.
 * Entry [limb][comp][d] holds the 16 bytes (8 samples x {I, Q}) of taps 8d .. 8d+7. */
static int build_a_tab(const fmd_taps *t, int offset_tuning, fmdk_params *k) {   /* -1: a tap does not fit three limbs */
  long long sum[2] = {0, 0};
  int8_t *tab = (int8_t *)k->a_tab;
  memset(k->a_tab, 0, sizeof(k->a_tab));
  for (int j = 0; j < 32; j++) {
    const double tap = (double)t->fb[j < 16 ? j : 31 - j];
    const long long T = llround(tap * 67108864.0);        /* 2^26 */
    const int d = j >> 3, jj = j & 7;
    for (int comp = 0; comp < 2; comp++) {
      int sel;
      long long E = rotation_sign(j, comp, offset_tuning, &sel) * T;
      sum[comp] += E;
      int limb[3];
      for (int i = 2; i >= 0; i--) {                       /* balanced digits, least significant first */
        long long r = ((E % 256) + 256) % 256;
        if (r >= 128) r -= 256;
        limb[i] = (int)r;
        E = (E - r) / 256;
      }
      if (E != 0) return -1;                               /* |tap| >= 0.1245: beyond 2^23 / 2^26 (the reference's largest is 0.1239) */
      for (int l = 0; l < 3; l++) tab[(((l * 2 + comp) * 4 + d) * 16) + 2 * jj + sel] = (int8_t)limb[l];
    }
  }
  k->a_bias_i = (float)ldexp((double)sum[0], -34);
  k->a_bias_q = (float)ldexp((double)sum[1], -34);
  return 0;
}

/* Limb l (0 = most significant) of a T in three balanced int8 limbs, as the byte the tables hold. */
static uint8_t limb_byte(int32_t T, int l) { return (uint8_t)((((uint32_t)T + 0x808080u) ^ 0x808080u) >> (8 * (2 - l))); }
/* THE tap quantiser of the matrix-pipe stages: the largest qf that keeps T = round(h 2^qf) inside three balanced int8 limbs (-8 421 504 .. 8 355 711),
 * the T, and the sums the accumulator bound and the error estimate are made of.  T[u] = rint(h[u] 2^qf) in double, ties to even: for a float tap that IS
 * the kernel's rintf(ldexpf(h, qf)) (kernel.inc, the stage-C byte tables: both products are exact and below 2^23) - the host bounds and reports the limbs
 * the kernel multiplies with.  -1 (out->n = 0): all zero, not finite, or qf < 8 (taps of magnitude 2^15: not a filter this form was made for). */
static int quantise_taps(const double *h, int n, fixed_taps *out) {
  memset(out, 0, sizeof(*out));
  double mx = 0.0;
  for (int u = 0; u < n; u++) mx = fmax(mx, fabs(h[u]));
  if (!(mx > 0.0) || !isfinite(mx)) return -1;
  int qf = 40;
  while (qf > 0 && rint(mx * ldexp(1.0, qf)) > 8355711.0) qf--;
  if (qf < 8) return -1;
  for (int u = 0; u < n; u++) {
    out->T[u] = (int32_t)rint(h[u] * ldexp(1.0, qf));
    for (int l = 0; l < 3; l++) out->limb_abs[l] += fabs((double)(int8_t)limb_byte(out->T[u], l));
    out->sum_abs += fabs(h[u]);
    out->sum_sq += h[u] * h[u];
  }
  out->n = n;
  out->qf = qf;
  return 0;
}
/* The kernel reads its int32 limb-pair sums as floats (accumulators started at the bits of 1.5 x 2^23, mpx_tile_i8): every weight
 * class must stay inside +-2^22 for ANY samples (limbs within +-128).  Classes by tap limb: class 0 = T0, class 1 = T0 + T1,
 * class 2 = T0 + T1 + T2, class 3 = T1 + T2 (the sample limb is what is left of the class index). */
static int fits_accumulators(const fixed_taps *q) {
  return 128.0 * (q->limb_abs[0] + q->limb_abs[1] + q->limb_abs[2]) < 4194304.0 - 65536.0;
}
/* (and the samples inside the limbs' range |x| < 8 for any discriminator output: |v| <= pi through the filter's half taps) */
static int keeps_limb_range(const float *half, int n2) {
  double sa = 0.0;
  for (int u = 0; u < n2; u++) sa += 2.0 * fabs((double)half[u]);
  return 3.1415927 * sa < 7.9;
}

/* Matrix-pipe form of stage C (fmd_kernels.inc, mpx_tile_i8): per filter (stereo: fm, fp, fs; the 128-tap mono path's one filter, resample_mono_dec: fm) the
 * qf of its quantised form and the scale that puts the integer sums together.  -1: a filter has no such form (quantise_taps), or its weight classes do not
 * fit the accumulators. */
static int build_ci_scales(const fixed_taps *q, int nf, fmdk_params *k) {
  for (int f = 0; f < nf; f++) {
    if (!q[f].n || !fits_accumulators(&q[f])) return -1;
    k->ci_qf[f] = q[f].qf;
    k->ci_scale[f] = (float)ldexp(1.0, 32 - 20 - q[f].qf);
    k->ci_scale_q[f] = (float)ldexp(1.0, 32 - q[f].qf);
  }
  return 0;
}

/* (stage_d_on_matrix_pipe, below: the second stage on the matrix pipe needs what stage C needs - build_ci_scales - and: at most eight groups of sixteen
 * frames per tile for stereo (rate_out >= 4 rate_out2; mono: sixteen, rate_out >= 2 rate_out2), both magic-number index forms, the error estimate under its
 * limit, and (L-R) x carrier inside the limbs' range |x| < 8 for any discriminator output - |v| <= pi, and what quirk Q1 can put in place of a sample:
 * |om - os| <= 2 pi sum|fm| sum|f| - true of any filter of the reference's design, checked for a caller's.) */
/* What a second-stage filter's fixed-point form (taps T = round(h 2^qf) and samples q = round(x 2^20) in three balanced int8 limbs each, six of the nine limb
 * pairs kept) adds to a PCM value, in LSB: the filter's output IS the PCM value before de-emphasis and scaling, so an error e in it is e x coef LSB
 * (coef = volume x 32768).  Three terms, each as an rms ESTIMATE and as a worst-case BOUND from the filter's own taps and limbs:
 *   the limb pairs left out (tap limb + sample limb >= 3): S3 = sum_k (t1 s2 + t2 s1) at weight c0 2^-24 and S4 = sum_k t2 s2 at c0 2^-32, c0 = 2^(12 - qf).
 *     rms: 2 n products of two limbs of rms 74 each; bound: |sample limb| <= 128, so |S3| <= 128 sum_k (|t1| + |t2|), |S4| <= 128 sum_k |t2|;
 *   the samples' rounding to 2^-20: rms 2^-21 / sqrt 3 per sample through the filter (x sqrt(sum h^2)); bound 2^-21 sum |h|;
 *   the taps' rounding to 2^-qf: rms 2^-(qf+1) / sqrt 3 per tap, n taps, samples of rms ~1.8 at most (a discriminator output uniform in +-pi);
 *     bound n 2^-(qf+1) pi (the L-R channel's samples are (L-R band) x carrier: the same range).
 * 300 k stereo / mono: rms 0.004 at volume 0.4, 0.08 - 0.09 at volume 8 (max |difference| 1 LSB measured); 25 k narrow FM (largest tap 0.58: qf 23, c0
 * eight times the 300 k filters'): 0.035 at volume 0.4, 0.09 at 1, 0.26 at 3 (still 1 LSB at most in 262 144 values) and 0.70 at volume 8, where 3 LSB
 * were measured (profiles/archive/r5q_low_amp_volume_scan_before.txt).  The GATE is the rms estimate <= FMD_STAGE_D_MAX_LSB (ten standard deviations below
 * one step: a statistical guarantee); the bound is reported (fmd_config_error_estimate) and is below half a step for the reference's
 * default configurations. */
static stage_error fixed_point_error(const fixed_taps *q, double coef) {
  stage_error e = {0.0, 0.0, 0.0, 0.0, q->qf, q->n};
  const int n = q->n, qf = q->qf;
  const double c0 = ldexp(1.0, 12 - qf), ac = fabs(coef), a1 = q->limb_abs[1], a2 = q->limb_abs[2];
  const double dropped = c0 * ldexp(1.0, -24) * sqrt(2.0 * n) * 74.0 * 74.0;
  const double samples = ldexp(1.0, -21) / sqrt(3.0) * sqrt(q->sum_sq);
  const double taps = sqrt((double)n) * ldexp(1.0, -(qf + 1)) / sqrt(3.0) * 1.8;
  e.rms = ac * sqrt(dropped * dropped + samples * samples + taps * taps);
  e.worst_dropped = ac * c0 * (ldexp(1.0, -24) * 128.0 * (a1 + a2) + ldexp(1.0, -32) * 128.0 * a2);
  e.worst_samples = ac * ldexp(1.0, -21) * q->sum_abs;
  e.worst_taps = ac * (double)n * ldexp(1.0, -(qf + 1)) * 3.14159265358979;
  return e;
}
static void fm_full(const float *fm, int n, double *h) { for (int u = 0; u < n; u++) h[u] = (double)fm[u < n / 2 ? u : n - 1 - u]; }
static void composite_taps(const float *fm, double *g /* [179] */) {
  for (int u = 0; u < 179; u++) {
    double a = 0.0;
    for (int i = 0; i < 90; i++) {
      const int j = u - i;
      if (j < 0 || j >= 90) continue;
      a += (double)fm[i < 45 ? i : 89 - i] * (double)fm[j < 45 ? j : 89 - j];
    }
    g[u] = a;
  }
}
#define FMD_STAGE_D_MAX_LSB 0.10

static int stage_d_on_matrix_pipe(const fmd_taps *t, const fmdk_params *k, const stage_error *fm_err) {
  if (k->resample && k->mode == 1 && k->size == 128)       /* mono: rate_out >= 2 rate_out2 (at most sixteen groups of sixteen frames per tile) */
    return (long long)k->fast >= 2LL * k->slow && k->emit_magic && k->tf_magic && fm_err->rms <= FMD_STAGE_D_MAX_LSB;
  if (!(k->resample && k->mode == 2 && k->size == 90)) return 0;
  if ((long long)k->fast < 4LL * k->slow || !k->emit_magic || !k->tf_magic) return 0;
  if (fm_err->rms > FMD_STAGE_D_MAX_LSB) return 0;
  return keeps_limb_range(t->fm, 45) && keeps_limb_range(t->fs, 45);
}

/* The L+R chain of the stereo path as ONE filter (FMD_MATH_FAST_MFMA_F).  The reference low-passes the discriminator output with fm into the
 * bm ring at every sample (src/rtl_fm_player.c:545, :560) and low-passes that ring with fm again at the emit instants (:588): with no
 * non-linear step between them the two are the 179-tap filter g = fm * fm over the discriminator output.  g in double from the float taps,
 * T_g = round(g 2^qf) in three balanced int8 limbs like every filter of the matrix-pipe stages; the same bound on the weight classes
 * (accumulators read as floats) and the same error estimate as stage D's (one quantisation of the samples instead of two). */
static int build_lr_composite(const fixed_taps *g, const stage_error *err, fmdk_params *k) {
  if (!g->n) return -1;
  for (int u = 0; u < 90; u++) k->gq[u] = g->T[u];
  if (!fits_accumulators(g)) return -1;
  /* (the decimating form's window holds every tap of every row; round 5's full-rate form lacked the last two in two of sixteen rows and carried a term for them) */
  if (err->rms > FMD_STAGE_D_MAX_LSB) return -1;
  k->g_qf = g->qf;
  k->g_scale = (float)ldexp(1.0, 12 - g->qf);
  k->g_unit = (float)ldexp(1.0, -g->qf);
  return 0;
}

/* ---- fmdk_params, by what is filled: each from the configuration and the taps alone (fill_params zeroes the struct first) ---- */

static void fill_decimator(const fmd_config *c, const fmd_taps *t, fmdk_params *k) {
  /* fast path of the /8 low-pass: y = c + sum_j s[j] (fb[min(j,31-j)] / 128) u[j]
   * with the (u - 127.5)/128 conversion folded in; s = j^n rotation signs */
  double ci = 0, cq = 0;
  for (int j = 0; j < 32; j++) {
    const float tap = t->fb[j < 16 ? j : 31 - j];
    int sel;
    ci += (double)((float)rotation_sign(j, 0, c->offset_tuning != 0, &sel) * tap);
    cq += (double)((float)rotation_sign(j, 1, c->offset_tuning != 0, &sel) * tap);
  }
  for (int j = 0; j < 16; j++) k->fbs[j] = t->fb[j] / 128.0f;
  /* the kernel converts the bytes as u - 128 (small signed integers: the partial sums then stay
   * at signal level instead of carrying the 127.5 offset): (u - 127.5)/128 = (u - 128)/128 + 0.5/128 */
  k->c_i = (float)((0.5 / 128.0) * ci);
  k->c_q = (float)((0.5 / 128.0) * cq);
}

static void fill_deemph_flush(const fmd_config *c, const fmd_taps *t, fmdk_params *k) {
  (void)t;
  k->deemph = c->deemph != 0;
  k->lambda = c->deemph_lambda;
  {
    float lp = c->deemph_lambda;
    for (int j = 0; j < 16; j++) { k->lam_pow[j] = lp; lp *= c->deemph_lambda; }
  }
  if (c->math != FMD_MATH_EXACT) {
    /* per-tile flush of the fast kernels: group size and the scan's powers; with de-emphasis off
     * every power is zero and the flush passes its input through */
    const long long tile = fmdk_tile();
    /* most frames a tile can hold: floor((acc + tile slow) / fast) with acc <= fast - 1 */
    const long long fmax = c->rate_out2 > 0 ? (tile * c->rate_out2 + c->rate_out - 1) / c->rate_out : tile;
    const int ch = c->mode == 2 ? 2 : 1;
    k->flush_g = (fmax + 3) / 4 <= 64 / ch ? 4 : 8;     /* lanes: 32 groups per channel (stereo), 64 (mono) */
    if (ch == 1 && (fmax + 1) / 2 <= 64)
      k->flush_g = 2;                                     /* mono with few frames per tile: shorter groups, fewer instructions */
    if (ch == 2 && (fmax + 2) / 3 <= 32)
      k->flush_g = 3;                                     /* stereo likewise: groups of three fit its 32 lanes per channel up to 96 frames */
    const int on = c->deemph != 0;
    k->lam_eff = on ? c->deemph_lambda : 0.f;
    if (!on) memset(k->lam_pow, 0, sizeof(k->lam_pow));
    double a = on ? pow((double)c->deemph_lambda, (double)k->flush_g) : 0.0;
    k->log2_a = (on && c->deemph_lambda > 0.f) ? (float)((double)k->flush_g * log2((double)c->deemph_lambda)) : -1e30f;
    for (int j = 0; j < 8; j++) { k->lam_scan[j] = (float)a; a *= a; }
  }
}

static void fill_thresholds(const fmd_config *c, const fmd_taps *t, fmdk_params *k) {   /* (after k->coef) */
  {
    /* origin threshold of the fast discriminator (fmdk_params.org_thr): an isolated phase error e / rho of a sample of magnitude rho reaches
     * the PCM as coef x (one tap of the filter behind the discriminator) x e / rho.  1e-3 was validated on narrow FM at volume 0.4
     * (coef x largest tap = 13 107 x 0.58 = 7 600: tests/test_gpu_parity.py::test_fast_math_nfm_noise_next_to_the_origin); a larger
     * product moves the threshold out in proportion, so that the PCM-level error at the threshold stays what it was there. */
    float hmax = 0.f;
    const float *first = (c->rate_out2 > 0 && c->mode != 0) ? t->fm : NULL;      /* mode 0 / no resampler: the discriminator output goes out as it is */
    if (first) { for (int i = 0; i < (c->size >> 1); i++) hmax = fmaxf(hmax, fabsf(first[i])); if (c->mode == 2) for (int i = 0; i < (c->size >> 1); i++) hmax = fmaxf(hmax, fabsf(t->fs[i])); }
    else hmax = 1.f;
    const float scale = fabsf(k->coef) * hmax / 7600.0f;
    k->org_thr = 1e-3f * (scale > 1.f ? (scale < 200.f ? scale : 200.f) : 1.f);
    k->org_thr15 = 1.5f * k->org_thr;
    k->pilot_pairs8 = fabsf(c->volume) >= 1.0f;      /* (mpx_tile_i8: eight limb pairs for the pilot filter instead of six) */
  }
  {
    /* carrier_fast: an error e in (x, y) moves sin 2 atan2 by 2 |e| / r; times |vs|, one tap of the
     * second-stage low-pass (largest |fm|) and the PCM scale it must stay below a quarter LSB.
     * |e| ~ 1.5 eps with eps = 1e-7 the rounding difference between the fast and the reference
     * pilot-filter sums  =>  r < K |vs| is redone exactly, K = 12 eps coef max|fm|.
     * Measured (tools/fuzz_parity.py 400 {1,2,3,4}, noise input): with K scaled by 0.2 and below the
     * 1 600 cases still hold 2-6 differences of 2-3 LSB, from 0.6 up none; this K is 3x that bound.
     * Noise input pays for it (every ~3rd tile holds such a sample at 300 kHz: 0.64 -> 0.83 ms per launch
     * of 256 x 16 blocks); an FM signal with a pilot never comes near (r ~ 0.06 against K |vs| ~ 0.002). */
    float gmax = 0.f;
    for (int i = 0; i < (c->size >> 1); i++) gmax = fmaxf(gmax, fabsf(t->fm[i]));
    /* eps follows the rounding noise of the pilot-filter sum, ~ sqrt(sum fp^2): 1e-7 is the 300 kHz / 90-tap
     * figure (sum over the 90 taps of fp^2 = 0.0031); filters at lower rates are wider (48 kHz: 0.04-0.07), and
     * there the fuzz soak (tools/fuzz_parity.py 400 5..24) found two 2-LSB cases that needed 2-4 x this K.
     * K grows with the square of the noise ratio (capped at 25): default-rate streams keep the K above. */
    double sfp2 = 0.0;
    for (int i = 0; i < (c->size >> 1); i++) sfp2 += 2.0 * (double)t->fp[i] * (double)t->fp[i];
    double widen = sfp2 / 0.0031;
    if (widen < 1.0) widen = 1.0;
    if (widen > 25.0) widen = 25.0;
    const float K = 12.0f * 1e-7f * (float)widen * fabsf(k->coef) * gmax;
    k->car_inv_k2 = K > 0.f ? 1.0f / (K * K) : 3.0e38f;
    k->car_inv_k2_q = k->car_inv_k2 < 3.0e38f * 0x1p-40f ? k->car_inv_k2 * 0x1p40f : 3.0e38f;
    /* Two levels (round 4).  A flagged sample first gets its pilot / L-R sums again from the worker's own window, in the
     * reference's ORDER of operations: that removes the order-of-summation part of the difference to the reference (what is left:
     * the window's samples are a few ulps off each, and roundings that fall differently because of it).  Only samples within
     * L K of the origin after that are recomputed from the IQ words.  L was measured like K (tools/fuzz_parity.py and the noise /
     * hand-over tests, profiles/archive/r04w_carrier_l2.txt): 0.125 fails 4 of the noise / hand-over tests, 0.25 and up none. */
    const float L2 = 0.5f;
    k->car_inv_k2_l2 = K > 0.f ? 1.0f / (K * L2 * K * L2) : 3.0e38f;
  }
}

/* floor(n / d) for n < 2^bits as mulhi(n, m) >> sh: with l = ceil(log2 d), p = bits + l and m = ceil(2^p / d) (*magic and *shift = p - 32 stay as they
 * are - zero: the kernel divides by float estimate - where p < 32 or m does not fit 32 bits).  The emit index's derivation below is the case bits = 29. */
static void magic_div(int32_t d, int bits, uint32_t *magic, uint32_t *shift) {
  int l = 0;
  while ((1LL << l) < d) l++;
  const int p = bits + l;
  const unsigned long long m = (((unsigned long long)1 << p) + (unsigned long long)d - 1) / (unsigned long long)d;
  if (p >= 32 && m <= 0xffffffffULL) { *magic = (uint32_t)m; *shift = (uint32_t)(p - 32); }
}

static void fill_resampler_index(const fmd_config *c, const fmd_taps *t, fmdk_params *k) {
  (void)t;
  k->size = c->size;
  k->half = c->size >> 1;
  k->mode = c->mode;
  k->slow = c->rate_out2 > 0 ? c->rate_out2 : 1;
  k->fast = c->rate_out2 > 0 ? c->rate_out : 1;
  k->inv_slow = 1.0f / (float)k->slow;      /* the estimates of the kernels' generic (no magic number) index forms */
  k->inv_fast = 1.0f / (float)k->fast;
  k->resample = c->rate_out2 > 0;
  /* floor(n / slow) for n < 2^29 as mulhi(n, m) >> sh: with l = ceil(log2 slow), p = 29 + l and
   * m = ceil(2^p / slow) the error term m slow - 2^p is below slow, so n (m slow - 2^p) < 2^p for every
   * n < 2^29 and the quotient is exact; m < 2^30 + 1 fits 32 bits.  Needs p >= 32, i.e. slow >= 5. */
  if (k->resample && k->slow >= 5 && (long long)k->fast * 600 < (1LL << 29))     /* numerators: < (frames per tile + 1) fast */
    magic_div(k->slow, 29, &k->emit_magic, &k->emit_shift);
  /* the same for the frames of a tile, floor((acc + tile slow) / fast): numerators below 2^30, p = 30 + l */
  if (k->resample && k->fast >= 5 && (long long)k->fast + (long long)fmdk_tile() * k->slow < (1LL << 30))
    magic_div(k->fast, 30, &k->tf_magic, &k->tf_shift);
  k->perm4 = k->resample && (4ll * k->fast) % k->slow == 0 && (((4ll * k->fast) / k->slow) & 1);
}

static void fill_warmup(const fmd_config *c, const fmd_taps *t, fmdk_params *k) {   /* (after k->deemph) */
  (void)t;
  /* Restart distance for the de-emphasis recurrence of the exact kernels.  A restarted trajectory is
   * within one fp32 ulp of the true one once lambda^n < 1e-7; from there a surviving 1-ulp difference
   * rounds away with probability ~ (1 - lambda) per step, i.e. survives k more steps with lambda^k.
   * lambda^warm < 1e-25 leaves 1e-18 per restart: with the 1.3 million restarts of a 256 x 16 block
   * launch, 1e-12 per launch that a carried state is one ulp off (round 1 used 1e-12: 6e-8 per restart). */
  int warm = 0;
  if (k->deemph) {
    const double lam = fabs((double)c->deemph_lambda);
    if (lam <= 0.0) warm = 1;
    else if (lam >= 1.0) warm = 1 << 30;   /* not contracting: never restart */
    else warm = (int)ceil(log(1e-25) / log(lam));
    if (warm < 16) warm = 16;
    if (warm < (1 << 29)) warm = (warm + 15) & ~15;   /* the kernel restarts in whole 16-frame blocks */
  }
  k->warm = warm;
  k->warm_fast = 0;
  if (k->deemph) {
    const double lam = fabs((double)c->deemph_lambda);
    k->warm_fast = (lam > 0.0 && lam < 1.0) ? (int)ceil(log(1e-9) / log(lam)) : warm;
    if (k->warm_fast < 1) k->warm_fast = 1;
  }
}

static void fill_params(const fmd_config *c, const fmd_taps *t, int pcm_stride, fmdk_params *k) {
  memset(k, 0, sizeof(*k));
  memcpy(k->fb, t->fb, sizeof(k->fb));
  memcpy(k->fm, t->fm, sizeof(k->fm));
  memcpy(k->fp, t->fp, sizeof(k->fp));
  memcpy(k->fs, t->fs, sizeof(k->fs));
  for (int j = 0; j < 127; j++) k->fm_sh[j] = t->fm[j + 1];
  k->mono_2to1 = c->math != FMD_MATH_EXACT && c->mode == 1 && c->size == 128 && c->rate_out2 > 0 &&
                 c->rate_out == 2 * c->rate_out2;
  k->swf = t->swf;
  k->cwf = t->cwf;
  k->coef = c->volume * 32768.0f;               /* src/rtl_fm_player.c:717 */
  k->offset_tuning = c->offset_tuning != 0;
  k->block_len = c->block_len;
  k->pcm_stride = pcm_stride;
  fill_decimator(c, t, k);
  fill_deemph_flush(c, t, k);
  fill_thresholds(c, t, k);
  fill_resampler_index(c, t, k);
  fill_warmup(c, t, k);
}

/* The fmd_fused_kernel instantiation a resolved family runs (fmd_kernels.inc builds exactly these). */
static fmdk_variant variant_of(int math, const fmdk_params *k) {
  fmdk_variant v;
  v.ex = math == FMD_MATH_EXACT;
  /* rate_out2 <= 0: full_demod skips lp_real_f32 altogether (src/rtl_fm_player.c:781) - the mode-0 kernel, whatever lpr.mode says */
  v.mode = (int8_t)(k->resample ? k->mode : 0);
  /* 90-tap stereo and 128-tap mono have kernels specialised for their size; every other size runs the generic one */
  v.half = (int8_t)(((v.mode == 2 && k->half == 45) || (v.mode == 1 && k->half == 64)) ? k->half : 0);
  /* FMD_MATH_FAST_MFMA: stage A on the matrix pipe; _MFMA_F: every stage that has a matrix form, where resolve_family found the decimating second
   * stage applicable (dec_p > 0: 90-tap stereo or 128-tap mono), else stage A only */
  v.mx = (int8_t)(math == FMD_MATH_FAST_MFMA_F && k->dec_p > 0 ? 2 : (math == FMD_MATH_FAST_MFMA || math == FMD_MATH_FAST_MFMA_F) ? 1 : 0);
  return v;
}

/* Configuration -> kernel family and launch parameters (r->cfg.math, r->taps, r->kp): everything fmd_batch_create decides before it touches
 * the device.  FMD_MATH_FAST and the named +-1 LSB families resolve downwards to what the configuration can run. */
int fmdk_resolve(const fmd_config *cfg, const fmd_taps *taps, fmdk_resolved *r) {
  int rc = fmdk_check_config(cfg);
  if (rc) return rc;
  memset(r, 0, sizeof(*r));
  r->cfg = *cfg;
  /* FMD_MATH_FAST = the fastest +-1 LSB kernel family for the configuration: FMD_MATH_FAST_MFMA_F where it applies, else FMD_MATH_FAST_MFMA, else (a
   * caller's decimator taps beyond the 26-bit form) FMD_MATH_FAST_VALU.  The names of the families round 6 retired (_MFMA_C / _D / _E: include/fmdemod_mi355x.h)
   * are accepted and mean FMD_MATH_FAST. */
  if (r->cfg.math == FMD_MATH_FAST || r->cfg.math == FMD_MATH_FAST_MFMA_C || r->cfg.math == FMD_MATH_FAST_MFMA_D || r->cfg.math == FMD_MATH_FAST_MFMA_E)
    r->cfg.math = FMD_MATH_FAST_MFMA_F;
  if (taps) r->taps = *taps;
  else if ((rc = fmd_design_taps(cfg, &r->taps))) return rc;
  r->pcm_stride = (max_result_len(cfg) + 7) & ~7;
  fill_params(&r->cfg, &r->taps, r->pcm_stride, &r->kp);
  /* The second-stage filters in fixed point, each quantised once, before any gate reads them: q[0..2] = fm, fp, fs and q[3] = the composite g (stereo),
   * q[0] = fm (mono); and what the form adds to a PCM value - err[] = g, fm (stereo) / fm (mono) - whatever family the gates then choose. */
  double h[256];
  const double coef = (double)r->kp.coef;
  if (cfg->rate_out2 > 0 && cfg->mode == 2 && cfg->size == 90) {
    const float *half[3] = {r->taps.fm, r->taps.fp, r->taps.fs};
    for (int f = 0; f < 3; f++) { fm_full(half[f], 90, h); quantise_taps(h, 90, &r->q[f]); }
    composite_taps(r->taps.fm, h);
    quantise_taps(h, 179, &r->q[3]);
    if (r->q[3].n) r->err[0] = fixed_point_error(&r->q[3], coef);
    if (r->q[0].n) r->err[1] = fixed_point_error(&r->q[0], coef);
    r->n_err = r->q[3].n && r->q[0].n ? 2 : 0;
  } else if (cfg->rate_out2 > 0 && cfg->mode == 1 && cfg->size == 128) {
    fm_full(r->taps.fm, 128, h);
    if (quantise_taps(h, 128, &r->q[0]) == 0) { r->err[0] = fixed_point_error(&r->q[0], coef); r->n_err = 1; }
  }
  if (r->cfg.math == FMD_MATH_FAST_MFMA_F) {
    /* What _MFMA_F needs; a configuration that lacks any of it runs the stage-A family, also when the caller named this one (it is a speed choice inside
     * one +-1 LSB contract).  Whole tiles (block_len a multiple of 8192 bytes) and the resampler on; the fixed-point forms of the filters fit their
     * accumulators (build_ci_scales*); rate_out >= 4 rate_out2 (stereo) / 2 rate_out2 (mono), the kernels' magic numbers exist and the second stage's
     * error estimate stays below FMD_STAGE_D_MAX_LSB (stage_d_on_matrix_pipe; stereo: the composite L+R filter's likewise, build_lr_composite); and
     * sixteen frames are a whole number P of samples, P a multiple of four (the groups' sample windows start P c - K0 bytes into the limb arrays: dword
     * reads) with the window K0 + P inside the K slices the kernels run: P <= 100 for stereo (five slices for the composite filter, three for fm),
     * 32 .. 128 for mono (four; below 64 a tile holds more than eight groups of sixteen frames: a column per group, fmdk_params.dec_wide). */
    const int whole = r->cfg.rate_out2 > 0 && (r->cfg.block_len % (16 * FMDK_TILE)) == 0;
    const long long p16 = 16LL * r->kp.fast, P = (r->kp.slow > 0 && p16 % r->kp.slow == 0) ? p16 / r->kp.slow : 0;
    int ok = 0;      /* (each step writes into kp as it goes, also where a later one fails: the order is part of the kernel arguments) */
    if (r->cfg.mode == 1)
      ok = whole && r->cfg.size == 128 && keeps_limb_range(r->taps.fm, 64) && build_ci_scales(r->q, 1, &r->kp) == 0 &&
           stage_d_on_matrix_pipe(&r->taps, &r->kp, &r->err[0]) && P % 4 == 0 && P >= 32 && P <= 128;
    else if (r->cfg.mode == 2)
      ok = whole && r->cfg.size == 90 && build_ci_scales(r->q, 3, &r->kp) == 0 && stage_d_on_matrix_pipe(&r->taps, &r->kp, &r->err[1]) && P % 4 == 0 &&
           P >= 64 && P <= 100 && build_lr_composite(&r->q[3], &r->err[0], &r->kp) == 0;
    if (ok) {
      r->kp.dec_p = (int32_t)P;
      r->kp.dec_wide = r->cfg.mode == 1 && P < 64;
    } else {
      r->cfg.math = FMD_MATH_FAST_MFMA;
    }
  }
  if (r->cfg.math == FMD_MATH_FAST_MFMA || r->cfg.math == FMD_MATH_FAST_MFMA_F) {
    /* caller-supplied decimator taps too large for the 26-bit fixed-point form: the vector-ALU kernels take any taps */
    if (build_a_tab(&r->taps, r->cfg.offset_tuning != 0, &r->kp) != 0) {
      if (cfg->math == FMD_MATH_FAST_MFMA || cfg->math == FMD_MATH_FAST_MFMA_F) { return fmd_fail(FMD_E_UNSUPPORTED, "decimator taps beyond +-0.1245: FMD_MATH_FAST_MFMA needs |fb| < 2^-3.005"); }
      r->cfg.math = FMD_MATH_FAST_VALU;
    }
  }
  r->var = variant_of(r->cfg.math, &r->kp);
  return FMD_OK;
}

/* The tap tables of the decimating second stage (csrc/stage_d.inc), as the kernel reads them: for byte phase r = 0 .. 15 and limb l = 0 .. 2, byte y of the
 * table = limb l of T[Y0 - r - y] (zero outside the filter), T = round(h 2^qf) in three balanced int8 limbs, Y0 = P - 1 + K0.  Stereo: the composite filter
 * (179 taps, gq, K0 180, 416 bytes per table) and behind it fm (90 taps, K0 92, 288 bytes); 128-tap mono: fm (K0 128, 368 bytes).  Returns malloc'd bytes. */
uint8_t *fmdk_dec_tables(const fmdk_resolved *r, size_t *bytes) {
  const fixed_taps *g = &r->q[3], *fm = &r->q[0];
  const int stereo = r->cfg.mode == 2, P = r->kp.dec_p;
  const int fn = stereo ? FMDK_DF_N : FMDK_DM_N, k0f = stereo ? FMDK_DEC_K0F : FMDK_DEC_K0M;
  const size_t gbytes = stereo ? (size_t)16 * 3 * FMDK_DG_N : 0, fbytes = (size_t)16 * 3 * (size_t)fn;
  uint8_t *t = (uint8_t *)calloc(1, gbytes + fbytes);
  if (!t) return NULL;
  for (int ph = 0; ph < 16; ph++)
    for (int l = 0; l < 3; l++) {
      if (stereo)
        for (int y = 0; y < FMDK_DG_N; y++) {
          const int u = P - 1 + FMDK_DEC_K0G - ph - y;
          if (u >= 0 && u < 179) t[((size_t)ph * 3 + l) * FMDK_DG_N + y] = limb_byte(g->T[u < 90 ? u : 178 - u], l);   /* (kp.gq, mirrored as the kernel reads it) */
        }
      for (int y = 0; y < fn; y++) {
        const int u = P - 1 + k0f - ph - y;
        if (u >= 0 && u < fm->n) t[gbytes + ((size_t)ph * 3 + l) * (size_t)fn + y] = limb_byte(fm->T[u], l);
      }
    }
  *bytes = gbytes + fbytes;
  return t;
}

int fmd_config_family(const fmd_config *cfg, const fmd_taps *taps) {
  fmdk_resolved r;
  const int rc = fmdk_resolve(cfg, taps, &r);
  return rc ? rc : r.cfg.math;
}

/* Time chunks per stream for a launch of n_blocks blocks that replays warm_tiles tiles.  Cut each stream's tiles into time chunks until the grid offers
 * enough workers (wavefronts) per CU; each chunk > 0 replays warm_tiles tiles first (see the kernel), so keep chunks at least 4x longer than the
 * replay.  (8x until round 3: a one-block launch of 256 streams then ran as four chunks per stream = ONE wave per SIMD, which takes 7 us per tile
 * with nobody to hide its latencies under - 0.094 ms; eight chunks of 4 + 1 tiles, two waves per SIMD: profiles/archive/r03y_blocks_per_launch.txt) */
static int plan_chunks(const fmdk_resolved *r, int n_streams, int n_cus, int time_split, int n_blocks, int dbg, int warm_tiles) {
  if (warm_tiles <= 0 || time_split < 0) return 1;
  const int per_cu = time_split > 0 ? time_split : fmdk_workers_per_cu(&r->var, dbg, NULL);
  const long long m = r->kp.block_len >> 4, tile = fmdk_tile();
  const long long tiles = ((m + tile - 1) / tile) * n_blocks;
  long long want = ((long long)per_cu * n_cus + n_streams - 1) / n_streams;
  /* short launches: when three workers per SIMD would leave chunks under six replays' length, two per SIMD with longer
   * chunks are faster (stereo, 2 blocks x 256 streams: 0.100 ms against 0.110) */
  if (time_split == 0 && per_cu >= 12 && tiles < 6LL * warm_tiles * want) {   /* (kernels budgeted for two per SIMD already are) */
    const long long want2 = ((long long)(per_cu - per_cu / 3) * n_cus + n_streams - 1) / n_streams;
    if (want2 < want) want = want2;
  }
  const long long most = tiles / (4LL * warm_tiles);
  if (want > most) want = most;
  return want > 1 ? (int)want : 1;
}

/* The kernel arguments of a launch of n_blocks blocks per stream (dbg: with debug taps). */
fmdk_params fmdk_launch_params(const fmdk_resolved *r, int n_streams, int n_cus, int time_split, int n_blocks, int dbg) {
  fmdk_params kp = r->kp;
  kp.n_blocks = n_blocks;
  kp.n_streams = n_streams;
  kp.warm_tiles = fmdk_warm_tiles(&kp, &r->var);
  kp.n_chunks = plan_chunks(r, n_streams, n_cus, time_split, n_blocks, dbg, kp.warm_tiles);
  return kp;
}

int fmdk_plan_launch(const fmd_config *cfg, const fmd_taps *taps, int n_streams, int n_blocks, int n_cus, int dbg, fmdk_plan *out) {
  fmdk_resolved r;
  const int rc = fmdk_resolve(cfg, taps, &r);
  if (rc) return rc;
  const fmdk_params kp = fmdk_launch_params(&r, n_streams, n_cus, 0, n_blocks, dbg);
  out->family = r.cfg.math;
  out->v = r.var;
  out->workers_per_cu = fmdk_workers_per_cu(&r.var, dbg, &out->kernel_per_simd);
  out->warm_tiles = kp.warm_tiles;
  out->n_chunks = kp.n_chunks;
  return FMD_OK;
}

int fmd_config_error_estimate(const fmd_config *cfg, const fmd_taps *taps, fmd_error_estimate *out) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  memset(out, 0, sizeof(*out));
  fmdk_resolved r;
  const int rc = fmdk_resolve(cfg, taps, &r);
  if (rc) return rc;
  out->family = r.cfg.math;
  out->limit_rms_lsb = (float)FMD_STAGE_D_MAX_LSB;
  out->filters = r.n_err;
  for (int i = 0; i < r.n_err; i++) {                   /* what the resolver found for the limbs the kernel uses: nothing is computed again here */
    const stage_error *e = &r.err[i];
    out->f[i].taps = e->n;
    out->f[i].qf = e->qf;
    out->f[i].rms_lsb = (float)e->rms;
    out->f[i].worst_samples_lsb = (float)e->worst_samples;
    out->f[i].worst_taps_lsb = (float)e->worst_taps;
    out->f[i].worst_dropped_lsb = (float)e->worst_dropped;
    out->f[i].worst_lsb = (float)(e->worst_samples + e->worst_taps + e->worst_dropped);
  }
  return FMD_OK;
}
