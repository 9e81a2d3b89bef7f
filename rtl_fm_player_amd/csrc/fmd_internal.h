/*
 * fmd_internal.h - private interface between the C host layer (fmd_host.c, fmd_objects.c, fmd_resolve.c, fmd_recv.c)
 * and the HIP kernel launchers (fmd_kernels.inc, built as three translation units; the receivers' fmd_kernels_recv.hip).  Not installed, not exported
 * (csrc/fmdemod_mi355x.map).
 */
#ifndef FMD_INTERNAL_H
#define FMD_INTERNAL_H

#include <stdint.h>

#include "fmdemod_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMDK_TILE 512         /* rate_in samples per tile: 64 lanes x 8 outputs           */
#define FMDK_WAVES 4          /* workers (wavefronts) per workgroup                       */
#define FMDK_DG_N 416         /* bytes per (byte phase, limb) of the decimating second stage's tap tables: composite L+R filter, */
#define FMDK_DF_N 288         /* ... fm (90 taps), */
#define FMDK_DM_N 368         /* ... fm (128 taps, mono) */
#define FMDK_DEC_K0G 180      /* the window's first sample before the tile's first, per filter (resample_tile_dec / resample_mono_dec) */
#define FMDK_DEC_K0F 92
#define FMDK_DEC_K0M 128
#ifndef FMDK_FRAME_CAP
#define FMDK_FRAME_CAP 512    /* pending resampler outputs (floats) per worker before a flush */
#endif

/* Uniform launch parameters, passed by value in the kernarg segment so that
 * tap reads with constant indices become scalar loads. */
typedef struct fmdk_params {
  float fb[16];           /* /8 IQ low-pass, half (reference lp_filter_f32)      */
  float fbs[16];          /* fast path: fb / 128 (exact scaling)                 */
  float c_i, c_q;         /* fast path: constant terms of the folded offset      */
  float fm[128], fp[128], fs[128];
  float fm_sh[128];       /* fm shifted by one tap (fm_sh[i] = fm[i + 1]): tap pairs that start on an odd tap as
                             aligned scalar pairs (resample_mono_2to1) */
  float swf, cwf, lambda, coef;
  float lam_pow[16];        /* lambda^(j+1), j = 0..15: the fast kernels' blocked de-emphasis */
  float lam_scan[8];        /* fast kernels' per-tile flush: lambda^(flush_g 2^k), k = 0..7 (zero with de-emphasis off) */
  float lam_eff;            /* lambda, or 0 with de-emphasis off (the fast flush then passes x through)  */
  float log2_a;             /* log2(lambda^flush_g), -1e30 with de-emphasis off: a^(i+1) = exp2((i+1) log2_a) */
  float car_inv_k2;         /* fast stereo: 1 / K^2, K = radius of (x, y) per unit |vs| below which the
                               regenerated 38 kHz carrier is redone exactly (fmd_kernels.inc, carrier_fast) */
  float inv_slow;           /* 1.0f / (float)slow: the generic emit-index form's estimate (made by the host: as a division in the kernel's prologue it held a register for the kernel's whole life) */
  float inv_fast;           /* 1.0f / (float)fast: tile_frames' estimate, likewise */
  float car_inv_k2_l2;      /* ... and 1 / (L K)^2: below L K the redo recomputes the window from the IQ words, between L K and K it
                               sums the worker's own window in the reference's order (redo_carrier, step 0)                 */
  int32_t size, half, mode;
  int32_t slow, fast;     /* rate_out2, rate_out                                 */
  int32_t resample;       /* rate_out2 > 0                                       */
  int32_t deemph, offset_tuning;
  int32_t warm;           /* de-emphasis warm-up frames for restarted segments   */
  int32_t block_len;      /* bytes per block                                     */
  int32_t n_blocks;
  int32_t pcm_stride;     /* int16 per (stream, block)                           */
  int32_t n_streams;
  int32_t n_chunks;       /* time chunks (workers) per stream                    */
  int32_t perm4;          /* resampler: four frames are a whole, odd number of samples apart (lane map)   */
  int32_t warm_fast;      /* frames after which a zero de-emphasis state is right to 1e-9 */
  int32_t warm_tiles;     /* tiles a chunk > 0 replays before its first tile     */
  uint32_t emit_magic, emit_shift;   /* resampler emit index: floor(n / slow) = mulhi(n, magic) >> shift for n < 2^29
                                        (0: slow too small for a 32-bit magic number, the kernel divides by float estimate) */
  int32_t mono_2to1;      /* fast mono, 128 taps, rate_out == 2 rate_out2: the four-frames-per-lane resampler */
  uint32_t tf_magic, tf_shift;       /* frames of a tile: floor(x / fast) = mulhi(x, magic) >> shift for x < 2^30 (0: divide) */
  int32_t flush_g;        /* fast kernels: frames per lane in the per-tile flush (2 mono only, 4 or 8): the smallest with
                             ceil(frames per tile / flush_g) x channels <= 64 lanes */
  /* matrix-pipe form of stage A (FMD_MATH_FAST_MFMA, v_mfma_i32_16x16x64_i8): the 32 decimator taps with the j^n
   * rotation signs as 26-bit fixed point, E = sgn * round(fb * 2^26) = l0 2^16 + l1 2^8 + l2 with balanced int8 limbs.
   * a_tab[limb][comp][d][4 dwords] = the 16 window bytes (8 IQ samples, I and Q slots) that taps 8d .. 8d+7 occupy in
   * the sum of component comp (0 = I, 1 = Q): the A operand of lane (row = 2 r + comp, g) for K slice s is entry
   * d = 4 s + g - r, zero outside 0..3 (fmd_resolve.c, build_a_tab). */
  int32_t a_tab[3 * 2 * 4 * 4];
  float a_bias_i, a_bias_q;          /* 2^-34 * sum of E over the window: the (u - 127.5) offset of the reference's table */
  /* matrix-pipe form of stage C (FMD_MATH_FAST_MFMA_F, 90-tap stereo): taps of filter f (fm, fp, fs) as T = round(h 2^qf) in three
   * balanced int8 limbs (the kernel builds its byte tables from fm / fp / fs and qf), samples as round(v 2^20):
   * y = ci_scale[f] (A0 + A1 2^-8 + A2 2^-16 + A3 2^-24), ci_scale = 2^(32 - 20 - qf)  (fmd_kernels.inc, mpx_tile_i8) */
  int32_t ci_qf[3];
  float ci_scale[3];
  /* ... whose second stage reads limbs: stage C hands (L-R) x carrier over as round(x 2^20) in three int8 limbs,
   * so its sums are put together at 2^20 times their value: ci_scale_q = 2^20 ci_scale, and the carrier's margin r^2 / K^2 - vs^2 is
   * taken with the scaled vs: car_inv_k2_q = 2^40 / K^2 (stage_c.inc, mpx_tile_i8; stage_d.inc, resample_tile_dec) */
  float ci_scale_q[3];
  float car_inv_k2_q;
  /* fast kernels: decimated samples with |I| + |Q| <= org_thr are redone in the reference's arithmetic (stage B).  1e-3 where it was
   * validated (narrow FM at the reference's default volume and everything with a larger PCM step per unit of discriminator error);
   * grows with coef x (largest tap of the filter behind the discriminator) beyond that: the phase error of such a sample is
   * (decimator difference) / magnitude and reaches the PCM through one tap */
  /* FMD_MATH_FAST_MFMA_F stereo: the L+R chain as one filter g = fm * fm (179 taps, symmetric) over the discriminator output: T_g = round(g 2^g_qf)
   * in three balanced int8 limbs, gq[u] = T_g[u] = T_g[178 - u] for u <= 89; y = g_scale (A0 + A1 2^-8 + A2 2^-16), g_scale = 2^(12 - g_qf);
   * g_unit = 2^-g_qf turns a T_g into its tap for the cold paths (cold_paths.inc: q1_patch_i8, lr_head_fix) */
  int32_t gq[90];
  int32_t g_qf;
  float g_scale, g_unit;
  int32_t dec_p;                 /* FMD_MATH_FAST_MFMA_F: 16 rate_out / rate_out2 = samples per sixteen frames (a multiple of four in 64 .. 100), 0: the family does not apply (resample_tile_dec) */
  const void *dec_tables;        /* ... device memory, made once per batch by the host (fmd_resolve.c, fmdk_dec_tables): the sixteen byte phases of the reversed, zero-padded
                                    limb tables the decimating second stage reads - stereo: 16 x 3 x FMDK_DG_N bytes of the composite filter, then 16 x 3 x FMDK_DF_N of
                                    fm; 128-tap mono: 16 x 3 x FMDK_DM_N of fm.  The kernel's prologue copies them into LDS (one 16-byte word per thread and step) */
  int32_t dec_wide;              /* ... mono: more than eight groups of sixteen frames per tile (rate_out < 4 rate_out2): a column per group (resample_mono_dec) */
  int32_t pilot_pairs8;          /* matrix-pipe stage C: the pilot filter's class-3 limb pairs too (volume >= 1: the carrier's accuracy in LSB scales with it) */
  float org_thr, org_thr15;      /* (and 1.5 x it: the lane-level pre-test on max(|cross|, |dot|)) */
} fmdk_params;

/* Which fmd_fused_kernel<EX, MODE, HALF, MX, DBG> a batch runs (fmd_resolve.c, variant_of; fmd_kernels.inc builds exactly these):
 * ex = 1 for FMD_MATH_EXACT; mode = lpr.mode, 0 without the resampler; half = 45 / 64 for the specialised 90-tap stereo / 128-tap mono kernels,
 * 0 for the generic size; mx = matrix-pipe stages, 0 none, 1 stage A, 2 every stage that has a matrix form (only where fmdk_params.dec_p > 0). */
typedef struct fmdk_variant {
  int8_t ex, mode, half, mx;
} fmdk_variant;

/* Launch the fused IQ->PCM kernel of variant v for n_streams streams (dbg with any tap set: its DBG build; d_lv_part not NULL: its LV build,
 * which writes each tile's level partials there - float2 [n_streams][n_blocks][tiles per block]).  Returns 0 or a
 * hipError_t (> 0).  All pointers are device pointers.  ev_start / ev_stop: hipEvent_t or NULL - recorded with the
 * kernel's own dispatch packet (hipExtLaunchKernelGGL), not as packets of their own around it. */
int fmdk_launch(const fmdk_params *p, const fmdk_variant *v, int n_streams, const void *d_iq, void *d_pcm,
                void *d_lens, const void *d_state_in, void *d_state_out, const fmd_debug_taps *dbg, void *d_lv_part,
                void *hip_stream, void *ev_start, void *ev_stop);
/* The finish kernel of a levels launch (levels.inc): per stream and block, the level from the LV kernel's tile partials into d_levels (NULL:
 * none) and - d_thr not NULL - the power squelch over d_hits (lens = 0 and the PCM slot zeroed for a closed block).  Plain launch on `stream`;
 * returns 0 or a hipError_t. */
int fmdk_levels(const void *d_part, int n_streams, int n_blocks, int block_len, int pcm_stride, void *d_levels, void *d_lens, void *d_pcm,
                const float *d_thr, int32_t *d_hits, int conseq, void *stream);
/* The capture spectrum (spectrum.inc).  _built: 1 for the n_bins the kernel is instantiated for.  _table_floats / _tables: the device table of
 * a (n_bins, window) pair - window, then the pass twiddles - made on the host in double and rounded once; *sum_w2 = sum of w^2.  fmdk_spectrum: one
 * workgroup per (stream, block), n_slots = n_streams x n_blocks; scale = 1 / (nseg n_bins sum_w2); plain launch on `stream`; 0 or a hipError_t. */
int fmdk_spectrum_built(int n_bins);
size_t fmdk_spectrum_table_floats(int n_bins);
void fmdk_spectrum_tables(int n_bins, int window, float *out, double *sum_w2);
int fmdk_spectrum(const void *d_iq, int n_slots, int block_len, int n_bins, const float *d_tab, double scale, void *d_power, void *stream);
/* The MPX subcarrier receiver (subcarrier.inc; the device-free helpers are fmd_recv.c's).  _check: the supported range of the header, FMD_OK or a
 * status with fmd_last_error's text.  _period: Pd = rate_in / gcd(fc, rate_in).  _carrier: the table 2 exp(-2 pi i ((p fc) mod R) / R), Pd {re, im} pairs,
 * in double, rounded once.  fmdk_subc_launch: the receiver kernel over n_streams x n_blocks blocks - one workgroup per (stream, block, chunk of
 * FMDK_SUBC_CHUNK samples) - and behind it on the same stream the state kernel (d_state: fmd_subc_state[n_streams], read by the first, advanced in
 * place by the second).  Plain launches on `stream`; 0 or a hipError_t. */
#define FMDK_SUBC_CHUNK 4096
int fmdk_subc_check(const fmd_subc_config *c);
int fmdk_subc_period(const fmd_subc_config *c);
void fmdk_subc_carrier(const fmd_subc_config *c, float *tab);
int fmdk_subc_launch(const void *d_v, int n_streams, int n_blocks, const fmd_subc_config *c, int period, const float *d_taps, const float *d_carrier,
                     void *d_state, void *d_z, void *stream);
/* The RDS receiver (rds.inc; the device-free part is fmd_rds.c).  _geometry: the integers of the header's definition - 2 rate_z, Pw, Hh = ceil(S/2),
 * L = Hh + 2, Hb = ceil(S), Hy = L + Hb + Hh and the soft-bit slot (the largest count of a block, rounded up to a multiple of 4).  _check: the supported
 * range.  _table: w, Pw {re, im} pairs, in double, rounded once.  fmdk_rds_launch: matched filter (one workgroup per stream, block and chunk of
 * FMDK_RDS_CHUNK samples; y into d_y, the chunk's partial sums into d_part), tracker (one workgroup per stream; d_blk), slicer (one per stream and
 * block) and the state kernel, in this order on `stream`; 0 or a hipError_t.  Scratch, per stream and block: d_y float2 [Bz], d_part float4
 * [chunks], d_blk fmdk_rds_blk. */
#define FMDK_RDS_Q 2375             /* 2 fb: a bit is 2 rate_z / 2375 samples */
#define FMDK_RDS_CHUNK 1024
#define FMDK_RDS_MAX_BLOCK 65536
typedef struct fmdk_rds_geom { int32_t two_rz, pw, hh, lb, hb, hy, slot; } fmdk_rds_geom;
typedef struct fmdk_rds_blk { float ts[2], phi, pw, tm[2]; int32_t count, e0; int64_t first; } fmdk_rds_blk;      /* e0: 2375 x (first bit's instant - (n0 - L - Hb)) */
void fmdk_rds_geometry(int rate_z, int block_z, fmdk_rds_geom *g);
int fmdk_rds_check(const fmd_rds_config *c);
void fmdk_rds_table(const fmd_rds_config *c, float *tab);
int fmdk_rds_launch(const void *d_z, int n_streams, int n_blocks, const fmd_rds_config *c, const fmdk_rds_geom *g, const float *d_taps, const float *d_w,
                    void *d_state, void *d_y, void *d_part, void *d_blk, void *d_soft, void *d_lens, void *d_first, void *d_est, void *stream);
/* The channel tuner (tuner.inc; the device-free helpers are fmd_recv.c's).  _check: the supported range of the header, FMD_OK or a status with
 * fmd_last_error's text.  _table: c[p] = exp(+2 pi i p / P), P {re, im} pairs, from the first octant by symmetry, in double, rounded once.  _channel: a
 * channel's range check and the entry of the device's channel table - sh = shift mod P in 0 .. P-1, sh8 = 8 sh mod P and sh2k = 2048 sh mod P (the
 * table-index steps from one 16-byte word of a thread to its next and from one of its words to the one 256 words on), g = float(128 gain).
 * fmdk_tuner_launch: the tuner kernel - one workgroup per (channel, block, chunk of FMDK_TUNER_CHUNK samples) - and behind it on the same stream the
 * state kernel (d_state: fmd_tuner_state[n_sources], read by the first, advanced in place by the second).  d_y may be NULL.  Plain launches on
 * `stream`; 0 or a hipError_t. */
#define FMDK_TUNER_CHUNK 4096
typedef struct fmdk_tuner_chan { int32_t source, sh, sh8, sh2k; float g; int32_t reserved[3]; } fmdk_tuner_chan;
int fmdk_tuner_check(const fmd_tuner_config *c);
void fmdk_tuner_table(int period, float *tab);
int fmdk_tuner_channel(const fmd_tuner_config *c, int n_sources, const fmd_tuner_channel *ch, fmdk_tuner_chan *out);
int fmdk_tuner_launch(const void *d_iq, int n_sources, int n_channels, int n_blocks, const fmd_tuner_config *c, const float *d_taps, const float *d_table,
                      const void *d_chan, void *d_state, void *d_out, void *d_y, void *stream);
/* The station finder (scan.inc; the device-free part is fmd_recv.c's).  _plan: the supported range of the header (FMD_OK or a status with
 * fmd_last_error's text) and the integers and doubles a launch needs - C, cmax, the floor's rank among the n_used bins, nb = double(2 bw N) /
 * double(rate).  cand (NULL: not wanted; else room for FMD_SCAN_MAX_CANDIDATES entries): per candidate the first signed bin s0 of its band, the
 * number of bins s0 .. s1 and the two edge weights, each one double division of 64-bit integers (count 1: the band IS the bin, both are 1 and
 * the kernel reads w_first).  fmdk_scan_launch: one workgroup per stream; d_chan may be NULL; a plain launch on `stream`; 0 or a hipError_t. */
typedef struct fmdk_scan_cand { int32_t first, count; double w_first, w_last; } fmdk_scan_cand;        /* 24 bytes */
typedef struct fmdk_scan_plan { int32_t n_cand, cmax, rank, n_used; double nb; } fmdk_scan_plan;
int fmdk_scan_plan_make(const fmd_scan_config *c, fmdk_scan_plan *p, fmdk_scan_cand *cand);
int fmdk_scan_launch(const void *d_power, int n_streams, int n_blocks, const fmd_scan_config *c, const fmdk_scan_plan *p, const void *d_cand,
                     void *d_stations, void *d_counts, void *d_chan, void *stream);
/* Stereo control (stereo.inc; the device-free part is fmd_recv.c's).  fmdk_stereo_plan: the supported range of the header (FMD_OK or a status
 * with fmd_last_error's text) and the four floats a launch needs, each made in double and rounded once (k may be NULL: the check alone).
 * fmdk_stereo_launch: the pilot meter (one workgroup per stream and block; skipped where d_z is NULL or Mz = 0), the tracker (one workgroup per
 * stream: the only reader and writer of d_state, fmd_stereo_state[n_streams]) and the apply kernel (one per stream and block), in this order on
 * `stream`; d_quality and d_meter may be NULL; 0 or a hipError_t. */
typedef struct fmdk_stereo_k { float thr_on, thr_off, inv_mz, inv_span; } fmdk_stereo_k;
int fmdk_stereo_plan(const fmd_stereo_config *c, fmdk_stereo_k *k);
int fmdk_stereo_launch(const void *d_pcm, const void *d_lens, const void *d_z, const void *d_quality, int n_streams, int n_blocks,
                       const fmd_stereo_config *c, const fmdk_stereo_k *k, int mode, void *d_state, void *d_out, void *d_info, void *d_meter, void *stream);
/* Tiles a time chunk must replay so that every FIR history is exact and the
 * de-emphasis recurrence has converged (0: the launch must not be split). */
int fmdk_warm_tiles(const fmdk_params *p, const fmdk_variant *v);
int fmdk_tile(void);
/* Workers (wavefronts) per CU the host cuts a launch's streams into time chunks for; *kernel_per_simd (if not NULL): the workers per SIMD
 * the kernel's registers are budgeted for (__launch_bounds__).  Where the two differ, fmd_kernels.inc says why. */
int fmdk_workers_per_cu(const fmdk_variant *v, int dbg, int *kernel_per_simd);

/* The launch plan fmd_batch_run_device_debug would make, without a device (tests/c/plan_check.c): family and variant as fmd_batch_create resolves
 * them, the budgets of fmdk_workers_per_cu, and the chunking of n_streams x n_blocks blocks on n_cus CUs. */
typedef struct fmdk_plan {
  int32_t family;
  fmdk_variant v;
  int32_t kernel_per_simd, workers_per_cu, warm_tiles, n_chunks;
} fmdk_plan;
int fmdk_plan_launch(const fmd_config *cfg, const fmd_taps *taps, int n_streams, int n_blocks, int n_cus, int dbg, fmdk_plan *out);

/* ---- the device-free resolver (fmd_resolve.c) ---- */

/* A second-stage filter in the fixed-point form of the matrix-pipe stages: T = round(h 2^qf) in three balanced int8 limbs (quantise_taps), and what that
 * form adds to a PCM value in LSB (fixed_point_error). */
typedef struct { int n, qf; int32_t T[256]; double limb_abs[3]; double sum_abs, sum_sq; } fixed_taps;   /* limb_abs[l] = sum |limb l|; sum |h|, sum h^2 */
typedef struct { double rms, worst_samples, worst_taps, worst_dropped; int qf, n; } stage_error;

/* Everything fmd_batch_create decides before it touches the device: the configuration with cfg.math the RESOLVED family, the taps, the kernel
 * arguments (all but the launch's n_blocks / n_streams / warm_tiles / n_chunks and the dec_tables device pointer), the kernel instantiation and
 * the PCM stride.  Host only, behind them: the quantised second-stage filters (stereo: fm, fp, fs, the composite g; mono: fm; n = 0 where the
 * configuration has none or quantise_taps refused) and the error estimates fmd_config_error_estimate reports (stereo: g, fm; mono: fm). */
typedef struct fmdk_resolved {
  fmd_config cfg;
  fmd_taps taps;
  fmdk_params kp;
  fmdk_variant var;
  int32_t pcm_stride;
  fixed_taps q[4];
  stage_error err[2];
  int n_err;
} fmdk_resolved;
int fmdk_check_config(const fmd_config *c);
int fmdk_resolve(const fmd_config *cfg, const fmd_taps *taps, fmdk_resolved *out);   /* (checks cfg itself) */
/* The tap tables of the decimating second stage as the kernel reads them (var.mx == 2 only): malloc'd, NULL when out of memory. */
uint8_t *fmdk_dec_tables(const fmdk_resolved *r, size_t *bytes);
/* The kernel arguments of a launch of n_blocks blocks per stream (dbg: with debug taps; time_split: fmd_batch_set_time_split). */
fmdk_params fmdk_launch_params(const fmdk_resolved *r, int n_streams, int n_cus, int time_split, int n_blocks, int dbg);
/* The reference's tap formulas, for the reference-shaped surface too (init_lp_real_f32, full_demod). */
void fmdk_design_fb(float *fb);
void fmdk_design_mpx(int size, int rate_in, float *fm, float *fp, float *fs, float *swf, float *cwf);
/* Sets fmd_last_error's text and returns code (fmd_error.c).  Hidden: the export map's fmd_* pattern would otherwise publish it. */
int fmd_fail(int code, const char *fmt, ...) __attribute__((visibility("hidden"), format(printf, 2, 3)));

#ifdef __cplusplus
}
#endif
#endif
