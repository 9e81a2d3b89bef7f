/*
 * fmdemod_mi355x.h - C ABI of the MI355X-native FM demodulation path.
 *
 * Drop-in boundary for the IQ -> PCM hot path of rtl_fm_player
 * (rotate_90_u8_f32 + full_demod, reference src/rtl_fm_player.c:206-226,
 * :758-788).  Plain C, plain pointers and sizes; no HIP or torch types appear
 * in any signature.  Everything here is exported by libfmdemod_mi355x.so
 * (rtl_fm_player_amd/csrc).  The library runs every stage on the GPU with
 * hand-written gfx950 kernels; there is no CPU fallback and every entry point
 * fails (status < 0, or abort() for the void reference-shaped calls) when no
 * HIP device is usable.
 *
 * Three groups of entry points:
 *   1. the reference's own operator surface (same names, same struct layout)
 *      so rtl_fm_player.c can link against this library instead of its own
 *      definitions;
 *   2. a batch API (many independent streams x many blocks per launch) which
 *      is what the bench and the parity tests drive;
 *   3. an rtlsdr_read_async_cb_t-compatible ingest callback feeding a
 *      per-stream pinned staging ring.
 */
#ifndef FMDEMOD_MI355X_H
#define FMDEMOD_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * 1. Reference-shaped surface
 * ------------------------------------------------------------------------
 * Layout-compatible restatement of struct lp_real / struct demod_state
 * (reference include/rtl_fm_player.h:95-110, :127-175; x86-64 glibc).  The
 * reference header cannot be included from a second translation unit (it
 * defines globals), so the layout is restated here and checked with static
 * assertions in csrc/fmd_host.c against the offsets recorded in SURVEY.md
 * section 8a (row a15).  Define FMD_NO_REFERENCE_TYPES before including this
 * header from a TU that already has the reference's own definitions.
 */
#define FMD_DEFAULT_BUF_LENGTH (1 * 16384)                 /* include/rtl_fm_player.h:31 */
#define FMD_MAXIMUM_OVERSAMPLE 16                          /* :32 */
#define FMD_MAXIMUM_BUF_LENGTH (FMD_MAXIMUM_OVERSAMPLE * FMD_DEFAULT_BUF_LENGTH) /* :33 */

#ifndef FMD_NO_REFERENCE_TYPES
/* pthread_rwlock_t is POSIX.1-2001: compile with -std=gnu11 (the reference's CMake default dialect)
 * or define _POSIX_C_SOURCE >= 200112L / _GNU_SOURCE before the first include under strict -std=c11 */
#include <pthread.h>

struct output_state;

struct lp_real {          /* include/rtl_fm_player.h:95-110 */
  float *br;              /* ring of discriminator samples                */
  float *bm;              /* ring of L+R low-pass outputs                 */
  float *bs;              /* ring of demodulated L-R samples              */
  float *fm;              /* half of the symmetric 0..16 kHz low-pass     */
  float *fp;              /* half of the 18..20 kHz pilot band-pass       */
  float *fs;              /* half of the 21..55 kHz L-R band-pass         */
  float swf;              /* sin(2 pi 19000 / rate_in)                    */
  float cwf;              /* cos(2 pi 19000 / rate_in)                    */
  float pp;               /* previous pilot band-pass output              */
  int pos;                /* ring write index                             */
  int size;               /* taps (90 stereo, 128 mono)                   */
  int rsize;              /* size / 2                                     */
  int mode;               /* 0 drop, 1 mono, 2 stereo                     */
};

struct demod_state {      /* include/rtl_fm_player.h:127-175 */
  int exit_flag;
  pthread_t thread;
  uint8_t buf[FMD_MAXIMUM_BUF_LENGTH];
  uint32_t buf_len;
  int16_t lowpassed[FMD_MAXIMUM_BUF_LENGTH << 1];
  int lp_len;
  float lowpass_tb[48];
  int16_t lp_i_hist[10][6];
  int16_t lp_q_hist[10][6];
  int16_t result[FMD_MAXIMUM_BUF_LENGTH];
  int result_len;
  int16_t droop_i_hist[9];
  int16_t droop_q_hist[9];
  int offset_tuning;
  int rate_in;
  int rate_out;
  int rate_out2;
  int now_r, now_j;
  int pre_r, pre_j;
  float pre_r_f32, pre_j_f32;
  int prev_index;
  int downsample;
  int post_downsample;
  int output_scale;
  int squelch_level, conseq_squelch, squelch_hits, terminate_on_squelch;
  int downsample_passes;
  int comp_fir_size;
  int custom_atan;
  double deemph;
  int deemph_a;
  int deemph_l;
  int deemph_r;
  float deemph_l_f32;
  float deemph_r_f32;
  float deemph_lambda;
  float volume;
  int now_lpr;
  int prev_lpr_index;
  struct lp_real lpr;
  pthread_rwlock_t rw;
  pthread_cond_t ready;
  pthread_mutex_t ready_m;
  struct output_state *output_target;
};

/* Same names, arguments and calling protocol as the reference:
 *   fill d->buf / d->buf_len, call rotate_90_u8_f32(d) (or u8_f32(d)), then
 *   full_demod(d), then read d->result_len int16 values from d->result
 *   (src/rtl_fm_player.c:870-889, :904-908).
 * rotate_90_u8_f32 / u8_f32 only record which conversion the next full_demod
 * applies (and set lp_len like the reference); full_demod uploads d->buf,
 * runs the whole chain on the GPU, downloads the PCM and mirrors every
 * mutable state field back into *d (lowpass_tb, pre_*_f32, lpr rings/pos/pp,
 * prev_lpr_index, deemph_*_f32), so CPU and GPU calls can be interleaved on
 * one struct.  They return void like the originals; an unusable device or an
 * unsupported configuration aborts with a message on stderr.
 *
 * One synchronisation per block (round 4): the carried state stays on the device between calls; the library keeps a
 * copy of what it last mirrored into the struct and uploads the struct's state only when the caller has changed it
 * (reset, restore, a CPU block in between) - IQ up, kernel, {PCM, length, new state} down into one pinned block, one
 * wait.  bench.py's `single_stream` leg: 0.10 ms per 262144-byte block against 1.04 ms for the reference on one host core.
 *
 * Limits of this surface (it serves one dongle, like the program it drops into; many streams
 * belong on the batch API below):
 *   - the device side of a struct is found through a registry keyed by the struct's address
 *     (the reference struct has no spare field); fmd_demod_release (or deinit_lp_real_f32) forgets a struct;
 *   - the arithmetic contract is read ONCE, at the first full_demod of the process, from the
 *     environment: FMD_MATH_FAST set -> +-1 LSB kernels, otherwise the bit-exact ones;
 *   - any HIP error is fatal (abort), because the signatures have no way to report it. */
void init_u8_f32_table(void);                       /* src/rtl_fm_player.c:195 */
void init_lp_f32(void);                             /* :241 */
void init_lp_real_f32(struct demod_state *fm);      /* :413 */
void deinit_lp_real_f32(struct demod_state *fm);    /* :455 */
void demod_init(struct demod_state *s);             /* :1156 */
void rotate_90_u8_f32(struct demod_state *d);       /* :206 */
void u8_f32(struct demod_state *d);                 /* :228 */
void full_demod(struct demod_state *d);             /* :758 */
/* Additive: release the device resources full_demod attached to *d. */
void fmd_demod_release(struct demod_state *d);

#endif /* FMD_NO_REFERENCE_TYPES */

/* Additive (declared whether or not FMD_NO_REFERENCE_TYPES is defined: a program that keeps its own struct definitions calls these too): what the void
 * reference-shaped calls cannot say through their signatures.
 *   fmd_dropin_set_math: the arithmetic family of the calls above (an fmd_config.math value), instead of the FMD_MATH_FAST environment variable; call it
 *     before the first full_demod (a struct's batch is rebuilt when the family changes).
 *   fmd_dropin_set_error_handler: by default a failure inside one of the calls above (no device, out of memory, a HIP error) prints a line and abort()s; with
 *     a handler installed it is told (which call, fmd_last_error()'s text) and the call returns with result_len = 0. */
int fmd_dropin_set_math(int math);
typedef void (*fmd_dropin_error_fn)(const char *where, const char *message, void *ctx);
void fmd_dropin_set_error_handler(fmd_dropin_error_fn fn, void *ctx);


/* ------------------------------------------------------------------------
 * 2. Batch API: n_streams independent demodulators, many blocks per launch
 * ------------------------------------------------------------------------ */

/* status codes (0 ok, < 0 error) */
#define FMD_OK 0
#define FMD_E_ARG (-1)          /* bad argument                              */
#define FMD_E_UNSUPPORTED (-2)  /* configuration outside the supported range */
#define FMD_E_NOMEM (-3)
#define FMD_E_HIP (-4)          /* HIP runtime error (see fmd_last_error)    */
#define FMD_E_NODEVICE (-5)     /* no usable gfx950 device                   */
#define FMD_E_STATE (-6)        /* call sequence error                       */

/* arithmetic contract */
#define FMD_MATH_EXACT 0  /* reference operation order, unfused mul/add: bit-exact PCM */
#define FMD_MATH_FAST 1   /* PCM within +-1 LSB: the fastest kernel family of this build for the configuration - FMD_MATH_FAST_MFMA_F where it
                             applies, FMD_MATH_FAST_MFMA otherwise (FMD_MATH_FAST_VALU for a caller's decimator taps beyond the 26-bit form);
                             a caller who wants a particular family names it here instead (the library reads no environment
                             variable for this).  fmd_batch_math() says what a batch runs.  Sharing the device with other
                             MFMA kernels: one packed-fp32 instruction form computed wrong results beside them (round 3); it is
                             gone from the kernels, and every build's device code is linted for it (tools/isa_lint.py over the
                             disassembly of the built library, run by the Makefile) - profiles/archive/r04_pk_opsel_hazard.md.  The
                             hazard is an empirical description of undocumented hardware behaviour: tests/test_gpu_neighbour.py
                             and tests/test_gpu_coresidency.py are the standing check. */
#define FMD_MATH_FAST_VALU 2   /* +-1 LSB, vector ALU only: fused multiply-adds in the reference's summation order */
#define FMD_MATH_FAST_MFMA 3   /* +-1 LSB, matrix pipe beside the vector ALU: the /8 decimator as exact int8 products
                                  of the IQ bytes with 26-bit fixed-point taps (v_mfma_i32_16x16x64_i8); any filter size, ragged tiles */
#define FMD_MATH_FAST_MFMA_F 7 /* +-1 LSB, every stage that has a matrix form there, in int8-limb fixed point with exact integer sums
                                  (samples round(v 2^20), taps round(h 2^qf)).  90-tap stereo: the pilot and L-R filters at full rate
                                  (src/rtl_fm_player.c:538-566), the L+R channel's two low-passes (:545 / :560, :588) as ONE 179-tap
                                  filter fm * fm and the second stage of L-R, both evaluated at the resampler's emit instants only, as
                                  the reference does (:570-598): a decimating banded product - rows = sixteen consecutive frames,
                                  columns = (group of sixteen frames, sample limb).  128-tap mono / narrow FM: the fm low-pass likewise
                                  (:500-532).  Needs whole tiles (block_len a multiple of 8192), sixteen frames a whole number P of
                                  samples, P a multiple of four (stereo: 64 .. 100 - 300 k, 240 k, 192 k -> 48 k; mono: 32 .. 128), and
                                  the fixed-point error estimates of DESIGN.md section 2a below 0.15 LSB (volume up to ~8 at 300 k; narrow
                                  FM up to ~1.7); other configurations run FMD_MATH_FAST_MFMA under this name */
/* retired in round 6 (tools/experiments/retired_round5_families.inc): the intermediate matrix-pipe families of rounds 4 and 5 - stage C alone
 * (_MFMA_C), the second stage at every sample (_MFMA_D), the composite L+R filter at every sample (_MFMA_E).  The names are accepted and mean
 * FMD_MATH_FAST. */
#define FMD_MATH_FAST_MFMA_C 4
#define FMD_MATH_FAST_MFMA_D 5
#define FMD_MATH_FAST_MFMA_E 6

typedef struct fmd_config {
  int32_t rate_in;        /* demod_state.rate_in                               */
  int32_t rate_out;       /* demod_state.rate_out  (resampler "fast")          */
  int32_t rate_out2;      /* demod_state.rate_out2 (resampler "slow"), <=0 off */
  int32_t mode;           /* lpr.mode 0/1/2                                    */
  int32_t size;           /* lpr.size (even, <= 256)                           */
  int32_t deemph;         /* nonzero: de-emphasis on                           */
  int32_t offset_tuning;  /* nonzero: no fs/4 rotation (u8_f32 path)           */
  float deemph_lambda;    /* demod_state.deemph_lambda                         */
  float volume;           /* demod_state.volume                                */
  int32_t block_len;      /* bytes of u8 IQ per block (reference: 262144);     */
                          /* multiple of 16, >= 64                             */
  int32_t math;           /* FMD_MATH_EXACT / FMD_MATH_FAST (/ _VALU / _MFMA / _MFMA_F) */
} fmd_config;

/* Filter tables; fmd_design_taps() fills them exactly as init_lp_f32 /
 * init_lp_real_f32 do (host libm).  A caller may override them (tests hand
 * the device path the very tables the oracle used). */
typedef struct fmd_taps {
  float fb[16];
  float fm[128], fp[128], fs[128];
  float swf, cwf;
} fmd_taps;

/* Carried state of one stream, linear oldest -> newest (mirrors the mutable
 * fields of struct demod_state / struct lp_real). */
typedef struct fmd_stream_state {
  float tb[48];
  float pre_r, pre_j;
  float pp;
  float deemph_l, deemph_r;
  int32_t acc;            /* prev_lpr_index */
  int32_t reserved[2];
  float br[256], bm[256], bs[256];   /* last `size` values, oldest first, at [0..size) */
} fmd_stream_state;

/* Optional stage taps for debugging / parity tests: device pointers or NULL.
 * Shapes per stream and block, M = block_len / 16:
 *   y [2*M] f32, v [M] f32 (before the Q1 overwrite), mpx [M] f32 (resampler
 *   output before de-emphasis, result_len entries used).  prof: see below.
 * A launch with at least one tap runs the debug build of its kernel (same arithmetic, plus the checks
 * and stores the taps need); launches without taps run the build that has none of them (~1 % faster). */
typedef struct fmd_debug_taps {
  void *y, *v, *mpx;
  void *prof;   /* i64 [n_streams][16]: shader-clock cycles per stage, summed over the launch
                   (0 load, 1 decimate, 2 discriminate, 3 q1, 4 mpx, 5 per-tile flush of the fast kernels, 6 resample,
                    7 roll, 8 flush, 9 state in/out, 15 total) */
} fmd_debug_taps;

typedef struct fmd_batch fmd_batch;

int fmd_design_taps(const fmd_config *cfg, fmd_taps *out);
float fmd_deemph_lambda(int output_rate, double tau);   /* src/rtl_fm_player.c:1577 */

/* device < 0: current device.  taps == NULL: fmd_design_taps(cfg). */
int fmd_batch_create(fmd_batch **out, const fmd_config *cfg, const fmd_taps *taps,
                     int n_streams, int device);
void fmd_batch_destroy(fmd_batch *b);

/* int16 slots per (stream, block) in the PCM buffer (multiple of 8). */
int fmd_batch_pcm_stride(const fmd_batch *b);
int fmd_batch_n_streams(const fmd_batch *b);
/* The kernel family this batch runs: FMD_MATH_EXACT, FMD_MATH_FAST_VALU, FMD_MATH_FAST_MFMA or FMD_MATH_FAST_MFMA_F (FMD_MATH_FAST
 * in the configuration resolves to one of the last three at creation; a named family the configuration cannot run resolves likewise). */
int fmd_batch_math(const fmd_batch *b);
/* The same question without a device or a batch: the family fmd_batch_create would run for this configuration (and these taps; NULL:
 * fmd_design_taps), or a negative status for a configuration it would refuse. */
int fmd_config_family(const fmd_config *cfg, const fmd_taps *taps);
/* What the fixed-point second stage of FMD_MATH_FAST_MFMA_F adds to a PCM value for this configuration, in LSB - whether or not the configuration runs it
 * (`family` says what it resolves to): per filter (stereo: [0] the composite L+R filter fm * fm, 179 taps, [1] fm over (L-R) x carrier; mono: [0] fm) the
 * rms ESTIMATE the family is gated on (limit_rms_lsb) and a worst-case BOUND with its three terms - samples rounded to 2^-20, taps rounded to 2^-qf, the
 * limb pairs left out (csrc/fmd_host.c, fixed_point_error).  The other stages' differences to the reference (fused multiply-adds,
 * v_rcp_f32, the exact redo of ill-conditioned samples) have no bound of this kind: tests/, the fuzz and the volume scans vouch for them.  No device needed. */
typedef struct fmd_error_estimate {
  int32_t family, filters;
  struct { int32_t taps, qf; float rms_lsb, worst_lsb, worst_samples_lsb, worst_taps_lsb, worst_dropped_lsb; } f[2];
  float limit_rms_lsb;
} fmd_error_estimate;
int fmd_config_error_estimate(const fmd_config *cfg, const fmd_taps *taps, fmd_error_estimate *out);
/* How a launch is cut into time chunks (one worker wavefront each; results do not depend on it - the tests hold the
 * library to that through this call): workers_per_cu > 0 = cut until the grid offers that many workers per CU,
 * 0 = the kernels' own figure (default), < 0 = never cut (one worker per stream). */
int fmd_batch_set_time_split(fmd_batch *b, int workers_per_cu);

/* fmd_batch_destroy waits for everything the batch has queued (on its own streams and on the
 * caller's stream of the most recent launch, which must therefore still exist) and detaches the
 * ingest rings bound to it: they stay valid and are destroyed by their owner with
 * fmd_ingest_destroy, before or after the batch. */

/* Device-resident run.  Layouts (all device pointers):
 *   d_iq   u8  [n_streams][n_blocks][block_len]
 *   d_pcm  s16 [n_streams][n_blocks][pcm_stride]
 *   d_lens i32 [n_streams][n_blocks]          (result_len of each block)
 * hip_stream: a hipStream_t passed as void* (NULL = the batch's own stream).
 * d_iq must be 16-byte aligned.  Asynchronous; state advances by n_blocks blocks
 * per stream.  Internally each stream's tiles are cut into time chunks so that
 * every CU holds 12 workers; results do not depend on that.
 * Stream rule: a batch's launches form ONE sequence (each reads the state the one before
 * wrote).  They may be queued on different streams - the library inserts the event wait when
 * the stream changes between two launches - but calls on one fmd_batch must come from one
 * thread at a time, and a caller's stream must outlive the work queued on it.  get_state /
 * set_state / reset / sync / destroy wait for the most recent launch whatever stream it is on. */
int fmd_batch_run_device(fmd_batch *b, const void *d_iq, int n_blocks, void *d_pcm,
                         void *d_lens, void *hip_stream);
int fmd_batch_run_device_debug(fmd_batch *b, const void *d_iq, int n_blocks, void *d_pcm,
                               void *d_lens, void *hip_stream, const fmd_debug_taps *dbg);
int fmd_batch_sync(fmd_batch *b);
/* The buffers of a launch must be READY on the stream it runs on: a caller that fills d_iq (or allocates d_pcm / d_lens from a
 * stream-ordered allocator) on another stream synchronises that stream first - or calls this: everything queued on
 * producer_stream so far happens before whatever this batch launches afterwards on its OWN stream (one event record + one wait,
 * no host synchronisation).  Launches with an explicit hip_stream are ordered by that stream and need none of it. */
int fmd_batch_wait_stream(fmd_batch *b, void *producer_stream);

/* Host-buffer convenience (H2D, run, D2H, sync); same layouts in host memory. */
int fmd_batch_run_host(fmd_batch *b, const uint8_t *iq, int n_blocks, int16_t *pcm,
                       int32_t *lens);

/* Per-stream carried state (synchronises first). */
int fmd_batch_get_state(fmd_batch *b, int stream, fmd_stream_state *out);
int fmd_batch_set_state(fmd_batch *b, int stream, const fmd_stream_state *in);
int fmd_batch_reset(fmd_batch *b);

/* Channel level and power squelch.
 *
 * Level of block b of stream s: the reference's rms() (src/rtl_fm_player.c:737-755, step = 1) applied to the float `lowpassed` buffer of
 * that block - n = 2 M interleaved I/Q values, M = block_len / 16 (lp_len, :410) - in real arithmetic, without the integer truncation:
 *   level = sqrt(max(0, S2/n - (S1/n)^2)),  S1 = sum of y[i],  S2 = sum of y[i]^2 over those 2 M floats.
 * The y values are the ones stage B of the running family consumes: the same values the `y` debug tap holds after the launch.  The fused
 * kernel sums them per tile as it goes (the decimated IQ never leaves its registers, so nothing is read twice); a small finish kernel on the
 * same stream right behind it adds the tiles up in double.
 *
 * Squelch takes a per-stream threshold thr[s] (<= 0: off for that stream) and a batch-wide conseq >= 0.  For each stream, the blocks are
 * processed in order across launches:
 *   hits = level < thr ? hits + 1 : 0                         (rtl_fm's power squelch: the step full_demod leaves as a todo, :773)
 *   the block is CLOSED when hits > conseq: then hits = conseq + 1 (the hair trigger of :895-900), the block's lens entry becomes 0 (the
 *   demod thread drops the block) and its pcm_stride PCM slots are zeroed.
 * fmd_batch_set_squelch sets every stream's hits to conseq + 1, and so does fmd_batch_reset while squelch is on: the reference's initial
 * values (squelch_hits 11, conseq_squelch 10, :1160-1163), so a stream starts closed.  Once set, squelch applies to every run path of the
 * batch: fmd_batch_run_device(_debug), fmd_batch_run_host, the pump and the calls below.  The counter lives beside the carried state, not
 * in fmd_stream_state.  The drop-in full_demod ignores squelch_level, as the reference's does.
 *
 * Deliberate departure from rtl_fm: squelch does not zero the decimated signal before the discriminator.  The demodulator state advances
 * exactly as it does without squelch, so open blocks are bit-identical to a run without squelch, the carried state can still be checked
 * against the oracle, and time-chunk replay stays valid.
 *
 * d_levels: f32 [n_streams][n_blocks] device pointer, or NULL (squelch alone).  dbg: as fmd_batch_run_device_debug, or NULL.  While squelch
 * is on, d_pcm must be 16-byte aligned.  fmd_batch_last_kernel_ms keeps timing the fused kernel alone, without the finish kernel.  Inside
 * a hipGraph capture the level scratch cannot grow: run one launch of the captured size before capturing. */
int fmd_batch_run_device_levels(fmd_batch *b, const void *d_iq, int n_blocks, void *d_pcm, void *d_lens,
                                void *d_levels, void *hip_stream, const fmd_debug_taps *dbg);
int fmd_batch_run_host_levels(fmd_batch *b, const uint8_t *iq, int n_blocks, int16_t *pcm, int32_t *lens, float *levels);
/* thresholds: host array of n_streams values, each finite (NULL: squelch off; the counters are kept); conseq in 0 .. 2^30 */
int fmd_batch_set_squelch(fmd_batch *b, const float *thresholds, int conseq);
/* One stream's hits (synchronises); FMD_E_STATE before the first fmd_batch_set_squelch.  set: 0 <= hits <= conseq + 1. */
int fmd_batch_get_squelch_hits(fmd_batch *b, int stream, int32_t *hits);
int fmd_batch_set_squelch_hits(fmd_batch *b, int stream, int32_t hits);

/* Capture spectrum: the averaged power spectrum of each block of the capture (the other half of rtl_power), for a scanner that asks where in
 * the 8 x rate_in of spectrum a stream delivers there is something worth tuning to.
 *
 * Block b of stream s holds L = block_len / 2 complex samples x[n] = (I - 127.5) / 128 + j (Q - 127.5) / 128: the reference's
 * u8_f32_table[0] (src/rtl_fm_player.c:201), WITHOUT the fs/4 rotation - the spectrum of the capture as the dongle delivered it.  With
 * N = n_bins, nseg = floor(L / N) non-overlapping segments are taken from the start of the block; the trailing L - nseg N samples are not used:
 *
 *   P[k] = ( sum_seg | sum_n w[n] x[seg N + n] e^(-2 pi i k n / N) |^2 ) / ( nseg N sum_n w[n]^2 ),   k = 0 .. N - 1
 *
 * Units: linear power in float32, full-scale^2: a complex tone of amplitude A on a bin centre reads A^2 with the rectangular window, and with
 * that window sum_k P[k] is the mean |x|^2 of the used samples (Parseval).  Decibels are the caller's business.  Bin order: natural FFT order -
 * bin k is frequency k fs / N for k < N / 2, otherwise (k - N) fs / N, fs = 8 rate_in.
 * Windows: FMD_WINDOW_RECT w = 1; FMD_WINDOW_HANN w[n] = 0.5 - 0.5 cos(2 pi n / N) (the periodic form).  Window and twiddles are made by the host
 * in double and rounded once to float.
 * Where the demodulated station sits: without offset_tuning the chain multiplies by j^n, so the tuned channel is centred on -fs / 4 = bin 3 N / 4;
 * with offset_tuning it is on bin 0.  (The oracle's DDS multiplex, dds_bytes(262144, amp = 100), peaks at bin 197 of 256, 747 of 1024 and 3149 of
 * 4096 with the rectangular window: tests/test_spectrum_cpu.py.)
 *
 * d_power: f32 [n_streams][n_blocks][n_bins], device pointer, 16-byte aligned.  d_iq as in fmd_batch_run_device (16-byte aligned).
 * n_bins: 256, 1024 or 4096 (FMD_E_UNSUPPORTED otherwise); n_bins <= L.  The call reads no demodulator state and advances none, is no part of the
 * batch's launch sequence, and is the same for every math family, with or without squelch.  The result for a (stream, block) depends on that
 * block's bytes, n_bins and window alone - not on n_streams, n_blocks, the stream's position or how blocks are split into calls - and equal
 * bytes give bit-equal P (no atomics, fixed summation order).
 * hip_stream == NULL: the batch's own stream, so the call is ordered with the demodulator launches queued there; otherwise a plain launch on
 * that stream, which must outlive the work queued on it (fmd_batch_destroy waits for the most recent one).  One thread at a time per batch.
 * The tables of a (n_bins, window) pair are made at its first use, kept in the batch and freed by fmd_batch_destroy.  Inside a stream capture
 * nothing can be allocated: run one call of that (n_bins, window) before capturing.
 * The host form: H2D, kernel, D2H, one wait; iq and power in host memory, same layouts. */
#define FMD_WINDOW_RECT 0
#define FMD_WINDOW_HANN 1
int fmd_batch_spectrum_device(fmd_batch *b, const void *d_iq, int n_blocks, int n_bins, int window,
                              void *d_power, void *hip_stream);
int fmd_batch_spectrum_host(fmd_batch *b, const uint8_t *iq, int n_blocks, int n_bins, int window, float *power);

/* MPX subcarrier receiver: complex down-conversion of the discriminator output at a centre frequency, low-pass, decimation - what rides on the FM
 * multiplex beside the audio.  At fc = 19000 with a narrow filter |z| is the pilot level (the stereo indicator); at fc = 57000 with +-2.4 kHz z is
 * the RDS baseband an RDS decoder takes; 67 kHz / 92 kHz likewise for SCA.  Carrier and bit recovery stay with the caller.
 *
 * Definition.  For one stream let v[n] be the concatenation of all its blocks since the last reset (samples before the reset are zero), M =
 * block_samples floats per block at rate_in.  With T = n_taps, D = decim, R = rate_in:
 *
 *   z[m] = 2 * sum_{k=0}^{T-1} h[k] * v[mD + D-1-k] * exp(-2 pi i * ((mD + D-1-k) * fc mod R) / R),   m = 0, 1, ...
 *
 * A block of M samples yields exactly M / D outputs.  The phase is integer arithmetic on the sample index, so it never drifts: the carrier has
 * the period Pd = R / gcd(fc, R) samples (57 kHz: 100, 80, 64 at 300 k, 240 k, 192 k; 19 kHz: 300, 240, 192) and the carried phase is the sample
 * count mod Pd.  The factor 2 makes a real tone A cos(2 pi fc t + phi) read A e^(i phi).  Output m belongs to the input instant
 * mD + D-1 - (T-1)/2: the filter's group delay of (T-1)/2 samples.  The output rate is R / D complex values per second.
 *
 * Taps.  fmd_subc_design (no device): a Blackman-windowed sinc, computed in double and rounded once to float,
 *   s[k] = sinc(2 bw (k - (T-1)/2) / R) * (0.42 - 0.5 cos(2 pi (k+1)/(T+1)) + 0.08 cos(4 pi (k+1)/(T+1))),  h = s / sum(s),  sinc(x) = sin(pi x) / (pi x);
 * bw is the half-width in Hz, the -6 dB point.  A caller may pass taps of their own to fmd_subc_create (bw is then not read beyond its range check).
 * The carrier table 2 exp(...), Pd complex values, is made by the host in double and rounded once to float.
 *
 * Supported range (FMD_E_ARG / FMD_E_UNSUPPORTED with a message otherwise): 0 < fc < R/2; 0 < bw < R/2; Pd <= 4096; T a multiple of 4 in 16 .. 256;
 * D in {4, 8, 16, 32}; block_samples a multiple of D and >= T (a block's history then never reaches past the block before it).
 *
 * Arithmetic.  float32: each sample is multiplied once by its table entry (one rounding per component), the T products with the taps are summed
 * with fused multiply-adds in the order k = 0 up to T-1, starting from zero.  Per component |z - exact| <= (T + 4) 2^-24 * 2 sum_k |h[k]| |v[..]| + 2^-149
 * (DESIGN.md section 5c).
 *
 * Buffers (device pointers, both 16-byte aligned):
 *   d_v  f32 [n_streams][n_blocks][M]          - exactly the layout of the `v` debug tap (fmd_debug_taps.v, M = block_len / 16): the tap's buffer
 *                                                is passed straight in
 *   d_z  f32 [n_streams][n_blocks][M / D][2]   - re, then im
 * Feeding it from the tap costs the debug build of the fused kernel (about 1 % slower) and the store of v, 4 bytes per 16 bytes of IQ.  The object
 * is independent of fmd_batch apart from the convenience constructor fmd_batch_subc_create (rate_in, M = block_len / 16, n_streams and device from the
 * batch): it takes an MPX from anywhere.
 *
 * Contract on the result.  z of a (stream, block) depends only on that stream's v so far, the taps and the configuration - not on n_streams, how
 * blocks are split into calls, the stream used or the grid.  Equal inputs give bit-equal z (no atomics, one fixed summation order per output); an
 * output whose history lies in the carried state is computed exactly as one whose history lies in the previous block of the same launch.
 *
 * Stream rule, as for the batch: hip_stream == NULL is the object's own stream; the launches of one object form ONE sequence (each reads the
 * state the one before wrote) and the library inserts an event wait when the stream changes between two launches; one thread at a time per object;
 * get_state / set_state / reset / sync / destroy wait for the most recent launch whatever stream it is on, which must therefore still exist.  A
 * launch on the object's own stream reads d_v there: order it behind the producer (fmd_batch_sync, or launch both on one stream).
 * Graph capture: nothing is allocated inside a stream capture - state and tables are made at create - and the state advances in place, so every
 * replay continues where the one before ended.  A launch whose stream differs from the previous launch's cannot be captured (FMD_E_STATE: call
 * fmd_subc_sync first).
 * The host form: H2D, kernel, D2H, one wait; v and z in host memory, same layouts. */
#define FMD_SUBC_MAX_TAPS 256
#define FMD_SUBC_MAX_PERIOD 4096
typedef struct fmd_subc_config { int32_t rate_in, fc, bw, n_taps, decim, block_samples; } fmd_subc_config;
typedef struct fmd_subc_state  { int32_t phase; int32_t reserved[3]; float hist[256]; } fmd_subc_state; /* sample count mod Pd; last n_taps samples, oldest first, at [0..n_taps) */
typedef struct fmd_subc fmd_subc;

int  fmd_subc_design(const fmd_subc_config *cfg, float *taps /* n_taps */);            /* no device */
/* taps == NULL: fmd_subc_design(cfg).  device < 0: current device. */
int  fmd_subc_create(fmd_subc **out, const fmd_subc_config *cfg, const float *taps, int n_streams, int device);
int  fmd_batch_subc_create(fmd_subc **out, const fmd_batch *b, int fc, int bw, int n_taps, int decim);
void fmd_subc_destroy(fmd_subc *s);
int  fmd_subc_out_per_block(const fmd_subc *s);                                        /* M / D */
int  fmd_subc_run_device(fmd_subc *s, const void *d_v, int n_blocks, void *d_z, void *hip_stream);
int  fmd_subc_run_host(fmd_subc *s, const float *v, int n_blocks, float *z);
int  fmd_subc_get_state(fmd_subc *s, int stream, fmd_subc_state *out);
int  fmd_subc_set_state(fmd_subc *s, int stream, const fmd_subc_state *in);           /* 0 <= phase < Pd */
int  fmd_subc_reset(fmd_subc *s);
int  fmd_subc_sync(fmd_subc *s);

/* RDS receiver: the 57 kHz baseband z of an fmd_subc at fc = 57000 (rate_z = rate_in / D, Bz = M / D complex values per block) to soft bits on
 * the device, and - without a device - bits to groups, PI, PTY and the PS name.  Feed-forward throughout: no loop on the device, no carrier
 * recovery (DESIGN.md section 5d has the derivations and limits; tests/rds_model.py is the definition in float64).
 *
 * Definition.  Per stream z[n] = all blocks since the last reset, zero before it; n the absolute sample index.  fb = 1187.5 bit/s, S = 2 rate_z / 2375
 * samples per bit (rational).  With Tg = n_taps real taps g:
 *   matched filter   y[n] = sum_{k<Tg} g[k] z[n-k]
 *   timing           Tm_b = sum_{n in block b} |y[n]|^2 w[n mod Pw],  w[i] = exp(-2 pi i ((i * 2375) mod 2 rate_z) / (2 rate_z)),  Pw = 2 rate_z / gcd(2375, 2 rate_z)
 *                    Ts_b = a Ts_{b-1} + Tm_b,  a = 1 - 1 / avg_blocks,  Ts = 0 at reset;  phi_b = -arg(Ts_b) / (2 pi) in [-1/2, 1/2)  (never unwrapped)
 *   ownership        bit k has the nominal instant k S; block b (first sample n0) emits the bits with n0 - L <= k S < n0 + Bz - L, k >= 0, in integers:
 *                    Hh = ceil(S / 2), L = Hh + 2, Hb = ceil(S); the total lookback of a block into y is Hy = L + Hb + Hh samples
 *   detection        s(k) = y interpolated linearly at (k + phi_b) S;  soft bit c_k = Re(s(k) conj(s(k-1))), both with the emitting block's phi_b;
 *                    c_k < 0 is data bit 1 (RDS is differentially encoded: this is the decoded data)
 * Taps.  fmd_rds_design (no device): the standard's biphase bit pulse p(t) = h(t + Td/4) - h(t - Td/4), h the inverse transform of cos(pi f Td / 4) on
 * |f| <= 2 / Td, Td = 1 / fb; g[k] = c p(((Tg-1)/2 - k) / rate_z) with c = 1 / sum p^2 over the taps (an ideal isolated bit reads 1 at its centre), in
 * double, rounded once.  A caller may pass taps of their own.
 *
 * Supported range (FMD_E_UNSUPPORTED otherwise): rate_z a multiple of 125 with 10 <= S <= 32; n_taps a multiple of 4 in 16 .. 64; block_z a multiple
 * of 4, >= n_taps and >= Hy; avg_blocks >= 1; max_blocks >= 1 (the largest n_blocks of one launch: everything is allocated at create).
 *
 * Buffers (device pointers, 16-byte aligned), for a launch of n_blocks <= max_blocks blocks:
 *   d_z     f32 [n_streams][n_blocks][Bz][2]    - the layout of fmd_subc_run_device's d_z
 *   d_soft  f32 [n_streams][n_blocks][fmd_rds_bits_per_block()]  - a slot's first `count` values are its bits' c_k, the rest zero
 *   d_lens  i32 [n_streams][n_blocks]           - bits in the slot (in the manner of the PCM lens)
 *   d_first i64 [n_streams][n_blocks] or NULL   - index k of the slot's first bit
 *   d_est   f32 [n_streams][n_blocks][4] or NULL - Re Ts_b, Im Ts_b, phi_b, sum over the block of |y|^2
 * The counts of a launch add up to the nominal count exactly, for any data: ownership is integer arithmetic.  Equal z gives bit-equal output for any
 * n_streams, split into calls, stream or captured graph (no atomics, fixed summation orders; three kernels and a state kernel on one stream).
 * Stream rule, graph capture and the host form: as for fmd_subc (fmd_rds_sync before capturing after a launch on another stream).
 * fmd_rds_last_y is for tests and diagnosis, not for a receiver's data path: it waits for the most recent launch and downloads the scratch it left -
 * y [n_streams][n_blocks][Bz][2] and Tm [n_streams][n_blocks][2] (either may be NULL); n_blocks must be that launch's (FMD_E_STATE otherwise).  It is no
 * part of the launch sequence, advances nothing, and unlike a launch it allocates: a host buffer per call, freed before it returns. */
#define FMD_RDS_MAX_TAPS 64
#define FMD_RDS_MAX_PERIOD 640
#define FMD_RDS_MAX_YHIST 68
typedef struct fmd_rds_config { int32_t rate_z, block_z, n_taps, avg_blocks, max_blocks; } fmd_rds_config;
/* phase: sample count mod Pw.  frac: (next bit's nominal instant - next block's first sample) x 2375, in [-2375 L, 2 rate_z - 2375 L).  bit: the next
 * bit's index.  zhist: the last n_taps z at [0, n_taps), yhist: the last Hy y at [0, Hy), oldest first.  All zero = the state after a reset. */
typedef struct fmd_rds_state { int32_t phase, frac; int64_t bit; float ts[2]; int32_t reserved[2]; float zhist[64][2]; float yhist[68][2]; } fmd_rds_state;
typedef struct fmd_rds fmd_rds;

int  fmd_rds_design(const fmd_rds_config *cfg, float *taps /* n_taps */);              /* no device */
/* taps == NULL: fmd_rds_design(cfg).  device < 0: current device. */
int  fmd_rds_create(fmd_rds **out, const fmd_rds_config *cfg, const float *taps, int n_streams, int device);
/* rate_z = rate_in / decim, block_z = block_samples / decim, n_streams and device from the subcarrier object */
int  fmd_subc_rds_create(fmd_rds **out, const fmd_subc *s, int n_taps, int avg_blocks, int max_blocks);
void fmd_rds_destroy(fmd_rds *r);
int  fmd_rds_bits_per_block(const fmd_rds *r);                                         /* floats per slot of d_soft: the largest count, rounded up to a multiple of 4 */
int  fmd_rds_run_device(fmd_rds *r, const void *d_z, int n_blocks, void *d_soft, void *d_lens, void *d_first, void *d_est, void *hip_stream);
int  fmd_rds_run_host(fmd_rds *r, const float *z, int n_blocks, float *soft, int32_t *lens, int64_t *first, float *est);
int  fmd_rds_last_y(fmd_rds *r, int n_blocks, float *y, float *tm);
int  fmd_rds_get_state(fmd_rds *r, int stream, fmd_rds_state *out);
int  fmd_rds_set_state(fmd_rds *r, int stream, const fmd_rds_state *in);
int  fmd_rds_reset(fmd_rds *r);
int  fmd_rds_sync(fmd_rds *r);

/* RDS decoder (csrc/fmd_rds.c: no device, no allocation - the structs are the caller's).  _push takes soft bits in any split (c < 0 is bit 1), keeps
 * a 26-bit register, takes the remainder mod g(x) = x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1 and compares it with the offset words A, B, C, C', D.
 * Acquisition: two blocks with valid remainders 26 bits apart in cyclic order.  In sync a block is ok when its remainder is its position's offset
 * word (C' only in a version-B group); FMD_RDS_SYNC_LOSS consecutive bad blocks drop the sync.  Errors are detected, never corrected.  A group comes
 * out after its block D, when at least one of its blocks was ok: blk[i] = the 16 information bits, ok_mask bit i = block i ok, version 0 = A, 1 = B
 * (from block B), 255 = unknown.  Returns the groups written; stops early when max_out are written (dec->consumed = soft bits taken: max_out >=
 * n / 104 + 1 never stops early).  A call stops BEFORE any bit that could complete a group it has no room for: in sync that is a group's last bit, out of
 * sync every bit (an acquisition at position D emits at once).  So with max_out == 0, or once the array is full, an unsynced decoder takes no bit at
 * all (consumed stays where it was, 0 for max_out == 0): there is no way to advance the decoder while discarding its groups - pass room for them. */
#define FMD_RDS_SYNC_LOSS 6
typedef struct fmd_rds_group { uint16_t blk[4]; uint8_t ok_mask; uint8_t version; } fmd_rds_group;
typedef struct fmd_rds_decoder {
  uint32_t reg;                 /* the last 26 bits, newest in bit 0 */
  int32_t fill;                 /* bits in reg, up to 26 */
  int32_t synced, pos, cnt;     /* in sync: position 0..3 of the block being received, bits of it so far */
  int32_t bad_run;
  int32_t hidx;                 /* acquisition: slot of the next bit in hpos / hword; steps 0..25 while out of sync, rests while in sync (the history is cleared at acquisition) */
  int8_t hpos[26];              /* ... the position (0..3) whose offset word the register held at each of the last 26 bits, -1: none */
  uint8_t ok_mask, reserved;
  uint16_t hword[26];           /* ... and its 16 information bits */
  uint16_t blk[4];
  int32_t consumed;
  uint32_t n_sync, n_loss;      /* acquisitions and sync losses so far */
  uint64_t bits;                /* bits pushed so far */
} fmd_rds_decoder;
/* PI, PTY and the PS name from group types 0A and 0B, from blocks marked ok only.  ps: 8 characters and a NUL, '\0' where no segment came yet;
 * ps_mask bit i = segment i (characters 2i, 2i+1) received. */
typedef struct fmd_rds_info { int32_t have_pi; uint16_t pi; uint8_t pty, ps_mask; char ps[9]; uint8_t reserved[3]; } fmd_rds_info;
void fmd_rds_decoder_init(fmd_rds_decoder *dec);
int  fmd_rds_decoder_push(fmd_rds_decoder *dec, const float *soft, int n, fmd_rds_group *groups_out, int max_out);
void fmd_rds_info_init(fmd_rds_info *info);
int  fmd_rds_info_update(fmd_rds_info *info, const fmd_rds_group *g);                  /* 1: something changed */

/* Channel tuner: a digital down-converter on the device.  It moves any station inside a capture to where the chain looks (-fs/4, or 0 with
 * offset_tuning), band-limits it and hands it back as u8 IQ in the layout fmd_batch_run_device takes - so one capture feeds K streams of one batch,
 * K stations, each with audio, level, pilot and RDS, without a hardware retune (tests/tuner_model.py is the definition in
 * float64 and float32).
 *
 * Sources and channels.  A tuner has n_sources capture streams and n_channels output channels; channel c has {source, shift, gain}, settable
 * between launches (fmd_tuner_set_channel).  fs = rate is the capture rate (8 x rate_in of the batch it feeds), P = rate / step_hz the length of the
 * one shared carrier table, L = block_len / 2 the complex samples of a block.
 *
 * Definition.  For one source, n = the sample count since the last reset; samples before the reset are zero (the value, not the byte):
 *   input      x[n] = ((I - 127.5) + j (Q - 127.5)) / 128            (the reference's u8_f32_table[0], the spectrum's definition; exact in float32)
 *   mix        m[n] = x[n] c[((n mod P) shift) mod P],  c[p] = exp(+2 pi i p / P): a shift of k steps moves the spectrum by +k step_hz.  The index is
 *              integer arithmetic and never drifts.  The table is made by the host in double from the first octant by symmetry and rounded once; at
 *              the quarter periods its entries are exactly 1, i, -1, -i.  Per component one rounded product, then one fused multiply-add:
 *              re = fma(xr, cr, -(xi ci)),  im = fma(xr, ci, xi cr)
 *   filter     y[n] = sum_{k<T} h[k] m[n-k], real taps, at the full rate (no decimation: the batch takes 8 x rate_in); fused multiply-adds in the
 *              order k = 0 .. T-1 from zero, ONE order for every output wherever its history lies.  Output n belongs to the input instant n - (T-1)/2.
 *   quantiser  G = float(128 gain); per component code = clamp(rint(fma(G, y, 127.5f)), 0, 255), ties to even; bytes I, Q interleaved.
 * Taps.  fmd_tuner_design (no device): the Blackman-windowed sinc of fmd_subc_design with R = rate - -6 dB at bw, unit DC gain, in double, rounded
 * once.  A caller may pass taps of their own to fmd_tuner_create (bw is then not read beyond its range check).
 * fmd_tuner_shift (no device): the steps that bring a station at offset_hz from the capture's centre to where the chain looks: -offset_hz with
 * offset_tuning, -rate/4 - offset_hz without, in units of step_hz (|offset_hz| <= rate/2, so -P < shift < P); FMD_E_ARG when that is not on the grid.
 *
 * Supported range (FMD_E_ARG / FMD_E_UNSUPPORTED with a message otherwise): step_hz divides rate; P a multiple of 4 in 4 .. 4096; T a multiple of 4 in
 * 16 .. 64; 0 < bw < rate/2; block_len a multiple of 16, >= 64, with L >= T; -P < shift < P; gain finite with 0 < gain <= 64; source in range; d_out
 * does not overlap d_iq; both 16-byte aligned.
 *
 * State is per SOURCE, not per channel: {count mod P, the last T raw IQ byte pairs}.  The history is raw bytes and the mix is recomputed from the
 * absolute index, so a channel's shift, gain or source can change between any two launches with no transient other than the filter's own.  valid = 0
 * (the state after a reset) says that hist holds nothing: what lies before the first sample is the VALUE zero, which no byte pair encodes; every
 * launch leaves valid = 1.  The main kernel only reads the state; a small state kernel behind it on the same stream advances it, so no workgroup
 * waits for another and a captured graph advances the state on every replay.
 *
 * Buffers (device pointers, 16-byte aligned):
 *   d_iq   u8  [n_sources][n_blocks][block_len]
 *   d_out  u8  [n_channels][n_blocks][block_len]    - passed straight to fmd_batch_run_device of a batch with n_channels streams
 *   d_y    f32 [n_channels][n_blocks][L][2] or NULL - the value before the quantiser, for tests and diagnosis (as fmd_rds_last_y is)
 * Channels start as {source 0, shift 0, gain 1}.  fmd_tuner_set_channel waits for the most recent launch and is refused while that launch's stream is
 * being captured (FMD_E_STATE): the channel table a captured launch reads is the one at replay.
 *
 * Contract on the result.  The bytes of a (channel, block) depend only on that source's bytes so far, the taps and the channel's parameters - not on
 * n_channels, n_sources, how blocks are split into calls, the stream, or a graph.  Equal inputs give equal bytes (no atomics).
 * Accuracy.  Per component |y - y_exact| <= (T + 6) 2^-24 sum_k |h[k]| (|xr| + |xi|)[n-k] + 2^-149.
 * Caveat.  u8 has no code for zero: 127.5 is a tie.  A channel with nothing in its passband comes out as codes 127 / 128, decided by rounding
 * noise; that is what the quiet-input path of the fused kernel already handles, and no defect.
 * Stream rule, event hand-over on a change of stream, graph capture and the host form: as for fmd_subc (fmd_tuner_sync before capturing after a
 * launch on another stream).  Nothing is allocated in a launch.
 * fmd_batch_tuner_create takes rate = 8 rate_in, block_len, n_channels = n_streams and the device from the batch. */
#define FMD_TUNER_MAX_TAPS 64
#define FMD_TUNER_MAX_PERIOD 4096
typedef struct fmd_tuner_config  { int32_t rate, step_hz, bw, n_taps, block_len, reserved; } fmd_tuner_config;
typedef struct fmd_tuner_channel { int32_t source, shift; float gain; int32_t reserved; } fmd_tuner_channel;
/* count: sample count mod P.  valid: 0 after a reset (no history: zero values), else 1.  hist: the last n_taps byte pairs, oldest first, at [0, n_taps). */
typedef struct fmd_tuner_state   { int32_t count; int32_t valid; int32_t reserved[2]; uint8_t hist[64][2]; } fmd_tuner_state;
typedef struct fmd_tuner fmd_tuner;

int  fmd_tuner_design(const fmd_tuner_config *cfg, float *taps /* n_taps */);          /* no device */
int  fmd_tuner_shift(const fmd_tuner_config *cfg, int offset_hz, int offset_tuning, int32_t *shift);   /* no device */
/* taps == NULL: fmd_tuner_design(cfg).  device < 0: current device. */
int  fmd_tuner_create(fmd_tuner **out, const fmd_tuner_config *cfg, const float *taps, int n_sources, int n_channels, int device);
int  fmd_batch_tuner_create(fmd_tuner **out, const fmd_batch *b, int step_hz, int bw, int n_taps, int n_sources);
void fmd_tuner_destroy(fmd_tuner *t);
int  fmd_tuner_set_channel(fmd_tuner *t, int channel, const fmd_tuner_channel *ch);
int  fmd_tuner_get_channel(fmd_tuner *t, int channel, fmd_tuner_channel *ch);
int  fmd_tuner_run_device(fmd_tuner *t, const void *d_iq, int n_blocks, void *d_out, void *d_y, void *hip_stream);
int  fmd_tuner_run_host(fmd_tuner *t, const uint8_t *iq, int n_blocks, uint8_t *out);
int  fmd_tuner_get_state(fmd_tuner *t, int source, fmd_tuner_state *out);
int  fmd_tuner_set_state(fmd_tuner *t, int source, const fmd_tuner_state *in);         /* 0 <= count < P; valid 0 or 1 */
int  fmd_tuner_reset(fmd_tuner *t);
int  fmd_tuner_sync(fmd_tuner *t);

/* Station finder: power spectra to a ranked list of stations per stream, on the device - the step between fmd_batch_spectrum_device (what is in
 * the capture) and fmd_tuner_shift (bring it to where the chain listens).  DESIGN.md section 5f; tests/scan_model.py is the definition in float64.
 * The object is stateless: the result of a launch depends only on that launch's d_power and the configuration - not on n_streams, the stream, the
 * grid or a graph.  Every table is made at create, so a launch allocates nothing and can be captured.
 *
 * Definition.  N = n_bins, D = rate / N the width of a bin.  The signed bin of index k is s = k for k < N/2, else k - N; bin s covers
 * [(s - 1/2) D, (s + 1/2) D).  P[b][k] is the input, one spectrum per block in natural FFT order.
 *   1 average     A[k] = (sum_b double(P[b][k])) / n_blocks: the sum in double from zero in the order b = 0, 1, ..., then ONE division.
 *   2 floor       the used bins are those with |s| >= dc_guard (dc_guard = 0: all), n_used = N - max(0, 2 dc_guard - 1).  F = the element of 0-based
 *                 rank floor(floor_permille (n_used - 1) / 1000) of the used A in ascending order: an element of A, no interpolation.  In all that
 *                 follows the guarded bins read F instead of A.
 *   3 candidates  cmax = floor(((rate - 2 bw) N - rate) / (2 N raster_hz)) in 64-bit integers; candidate i = c + cmax, c = -cmax .. cmax, is centred
 *                 on c raster_hz; C = 2 cmax + 1.  Every band then lies inside +-(rate/2 - D/2): bin -N/2 belongs to no channel.
 *   4 power       Pc[i] = sum_s w_i[s] A[s], w_i[s] = the overlap of bin s with [c raster_hz - bw, c raster_hz + bw] divided by D: 1 for interior
 *                 bins; each of the two edge weights is ONE double division of 64-bit integers, (2 (s0 + 1/2) rate - 2 N lo) / (2 rate) for the
 *                 first bin s0 and (2 N hi - 2 (s1 - 1/2) rate) / (2 rate) for the last bin s1 (made by the host without a device and rounded
 *                 nowhere else).  The sum runs over s = s0 .. s1 ascending, in double from zero, each term one rounded product w A (interior: A
 *                 itself) - one order, no floating-point atomics: equal input gives bit-equal output.  M[i] = sum_s (w A) (s D - c raster_hz), the
 *                 same way (s D - c raster_hz = (s rate - c raster_hz N) / N is exact).
 *   5 occupied    Fc = F nb, nb = double(2 bw N) / double(rate) the bins of a channel; i is occupied when Pc[i] > double(threshold) Fc.
 *   6 stations    non-maximum suppression over a window, not greedy: an occupied i is a station when no j != i with |i - j| <= min_sep beats it; j
 *                 beats i when Pc[j] > Pc[i], or Pc[j] == Pc[i] and j < i.  j need not be occupied or be a station itself.
 *   7 rank        stations by Pc descending, ties by lower i first; found = their number, written = min(found, max_stations); the slots of
 *                 d_stations beyond `written` are all-zero bytes.
 *   8 fields      offset_hz = c raster_hz (from the capture's centre: what fmd_tuner_shift takes), candidate = i, power = float(Pc),
 *                 snr = float(Pc / Fc) (IEEE: +inf where F = 0), centroid_hz = float(c raster_hz + M / Pc).
 * Every decision of steps 5 to 7 is taken on the doubles; every float is rounded once, at the store.  Inputs are assumed finite and >= 0; with
 * anything else the values are unspecified, but the launch terminates and writes only inside its buffers.
 *
 * Supported range (FMD_E_ARG / FMD_E_UNSUPPORTED with a message otherwise, before a device is looked for): rate > 0; n_bins a power of two in
 * 64 .. 4096; raster_hz > 0; bw > 0 with rate / n_bins <= 2 bw; cmax >= 0; C <= 1024; 1 <= min_sep <= C; 0 <= floor_permille <= 1000;
 * 0 <= dc_guard <= n_bins / 4; 1 <= max_stations <= 64; threshold finite and > 0; reserved zero; n_blocks >= 1.
 *
 * Buffers (device pointers, 16-byte aligned):
 *   d_power    f32 [n_streams][n_blocks][n_bins], natural FFT order - the layout fmd_batch_spectrum_device writes; it may come from anywhere
 *   d_stations fmd_scan_station [n_streams][max_stations]
 *   d_counts   i32 [n_streams][2] = {found, written}
 *   d_chan     f32 [n_streams][C] or NULL: float(Pc) of every candidate, for tests and diagnosis
 * Stream rule and the host form: as for fmd_subc (hip_stream NULL: the object's own stream).  There is no state, so a change of stream needs no
 * hand-over; fmd_scan_sync and fmd_scan_destroy wait for the most recent launch.  For the tuner raster_hz must be a multiple of its step_hz.
 * fmd_batch_scan_create takes rate = 8 rate_in, n_streams and the device from the batch; min_sep 1, floor_permille 250, dc_guard 0, threshold 4. */
#define FMD_SCAN_MAX_BINS 4096
#define FMD_SCAN_MAX_CANDIDATES 1024
#define FMD_SCAN_MAX_STATIONS 64
typedef struct fmd_scan_config  { int32_t rate, n_bins, raster_hz, bw, min_sep, floor_permille, dc_guard, max_stations; float threshold; int32_t reserved[3]; } fmd_scan_config;   /* 48 bytes */
typedef struct fmd_scan_station { int32_t offset_hz, candidate; float power, snr, centroid_hz; int32_t reserved[3]; } fmd_scan_station;                                          /* 32 bytes */
typedef struct fmd_scan fmd_scan;

int  fmd_scan_candidates(const fmd_scan_config *cfg);     /* no device: C = 2 cmax + 1, or a negative status */
int  fmd_scan_create(fmd_scan **out, const fmd_scan_config *cfg, int n_streams, int device);
int  fmd_batch_scan_create(fmd_scan **out, const fmd_batch *b, int n_bins, int raster_hz, int bw, int max_stations);  /* rate = 8 rate_in, n_streams, device from the batch; min_sep 1, floor_permille 250, dc_guard 0, threshold 4 */
void fmd_scan_destroy(fmd_scan *s);
int  fmd_scan_run_device(fmd_scan *s, const void *d_power, int n_blocks, void *d_stations, void *d_counts, void *d_chan, void *hip_stream);
int  fmd_scan_run_host(fmd_scan *s, const float *power, int n_blocks, fmd_scan_station *stations, int32_t *counts, float *chan);
int  fmd_scan_sync(fmd_scan *s);

/* Stereo control: the pilot indicator, a blend of the stereo PCM towards mono, and audio meters (tests/stereo_model.py is
 * this definition in numpy, operation for operation).  The chain decodes stereo whether or not a 19 kHz pilot exists (the reference's
 * lp_real_f32 mode 2): on a mono or weak station L-R is demodulated noise.  This object measures the pilot an fmd_subc at 19 kHz delivers, decides
 * per block and stream, and rewrites the PCM of fmd_batch_run_device (mode 2) with a separation g in [0, 1]: g = 1 is the input, g = 0 is mono.
 *
 * Definition.  Every float operation is ONE float32 operation with one rounding (no contraction, no fast-math; `/` correctly rounded); fma is
 * the fused multiply-add.  The host, without a device: thr_on = float(double(pilot_on)^2), thr_off likewise, inv_mz = float(1.0 / Mz) (0 at
 * Mz = 0), inv_span = float(1.0 / (double(blend_hi) - blend_lo)).  Mz = pilot_per_block.  Per launch, three kernels on one stream:
 *   1 pilot meter  per (stream, block), 256 threads: thread t takes z[t], z[t + 256], ... in that order, p = fma(zi, zi, zr * zr), acc = acc + p
 *                  from zero; then a[t] = a[t] + a[t + h] for h = 128, 64 .. 1; pilot_ms = a[0] * inv_mz: the mean of |z|^2, the squared pilot
 *                  amplitude in the units of v (the square root is the caller's).  Without d_z (or at Mz = 0) pilot_ms reads 0.
 *   2 tracker      per stream, the blocks in order; it alone reads and writes fmd_stereo_state {g, stereo, run} (all zero after create and reset:
 *                  mono).  For each block: frames = min(max(lens, 0), pcm_stride) / 2 and g0 = g.  If frames > 0, the mode is FMD_STEREO_AUTO
 *                  and d_z is given: want = stereo ? (pilot_ms >= thr_off) : (pilot_ms >= thr_on) (a NaN compares false); if want != stereo then
 *                  run += 1 and at run >= hold_blocks stereo = want, run = 0; otherwise run = 0.  If frames > 0: target = 0 in
 *                  FMD_STEREO_FORCE_MONO, 1 in FMD_STEREO_FORCE_STEREO; in AUTO 0 when not stereo, 1 when stereo and d_quality is NULL, else with
 *                  x = d_quality's value t = (x - blend_lo) * inv_span and target = t > 0 ? min(t, 1) : 0 (a NaN quality reads 0);
 *                  d = min(max(target - g, -slew), slew), g = min(max(g + d, 0), 1).  g_step = frames > 0 ? (g - g0) / float(frames) : 0.
 *                  The record: {pilot_ms, g_start = g0, g_step, g_end = g, stereo, frames}.  A closed block (lens <= 0: squelched) holds everything.
 *   3 apply        per (stream, block), 256 threads, 16-byte words.  Frame i < frames: gi = min(max(fma(float(i + 1), g_step, g_start), 0), 1),
 *                  m = 0.5f (L + R), s = 0.5f (L - R) (both exact), Lo = rint(fma(gi, s, m)), Ro = rint(fma(-gi, s, m)), ties to even, clamped
 *                  to int16.  The slot's values from 2 frames on are copied unchanged.  So g = 1 returns the input bit for bit, g = 0 gives
 *                  Lo == Ro == rint((L + R) / 2), the output lies between m and the input (the blend never clips), and the ramp runs from the
 *                  block before's g to this block's: a change of separation never steps at a block edge.
 *   meters         over the OUTPUT frames, integers only (exact in any order): peak |Lo| and |Ro|, full_scale = the count of output values equal
 *                  to -32768 or 32767 (the chain's own clipping shows there), frames, and the sums of squares as uint64.
 * No floating-point atomics; nothing depends on the grid, on n_streams or on how blocks are split into calls.
 *
 * Timing.  z lags its block by the subcarrier filter's group delay and the PCM by the chain's; both are far below a block, the granularity of
 * the decision.
 *
 * Supported range (FMD_E_UNSUPPORTED / FMD_E_ARG with a message otherwise, before a device is looked for): pcm_stride a multiple of 8 in
 * 8 .. 65536; pilot_per_block in 0 .. 65536; hold_blocks in 1 .. 2^20; 0 < pilot_off <= pilot_on, finite; blend_lo < blend_hi, finite;
 * 0 < slew <= 1; reserved fields zero.
 *
 * Buffers (device pointers, 16-byte aligned):
 *   d_pcm      s16 [n_streams][n_blocks][pcm_stride] - exactly what fmd_batch_run_device wrote in mode 2: L, R interleaved
 *   d_out      s16, same layout; may be d_pcm itself (in place), any other overlap is FMD_E_ARG
 *   d_lens     i32 [n_streams][n_blocks]
 *   d_z        f32 [n_streams][n_blocks][Mz][2] - the d_z of fmd_subc_run_device; may be NULL (FMD_E_ARG in FMD_STEREO_AUTO, as is Mz = 0)
 *   d_quality  f32 [n_streams][n_blocks] or NULL - for instance the d_levels of fmd_batch_run_device_levels
 *   d_info     fmd_stereo_info [n_streams][n_blocks], required
 *   d_meter    fmd_stereo_meter [n_streams][n_blocks] or NULL
 * The mode (fmd_stereo_set_mode; FMD_STEREO_AUTO after create) is a launch argument: a captured launch keeps the mode it was captured with.
 * Stream rule, graph capture and the host form: as for fmd_subc - everything is made at create, a launch allocates nothing, the state advances
 * on every replay, a change of stream is handed over with an event and refused inside a capture (FMD_E_STATE: call fmd_stereo_sync first).
 * fmd_batch_stereo_create takes pcm_stride, n_streams and the device from the batch (which must be mode 2) and pilot_per_block from `pilot`, an
 * fmd_subc at 19 kHz (NULL: pilot_per_block 0, forced modes only); the other fields from cfg. */
#define FMD_STEREO_AUTO 0
#define FMD_STEREO_FORCE_MONO 1
#define FMD_STEREO_FORCE_STEREO 2
typedef struct fmd_stereo_config { int32_t pcm_stride, pilot_per_block, hold_blocks, reserved0;
                                   float pilot_on, pilot_off, blend_lo, blend_hi, slew; int32_t reserved[3]; } fmd_stereo_config;   /* 48 bytes */
typedef struct fmd_stereo_state  { float g; int32_t stereo, run, reserved; } fmd_stereo_state;                                      /* 16 bytes */
typedef struct fmd_stereo_info   { float pilot_ms, g_start, g_step, g_end; int32_t stereo, frames, reserved[2]; } fmd_stereo_info;  /* 32 bytes */
typedef struct fmd_stereo_meter  { int32_t peak_l, peak_r, full_scale, frames; uint64_t sumsq_l, sumsq_r; } fmd_stereo_meter;       /* 32 bytes */
typedef struct fmd_stereo fmd_stereo;

int  fmd_stereo_create(fmd_stereo **out, const fmd_stereo_config *cfg, int n_streams, int device);
int  fmd_batch_stereo_create(fmd_stereo **out, const fmd_batch *b, const fmd_subc *pilot, const fmd_stereo_config *cfg);
void fmd_stereo_destroy(fmd_stereo *s);
int  fmd_stereo_set_mode(fmd_stereo *s, int mode);
int  fmd_stereo_run_device(fmd_stereo *s, const void *d_pcm, const void *d_lens, const void *d_z, const void *d_quality,
                           int n_blocks, void *d_out, void *d_info, void *d_meter, void *hip_stream);
int  fmd_stereo_run_host(fmd_stereo *s, const int16_t *pcm, const int32_t *lens, const float *z, const float *quality,
                         int n_blocks, int16_t *out, fmd_stereo_info *info, fmd_stereo_meter *meter);
int  fmd_stereo_get_state(fmd_stereo *s, int stream, fmd_stereo_state *out);
int  fmd_stereo_set_state(fmd_stereo *s, int stream, const fmd_stereo_state *in);     /* g finite in 0 .. 1, stereo 0 or 1, 0 <= run < hold_blocks, reserved 0 */
int  fmd_stereo_reset(fmd_stereo *s);
int  fmd_stereo_sync(fmd_stereo *s);

/* Duration of the most recent fmd_batch_run_device kernel, measured with HIP
 * events recorded on the stream the kernel was launched on (synchronises).  The fused kernel alone: the finish kernel of a levels or
 * squelch launch is not included. */
int fmd_batch_last_kernel_ms(fmd_batch *b, float *ms);
/* Every launch is bracketed by an event pair for fmd_batch_last_kernel_ms; a caller that
 * launches back to back and times the whole run itself can turn that off (on = 0): the two
 * event records cost about 10 us of GPU time per launch. */
int fmd_batch_set_timing(fmd_batch *b, int on);
/* Name of the dominant kernel (as rocprofv3 reports it) for this batch. */
const char *fmd_batch_kernel_name(const fmd_batch *b);

const char *fmd_last_error(void);
int fmd_device_count(void);

/* ------------------------------------------------------------------------
 * 3. Ingest: rtlsdr_read_async callback -> pinned staging ring -> batch
 * ------------------------------------------------------------------------
 * fmd_ingest_callback has the exact rtlsdr_read_async_cb_t signature
 * (reference include/rtl-sdr.h:340) and the contract of rtlsdr_callback
 * (src/rtl_fm_player.c:790-837): it copies `len` bytes before returning and
 * never blocks on the GPU.  ctx is an fmd_ingest* bound to one stream of a batch.
 * The ring is pinned memory and is itself the source of the H2D copies.
 *
 * Overflow.  DEFAULT IS NOT THE REFERENCE'S: FMD_OVERFLOW_DROP_OLDEST splits a copy at the end
 * of the ring and, when the ring is full, advances the read position over the oldest bytes (a clean
 * loss, counted).  The reference instead restarts a transfer that does not fit before the end of
 * the ring at offset 0 and, on overflow, clamps its byte count without moving the read position, so
 * the demod thread then reads new data where old was expected (src/rtl_fm_player.c:813-834).
 * FMD_OVERFLOW_REFERENCE reproduces exactly that, for callers that want identical behaviour. */
#define FMD_OVERFLOW_DROP_OLDEST 0
#define FMD_OVERFLOW_REFERENCE 1
typedef struct fmd_ingest fmd_ingest;
typedef void (*fmd_read_async_cb_t)(unsigned char *buf, uint32_t len, void *ctx);

/* ring_bytes 0: the reference's 4 MiB (16 blocks).  b == NULL makes an unbound ring in ordinary
 * host memory (no device needed; `stream` ignored) that its owner drains with fmd_ingest_pop. */
int fmd_ingest_create(fmd_ingest **out, fmd_batch *b, int stream, uint32_t ring_bytes);
void fmd_ingest_destroy(fmd_ingest *g);
int fmd_ingest_set_overflow(fmd_ingest *g, int mode);
void fmd_ingest_callback(unsigned char *buf, uint32_t len, void *ctx);
/* Bytes buffered that no job has taken yet / bytes dropped so far.  Thread-safe, like the callback
 * and fmd_ingest_mute: the callback may run on any thread (librtlsdr's event thread in the reference)
 * while another thread pumps. */
uint32_t fmd_ingest_buffered(const fmd_ingest *g);
uint64_t fmd_ingest_dropped(const fmd_ingest *g);
/* The dequeue of demod_thread_fn (src/rtl_fm_player.c:863-876): when at least len bytes are
 * buffered, copies them to out and returns len, else returns 0.  Not while pump jobs are in flight. */
uint32_t fmd_ingest_pop(fmd_ingest *g, uint8_t *out, uint32_t len);
/* Mute the first n bytes of the next callback buffer (retune, :805-810). */
void fmd_ingest_mute(fmd_ingest *g, int n_bytes);
/* Demodulate whole blocks that every bound stream has buffered: returns the
 * number of blocks processed per stream (>= 0) or an error.  pcm/lens as in
 * fmd_batch_run_host, for max_blocks blocks. */
int fmd_batch_pump(fmd_batch *b, int max_blocks, int16_t *pcm, int32_t *lens);
/* Pipelined form of the same: _begin queues the H2D of what is buffered (straight from the
 * pinned rings), the kernel and the D2H, and returns the job's block count at once (0: nothing
 * buffered); _end waits for the oldest job begun and hands out its PCM and lengths.
 * Two jobs may be in flight, so the H2D of one overlaps the kernel of the other (the demod
 * thread's copy / demodulate alternation, src/rtl_fm_player.c:871-889, without the
 * serialisation).  A job's bytes stay in the ring until their H2D has finished: size the ring
 * (fmd_ingest_create's ring_bytes) at twice the job when the producer must not wait. */
int fmd_batch_pump_begin(fmd_batch *b, int max_blocks);
int fmd_batch_pump_end(fmd_batch *b, int16_t *pcm, int32_t *lens);

/* ------------------------------------------------------------------------
 * 4. WAV output in the reference's format (InitWaveOut / CloseWaveOut,
 *    src/rtl_fm_player.c:1259-1328; headers include/rtl_fm_player.h:216-253)
 * ------------------------------------------------------------------------
 * 260-byte header (44-byte PCM header, 16 bit / 48000 Hz / mode == 2 ? stereo :
 * mono, then 216 zero bytes); close patches the sizes at offsets 4 and 40.
 * path "-" writes to stdout (sizes then stay at the reference's placeholders). */
#define FMD_WAV_HEADER_BYTES 260
typedef struct fmd_wav fmd_wav;
int fmd_wav_header(int mode, unsigned char out[FMD_WAV_HEADER_BYTES]);
int fmd_wav_open(fmd_wav **out, const char *path, int mode);
int fmd_wav_write(fmd_wav *w, const int16_t *pcm, size_t n_values);
int fmd_wav_close(fmd_wav *w);

#ifdef __cplusplus
}
#endif
#endif /* FMDEMOD_MI355X_H */
