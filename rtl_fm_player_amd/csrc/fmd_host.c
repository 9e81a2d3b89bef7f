/*
 * fmd_host.c - the batch of libfmdemod_mi355x.so's C host layer, and what reaches into it.
 *
 * Plain C above the HIP runtime's C API.  Here: the batch object (fmd_batch_*: device buffers, carried state, launches, host forms, channel levels
 * and squelch), the capture spectrum of its input, the constructors that make a receiver object from its configuration, the reference-shaped entry
 * points (same names and struct layout as rtl_fm_player.c; one single-stream batch each), and the memory of the ingest rings with the pump that
 * drains them into a batch.
 * Elsewhere: what needs no device - configuration checks, filter design, the kernel family and its arguments - is fmd_resolve.c for the fused chain
 * and fmd_recv.c / fmd_rds.c for the receivers, with the error text in fmd_error.c; the ring and its accounting are fmd_ring.c; the device plumbing
 * shared with the receiver objects is fmd_dev.c, those objects (subcarrier, tuner, scan, RDS) are fmd_objects.c.  All arithmetic of the hot path
 * runs in the kernels of fmd_kernels.inc (built as fmd_kernels_{exact,fast,mfma}.hip), the receivers' in fmd_kernels_recv.hip; nothing here computes
 * a sample.
 */
#define _GNU_SOURCE
#include <math.h>
#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fmd_dev.h"
#include "fmd_ring.h"

/* ---- layout of the reference structs ---- */
_Static_assert(offsetof(struct demod_state, buf) == 16, "demod_state.buf");
_Static_assert(offsetof(struct demod_state, buf_len) == 262160, "demod_state.buf_len");
_Static_assert(offsetof(struct demod_state, lowpassed) == 262164, "demod_state.lowpassed");
_Static_assert(offsetof(struct demod_state, lp_len) == 1310740, "demod_state.lp_len");
_Static_assert(offsetof(struct demod_state, lowpass_tb) == 1310744, "demod_state.lowpass_tb");
_Static_assert(offsetof(struct demod_state, result) == 1311176, "demod_state.result");
_Static_assert(offsetof(struct demod_state, result_len) == 1835464, "demod_state.result_len");
_Static_assert(offsetof(struct demod_state, rate_in) == 1835508, "demod_state.rate_in");
_Static_assert(offsetof(struct demod_state, rate_out) == 1835512, "demod_state.rate_out");
_Static_assert(offsetof(struct demod_state, rate_out2) == 1835516, "demod_state.rate_out2");
_Static_assert(offsetof(struct demod_state, pre_r_f32) == 1835536, "demod_state.pre_r_f32");
_Static_assert(offsetof(struct demod_state, deemph) == 1835592, "demod_state.deemph");
_Static_assert(offsetof(struct demod_state, deemph_l_f32) == 1835612, "demod_state.deemph_l_f32");
_Static_assert(offsetof(struct demod_state, deemph_lambda) == 1835620, "demod_state.deemph_lambda");
_Static_assert(offsetof(struct demod_state, volume) == 1835624, "demod_state.volume");
_Static_assert(offsetof(struct demod_state, prev_lpr_index) == 1835632, "demod_state.prev_lpr_index");
_Static_assert(offsetof(struct demod_state, lpr) == 1835640, "demod_state.lpr");
_Static_assert(offsetof(struct demod_state, rw) == 1835720, "demod_state.rw");
_Static_assert(offsetof(struct demod_state, ready) == 1835776, "demod_state.ready");
_Static_assert(offsetof(struct demod_state, ready_m) == 1835824, "demod_state.ready_m");
_Static_assert(offsetof(struct demod_state, output_target) == 1835864, "demod_state.output_target");
_Static_assert(sizeof(struct demod_state) == 1835872, "sizeof(struct demod_state)");
_Static_assert(sizeof(struct lp_real) == 80, "sizeof(struct lp_real)");
_Static_assert(offsetof(struct lp_real, swf) == 48, "lp_real.swf");
_Static_assert(offsetof(struct lp_real, pos) == 60, "lp_real.pos");
_Static_assert(offsetof(struct lp_real, mode) == 72, "lp_real.mode");

int fmd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

/* The library reads ONE environment variable, FMD_MATH_FAST, and only for the reference-shaped surface whose signatures have no room for the
 * choice (dropin_read_env).  The batch API's kernel family is fmd_config.math and nothing else. */

/* ---- batch object --------------------------------------------------------- */

#define FMD_SP_TABLES 8        /* (n_bins, window) pairs a batch keeps tables for: three sizes x two windows today */

struct fmd_batch {
  fmdk_resolved r;              /* configuration, taps, kernel arguments and instantiation as fmdk_resolve made them; fmd_batch_create adds kp.dec_tables */
  int n_streams;
  struct fmdh_obj o;           /* device, own stream and launch order; o.d_state: the current fmd_stream_state[n_streams]; o.also: the pump's copy stream */
  void *d_state_out;           /* ... and its ping-pong partner: a multi-chunk launch reads one and writes the other, then they swap */
  hipEvent_t ev0, ev1;
  int no_timing;               /* fmd_batch_set_timing(b, 0): no event pair around the kernel */
  int timed;
  int n_cus;
  int time_split;              /* fmd_batch_set_time_split: 0 default, > 0 workers per CU to cut for, < 0 never split */
  /* staging for the host-buffer path, grown on demand */
  void *d_iq, *d_pcm, *d_lens;
  void *d_dec_tables;          /* FMD_MATH_FAST_MFMA_F: the phase tables of the decimating second stage (fmdk_dec_tables), NULL otherwise */
  size_t cap_blocks;
  /* ingest */
  struct fmd_ingest **ingest;  /* [n_streams], NULL when unbound */
  /* fmd_batch_pump_begin/_end: two jobs in flight, each with its own pinned and device buffers */
  struct pump_slot {
    int16_t *h_pcm; int32_t *h_lens;                   /* pinned */
    void *d_iq, *d_pcm, *d_lens;
    size_t cap_blocks;
    int n_blocks;                                      /* > 0: job in flight */
    int ring_held;                                     /* its bytes are still held in the rings (H2D source) */
    int failed;                                        /* hipError_t of a D2H enqueue that failed after the kernel was launched */
    hipEvent_t h2d_done, done;
  } pump[2];
  int pump_head, pump_tail;    /* next slot to begin / oldest slot not yet ended; on o.also the H2D of job k+1 runs beside the kernel of job k */
  /* channel levels and power squelch (fmd_batch_run_device_levels, fmd_batch_set_squelch; csrc/levels.inc) */
  void *d_lv_part;             /* the LV kernels' tile partials, float2 [n_streams][n_blocks][tiles per block], grown on demand */
  size_t lv_part_cap;          /* ... its capacity in float2 */
  void *d_levels;              /* staging of fmd_batch_run_host_levels, f32 [n_streams][lv_cap_blocks] */
  size_t lv_cap_blocks;
  float *d_sq_thr;             /* [n_streams] thresholds, made by fmd_batch_set_squelch */
  int32_t *d_sq_hits;          /* [n_streams] rtl_fm's squelch_hits: beside the carried state, not inside fmd_stream_state */
  int sq_on, sq_conseq;
  /* capture spectrum (fmd_batch_spectrum_device / _host; csrc/spectrum.inc) */
  struct sp_table {
    int n_bins, window;
    float *d_tab;                /* window and pass twiddles (fmdk_spectrum_tables), made at the pair's first use */
    double sum_w2;
  } sp_tab[FMD_SP_TABLES];
  int sp_n_tab;
  void *d_sp_power;            /* staging of fmd_batch_spectrum_host, f32 [n_streams][n_blocks][n_bins] */
  size_t sp_power_cap;         /* ... its capacity in floats */
  hipStream_t sp_stream;       /* the caller's stream of the most recent spectrum launch (NULL: none, or the batch's own) */
};

int fmd_batch_create(fmd_batch **out, const fmd_config *cfg, const fmd_taps *taps, int n_streams, int device) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  int rc = fmdk_check_config(cfg);
  if (rc) return rc;
  if (n_streams <= 0) return fmd_fail(FMD_E_ARG, "n_streams must be positive");

  fmd_batch *b = (fmd_batch *)calloc(1, sizeof(*b));
  if (!b) return fmd_fail(FMD_E_NOMEM, "out of host memory");
  b->n_streams = n_streams;
  const size_t st_bytes = sizeof(fmd_stream_state) * (size_t)n_streams;
  if ((rc = fmdh_obj_open(&b->o, device, sizeof(fmd_stream_state), n_streams, 1)) || (rc = fmdk_resolve(cfg, taps, &b->r)) ||
      (rc = fmdh_obj_alloc(&b->o, &b->d_state_out, st_bytes, NULL, 0))) {
    fmd_batch_destroy(b);
    return rc;
  }
  hipError_t e;
  if ((e = hipEventCreate(&b->ev0)) != hipSuccess || (e = hipEventCreate(&b->ev1)) != hipSuccess ||
      (e = hipMemsetAsync(b->d_state_out, 0, st_bytes, b->o.ord.stream)) != hipSuccess || (e = hipStreamSynchronize(b->o.ord.stream)) != hipSuccess) {
    rc = fmd_fail(FMD_E_HIP, "device setup failed: %s", hipGetErrorString(e));
    fmd_batch_destroy(b);
    return rc;
  }
  if (b->r.cfg.math == FMD_MATH_FAST_MFMA_F && b->r.kp.dec_p > 0) {
    size_t nb = 0;
    uint8_t *t = fmdk_dec_tables(&b->r, &nb);
    if (!t) { fmd_batch_destroy(b); return fmd_fail(FMD_E_NOMEM, "out of host memory"); }
    rc = fmdh_obj_alloc(&b->o, &b->d_dec_tables, nb, t, nb);
    free(t);
    if (rc) { fmd_batch_destroy(b); return rc; }
    b->r.kp.dec_tables = b->d_dec_tables;
  }
  {
    hipDeviceProp_t prop;
    b->n_cus = (hipGetDeviceProperties(&prop, b->o.device) == hipSuccess && prop.multiProcessorCount > 0)
                   ? prop.multiProcessorCount : 256;
  }
  b->ingest = (struct fmd_ingest **)calloc((size_t)n_streams, sizeof(*b->ingest));
  if (!b->ingest) { fmd_batch_destroy(b); return fmd_fail(FMD_E_NOMEM, "out of host memory"); }
  *out = b;
  return FMD_OK;
}

void fmd_batch_destroy(fmd_batch *b) {
  if (!b) return;
  /* wait for everything this batch has queued: its own stream, the copy stream of the pump and the stream of the most recent launch when the caller supplied one */
  hipSetDevice(b->o.device);
  fmdh_order_quiesce(&b->o.ord, b->o.also);
  if (b->sp_stream && b->sp_stream != b->o.ord.stream) hipStreamSynchronize(b->sp_stream);   /* a spectrum launch may still read its table */
  for (int i = 0; i < b->sp_n_tab; i++)
    if (b->sp_tab[i].d_tab) hipFree(b->sp_tab[i].d_tab);
  /* rings outlive the batch (their owner destroys them with fmd_ingest_destroy, before or after this call): detach them so that neither side touches freed memory */
  if (b->ingest)
    for (int i = 0; i < b->n_streams; i++)
      if (b->ingest[i]) fmdk_ring_detach(b->ingest[i]);
  /* (the states and the decimator's tables are the core's: fmdh_obj_close) */
  void *const dev[] = {b->d_sp_power, b->d_lv_part, b->d_levels, b->d_sq_thr, b->d_sq_hits, b->d_iq, b->d_pcm,
                       b->d_lens, b->pump[0].d_iq, b->pump[0].d_pcm, b->pump[0].d_lens, b->pump[1].d_iq, b->pump[1].d_pcm, b->pump[1].d_lens};
  for (size_t i = 0; i < sizeof(dev) / sizeof(*dev); i++)
    if (dev[i]) hipFree(dev[i]);
  for (int i = 0; i < 2; i++) {
    struct pump_slot *p = &b->pump[i];
    if (p->h_pcm) hipHostFree(p->h_pcm);
    if (p->h_lens) hipHostFree(p->h_lens);
    if (p->h2d_done) hipEventDestroy(p->h2d_done);
    if (p->done) hipEventDestroy(p->done);
  }
  if (b->ev0) hipEventDestroy(b->ev0);
  if (b->ev1) hipEventDestroy(b->ev1);
  fmdh_obj_close(&b->o);
  free(b->ingest);
  free(b);
}

int fmd_batch_pcm_stride(const fmd_batch *b) { return b ? b->r.pcm_stride : FMD_E_ARG; }
int fmd_batch_n_streams(const fmd_batch *b) { return b ? b->n_streams : FMD_E_ARG; }
int fmd_batch_math(const fmd_batch *b) { return b ? b->r.cfg.math : FMD_E_ARG; }
int fmd_batch_set_time_split(fmd_batch *b, int workers_per_cu) {
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  b->time_split = workers_per_cu;
  return FMD_OK;
}
const char *fmd_batch_kernel_name(const fmd_batch *b) {
  return b ? "fmd_fused_kernel" : "";   /* every variant: rocprofv3 prints the name with its template arguments (prefix match) */
}

/* Every device run: the fused kernel, and - with a level buffer or while squelch is on - its LV build and the finish kernel (levels.inc) right
 * behind it on the same stream.  The timing events ride on the fused kernel alone. */
static int run_launch(fmd_batch *b, const void *d_iq, int n_blocks, void *d_pcm, void *d_lens, void *d_levels, void *hip_stream, const fmd_debug_taps *dbg) {
  if (!b || !d_iq || !d_pcm || !d_lens) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks < 0) return fmd_fail(FMD_E_ARG, "n_blocks < 0");
  if (n_blocks == 0) return FMD_OK;
  if (((uintptr_t)d_iq & 15) != 0) return fmd_fail(FMD_E_ARG, "d_iq must be 16-byte aligned");
  if ((long long)b->r.cfg.block_len * n_blocks >= (1LL << 32))   /* one raw buffer (32-bit size) per stream */
    return fmd_fail(FMD_E_ARG, "n_blocks too large: block_len * n_blocks must stay below 2^32 bytes per stream");
  HIP_TRY(hipSetDevice(b->o.device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->o.ord.stream;
  const fmdk_params kp = fmdk_launch_params(&b->r, b->n_streams, b->n_cus, b->time_split, n_blocks, dbg && (dbg->y || dbg->v || dbg->mpx || dbg->prof));
  /* The state is always ping-ponged (the kernel's in / out pointers never alias); order_handover orders a launch behind the previous one's output. */
  /* A caller's stream that is being captured into a hipGraph: the launch becomes a node of the graph.  The timing events have no meaning there (the launch
   * carries none and fmd_batch_last_kernel_ms says so afterwards), and the event hand-over between streams would record an event of the batch on a stream
   * outside the capture - which invalidates the capture: refused, with what to do instead. */
  const int capturing = fmdh_stream_is_capturing(st);
  int rc = fmdh_order_handover(&b->o.ord, st);
  if (rc > 0)
    return fmd_fail(FMD_E_STATE, "the batch's previous launch ran on another stream: call fmd_batch_sync() before capturing this one into a graph (an event "
                             "hand-over between streams cannot be recorded inside a capture)");
  if (rc) return rc;
  const int lv = d_levels || b->sq_on;
  if (lv) {
    if (b->sq_on && ((uintptr_t)d_pcm & 15) != 0) return fmd_fail(FMD_E_ARG, "d_pcm must be 16-byte aligned while squelch is on");
    const size_t m = (size_t)(b->r.cfg.block_len >> 4), tile = (size_t)fmdk_tile();
    const size_t need = (size_t)b->n_streams * (size_t)n_blocks * ((m + tile - 1) / tile);
    if (need > b->lv_part_cap) {
      if (capturing)
        return fmd_fail(FMD_E_STATE, "the level scratch of %d blocks per launch does not exist yet: run one launch of this size before the capture", n_blocks);
      HIP_TRY(fmdh_order_quiesce(&b->o.ord, b->o.also));   /* (the launch in flight may still read the old area) */
      const grow_buf v = {&b->d_lv_part, need * 2 * sizeof(float), 0};
      if ((rc = fmdh_grow(&b->lv_part_cap, need, &v, 1))) return rc;
    }
  }
  const int with_events = !b->no_timing && !capturing;
  /* the timing events ride on the kernel's dispatch packet (fmdk_launch): no packets of their own */
  void *const d_state_in = b->o.d_state;
  int e = fmdk_launch(&kp, &b->r.var, b->n_streams, d_iq, d_pcm, d_lens, d_state_in,
                      b->d_state_out, dbg, lv ? b->d_lv_part : NULL, st, with_events ? (void *)b->ev0 : NULL, with_events ? (void *)b->ev1 : NULL);
  if (e) return fmd_fail(FMD_E_HIP, "kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  b->o.d_state = b->d_state_out;
  b->d_state_out = d_state_in;
  fmdh_order_launched(&b->o.ord, st);
  b->timed = with_events;           /* (a captured launch has no events: fmd_batch_last_kernel_ms then reports FMD_E_STATE instead of a stale time) */
  if (lv) {
    e = fmdk_levels(b->d_lv_part, b->n_streams, n_blocks, b->r.cfg.block_len, b->r.pcm_stride, d_levels, d_lens, d_pcm,
                    b->sq_on ? b->d_sq_thr : NULL, b->d_sq_hits, b->sq_conseq, st);
    if (e) return fmd_fail(FMD_E_HIP, "level kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  }
  return FMD_OK;
}

int fmd_batch_run_device_debug(fmd_batch *b, const void *d_iq, int n_blocks, void *d_pcm, void *d_lens, void *hip_stream, const fmd_debug_taps *dbg) {
  return run_launch(b, d_iq, n_blocks, d_pcm, d_lens, NULL, hip_stream, dbg);
}

int fmd_batch_run_device(fmd_batch *b, const void *d_iq, int n_blocks, void *d_pcm, void *d_lens, void *hip_stream) {
  return run_launch(b, d_iq, n_blocks, d_pcm, d_lens, NULL, hip_stream, NULL);
}

int fmd_batch_run_device_levels(fmd_batch *b, const void *d_iq, int n_blocks, void *d_pcm, void *d_lens, void *d_levels, void *hip_stream, const fmd_debug_taps *dbg) {
  return run_launch(b, d_iq, n_blocks, d_pcm, d_lens, d_levels, hip_stream, dbg);
}

#define FMD_SQUELCH_CONSEQ_MAX (1 << 30)   /* (hits + 1 stays an int) */

/* every stream's hits = conseq + 1 (closed: the reference's initial squelch_hits 11 against conseq_squelch 10); the batch is quiescent */
static int squelch_close_all(fmd_batch *b) {
  int32_t *h = (int32_t *)malloc(sizeof(int32_t) * (size_t)b->n_streams);
  if (!h) return fmd_fail(FMD_E_NOMEM, "out of host memory");
  for (int i = 0; i < b->n_streams; i++) h[i] = b->sq_conseq + 1;
  const hipError_t e = hipMemcpy(b->d_sq_hits, h, sizeof(int32_t) * (size_t)b->n_streams, hipMemcpyHostToDevice);
  free(h);
  if (e != hipSuccess) return fmd_fail(FMD_E_HIP, "squelch: %s", hipGetErrorString(e));
  return FMD_OK;
}

int fmd_batch_set_squelch(fmd_batch *b, const float *thresholds, int conseq) {
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  if (conseq < 0 || conseq > FMD_SQUELCH_CONSEQ_MAX) return fmd_fail(FMD_E_ARG, "conseq must lie in 0 .. %d", FMD_SQUELCH_CONSEQ_MAX);
  if (thresholds)
    for (int i = 0; i < b->n_streams; i++)
      if (!isfinite(thresholds[i])) return fmd_fail(FMD_E_ARG, "threshold of stream %d is not finite", i);
  int rc = fmdh_obj_sync(&b->o);
  if (rc) return rc;
  if (!thresholds) {
    b->sq_on = 0;
    return FMD_OK;
  }
  if (!b->d_sq_thr) HIP_TRY(hipMalloc((void **)&b->d_sq_thr, sizeof(float) * (size_t)b->n_streams));
  if (!b->d_sq_hits) HIP_TRY(hipMalloc((void **)&b->d_sq_hits, sizeof(int32_t) * (size_t)b->n_streams));
  HIP_TRY(hipMemcpy(b->d_sq_thr, thresholds, sizeof(float) * (size_t)b->n_streams, hipMemcpyHostToDevice));
  b->sq_conseq = conseq;
  if ((rc = squelch_close_all(b))) return rc;
  b->sq_on = 1;
  return FMD_OK;
}

int fmd_batch_get_squelch_hits(fmd_batch *b, int stream, int32_t *hits) {
  if (!b || !hits || stream < 0 || stream >= b->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  if (!b->d_sq_hits) return fmd_fail(FMD_E_STATE, "squelch was never set on this batch (fmd_batch_set_squelch)");
  const int rc = fmdh_obj_sync(&b->o);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(hits, b->d_sq_hits + stream, sizeof(int32_t), hipMemcpyDeviceToHost));
  return FMD_OK;
}

int fmd_batch_set_squelch_hits(fmd_batch *b, int stream, int32_t hits) {
  if (!b || stream < 0 || stream >= b->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  if (!b->d_sq_hits) return fmd_fail(FMD_E_STATE, "squelch was never set on this batch (fmd_batch_set_squelch)");
  if (hits < 0 || hits > b->sq_conseq + 1) return fmd_fail(FMD_E_ARG, "hits must lie in 0 .. conseq + 1 = %d", b->sq_conseq + 1);
  const int rc = fmdh_obj_sync(&b->o);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(b->d_sq_hits + stream, &hits, sizeof(int32_t), hipMemcpyHostToDevice));
  return FMD_OK;
}

int fmd_batch_sync(fmd_batch *b) {
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  return fmdh_obj_sync(&b->o);           /* (its own stream, the pump's copy stream and the stream of the most recent launch when the caller supplied one) */
}

int fmd_batch_wait_stream(fmd_batch *b, void *producer_stream) {
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  HIP_TRY(hipSetDevice(b->o.device));
  hipStream_t ps = (hipStream_t)producer_stream;
  if (ps == b->o.ord.stream) return FMD_OK;
  hipEvent_t ev;
  HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, ps);
  if (e == hipSuccess) e = hipStreamWaitEvent(b->o.ord.stream, ev, 0);
  hipEventDestroy(ev);                         /* (released by the runtime once the recorded work has completed) */
  if (e != hipSuccess) return fmd_fail(FMD_E_HIP, "fmd_batch_wait_stream: %s", hipGetErrorString(e));
  return FMD_OK;
}

int fmd_batch_last_kernel_ms(fmd_batch *b, float *ms) {
  if (!b || !ms) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (!b->timed) return fmd_fail(FMD_E_STATE, "the most recent launch carries no timing events (none launched yet, timing off, or captured into a graph)");
  HIP_TRY(hipEventSynchronize(b->ev1));
  HIP_TRY(hipEventElapsedTime(ms, b->ev0, b->ev1));
  return FMD_OK;
}

int fmd_batch_set_timing(fmd_batch *b, int on) {
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  b->no_timing = !on;
  if (!on) b->timed = 0;
  return FMD_OK;
}

static int ensure_staging(fmd_batch *b, int n_blocks) {
  const size_t slots = (size_t)b->n_streams * (size_t)n_blocks;
  const grow_buf v[3] = {{&b->d_iq, slots * (size_t)b->r.cfg.block_len, 0}, {&b->d_pcm, slots * (size_t)b->r.pcm_stride * sizeof(int16_t), 0},
                         {&b->d_lens, slots * sizeof(int32_t), 0}};
  /* no wait: the staging is used only on the batch's own stream, by calls (_run_host, _spectrum_host, full_demod) that wait for it before they return */
  return fmdh_grow(&b->cap_blocks, (size_t)n_blocks, v, 3);
}

static int batch_run_host(fmd_batch *b, const uint8_t *iq, int n_blocks, int16_t *pcm, int32_t *lens, float *levels) {
  if (!b || !iq || !pcm || !lens) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks <= 0) return fmd_fail(FMD_E_ARG, "n_blocks must be positive");
  HIP_TRY(hipSetDevice(b->o.device));
  int rc = ensure_staging(b, n_blocks);
  if (rc) return rc;
  const size_t slots = (size_t)b->n_streams * (size_t)n_blocks;
  const grow_buf lv = {&b->d_levels, slots * sizeof(float), 0};
  /* no wait: d_levels is used only on the batch's own stream, by this call, which waits for it below */
  if (levels && (rc = fmdh_grow(&b->lv_cap_blocks, (size_t)n_blocks, &lv, 1))) return rc;
  const hipStream_t st = b->o.ord.stream;
  rc = fmdh_host_copy(FMD_OK, __func__, st, b->d_iq, iq, slots * (size_t)b->r.cfg.block_len, hipMemcpyHostToDevice);
  if (!rc) rc = run_launch(b, b->d_iq, n_blocks, b->d_pcm, b->d_lens, levels ? b->d_levels : NULL, NULL, NULL);
  rc = fmdh_host_copy(rc, __func__, st, pcm, b->d_pcm, slots * (size_t)b->r.pcm_stride * sizeof(int16_t), hipMemcpyDeviceToHost);
  rc = fmdh_host_copy(rc, __func__, st, lens, b->d_lens, slots * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (levels) rc = fmdh_host_copy(rc, __func__, st, levels, b->d_levels, slots * sizeof(float), hipMemcpyDeviceToHost);
  return fmdh_host_wait(rc, __func__, st);
}

int fmd_batch_run_host(fmd_batch *b, const uint8_t *iq, int n_blocks, int16_t *pcm, int32_t *lens) {
  return batch_run_host(b, iq, n_blocks, pcm, lens, NULL);
}

int fmd_batch_run_host_levels(fmd_batch *b, const uint8_t *iq, int n_blocks, int16_t *pcm, int32_t *lens, float *levels) {
  if (!levels) return fmd_fail(FMD_E_ARG, "NULL argument");
  return batch_run_host(b, iq, n_blocks, pcm, lens, levels);
}

/* ---- capture spectrum ------------------------------------------------------ */

/* The table of (n_bins, window): found, or made now - not while `st` is being captured (nothing can be allocated there). */
static int spectrum_table(fmd_batch *b, int n_bins, int window, hipStream_t st, const struct sp_table **out) {
  for (int i = 0; i < b->sp_n_tab; i++)
    if (b->sp_tab[i].n_bins == n_bins && b->sp_tab[i].window == window) { *out = &b->sp_tab[i]; return FMD_OK; }
  if (fmdh_stream_is_capturing(st))
    return fmd_fail(FMD_E_STATE, "the spectrum tables of n_bins %d, window %d do not exist yet: run one call with them before the capture", n_bins, window);
  if (b->sp_n_tab >= FMD_SP_TABLES) return fmd_fail(FMD_E_UNSUPPORTED, "more than %d (n_bins, window) pairs on one batch", FMD_SP_TABLES);
  const size_t nf = fmdk_spectrum_table_floats(n_bins);
  float *h = (float *)malloc(nf * sizeof(float));
  if (!h) return fmd_fail(FMD_E_NOMEM, "out of host memory");
  struct sp_table *t = &b->sp_tab[b->sp_n_tab];
  memset(t, 0, sizeof(*t));
  fmdk_spectrum_tables(n_bins, window, h, &t->sum_w2);
  hipError_t e = hipMalloc((void **)&t->d_tab, nf * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(t->d_tab, h, nf * sizeof(float), hipMemcpyHostToDevice);   /* (returns when the table is on the device) */
  free(h);
  if (e != hipSuccess) {
    if (t->d_tab) hipFree(t->d_tab);
    t->d_tab = NULL;
    return fmd_fail(FMD_E_HIP, "spectrum tables: %s", hipGetErrorString(e));
  }
  t->n_bins = n_bins;
  t->window = window;
  b->sp_n_tab++;
  *out = t;
  return FMD_OK;
}

static int spectrum_check(const fmd_batch *b, int n_blocks, int n_bins, int window) {
  if (n_blocks < 1) return fmd_fail(FMD_E_ARG, "n_blocks must be positive");
  if (window != FMD_WINDOW_RECT && window != FMD_WINDOW_HANN) return fmd_fail(FMD_E_ARG, "window must be FMD_WINDOW_RECT or FMD_WINDOW_HANN");
  if (n_bins < 1) return fmd_fail(FMD_E_ARG, "n_bins must be positive");
  if (!fmdk_spectrum_built(n_bins)) return fmd_fail(FMD_E_UNSUPPORTED, "n_bins %d is not built: 256, 1024 and 4096 are", n_bins);
  if (n_bins > b->r.cfg.block_len / 2) return fmd_fail(FMD_E_ARG, "n_bins %d exceeds the block's %d samples", n_bins, b->r.cfg.block_len / 2);
  if ((long long)b->n_streams * n_blocks > 0x7fffffffLL) return fmd_fail(FMD_E_ARG, "n_blocks too large: n_streams * n_blocks must stay below 2^31");
  return FMD_OK;
}

int fmd_batch_spectrum_device(fmd_batch *b, const void *d_iq, int n_blocks, int n_bins, int window, void *d_power, void *hip_stream) {
  if (!b || !d_iq || !d_power) return fmd_fail(FMD_E_ARG, "NULL argument");
  int rc = spectrum_check(b, n_blocks, n_bins, window);
  if (rc) return rc;
  if (((uintptr_t)d_iq & 15) != 0 || ((uintptr_t)d_power & 15) != 0) return fmd_fail(FMD_E_ARG, "d_iq and d_power must be 16-byte aligned");
  HIP_TRY(hipSetDevice(b->o.device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->o.ord.stream;
  const struct sp_table *t = NULL;
  if ((rc = spectrum_table(b, n_bins, window, st, &t))) return rc;
  const int nseg = (b->r.cfg.block_len / 2) / n_bins;
  const double scale = 1.0 / ((double)nseg * (double)n_bins * t->sum_w2);
  const int e = fmdk_spectrum(d_iq, b->n_streams * n_blocks, b->r.cfg.block_len, n_bins, t->d_tab, scale, d_power, st);
  if (e) return fmd_fail(FMD_E_HIP, "spectrum kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  b->sp_stream = st == b->o.ord.stream ? NULL : st;
  return FMD_OK;
}

int fmd_batch_spectrum_host(fmd_batch *b, const uint8_t *iq, int n_blocks, int n_bins, int window, float *power) {
  if (!b || !iq || !power) return fmd_fail(FMD_E_ARG, "NULL argument");
  int rc = spectrum_check(b, n_blocks, n_bins, window);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(b->o.device));
  if ((rc = ensure_staging(b, n_blocks))) return rc;
  const size_t slots = (size_t)b->n_streams * (size_t)n_blocks, nf = slots * (size_t)n_bins;
  const grow_buf v = {&b->d_sp_power, nf * sizeof(float), 0};
  /* no wait: d_sp_power is used only on the batch's own stream, by this call, which waits for it below */
  if ((rc = fmdh_grow(&b->sp_power_cap, nf, &v, 1))) return rc;
  const hipStream_t st = b->o.ord.stream;
  rc = fmdh_host_copy(FMD_OK, __func__, st, b->d_iq, iq, slots * (size_t)b->r.cfg.block_len, hipMemcpyHostToDevice);
  if (!rc) rc = fmd_batch_spectrum_device(b, b->d_iq, n_blocks, n_bins, window, b->d_sp_power, NULL);
  rc = fmdh_host_copy(rc, __func__, st, power, b->d_sp_power, nf * sizeof(float), hipMemcpyDeviceToHost);
  return fmdh_host_wait(rc, __func__, st);
}

/* ---- receiver objects (fmd_objects.c) with rates, block length, stream count and device from a batch ---- */

int fmd_batch_subc_create(fmd_subc **out, const fmd_batch *b, int fc, int bw, int n_taps, int decim) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  const fmd_subc_config c = {b->r.cfg.rate_in, fc, bw, n_taps, decim, b->r.cfg.block_len >> 4};
  return fmd_subc_create(out, &c, NULL, b->n_streams, b->o.device);
}

int fmd_batch_tuner_create(fmd_tuner **out, const fmd_batch *b, int step_hz, int bw, int n_taps, int n_sources) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  if (b->r.cfg.rate_in > 0x7fffffff / 8) return fmd_fail(FMD_E_ARG, "8 x rate_in does not fit");
  const fmd_tuner_config c = {8 * b->r.cfg.rate_in, step_hz, bw, n_taps, b->r.cfg.block_len, 0};
  return fmd_tuner_create(out, &c, NULL, n_sources, b->n_streams, b->o.device);
}

int fmd_batch_scan_create(fmd_scan **out, const fmd_batch *b, int n_bins, int raster_hz, int bw, int max_stations) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  if (b->r.cfg.rate_in > 0x7fffffff / 8) return fmd_fail(FMD_E_ARG, "8 x rate_in does not fit");
  const fmd_scan_config c = {8 * b->r.cfg.rate_in, n_bins, raster_hz, bw, 1, 250, 0, max_stations, 4.0f, {0, 0, 0}};
  return fmd_scan_create(out, &c, b->n_streams, b->o.device);
}

int fmd_batch_stereo_create(fmd_stereo **out, const fmd_batch *b, const fmd_subc *pilot, const fmd_stereo_config *cfg) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  if (!cfg) return fmd_fail(FMD_E_ARG, "stereo config is NULL");
  if (b->r.cfg.mode != 2) return fmd_fail(FMD_E_ARG, "the batch is not stereo (mode %d): its PCM has no L, R frames to blend", b->r.cfg.mode);
  fmd_stereo_config c = *cfg;
  c.pcm_stride = b->r.pcm_stride;
  c.pilot_per_block = pilot ? fmd_subc_out_per_block(pilot) : 0;
  return fmd_stereo_create(out, &c, b->n_streams, b->o.device);
}

int fmd_batch_get_state(fmd_batch *b, int stream, fmd_stream_state *out) {
  if (!b || !out || stream < 0 || stream >= b->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  return fmdh_obj_get_state(&b->o, stream, out);
}

int fmd_batch_set_state(fmd_batch *b, int stream, const fmd_stream_state *in) {
  if (!b || !in || stream < 0 || stream >= b->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  return fmdh_obj_set_state(&b->o, stream, in);
}

int fmd_batch_reset(fmd_batch *b) {
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  const int rc = fmdh_obj_reset(&b->o);      /* (the current state: the one the next launch reads) */
  if (rc) return rc;
  if (b->sq_on) return squelch_close_all(b);
  return FMD_OK;
}

/* ---- reference-shaped surface --------------------------------------------- */
/*
 * One single-stream batch per demod_state, found through a small registry
 * keyed by the struct's address (the reference struct has no spare pointer
 * field).  The batch is (re)built when the parameters that shape the kernels
 * change.  State lives in the struct between calls, like in the reference.
 */
struct drop_in {
  struct demod_state *key;
  fmd_batch *batch;
  fmd_config cfg;
  int convert_mode;   /* 0: rotate_90_u8_f32, 1: u8_f32 */
  /* One synchronisation per block (round 4).  The carried state stays on the device; `shadow` is what the last call
   * mirrored into the struct (linear histories, as the device keeps them).  A call whose struct still holds exactly
   * that skips the state upload; a caller that edited the struct's state between calls (the reference allows it: it is
   * a plain struct) is noticed by the comparison and gets its values uploaded.  `pin` is one pinned block the PCM, the
   * block length and the new state land in, behind a single hipStreamSynchronize. */
  fmd_stream_state shadow;
  int shadow_valid;
  int shadow_pos;     /* lpr.pos the shadow's linear histories correspond to */
  struct dropin_pin { fmd_stream_state st; int32_t len; int32_t pad[3]; int16_t pcm[]; } *pin;
  size_t pin_pcm;     /* int16 capacity of pin->pcm */
};

/* The registry: heap nodes behind a growing array of pointers (a node's address is stable for as long as its struct is registered; rounds 1 - 5 had 64
 * fixed slots and aborted on the 65th struct). */
static struct drop_in **g_drop;
static int g_drop_n, g_drop_cap;
static pthread_mutex_t g_drop_m = PTHREAD_MUTEX_INITIALIZER;

static struct drop_in *drop_find(struct demod_state *d, int create) {
  struct drop_in *hit = NULL;
  int empty = -1;
  pthread_mutex_lock(&g_drop_m);
  for (int i = 0; i < g_drop_n; i++) {
    if (g_drop[i] && g_drop[i]->key == d) { hit = g_drop[i]; break; }
    if (!g_drop[i] && empty < 0) empty = i;
  }
  if (!hit && create) {
    if (empty < 0 && g_drop_n == g_drop_cap) {
      const int cap = g_drop_cap ? 2 * g_drop_cap : 16;
      struct drop_in **g = (struct drop_in **)realloc(g_drop, (size_t)cap * sizeof(*g));
      if (g) { g_drop = g; g_drop_cap = cap; }
    }
    if (empty < 0 && g_drop_n < g_drop_cap) { empty = g_drop_n++; g_drop[empty] = NULL; }
    if (empty >= 0 && (hit = (struct drop_in *)calloc(1, sizeof(*hit)))) {
      hit->key = d;
      g_drop[empty] = hit;
    }
  }
  pthread_mutex_unlock(&g_drop_m);
  return hit;
}
static void drop_forget(struct drop_in *di) {
  pthread_mutex_lock(&g_drop_m);
  for (int i = 0; i < g_drop_n; i++)
    if (g_drop[i] == di) g_drop[i] = NULL;
  pthread_mutex_unlock(&g_drop_m);
  free(di);
}

/* The arithmetic family of the reference-shaped calls, whose signatures have no room for it: fmd_dropin_set_math() if the caller said so, else FMD_MATH_FAST in
 * the environment selects the +-1 LSB kernels (read once, at the first full_demod), else the bit-exact ones. */
static int g_dropin_math = -1, g_dropin_math_set = 0;
static pthread_once_t g_dropin_once = PTHREAD_ONCE_INIT;
static void dropin_read_env(void) { if (!g_dropin_math_set) g_dropin_math = getenv("FMD_MATH_FAST") ? FMD_MATH_FAST : FMD_MATH_EXACT; }
int fmd_dropin_set_math(int math) {
  if (math < FMD_MATH_EXACT || math > FMD_MATH_FAST_MFMA_F) return fmd_fail(FMD_E_ARG, "fmd_dropin_set_math: not a math value");
  g_dropin_math = math;
  g_dropin_math_set = 1;
  return FMD_OK;
}

/* What a failure inside a void reference-shaped call does: the caller's handler if one is installed (the call then returns with result_len = 0), else a line
 * on stderr and abort() - a demodulator that silently stops producing audio is the worse failure for the program this drops into. */
static fmd_dropin_error_fn g_dropin_err;
static void *g_dropin_err_ctx;
void fmd_dropin_set_error_handler(fmd_dropin_error_fn fn, void *ctx) { g_dropin_err = fn; g_dropin_err_ctx = ctx; }
static void die(const char *what) {
  if (g_dropin_err) { g_dropin_err(what, fmd_last_error(), g_dropin_err_ctx); return; }
  fprintf(stderr, "fmdemod_mi355x: %s: %s\n", what, fmd_last_error());
  abort();
}
#define DIE(d, what) do { die(what); if (d) (d)->result_len = 0; return; } while (0)

void init_u8_f32_table(void) {}  /* the conversion is arithmetic on the device (exact, no table) */
void init_lp_f32(void) {}        /* taps are designed per batch in fmd_design_taps              */

void demod_init(struct demod_state *s) {   /* src/rtl_fm_player.c:1156-1195 */
  s->rate_in = 240000;
  s->rate_out = 240000;
  s->squelch_level = 0;
  s->conseq_squelch = 10;
  s->terminate_on_squelch = 0;
  s->squelch_hits = 11;
  s->downsample_passes = 0;
  s->comp_fir_size = 0;
  s->prev_index = 0;
  s->post_downsample = 1;
  s->custom_atan = 1;
  s->deemph = 0.000050;
  s->offset_tuning = 0;
  s->rate_out2 = 48000;
  s->pre_j = s->pre_r = s->now_r = s->now_j = 0;
  s->pre_j_f32 = s->pre_r_f32 = 0;
  s->prev_lpr_index = 0;
  s->deemph_a = 0;
  s->deemph_l = 0;
  s->deemph_r = 0;
  s->deemph_l_f32 = 0;
  s->deemph_r_f32 = 0;
  s->volume = 0.4f;
  s->now_lpr = 0;
  s->lpr.mode = 2;
  s->lpr.size = 90;
  s->lpr.br = s->lpr.bm = s->lpr.bs = NULL;
  s->lpr.fm = s->lpr.fp = s->lpr.fs = NULL;
  pthread_rwlock_init(&s->rw, NULL);
  pthread_cond_init(&s->ready, NULL);
  pthread_mutex_init(&s->ready_m, NULL);
  s->output_target = NULL;
}

void init_lp_real_f32(struct demod_state *fm) {   /* src/rtl_fm_player.c:413-453 */
  struct lp_real *l = &fm->lpr;
  l->rsize = l->size >> 1;
  l->pp = 0;
  l->pos = 0;
  l->br = (float *)calloc((size_t)l->size, 4);
  l->bm = (float *)calloc((size_t)l->size, 4);
  l->bs = (float *)calloc((size_t)l->size, 4);
  l->fm = (float *)calloc((size_t)l->rsize, 4);
  l->fp = (float *)calloc((size_t)l->rsize, 4);
  l->fs = (float *)calloc((size_t)l->rsize, 4);
  fmdk_design_mpx(l->size, fm->rate_in, l->fm, l->fp, l->fs, &l->swf, &l->cwf);
}

void fmd_demod_release(struct demod_state *d) {
  struct drop_in *di = drop_find(d, 0);
  if (!di) return;
  fmd_batch_destroy(di->batch);
  if (di->pin) hipHostFree(di->pin);
  drop_forget(di);
}

void deinit_lp_real_f32(struct demod_state *fm) {   /* src/rtl_fm_player.c:455-470 */
  struct lp_real *l = &fm->lpr;
  fmd_demod_release(fm);
  l->rsize = 0;
  free(l->br); free(l->bm); free(l->bs); free(l->fm); free(l->fp); free(l->fs);
  l->br = l->bm = l->bs = l->fm = l->fp = l->fs = NULL;
}

void rotate_90_u8_f32(struct demod_state *d) {   /* src/rtl_fm_player.c:206-226 */
  struct drop_in *di = drop_find(d, 1);
  if (!di) { fmd_fail(FMD_E_NOMEM, "out of host memory"); DIE(d, "rotate_90_u8_f32"); }
  di->convert_mode = 0;
  d->lp_len = (int)d->buf_len;
}

void u8_f32(struct demod_state *d) {             /* src/rtl_fm_player.c:228-239 */
  struct drop_in *di = drop_find(d, 1);
  if (!di) { fmd_fail(FMD_E_NOMEM, "out of host memory"); DIE(d, "u8_f32"); }
  di->convert_mode = 1;
  d->lp_len = (int)d->buf_len;
}

/* ring (write index pos) -> linear oldest-first */
static void ring_to_linear(const float *ring, int size, int pos, float *lin) {
  for (int i = 0; i < size; i++) lin[i] = ring[(pos + i) % size];
}
static void linear_to_ring(const float *lin, int size, int pos, float *ring) {
  for (int i = 0; i < size; i++) ring[(pos + i) % size] = lin[i];
}

/* The carried state as the struct holds it, in the device's form (linear histories). */
static void pack_state(const struct demod_state *d, fmd_stream_state *st) {
  const int size = d->lpr.size;
  memset(st, 0, sizeof(*st));
  memcpy(st->tb, d->lowpass_tb, sizeof(st->tb));
  st->pre_r = d->pre_r_f32;
  st->pre_j = d->pre_j_f32;
  st->pp = d->lpr.pp;
  st->deemph_l = d->deemph_l_f32;
  st->deemph_r = d->deemph_r_f32;
  st->acc = d->prev_lpr_index;
  ring_to_linear(d->lpr.br, size, d->lpr.pos, st->br);
  ring_to_linear(d->lpr.bm, size, d->lpr.pos, st->bm);
  ring_to_linear(d->lpr.bs, size, d->lpr.pos, st->bs);
}

void full_demod(struct demod_state *d) {         /* src/rtl_fm_player.c:758-788 */
  struct drop_in *di = drop_find(d, 1);
  if (!di) { fmd_fail(FMD_E_NOMEM, "out of host memory"); DIE(d, "full_demod"); }
  if (!d->lpr.br || !d->lpr.fm) { fmd_fail(FMD_E_STATE, "init_lp_real_f32 was not called"); DIE(d, "full_demod"); }
  pthread_once(&g_dropin_once, dropin_read_env);
  const int math = g_dropin_math;
  fmd_config c = {d->rate_in, d->rate_out, d->rate_out2, d->lpr.mode, d->lpr.size, d->deemph != 0.0,
                  di->convert_mode, d->deemph_lambda, d->volume, (int32_t)d->buf_len, math};
  if (!di->batch || memcmp(&c, &di->cfg, sizeof(c)) != 0) {
    fmd_batch_destroy(di->batch);
    di->batch = NULL;
    fmd_taps t;
    memset(&t, 0, sizeof(t));
    fmdk_design_fb(t.fb);
    memcpy(t.fm, d->lpr.fm, sizeof(float) * (size_t)(d->lpr.size >> 1));   /* the caller's own tables */
    memcpy(t.fp, d->lpr.fp, sizeof(float) * (size_t)(d->lpr.size >> 1));
    memcpy(t.fs, d->lpr.fs, sizeof(float) * (size_t)(d->lpr.size >> 1));
    t.swf = d->lpr.swf;
    t.cwf = d->lpr.cwf;
    if (fmd_batch_create(&di->batch, &c, &t, 1, -1)) DIE(d, "full_demod: fmd_batch_create");
    di->cfg = c;
    /* a new batch starts from zeroed device state: what the struct holds (the stream so far - the reference keeps running across a
     * change of volume, buf_len, rates or de-emphasis, all of which are in fmd_config) must be uploaded whatever the shadow says */
    di->shadow_valid = 0;
  }
  fmd_batch *b = di->batch;
  const int size = d->lpr.size;

  /* struct -> device state: only when the struct does not hold what the last call left in it */
  fmd_stream_state st;
  pack_state(d, &st);
  const int upload = !(di->shadow_valid && di->shadow_pos == d->lpr.pos && memcmp(&st, &di->shadow, sizeof(st)) == 0);

  if (hipSetDevice(b->o.device) != hipSuccess) { fmd_fail(FMD_E_HIP, "hipSetDevice failed"); DIE(d, "full_demod"); }
  if (ensure_staging(b, 1)) DIE(d, "full_demod: staging");
  if (!di->pin || di->pin_pcm < (size_t)b->r.pcm_stride) {
    if (di->pin) hipHostFree(di->pin);
    di->pin = NULL;
    if (hipHostMalloc((void **)&di->pin, sizeof(*di->pin) + sizeof(int16_t) * (size_t)b->r.pcm_stride, hipHostMallocDefault) != hipSuccess) {
      fmd_fail(FMD_E_NOMEM, "pinned staging for the drop-in surface");
      DIE(d, "full_demod");
    }
    di->pin_pcm = (size_t)b->r.pcm_stride;
  }
  hipError_t e = hipSuccess;
  if (upload) {
    /* (a caller-edited state, or the first block: everything queued on the batch's own stream, in order) */
    if (fmdh_order_quiesce(&b->o.ord, b->o.also) != hipSuccess) { fmd_fail(FMD_E_HIP, "device busy"); DIE(d, "full_demod"); }
    di->pin->st = st;
    e = hipMemcpyAsync(b->o.d_state, &di->pin->st, sizeof(st), hipMemcpyHostToDevice, b->o.ord.stream);
    if (e != hipSuccess) { fmd_fail(FMD_E_HIP, "state upload: %s", hipGetErrorString(e)); DIE(d, "full_demod"); }
    if (hipStreamSynchronize(b->o.ord.stream) != hipSuccess) { fmd_fail(FMD_E_HIP, "state upload"); DIE(d, "full_demod"); }   /* pin->st is reused below */
  }
  e = hipMemcpyAsync(b->d_iq, d->buf, (size_t)d->buf_len, hipMemcpyHostToDevice, b->o.ord.stream);
  if (e != hipSuccess) { fmd_fail(FMD_E_HIP, "IQ upload: %s", hipGetErrorString(e)); DIE(d, "full_demod"); }
  if (fmd_batch_run_device(b, b->d_iq, 1, b->d_pcm, b->d_lens, NULL)) DIE(d, "full_demod: run");
  if ((e = hipMemcpyAsync(di->pin->pcm, b->d_pcm, sizeof(int16_t) * (size_t)b->r.pcm_stride, hipMemcpyDeviceToHost, b->o.ord.stream)) != hipSuccess ||
      (e = hipMemcpyAsync(&di->pin->len, b->d_lens, sizeof(int32_t), hipMemcpyDeviceToHost, b->o.ord.stream)) != hipSuccess ||
      (e = hipMemcpyAsync(&di->pin->st, b->o.d_state, sizeof(st), hipMemcpyDeviceToHost, b->o.ord.stream)) != hipSuccess ||
      (e = hipStreamSynchronize(b->o.ord.stream)) != hipSuccess) {                       /* the one wait of the block */
    fmd_fail(FMD_E_HIP, "full_demod: %s", hipGetErrorString(e));
    DIE(d, "full_demod");
  }
  const int32_t len = di->pin->len;
  memcpy(d->result, di->pin->pcm, sizeof(int16_t) * (size_t)(len > 0 ? len : 0));
  d->result_len = len;
  d->lp_len = (int)d->buf_len >> 3;                       /* :410 */

  /* device state -> struct (the reference keeps its state there; callers may read it) */
  st = di->pin->st;
  memcpy(d->lowpass_tb, st.tb, sizeof(st.tb));
  d->pre_r_f32 = st.pre_r;
  d->pre_j_f32 = st.pre_j;
  d->deemph_l_f32 = st.deemph_l;
  d->deemph_r_f32 = st.deemph_r;
  d->prev_lpr_index = st.acc;
  if (d->rate_out2 > 0 && d->lpr.mode != 0) {
    const int m = (int)(d->buf_len >> 4);
    const int pos = (d->lpr.pos + m) % size;
    linear_to_ring(st.br, size, pos, d->lpr.br);
    if (d->lpr.mode == 2) {
      linear_to_ring(st.bm, size, pos, d->lpr.bm);
      linear_to_ring(st.bs, size, pos, d->lpr.bs);
      d->lpr.pp = st.pp;
    }
    d->lpr.pos = pos;
  }
  /* what the struct holds now, as the next call will read it back: the fields a mode does not mirror keep the struct's values */
  pack_state(d, &di->shadow);
  di->shadow_pos = d->lpr.pos;
  /* the device's state and the struct's view of it agree exactly when every mirrored field went both ways */
  di->shadow_valid = memcmp(&di->shadow, &st, sizeof(st)) == 0;
}

/* ---- ingest: rings and the pump -------------------------------------------- */
/* The ring, its writer (fmd_ingest_callback) and its accounting are fmd_ring.c, which needs no device.  Here: a ring's memory (pinned when it is
 * bound to a batch, since the ring IS the H2D source of the pump's jobs) and the pump. */
int fmd_ingest_create(fmd_ingest **out, fmd_batch *b, int stream, uint32_t ring_bytes) {
  if (!out) return fmd_fail(FMD_E_ARG, "bad argument");
  *out = NULL;
  if (ring_bytes == 0) ring_bytes = 16u * FMD_MAXIMUM_BUF_LENGTH;   /* include/rtl_fm_player.h:65 */
  if (b) {
    if (stream < 0 || stream >= b->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
    if (b->ingest[stream]) return fmd_fail(FMD_E_STATE, "stream %d already has an ingest ring", stream);
    if (ring_bytes < (uint32_t)b->r.cfg.block_len) return fmd_fail(FMD_E_ARG, "ring smaller than one block");
    if (hipSetDevice(b->o.device) != hipSuccess) return fmd_fail(FMD_E_HIP, "hipSetDevice(%d) failed", b->o.device);
  }
  fmd_ingest *g = (fmd_ingest *)calloc(1, sizeof(*g));
  if (!g) return fmd_fail(FMD_E_NOMEM, "out of host memory");
  /* zero like the reference's static _input_buffer.  An unbound ring: plain host memory, no device involved; drained with fmd_ingest_pop */
  uint8_t *mem = NULL;
  if (!b) mem = (uint8_t *)calloc(ring_bytes, 1);
  else if (hipHostMalloc((void **)&mem, ring_bytes, hipHostMallocDefault) == hipSuccess) memset(mem, 0, ring_bytes);
  else mem = NULL;
  if (!mem) {
    free(g);
    return b ? fmd_fail(FMD_E_NOMEM, "pinned allocation of %u bytes failed", ring_bytes) : fmd_fail(FMD_E_NOMEM, "out of host memory");
  }
  g->batch = b;
  g->stream = b ? stream : -1;
  g->unbound = !b;
  fmdk_ring_init(g, mem, ring_bytes);
  if (b) b->ingest[stream] = g;
  *out = g;
  return FMD_OK;
}

void fmd_ingest_destroy(fmd_ingest *g) {
  if (!g) return;
  int busy;
  fmd_batch *b = fmdk_ring_owner(g, &busy);
  if (b) {
    /* a queued H2D copy may still read this pinned ring: any job of the batch that holds ring bytes, whatever this ring's own counters say after an
     * overflow - let it finish before the memory goes away */
    if (busy || b->pump[0].ring_held || b->pump[1].ring_held) {
      hipSetDevice(b->o.device);
      fmdh_order_quiesce(&b->o.ord, b->o.also);
    }
    if (b->ingest) b->ingest[g->stream] = NULL;
  }
  if (g->unbound) free(g->ring);
  else hipHostFree(g->ring);
  fmdk_ring_fini(g);
  free(g);
}

static int pump_slot_reserve(fmd_batch *b, struct pump_slot *p, int nb) {
  if (!p->done) {
    HIP_TRY(hipEventCreateWithFlags(&p->h2d_done, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p->done, hipEventDisableTiming));
  }
  const size_t slots = (size_t)b->n_streams * (size_t)nb, pcm = slots * (size_t)b->r.pcm_stride * sizeof(int16_t), lens = slots * sizeof(int32_t);
  const grow_buf v[5] = {{(void **)&p->h_pcm, pcm, 1}, {(void **)&p->h_lens, lens, 1},
                         {&p->d_iq, slots * (size_t)b->r.cfg.block_len, 0}, {&p->d_pcm, pcm, 0}, {&p->d_lens, lens, 0}};
  /* no wait: the slot is free, and a slot's buffers are used only by its own job, on the batch's streams, which fmd_batch_pump_end has waited for */
  return fmdh_grow(&p->cap_blocks, (size_t)nb, v, 5);
}

/* Hand a job's bytes back to the rings' writers: its H2D copies have finished. */
static void pump_release_ring(fmd_batch *b, struct pump_slot *p) {
  if (!p->ring_held) return;
  const uint32_t take = (uint32_t)p->n_blocks * (uint32_t)b->r.cfg.block_len;
  for (int s = 0; s < b->n_streams; s++)
    if (b->ingest[s]) fmdk_ring_release(b->ingest[s], take);
  p->ring_held = 0;
}

/* Release the ring space of jobs whose H2D has completed, without waiting. */
static void pump_release_completed(fmd_batch *b) {
  for (int i = 0; i < 2; i++) {
    struct pump_slot *p = &b->pump[i];
    if (p->n_blocks > 0 && p->ring_held && hipEventQuery(p->h2d_done) == hipSuccess) pump_release_ring(b, p);
  }
}

/* Start one job: whole blocks that every bound stream has buffered (at most max_blocks) are copied to the device STRAIGHT FROM THE PINNED RINGS on the
 * copy stream (one or two asynchronous copies per stream), then kernel and D2H are queued on the batch stream and the call returns.  The bytes stay
 * accounted in the rings until their copy has finished (released by the next _begin / _end that finds the copy done), so nothing is lost if a later
 * step of this call fails.  Up to two jobs may be in flight: the H2D of job k+1 runs beside the kernel of job k. */
int fmd_batch_pump_begin(fmd_batch *b, int max_blocks) {
  if (!b || max_blocks <= 0) return fmd_fail(FMD_E_ARG, "bad argument");
  struct pump_slot *p = &b->pump[b->pump_head];
  if (p->n_blocks > 0) return fmd_fail(FMD_E_STATE, "two jobs already in flight: call fmd_batch_pump_end first");
  HIP_TRY(hipSetDevice(b->o.device));
  pump_release_completed(b);
  const uint32_t bl = (uint32_t)b->r.cfg.block_len;
  int nb = max_blocks;
  for (int s = 0; s < b->n_streams; s++) {
    fmd_ingest *g = b->ingest[s];
    if (!g) return fmd_fail(FMD_E_STATE, "stream %d has no ingest ring", s);
    const int have = (int)(fmdk_ring_ready(g) / bl);
    if (have < nb) nb = have;
  }
  if (nb == 0) return 0;
  if (!b->o.also) HIP_TRY(hipStreamCreateWithFlags(&b->o.also, hipStreamNonBlocking));
  int rc = pump_slot_reserve(b, p, nb);              /* every buffer the job needs, before a byte is taken */
  if (rc) return rc;
  const uint32_t take = (uint32_t)nb * bl;
  int taken = 0;
  hipError_t e = hipSuccess;
  for (int s = 0; s < b->n_streams && e == hipSuccess; s++) {
    fmd_ingest *g = b->ingest[s];
    uint8_t *dst = (uint8_t *)p->d_iq + (size_t)s * take;
    const uint32_t from = fmdk_ring_take(g, take);
    taken = s + 1;
    uint32_t first;
    const uint8_t *ring = fmdk_ring_split(g, from, take, &first);
    e = hipMemcpyAsync(dst, ring + from, first, hipMemcpyHostToDevice, b->o.also);
    if (e == hipSuccess && take > first) e = hipMemcpyAsync(dst + first, ring, take - first, hipMemcpyHostToDevice, b->o.also);
  }
  const size_t slots = (size_t)b->n_streams * (size_t)nb;
  if (e == hipSuccess) e = hipEventRecord(p->h2d_done, b->o.also);
  if (e == hipSuccess) e = hipStreamWaitEvent(b->o.ord.stream, p->h2d_done, 0);
  int launched = 0;
  if (e == hipSuccess) {
    rc = fmd_batch_run_device(b, p->d_iq, nb, p->d_pcm, p->d_lens, NULL);
    if (rc == FMD_OK) {
      launched = 1;                                    /* the streams' state has advanced by nb blocks from here on */
      e = hipMemcpyAsync(p->h_pcm, p->d_pcm, slots * (size_t)b->r.pcm_stride * sizeof(int16_t), hipMemcpyDeviceToHost, b->o.ord.stream);
      if (e == hipSuccess) e = hipMemcpyAsync(p->h_lens, p->d_lens, slots * sizeof(int32_t), hipMemcpyDeviceToHost, b->o.ord.stream);
      if (e == hipSuccess) e = hipEventRecord(p->done, b->o.ord.stream);
    }
  }
  if (!launched) {
    /* nothing has been demodulated: give the bytes back.  Wait for the copies already queued, then un-take them (they are still in the rings, so the
     * next call sees them again); a part an overflow has meanwhile released (moved from inflight to debt) is not taken back a second time:
     * fmdk_ring_untake says whose bytes the debt is - the other job's first, if it still holds ring space */
    hipStreamSynchronize(b->o.also);
    const struct pump_slot *other = &b->pump[b->pump_head ^ 1];
    const uint32_t old_take = (other->n_blocks > 0 && other->ring_held) ? (uint32_t)other->n_blocks * bl : 0;
    for (int s = 0; s < taken; s++) fmdk_ring_untake(b->ingest[s], take, old_take);
    if (e != hipSuccess) return fmd_fail(FMD_E_HIP, "pump: %s (%d)", hipGetErrorString(e), (int)e);
    return rc;
  }
  /* the kernel is queued: the job exists whatever happened to its D2H (un-taking the bytes now would demodulate
   * the same blocks twice); a failed D2H is reported by fmd_batch_pump_end, which still releases the ring */
  p->n_blocks = nb;
  p->ring_held = 1;
  p->failed = (e != hipSuccess) ? (int)e : 0;
  b->pump_head ^= 1;
  return nb;
}

/* Finish the oldest job begun: waits for it and copies its PCM and lengths out (layout as fmd_batch_run_host for that job's block count).  Returns the
 * block count, 0 if none. */
int fmd_batch_pump_end(fmd_batch *b, int16_t *pcm, int32_t *lens) {
  if (!b || !pcm || !lens) return fmd_fail(FMD_E_ARG, "bad argument");
  struct pump_slot *p = &b->pump[b->pump_tail];
  if (p->n_blocks <= 0) return 0;
  HIP_TRY(hipSetDevice(b->o.device));
  if (p->failed) {
    /* the job ran (state advanced) but its PCM never left the device: wait for the kernel, free the slot and the ring space, report */
    const int err = p->failed;
    hipStreamSynchronize(b->o.ord.stream);
    pump_release_ring(b, p);
    p->n_blocks = 0;
    p->failed = 0;
    b->pump_tail ^= 1;
    return fmd_fail(FMD_E_HIP, "pump: the job's device-to-host copy could not be queued: %s (%d); its %s", hipGetErrorString((hipError_t)err),
                err, "blocks were demodulated and are lost");
  }
  HIP_TRY(hipEventSynchronize(p->done));
  pump_release_ring(b, p);                           /* done implies its H2D is done */
  pump_release_completed(b);
  const size_t slots = (size_t)b->n_streams * (size_t)p->n_blocks;
  memcpy(pcm, p->h_pcm, slots * (size_t)b->r.pcm_stride * sizeof(int16_t));
  memcpy(lens, p->h_lens, slots * sizeof(int32_t));
  const int nb = p->n_blocks;
  p->n_blocks = 0;
  b->pump_tail ^= 1;
  return nb;
}

int fmd_batch_pump(fmd_batch *b, int max_blocks, int16_t *pcm, int32_t *lens) {
  if (!b || !pcm || !lens || max_blocks <= 0) return fmd_fail(FMD_E_ARG, "bad argument");
  if (b->pump[b->pump_tail].n_blocks > 0) return fmd_fail(FMD_E_STATE, "jobs in flight: finish them with fmd_batch_pump_end");
  const int nb = fmd_batch_pump_begin(b, max_blocks);
  if (nb <= 0) return nb;
  const int got = fmd_batch_pump_end(b, pcm, lens);
  return got < 0 ? got : nb;
}
