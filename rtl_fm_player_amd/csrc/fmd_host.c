/*
 * fmd_host.c - C host layer of libfmdemod_mi355x.so.
 *
 * Plain C above the HIP runtime's C API: device buffers and carried state
 * (what needs no device - configuration checks, filter design, the kernel
 * family and its arguments - is fmd_resolve.c), the batch API, the reference-shaped
 * entry points (same names / struct layout as rtl_fm_player.c) and the
 * pump that drains the ingest rings (the ring itself and its accounting need no device either: fmd_ring.c).  All arithmetic of the hot path
 * runs in the kernels of fmd_kernels.inc (built as fmd_kernels_{exact,fast,mfma}.hip); nothing here computes a sample.
 */
#define _GNU_SOURCE
#include <math.h>
#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "fmd_internal.h"
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

#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fmd_fail(FMD_E_HIP, "%s failed: %s (%d)", #expr, hipGetErrorString(e_), (int)e_); \
  } while (0)

int fmd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

/* ---- device plumbing shared by the objects below --------------------------- */
/* Count the devices, default *dev (< 0) to the current one, range-check it and make it current. */
static int open_device(int *dev) {
  int ndev = 0, device = *dev;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fmd_fail(FMD_E_NODEVICE, "no HIP device: the MI355X path has no CPU fallback");
  if (device < 0) HIP_TRY(hipGetDevice(&device));
  if (device >= ndev) return fmd_fail(FMD_E_ARG, "device %d out of range (%d devices)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  *dev = device;
  return FMD_OK;
}

/* Is st being captured into a hipGraph (nothing can be allocated, and no event of ours recorded outside it, then). */
static int stream_is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess) { cap = hipStreamCaptureStatusNone; (void)hipGetLastError(); }
  return cap != hipStreamCaptureStatusNone;
}

/* Buffers (device, or pinned host) that share one capacity, grown on demand: below `need` all n are freed and made anew (on a failure the pointers
 * not yet made are NULL and the capacity 0).  Does not synchronise: each caller says why nothing queued still uses the old buffers. */
typedef struct { void **p; size_t bytes; int pinned; } grow_buf;
static int grow(size_t *cap, size_t need, const grow_buf *v, int n) {
  if (need <= *cap) return FMD_OK;
  for (int i = 0; i < n; i++) {
    if (*v[i].p) (void)(v[i].pinned ? hipHostFree(*v[i].p) : hipFree(*v[i].p));
    *v[i].p = NULL;
  }
  *cap = 0;
  for (int i = 0; i < n; i++) HIP_TRY(v[i].pinned ? hipHostMalloc(v[i].p, v[i].bytes, hipHostMallocDefault) : hipMalloc(v[i].p, v[i].bytes));
  *cap = need;
  return FMD_OK;
}

/* Where an object's launches run.  Each launch reads the state the one before wrote: launches on one stream are ordered by the stream, a change
 * of stream between two launches is handed over with an event. */
struct launch_order {
  hipStream_t stream;          /* the object's own */
  hipStream_t last_stream;     /* stream of the most recent launch (the own or the caller's) */
  int launched;                /* a launch has been queued on last_stream */
  hipEvent_t ev_order;         /* makes the new stream wait for the previous launch */
};

/* Wait for everything queued: the stream of the most recent launch when the caller supplied it, `also` (NULL: none) and the own stream. */
static hipError_t order_quiesce(struct launch_order *o, hipStream_t also) {
  hipError_t e = hipSuccess, t;
  if (o->launched && o->last_stream && o->last_stream != o->stream && (t = hipStreamSynchronize(o->last_stream)) != hipSuccess) e = t;
  if (also && (t = hipStreamSynchronize(also)) != hipSuccess) e = t;
  if (o->stream && (t = hipStreamSynchronize(o->stream)) != hipSuccess) e = t;
  if (e == hipSuccess) o->launched = 0;        /* nothing is in flight: the next launch needs no hand-over, whatever stream it is on */
  return e;
}

/* Before a launch on st: 0 when st is ordered behind the previous launch, 1 when that needs the event and st is being captured - recording an event
 * of ours on a stream outside the capture would invalidate it, so the caller refuses with what to do instead - or a status (< 0). */
static int order_handover(struct launch_order *o, hipStream_t st) {
  if (!o->launched || o->last_stream == st) return 0;
  if (stream_is_capturing(st)) return 1;
  HIP_TRY(hipEventRecord(o->ev_order, o->last_stream));
  HIP_TRY(hipStreamWaitEvent(st, o->ev_order, 0));
  return 0;
}

static void order_launched(struct launch_order *o, hipStream_t st) { o->last_stream = st; o->launched = 1; }

/* The library reads ONE environment variable, FMD_MATH_FAST, and only for the reference-shaped surface whose signatures have no room for the
 * choice (dropin_read_env).  The batch API's kernel family is fmd_config.math and nothing else. */

/* ---- batch object --------------------------------------------------------- */

#define FMD_SP_TABLES 8        /* (n_bins, window) pairs a batch keeps tables for: three sizes x two windows today */

struct fmd_batch {
  fmdk_resolved r;              /* configuration, taps, kernel arguments and instantiation as fmdk_resolve made them; fmd_batch_create adds kp.dec_tables */
  int n_streams;
  int device;
  struct launch_order ord;     /* own stream and the order of the state ping-pong across streams */
  hipEvent_t ev0, ev1;
  int no_timing;               /* fmd_batch_set_timing(b, 0): no event pair around the kernel */
  int timed;
  void *d_state[2];            /* fmd_stream_state[n_streams], ping-pong: a multi-chunk launch
                                  reads one and writes the other                        */
  int cur;                     /* index of the buffer holding the current state          */
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
  int pump_head, pump_tail;    /* next slot to begin / oldest slot not yet ended */
  hipStream_t copy_stream;     /* H2D of job k+1 runs beside the kernel of job k */
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
  if ((rc = open_device(&device))) return rc;

  fmd_batch *b = (fmd_batch *)calloc(1, sizeof(*b));
  if (!b) return fmd_fail(FMD_E_NOMEM, "out of host memory");
  b->n_streams = n_streams;
  b->device = device;
  if ((rc = fmdk_resolve(cfg, taps, &b->r))) { free(b); return rc; }

  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&b->ord.stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreate(&b->ev0)) != hipSuccess || (e = hipEventCreate(&b->ev1)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&b->ord.ev_order, hipEventDisableTiming)) != hipSuccess ||
      (e = hipMalloc(&b->d_state[0], sizeof(fmd_stream_state) * (size_t)n_streams)) != hipSuccess ||
      (e = hipMalloc(&b->d_state[1], sizeof(fmd_stream_state) * (size_t)n_streams)) != hipSuccess ||
      (e = hipMemsetAsync(b->d_state[0], 0, sizeof(fmd_stream_state) * (size_t)n_streams, b->ord.stream)) != hipSuccess ||
      (e = hipMemsetAsync(b->d_state[1], 0, sizeof(fmd_stream_state) * (size_t)n_streams, b->ord.stream)) != hipSuccess ||
      (e = hipStreamSynchronize(b->ord.stream)) != hipSuccess) {
    rc = fmd_fail(FMD_E_HIP, "device setup failed: %s", hipGetErrorString(e));
    fmd_batch_destroy(b);
    return rc;
  }
  if (b->r.cfg.math == FMD_MATH_FAST_MFMA_F && b->r.kp.dec_p > 0) {
    size_t nb = 0;
    uint8_t *t = fmdk_dec_tables(&b->r, &nb);
    if (!t) { fmd_batch_destroy(b); return fmd_fail(FMD_E_NOMEM, "out of host memory"); }
    e = hipMalloc(&b->d_dec_tables, nb);
    if (e == hipSuccess) e = hipMemcpy(b->d_dec_tables, t, nb, hipMemcpyHostToDevice);
    free(t);
    if (e != hipSuccess) { rc = fmd_fail(FMD_E_HIP, "device setup failed: %s", hipGetErrorString(e)); fmd_batch_destroy(b); return rc; }
    b->r.kp.dec_tables = b->d_dec_tables;
  }
  {
    hipDeviceProp_t prop;
    b->n_cus = (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
                   ? prop.multiProcessorCount : 256;
  }
  b->ingest = (struct fmd_ingest **)calloc((size_t)n_streams, sizeof(*b->ingest));
  if (!b->ingest) { fmd_batch_destroy(b); return fmd_fail(FMD_E_NOMEM, "out of host memory"); }
  *out = b;
  return FMD_OK;
}

/* Wait for everything this batch has queued: its own stream, the copy stream of the pump and the stream of the most recent launch when the caller supplied one. */
static hipError_t batch_quiesce(fmd_batch *b) { return order_quiesce(&b->ord, b->copy_stream); }

void fmd_batch_destroy(fmd_batch *b) {
  if (!b) return;
  hipSetDevice(b->device);
  batch_quiesce(b);
  if (b->sp_stream && b->sp_stream != b->ord.stream) hipStreamSynchronize(b->sp_stream);   /* a spectrum launch may still read its table */
  for (int i = 0; i < b->sp_n_tab; i++)
    if (b->sp_tab[i].d_tab) hipFree(b->sp_tab[i].d_tab);
  /* rings outlive the batch (their owner destroys them with fmd_ingest_destroy, before or after this call): detach them so that neither side touches freed memory */
  if (b->ingest)
    for (int i = 0; i < b->n_streams; i++)
      if (b->ingest[i]) fmdk_ring_detach(b->ingest[i]);
  void *const dev[] = {b->d_sp_power, b->d_dec_tables, b->d_lv_part, b->d_levels, b->d_sq_thr, b->d_sq_hits, b->d_state[0], b->d_state[1], b->d_iq, b->d_pcm,
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
  if (b->copy_stream) hipStreamDestroy(b->copy_stream);
  if (b->ev0) hipEventDestroy(b->ev0);
  if (b->ev1) hipEventDestroy(b->ev1);
  if (b->ord.ev_order) hipEventDestroy(b->ord.ev_order);
  if (b->ord.stream) hipStreamDestroy(b->ord.stream);
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
  HIP_TRY(hipSetDevice(b->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->ord.stream;
  const fmdk_params kp = fmdk_launch_params(&b->r, b->n_streams, b->n_cus, b->time_split, n_blocks, dbg && (dbg->y || dbg->v || dbg->mpx || dbg->prof));
  /* The state is always ping-ponged (the kernel's in / out pointers never alias); order_handover orders a launch behind the previous one's output. */
  /* A caller's stream that is being captured into a hipGraph: the launch becomes a node of the graph.  The timing events have no meaning there (the launch
   * carries none and fmd_batch_last_kernel_ms says so afterwards), and the event hand-over between streams would record an event of the batch on a stream
   * outside the capture - which invalidates the capture: refused, with what to do instead. */
  const int capturing = stream_is_capturing(st);
  int rc = order_handover(&b->ord, st);
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
      HIP_TRY(batch_quiesce(b));                  /* (the launch in flight may still read the old area) */
      const grow_buf v = {&b->d_lv_part, need * 2 * sizeof(float), 0};
      if ((rc = grow(&b->lv_part_cap, need, &v, 1))) return rc;
    }
  }
  const int nxt = b->cur ^ 1;
  const int with_events = !b->no_timing && !capturing;
  /* the timing events ride on the kernel's dispatch packet (fmdk_launch): no packets of their own */
  int e = fmdk_launch(&kp, &b->r.var, b->n_streams, d_iq, d_pcm, d_lens, b->d_state[b->cur],
                      b->d_state[nxt], dbg, lv ? b->d_lv_part : NULL, st, with_events ? (void *)b->ev0 : NULL, with_events ? (void *)b->ev1 : NULL);
  if (e) return fmd_fail(FMD_E_HIP, "kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  b->cur = nxt;
  order_launched(&b->ord, st);
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
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(batch_quiesce(b));
  if (!thresholds) {
    b->sq_on = 0;
    return FMD_OK;
  }
  if (!b->d_sq_thr) HIP_TRY(hipMalloc((void **)&b->d_sq_thr, sizeof(float) * (size_t)b->n_streams));
  if (!b->d_sq_hits) HIP_TRY(hipMalloc((void **)&b->d_sq_hits, sizeof(int32_t) * (size_t)b->n_streams));
  HIP_TRY(hipMemcpy(b->d_sq_thr, thresholds, sizeof(float) * (size_t)b->n_streams, hipMemcpyHostToDevice));
  b->sq_conseq = conseq;
  const int rc = squelch_close_all(b);
  if (rc) return rc;
  b->sq_on = 1;
  return FMD_OK;
}

int fmd_batch_get_squelch_hits(fmd_batch *b, int stream, int32_t *hits) {
  if (!b || !hits || stream < 0 || stream >= b->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  if (!b->d_sq_hits) return fmd_fail(FMD_E_STATE, "squelch was never set on this batch (fmd_batch_set_squelch)");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(batch_quiesce(b));
  HIP_TRY(hipMemcpy(hits, b->d_sq_hits + stream, sizeof(int32_t), hipMemcpyDeviceToHost));
  return FMD_OK;
}

int fmd_batch_set_squelch_hits(fmd_batch *b, int stream, int32_t hits) {
  if (!b || stream < 0 || stream >= b->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  if (!b->d_sq_hits) return fmd_fail(FMD_E_STATE, "squelch was never set on this batch (fmd_batch_set_squelch)");
  if (hits < 0 || hits > b->sq_conseq + 1) return fmd_fail(FMD_E_ARG, "hits must lie in 0 .. conseq + 1 = %d", b->sq_conseq + 1);
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(batch_quiesce(b));
  HIP_TRY(hipMemcpy(b->d_sq_hits + stream, &hits, sizeof(int32_t), hipMemcpyHostToDevice));
  return FMD_OK;
}

int fmd_batch_sync(fmd_batch *b) {
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(batch_quiesce(b));
  return FMD_OK;
}

int fmd_batch_wait_stream(fmd_batch *b, void *producer_stream) {
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  HIP_TRY(hipSetDevice(b->device));
  hipStream_t ps = (hipStream_t)producer_stream;
  if (ps == b->ord.stream) return FMD_OK;
  hipEvent_t ev;
  HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, ps);
  if (e == hipSuccess) e = hipStreamWaitEvent(b->ord.stream, ev, 0);
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
  return grow(&b->cap_blocks, (size_t)n_blocks, v, 3);
}

static int run_host(fmd_batch *b, const uint8_t *iq, int n_blocks, int16_t *pcm, int32_t *lens, float *levels) {
  if (!b || !iq || !pcm || !lens) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks <= 0) return fmd_fail(FMD_E_ARG, "n_blocks must be positive");
  HIP_TRY(hipSetDevice(b->device));
  int rc = ensure_staging(b, n_blocks);
  if (rc) return rc;
  const size_t slots = (size_t)b->n_streams * (size_t)n_blocks;
  const grow_buf lv = {&b->d_levels, slots * sizeof(float), 0};
  /* no wait: d_levels is used only on the batch's own stream, by this call, which waits for it below */
  if (levels && (rc = grow(&b->lv_cap_blocks, (size_t)n_blocks, &lv, 1))) return rc;
  HIP_TRY(hipMemcpyAsync(b->d_iq, iq, slots * (size_t)b->r.cfg.block_len, hipMemcpyHostToDevice, b->ord.stream));
  rc = run_launch(b, b->d_iq, n_blocks, b->d_pcm, b->d_lens, levels ? b->d_levels : NULL, NULL, NULL);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(pcm, b->d_pcm, slots * (size_t)b->r.pcm_stride * sizeof(int16_t), hipMemcpyDeviceToHost, b->ord.stream));
  HIP_TRY(hipMemcpyAsync(lens, b->d_lens, slots * sizeof(int32_t), hipMemcpyDeviceToHost, b->ord.stream));
  if (levels) HIP_TRY(hipMemcpyAsync(levels, b->d_levels, slots * sizeof(float), hipMemcpyDeviceToHost, b->ord.stream));
  HIP_TRY(hipStreamSynchronize(b->ord.stream));
  return FMD_OK;
}

int fmd_batch_run_host(fmd_batch *b, const uint8_t *iq, int n_blocks, int16_t *pcm, int32_t *lens) {
  return run_host(b, iq, n_blocks, pcm, lens, NULL);
}

int fmd_batch_run_host_levels(fmd_batch *b, const uint8_t *iq, int n_blocks, int16_t *pcm, int32_t *lens, float *levels) {
  if (!levels) return fmd_fail(FMD_E_ARG, "NULL argument");
  return run_host(b, iq, n_blocks, pcm, lens, levels);
}

/* ---- capture spectrum ------------------------------------------------------ */

/* The table of (n_bins, window): found, or made now - not while `st` is being captured (nothing can be allocated there). */
static int spectrum_table(fmd_batch *b, int n_bins, int window, hipStream_t st, const struct sp_table **out) {
  for (int i = 0; i < b->sp_n_tab; i++)
    if (b->sp_tab[i].n_bins == n_bins && b->sp_tab[i].window == window) { *out = &b->sp_tab[i]; return FMD_OK; }
  if (stream_is_capturing(st))
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
  HIP_TRY(hipSetDevice(b->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->ord.stream;
  const struct sp_table *t = NULL;
  if ((rc = spectrum_table(b, n_bins, window, st, &t))) return rc;
  const int nseg = (b->r.cfg.block_len / 2) / n_bins;
  const double scale = 1.0 / ((double)nseg * (double)n_bins * t->sum_w2);
  const int e = fmdk_spectrum(d_iq, b->n_streams * n_blocks, b->r.cfg.block_len, n_bins, t->d_tab, scale, d_power, st);
  if (e) return fmd_fail(FMD_E_HIP, "spectrum kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  b->sp_stream = st == b->ord.stream ? NULL : st;
  return FMD_OK;
}

int fmd_batch_spectrum_host(fmd_batch *b, const uint8_t *iq, int n_blocks, int n_bins, int window, float *power) {
  if (!b || !iq || !power) return fmd_fail(FMD_E_ARG, "NULL argument");
  int rc = spectrum_check(b, n_blocks, n_bins, window);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(b->device));
  if ((rc = ensure_staging(b, n_blocks))) return rc;
  const size_t slots = (size_t)b->n_streams * (size_t)n_blocks, nf = slots * (size_t)n_bins;
  const grow_buf v = {&b->d_sp_power, nf * sizeof(float), 0};
  /* no wait: d_sp_power is used only on the batch's own stream, by this call, which waits for it below */
  if ((rc = grow(&b->sp_power_cap, nf, &v, 1))) return rc;
  HIP_TRY(hipMemcpyAsync(b->d_iq, iq, slots * (size_t)b->r.cfg.block_len, hipMemcpyHostToDevice, b->ord.stream));
  rc = fmd_batch_spectrum_device(b, b->d_iq, n_blocks, n_bins, window, b->d_sp_power, NULL);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(power, b->d_sp_power, nf * sizeof(float), hipMemcpyDeviceToHost, b->ord.stream));
  HIP_TRY(hipStreamSynchronize(b->ord.stream));
  return FMD_OK;
}

/* ---- MPX subcarrier receiver ------------------------------------------------ */
/* An object of its own (csrc/subcarrier.inc): configuration check, tap design and carrier table are fmd_resolve.c's; here its device side.  Everything
 * a launch needs - taps, table, state - is made at create, so a launch allocates nothing and can be captured into a graph. */

struct fmd_subc {
  fmd_subc_config cfg;
  int period;                  /* Pd */
  int n_streams, device;
  struct launch_order ord;     /* own stream; each launch reads the state the one before wrote */
  float *d_taps, *d_carrier;
  void *d_state;               /* fmd_subc_state[n_streams]: read by the receiver kernel, advanced in place by the state kernel behind it */
  void *d_v, *d_z;             /* staging of fmd_subc_run_host, grown on demand */
  size_t cap_blocks;
};

static hipError_t subc_quiesce(fmd_subc *s) { return order_quiesce(&s->ord, NULL); }

int fmd_subc_create(fmd_subc **out, const fmd_subc_config *cfg, const float *taps, int n_streams, int device) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  int rc = fmdk_subc_check(cfg);
  if (rc) return rc;
  if (n_streams <= 0) return fmd_fail(FMD_E_ARG, "n_streams must be positive");
  float h[FMD_SUBC_MAX_TAPS];
  if (taps) {
    for (int k = 0; k < cfg->n_taps; k++) {
      if (!isfinite(taps[k])) return fmd_fail(FMD_E_ARG, "tap %d is not finite", k);
      h[k] = taps[k];
    }
  } else if ((rc = fmd_subc_design(cfg, h))) {
    return rc;
  }
  if ((rc = open_device(&device))) return rc;

  fmd_subc *s = (fmd_subc *)calloc(1, sizeof(*s));
  if (!s) return fmd_fail(FMD_E_NOMEM, "out of host memory");
  s->cfg = *cfg;
  s->period = fmdk_subc_period(cfg);
  s->n_streams = n_streams;
  s->device = device;
  float *car = (float *)malloc(sizeof(float) * 2 * (size_t)s->period);
  if (!car) { free(s); return fmd_fail(FMD_E_NOMEM, "out of host memory"); }
  fmdk_subc_carrier(cfg, car);
  const size_t st_bytes = sizeof(fmd_subc_state) * (size_t)n_streams;
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&s->ord.stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&s->ord.ev_order, hipEventDisableTiming)) != hipSuccess ||
      (e = hipMalloc((void **)&s->d_taps, sizeof(float) * FMD_SUBC_MAX_TAPS)) != hipSuccess ||
      (e = hipMalloc((void **)&s->d_carrier, sizeof(float) * 2 * (size_t)s->period)) != hipSuccess ||
      (e = hipMalloc(&s->d_state, st_bytes)) != hipSuccess ||
      (e = hipMemcpy(s->d_taps, h, sizeof(float) * (size_t)cfg->n_taps, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(s->d_carrier, car, sizeof(float) * 2 * (size_t)s->period, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemsetAsync(s->d_state, 0, st_bytes, s->ord.stream)) != hipSuccess ||
      (e = hipStreamSynchronize(s->ord.stream)) != hipSuccess) {
    free(car);
    rc = fmd_fail(FMD_E_HIP, "device setup failed: %s", hipGetErrorString(e));
    fmd_subc_destroy(s);
    return rc;
  }
  free(car);
  *out = s;
  return FMD_OK;
}

int fmd_batch_subc_create(fmd_subc **out, const fmd_batch *b, int fc, int bw, int n_taps, int decim) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  const fmd_subc_config c = {b->r.cfg.rate_in, fc, bw, n_taps, decim, b->r.cfg.block_len >> 4};
  return fmd_subc_create(out, &c, NULL, b->n_streams, b->device);
}

void fmd_subc_destroy(fmd_subc *s) {
  if (!s) return;
  hipSetDevice(s->device);
  subc_quiesce(s);
  if (s->d_taps) hipFree(s->d_taps);
  if (s->d_carrier) hipFree(s->d_carrier);
  if (s->d_state) hipFree(s->d_state);
  if (s->d_v) hipFree(s->d_v);
  if (s->d_z) hipFree(s->d_z);
  if (s->ord.ev_order) hipEventDestroy(s->ord.ev_order);
  if (s->ord.stream) hipStreamDestroy(s->ord.stream);
  free(s);
}

int fmd_subc_out_per_block(const fmd_subc *s) { return s ? s->cfg.block_samples / s->cfg.decim : FMD_E_ARG; }

int fmd_subc_run_device(fmd_subc *s, const void *d_v, int n_blocks, void *d_z, void *hip_stream) {
  if (!s || !d_v || !d_z) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks < 0) return fmd_fail(FMD_E_ARG, "n_blocks < 0");
  if (n_blocks == 0) return FMD_OK;
  if (((uintptr_t)d_v & 15) != 0 || ((uintptr_t)d_z & 15) != 0) return fmd_fail(FMD_E_ARG, "d_v and d_z must be 16-byte aligned");
  const long long M = s->cfg.block_samples, cpb = (M + FMDK_SUBC_CHUNK - 1) / FMDK_SUBC_CHUNK;
  if (M * n_blocks > 0x7fffffffLL - 2 * FMDK_SUBC_CHUNK)       /* (the kernel's sample index within a stream's launch is 32-bit) */
    return fmd_fail(FMD_E_ARG, "n_blocks too large: block_samples * n_blocks must stay below 2^31 - %d per stream", 2 * FMDK_SUBC_CHUNK);
  if ((long long)s->n_streams * n_blocks * cpb > 0x7fffffffLL) return fmd_fail(FMD_E_ARG, "n_blocks too large: the grid must stay below 2^31 workgroups");
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : s->ord.stream;
  const int rc = order_handover(&s->ord, st);
  if (rc > 0) return fmd_fail(FMD_E_STATE, "the previous launch ran on another stream: call fmd_subc_sync() before capturing this one into a graph");
  if (rc) return rc;
  const int e = fmdk_subc_launch(d_v, s->n_streams, n_blocks, &s->cfg, s->period, s->d_taps, s->d_carrier, s->d_state, d_z, st);
  if (e) return fmd_fail(FMD_E_HIP, "subcarrier kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  order_launched(&s->ord, st);
  return FMD_OK;
}

int fmd_subc_run_host(fmd_subc *s, const float *v, int n_blocks, float *z) {
  if (!s || !v || !z) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks <= 0) return fmd_fail(FMD_E_ARG, "n_blocks must be positive");
  HIP_TRY(hipSetDevice(s->device));
  const size_t slots = (size_t)s->n_streams * (size_t)n_blocks, M = (size_t)s->cfg.block_samples, nz = 2 * (M / (size_t)s->cfg.decim);
  int rc;
  if ((size_t)n_blocks > s->cap_blocks) {
    HIP_TRY(subc_quiesce(s));
    const grow_buf v[2] = {{&s->d_v, slots * M * sizeof(float), 0}, {&s->d_z, slots * nz * sizeof(float), 0}};
    if ((rc = grow(&s->cap_blocks, (size_t)n_blocks, v, 2))) return rc;
  }
  HIP_TRY(hipMemcpyAsync(s->d_v, v, slots * M * sizeof(float), hipMemcpyHostToDevice, s->ord.stream));
  if ((rc = fmd_subc_run_device(s, s->d_v, n_blocks, s->d_z, NULL))) return rc;
  HIP_TRY(hipMemcpyAsync(z, s->d_z, slots * nz * sizeof(float), hipMemcpyDeviceToHost, s->ord.stream));
  HIP_TRY(hipStreamSynchronize(s->ord.stream));
  return FMD_OK;
}

int fmd_subc_get_state(fmd_subc *s, int stream, fmd_subc_state *out) {
  if (!s || !out || stream < 0 || stream >= s->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(subc_quiesce(s));
  HIP_TRY(hipMemcpy(out, (char *)s->d_state + sizeof(*out) * (size_t)stream, sizeof(*out), hipMemcpyDeviceToHost));
  return FMD_OK;
}

int fmd_subc_set_state(fmd_subc *s, int stream, const fmd_subc_state *in) {
  if (!s || !in || stream < 0 || stream >= s->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  if (in->phase < 0 || in->phase >= s->period) return fmd_fail(FMD_E_ARG, "phase %d outside 0 .. %d (the carrier's period)", in->phase, s->period - 1);
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(subc_quiesce(s));
  HIP_TRY(hipMemcpy((char *)s->d_state + sizeof(*in) * (size_t)stream, in, sizeof(*in), hipMemcpyHostToDevice));
  return FMD_OK;
}

int fmd_subc_reset(fmd_subc *s) {
  if (!s) return fmd_fail(FMD_E_ARG, "NULL subcarrier object");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(subc_quiesce(s));
  HIP_TRY(hipMemsetAsync(s->d_state, 0, sizeof(fmd_subc_state) * (size_t)s->n_streams, s->ord.stream));   /* (on the own stream and waited for: see fmd_batch_reset) */
  HIP_TRY(hipStreamSynchronize(s->ord.stream));
  return FMD_OK;
}

int fmd_subc_sync(fmd_subc *s) {
  if (!s) return fmd_fail(FMD_E_ARG, "NULL subcarrier object");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(subc_quiesce(s));
  return FMD_OK;
}

/* ---- channel tuner ---------------------------------------------------------- */
/* An object of its own (csrc/tuner.inc): range checks, tap design, carrier table and the channel table's entries are fmd_resolve.c's; here its device
 * side.  Everything a launch needs - taps, table, channel table, state - is made at create, so a launch allocates nothing and can be captured. */

struct fmd_tuner {
  fmd_tuner_config cfg;
  int period;                  /* P */
  int n_sources, n_channels, device;
  struct launch_order ord;     /* own stream; each launch reads the state the one before wrote */
  float *d_taps, *d_table;
  void *d_chan;                /* fmdk_tuner_chan[n_channels]: written by fmd_tuner_set_channel between launches */
  fmd_tuner_channel *chan;     /* ... as the caller set them */
  void *d_state;               /* fmd_tuner_state[n_sources]: read by the tuner kernel, advanced in place by the state kernel behind it */
  void *d_in, *d_o;            /* staging of fmd_tuner_run_host, grown on demand */
  size_t cap_blocks;
};

static hipError_t tuner_quiesce(fmd_tuner *t) { return order_quiesce(&t->ord, NULL); }

int fmd_tuner_create(fmd_tuner **out, const fmd_tuner_config *cfg, const float *taps, int n_sources, int n_channels, int device) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  int rc = fmdk_tuner_check(cfg);
  if (rc) return rc;
  if (n_sources <= 0 || n_channels <= 0) return fmd_fail(FMD_E_ARG, "n_sources and n_channels must be positive");
  float h[FMD_TUNER_MAX_TAPS];
  if (taps) {
    for (int k = 0; k < cfg->n_taps; k++) {
      if (!isfinite(taps[k])) return fmd_fail(FMD_E_ARG, "tap %d is not finite", k);
      h[k] = taps[k];
    }
  } else if ((rc = fmd_tuner_design(cfg, h))) {
    return rc;
  }
  if ((rc = open_device(&device))) return rc;

  fmd_tuner *t = (fmd_tuner *)calloc(1, sizeof(*t));
  if (!t) return fmd_fail(FMD_E_NOMEM, "out of host memory");
  t->cfg = *cfg;
  t->period = cfg->rate / cfg->step_hz;
  t->n_sources = n_sources;
  t->n_channels = n_channels;
  t->device = device;
  float *tab = (float *)malloc(sizeof(float) * 2 * (size_t)t->period);
  fmdk_tuner_chan *kc = (fmdk_tuner_chan *)calloc((size_t)n_channels, sizeof(*kc));
  t->chan = (fmd_tuner_channel *)calloc((size_t)n_channels, sizeof(*t->chan));
  if (!tab || !kc || !t->chan) { free(tab); free(kc); free(t->chan); free(t); return fmd_fail(FMD_E_NOMEM, "out of host memory"); }
  fmdk_tuner_table(t->period, tab);
  for (int c = 0; c < n_channels; c++) {                /* {source 0, shift 0, gain 1}: always in range */
    t->chan[c].gain = 1.0f;
    (void)fmdk_tuner_channel(cfg, n_sources, &t->chan[c], &kc[c]);
  }
  const size_t st_bytes = sizeof(fmd_tuner_state) * (size_t)n_sources, ch_bytes = sizeof(*kc) * (size_t)n_channels;
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&t->ord.stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&t->ord.ev_order, hipEventDisableTiming)) != hipSuccess ||
      (e = hipMalloc((void **)&t->d_taps, sizeof(float) * FMD_TUNER_MAX_TAPS)) != hipSuccess ||
      (e = hipMalloc((void **)&t->d_table, sizeof(float) * 2 * (size_t)t->period)) != hipSuccess ||
      (e = hipMalloc(&t->d_chan, ch_bytes)) != hipSuccess ||
      (e = hipMalloc(&t->d_state, st_bytes)) != hipSuccess ||
      (e = hipMemcpy(t->d_taps, h, sizeof(float) * (size_t)cfg->n_taps, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(t->d_table, tab, sizeof(float) * 2 * (size_t)t->period, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(t->d_chan, kc, ch_bytes, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemsetAsync(t->d_state, 0, st_bytes, t->ord.stream)) != hipSuccess ||
      (e = hipStreamSynchronize(t->ord.stream)) != hipSuccess) {
    free(tab);
    free(kc);
    rc = fmd_fail(FMD_E_HIP, "device setup failed: %s", hipGetErrorString(e));
    fmd_tuner_destroy(t);
    return rc;
  }
  free(tab);
  free(kc);
  *out = t;
  return FMD_OK;
}

int fmd_batch_tuner_create(fmd_tuner **out, const fmd_batch *b, int step_hz, int bw, int n_taps, int n_sources) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  if (b->r.cfg.rate_in > 0x7fffffff / 8) return fmd_fail(FMD_E_ARG, "8 x rate_in does not fit");
  const fmd_tuner_config c = {8 * b->r.cfg.rate_in, step_hz, bw, n_taps, b->r.cfg.block_len, 0};
  return fmd_tuner_create(out, &c, NULL, n_sources, b->n_streams, b->device);
}

void fmd_tuner_destroy(fmd_tuner *t) {
  if (!t) return;
  hipSetDevice(t->device);
  tuner_quiesce(t);
  if (t->d_taps) hipFree(t->d_taps);
  if (t->d_table) hipFree(t->d_table);
  if (t->d_chan) hipFree(t->d_chan);
  if (t->d_state) hipFree(t->d_state);
  if (t->d_in) hipFree(t->d_in);
  if (t->d_o) hipFree(t->d_o);
  if (t->ord.ev_order) hipEventDestroy(t->ord.ev_order);
  if (t->ord.stream) hipStreamDestroy(t->ord.stream);
  free(t->chan);
  free(t);
}

int fmd_tuner_set_channel(fmd_tuner *t, int channel, const fmd_tuner_channel *ch) {
  if (!t || !ch || channel < 0 || channel >= t->n_channels) return fmd_fail(FMD_E_ARG, "bad argument");
  fmdk_tuner_chan kc;
  const int rc = fmdk_tuner_channel(&t->cfg, t->n_sources, ch, &kc);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(t->device));
  if (t->ord.launched && t->ord.last_stream && stream_is_capturing(t->ord.last_stream))
    return fmd_fail(FMD_E_STATE, "the most recent launch's stream is being captured: set the channel before the capture or after it ends");
  HIP_TRY(tuner_quiesce(t));                            /* the most recent launch reads the table */
  HIP_TRY(hipMemcpy((char *)t->d_chan + sizeof(kc) * (size_t)channel, &kc, sizeof(kc), hipMemcpyHostToDevice));
  t->chan[channel] = *ch;
  t->chan[channel].reserved = 0;
  return FMD_OK;
}

int fmd_tuner_get_channel(fmd_tuner *t, int channel, fmd_tuner_channel *ch) {
  if (!t || !ch || channel < 0 || channel >= t->n_channels) return fmd_fail(FMD_E_ARG, "bad argument");
  *ch = t->chan[channel];
  return FMD_OK;
}

int fmd_tuner_run_device(fmd_tuner *t, const void *d_iq, int n_blocks, void *d_out, void *d_y, void *hip_stream) {
  if (!t || !d_iq || !d_out) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks < 0) return fmd_fail(FMD_E_ARG, "n_blocks < 0");
  if (n_blocks == 0) return FMD_OK;
  if (((uintptr_t)d_iq & 15) != 0 || ((uintptr_t)d_out & 15) != 0 || ((uintptr_t)d_y & 15) != 0)
    return fmd_fail(FMD_E_ARG, "d_iq, d_out and d_y must be 16-byte aligned");
  const long long L = t->cfg.block_len / 2, cpb = (L + FMDK_TUNER_CHUNK - 1) / FMDK_TUNER_CHUNK;
  if (L * n_blocks > 0x7fffffffLL - 4 * FMDK_TUNER_CHUNK)      /* (the kernel's sample index within a source's launch is 32-bit) */
    return fmd_fail(FMD_E_ARG, "n_blocks too large: block_len / 2 * n_blocks must stay below 2^31 - %d per source", 4 * FMDK_TUNER_CHUNK);
  if ((long long)t->n_channels * n_blocks * cpb > 0x7fffffffLL) return fmd_fail(FMD_E_ARG, "n_blocks too large: the grid must stay below 2^31 workgroups");
  const uintptr_t in0 = (uintptr_t)d_iq, in1 = in0 + (uintptr_t)t->n_sources * (uintptr_t)n_blocks * (uintptr_t)t->cfg.block_len;
  const uintptr_t out0 = (uintptr_t)d_out, out1 = out0 + (uintptr_t)t->n_channels * (uintptr_t)n_blocks * (uintptr_t)t->cfg.block_len;
  if (in0 < out1 && out0 < in1) return fmd_fail(FMD_E_ARG, "d_out overlaps d_iq: a workgroup reads the bytes before its chunk while another writes");
  HIP_TRY(hipSetDevice(t->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : t->ord.stream;
  const int rc = order_handover(&t->ord, st);
  if (rc > 0) return fmd_fail(FMD_E_STATE, "the previous launch ran on another stream: call fmd_tuner_sync() before capturing this one into a graph");
  if (rc) return rc;
  const int e = fmdk_tuner_launch(d_iq, t->n_sources, t->n_channels, n_blocks, &t->cfg, t->d_taps, t->d_table, t->d_chan, t->d_state, d_out, d_y, st);
  if (e) return fmd_fail(FMD_E_HIP, "tuner kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  order_launched(&t->ord, st);
  return FMD_OK;
}

int fmd_tuner_run_host(fmd_tuner *t, const uint8_t *iq, int n_blocks, uint8_t *out) {
  if (!t || !iq || !out) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks <= 0) return fmd_fail(FMD_E_ARG, "n_blocks must be positive");
  HIP_TRY(hipSetDevice(t->device));
  const size_t slot = (size_t)n_blocks * (size_t)t->cfg.block_len;
  int rc;
  if ((size_t)n_blocks > t->cap_blocks) {
    HIP_TRY(tuner_quiesce(t));
    const grow_buf v[2] = {{&t->d_in, slot * (size_t)t->n_sources, 0}, {&t->d_o, slot * (size_t)t->n_channels, 0}};
    if ((rc = grow(&t->cap_blocks, (size_t)n_blocks, v, 2))) return rc;
  }
  HIP_TRY(hipMemcpyAsync(t->d_in, iq, slot * (size_t)t->n_sources, hipMemcpyHostToDevice, t->ord.stream));
  if ((rc = fmd_tuner_run_device(t, t->d_in, n_blocks, t->d_o, NULL, NULL))) return rc;
  HIP_TRY(hipMemcpyAsync(out, t->d_o, slot * (size_t)t->n_channels, hipMemcpyDeviceToHost, t->ord.stream));
  HIP_TRY(hipStreamSynchronize(t->ord.stream));
  return FMD_OK;
}

int fmd_tuner_get_state(fmd_tuner *t, int source, fmd_tuner_state *out) {
  if (!t || !out || source < 0 || source >= t->n_sources) return fmd_fail(FMD_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(t->device));
  HIP_TRY(tuner_quiesce(t));
  HIP_TRY(hipMemcpy(out, (char *)t->d_state + sizeof(*out) * (size_t)source, sizeof(*out), hipMemcpyDeviceToHost));
  return FMD_OK;
}

int fmd_tuner_set_state(fmd_tuner *t, int source, const fmd_tuner_state *in) {
  if (!t || !in || source < 0 || source >= t->n_sources) return fmd_fail(FMD_E_ARG, "bad argument");
  if (in->count < 0 || in->count >= t->period) return fmd_fail(FMD_E_ARG, "count %d outside 0 .. %d (the table's period)", in->count, t->period - 1);
  if (in->valid != 0 && in->valid != 1) return fmd_fail(FMD_E_ARG, "valid must be 0 or 1 (got %d)", in->valid);
  HIP_TRY(hipSetDevice(t->device));
  HIP_TRY(tuner_quiesce(t));
  HIP_TRY(hipMemcpy((char *)t->d_state + sizeof(*in) * (size_t)source, in, sizeof(*in), hipMemcpyHostToDevice));
  return FMD_OK;
}

int fmd_tuner_reset(fmd_tuner *t) {
  if (!t) return fmd_fail(FMD_E_ARG, "NULL tuner object");
  HIP_TRY(hipSetDevice(t->device));
  HIP_TRY(tuner_quiesce(t));
  HIP_TRY(hipMemsetAsync(t->d_state, 0, sizeof(fmd_tuner_state) * (size_t)t->n_sources, t->ord.stream));   /* (on the own stream and waited for: see fmd_batch_reset) */
  HIP_TRY(hipStreamSynchronize(t->ord.stream));
  return FMD_OK;
}

int fmd_tuner_sync(fmd_tuner *t) {
  if (!t) return fmd_fail(FMD_E_ARG, "NULL tuner object");
  HIP_TRY(hipSetDevice(t->device));
  HIP_TRY(tuner_quiesce(t));
  return FMD_OK;
}

/* ---- station finder ---------------------------------------------------------- */
/* An object of its own (csrc/scan.inc): the range check and the plan - cmax, the floor's rank, per candidate the first bin, the bin count and the
 * two edge weights - are fmd_resolve.c's; here its device side.  The candidate table is made at create, so a launch allocates nothing and can be
 * captured.  There is no state: launches are not ordered against each other, and the launch order only remembers which stream to wait for. */

struct fmd_scan {
  fmd_scan_config cfg;
  fmdk_scan_plan plan;
  int n_streams, device;
  struct launch_order ord;     /* own stream; the stream of the most recent launch, for sync and destroy (no event: nothing is handed over) */
  void *d_cand;                /* fmdk_scan_cand[C] */
  void *d_p;                   /* staging of fmd_scan_run_host: the spectra, grown on demand ... */
  size_t cap_blocks;
  void *d_st, *d_cnt, *d_ch;   /* ... and its results, whose sizes do not depend on n_blocks: made at create */
};

static hipError_t scan_quiesce(fmd_scan *s) { return order_quiesce(&s->ord, NULL); }

int fmd_scan_create(fmd_scan **out, const fmd_scan_config *cfg, int n_streams, int device) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  fmdk_scan_plan plan;
  fmdk_scan_cand *cand = (fmdk_scan_cand *)malloc(sizeof(*cand) * FMD_SCAN_MAX_CANDIDATES);
  if (!cand) return fmd_fail(FMD_E_NOMEM, "out of host memory");
  int rc = fmdk_scan_plan_make(cfg, &plan, cand);
  if (!rc && n_streams <= 0) rc = fmd_fail(FMD_E_ARG, "n_streams must be positive");
  if (!rc) rc = open_device(&device);
  if (rc) { free(cand); return rc; }

  fmd_scan *s = (fmd_scan *)calloc(1, sizeof(*s));
  if (!s) { free(cand); return fmd_fail(FMD_E_NOMEM, "out of host memory"); }
  s->cfg = *cfg;
  s->plan = plan;
  s->n_streams = n_streams;
  s->device = device;
  const size_t cd_bytes = sizeof(*cand) * (size_t)plan.n_cand;
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&s->ord.stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipMalloc(&s->d_cand, cd_bytes)) != hipSuccess ||
      (e = hipMalloc(&s->d_st, sizeof(fmd_scan_station) * (size_t)cfg->max_stations * (size_t)n_streams)) != hipSuccess ||
      (e = hipMalloc(&s->d_cnt, sizeof(int32_t) * 2 * (size_t)n_streams)) != hipSuccess ||
      (e = hipMalloc(&s->d_ch, sizeof(float) * (size_t)plan.n_cand * (size_t)n_streams)) != hipSuccess ||
      (e = hipMemcpy(s->d_cand, cand, cd_bytes, hipMemcpyHostToDevice)) != hipSuccess) {
    free(cand);
    rc = fmd_fail(FMD_E_HIP, "device setup failed: %s", hipGetErrorString(e));
    fmd_scan_destroy(s);
    return rc;
  }
  free(cand);
  *out = s;
  return FMD_OK;
}

int fmd_batch_scan_create(fmd_scan **out, const fmd_batch *b, int n_bins, int raster_hz, int bw, int max_stations) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  if (b->r.cfg.rate_in > 0x7fffffff / 8) return fmd_fail(FMD_E_ARG, "8 x rate_in does not fit");
  const fmd_scan_config c = {8 * b->r.cfg.rate_in, n_bins, raster_hz, bw, 1, 250, 0, max_stations, 4.0f, {0, 0, 0}};
  return fmd_scan_create(out, &c, b->n_streams, b->device);
}

void fmd_scan_destroy(fmd_scan *s) {
  if (!s) return;
  hipSetDevice(s->device);
  scan_quiesce(s);
  if (s->d_cand) hipFree(s->d_cand);
  if (s->d_p) hipFree(s->d_p);
  if (s->d_st) hipFree(s->d_st);
  if (s->d_cnt) hipFree(s->d_cnt);
  if (s->d_ch) hipFree(s->d_ch);
  if (s->ord.stream) hipStreamDestroy(s->ord.stream);
  free(s);
}

int fmd_scan_run_device(fmd_scan *s, const void *d_power, int n_blocks, void *d_stations, void *d_counts, void *d_chan, void *hip_stream) {
  if (!s || !d_power || !d_stations || !d_counts) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks < 1) return fmd_fail(FMD_E_ARG, "n_blocks must be positive");
  if (((uintptr_t)d_power & 15) != 0 || ((uintptr_t)d_stations & 15) != 0 || ((uintptr_t)d_counts & 15) != 0 || ((uintptr_t)d_chan & 15) != 0)
    return fmd_fail(FMD_E_ARG, "d_power, d_stations, d_counts and d_chan must be 16-byte aligned");
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : s->ord.stream;
  /* a launch on another stream than the one before: both read the table only, so nothing is handed over; sync and destroy wait for the most recent
   * stream and the own one, the caller for their earlier streams (as for every buffer they pass) */
  const int e = fmdk_scan_launch(d_power, s->n_streams, n_blocks, &s->cfg, &s->plan, s->d_cand, d_stations, d_counts, d_chan, st);
  if (e) return fmd_fail(FMD_E_HIP, "scan kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  order_launched(&s->ord, st);
  return FMD_OK;
}

int fmd_scan_run_host(fmd_scan *s, const float *power, int n_blocks, fmd_scan_station *stations, int32_t *counts, float *chan) {
  if (!s || !power || !stations || !counts) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks < 1) return fmd_fail(FMD_E_ARG, "n_blocks must be positive");
  HIP_TRY(hipSetDevice(s->device));
  const size_t np = (size_t)s->n_streams * (size_t)n_blocks * (size_t)s->cfg.n_bins * sizeof(float);
  const size_t nst = sizeof(fmd_scan_station) * (size_t)s->cfg.max_stations * (size_t)s->n_streams;
  int rc;
  const grow_buf v = {&s->d_p, np, 0};
  /* no wait: d_p is used only on the own stream, by this call, which waits for it below */
  if ((rc = grow(&s->cap_blocks, (size_t)n_blocks, &v, 1))) return rc;
  HIP_TRY(hipMemcpyAsync(s->d_p, power, np, hipMemcpyHostToDevice, s->ord.stream));
  if ((rc = fmd_scan_run_device(s, s->d_p, n_blocks, s->d_st, s->d_cnt, chan ? s->d_ch : NULL, NULL))) return rc;
  HIP_TRY(hipMemcpyAsync(stations, s->d_st, nst, hipMemcpyDeviceToHost, s->ord.stream));
  HIP_TRY(hipMemcpyAsync(counts, s->d_cnt, sizeof(int32_t) * 2 * (size_t)s->n_streams, hipMemcpyDeviceToHost, s->ord.stream));
  if (chan) HIP_TRY(hipMemcpyAsync(chan, s->d_ch, sizeof(float) * (size_t)s->plan.n_cand * (size_t)s->n_streams, hipMemcpyDeviceToHost, s->ord.stream));
  HIP_TRY(hipStreamSynchronize(s->ord.stream));
  return FMD_OK;
}

int fmd_scan_sync(fmd_scan *s) {
  if (!s) return fmd_fail(FMD_E_ARG, "NULL scan object");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(scan_quiesce(s));
  return FMD_OK;
}

/* ---- RDS receiver ----------------------------------------------------------- */
/* An object of its own (csrc/rds.inc): range check, geometry, taps and timing table are fmd_rds.c's; here its device side.  Everything a launch of
 * up to max_blocks blocks needs - taps, table, state, the scratch for y, the chunk partials and the per-block records - is made at create. */

struct fmd_rds {
  fmd_rds_config cfg;
  fmdk_rds_geom g;
  int n_streams, device, cpb;
  struct launch_order ord;
  float *d_taps, *d_w;
  void *d_state;               /* fmd_rds_state[n_streams]: read by the first three kernels, advanced in place by the state kernel behind them */
  void *d_y, *d_part, *d_blk;  /* scratch of a launch, for max_blocks blocks per stream */
  void *d_zin, *d_soft, *d_lens, *d_first, *d_est;      /* staging of fmd_rds_run_host, made at its first use */
  int last_blocks;             /* n_blocks of the most recent launch (fmd_rds_last_y) */
};

static hipError_t rds_quiesce(fmd_rds *r) { return order_quiesce(&r->ord, NULL); }

int fmd_rds_create(fmd_rds **out, const fmd_rds_config *cfg, const float *taps, int n_streams, int device) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  int rc = fmdk_rds_check(cfg);
  if (rc) return rc;
  if (n_streams <= 0) return fmd_fail(FMD_E_ARG, "n_streams must be positive");
  const long long cpb = (cfg->block_z + FMDK_RDS_CHUNK - 1) / FMDK_RDS_CHUNK;
  if ((long long)cfg->block_z * cfg->max_blocks > 0x7fffffffLL - 2 * FMDK_RDS_CHUNK)      /* (the kernels' sample index within a stream's launch is 32-bit) */
    return fmd_fail(FMD_E_ARG, "max_blocks too large: block_z * max_blocks must stay below 2^31 - %d per stream", 2 * FMDK_RDS_CHUNK);
  if ((long long)n_streams * cfg->max_blocks * cpb > 0x7fffffffLL) return fmd_fail(FMD_E_ARG, "max_blocks too large: the grid must stay below 2^31 workgroups");
  float h[FMD_RDS_MAX_TAPS], w[2 * FMD_RDS_MAX_PERIOD];
  if (taps) {
    for (int k = 0; k < cfg->n_taps; k++) {
      if (!isfinite(taps[k])) return fmd_fail(FMD_E_ARG, "tap %d is not finite", k);
      h[k] = taps[k];
    }
  } else if ((rc = fmd_rds_design(cfg, h))) {
    return rc;
  }
  if ((rc = open_device(&device))) return rc;

  fmd_rds *r = (fmd_rds *)calloc(1, sizeof(*r));
  if (!r) return fmd_fail(FMD_E_NOMEM, "out of host memory");
  r->cfg = *cfg;
  fmdk_rds_geometry(cfg->rate_z, cfg->block_z, &r->g);
  r->n_streams = n_streams;
  r->device = device;
  r->cpb = (int)cpb;
  fmdk_rds_table(cfg, w);
  const size_t st_bytes = sizeof(fmd_rds_state) * (size_t)n_streams, slots = (size_t)n_streams * (size_t)cfg->max_blocks;
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&r->ord.stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&r->ord.ev_order, hipEventDisableTiming)) != hipSuccess ||
      (e = hipMalloc((void **)&r->d_taps, sizeof(float) * FMD_RDS_MAX_TAPS)) != hipSuccess ||
      (e = hipMalloc((void **)&r->d_w, sizeof(float) * 2 * (size_t)r->g.pw)) != hipSuccess ||
      (e = hipMalloc(&r->d_state, st_bytes)) != hipSuccess ||
      (e = hipMalloc(&r->d_y, slots * (size_t)cfg->block_z * 2 * sizeof(float))) != hipSuccess ||
      (e = hipMalloc(&r->d_part, slots * (size_t)cpb * 4 * sizeof(float))) != hipSuccess ||
      (e = hipMalloc(&r->d_blk, slots * sizeof(fmdk_rds_blk))) != hipSuccess ||
      (e = hipMemcpy(r->d_taps, h, sizeof(float) * (size_t)cfg->n_taps, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(r->d_w, w, sizeof(float) * 2 * (size_t)r->g.pw, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemsetAsync(r->d_state, 0, st_bytes, r->ord.stream)) != hipSuccess ||
      (e = hipStreamSynchronize(r->ord.stream)) != hipSuccess) {
    rc = fmd_fail(FMD_E_HIP, "device setup failed: %s", hipGetErrorString(e));
    fmd_rds_destroy(r);
    return rc;
  }
  *out = r;
  return FMD_OK;
}

int fmd_subc_rds_create(fmd_rds **out, const fmd_subc *s, int n_taps, int avg_blocks, int max_blocks) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  if (!s) return fmd_fail(FMD_E_ARG, "NULL subcarrier object");
  if (s->cfg.rate_in % s->cfg.decim) return fmd_fail(FMD_E_UNSUPPORTED, "rate_in %d is no multiple of decim %d", s->cfg.rate_in, s->cfg.decim);
  const fmd_rds_config c = {s->cfg.rate_in / s->cfg.decim, s->cfg.block_samples / s->cfg.decim, n_taps, avg_blocks, max_blocks};
  return fmd_rds_create(out, &c, NULL, s->n_streams, s->device);
}

void fmd_rds_destroy(fmd_rds *r) {
  if (!r) return;
  hipSetDevice(r->device);
  rds_quiesce(r);
  void *v[] = {r->d_taps, r->d_w, r->d_state, r->d_y, r->d_part, r->d_blk, r->d_zin, r->d_soft, r->d_lens, r->d_first, r->d_est};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++)
    if (v[i]) hipFree(v[i]);
  if (r->ord.ev_order) hipEventDestroy(r->ord.ev_order);
  if (r->ord.stream) hipStreamDestroy(r->ord.stream);
  free(r);
}

int fmd_rds_bits_per_block(const fmd_rds *r) { return r ? r->g.slot : FMD_E_ARG; }

int fmd_rds_run_device(fmd_rds *r, const void *d_z, int n_blocks, void *d_soft, void *d_lens, void *d_first, void *d_est, void *hip_stream) {
  if (!r || !d_z || !d_soft || !d_lens) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks < 0) return fmd_fail(FMD_E_ARG, "n_blocks < 0");
  if (n_blocks == 0) return FMD_OK;
  if (n_blocks > r->cfg.max_blocks) return fmd_fail(FMD_E_ARG, "n_blocks %d exceeds the object's max_blocks %d", n_blocks, r->cfg.max_blocks);
  if (((uintptr_t)d_z & 15) != 0 || ((uintptr_t)d_soft & 15) != 0 || ((uintptr_t)d_lens & 15) != 0 || ((uintptr_t)d_first & 15) != 0 || ((uintptr_t)d_est & 15) != 0)
    return fmd_fail(FMD_E_ARG, "d_z, d_soft, d_lens, d_first and d_est must be 16-byte aligned");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : r->ord.stream;
  const int rc = order_handover(&r->ord, st);
  if (rc > 0) return fmd_fail(FMD_E_STATE, "the previous launch ran on another stream: call fmd_rds_sync() before capturing this one into a graph");
  if (rc) return rc;
  const int e = fmdk_rds_launch(d_z, r->n_streams, n_blocks, &r->cfg, &r->g, r->d_taps, r->d_w, r->d_state, r->d_y, r->d_part, r->d_blk, d_soft, d_lens,
                                d_first, d_est, st);
  if (e) return fmd_fail(FMD_E_HIP, "RDS kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  order_launched(&r->ord, st);
  r->last_blocks = n_blocks;
  return FMD_OK;
}

int fmd_rds_run_host(fmd_rds *r, const float *z, int n_blocks, float *soft, int32_t *lens, int64_t *first, float *est) {
  if (!r || !z || !soft || !lens) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks <= 0 || n_blocks > r->cfg.max_blocks) return fmd_fail(FMD_E_ARG, "n_blocks must lie in 1 .. max_blocks = %d", r->cfg.max_blocks);
  HIP_TRY(hipSetDevice(r->device));
  const size_t cap = (size_t)r->n_streams * (size_t)r->cfg.max_blocks, slots = (size_t)r->n_streams * (size_t)n_blocks;
  const size_t zb = (size_t)r->cfg.block_z * 2 * sizeof(float), sb = (size_t)r->g.slot * sizeof(float);
  if (!r->d_zin) {              /* the staging, once, for max_blocks (nothing of it is in use: it is touched only here, and this call waits below) */
    hipError_t e;
    if ((e = hipMalloc(&r->d_zin, cap * zb)) != hipSuccess || (e = hipMalloc(&r->d_soft, cap * sb)) != hipSuccess ||
        (e = hipMalloc(&r->d_lens, cap * sizeof(int32_t))) != hipSuccess || (e = hipMalloc(&r->d_first, cap * sizeof(int64_t))) != hipSuccess ||
        (e = hipMalloc(&r->d_est, cap * 4 * sizeof(float))) != hipSuccess) {
      void **v[] = {&r->d_zin, &r->d_soft, &r->d_lens, &r->d_first, &r->d_est};
      for (int i = 0; i < 5; i++) { if (*v[i]) hipFree(*v[i]); *v[i] = NULL; }
      return fmd_fail(FMD_E_HIP, "staging: %s", hipGetErrorString(e));
    }
  }
  /* whatever fails below, the stream is waited for before the call returns: a copy from or into the caller's memory may already be queued */
  int rc = FMD_OK;
  hipError_t e = hipMemcpyAsync(r->d_zin, z, slots * zb, hipMemcpyHostToDevice, r->ord.stream);
  if (e == hipSuccess && (rc = fmd_rds_run_device(r, r->d_zin, n_blocks, r->d_soft, r->d_lens, r->d_first, r->d_est, NULL)) == FMD_OK) {
    e = hipMemcpyAsync(soft, r->d_soft, slots * sb, hipMemcpyDeviceToHost, r->ord.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(lens, r->d_lens, slots * sizeof(int32_t), hipMemcpyDeviceToHost, r->ord.stream);
    if (e == hipSuccess && first) e = hipMemcpyAsync(first, r->d_first, slots * sizeof(int64_t), hipMemcpyDeviceToHost, r->ord.stream);
    if (e == hipSuccess && est) e = hipMemcpyAsync(est, r->d_est, slots * 4 * sizeof(float), hipMemcpyDeviceToHost, r->ord.stream);
  }
  const hipError_t w = hipStreamSynchronize(r->ord.stream);
  if (rc) return rc;                                     /* (fmd_last_error's text is the launch's) */
  if (e != hipSuccess || w != hipSuccess) return fmd_fail(FMD_E_HIP, "fmd_rds_run_host: %s", hipGetErrorString(e != hipSuccess ? e : w));
  return FMD_OK;
}

int fmd_rds_last_y(fmd_rds *r, int n_blocks, float *y, float *tm) {
  if (!r || (!y && !tm)) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks <= 0 || n_blocks != r->last_blocks) return fmd_fail(FMD_E_STATE, "the most recent launch had %d blocks, not %d", r->last_blocks, n_blocks);
  HIP_TRY(hipSetDevice(r->device));
  HIP_TRY(rds_quiesce(r));
  const size_t slots = (size_t)r->n_streams * (size_t)n_blocks;
  if (y) HIP_TRY(hipMemcpy(y, r->d_y, slots * (size_t)r->cfg.block_z * 2 * sizeof(float), hipMemcpyDeviceToHost));
  if (tm) {
    fmdk_rds_blk *h = (fmdk_rds_blk *)malloc(slots * sizeof(*h));
    if (!h) return fmd_fail(FMD_E_NOMEM, "out of host memory");
    const hipError_t e = hipMemcpy(h, r->d_blk, slots * sizeof(*h), hipMemcpyDeviceToHost);
    for (size_t i = 0; e == hipSuccess && i < slots; i++) { tm[2 * i] = h[i].tm[0]; tm[2 * i + 1] = h[i].tm[1]; }
    free(h);
    if (e != hipSuccess) return fmd_fail(FMD_E_HIP, "fmd_rds_last_y: %s", hipGetErrorString(e));
  }
  return FMD_OK;
}

int fmd_rds_get_state(fmd_rds *r, int stream, fmd_rds_state *out) {
  if (!r || !out || stream < 0 || stream >= r->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(r->device));
  HIP_TRY(rds_quiesce(r));
  HIP_TRY(hipMemcpy(out, (char *)r->d_state + sizeof(*out) * (size_t)stream, sizeof(*out), hipMemcpyDeviceToHost));
  return FMD_OK;
}

int fmd_rds_set_state(fmd_rds *r, int stream, const fmd_rds_state *in) {
  if (!r || !in || stream < 0 || stream >= r->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  if (in->phase < 0 || in->phase >= r->g.pw) return fmd_fail(FMD_E_ARG, "phase %d outside 0 .. %d (the timing table's period)", in->phase, r->g.pw - 1);
  const int lo = -FMDK_RDS_Q * r->g.lb;
  if (in->frac < lo || in->frac >= lo + r->g.two_rz) return fmd_fail(FMD_E_ARG, "frac %d outside %d .. %d", in->frac, lo, lo + r->g.two_rz - 1);
  if (in->bit < 0) return fmd_fail(FMD_E_ARG, "bit index is negative");
  HIP_TRY(hipSetDevice(r->device));
  HIP_TRY(rds_quiesce(r));
  HIP_TRY(hipMemcpy((char *)r->d_state + sizeof(*in) * (size_t)stream, in, sizeof(*in), hipMemcpyHostToDevice));
  return FMD_OK;
}

int fmd_rds_reset(fmd_rds *r) {
  if (!r) return fmd_fail(FMD_E_ARG, "NULL RDS object");
  HIP_TRY(hipSetDevice(r->device));
  HIP_TRY(rds_quiesce(r));
  HIP_TRY(hipMemsetAsync(r->d_state, 0, sizeof(fmd_rds_state) * (size_t)r->n_streams, r->ord.stream));
  HIP_TRY(hipStreamSynchronize(r->ord.stream));
  return FMD_OK;
}

int fmd_rds_sync(fmd_rds *r) {
  if (!r) return fmd_fail(FMD_E_ARG, "NULL RDS object");
  HIP_TRY(hipSetDevice(r->device));
  HIP_TRY(rds_quiesce(r));
  return FMD_OK;
}

int fmd_batch_get_state(fmd_batch *b, int stream, fmd_stream_state *out) {
  if (!b || !out || stream < 0 || stream >= b->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(batch_quiesce(b));
  HIP_TRY(hipMemcpy(out, (char *)b->d_state[b->cur] + sizeof(*out) * (size_t)stream, sizeof(*out), hipMemcpyDeviceToHost));
  return FMD_OK;
}

int fmd_batch_set_state(fmd_batch *b, int stream, const fmd_stream_state *in) {
  if (!b || !in || stream < 0 || stream >= b->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(batch_quiesce(b));
  HIP_TRY(hipMemcpy((char *)b->d_state[b->cur] + sizeof(*in) * (size_t)stream, in, sizeof(*in), hipMemcpyHostToDevice));
  return FMD_OK;
}

int fmd_batch_reset(fmd_batch *b) {
  if (!b) return fmd_fail(FMD_E_ARG, "NULL batch");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(batch_quiesce(b));
  /* on the batch's own stream and waited for: hipMemset on device memory may return before the fill has run, and the
   * batch's stream (non-blocking) does not order itself behind the null stream */
  HIP_TRY(hipMemsetAsync(b->d_state[b->cur], 0, sizeof(fmd_stream_state) * (size_t)b->n_streams, b->ord.stream));
  HIP_TRY(hipStreamSynchronize(b->ord.stream));
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

  if (hipSetDevice(b->device) != hipSuccess) { fmd_fail(FMD_E_HIP, "hipSetDevice failed"); DIE(d, "full_demod"); }
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
    if (batch_quiesce(b) != hipSuccess) { fmd_fail(FMD_E_HIP, "device busy"); DIE(d, "full_demod"); }
    di->pin->st = st;
    e = hipMemcpyAsync(b->d_state[b->cur], &di->pin->st, sizeof(st), hipMemcpyHostToDevice, b->ord.stream);
    if (e != hipSuccess) { fmd_fail(FMD_E_HIP, "state upload: %s", hipGetErrorString(e)); DIE(d, "full_demod"); }
    if (hipStreamSynchronize(b->ord.stream) != hipSuccess) { fmd_fail(FMD_E_HIP, "state upload"); DIE(d, "full_demod"); }   /* pin->st is reused below */
  }
  e = hipMemcpyAsync(b->d_iq, d->buf, (size_t)d->buf_len, hipMemcpyHostToDevice, b->ord.stream);
  if (e != hipSuccess) { fmd_fail(FMD_E_HIP, "IQ upload: %s", hipGetErrorString(e)); DIE(d, "full_demod"); }
  if (fmd_batch_run_device(b, b->d_iq, 1, b->d_pcm, b->d_lens, NULL)) DIE(d, "full_demod: run");
  if ((e = hipMemcpyAsync(di->pin->pcm, b->d_pcm, sizeof(int16_t) * (size_t)b->r.pcm_stride, hipMemcpyDeviceToHost, b->ord.stream)) != hipSuccess ||
      (e = hipMemcpyAsync(&di->pin->len, b->d_lens, sizeof(int32_t), hipMemcpyDeviceToHost, b->ord.stream)) != hipSuccess ||
      (e = hipMemcpyAsync(&di->pin->st, b->d_state[b->cur], sizeof(st), hipMemcpyDeviceToHost, b->ord.stream)) != hipSuccess ||
      (e = hipStreamSynchronize(b->ord.stream)) != hipSuccess) {                       /* the one wait of the block */
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
    if (hipSetDevice(b->device) != hipSuccess) return fmd_fail(FMD_E_HIP, "hipSetDevice(%d) failed", b->device);
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
      hipSetDevice(b->device);
      batch_quiesce(b);
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
  return grow(&p->cap_blocks, (size_t)nb, v, 5);
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
  HIP_TRY(hipSetDevice(b->device));
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
  if (!b->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&b->copy_stream, hipStreamNonBlocking));
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
    e = hipMemcpyAsync(dst, ring + from, first, hipMemcpyHostToDevice, b->copy_stream);
    if (e == hipSuccess && take > first) e = hipMemcpyAsync(dst + first, ring, take - first, hipMemcpyHostToDevice, b->copy_stream);
  }
  const size_t slots = (size_t)b->n_streams * (size_t)nb;
  if (e == hipSuccess) e = hipEventRecord(p->h2d_done, b->copy_stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(b->ord.stream, p->h2d_done, 0);
  int launched = 0;
  if (e == hipSuccess) {
    rc = fmd_batch_run_device(b, p->d_iq, nb, p->d_pcm, p->d_lens, NULL);
    if (rc == FMD_OK) {
      launched = 1;                                    /* the streams' state has advanced by nb blocks from here on */
      e = hipMemcpyAsync(p->h_pcm, p->d_pcm, slots * (size_t)b->r.pcm_stride * sizeof(int16_t), hipMemcpyDeviceToHost, b->ord.stream);
      if (e == hipSuccess) e = hipMemcpyAsync(p->h_lens, p->d_lens, slots * sizeof(int32_t), hipMemcpyDeviceToHost, b->ord.stream);
      if (e == hipSuccess) e = hipEventRecord(p->done, b->ord.stream);
    }
  }
  if (!launched) {
    /* nothing has been demodulated: give the bytes back.  Wait for the copies already queued, then un-take them (they are still in the rings, so the
     * next call sees them again); a part an overflow has meanwhile released (moved from inflight to debt) is not taken back a second time:
     * fmdk_ring_untake says whose bytes the debt is - the other job's first, if it still holds ring space */
    hipStreamSynchronize(b->copy_stream);
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
  HIP_TRY(hipSetDevice(b->device));
  if (p->failed) {
    /* the job ran (state advanced) but its PCM never left the device: wait for the kernel, free the slot and the ring space, report */
    const int err = p->failed;
    hipStreamSynchronize(b->ord.stream);
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
