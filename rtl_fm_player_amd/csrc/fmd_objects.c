/*
 * fmd_objects.c - the receiver objects beside the batch: MPX subcarrier receiver (fmd_subc_*), channel tuner (fmd_tuner_*), station finder
 * (fmd_scan_*), stereo control (fmd_stereo_*) and RDS receiver (fmd_rds_*): create / destroy, launches, host forms and state access, each on the core
 * of fmd_dev.h (device, own stream, launch order, carried state, owned buffers).  What needs no device is fmd_recv.c's and fmd_rds.c's; the four
 * constructors that read a batch (fmd_batch_subc_create, _tuner_create, _scan_create, _stereo_create) are fmd_host.c's.
 */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdlib.h>

#include "fmd_dev.h"

/* ---- MPX subcarrier receiver ------------------------------------------------ */
/* An object of its own (csrc/subcarrier.inc): configuration check, tap design and carrier table are fmd_recv.c's; here its device side.  Everything
 * a launch needs - taps, table, state - is made at create, so a launch allocates nothing and can be captured into a graph. */

struct fmd_subc {
  struct fmdh_obj o;           /* its state: fmd_subc_state[n_streams] */
  fmd_subc_config cfg;
  int period;                  /* Pd */
  int n_streams;
  float *d_taps, *d_carrier;
  void *d_v, *d_z;             /* staging of fmd_subc_run_host, grown on demand */
  size_t cap_blocks;
};

int fmd_subc_create(fmd_subc **out, const fmd_subc_config *cfg, const float *taps, int n_streams, int device) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  int rc = fmdk_subc_check(cfg);
  if (rc) return rc;
  if (n_streams <= 0) return fmd_fail(FMD_E_ARG, "n_streams must be positive");
  float h[FMD_SUBC_MAX_TAPS];
  if ((rc = taps ? fmdh_copy_taps(h, taps, cfg->n_taps) : fmd_subc_design(cfg, h))) return rc;

  fmd_subc *s = (fmd_subc *)calloc(1, sizeof(*s));
  if (!s) return fmd_fail(FMD_E_NOMEM, "out of host memory");
  s->cfg = *cfg;
  s->period = fmdk_subc_period(cfg);
  s->n_streams = n_streams;
  const size_t car_bytes = sizeof(float) * 2 * (size_t)s->period;
  float *car = (float *)malloc(car_bytes);
  if (!car) { free(s); return fmd_fail(FMD_E_NOMEM, "out of host memory"); }
  fmdk_subc_carrier(cfg, car);
  (void)((rc = fmdh_obj_open(&s->o, device, sizeof(fmd_subc_state), n_streams, 1)) ||
         (rc = fmdh_obj_alloc(&s->o, (void **)&s->d_taps, sizeof(float) * FMD_SUBC_MAX_TAPS, h, sizeof(float) * (size_t)cfg->n_taps)) ||
         (rc = fmdh_obj_alloc(&s->o, (void **)&s->d_carrier, car_bytes, car, car_bytes)));
  fmdh_obj_own(&s->o, &s->d_v);
  fmdh_obj_own(&s->o, &s->d_z);
  free(car);
  if (rc) { fmd_subc_destroy(s); return rc; }
  *out = s;
  return FMD_OK;
}

void fmd_subc_destroy(fmd_subc *s) {
  if (!s) return;
  fmdh_obj_close(&s->o);
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
  hipStream_t st;
  const int rc = fmdh_obj_launch_begin(&s->o, hip_stream, "fmd_subc_sync", &st);
  if (rc) return rc;
  const int e = fmdk_subc_launch(d_v, s->n_streams, n_blocks, &s->cfg, s->period, s->d_taps, s->d_carrier, s->o.d_state, d_z, st);
  if (e) return fmd_fail(FMD_E_HIP, "subcarrier kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  fmdh_order_launched(&s->o.ord, st);
  return FMD_OK;
}

int fmd_subc_run_host(fmd_subc *s, const float *v, int n_blocks, float *z) {
  if (!s || !v || !z) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks <= 0) return fmd_fail(FMD_E_ARG, "n_blocks must be positive");
  HIP_TRY(hipSetDevice(s->o.device));
  const size_t slots = (size_t)s->n_streams * (size_t)n_blocks, M = (size_t)s->cfg.block_samples, nz = 2 * (M / (size_t)s->cfg.decim);
  int rc;
  if ((size_t)n_blocks > s->cap_blocks) {
    const grow_buf g[2] = {{&s->d_v, slots * M * sizeof(float), 0}, {&s->d_z, slots * nz * sizeof(float), 0}};
    if ((rc = fmdh_obj_sync(&s->o)) || (rc = fmdh_grow(&s->cap_blocks, (size_t)n_blocks, g, 2))) return rc;
  }
  const hipStream_t st = s->o.ord.stream;
  rc = fmdh_host_copy(FMD_OK, __func__, st, s->d_v, v, slots * M * sizeof(float), hipMemcpyHostToDevice);
  if (!rc) rc = fmd_subc_run_device(s, s->d_v, n_blocks, s->d_z, NULL);
  rc = fmdh_host_copy(rc, __func__, st, z, s->d_z, slots * nz * sizeof(float), hipMemcpyDeviceToHost);
  return fmdh_host_wait(rc, __func__, st);
}

int fmd_subc_get_state(fmd_subc *s, int stream, fmd_subc_state *out) {
  if (!s || !out || stream < 0 || stream >= s->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  return fmdh_obj_get_state(&s->o, stream, out);
}

int fmd_subc_set_state(fmd_subc *s, int stream, const fmd_subc_state *in) {
  if (!s || !in || stream < 0 || stream >= s->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  if (in->phase < 0 || in->phase >= s->period) return fmd_fail(FMD_E_ARG, "phase %d outside 0 .. %d (the carrier's period)", in->phase, s->period - 1);
  return fmdh_obj_set_state(&s->o, stream, in);
}

int fmd_subc_reset(fmd_subc *s) {
  if (!s) return fmd_fail(FMD_E_ARG, "NULL subcarrier object");
  return fmdh_obj_reset(&s->o);
}

int fmd_subc_sync(fmd_subc *s) {
  if (!s) return fmd_fail(FMD_E_ARG, "NULL subcarrier object");
  return fmdh_obj_sync(&s->o);
}

/* ---- channel tuner ---------------------------------------------------------- */
/* An object of its own (csrc/tuner.inc): range checks, tap design, carrier table and the channel table's entries are fmd_recv.c's; here its device
 * side.  Everything a launch needs - taps, table, channel table, state - is made at create, so a launch allocates nothing and can be captured. */

struct fmd_tuner {
  struct fmdh_obj o;           /* its state: fmd_tuner_state[n_sources] */
  fmd_tuner_config cfg;
  int period;                  /* P */
  int n_sources, n_channels;
  float *d_taps, *d_table;
  void *d_chan;                /* fmdk_tuner_chan[n_channels]: written by fmd_tuner_set_channel between launches */
  fmd_tuner_channel *chan;     /* ... as the caller set them */
  void *d_in, *d_o;            /* staging of fmd_tuner_run_host, grown on demand */
  size_t cap_blocks;
};

int fmd_tuner_create(fmd_tuner **out, const fmd_tuner_config *cfg, const float *taps, int n_sources, int n_channels, int device) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  int rc = fmdk_tuner_check(cfg);
  if (rc) return rc;
  if (n_sources <= 0 || n_channels <= 0) return fmd_fail(FMD_E_ARG, "n_sources and n_channels must be positive");
  float h[FMD_TUNER_MAX_TAPS];
  if ((rc = taps ? fmdh_copy_taps(h, taps, cfg->n_taps) : fmd_tuner_design(cfg, h))) return rc;

  fmd_tuner *t = (fmd_tuner *)calloc(1, sizeof(*t));
  if (!t) return fmd_fail(FMD_E_NOMEM, "out of host memory");
  t->cfg = *cfg;
  t->period = cfg->rate / cfg->step_hz;
  t->n_sources = n_sources;
  t->n_channels = n_channels;
  const size_t tab_bytes = sizeof(float) * 2 * (size_t)t->period, ch_bytes = sizeof(fmdk_tuner_chan) * (size_t)n_channels;
  float *tab = (float *)malloc(tab_bytes);
  fmdk_tuner_chan *kc = (fmdk_tuner_chan *)calloc((size_t)n_channels, sizeof(*kc));
  t->chan = (fmd_tuner_channel *)calloc((size_t)n_channels, sizeof(*t->chan));
  if (!tab || !kc || !t->chan) { free(tab); free(kc); fmd_tuner_destroy(t); return fmd_fail(FMD_E_NOMEM, "out of host memory"); }
  fmdk_tuner_table(t->period, tab);
  for (int c = 0; c < n_channels; c++) {                /* {source 0, shift 0, gain 1}: always in range */
    t->chan[c].gain = 1.0f;
    (void)fmdk_tuner_channel(cfg, n_sources, &t->chan[c], &kc[c]);
  }
  (void)((rc = fmdh_obj_open(&t->o, device, sizeof(fmd_tuner_state), n_sources, 1)) ||
         (rc = fmdh_obj_alloc(&t->o, (void **)&t->d_taps, sizeof(float) * FMD_TUNER_MAX_TAPS, h, sizeof(float) * (size_t)cfg->n_taps)) ||
         (rc = fmdh_obj_alloc(&t->o, (void **)&t->d_table, tab_bytes, tab, tab_bytes)) ||
         (rc = fmdh_obj_alloc(&t->o, &t->d_chan, ch_bytes, kc, ch_bytes)));
  fmdh_obj_own(&t->o, &t->d_in);
  fmdh_obj_own(&t->o, &t->d_o);
  free(tab);
  free(kc);
  if (rc) { fmd_tuner_destroy(t); return rc; }
  *out = t;
  return FMD_OK;
}

void fmd_tuner_destroy(fmd_tuner *t) {
  if (!t) return;
  fmdh_obj_close(&t->o);
  free(t->chan);
  free(t);
}

int fmd_tuner_set_channel(fmd_tuner *t, int channel, const fmd_tuner_channel *ch) {
  if (!t || !ch || channel < 0 || channel >= t->n_channels) return fmd_fail(FMD_E_ARG, "bad argument");
  fmdk_tuner_chan kc;
  const int rc = fmdk_tuner_channel(&t->cfg, t->n_sources, ch, &kc);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(t->o.device));
  if (t->o.ord.launched && t->o.ord.last_stream && fmdh_stream_is_capturing(t->o.ord.last_stream))
    return fmd_fail(FMD_E_STATE, "the most recent launch's stream is being captured: set the channel before the capture or after it ends");
  HIP_TRY(fmdh_order_quiesce(&t->o.ord, NULL));         /* the most recent launch reads the table */
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
  hipStream_t st;
  const int rc = fmdh_obj_launch_begin(&t->o, hip_stream, "fmd_tuner_sync", &st);
  if (rc) return rc;
  const int e = fmdk_tuner_launch(d_iq, t->n_sources, t->n_channels, n_blocks, &t->cfg, t->d_taps, t->d_table, t->d_chan, t->o.d_state, d_out, d_y, st);
  if (e) return fmd_fail(FMD_E_HIP, "tuner kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  fmdh_order_launched(&t->o.ord, st);
  return FMD_OK;
}

int fmd_tuner_run_host(fmd_tuner *t, const uint8_t *iq, int n_blocks, uint8_t *out) {
  if (!t || !iq || !out) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks <= 0) return fmd_fail(FMD_E_ARG, "n_blocks must be positive");
  HIP_TRY(hipSetDevice(t->o.device));
  const size_t slot = (size_t)n_blocks * (size_t)t->cfg.block_len;
  int rc;
  if ((size_t)n_blocks > t->cap_blocks) {
    const grow_buf g[2] = {{&t->d_in, slot * (size_t)t->n_sources, 0}, {&t->d_o, slot * (size_t)t->n_channels, 0}};
    if ((rc = fmdh_obj_sync(&t->o)) || (rc = fmdh_grow(&t->cap_blocks, (size_t)n_blocks, g, 2))) return rc;
  }
  const hipStream_t st = t->o.ord.stream;
  rc = fmdh_host_copy(FMD_OK, __func__, st, t->d_in, iq, slot * (size_t)t->n_sources, hipMemcpyHostToDevice);
  if (!rc) rc = fmd_tuner_run_device(t, t->d_in, n_blocks, t->d_o, NULL, NULL);
  rc = fmdh_host_copy(rc, __func__, st, out, t->d_o, slot * (size_t)t->n_channels, hipMemcpyDeviceToHost);
  return fmdh_host_wait(rc, __func__, st);
}

int fmd_tuner_get_state(fmd_tuner *t, int source, fmd_tuner_state *out) {
  if (!t || !out || source < 0 || source >= t->n_sources) return fmd_fail(FMD_E_ARG, "bad argument");
  return fmdh_obj_get_state(&t->o, source, out);
}

int fmd_tuner_set_state(fmd_tuner *t, int source, const fmd_tuner_state *in) {
  if (!t || !in || source < 0 || source >= t->n_sources) return fmd_fail(FMD_E_ARG, "bad argument");
  if (in->count < 0 || in->count >= t->period) return fmd_fail(FMD_E_ARG, "count %d outside 0 .. %d (the table's period)", in->count, t->period - 1);
  if (in->valid != 0 && in->valid != 1) return fmd_fail(FMD_E_ARG, "valid must be 0 or 1 (got %d)", in->valid);
  return fmdh_obj_set_state(&t->o, source, in);
}

int fmd_tuner_reset(fmd_tuner *t) {
  if (!t) return fmd_fail(FMD_E_ARG, "NULL tuner object");
  return fmdh_obj_reset(&t->o);
}

int fmd_tuner_sync(fmd_tuner *t) {
  if (!t) return fmd_fail(FMD_E_ARG, "NULL tuner object");
  return fmdh_obj_sync(&t->o);
}

/* ---- station finder ---------------------------------------------------------- */
/* An object of its own (csrc/scan.inc): the range check and the plan - cmax, the floor's rank, per candidate the first bin, the bin count and the
 * two edge weights - are fmd_recv.c's; here its device side.  The candidate table is made at create, so a launch allocates nothing and can be
 * captured.  There is no state: launches are not ordered against each other, and the launch order only remembers which stream to wait for. */

struct fmd_scan {
  struct fmdh_obj o;           /* no state and no event (nothing is handed over): the own stream, and the stream of the most recent launch for sync and destroy */
  fmd_scan_config cfg;
  fmdk_scan_plan plan;
  int n_streams;
  void *d_cand;                /* fmdk_scan_cand[C] */
  void *d_p;                   /* staging of fmd_scan_run_host: the spectra, grown on demand ... */
  size_t cap_blocks;
  void *d_st, *d_cnt, *d_ch;   /* ... and its results, whose sizes do not depend on n_blocks: made at create */
};

int fmd_scan_create(fmd_scan **out, const fmd_scan_config *cfg, int n_streams, int device) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  fmdk_scan_cand *cand = (fmdk_scan_cand *)malloc(sizeof(*cand) * FMD_SCAN_MAX_CANDIDATES);
  fmd_scan *s = (fmd_scan *)calloc(1, sizeof(*s));
  if (!cand || !s) { free(cand); free(s); return fmd_fail(FMD_E_NOMEM, "out of host memory"); }
  int rc = fmdk_scan_plan_make(cfg, &s->plan, cand);
  if (!rc && n_streams <= 0) rc = fmd_fail(FMD_E_ARG, "n_streams must be positive");
  if (!rc) {
    s->cfg = *cfg;
    s->n_streams = n_streams;
    const size_t cd_bytes = sizeof(*cand) * (size_t)s->plan.n_cand;
    (void)((rc = fmdh_obj_open(&s->o, device, 0, 0, 0)) ||
           (rc = fmdh_obj_alloc(&s->o, &s->d_cand, cd_bytes, cand, cd_bytes)) ||
           (rc = fmdh_obj_alloc(&s->o, &s->d_st, sizeof(fmd_scan_station) * (size_t)cfg->max_stations * (size_t)n_streams, NULL, 0)) ||
           (rc = fmdh_obj_alloc(&s->o, &s->d_cnt, sizeof(int32_t) * 2 * (size_t)n_streams, NULL, 0)) ||
           (rc = fmdh_obj_alloc(&s->o, &s->d_ch, sizeof(float) * (size_t)s->plan.n_cand * (size_t)n_streams, NULL, 0)));
    fmdh_obj_own(&s->o, &s->d_p);
  }
  free(cand);
  if (rc) { fmd_scan_destroy(s); return rc; }
  *out = s;
  return FMD_OK;
}

void fmd_scan_destroy(fmd_scan *s) {
  if (!s) return;
  fmdh_obj_close(&s->o);
  free(s);
}

int fmd_scan_run_device(fmd_scan *s, const void *d_power, int n_blocks, void *d_stations, void *d_counts, void *d_chan, void *hip_stream) {
  if (!s || !d_power || !d_stations || !d_counts) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks < 1) return fmd_fail(FMD_E_ARG, "n_blocks must be positive");
  if (((uintptr_t)d_power & 15) != 0 || ((uintptr_t)d_stations & 15) != 0 || ((uintptr_t)d_counts & 15) != 0 || ((uintptr_t)d_chan & 15) != 0)
    return fmd_fail(FMD_E_ARG, "d_power, d_stations, d_counts and d_chan must be 16-byte aligned");
  HIP_TRY(hipSetDevice(s->o.device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : s->o.ord.stream;
  /* a launch on another stream than the one before: both read the table only, so nothing is handed over; sync and destroy wait for the most recent
   * stream and the own one, the caller for their earlier streams (as for every buffer they pass) */
  const int e = fmdk_scan_launch(d_power, s->n_streams, n_blocks, &s->cfg, &s->plan, s->d_cand, d_stations, d_counts, d_chan, st);
  if (e) return fmd_fail(FMD_E_HIP, "scan kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  fmdh_order_launched(&s->o.ord, st);
  return FMD_OK;
}

int fmd_scan_run_host(fmd_scan *s, const float *power, int n_blocks, fmd_scan_station *stations, int32_t *counts, float *chan) {
  if (!s || !power || !stations || !counts) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks < 1) return fmd_fail(FMD_E_ARG, "n_blocks must be positive");
  HIP_TRY(hipSetDevice(s->o.device));
  const size_t np = (size_t)s->n_streams * (size_t)n_blocks * (size_t)s->cfg.n_bins * sizeof(float);
  const size_t nst = sizeof(fmd_scan_station) * (size_t)s->cfg.max_stations * (size_t)s->n_streams;
  const grow_buf g = {&s->d_p, np, 0};
  /* no wait: d_p is used only on the own stream, by this call, which waits for it below */
  int rc = fmdh_grow(&s->cap_blocks, (size_t)n_blocks, &g, 1);
  if (rc) return rc;
  const hipStream_t st = s->o.ord.stream;
  rc = fmdh_host_copy(FMD_OK, __func__, st, s->d_p, power, np, hipMemcpyHostToDevice);
  if (!rc) rc = fmd_scan_run_device(s, s->d_p, n_blocks, s->d_st, s->d_cnt, chan ? s->d_ch : NULL, NULL);
  rc = fmdh_host_copy(rc, __func__, st, stations, s->d_st, nst, hipMemcpyDeviceToHost);
  rc = fmdh_host_copy(rc, __func__, st, counts, s->d_cnt, sizeof(int32_t) * 2 * (size_t)s->n_streams, hipMemcpyDeviceToHost);
  if (chan) rc = fmdh_host_copy(rc, __func__, st, chan, s->d_ch, sizeof(float) * (size_t)s->plan.n_cand * (size_t)s->n_streams, hipMemcpyDeviceToHost);
  return fmdh_host_wait(rc, __func__, st);
}

int fmd_scan_sync(fmd_scan *s) {
  if (!s) return fmd_fail(FMD_E_ARG, "NULL scan object");
  return fmdh_obj_sync(&s->o);
}

/* ---- stereo control ---------------------------------------------------------- */
/* An object of its own (csrc/stereo.inc): the range check and the four derived floats are fmd_recv.c's; here its device side.  The state is all
 * a launch needs beside its arguments, so a launch allocates nothing and can be captured.  The mode is the host's and travels as a launch argument. */

struct fmd_stereo {
  struct fmdh_obj o;           /* its state: fmd_stereo_state[n_streams] */
  fmd_stereo_config cfg;
  fmdk_stereo_k k;
  int n_streams, mode;
  void *d_pcm, *d_lens, *d_z, *d_q, *d_info, *d_meter;   /* staging of fmd_stereo_run_host, grown on demand (the PCM is rewritten in place) */
  size_t cap_blocks;
};

int fmd_stereo_create(fmd_stereo **out, const fmd_stereo_config *cfg, int n_streams, int device) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  fmdk_stereo_k k;
  int rc = fmdk_stereo_plan(cfg, &k);
  if (rc) return rc;
  if (n_streams <= 0) return fmd_fail(FMD_E_ARG, "n_streams must be positive");
  fmd_stereo *s = (fmd_stereo *)calloc(1, sizeof(*s));
  if (!s) return fmd_fail(FMD_E_NOMEM, "out of host memory");
  s->cfg = *cfg;
  s->k = k;
  s->n_streams = n_streams;
  s->mode = FMD_STEREO_AUTO;
  rc = fmdh_obj_open(&s->o, device, sizeof(fmd_stereo_state), n_streams, 1);
  void **const staging[] = {&s->d_pcm, &s->d_lens, &s->d_z, &s->d_q, &s->d_info, &s->d_meter};
  for (int i = 0; i < 6; i++) fmdh_obj_own(&s->o, staging[i]);
  if (rc) { fmd_stereo_destroy(s); return rc; }
  *out = s;
  return FMD_OK;
}

void fmd_stereo_destroy(fmd_stereo *s) {
  if (!s) return;
  fmdh_obj_close(&s->o);
  free(s);
}

int fmd_stereo_set_mode(fmd_stereo *s, int mode) {
  if (!s) return fmd_fail(FMD_E_ARG, "NULL stereo object");
  if (mode != FMD_STEREO_AUTO && mode != FMD_STEREO_FORCE_MONO && mode != FMD_STEREO_FORCE_STEREO)
    return fmd_fail(FMD_E_ARG, "mode must be FMD_STEREO_AUTO, _FORCE_MONO or _FORCE_STEREO (got %d)", mode);
  s->mode = mode;
  return FMD_OK;
}

int fmd_stereo_run_device(fmd_stereo *s, const void *d_pcm, const void *d_lens, const void *d_z, const void *d_quality, int n_blocks, void *d_out,
                          void *d_info, void *d_meter, void *hip_stream) {
  if (!s || !d_pcm || !d_lens || !d_out || !d_info) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks < 0) return fmd_fail(FMD_E_ARG, "n_blocks < 0");
  if (s->mode == FMD_STEREO_AUTO && (!d_z || s->cfg.pilot_per_block == 0))
    return fmd_fail(FMD_E_ARG, "FMD_STEREO_AUTO needs the pilot: d_z is NULL or pilot_per_block is 0 (fmd_stereo_set_mode forces mono or stereo)");
  if (n_blocks == 0) return FMD_OK;
  if ((((uintptr_t)d_pcm | (uintptr_t)d_lens | (uintptr_t)d_z | (uintptr_t)d_quality | (uintptr_t)d_out | (uintptr_t)d_info | (uintptr_t)d_meter) & 15) != 0)
    return fmd_fail(FMD_E_ARG, "d_pcm, d_lens, d_z, d_quality, d_out, d_info and d_meter must be 16-byte aligned");
  if ((long long)s->n_streams * n_blocks > 0x7fffffffLL) return fmd_fail(FMD_E_ARG, "n_blocks too large: the grid must stay below 2^31 workgroups");
  const uintptr_t bytes = (uintptr_t)s->n_streams * (uintptr_t)n_blocks * (uintptr_t)s->cfg.pcm_stride * sizeof(int16_t);
  const uintptr_t in0 = (uintptr_t)d_pcm, out0 = (uintptr_t)d_out;
  if (in0 != out0 && in0 < out0 + bytes && out0 < in0 + bytes)
    return fmd_fail(FMD_E_ARG, "d_out overlaps d_pcm without being d_pcm: a workgroup would read what another has rewritten");
  hipStream_t st;
  const int rc = fmdh_obj_launch_begin(&s->o, hip_stream, "fmd_stereo_sync", &st);
  if (rc) return rc;
  const int e = fmdk_stereo_launch(d_pcm, d_lens, d_z, d_quality, s->n_streams, n_blocks, &s->cfg, &s->k, s->mode, s->o.d_state, d_out, d_info, d_meter, st);
  if (e) return fmd_fail(FMD_E_HIP, "stereo kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  fmdh_order_launched(&s->o.ord, st);
  return FMD_OK;
}

int fmd_stereo_run_host(fmd_stereo *s, const int16_t *pcm, const int32_t *lens, const float *z, const float *quality, int n_blocks, int16_t *out,
                        fmd_stereo_info *info, fmd_stereo_meter *meter) {
  if (!s || !pcm || !lens || !out || !info) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks <= 0) return fmd_fail(FMD_E_ARG, "n_blocks must be positive");
  HIP_TRY(hipSetDevice(s->o.device));
  const size_t slots = (size_t)s->n_streams * (size_t)n_blocks, pb = slots * (size_t)s->cfg.pcm_stride * sizeof(int16_t);
  const size_t zb = slots * (size_t)s->cfg.pilot_per_block * 2 * sizeof(float);
  const int with_z = z && zb;
  int rc;
  if ((size_t)n_blocks > s->cap_blocks) {
    const grow_buf g[6] = {{&s->d_pcm, pb, 0}, {&s->d_lens, slots * sizeof(int32_t), 0}, {&s->d_z, zb ? zb : 16, 0}, {&s->d_q, slots * sizeof(float), 0},
                           {&s->d_info, slots * sizeof(fmd_stereo_info), 0}, {&s->d_meter, slots * sizeof(fmd_stereo_meter), 0}};
    if ((rc = fmdh_obj_sync(&s->o)) || (rc = fmdh_grow(&s->cap_blocks, (size_t)n_blocks, g, 6))) return rc;
  }
  const hipStream_t st = s->o.ord.stream;
  rc = fmdh_host_copy(FMD_OK, __func__, st, s->d_pcm, pcm, pb, hipMemcpyHostToDevice);
  rc = fmdh_host_copy(rc, __func__, st, s->d_lens, lens, slots * sizeof(int32_t), hipMemcpyHostToDevice);
  if (with_z) rc = fmdh_host_copy(rc, __func__, st, s->d_z, z, zb, hipMemcpyHostToDevice);
  if (quality) rc = fmdh_host_copy(rc, __func__, st, s->d_q, quality, slots * sizeof(float), hipMemcpyHostToDevice);
  if (!rc) rc = fmd_stereo_run_device(s, s->d_pcm, s->d_lens, with_z ? s->d_z : NULL, quality ? s->d_q : NULL, n_blocks, s->d_pcm, s->d_info,
                                      meter ? s->d_meter : NULL, NULL);
  rc = fmdh_host_copy(rc, __func__, st, out, s->d_pcm, pb, hipMemcpyDeviceToHost);
  rc = fmdh_host_copy(rc, __func__, st, info, s->d_info, slots * sizeof(fmd_stereo_info), hipMemcpyDeviceToHost);
  if (meter) rc = fmdh_host_copy(rc, __func__, st, meter, s->d_meter, slots * sizeof(fmd_stereo_meter), hipMemcpyDeviceToHost);
  return fmdh_host_wait(rc, __func__, st);
}

int fmd_stereo_get_state(fmd_stereo *s, int stream, fmd_stereo_state *out) {
  if (!s || !out || stream < 0 || stream >= s->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  return fmdh_obj_get_state(&s->o, stream, out);
}

int fmd_stereo_set_state(fmd_stereo *s, int stream, const fmd_stereo_state *in) {
  if (!s || !in || stream < 0 || stream >= s->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  if (!(in->g >= 0.0f) || !(in->g <= 1.0f)) return fmd_fail(FMD_E_ARG, "g %g outside 0 .. 1", (double)in->g);
  if (in->stereo != 0 && in->stereo != 1) return fmd_fail(FMD_E_ARG, "stereo must be 0 or 1 (got %d)", in->stereo);
  if (in->run < 0 || in->run >= s->cfg.hold_blocks) return fmd_fail(FMD_E_ARG, "run %d outside 0 .. %d (hold_blocks - 1)", in->run, s->cfg.hold_blocks - 1);
  if (in->reserved) return fmd_fail(FMD_E_ARG, "the reserved word of the state must be zero");
  return fmdh_obj_set_state(&s->o, stream, in);
}

int fmd_stereo_reset(fmd_stereo *s) {
  if (!s) return fmd_fail(FMD_E_ARG, "NULL stereo object");
  return fmdh_obj_reset(&s->o);
}

int fmd_stereo_sync(fmd_stereo *s) {
  if (!s) return fmd_fail(FMD_E_ARG, "NULL stereo object");
  return fmdh_obj_sync(&s->o);
}

/* ---- RDS receiver ----------------------------------------------------------- */
/* An object of its own (csrc/rds.inc): range check, geometry, taps and timing table are fmd_rds.c's; here its device side.  Everything a launch of
 * up to max_blocks blocks needs - taps, table, state, the scratch for y, the chunk partials and the per-block records - is made at create. */

struct fmd_rds {
  struct fmdh_obj o;           /* its state: fmd_rds_state[n_streams] */
  fmd_rds_config cfg;
  fmdk_rds_geom g;
  int n_streams, cpb;
  float *d_taps, *d_w;
  void *d_y, *d_part, *d_blk;  /* scratch of a launch, for max_blocks blocks per stream */
  void *d_zin, *d_soft, *d_lens, *d_first, *d_est;      /* staging of fmd_rds_run_host, made at its first use */
  int last_blocks;             /* n_blocks of the most recent launch (fmd_rds_last_y) */
};

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
  if ((rc = taps ? fmdh_copy_taps(h, taps, cfg->n_taps) : fmd_rds_design(cfg, h))) return rc;

  fmd_rds *r = (fmd_rds *)calloc(1, sizeof(*r));
  if (!r) return fmd_fail(FMD_E_NOMEM, "out of host memory");
  r->cfg = *cfg;
  fmdk_rds_geometry(cfg->rate_z, cfg->block_z, &r->g);
  r->n_streams = n_streams;
  r->cpb = (int)cpb;
  fmdk_rds_table(cfg, w);
  const size_t slots = (size_t)n_streams * (size_t)cfg->max_blocks, w_bytes = sizeof(float) * 2 * (size_t)r->g.pw;
  void **const staging[] = {&r->d_zin, &r->d_soft, &r->d_lens, &r->d_first, &r->d_est};
  (void)((rc = fmdh_obj_open(&r->o, device, sizeof(fmd_rds_state), n_streams, 1)) ||
         (rc = fmdh_obj_alloc(&r->o, (void **)&r->d_taps, sizeof(float) * FMD_RDS_MAX_TAPS, h, sizeof(float) * (size_t)cfg->n_taps)) ||
         (rc = fmdh_obj_alloc(&r->o, (void **)&r->d_w, w_bytes, w, w_bytes)) ||
         (rc = fmdh_obj_alloc(&r->o, &r->d_y, slots * (size_t)cfg->block_z * 2 * sizeof(float), NULL, 0)) ||
         (rc = fmdh_obj_alloc(&r->o, &r->d_part, slots * (size_t)cpb * 4 * sizeof(float), NULL, 0)) ||
         (rc = fmdh_obj_alloc(&r->o, &r->d_blk, slots * sizeof(fmdk_rds_blk), NULL, 0)));
  for (int i = 0; i < 5; i++) fmdh_obj_own(&r->o, staging[i]);
  if (rc) { fmd_rds_destroy(r); return rc; }
  *out = r;
  return FMD_OK;
}

int fmd_subc_rds_create(fmd_rds **out, const fmd_subc *s, int n_taps, int avg_blocks, int max_blocks) {
  if (!out) return fmd_fail(FMD_E_ARG, "out is NULL");
  *out = NULL;
  if (!s) return fmd_fail(FMD_E_ARG, "NULL subcarrier object");
  if (s->cfg.rate_in % s->cfg.decim) return fmd_fail(FMD_E_UNSUPPORTED, "rate_in %d is no multiple of decim %d", s->cfg.rate_in, s->cfg.decim);
  const fmd_rds_config c = {s->cfg.rate_in / s->cfg.decim, s->cfg.block_samples / s->cfg.decim, n_taps, avg_blocks, max_blocks};
  return fmd_rds_create(out, &c, NULL, s->n_streams, s->o.device);
}

void fmd_rds_destroy(fmd_rds *r) {
  if (!r) return;
  fmdh_obj_close(&r->o);
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
  hipStream_t st;
  const int rc = fmdh_obj_launch_begin(&r->o, hip_stream, "fmd_rds_sync", &st);
  if (rc) return rc;
  const int e = fmdk_rds_launch(d_z, r->n_streams, n_blocks, &r->cfg, &r->g, r->d_taps, r->d_w, r->o.d_state, r->d_y, r->d_part, r->d_blk, d_soft, d_lens,
                                d_first, d_est, st);
  if (e) return fmd_fail(FMD_E_HIP, "RDS kernel launch failed: %s (%d)", hipGetErrorString((hipError_t)e), e);
  fmdh_order_launched(&r->o.ord, st);
  r->last_blocks = n_blocks;
  return FMD_OK;
}

int fmd_rds_run_host(fmd_rds *r, const float *z, int n_blocks, float *soft, int32_t *lens, int64_t *first, float *est) {
  if (!r || !z || !soft || !lens) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks <= 0 || n_blocks > r->cfg.max_blocks) return fmd_fail(FMD_E_ARG, "n_blocks must lie in 1 .. max_blocks = %d", r->cfg.max_blocks);
  HIP_TRY(hipSetDevice(r->o.device));
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
  const hipStream_t st = r->o.ord.stream;
  int rc = fmdh_host_copy(FMD_OK, __func__, st, r->d_zin, z, slots * zb, hipMemcpyHostToDevice);
  if (!rc) rc = fmd_rds_run_device(r, r->d_zin, n_blocks, r->d_soft, r->d_lens, r->d_first, r->d_est, NULL);
  rc = fmdh_host_copy(rc, __func__, st, soft, r->d_soft, slots * sb, hipMemcpyDeviceToHost);
  rc = fmdh_host_copy(rc, __func__, st, lens, r->d_lens, slots * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (first) rc = fmdh_host_copy(rc, __func__, st, first, r->d_first, slots * sizeof(int64_t), hipMemcpyDeviceToHost);
  if (est) rc = fmdh_host_copy(rc, __func__, st, est, r->d_est, slots * 4 * sizeof(float), hipMemcpyDeviceToHost);
  return fmdh_host_wait(rc, __func__, st);
}

int fmd_rds_last_y(fmd_rds *r, int n_blocks, float *y, float *tm) {
  if (!r || (!y && !tm)) return fmd_fail(FMD_E_ARG, "NULL argument");
  if (n_blocks <= 0 || n_blocks != r->last_blocks) return fmd_fail(FMD_E_STATE, "the most recent launch had %d blocks, not %d", r->last_blocks, n_blocks);
  const int rc = fmdh_obj_sync(&r->o);
  if (rc) return rc;
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
  return fmdh_obj_get_state(&r->o, stream, out);
}

int fmd_rds_set_state(fmd_rds *r, int stream, const fmd_rds_state *in) {
  if (!r || !in || stream < 0 || stream >= r->n_streams) return fmd_fail(FMD_E_ARG, "bad argument");
  if (in->phase < 0 || in->phase >= r->g.pw) return fmd_fail(FMD_E_ARG, "phase %d outside 0 .. %d (the timing table's period)", in->phase, r->g.pw - 1);
  const int lo = -FMDK_RDS_Q * r->g.lb;
  if (in->frac < lo || in->frac >= lo + r->g.two_rz) return fmd_fail(FMD_E_ARG, "frac %d outside %d .. %d", in->frac, lo, lo + r->g.two_rz - 1);
  if (in->bit < 0) return fmd_fail(FMD_E_ARG, "bit index is negative");
  return fmdh_obj_set_state(&r->o, stream, in);
}

int fmd_rds_reset(fmd_rds *r) {
  if (!r) return fmd_fail(FMD_E_ARG, "NULL RDS object");
  return fmdh_obj_reset(&r->o);
}

int fmd_rds_sync(fmd_rds *r) {
  if (!r) return fmd_fail(FMD_E_ARG, "NULL RDS object");
  return fmdh_obj_sync(&r->o);
}
