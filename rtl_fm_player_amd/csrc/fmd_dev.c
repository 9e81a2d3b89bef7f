/*
 * fmd_dev.c - the device plumbing of the C host layer (fmd_dev.h): device opening, grow-on-demand buffers, the launch order across streams, the
 * copies of the host forms and the core the receiver objects embed.  Plain C above the HIP runtime's C API; nothing here launches a kernel.
 */
#define _GNU_SOURCE
#include <assert.h>
#include <math.h>

#include "fmd_dev.h"

int fmdh_open_device(int *dev) {
  int ndev = 0, device = *dev;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fmd_fail(FMD_E_NODEVICE, "no HIP device: the MI355X path has no CPU fallback");
  if (device < 0) HIP_TRY(hipGetDevice(&device));
  if (device >= ndev) return fmd_fail(FMD_E_ARG, "device %d out of range (%d devices)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  *dev = device;
  return FMD_OK;
}

int fmdh_stream_is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess) { cap = hipStreamCaptureStatusNone; (void)hipGetLastError(); }
  return cap != hipStreamCaptureStatusNone;
}

int fmdh_grow(size_t *cap, size_t need, const grow_buf *v, int n) {
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

int fmdh_copy_taps(float *h, const float *taps, int n) {
  for (int k = 0; k < n; k++) {
    if (!isfinite(taps[k])) return fmd_fail(FMD_E_ARG, "tap %d is not finite", k);
    h[k] = taps[k];
  }
  return FMD_OK;
}

hipError_t fmdh_order_quiesce(struct launch_order *o, hipStream_t also) {
  hipError_t e = hipSuccess, t;
  if (o->launched && o->last_stream && o->last_stream != o->stream && (t = hipStreamSynchronize(o->last_stream)) != hipSuccess) e = t;
  if (also && (t = hipStreamSynchronize(also)) != hipSuccess) e = t;
  if (o->stream && (t = hipStreamSynchronize(o->stream)) != hipSuccess) e = t;
  if (e == hipSuccess) o->launched = 0;        /* nothing is in flight: the next launch needs no hand-over, whatever stream it is on */
  return e;
}

int fmdh_order_handover(struct launch_order *o, hipStream_t st) {
  if (!o->launched || o->last_stream == st) return 0;
  if (fmdh_stream_is_capturing(st)) return 1;
  HIP_TRY(hipEventRecord(o->ev_order, o->last_stream));
  HIP_TRY(hipStreamWaitEvent(st, o->ev_order, 0));
  return 0;
}

int fmdh_host_copy(int rc, const char *what, hipStream_t st, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
  if (rc) return rc;
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
  return e == hipSuccess ? FMD_OK : fmd_fail(FMD_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

int fmdh_host_wait(int rc, const char *what, hipStream_t st) {
  const hipError_t w = hipStreamSynchronize(st);
  if (rc) return rc;                                     /* (fmd_last_error's text is the first failure's) */
  return w == hipSuccess ? FMD_OK : fmd_fail(FMD_E_HIP, "%s: %s", what, hipGetErrorString(w));
}

/* ---- the core of a receiver object ------------------------------------------ */

static int setup_failed(hipError_t e) { return fmd_fail(FMD_E_HIP, "device setup failed: %s", hipGetErrorString(e)); }

int fmdh_obj_open(struct fmdh_obj *o, int device, size_t state_elem, int n_state, int want_event) {
  const int rc = fmdh_open_device(&device);
  if (rc) return rc;
  o->device = device;
  o->state_elem = state_elem;
  o->n_state = n_state;
  const size_t st_bytes = state_elem * (size_t)n_state;
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&o->ord.stream, hipStreamNonBlocking)) != hipSuccess ||
      (want_event && (e = hipEventCreateWithFlags(&o->ord.ev_order, hipEventDisableTiming)) != hipSuccess))
    return setup_failed(e);
  if (st_bytes && ((e = hipMalloc(&o->d_state, st_bytes)) != hipSuccess ||
                   (e = hipMemsetAsync(o->d_state, 0, st_bytes, o->ord.stream)) != hipSuccess ||
                   (e = hipStreamSynchronize(o->ord.stream)) != hipSuccess))
    return setup_failed(e);
  return FMD_OK;
}

void fmdh_obj_own(struct fmdh_obj *o, void **p) {
  assert(o->n_owned < FMDH_MAX_OWNED);                   /* (how many an object owns is written in its create) */
  o->owned[o->n_owned++] = p;
}

int fmdh_obj_alloc(struct fmdh_obj *o, void **p, size_t bytes, const void *src, size_t src_bytes) {
  fmdh_obj_own(o, p);
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess && src) e = hipMemcpy(*p, src, src_bytes, hipMemcpyHostToDevice);
  return e == hipSuccess ? FMD_OK : setup_failed(e);
}

void fmdh_obj_close(struct fmdh_obj *o) {
  if (!o->ord.stream) return;                            /* never opened: no device was made current and nothing exists */
  hipSetDevice(o->device);
  fmdh_order_quiesce(&o->ord, o->also);
  if (o->d_state) hipFree(o->d_state);
  for (int i = 0; i < o->n_owned; i++)
    if (*o->owned[i]) hipFree(*o->owned[i]);
  if (o->also) hipStreamDestroy(o->also);
  if (o->ord.ev_order) hipEventDestroy(o->ord.ev_order);
  hipStreamDestroy(o->ord.stream);
}

int fmdh_obj_sync(struct fmdh_obj *o) {
  HIP_TRY(hipSetDevice(o->device));
  HIP_TRY(fmdh_order_quiesce(&o->ord, o->also));
  return FMD_OK;
}

int fmdh_obj_reset(struct fmdh_obj *o) {
  const int rc = fmdh_obj_sync(o);
  if (rc) return rc;
  /* on the own stream and waited for: hipMemset on device memory may return before the fill has run, and the own stream (non-blocking) does not
   * order itself behind the null stream */
  HIP_TRY(hipMemsetAsync(o->d_state, 0, o->state_elem * (size_t)o->n_state, o->ord.stream));
  HIP_TRY(hipStreamSynchronize(o->ord.stream));
  return FMD_OK;
}

int fmdh_obj_get_state(struct fmdh_obj *o, int i, void *out) {
  const int rc = fmdh_obj_sync(o);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(out, (char *)o->d_state + o->state_elem * (size_t)i, o->state_elem, hipMemcpyDeviceToHost));
  return FMD_OK;
}

int fmdh_obj_set_state(struct fmdh_obj *o, int i, const void *in) {
  const int rc = fmdh_obj_sync(o);
  if (rc) return rc;
  HIP_TRY(hipMemcpy((char *)o->d_state + o->state_elem * (size_t)i, in, o->state_elem, hipMemcpyHostToDevice));
  return FMD_OK;
}

int fmdh_obj_launch_begin(struct fmdh_obj *o, void *hip_stream, const char *sync_fn, hipStream_t *st) {
  HIP_TRY(hipSetDevice(o->device));
  *st = hip_stream ? (hipStream_t)hip_stream : o->ord.stream;
  const int rc = fmdh_order_handover(&o->ord, *st);
  if (rc > 0) return fmd_fail(FMD_E_STATE, "the previous launch ran on another stream: call %s() before capturing this one into a graph", sync_fn);
  return rc;
}
