/*
 * fmd_dev.h - the device plumbing the batch (fmd_host.c) and the receiver objects beside it (fmd_objects.c) share, and the core those objects embed.
 * Private to the library: the fmdh_ names stay inside it (csrc/fmdemod_mi355x.map exports fmd_* only).
 */
#ifndef FMD_DEV_H
#define FMD_DEV_H

#include <hip/hip_runtime_api.h>

#include "fmd_internal.h"

#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fmd_fail(FMD_E_HIP, "%s failed: %s (%d)", #expr, hipGetErrorString(e_), (int)e_); \
  } while (0)

/* Count the devices, default *dev (< 0) to the current one, range-check it and make it current. */
int fmdh_open_device(int *dev);
/* Is st being captured into a hipGraph (nothing can be allocated, and no event of ours recorded outside it, then). */
int fmdh_stream_is_capturing(hipStream_t st);
/* The caller's n taps into h, refused where one is not finite (needs no device). */
int fmdh_copy_taps(float *h, const float *taps, int n);

/* Buffers (device, or pinned host) that share one capacity, grown on demand: below `need` all n are freed and made anew (on a failure the pointers
 * not yet made are NULL and the capacity 0).  Does not synchronise: each caller says why nothing queued still uses the old buffers. */
typedef struct { void **p; size_t bytes; int pinned; } grow_buf;
int fmdh_grow(size_t *cap, size_t need, const grow_buf *v, int n);

/* Where an object's launches run.  Each launch reads the state the one before wrote: launches on one stream are ordered by the stream, a change
 * of stream between two launches is handed over with an event. */
struct launch_order {
  hipStream_t stream;          /* the object's own */
  hipStream_t last_stream;     /* stream of the most recent launch (the own or the caller's) */
  int launched;                /* a launch has been queued on last_stream */
  hipEvent_t ev_order;         /* makes the new stream wait for the previous launch */
};
/* Wait for everything queued: the stream of the most recent launch when the caller supplied it, `also` (NULL: none) and the own stream. */
hipError_t fmdh_order_quiesce(struct launch_order *o, hipStream_t also);
/* Before a launch on st: 0 when st is ordered behind the previous launch, 1 when that needs the event and st is being captured - recording an event
 * of ours on a stream outside the capture would invalidate it, so the caller refuses with what to do instead - or a status (< 0). */
int fmdh_order_handover(struct launch_order *o, hipStream_t st);
static inline void fmdh_order_launched(struct launch_order *o, hipStream_t st) { o->last_stream = st; o->launched = 1; }

/* The copies of a host form (*_run_host, fmd_batch_spectrum_host) between the caller's memory and the staging, on the object's own stream `st`, and
 * the wait that ends it.  rc carries the first failure through: a copy after it is not queued, and its status and text are what the wait returns -
 * after it has waited, whatever failed: a queued copy must not outlive the call that passed its buffer.  `what` names the function in a HIP failure's text. */
int fmdh_host_copy(int rc, const char *what, hipStream_t st, void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
int fmdh_host_wait(int rc, const char *what, hipStream_t st);

/* The core of a receiver object, embedded as a member: device, own stream and launch order, the carried state, and the device buffers to free.  An
 * owned buffer is recorded by the address of the object's pointer to it: staging made or grown later through that pointer is freed by the same close. */
#define FMDH_MAX_OWNED 12
struct fmdh_obj {
  int device;
  struct launch_order ord;
  hipStream_t also;            /* a second stream of the object's, made by it when first needed (NULL: none): waited for with the own one, destroyed with it */
  void *d_state;              /* n_state elements of state_elem bytes (none: NULL, 0): read by a launch's kernels, advanced in place by the state kernel behind them */
  size_t state_elem;
  int n_state;
  void **owned[FMDH_MAX_OWNED];
  int n_owned;
};
/* o zeroed.  Opens the device, makes the own stream and - want_event - the hand-over event, allocates the state, zeroes it on the own stream and waits. */
int fmdh_obj_open(struct fmdh_obj *o, int device, size_t state_elem, int n_state, int want_event);
/* Record *p (a buffer, or NULL until one is made) as o's to free. */
void fmdh_obj_own(struct fmdh_obj *o, void **p);
/* hipMalloc of `bytes` into *p, owned, and - src not NULL - its first src_bytes copied from the host (returns when they are there). */
int fmdh_obj_alloc(struct fmdh_obj *o, void **p, size_t bytes, const void *src, size_t src_bytes);
/* Waits for everything o has queued, frees the state and every owned buffer, destroys event and stream.  Also the failure path of a create: safe
 * after an open that failed or never ran. */
void fmdh_obj_close(struct fmdh_obj *o);
/* Make the device current and wait for everything queued. */
int fmdh_obj_sync(struct fmdh_obj *o);
/* The carried state, after such a wait: all of it zeroed; element i (in range: the caller checked) copied out, or in. */
int fmdh_obj_reset(struct fmdh_obj *o);
int fmdh_obj_get_state(struct fmdh_obj *o, int i, void *out);
int fmdh_obj_set_state(struct fmdh_obj *o, int i, const void *in);
/* The head of a *_run_device: the device made current and *st - hip_stream, or the own stream - ordered behind the previous launch; FMD_E_STATE,
 * naming sync_fn, where that needs the event and *st is being captured.  After the launch: fmdh_order_launched(&o->ord, *st). */
int fmdh_obj_launch_begin(struct fmdh_obj *o, void *hip_stream, const char *sync_fn, hipStream_t *st);

#endif
