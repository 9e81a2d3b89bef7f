/* fmd_ring.h - the ingest ring without a device (fmd_ring.c).  Private, like fmd_internal.h; a header of its own so that fmd_ring.c and
 * tests/c/ring_check.c need nothing of HIP and the kernel units' dependency list stays as it is. */
#ifndef FMD_RING_H
#define FMD_RING_H

#include <pthread.h>
#include <stdint.h>

#include "fmdemod_mi355x.h"

struct fmd_ingest {
  struct fmd_batch *batch; /* NULL once the batch has been destroyed; never dereferenced by fmd_ring.c */
  int stream;
  uint8_t *ring;           /* the caller's memory: pinned for a bound ring, calloc for an unbound one */
  uint32_t cap, rpos, wpos, size, inflight;
  uint32_t debt;           /* in-flight bytes an overflow has already released (drop-oldest) */
  uint64_t dropped;
  int mute;
  int overflow_mode;
  int unbound;             /* created without a batch: ring in pageable memory */
  pthread_mutex_t m;
};

/* An empty drop-oldest ring over the cap bytes at mem, and its mutex; _fini destroys the mutex (the memory stays the caller's). */
void fmdk_ring_init(struct fmd_ingest *g, uint8_t *mem, uint32_t cap);
void fmdk_ring_fini(struct fmd_ingest *g);
/* The pump's four accounting steps; each takes the ring's lock itself.  _ready: bytes no job has taken.  _take: hands the next `take` bytes to a job
 * and returns where they start.  _release: a job's H2D copies have finished.  _untake: the newest job was never launched; old_take = the take of the
 * other job while it still holds ring bytes, else 0. */
uint32_t fmdk_ring_ready(struct fmd_ingest *g);
uint32_t fmdk_ring_take(struct fmd_ingest *g, uint32_t take);
void fmdk_ring_release(struct fmd_ingest *g, uint32_t take);
void fmdk_ring_untake(struct fmd_ingest *g, uint32_t take, uint32_t old_take);
/* The n bytes at `from` as one or two pieces: *first bytes at (returned base) + from, the other n - *first at the base. */
const uint8_t *fmdk_ring_split(const struct fmd_ingest *g, uint32_t from, uint32_t n, uint32_t *first);
/* _owner: the batch (NULL: none, or destroyed), and whether a job holds bytes of the ring.  _detach: the batch is going away. */
struct fmd_batch *fmdk_ring_owner(struct fmd_ingest *g, int *busy);
void fmdk_ring_detach(struct fmd_ingest *g);
/* fmd_resolve.c's (fmd_internal.h declares it too); a program that links fmd_ring.c alone supplies its own. */
int fmd_fail(int code, const char *fmt, ...) __attribute__((visibility("hidden"), format(printf, 2, 3)));

#endif
