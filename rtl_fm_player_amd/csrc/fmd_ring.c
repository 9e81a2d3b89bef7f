/*
 * fmd_ring.c - the rtlsdr_read_async-compatible ingest ring and its accounting.  No device: this unit includes no GPU header and makes no GPU
 * call, so tests/c/ring_check.c links it alone (tests/test_ring_cpu.py).  A ring's memory and the pump that copies out of it are fmd_host.c's.
 *
 * One ring per stream, written by fmd_ingest_callback (any thread: librtlsdr's USB event thread in the reference, src/rtl_fm_player.c:839-853)
 * and drained by the pump (the demod thread's role, :855-933).  The ring IS the H2D source: a job's bytes are copied to the device straight from
 * the ring (no second host copy) and stay accounted as buffered until that copy has finished.
 *
 * Accounting (all under g->m):
 *   rpos      oldest byte not yet released        size      bytes in [rpos, rpos + size) (mod cap)
 *   inflight  leading bytes of that range handed to jobs whose H2D may still be reading them
 *   wpos      next write position
 * Two overflow behaviours (fmd_ingest_set_overflow):
 *   FMD_OVERFLOW_DROP_OLDEST (default)  the copy wraps at the end of the ring; bytes beyond the capacity push rpos forward (the oldest data is
 *       lost, counted in `dropped`).  A clean loss.
 *   FMD_OVERFLOW_REFERENCE  rtlsdr_callback to the letter (:813-834): a transfer that does not fit before the end of the ring restarts at offset 0
 *       (no split copy; whatever lies between wpos and the end is left as it is), and on overflow only the byte count is clamped - rpos stays, so
 *       the reader next sees new data where it expected old.  Kept for identical behaviour (tests/test_ring_ref.py holds it against the
 *       reference's own callback).
 */
#define _GNU_SOURCE
#include <string.h>

#include "fmd_ring.h"

void fmdk_ring_init(struct fmd_ingest *g, uint8_t *mem, uint32_t cap) {
  g->ring = mem;
  g->cap = cap;
  g->overflow_mode = FMD_OVERFLOW_DROP_OLDEST;
  pthread_mutex_init(&g->m, NULL);
}
void fmdk_ring_fini(struct fmd_ingest *g) { pthread_mutex_destroy(&g->m); }

struct fmd_batch *fmdk_ring_owner(struct fmd_ingest *g, int *busy) {
  pthread_mutex_lock(&g->m);
  struct fmd_batch *b = g->batch;
  *busy = g->inflight != 0 || g->debt != 0;     /* debt: in-flight bytes an overflow has moved out of `inflight` */
  pthread_mutex_unlock(&g->m);
  return b;
}

void fmdk_ring_detach(struct fmd_ingest *g) {
  pthread_mutex_lock(&g->m);
  g->batch = NULL;
  g->inflight = 0;
  g->debt = 0;
  pthread_mutex_unlock(&g->m);
}

int fmd_ingest_set_overflow(fmd_ingest *g, int mode) {
  if (!g || (mode != FMD_OVERFLOW_DROP_OLDEST && mode != FMD_OVERFLOW_REFERENCE)) return fmd_fail(FMD_E_ARG, "bad argument");
  pthread_mutex_lock(&g->m);
  g->overflow_mode = mode;
  pthread_mutex_unlock(&g->m);
  return FMD_OK;
}

void fmd_ingest_mute(fmd_ingest *g, int n_bytes) {
  if (!g) return;
  pthread_mutex_lock(&g->m);
  g->mute = n_bytes;
  pthread_mutex_unlock(&g->m);
}

/* rtlsdr_read_async_cb_t; the role of rtlsdr_callback (src/rtl_fm_player.c:790-837): optional mute fill (:805-810), copy into the ring under the lock,
 * overflow accounting.  Never blocks on the GPU. */
void fmd_ingest_callback(unsigned char *buf, uint32_t len, void *ctx) {
  fmd_ingest *g = (fmd_ingest *)ctx;
  if (!g || !buf || len == 0) return;
  pthread_mutex_lock(&g->m);
  if (g->mute) {
    uint32_t n = (uint32_t)g->mute < len ? (uint32_t)g->mute : len;
    memset(buf, 127, n);               /* the reference fills the USB buffer itself too (:807-808) */
    g->mute = 0;
  }
  if (g->overflow_mode == FMD_OVERFLOW_REFERENCE) {
    if (len > g->cap) { buf += len - g->cap; g->dropped += len - g->cap; len = g->cap; }   /* cannot happen with USB transfers */
    if (g->wpos + len <= g->cap) {                                  /* :813-820 */
      memcpy(g->ring + g->wpos, buf, len);
      g->wpos += len;
      if (g->wpos == g->cap) g->wpos = 0;
    } else {                                                        /* :821-827: restart at zero */
      memcpy(g->ring, buf, len);
      g->wpos = len;
    }
    if ((uint64_t)g->size + len > g->cap) {                         /* :829-834: clamp the count, rpos stays */
      g->dropped += (uint64_t)g->size + len - g->cap;
      g->size = g->cap;
    } else {
      g->size += len;
    }
    pthread_mutex_unlock(&g->m);
    return;
  }
  if (len > g->cap) {            /* keep the newest cap bytes */
    g->dropped += len - g->cap;
    buf += len - g->cap;
    len = g->cap;
  }
  uint32_t first = g->cap - g->wpos;
  if (first > len) first = len;
  memcpy(g->ring + g->wpos, buf, first);
  memcpy(g->ring, buf + first, len - first);
  g->wpos = (g->wpos + len) % g->cap;
  if ((uint64_t)g->size + len > g->cap) {        /* overwrote the oldest data */
    const uint32_t over = (uint32_t)((uint64_t)g->size + len - g->cap);
    g->dropped += over;
    g->rpos = (g->rpos + over) % g->cap;
    g->size = g->cap;
    /* bytes a job was still reading have been overwritten (that job's block is damaged, as any overflow damages the stream): they are released
     * here, not again when the job ends */
    const uint32_t eaten = over < g->inflight ? over : g->inflight;
    g->inflight -= eaten;
    g->debt += eaten;
  } else {
    g->size += len;
  }
  pthread_mutex_unlock(&g->m);
}

const uint8_t *fmdk_ring_split(const struct fmd_ingest *g, uint32_t from, uint32_t n, uint32_t *first) {
  *first = g->cap - from < n ? g->cap - from : n;
  return g->ring;
}

/* The dequeue of demod_thread_fn (src/rtl_fm_player.c:863-876) for callers that drain a ring themselves: when at least len bytes are buffered, copies
 * them out and returns len, else 0. */
uint32_t fmd_ingest_pop(fmd_ingest *g, uint8_t *out, uint32_t len) {
  if (!g || !out || len == 0 || len > g->cap) return 0;
  pthread_mutex_lock(&g->m);
  /* jobs hold the bytes in front of these (they cannot be released out of order): nothing is copied then */
  if (g->inflight != 0 || g->debt != 0 || g->size < len) { pthread_mutex_unlock(&g->m); return 0; }
  const uint32_t from = g->rpos;
  uint32_t first = g->cap - from;
  if (first > len) first = len;
  memcpy(out, g->ring + from, first);
  memcpy(out + first, g->ring, len - first);
  g->rpos = (g->rpos + len) % g->cap;
  g->size -= len;
  pthread_mutex_unlock(&g->m);
  return len;
}

uint32_t fmdk_ring_ready(struct fmd_ingest *g) {
  pthread_mutex_lock(&g->m);
  const uint32_t n = g->size - g->inflight;     /* bytes no job has taken yet */
  pthread_mutex_unlock(&g->m);
  return n;
}

uint32_t fmd_ingest_buffered(const fmd_ingest *g) { return g ? fmdk_ring_ready((fmd_ingest *)g) : 0; }

uint64_t fmd_ingest_dropped(const fmd_ingest *gc) {
  fmd_ingest *g = (fmd_ingest *)gc;
  if (!g) return 0;
  pthread_mutex_lock(&g->m);
  const uint64_t n = g->dropped;
  pthread_mutex_unlock(&g->m);
  return n;
}

uint32_t fmdk_ring_take(struct fmd_ingest *g, uint32_t take) {
  pthread_mutex_lock(&g->m);
  const uint32_t from = (g->rpos + g->inflight) % g->cap;
  g->inflight += take;
  pthread_mutex_unlock(&g->m);
  return from;
}

void fmdk_ring_release(struct fmd_ingest *g, uint32_t take) {
  pthread_mutex_lock(&g->m);
  uint32_t r = take;
  const uint32_t d = g->debt < r ? g->debt : r;    /* part an overflow has released already */
  g->debt -= d;
  r -= d;
  if (r > g->inflight) r = g->inflight;
  g->rpos = (g->rpos + r) % g->cap;
  g->size -= r;
  g->inflight -= r;
  pthread_mutex_unlock(&g->m);
}

/* debt = bytes an overflow has eaten from the OLDEST end of the in-flight region: they belong to the other job first (if one still holds ring space),
 * and only what exceeds that job's take was eaten from this one.  That part is already released (rpos and size moved on when the overflow happened);
 * the rest of this job's take goes back to "buffered", and the other job's share of the debt stays for its own release. */
void fmdk_ring_untake(struct fmd_ingest *g, uint32_t take, uint32_t old_take) {
  pthread_mutex_lock(&g->m);
  const uint32_t mine = g->debt > old_take ? g->debt - old_take : 0;      /* eaten from this job's bytes */
  const uint32_t eaten = mine < take ? mine : take;
  g->debt -= eaten;
  const uint32_t r = take - eaten;
  g->inflight -= r < g->inflight ? r : g->inflight;
  pthread_mutex_unlock(&g->m);
}
