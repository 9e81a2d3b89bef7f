/* stereo.inc - stereo control (fmd_stereo_*; include/fmdemod_mi355x.h, "Stereo control"): included by fmd_kernels_recv.hip, the receivers' translation
 * unit, beside scan.inc.  Kernels of their own: they share nothing with the fused kernel but the PCM layout it writes and the z
 * layout of the subcarrier receiver, and reference nothing of the host layer.  gfx950, no inline assembly, no floating-point atomics.  The unit is
 * built with -ffp-contract=off and without fast-math: every operation below is one float32 operation with one rounding, fmaf the only fused one,
 * `/` the correctly rounded division - tests/stereo_model.py repeats them in numpy.
 *
 *   1. fmd_stereo_pilot_kernel, one workgroup of 256 threads per (stream, block): thread t sums p = fma(zi, zi, zr zr) over z[t], z[t + 256], ...
 *      in that order from zero, then the LDS tree a[t] = a[t] + a[t + h], h = 128 .. 1; info.pilot_ms = a[0] inv_mz.
 *   2. fmd_stereo_track_kernel, one workgroup per stream, one thread at work: walks the launch's blocks in order - indicator with hysteresis and
 *      hold, blend target, slew-limited g - and writes every field of the block's fmd_stereo_info.  The only reader and the only writer of
 *      fmd_stereo_state, which it stores at its end: the stream orders the next launch behind it, and a captured graph advances it on every replay.
 *   3. fmd_stereo_apply_kernel, one workgroup of 256 threads per (stream, block): a thread takes the 16-byte words t, t + 256, ... of the slot (four
 *      frames each; consecutive threads at consecutive words), blends the frames below info.frames with the ramp of g and stores the word - every
 *      word of the slot is written, so out may be the input (a word is read and written by one thread) or another buffer.  The meters are integers
 *      gathered with LDS integer atomics: a maximum and a sum do not depend on the order of their terms.
 * Every index is bounded by the configuration: frames <= pcm_stride / 2 whatever lens holds, the word loop by pcm_stride / 8, the z loop by Mz. */

namespace {

constexpr int STC_NT = 256;
static_assert(sizeof(fmd_stereo_config) == 48 && sizeof(fmd_stereo_state) == 16 && sizeof(fmd_stereo_info) == 32 && sizeof(fmd_stereo_meter) == 32,
              "the layouts of the header");

__device__ __forceinline__ float stc_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ __launch_bounds__(STC_NT) void fmd_stereo_pilot_kernel(const float2 *__restrict__ z, int Mz, float inv_mz, fmd_stereo_info *__restrict__ info) {
  __shared__ float a[STC_NT];
  const int t = threadIdx.x;
  const size_t sb = blockIdx.x;
  const float2 *src = z + sb * (size_t)Mz;
  float acc = 0.f;
  for (int i = t; i < Mz; i += STC_NT) {
    const float2 q = src[i];
    const float p = __builtin_fmaf(q.y, q.y, q.x * q.x);
    acc = acc + p;
  }
  a[t] = acc;
  __syncthreads();
#pragma unroll
  for (int h = STC_NT / 2; h >= 1; h >>= 1) {
    if (t < h) a[t] = a[t] + a[t + h];
    __syncthreads();
  }
  if (t == 0) info[sb].pilot_ms = a[0] * inv_mz;
}

struct stc_track_args {
  const int32_t *lens;
  const float *quality;        /* or NULL */
  fmd_stereo_state *state;
  fmd_stereo_info *info;
  float thr_on, thr_off, blend_lo, inv_span, slew;
  int32_t n_blocks, pcm_stride, hold_blocks, mode, has_z;
};

__global__ __launch_bounds__(64) void fmd_stereo_track_kernel(const stc_track_args a) {
  if (threadIdx.x != 0) return;
  const size_t s = blockIdx.x;
  fmd_stereo_state *st = a.state + s;
  float g = st->g;
  int stereo = st->stereo, run = st->run;
  for (int b = 0; b < a.n_blocks; b++) {
    const size_t sb = s * (size_t)a.n_blocks + (size_t)b;
    int len = a.lens[sb];
    len = len < 0 ? 0 : (len > a.pcm_stride ? a.pcm_stride : len);
    const int frames = len >> 1;
    const float q = a.has_z ? a.info[sb].pilot_ms : 0.f;
    const float g0 = g;
    if (frames > 0 && a.mode == FMD_STEREO_AUTO && a.has_z) {
      const int want = stereo ? (q >= a.thr_off) : (q >= a.thr_on);
      if (want != stereo) {
        run += 1;
        if (run >= a.hold_blocks) { stereo = want; run = 0; }
      } else {
        run = 0;
      }
    }
    float step = 0.f;
    if (frames > 0) {
      float target;
      if (a.mode == FMD_STEREO_FORCE_MONO) target = 0.f;
      else if (a.mode == FMD_STEREO_FORCE_STEREO) target = 1.f;
      else if (!stereo) target = 0.f;
      else if (!a.quality) target = 1.f;
      else {
        const float tq = (a.quality[sb] - a.blend_lo) * a.inv_span;
        target = tq > 0.f ? (tq < 1.f ? tq : 1.f) : 0.f;
      }
      const float d = stc_clamp(target - g, -a.slew, a.slew);
      g = stc_clamp(g + d, 0.f, 1.f);
      step = (g - g0) / (float)frames;
    }
    fmd_stereo_info r;
    r.pilot_ms = q;
    r.g_start = g0;
    r.g_step = step;
    r.g_end = g;
    r.stereo = stereo;
    r.frames = frames;
    r.reserved[0] = r.reserved[1] = 0;
    a.info[sb] = r;
  }
  st->g = g;
  st->stereo = stereo;
  st->run = run;
  st->reserved = 0;
}

/* one frame: its two int16 in a 32-bit word, L low; the meters of the output into the thread's accumulators */
struct stc_acc { int pl, pr, full; unsigned long long sl, sr; };

__device__ __forceinline__ unsigned stc_frame(unsigned w, int i, float g0, float step, stc_acc &m) {
  const float L = (float)(short)(w & 0xffffu), R = (float)(short)(w >> 16);
  const float gi = stc_clamp(__builtin_fmaf((float)(i + 1), step, g0), 0.f, 1.f);
  const float mid = 0.5f * (L + R), sd = 0.5f * (L - R);
  const float lo = stc_clamp(__builtin_rintf(__builtin_fmaf(gi, sd, mid)), -32768.f, 32767.f);
  const float ro = stc_clamp(__builtin_rintf(__builtin_fmaf(-gi, sd, mid)), -32768.f, 32767.f);
  const int li = (int)lo, ri = (int)ro;
  const int al = li < 0 ? -li : li, ar = ri < 0 ? -ri : ri;
  m.pl = al > m.pl ? al : m.pl;
  m.pr = ar > m.pr ? ar : m.pr;
  m.full += (li == -32768 || li == 32767) + (ri == -32768 || ri == 32767);
  m.sl += (unsigned long long)((unsigned)al * (unsigned)al);
  m.sr += (unsigned long long)((unsigned)ar * (unsigned)ar);
  return ((unsigned)li & 0xffffu) | ((unsigned)ri << 16);
}

__global__ __launch_bounds__(STC_NT) void fmd_stereo_apply_kernel(const uint4 *pcm, const fmd_stereo_info *__restrict__ info, int words, uint4 *out,
                                                                  fmd_stereo_meter *__restrict__ meter) {      /* (out may be pcm: neither is restrict) */
  __shared__ int s_pl, s_pr, s_full;
  __shared__ unsigned long long s_sl, s_sr;
  const int t = threadIdx.x;
  const size_t sb = blockIdx.x;
  const fmd_stereo_info r = info[sb];
  int frames = r.frames;                                 /* the tracker's, bounded here as well: no index below depends on a stored value alone */
  frames = frames < 0 ? 0 : (frames > 4 * words ? 4 * words : frames);
  if (t == 0) { s_pl = 0; s_pr = 0; s_full = 0; s_sl = 0ull; s_sr = 0ull; }
  __syncthreads();
  stc_acc m = {0, 0, 0, 0ull, 0ull};
  const uint4 *src = pcm + sb * (size_t)words;
  uint4 *dst = out + sb * (size_t)words;
  for (int w = t; w < words; w += STC_NT) {
    uint4 q = src[w];
    const int i0 = 4 * w;
    if (i0 < frames) q.x = stc_frame(q.x, i0, r.g_start, r.g_step, m);
    if (i0 + 1 < frames) q.y = stc_frame(q.y, i0 + 1, r.g_start, r.g_step, m);
    if (i0 + 2 < frames) q.z = stc_frame(q.z, i0 + 2, r.g_start, r.g_step, m);
    if (i0 + 3 < frames) q.w = stc_frame(q.w, i0 + 3, r.g_start, r.g_step, m);
    dst[w] = q;
  }
  if (!meter) return;
  if (m.pl) atomicMax(&s_pl, m.pl);
  if (m.pr) atomicMax(&s_pr, m.pr);
  if (m.full) atomicAdd(&s_full, m.full);
  if (m.sl) atomicAdd(&s_sl, m.sl);
  if (m.sr) atomicAdd(&s_sr, m.sr);
  __syncthreads();
  if (t == 0) {
    fmd_stereo_meter o;
    o.peak_l = s_pl;
    o.peak_r = s_pr;
    o.full_scale = s_full;
    o.frames = frames;
    o.sumsq_l = s_sl;
    o.sumsq_r = s_sr;
    meter[sb] = o;
  }
}

}  // namespace

extern "C" int fmdk_stereo_launch(const void *d_pcm, const void *d_lens, const void *d_z, const void *d_quality, int n_streams, int n_blocks,
                                  const fmd_stereo_config *c, const fmdk_stereo_k *k, int mode, void *d_state, void *d_out, void *d_info, void *d_meter,
                                  void *stream) {
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned slots = (unsigned)n_streams * (unsigned)n_blocks;
  fmd_stereo_info *info = static_cast<fmd_stereo_info *>(d_info);
  const int has_z = d_z != nullptr && c->pilot_per_block > 0;
  int e;
  if (has_z) {
    hipLaunchKernelGGL(fmd_stereo_pilot_kernel, dim3(slots), dim3(STC_NT), 0, st, static_cast<const float2 *>(d_z), c->pilot_per_block, k->inv_mz, info);
    if ((e = (int)hipGetLastError())) return e;
  }
  stc_track_args a;
  a.lens = static_cast<const int32_t *>(d_lens);
  a.quality = static_cast<const float *>(d_quality);
  a.state = static_cast<fmd_stereo_state *>(d_state);
  a.info = info;
  a.thr_on = k->thr_on;
  a.thr_off = k->thr_off;
  a.blend_lo = c->blend_lo;
  a.inv_span = k->inv_span;
  a.slew = c->slew;
  a.n_blocks = n_blocks;
  a.pcm_stride = c->pcm_stride;
  a.hold_blocks = c->hold_blocks;
  a.mode = mode;
  a.has_z = has_z;
  hipLaunchKernelGGL(fmd_stereo_track_kernel, dim3((unsigned)n_streams), dim3(64), 0, st, a);
  if ((e = (int)hipGetLastError())) return e;
  hipLaunchKernelGGL(fmd_stereo_apply_kernel, dim3(slots), dim3(STC_NT), 0, st, static_cast<const uint4 *>(d_pcm), info, c->pcm_stride / 8,
                     static_cast<uint4 *>(d_out), static_cast<fmd_stereo_meter *>(d_meter));
  return (int)hipGetLastError();
}
