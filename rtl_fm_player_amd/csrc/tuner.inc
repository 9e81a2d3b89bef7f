/* tuner.inc - the channel tuner (fmd_tuner_*; include/fmdemod_mi355x.h, "Channel tuner"): included by fmd_kernels_recv.hip, the receivers' translation
 * unit, beside subcarrier.inc.  Kernels of their own: they share nothing with the fused kernel but the layout of d_iq, and reference
 * nothing of the host layer.  gfx950, no inline assembly, no atomics.
 *
 * For one source, x[n] = its samples since the last reset (zero before it), P the table's period, channel {source, shift, gain}, T taps h:
 *   m[n] = x[n] c[(n shift) mod P],   y[n] = sum_{k=0}^{T-1} h[k] m[n-k],   code = clamp(rint(fma(128 gain, y, 127.5)), 0, 255) per component.
 *
 * Decomposition.  One workgroup of 256 threads per (channel, block, chunk of TN_NS = 4096 samples of the block; the last chunk of a block may be
 * shorter - a whole number of 16-byte words always, as block_len is a multiple of 16).  The workgroup
 *   1. loads the chunk's bytes and the TN_H = 64 samples before them as 16-byte words of 8 samples (coalesced).  Samples before the block's first come
 *      from the block before it in the same launch - a source's blocks are contiguous in d_iq - or, for the launch's first block, from the carried
 *      state's last T byte pairs (zero values after a reset).  What is older than T samples is set to zero and, in the state, never read;
 *   2. converts and mixes each sample ONCE into LDS as complex float.  The table index of a thread's first word costs the thread one integer
 *      remainder, (qb + t sh8) mod P with qb the workgroup's; from there it steps by sh and wraps, and by sh2k to the thread's next word;
 *   3. runs the real-tap FIR.  Thread t owns the 8 ADJACENT outputs 8t .. 8t + 7 of each half of the chunk: it walks the staged samples backwards a
 *      word (an LDS column) at a time, and each value it reads feeds the 8 accumulator pairs with 8 different taps - 16 FMAs per 8-byte LDS read.
 *      For output j the taps come in the order k = 0 .. T-1 from zero: ONE order for every output, wherever its history came from - the values
 *      are in LDS either way - so a split into calls, blocks or chunks cannot show in the bits.  Taps from LDS as 16-byte broadcast reads, the tap
 *      array padded with zeros on both sides (a zero tap adds +0 to an accumulator that is never -0: it changes no bit);
 *   4. quantises and stores 16 bytes per thread and half, consecutive threads to consecutive addresses (and, on request, y as 4 x 16 bytes).
 * LDS layout.  Staged sample i (i = 0 is the oldest) lives at [i mod 8][i / 8], rows an odd number of values long: the threads of a wave read
 * CONSECUTIVE 8-byte values of one row for every tap (no bank conflict), the 8 rows of a column at immediate offsets from one address, and step 2
 * stores a word as one value in each row.  8 x 521 x 8 bytes = 33 344 bytes and 384 of taps: four workgroups per CU.
 *
 * State.  The tuner kernel only READS fmd_tuner_state (count, valid, hist); a second, small kernel behind it on the same stream - one workgroup per
 * source - writes the last T byte pairs of the launch's last block into hist, advances count by n_blocks L mod P and sets valid.  The stream orders
 * the two, and the next launch behind them: no workgroup waits for another, and a captured graph advances the state on every replay. */

namespace {

constexpr int TN_NT = 256;
constexpr int TN_NS = FMDK_TUNER_CHUNK;      /* samples per chunk */
constexpr int TN_H = FMD_TUNER_MAX_TAPS;     /* history samples staged before a chunk, whatever T */
constexpr int TN_W = 8;                      /* samples per 16-byte word = adjacent outputs per thread = LDS rows */
constexpr int TN_ROWS = ((TN_H + TN_NS) / TN_W) | 1;     /* values per LDS row: odd */
constexpr int TN_HALVES = TN_NS / (TN_W * TN_NT);        /* output words per thread and chunk */
constexpr int TN_HT = 8 + FMD_TUNER_MAX_TAPS + 24;       /* 8 zeros, the taps, zeros up to the last 16-tap window's end */
static_assert(TN_HALVES == 2 && TN_H == 64 && TN_H % TN_W == 0 && sizeof(fmd_tuner_state) == 144, "two output words per thread; whole history columns; hist at byte 16");
static_assert(sizeof(fmdk_tuner_chan) == 32, "the channel table's entry");

/* one column of staged samples s[e] (e = its row) into the 8 outputs: output j takes s[e] with tap k = 8 g + j - e = window entry 8 + j - e; e
 * descends so that k ascends per output.  FIRST (g = 0): the taps below 0 are not there (j >= e only).  The taps from T on, in the last column, are
 * zeros of the padding: skipping them where T is a multiple of 8 was measured and is no faster (DESIGN.md section 5e). */
template <bool FIRST>
__device__ __forceinline__ void tn_column(const float (&hh)[16], const float2 *__restrict__ xc, float (&ar)[TN_W], float (&ai)[TN_W]) {
  float2 s[TN_W];
#pragma unroll
  for (int e = 0; e < TN_W; e++) s[e] = xc[e * TN_ROWS];
#pragma unroll
  for (int e = TN_W - 1; e >= 0; e--)
#pragma unroll
    for (int j = 0; j < TN_W; j++)
      if (!FIRST || j >= e) {
        ar[j] = __builtin_fmaf(hh[8 + j - e], s[e].x, ar[j]);
        ai[j] = __builtin_fmaf(hh[8 + j - e], s[e].y, ai[j]);
      }
}

__device__ __forceinline__ unsigned tn_code(float g, float v) {
  const float q = __builtin_rintf(__builtin_fmaf(g, v, 127.5f));      /* ties to even */
  return (unsigned)__builtin_fminf(__builtin_fmaxf(q, 0.f), 255.f);
}

__global__ __launch_bounds__(TN_NT) void fmd_tuner_kernel(const uint8_t *__restrict__ iq, int n_blocks, int block_len, int T, int P, int bias, int cpb,
                                                          const float *__restrict__ taps, const float2 *__restrict__ car,
                                                          const fmdk_tuner_chan *__restrict__ chan, const fmd_tuner_state *__restrict__ state,
                                                          uint8_t *__restrict__ out, float2 *__restrict__ y) {
  __shared__ float2 x[TN_W * TN_ROWS];
  __shared__ __attribute__((aligned(16))) float ht[TN_HT];

  const int t = threadIdx.x;
  const unsigned wg = blockIdx.x;                       /* (channel, block, chunk), chunk fastest */
  const int c = (int)(wg % (unsigned)cpb);
  const unsigned cb = wg / (unsigned)cpb;               /* channel x n_blocks + block */
  const int b = (int)(cb % (unsigned)n_blocks), ch = (int)(cb / (unsigned)n_blocks);
  const fmdk_tuner_chan cc = chan[ch];
  const int L = block_len >> 1;
  const int c0 = c * TN_NS;
  const int ns = (L - c0) < TN_NS ? (L - c0) : TN_NS;   /* this chunk's samples: a multiple of 8 */
  const uint8_t *src = iq + ((size_t)cc.source * (size_t)n_blocks + (size_t)b) * (size_t)block_len;      /* the block's first byte */
  const fmd_tuner_state *st = state + cc.source;
  const int have = st->valid;

  if (t < TN_HT) ht[t] = (t >= 8 && t < 8 + T) ? taps[t - 8] : 0.f;

  /* the table index of staged sample 0 = sample b L + c0 - TN_H of the launch (bias: a multiple of P, >= TN_H; the host keeps n_blocks L well below 2^31) */
  const unsigned n0 = (unsigned)st->count + (unsigned)b * (unsigned)L + (unsigned)(c0 - TN_H + bias);
  const unsigned qb = ((n0 % (unsigned)P) * (unsigned)cc.sh) % (unsigned)P;
  unsigned idx = (qb + (unsigned)t * (unsigned)cc.sh8) % (unsigned)P;         /* ... of this thread's first word */

  const int nw = (TN_H + ns) >> 3;
  for (int w = t; w < nw; w += TN_NT) {
    const int rel = c0 - TN_H + TN_W * w;               /* first sample of the word, relative to the block's first: a multiple of 8 */
    bool lo = rel >= -T, hi = rel + 4 >= -T;            /* its two halves: within T samples of the block's first (T is a multiple of 4) */
    uint4 q = uint4{0u, 0u, 0u, 0u};
    if (hi) {
      if (rel >= 0 || b > 0) {                          /* this block, or the one before it: -rel <= the next multiple of 8 from T <= L */
        q = *reinterpret_cast<const uint4 *>(src + 2 * rel);
      } else if (have) {                                /* the carried state: hist[T + rel ..], 8-byte halves */
        const uint8_t *hp = &st->hist[0][0] + 2 * (T + rel);
        uint2 a = uint2{0u, 0u};
        if (lo) a = *reinterpret_cast<const uint2 *>(hp);
        const uint2 d = *reinterpret_cast<const uint2 *>(hp + 8);
        q = uint4{a.x, a.y, d.x, d.y};
      } else {
        lo = hi = false;                                /* after a reset: zero values */
      }
    }
    const unsigned wd[4] = {q.x, q.y, q.z, q.w};
    float2 *o = x + w;
    unsigned p = idx;
#pragma unroll
    for (int e = 0; e < TN_W; e++) {
      const unsigned d = wd[e >> 1] >> (16 * (e & 1));
      const float xr = ((float)(d & 255u) - 127.5f) * 0.0078125f;
      const float xi = ((float)((d >> 8) & 255u) - 127.5f) * 0.0078125f;
      const float2 cv = car[p];
      const float pr = xi * cv.y, pi = xi * cv.x;       /* one rounded product, then one fused multiply-add */
      const float re = __builtin_fmaf(xr, cv.x, -pr), im = __builtin_fmaf(xr, cv.y, pi);
      const bool ok = e < 4 ? lo : hi;
      o[e * TN_ROWS] = ok ? float2{re, im} : float2{0.f, 0.f};
      p += (unsigned)cc.sh;
      p = p >= (unsigned)P ? p - (unsigned)P : p;
    }
    idx += (unsigned)cc.sh2k;
    idx = idx >= (unsigned)P ? idx - (unsigned)P : idx;
  }
  __syncthreads();

  /* output j of half r is staged sample TN_H + 8 (t + 256 r) + j: column 8 + t + 256 r, row j; column group g lies g columns before it */
  float ar[TN_HALVES][TN_W], ai[TN_HALVES][TN_W];
#pragma unroll
  for (int r = 0; r < TN_HALVES; r++)
#pragma unroll
    for (int j = 0; j < TN_W; j++) { ar[r][j] = 0.f; ai[r][j] = 0.f; }
  const bool second = ns > TN_W * TN_NT;                /* uniform: the chunk reaches into its second half */
  const float2 *xc = x + (TN_H / TN_W + t);
  const int ng = (T + 6) >> 3;                          /* the last column group that holds a tap below T */
  for (int g = 0; g <= ng; g++) {
    float hh[16];                                       /* window entry i = tap 8 g - 8 + i */
#pragma unroll
    for (int i4 = 0; i4 < 4; i4++) {
      const float4 h4 = *reinterpret_cast<const float4 *>(ht + 8 * g + 4 * i4);
      hh[4 * i4] = h4.x; hh[4 * i4 + 1] = h4.y; hh[4 * i4 + 2] = h4.z; hh[4 * i4 + 3] = h4.w;
    }
    if (g == 0) {
      tn_column<true>(hh, xc, ar[0], ai[0]);
      if (second) tn_column<true>(hh, xc + TN_NT, ar[1], ai[1]);
    } else {
      tn_column<false>(hh, xc - g, ar[0], ai[0]);
      if (second) tn_column<false>(hh, xc + TN_NT - g, ar[1], ai[1]);
    }
  }

#pragma unroll
  for (int r = 0; r < TN_HALVES; r++) {
    const int o0 = TN_W * (t + r * TN_NT);
    if (o0 < ns) {
      const size_t so = (size_t)cb * (size_t)L + (size_t)(c0 + o0);      /* complex sample index in [n_channels][n_blocks][L] */
      unsigned pk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < TN_W; j++) pk[j >> 1] |= (tn_code(cc.g, ar[r][j]) | (tn_code(cc.g, ai[r][j]) << 8)) << (16 * (j & 1));
      *reinterpret_cast<uint4 *>(out + 2 * so) = uint4{pk[0], pk[1], pk[2], pk[3]};
      if (y) {
        float4 *yo = reinterpret_cast<float4 *>(y + so);
#pragma unroll
        for (int j = 0; j < TN_W; j += 2) yo[j >> 1] = float4{ar[r][j], ai[r][j], ar[r][j + 1], ai[r][j + 1]};
      }
    }
  }
}

/* behind the tuner kernel on the same stream: the state after the launch.  L >= T, so the last T samples lie in the launch's last block. */
__global__ __launch_bounds__(2 * FMD_TUNER_MAX_TAPS) void fmd_tuner_state_kernel(const uint8_t *__restrict__ iq, int n_blocks, int block_len, int T, int P,
                                                                                 fmd_tuner_state *state) {
  const int s = blockIdx.x, t = threadIdx.x;
  const uint8_t *last = iq + ((size_t)s * (size_t)n_blocks + (size_t)(n_blocks - 1)) * (size_t)block_len + (size_t)(block_len - 2 * T);
  fmd_tuner_state *st = state + s;
  if (t < 2 * T) (&st->hist[0][0])[t] = last[t];
  if (t == 0) {
    st->count = (int32_t)(((long long)st->count + (long long)n_blocks * (block_len >> 1)) % P);
    st->valid = 1;
  }
}

}  // namespace

extern "C" int fmdk_tuner_launch(const void *d_iq, int n_sources, int n_channels, int n_blocks, const fmd_tuner_config *c, const float *d_taps,
                                 const float *d_table, const void *d_chan, void *d_state, void *d_out, void *d_y, void *stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int L = c->block_len >> 1, cpb = (L + TN_NS - 1) / TN_NS, P = c->rate / c->step_hz;
  const int bias = P * ((TN_H + P - 1) / P);
  const unsigned grid = (unsigned)n_channels * (unsigned)n_blocks * (unsigned)cpb;         /* (the host has checked that it stays below 2^31) */
  hipLaunchKernelGGL(fmd_tuner_kernel, dim3(grid), dim3(TN_NT), 0, st, static_cast<const uint8_t *>(d_iq), n_blocks, c->block_len, c->n_taps, P, bias, cpb,
                     d_taps, reinterpret_cast<const float2 *>(d_table), static_cast<const fmdk_tuner_chan *>(d_chan),
                     static_cast<const fmd_tuner_state *>(d_state), static_cast<uint8_t *>(d_out), static_cast<float2 *>(d_y));
  int e = (int)hipGetLastError();
  if (e) return e;
  hipLaunchKernelGGL(fmd_tuner_state_kernel, dim3((unsigned)n_sources), dim3(2 * FMD_TUNER_MAX_TAPS), 0, st, static_cast<const uint8_t *>(d_iq), n_blocks,
                     c->block_len, c->n_taps, P, static_cast<fmd_tuner_state *>(d_state));
  return (int)hipGetLastError();
}
