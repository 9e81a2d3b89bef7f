/* subcarrier.inc - the MPX subcarrier receiver (fmd_subc_*; include/fmdemod_mi355x.h, "MPX subcarrier receiver"): included by fmd_kernels_recv.hip,
 * the receivers' translation unit, beside levels.inc and spectrum.inc.  Kernels of their own: they share nothing with the fused kernel but the
 * layout of the `v` debug tap, and reference nothing of the host layer.  gfx950, no inline assembly, no atomics.
 *
 * For one stream, v[n] = all its blocks since the last reset (zero before it), T taps h, decimation D, carrier period Pd = R / gcd(fc, R):
 *   z[m] = sum_{k=0}^{T-1} h[k] * ( v[n] * c[n mod Pd] ),  n = mD + D-1-k,   c[p] = 2 exp(-2 pi i ((p fc) mod R) / R)  (the host's float table).
 *
 * Decomposition.  The FIR has no feedback, so every (stream, block, chunk) is independent given v: one workgroup of 256 threads each, a chunk being
 * SC_NS = 4096 input samples of a block (the last chunk of a block may be shorter; a whole number of outputs always, as D divides M).  The workgroup
 *   1. loads the chunk's samples and the SC_H = 256 before them as 16-byte words (coalesced).  Samples before the block's first come from the block
 *      before it in the same launch - the blocks of a stream are contiguous in d_v - or, for the launch's first block, from the carried state's last T
 *      samples; what is older than T samples is never used by the filter and reads as zero, so nothing is read that the caller did not provide;
 *   2. mixes each sample ONCE with its table entry, x = v * c (one rounding per component), and stores the complex value to LDS.  The table index of
 *      the chunk's first word is (carried sample count + samples of the launch before it) mod Pd in integers; within a word it steps and wraps;
 *   3. runs the real-tap FIR over the complex values: thread t owns outputs t, t + 256, ... of the chunk (16 / D of them, one for D >= 16), taps
 *      from LDS as 16-byte broadcast reads, acc = fma(h[k], x, acc) for k = 0 .. T-1 from zero: ONE order for every output, wherever its history
 *      came from - the values are in LDS either way - so a split into calls, blocks or chunks cannot show in the bits;
 *   4. stores the outputs as float2, consecutive threads to consecutive addresses.
 * LDS layout.  Sample i of the staged range (i = 0 is the oldest) lives at [i mod D][i / D]: output o, tap k reads i = oD + q, q = SC_H + D-1-k, so the
 * threads of a wave read CONSECUTIVE 8-byte values of row q mod D (no bank conflict for any D), and within a group of D taps the row changes by a
 * compile-time offset while the column stays: one address per group, immediate offsets for its D reads.  Rows are an odd number of values long, which
 * spreads step 2's stores (four rows per thread) over the banks.
 *
 * State.  The receiver kernel only READS fmd_subc_state (phase, hist); a second, small kernel behind it on the same stream - one workgroup per
 * stream - writes the last T samples of the launch's last block into hist and advances phase by n_blocks M mod Pd.  The stream orders the two, and
 * the next launch behind them: no workgroup waits for another, and a captured graph advances the state on every replay. */

namespace {

constexpr int SC_NT = 256;
constexpr int SC_NS = FMDK_SUBC_CHUNK;       /* input samples per chunk */
constexpr int SC_H = FMD_SUBC_MAX_TAPS;      /* history samples staged before a chunk, whatever T */
static_assert(SC_NS % (4 * SC_NT) == 0 && SC_H % 32 == 0 && SC_H == 256, "whole words per thread, whole columns for every D; fmd_subc_state.hist has 256 values");

template <int D> constexpr int sc_rows() { return ((SC_H + SC_NS) / D) | 1; }          /* values per LDS row: odd */
template <int D> constexpr int sc_outs() { return SC_NS / D > SC_NT ? SC_NS / D / SC_NT : 1; }   /* outputs per thread and chunk */
constexpr int SC_LDS = (SC_H + SC_NS) + 32;  /* >= D x sc_rows<D>() for D = 4 .. 32 */

template <int D>
__global__ __launch_bounds__(SC_NT) void fmd_subc_kernel(const float *__restrict__ v, int n_blocks, int M, int T, int Pd, int bias, int cpb,
                                                         const float *__restrict__ taps, const float2 *__restrict__ car,
                                                         const fmd_subc_state *__restrict__ state, float2 *__restrict__ z) {
  constexpr int ROWS = sc_rows<D>(), RO = sc_outs<D>();
  static_assert(D * ROWS <= SC_LDS && (D & (D - 1)) == 0 && D >= 4, "the staged range fits; D a power of two, whole 16-byte words per row step");
  __shared__ float2 x[SC_LDS];
  __shared__ __attribute__((aligned(16))) float ht[FMD_SUBC_MAX_TAPS];

  const int t = threadIdx.x;
  const unsigned wg = blockIdx.x;                       /* (stream, block, chunk), chunk fastest */
  const int c = (int)(wg % (unsigned)cpb);
  const unsigned sb = wg / (unsigned)cpb;               /* stream x n_blocks + block */
  const int b = (int)(sb % (unsigned)n_blocks), s = (int)(sb / (unsigned)n_blocks);
  const int c0 = c * SC_NS;
  const int ns = (M - c0) < SC_NS ? (M - c0) : SC_NS;   /* this chunk's samples: a multiple of D (and of 4) */
  const float *vb = v + (size_t)sb * (size_t)M;         /* the block's first sample */
  const fmd_subc_state *st = state + s;

  /* the table index of staged sample 0 = sample b M + c0 - SC_H of the launch (bias: a multiple of Pd, >= SC_H) */
  const unsigned n0 = (unsigned)st->phase + (unsigned)b * (unsigned)M + (unsigned)(c0 - SC_H + bias);     /* (the host keeps n_blocks M well below 2^31) */
  const int p0 = (int)(n0 % (unsigned)Pd);

  if (t < T) ht[t] = taps[t];

  const int nw = (SC_H + ns) >> 2;
  for (int w = t; w < nw; w += SC_NT) {
    const int rel = c0 - SC_H + 4 * w;                  /* first sample of the word, relative to the block's first: a multiple of 4 */
    float4 q = float4{0.f, 0.f, 0.f, 0.f};
    if (rel + T >= 0) {                                 /* (older than T samples: never used, never read) */
      if (rel >= 0 || b > 0) q = *reinterpret_cast<const float4 *>(vb + rel);        /* rel >= -T >= -M: this block or the one before it */
      else q = *reinterpret_cast<const float4 *>(st->hist + (T + rel));              /* the carried state: hist[T + rel .. T + rel + 3], rel <= -4 */
    }
    unsigned p = (unsigned)(p0 + 4 * w) % (unsigned)Pd;
    const float ve[4] = {q.x, q.y, q.z, q.w};
    float2 *o = x + ((4 * w) & (D - 1)) * ROWS + ((4 * w) / D);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float2 cc = car[p];
      o[e * ROWS] = float2{ve[e] * cc.x, ve[e] * cc.y};
      p = p + 1 == (unsigned)Pd ? 0u : p + 1;
    }
  }
  __syncthreads();

  const int no = ns / D;                                /* outputs of this chunk: >= 1 */
  float ar[RO], ai[RO];
  int oc[RO];
#pragma unroll
  for (int r = 0; r < RO; r++) {
    ar[r] = 0.f; ai[r] = 0.f;
    const int o = t + r * SC_NT;
    oc[r] = o < no ? o : no - 1;                        /* past a short chunk's end: computed on the last output's values, not stored */
  }
  /* taps k = g D + e: q = SC_H + D-1-k -> row D-1-e, column SC_H / D - g (+ the output's) */
  for (int g = 0; g * D < T; g++) {
    const float *hg = ht + g * D;
    const int col = SC_H / D - g;
#pragma unroll
    for (int e4 = 0; e4 < D; e4 += 4) {
      if (g * D + e4 < T) {                             /* uniform; T is a multiple of 4 */
        const float4 h4 = *reinterpret_cast<const float4 *>(hg + e4);
        const float h[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
          for (int r = 0; r < RO; r++) {
            const float2 u = x[(D - 1 - (e4 + e)) * ROWS + col + oc[r]];
            ar[r] = __builtin_fmaf(h[e], u.x, ar[r]);
            ai[r] = __builtin_fmaf(h[e], u.y, ai[r]);
          }
      }
    }
  }
  float2 *zo = z + (size_t)sb * (size_t)(M / D) + (size_t)(c0 / D);
#pragma unroll
  for (int r = 0; r < RO; r++) {
    const int o = t + r * SC_NT;
    if (o < no) zo[o] = float2{ar[r], ai[r]};
  }
}

/* behind the receiver kernel on the same stream: the state after the launch.  M >= T, so the last T samples lie in the launch's last block. */
__global__ __launch_bounds__(SC_NT) void fmd_subc_state_kernel(const float *__restrict__ v, int n_blocks, int M, int T, int Pd, fmd_subc_state *state) {
  const int s = blockIdx.x, t = threadIdx.x;
  const float *last = v + ((size_t)s * (size_t)n_blocks + (size_t)(n_blocks - 1)) * (size_t)M + (size_t)(M - T);
  fmd_subc_state *st = state + s;
  if (t < T) st->hist[t] = last[t];
  if (t == 0) st->phase = (int32_t)(((long long)st->phase + (long long)n_blocks * M) % Pd);
}

template <int D>
int sc_launch(const void *d_v, int n_streams, int n_blocks, const fmd_subc_config *c, int period, const float *d_taps, const float *d_carrier,
              void *d_state, void *d_z, hipStream_t st) {
  const int M = c->block_samples, cpb = (M + SC_NS - 1) / SC_NS;
  const int bias = period * ((SC_H + period - 1) / period);
  const unsigned grid = (unsigned)n_streams * (unsigned)n_blocks * (unsigned)cpb;       /* (the host has checked that it stays below 2^31) */
  hipLaunchKernelGGL(fmd_subc_kernel<D>, dim3(grid), dim3(SC_NT), 0, st, static_cast<const float *>(d_v), n_blocks, M, c->n_taps, period, bias, cpb, d_taps,
                     reinterpret_cast<const float2 *>(d_carrier), static_cast<const fmd_subc_state *>(d_state), static_cast<float2 *>(d_z));
  int e = (int)hipGetLastError();
  if (e) return e;
  hipLaunchKernelGGL(fmd_subc_state_kernel, dim3((unsigned)n_streams), dim3(SC_NT), 0, st, static_cast<const float *>(d_v), n_blocks, M, c->n_taps, period,
                     static_cast<fmd_subc_state *>(d_state));
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int fmdk_subc_launch(const void *d_v, int n_streams, int n_blocks, const fmd_subc_config *c, int period, const float *d_taps,
                                const float *d_carrier, void *d_state, void *d_z, void *stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (c->decim) {
    case 4: return sc_launch<4>(d_v, n_streams, n_blocks, c, period, d_taps, d_carrier, d_state, d_z, st);
    case 8: return sc_launch<8>(d_v, n_streams, n_blocks, c, period, d_taps, d_carrier, d_state, d_z, st);
    case 16: return sc_launch<16>(d_v, n_streams, n_blocks, c, period, d_taps, d_carrier, d_state, d_z, st);
    case 32: return sc_launch<32>(d_v, n_streams, n_blocks, c, period, d_taps, d_carrier, d_state, d_z, st);
  }
  return (int)hipErrorInvalidValue;
}
