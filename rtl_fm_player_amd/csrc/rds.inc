/* rds.inc - the RDS receiver (fmd_rds_*; include/fmdemod_mi355x.h, "RDS receiver"; DESIGN.md section 5d): included by fmd_kernels_recv.hip, the receivers'
 * translation unit, beside subcarrier.inc.  Kernels of their own over the z an fmd_subc writes; they share nothing with the fused kernel
 * and reference nothing of the host layer.  gfx950, no inline assembly, no atomics, no workgroup that waits for another.
 *
 * Four launches on one stream, feed-forward (the definition and its integers: the header; fmdk_rds_geom: fmd_rds.c):
 *   1. fmd_rds_mf_kernel, one workgroup of 256 threads per (stream, block, chunk of RD_NS = 1024 samples; the last chunk of a block may be shorter).
 *      Stages the chunk's z and the RD_H = 64 samples before it in LDS - from the block before it in the same launch (a stream's blocks are
 *      contiguous), or for the launch's first block from the carried state's last Tg samples; what is older than Tg samples is never used and
 *      never read.  Thread t owns outputs t, t + 256, ...: y = sum_k g[k] z[n-k] as acc = fma(g[k], z, acc) for k = 0 .. Tg-1 from zero - ONE order
 *      for every output, wherever its history came from.  y goes to the object's scratch; p = fma(yi, yi, yr yr) is summed with the timing table,
 *      acc = fma(p, w[n mod Pw], acc) over the thread's outputs in order, then over the 256 threads by a fixed tree (t += t + 128, 64, .. 1) in LDS:
 *      the chunk's partial {Re Tm, Im Tm, sum p}.  The table index is the sample index in integers (carried count + samples of the launch before).
 *   2. fmd_rds_track_kernel, one workgroup per stream, one thread at work: walks the launch's blocks in order - Tm = the chunks' partials summed in
 *      order from zero, Ts = fma(a, Ts, Tm), phi = -atan2f(Im Ts, Re Ts) / (2 pi) put into [-1/2, 1/2), and in integers the block's first bit
 *      and count - into fmdk_rds_blk per block.  It reads the carried state and writes none of it.
 *   3. fmd_rds_slice_kernel, one workgroup per (stream, block), one thread per bit (looping where a block has more than 256): the two linear
 *      interpolations of y at (k + phi) S and (k - 1 + phi) S - y before the block's first sample from the block before it in the scratch, or
 *      for the launch's first block from the carried state's last Hy values - and c = fma(si, pi, sr pr).  The rest of the slot is zeroed.
 *   4. fmd_rds_state_kernel, one workgroup per stream: the state after the launch (last Tg z, last Hy y, sample count mod Pw, Ts, next bit and its
 *      offset).  It is the only writer of fmd_rds_state, behind the slicer that still reads the old y history; the stream orders the four and the
 *      next launch behind them, and a captured graph advances the state on every replay.
 * Instant of a bit, in integers: E = 2375 x (k S - (n0 - L - Hb)) >= 0 for both bits of a pair; q = E / 2375 whole samples and r = E mod 2375;
 * u = fma(phi, S, r / 2375), index q + floor(u) + Hh from the first sample of the y lookback (n0 - Hy), weight u - floor(u) (exact).  By the
 * definition of L, Hb and Hh the two samples lie in [n0 - Hy, n0 + Bz - 2]; the index is clamped to that range all the same. */

namespace {

constexpr int RD_NT = 256;
constexpr int RD_NS = FMDK_RDS_CHUNK;
constexpr int RD_H = FMD_RDS_MAX_TAPS;
constexpr int RD_RO = RD_NS / RD_NT;
static_assert(RD_NS % RD_NT == 0 && RD_H == 64 && FMD_RDS_MAX_YHIST <= RD_NT && RD_H <= RD_NT, "whole outputs per thread; the state kernel copies a history per pass");
static_assert(sizeof(fmd_rds_state) == 32 + 8 * 64 + 8 * FMD_RDS_MAX_YHIST && sizeof(fmdk_rds_blk) == 40, "layouts the kernels index");

__global__ __launch_bounds__(RD_NT) void fmd_rds_mf_kernel(const float2 *__restrict__ z, int n_blocks, int Bz, int Tg, int Pw, int cpb,
                                                           const float *__restrict__ taps, const float2 *__restrict__ w,
                                                           const fmd_rds_state *__restrict__ state, float2 *__restrict__ y, float4 *__restrict__ part) {
  __shared__ float2 x[RD_H + RD_NS];
  __shared__ __attribute__((aligned(16))) float gt[RD_H];
  __shared__ float red[3][RD_NT];

  const int t = threadIdx.x;
  const unsigned wg = blockIdx.x;                       /* (stream, block, chunk), chunk fastest */
  const int c = (int)(wg % (unsigned)cpb);
  const unsigned sb = wg / (unsigned)cpb;               /* stream x n_blocks + block */
  const int b = (int)(sb % (unsigned)n_blocks), s = (int)(sb / (unsigned)n_blocks);
  const int c0 = c * RD_NS;
  const int ns = (Bz - c0) < RD_NS ? (Bz - c0) : RD_NS;
  const float2 *zb = z + (size_t)sb * (size_t)Bz;       /* the block's first sample */
  const fmd_rds_state *st = state + s;

  if (t < RD_H) gt[t] = t < Tg ? taps[t] : 0.f;
  for (int i = t; i < RD_H + ns; i += RD_NT) {
    const int rel = c0 - RD_H + i;                      /* relative to the block's first sample; < Bz */
    float2 q = float2{0.f, 0.f};
    if (rel + Tg >= 0) {                                /* (older than Tg samples: never used, never read) */
      if (rel >= 0 || b > 0) q = zb[rel];               /* rel >= -Tg >= -Bz: this block or the one before it */
      else q = float2{st->zhist[Tg + rel][0], st->zhist[Tg + rel][1]};
    }
    x[i] = q;
  }
  __syncthreads();

  /* the table index of the chunk's first sample (the host keeps n_blocks Bz below 2^31) */
  const unsigned p0 = ((unsigned)st->phase + (unsigned)b * (unsigned)Bz + (unsigned)c0) % (unsigned)Pw;
  float are = 0.f, aim = 0.f, apw = 0.f;
#pragma unroll
  for (int r = 0; r < RD_RO; r++) {
    const int o = t + r * RD_NT;
    if (o < ns) {
      float yr = 0.f, yi = 0.f;
      const float2 *xo = x + RD_H + o;
      for (int k4 = 0; k4 < Tg; k4 += 4) {              /* Tg is a multiple of 4 */
        const float4 g4 = *reinterpret_cast<const float4 *>(gt + k4);
        const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const float2 u = xo[-(k4 + e)];
          yr = __builtin_fmaf(g[e], u.x, yr);
          yi = __builtin_fmaf(g[e], u.y, yi);
        }
      }
      y[(size_t)sb * (size_t)Bz + (size_t)(c0 + o)] = float2{yr, yi};
      const float p = __builtin_fmaf(yi, yi, yr * yr);
      const float2 ww = w[(p0 + (unsigned)o) % (unsigned)Pw];
      are = __builtin_fmaf(p, ww.x, are);
      aim = __builtin_fmaf(p, ww.y, aim);
      apw = apw + p;
    }
  }
  red[0][t] = are; red[1][t] = aim; red[2][t] = apw;
  __syncthreads();
  for (int h = RD_NT / 2; h > 0; h >>= 1) {
    if (t < h) {
      red[0][t] = red[0][t] + red[0][t + h];
      red[1][t] = red[1][t] + red[1][t + h];
      red[2][t] = red[2][t] + red[2][t + h];
    }
    __syncthreads();
  }
  if (t == 0) part[(size_t)sb * (size_t)cpb + (size_t)c] = float4{red[0][0], red[1][0], red[2][0], 0.f};
}

__global__ __launch_bounds__(64) void fmd_rds_track_kernel(int n_blocks, int Bz, int cpb, float a, fmdk_rds_geom g, const float4 *__restrict__ part,
                                                           const fmd_rds_state *__restrict__ state, fmdk_rds_blk *__restrict__ blk) {
  if (threadIdx.x != 0) return;
  const int s = blockIdx.x;
  const fmd_rds_state *st = state + s;
  float tsr = st->ts[0], tsi = st->ts[1];
  int e = st->frac + FMDK_RDS_Q * g.lb;                 /* 2375 x (next bit's instant - (n0 - L)), in [0, 2 rate_z) */
  long long bit = st->bit;
  const int lim = FMDK_RDS_Q * Bz;
  for (int b = 0; b < n_blocks; b++) {
    const size_t sb = (size_t)s * (size_t)n_blocks + (size_t)b;
    float tr = 0.f, ti = 0.f, pw = 0.f;
    for (int c = 0; c < cpb; c++) {
      const float4 p = part[sb * (size_t)cpb + (size_t)c];
      tr = tr + p.x; ti = ti + p.y; pw = pw + p.z;
    }
    tsr = __builtin_fmaf(a, tsr, tr);
    tsi = __builtin_fmaf(a, tsi, ti);
    float phi = -atan2f(tsi, tsr) * 0.15915494309189535f;
    if (!(phi < 0.5f) || phi < -0.5f) phi = -0.5f;
    const int count = e < lim ? (lim - e + g.two_rz - 1) / g.two_rz : 0;
    fmdk_rds_blk o;
    o.ts[0] = tsr; o.ts[1] = tsi; o.phi = phi; o.pw = pw; o.tm[0] = tr; o.tm[1] = ti;
    o.count = count; o.e0 = e + FMDK_RDS_Q * g.hb; o.first = bit;
    blk[sb] = o;
    bit += count;
    e = e + count * g.two_rz - lim;
  }
}

__global__ __launch_bounds__(RD_NT) void fmd_rds_slice_kernel(int n_blocks, int Bz, float Sf, fmdk_rds_geom g, const float2 *__restrict__ y,
                                                              const fmd_rds_state *__restrict__ state, const fmdk_rds_blk *__restrict__ blk,
                                                              float *__restrict__ soft, int32_t *__restrict__ lens, long long *__restrict__ first,
                                                              float4 *__restrict__ est) {
  const int t = threadIdx.x;
  const unsigned sb = blockIdx.x;
  const int b = (int)(sb % (unsigned)n_blocks), s = (int)(sb / (unsigned)n_blocks);
  const fmd_rds_state *st = state + s;
  const fmdk_rds_blk bi = blk[sb];
  const float2 *yb = y + (size_t)sb * (size_t)Bz;
  const int top = g.hy + Bz - 2;                        /* the last index a pair may start at */
  const int count = bi.count < g.slot ? bi.count : g.slot;
  for (int j = t; j < g.slot; j += RD_NT) {
    float c = 0.f;
    if (j < count) {
      float sr[2], si[2];
#pragma unroll
      for (int m = 0; m < 2; m++) {                     /* bit k, then bit k - 1 */
        const int E = bi.e0 + (j - m) * g.two_rz;       /* >= 0: e0 >= 2375 Hb >= 2 rate_z */
        const int q = E / FMDK_RDS_Q, r = E - q * FMDK_RDS_Q;
        const float frac = (float)r * (1.0f / 2375.0f);
        const float u = __builtin_fmaf(bi.phi, Sf, frac);
        const float fl = floorf(u);
        const float mu = u - fl;
        int idx = q + (int)fl + g.hh;
        idx = idx < 0 ? 0 : (idx > top ? top : idx);
        float2 v[2];
#pragma unroll
        for (int d = 0; d < 2; d++) {
          const int rel = idx + d - g.hy;               /* relative to the block's first sample: -Hy .. Bz - 1 */
          if (rel >= 0 || b > 0) v[d] = yb[rel];        /* rel >= -Hy >= -Bz: this block or the one before it */
          else v[d] = float2{st->yhist[idx + d][0], st->yhist[idx + d][1]};
        }
        sr[m] = __builtin_fmaf(mu, v[1].x - v[0].x, v[0].x);
        si[m] = __builtin_fmaf(mu, v[1].y - v[0].y, v[0].y);
      }
      c = __builtin_fmaf(si[0], si[1], sr[0] * sr[1]);
    }
    soft[(size_t)sb * (size_t)g.slot + (size_t)j] = c;
  }
  if (t == 0) {
    lens[sb] = count;
    if (first) first[sb] = bi.first;
    if (est) est[sb] = float4{bi.ts[0], bi.ts[1], bi.phi, bi.pw};
  }
}

/* behind the slicer on the same stream: the state after the launch.  Bz >= Tg and Bz >= Hy, so both histories lie in the launch's last block. */
__global__ __launch_bounds__(RD_NT) void fmd_rds_state_kernel(const float2 *__restrict__ z, const float2 *__restrict__ y, int n_blocks, int Bz, int Tg,
                                                              fmdk_rds_geom g, const fmdk_rds_blk *__restrict__ blk, fmd_rds_state *state) {
  const int s = blockIdx.x, t = threadIdx.x;
  const size_t last = (size_t)s * (size_t)n_blocks + (size_t)(n_blocks - 1);
  fmd_rds_state *st = state + s;
  if (t < Tg) {
    const float2 v = z[last * (size_t)Bz + (size_t)(Bz - Tg + t)];
    st->zhist[t][0] = v.x; st->zhist[t][1] = v.y;
  }
  if (t < g.hy) {
    const float2 v = y[last * (size_t)Bz + (size_t)(Bz - g.hy + t)];
    st->yhist[t][0] = v.x; st->yhist[t][1] = v.y;
  }
  if (t == 0) {
    const fmdk_rds_blk bi = blk[last];
    st->phase = (int32_t)(((long long)st->phase + (long long)n_blocks * Bz) % g.pw);
    st->ts[0] = bi.ts[0]; st->ts[1] = bi.ts[1];
    st->bit = bi.first + bi.count;
    st->frac = bi.e0 - FMDK_RDS_Q * g.hb + bi.count * g.two_rz - FMDK_RDS_Q * Bz - FMDK_RDS_Q * g.lb;
  }
}

}  // namespace

extern "C" int fmdk_rds_launch(const void *d_z, int n_streams, int n_blocks, const fmd_rds_config *c, const fmdk_rds_geom *g, const float *d_taps,
                               const float *d_w, void *d_state, void *d_y, void *d_part, void *d_blk, void *d_soft, void *d_lens, void *d_first,
                               void *d_est, void *stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int Bz = c->block_z, cpb = (Bz + RD_NS - 1) / RD_NS;
  const unsigned slots = (unsigned)n_streams * (unsigned)n_blocks;      /* (the host has checked that the grids stay below 2^31) */
  const float a = (float)(1.0 - 1.0 / (double)c->avg_blocks);
  const float Sf = (float)((double)g->two_rz / (double)FMDK_RDS_Q);
  const float2 *z = static_cast<const float2 *>(d_z);
  float2 *y = static_cast<float2 *>(d_y);
  const fmd_rds_state *state = static_cast<const fmd_rds_state *>(d_state);
  fmdk_rds_blk *blk = static_cast<fmdk_rds_blk *>(d_blk);
  hipLaunchKernelGGL(fmd_rds_mf_kernel, dim3(slots * (unsigned)cpb), dim3(RD_NT), 0, st, z, n_blocks, Bz, c->n_taps, g->pw, cpb, d_taps,
                     reinterpret_cast<const float2 *>(d_w), state, y, static_cast<float4 *>(d_part));
  int e = (int)hipGetLastError();
  if (e) return e;
  hipLaunchKernelGGL(fmd_rds_track_kernel, dim3((unsigned)n_streams), dim3(64), 0, st, n_blocks, Bz, cpb, a, *g, static_cast<const float4 *>(d_part), state, blk);
  if ((e = (int)hipGetLastError())) return e;
  hipLaunchKernelGGL(fmd_rds_slice_kernel, dim3(slots), dim3(RD_NT), 0, st, n_blocks, Bz, Sf, *g, y, state, blk, static_cast<float *>(d_soft),
                     static_cast<int32_t *>(d_lens), static_cast<long long *>(d_first), static_cast<float4 *>(d_est));
  if ((e = (int)hipGetLastError())) return e;
  hipLaunchKernelGGL(fmd_rds_state_kernel, dim3((unsigned)n_streams), dim3(RD_NT), 0, st, z, y, n_blocks, Bz, c->n_taps, *g, blk,
                     static_cast<fmd_rds_state *>(d_state));
  return (int)hipGetLastError();
}
