/* spectrum.inc - the capture spectrum (fmd_batch_spectrum_device / _host; include/fmdemod_mi355x.h, "Capture spectrum"): included by
 * fmd_kernels_recv.hip, the receivers' translation unit, beside levels.inc.  A kernel of its own: it shares nothing with the fused kernel
 * but the d_iq layout, and is no part of a batch's launch sequence.  gfx950, no inline assembly, no atomics.
 *
 * Block b of stream s holds L = block_len / 2 samples x[n] = (I - 127.5) / 128 + j (Q - 127.5) / 128; N = n_bins, nseg = L / N whole segments:
 *   P[k] = sum_seg | sum_n w[n] x[seg N + n] exp(-2 pi i k n / N) |^2 * scale,   scale = 1 / (nseg N sum w^2) made by the host in double.
 *
 * Arithmetic.  The transform, the power sums and the scale are float64 (v_fma_f64 / v_add_f64); P is rounded to float32 ONCE, at the store.  A
 * float32 transform is right to one to three float32 steps in a bin that carries a lone tone (the last butterfly alone rounds the amplitude to
 * half a step, the power to a whole one), and the check this kernel is held to - its error against a float64 model within 2 x rms / 3 x worst
 * of a float32 reference's - cannot be met that way wherever the reference happens to be right to a fraction of a step (measured: 157 % / 105 %
 * of the limits on such a block).  Rounded once, the result is within half a step of the true value, which no float32 reference beats.  Window and
 * twiddles stay the host's float tables (double, rounded once): their rounding is random from value to value and leaves 1.5e-9 of a bin's power.
 *
 * Decomposition.  One workgroup of 256 threads per (stream, block).  A segment is transformed by T = N / 16 threads, 16 complex values each, so the
 * workgroup holds G = 256 / T segments at a time - N = 256: sixteen lanes per segment, 16 segments; N = 1024: one wave per segment, 4 segments;
 * N = 4096: the whole workgroup on one segment - and slot g takes segments g, g + G, ...  The two 16-byte IQ words of a thread's next segment are
 * in flight while it transforms the current one.
 *
 * The FFT is a Stockham autosort (natural order in, natural order out) in passes of radix 16 (two layers of radix 4 in registers), N = 1024 with a
 * first pass of radix 4: 256 = 16 x 16, 1024 = 4 x 16 x 16, 4096 = 16 x 16 x 16.  Pass with radix R after passes of product p, butterfly i of N / R:
 *   k = i mod p,  u[r] = x[i + r N / R] W^(r k),  W = exp(-2 pi i / (p R)),  U = DFT_R(u),  y[(i - k) R + k + r p] = U[r].
 * Between passes the values cross threads through the slot's N complex doubles of LDS (16-byte accesses), in place: every thread of the slot reads
 * its 16 values before any writes (one wave: program order, the DS operations of a wave execute in order; N = 4096: a workgroup barrier between the
 * reads and the writes).  Index a lives at a + (a >> 4): the pad spreads the passes' strides of 16 and 64 values over the banks.  The last pass
 * writes nothing: thread i then holds bins i + r T and adds |U[r]|^2 to 16 accumulators it keeps across its segments.  Window and pass twiddles
 * (15 per thread and twiddled pass) come from the host's table, are the same for every segment of a thread and are loaded once into registers.
 * No __sinf / __cosf.
 *
 * At the end the G partial spectra go to LDS and are added in the order of g - fixed, so equal bytes give bit-equal P whatever the batch's shape -
 * scaled once, rounded to float and stored as 16-byte words.
 *
 * Table (floats), made by fmdk_spectrum_tables:  w[N], then per twiddled pass q (p = P1, then P1 x 16 while < N), r = 1 .. 15, i = 0 .. T - 1:
 *   {cos, -sin}(2 pi r (i mod p) / (16 p)). */
#include <cmath>

namespace {

constexpr int SP_NT = 256;
constexpr int SP_LDS = 4096 + 4096 / 16;      /* complex values: G x N = 4096 for every N, plus the pad */

constexpr double SP_C8 = 0.92387953251128674, SP_S8 = 0.38268343236508977, SP_H = 0.70710678118654752;   /* cos(pi / 8), sin(pi / 8), sqrt(1 / 2) */

constexpr int sp_p1(int n) { return n == 1024 ? 4 : 16; }                       /* p of the second pass */
constexpr int sp_passes(int n) { return sp_p1(n) * 16 < n ? 3 : 2; }
constexpr int sp_tw_passes(int n) { return sp_passes(n) - 1; }                  /* the first pass has p = 1: no twiddles */

__device__ __forceinline__ int sp_pad(int a) { return a + (a >> 4); }

/* x *= w, fused explicitly (the unit is compiled with -ffp-contract=off) */
__device__ __forceinline__ void sp_cmul(double &x, double &y, double wx, double wy) {
  const double nx = __builtin_fma(x, wx, -(y * wy));
  const double ny = __builtin_fma(x, wy, y * wx);
  x = nx;
  y = ny;
}

/* forward DFT of four values in place, natural order */
__device__ __forceinline__ void sp_dft4(double &x0, double &y0, double &x1, double &y1, double &x2, double &y2, double &x3, double &y3) {
  const double ax = x0 + x2, ay = y0 + y2, bx = x0 - x2, by = y0 - y2;
  const double cx = x1 + x3, cy = y1 + y3, dx = x1 - x3, dy = y1 - y3;
  x0 = ax + cx; y0 = ay + cy;
  x2 = ax - cx; y2 = ay - cy;
  x1 = bx + dy; y1 = by - dx;          /* b - j d */
  x3 = bx - dy; y3 = by + dx;          /* b + j d */
}

/* forward DFT of sixteen values in place as 4 x 4: n = 4 n1 + n2, k = k1 + 4 k2.  X[k1 + 4 k2] ends at index 4 k1 + k2 (sp_at). */
__device__ __forceinline__ void sp_dft16(double (&x)[16], double (&y)[16]) {
#pragma unroll
  for (int n2 = 0; n2 < 4; n2++) sp_dft4(x[n2], y[n2], x[4 + n2], y[4 + n2], x[8 + n2], y[8 + n2], x[12 + n2], y[12 + n2]);
  /* index 4 k1 + n2 holds A[n2][k1]: times W16^(n2 k1) */
  sp_cmul(x[5], y[5], SP_C8, -SP_S8);                                                     /* W^1 */
  { const double a = x[6], b = y[6]; x[6] = SP_H * (a + b); y[6] = SP_H * (b - a); }      /* W^2 = h (1 - j) */
  sp_cmul(x[7], y[7], SP_S8, -SP_C8);                                                     /* W^3 */
  { const double a = x[9], b = y[9]; x[9] = SP_H * (a + b); y[9] = SP_H * (b - a); }      /* W^2 */
  { const double a = x[10], b = y[10]; x[10] = b; y[10] = -a; }                           /* W^4 = -j */
  { const double a = x[11], b = y[11]; x[11] = SP_H * (b - a); y[11] = -(SP_H * (a + b)); }    /* W^6 = -h (1 + j) */
  sp_cmul(x[13], y[13], SP_S8, -SP_C8);                                                   /* W^3 */
  { const double a = x[14], b = y[14]; x[14] = SP_H * (b - a); y[14] = -(SP_H * (a + b)); }    /* W^6 */
  sp_cmul(x[15], y[15], -SP_C8, SP_S8);                                                   /* W^9 */
#pragma unroll
  for (int k1 = 0; k1 < 4; k1++) sp_dft4(x[4 * k1], y[4 * k1], x[4 * k1 + 1], y[4 * k1 + 1], x[4 * k1 + 2], y[4 * k1 + 2], x[4 * k1 + 3], y[4 * k1 + 3]);
}
constexpr int sp_at(int r) { return 4 * (r & 3) + (r >> 2); }     /* where sp_dft16 leaves X[r] */

/* the threads of one segment slot hand values over through LDS: one wave or less - the compiler-level ordering of k_common.inc's wave_lds_sync;
 * the whole workgroup (N = 4096) - a barrier */
template <int T> __device__ __forceinline__ void sp_sync() {
  if constexpr (T > 64) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

/* (u - 127.5) / 128 of byte m of a dword: exact */
__device__ __forceinline__ double sp_byte(uint32_t w, int m) { return __builtin_fma((double)((w >> (8 * m)) & 0xffu), 0.0078125, -0.99609375); }

/* one 16-byte IQ word = 8 samples, windowed, to LDS values [at, at + 8) (at a multiple of 8: one pad for all eight) */
__device__ __forceinline__ void sp_stage(double2 *lds, int at, const uint4 &q, const float (&w)[16], int w0) {
  const uint32_t d[4] = {q.x, q.y, q.z, q.w};
  double2 *o = lds + sp_pad(at);
#pragma unroll
  for (int m = 0; m < 4; m++) {
    const double wa = (double)w[w0 + 2 * m], wb = (double)w[w0 + 2 * m + 1];
    o[2 * m] = double2{sp_byte(d[m], 0) * wa, sp_byte(d[m], 1) * wa};
    o[2 * m + 1] = double2{sp_byte(d[m], 2) * wb, sp_byte(d[m], 3) * wb};
  }
}

template <int N>
__global__ __launch_bounds__(SP_NT) void fmd_spectrum_kernel(const uint8_t *__restrict__ iq, int block_len, int nseg, const float *__restrict__ tab,
                                                             double scale, float *__restrict__ power) {
  constexpr int T = N / 16, G = SP_NT / T;
  constexpr int P1 = sp_p1(N), P2 = P1 * 16;
  constexpr bool THREE = sp_passes(N) == 3;
  static_assert(G * N == 4096 && T * 16 == N, "a workgroup holds 4096 values");
  __shared__ double2 lds[SP_LDS];

  const int t = threadIdx.x, g = t / T, i = t % T, sb = g * N;
  const uint4 *src = reinterpret_cast<const uint4 *>(iq + (size_t)blockIdx.x * (size_t)block_len);   /* block_len is a multiple of 16, d_iq 16-byte aligned */
  constexpr int WPS = N / 8;          /* 16-byte words per segment: thread i takes words i and i + T */

  /* what is the same for every segment of this thread: 16 window values, 15 twiddles per twiddled pass */
  float w[16];
  {
    const float4 *wt = reinterpret_cast<const float4 *>(tab);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const float4 a = wt[2 * (i + h * T)], b = wt[2 * (i + h * T) + 1];
      w[8 * h] = a.x; w[8 * h + 1] = a.y; w[8 * h + 2] = a.z; w[8 * h + 3] = a.w;
      w[8 * h + 4] = b.x; w[8 * h + 5] = b.y; w[8 * h + 6] = b.z; w[8 * h + 7] = b.w;
    }
  }
  double t1x[15], t1y[15], t2x[15], t2y[15];
  {
    const float2 *tw = reinterpret_cast<const float2 *>(tab + N);
#pragma unroll
    for (int r = 0; r < 15; r++) {
      const float2 a = tw[r * T + i];
      t1x[r] = a.x; t1y[r] = a.y;
      if constexpr (THREE) {
        const float2 b = tw[(15 + r) * T + i];
        t2x[r] = b.x; t2y[r] = b.y;
      } else {
        t2x[r] = 1.0; t2y[r] = 0.0;
      }
    }
  }
  double acc[16];
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.0;

  int seg = g;
  uint4 c0 = uint4{0, 0, 0, 0}, c1 = c0;
  if (seg < nseg) {
    c0 = src[(size_t)seg * WPS + i];
    c1 = src[(size_t)seg * WPS + i + T];
  }
  while (seg < nseg) {
    const int nxt = seg + G;
    uint4 n0 = uint4{0, 0, 0, 0}, n1 = n0;
    if (nxt < nseg) {                           /* in flight while this segment is transformed */
      n0 = src[(size_t)nxt * WPS + i];
      n1 = src[(size_t)nxt * WPS + i + T];
    }
    sp_stage(lds, sb + 8 * i, c0, w, 0);
    sp_stage(lds, sb + 8 * (i + T), c1, w, 8);
    sp_sync<T>();

    double x[16], y[16];
    if constexpr (N == 1024) {
      /* first pass, radix 4, p = 1: butterflies i + 64 b, b = 0 .. 3 */
#pragma unroll
      for (int b = 0; b < 4; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const double2 v = lds[sp_pad(sb + i + 64 * b + r * 256)];
          x[4 * b + r] = v.x; y[4 * b + r] = v.y;
        }
      sp_sync<T>();
#pragma unroll
      for (int b = 0; b < 4; b++) {
        sp_dft4(x[4 * b], y[4 * b], x[4 * b + 1], y[4 * b + 1], x[4 * b + 2], y[4 * b + 2], x[4 * b + 3], y[4 * b + 3]);
#pragma unroll
        for (int r = 0; r < 4; r++) lds[sp_pad(sb + 4 * (i + 64 * b) + r)] = double2{x[4 * b + r], y[4 * b + r]};
      }
    } else {
      /* first pass, radix 16, p = 1 */
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const double2 v = lds[sp_pad(sb + i + r * T)];
        x[r] = v.x; y[r] = v.y;
      }
      sp_sync<T>();
      sp_dft16(x, y);
#pragma unroll
      for (int r = 0; r < 16; r++) lds[sp_pad(sb + 16 * i + r)] = double2{x[sp_at(r)], y[sp_at(r)]};
    }
    sp_sync<T>();

    /* second pass, radix 16, p = P1 */
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const double2 v = lds[sp_pad(sb + i + r * T)];
      x[r] = v.x; y[r] = v.y;
    }
#pragma unroll
    for (int r = 1; r < 16; r++) sp_cmul(x[r], y[r], t1x[r - 1], t1y[r - 1]);
    sp_dft16(x, y);
    if constexpr (THREE) {
      sp_sync<T>();
      {
        const int k = i % P1, j = (i - k) * 16 + k;
#pragma unroll
        for (int r = 0; r < 16; r++) lds[sp_pad(sb + j + r * P1)] = double2{x[sp_at(r)], y[sp_at(r)]};
      }
      sp_sync<T>();
      /* third pass, radix 16, p = P2 = N / 16: k = i, nothing to write */
      static_assert(!THREE || P2 == T, "the last pass has p = N / 16");
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const double2 v = lds[sp_pad(sb + i + r * T)];
        x[r] = v.x; y[r] = v.y;
      }
#pragma unroll
      for (int r = 1; r < 16; r++) sp_cmul(x[r], y[r], t2x[r - 1], t2y[r - 1]);
      sp_dft16(x, y);
    } else {
      static_assert(THREE || P1 == T, "the last pass has p = N / 16");
    }
    /* this thread holds bins i + r T */
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = __builtin_fma(x[sp_at(r)], x[sp_at(r)], __builtin_fma(y[sp_at(r)], y[sp_at(r)], acc[r]));
    sp_sync<T>();                               /* the slot's values have been read: the next segment may be staged */
    c0 = n0;
    c1 = n1;
    seg = nxt;
  }

  /* the G partial spectra, added in the order of g */
  __syncthreads();
  double *part = reinterpret_cast<double *>(lds);
#pragma unroll
  for (int r = 0; r < 16; r++) part[sb + i + r * T] = acc[r];
  __syncthreads();
  float4 *out = reinterpret_cast<float4 *>(power + (size_t)blockIdx.x * N);
  const double2 *p2 = reinterpret_cast<const double2 *>(part);
  for (int o = t; o < N / 4; o += SP_NT) {
    double2 a = p2[2 * o], b = p2[2 * o + 1];
#pragma unroll
    for (int h = 1; h < G; h++) {
      const double2 u = p2[h * (N / 2) + 2 * o], v = p2[h * (N / 2) + 2 * o + 1];
      a.x += u.x; a.y += u.y; b.x += v.x; b.y += v.y;
    }
    out[o] = float4{(float)(a.x * scale), (float)(a.y * scale), (float)(b.x * scale), (float)(b.y * scale)};     /* the one rounding to float */
  }
}

template <int N>
int sp_launch(const void *d_iq, int n_slots, int block_len, int nseg, const float *d_tab, double scale, void *d_power, hipStream_t st) {
  hipLaunchKernelGGL(fmd_spectrum_kernel<N>, dim3((unsigned)n_slots), dim3(SP_NT), 0, st, static_cast<const uint8_t *>(d_iq), block_len, nseg, d_tab,
                     scale, static_cast<float *>(d_power));
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int fmdk_spectrum_built(int n_bins) { return n_bins == 256 || n_bins == 1024 || n_bins == 4096; }

extern "C" size_t fmdk_spectrum_table_floats(int n_bins) {
  return (size_t)n_bins + (size_t)sp_tw_passes(n_bins) * 15 * (size_t)(n_bins / 16) * 2;
}

/* window and twiddles in double, rounded once to float; *sum_w2 = sum of w^2 in double (of the unrounded window: the definition's) */
extern "C" void fmdk_spectrum_tables(int n_bins, int window, float *out, double *sum_w2) {
  const double two_pi = 6.283185307179586476925286766559;
  const int N = n_bins, T = N / 16;
  double s2 = 0.0;
  for (int n = 0; n < N; n++) {
    const double w = window == FMD_WINDOW_HANN ? 0.5 - 0.5 * cos(two_pi * (double)n / (double)N) : 1.0;
    out[n] = (float)w;
    s2 += w * w;
  }
  *sum_w2 = s2;
  float *tw = out + N;
  int p = sp_p1(N);
  for (int q = 0; q < sp_tw_passes(N); q++, p *= 16)
    for (int r = 1; r < 16; r++)
      for (int i = 0; i < T; i++) {
        const double a = two_pi * (double)(r * (i % p)) / (16.0 * (double)p);
        float *o = tw + ((size_t)(q * 15 + (r - 1)) * T + i) * 2;
        o[0] = (float)cos(a);
        o[1] = (float)-sin(a);
      }
}

/* n_slots = n_streams x n_blocks workgroups; nseg = (block_len / 2) / n_bins >= 1.  Plain launch on `stream`; returns 0 or a hipError_t. */
extern "C" int fmdk_spectrum(const void *d_iq, int n_slots, int block_len, int n_bins, const float *d_tab, double scale, void *d_power, void *stream) {
  const int nseg = (block_len / 2) / n_bins;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (n_bins) {
    case 256: return sp_launch<256>(d_iq, n_slots, block_len, nseg, d_tab, scale, d_power, st);
    case 1024: return sp_launch<1024>(d_iq, n_slots, block_len, nseg, d_tab, scale, d_power, st);
    case 4096: return sp_launch<4096>(d_iq, n_slots, block_len, nseg, d_tab, scale, d_power, st);
  }
  return (int)hipErrorInvalidValue;
}
