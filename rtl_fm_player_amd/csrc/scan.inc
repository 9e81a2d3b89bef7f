/* scan.inc - the station finder (fmd_scan_*; include/fmdemod_mi355x.h, "Station finder"): included by fmd_kernels_recv.hip, the receivers' translation
 * unit, beside spectrum.inc and tuner.inc.  A kernel of its own: it shares nothing with the fused kernel but the layout
 * fmd_batch_spectrum_device writes, and references nothing of the host layer.  gfx950, no inline assembly, no floating-point atomics.
 *
 * One workgroup of 256 threads per stream; every decision is taken on doubles held in LDS:
 *   1. average: a thread owns four adjacent bins of every 1024 (one 16-byte load per block, consecutive threads at consecutive addresses) and sums
 *      them over the blocks in double, b = 0, 1, ... from zero; one division; A into LDS (32 KiB at 4096 bins).
 *   2. floor: an exact order statistic by radix select over the 64-bit patterns of the used A (for values >= 0 the pattern's order is the value's):
 *      eight passes of eight bits from the top, a 256-bin histogram per pass with integer LDS atomics (a count does not depend on the order of
 *      its increments), a scan of the histogram across the workgroup, and the digit that holds the rank fixes the next byte.  It ends after eight
 *      passes whatever the bits are.  The guarded bins of A are then overwritten with F.
 *   3. channel power: a thread takes the candidates t, t + 256, ...; for each it walks the bins of its band upwards, s0 .. s1, from zero: one
 *      rounded product w A per term (interior: A itself), one add - the order of the definition, so the model reproduces Pc and M.
 *   4. occupied, suppression over the window and rank, all by counting: a station's rank is the number of stations that beat it, a strict total
 *      order (Pc descending, then the lower candidate), so every rank below `found` is taken once; the slots from `written` on are zeroed by
 *      other threads - no two threads write one slot.
 * A value that is not finite and >= 0 changes values only: every loop bound is an integer of the plan, a rank is below C by construction and a
 * slot is written only where the rank is below max_stations. */

namespace {

constexpr int SCN_NT = 256;
static_assert(sizeof(fmd_scan_station) == 32 && sizeof(fmd_scan_config) == 48 && sizeof(fmdk_scan_cand) == 24, "the layouts of the header");
static_assert(FMD_SCAN_MAX_BINS == 4096 && FMD_SCAN_MAX_CANDIDATES == 1024 && (FMD_SCAN_MAX_BINS % (4 * SCN_NT)) == 0, "LDS arrays; the load's stride");

struct scn_args {
  const float *power;
  const fmdk_scan_cand *cand;
  fmd_scan_station *stations;
  int32_t *counts;
  float *chan;
  double nb, thr;              /* bins of a channel; double(threshold) */
  int32_t n_blocks, n_bins, n_cand, cmax, raster_hz, rate, min_sep, dc_guard, rank, max_stations;
};

__device__ __forceinline__ bool scn_beats(double pj, int j, double pi, int i) { return pj > pi || (pj == pi && j < i); }

__global__ __launch_bounds__(SCN_NT) void fmd_scan_kernel(const scn_args a) {
  __shared__ double A[FMD_SCAN_MAX_BINS];
  __shared__ double Pc[FMD_SCAN_MAX_CANDIDATES];
  __shared__ double Mc[FMD_SCAN_MAX_CANDIDATES];
  __shared__ unsigned hist[256];
  __shared__ unsigned char is_st[FMD_SCAN_MAX_CANDIDATES];
  __shared__ unsigned wsum[SCN_NT / 64];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned s_want;
  __shared__ int s_found;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int N = a.n_bins, C = a.n_cand;
  const size_t stream = blockIdx.x;
  const float *P = a.power + stream * (size_t)a.n_blocks * (size_t)N;

  /* 1. the average over the blocks */
  const double nbl = (double)a.n_blocks;
  for (int v = t; 4 * v < N; v += SCN_NT) {
    const float4 *src = reinterpret_cast<const float4 *>(P) + v;
    const size_t step = (size_t)(N >> 2);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 4
    for (int b = 0; b < a.n_blocks; b++) {
      const float4 q = src[(size_t)b * step];
      s0 += (double)q.x;
      s1 += (double)q.y;
      s2 += (double)q.z;
      s3 += (double)q.w;
    }
    A[4 * v] = s0 / nbl;
    A[4 * v + 1] = s1 / nbl;
    A[4 * v + 2] = s2 / nbl;
    A[4 * v + 3] = s3 / nbl;
  }
  if (t == 0) {
    s_prefix = 0ull;
    s_want = (unsigned)a.rank;
    s_found = 0;
  }
  __syncthreads();

  /* 2. the floor: the element of rank a.rank among the used bins (|s| >= dc_guard), by radix select from the top byte down */
  const int g = a.dc_guard, half = N >> 1;
  for (int pass = 0; pass < 8; pass++) {
    const int shift = 56 - 8 * pass;
    const unsigned long long prefix = s_prefix;
    const unsigned want = s_want;
    hist[t] = 0u;
    __syncthreads();
    for (int k = t; k < N; k += SCN_NT) {
      const int s = k < half ? k : N - k;                /* |s| */
      const unsigned long long key = (unsigned long long)__double_as_longlong(A[k]);
      const bool match = pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8));
      if (s >= g && match) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const unsigned h = hist[t];
    unsigned inc = h;                                    /* inclusive scan over the wave, then over the waves */
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    for (int w = 0; w < wave; w++) inc += wsum[w];
    const unsigned exc = inc - h;
    if (want >= exc && want < inc) {                     /* one digit holds the rank: the counts of the matching keys add up to more than it */
      s_prefix = prefix | ((unsigned long long)t << shift);
      s_want = want - exc;
    }
    __syncthreads();
  }
  const double F = __longlong_as_double((long long)s_prefix);
  for (int k = t; k < 2 * g - 1; k += SCN_NT) A[(k - (g - 1)) & (N - 1)] = F;      /* the guarded bins s = -(g-1) .. g-1 read F from here on */
  __syncthreads();

  /* 3. channel power and first moment of every candidate */
  const double invN = 1.0 / (double)N;                   /* a power of two: exact */
  for (int i = t; i < C; i += SCN_NT) {
    const fmdk_scan_cand cd = a.cand[i];
    const long long cn = (long long)(i - a.cmax) * (long long)a.raster_hz * (long long)N;
    double pc = 0.0, m = 0.0;
    for (int n = 0; n < cd.count; n++) {
      const int s = cd.first + n;
      double term = A[s & (N - 1)];
      if (n == 0) term = cd.w_first * term;
      else if (n == cd.count - 1) term = cd.w_last * term;
      const double d = (double)((long long)s * (long long)a.rate - cn) * invN;
      pc += term;
      m += term * d;
    }
    Pc[i] = pc;
    Mc[i] = m;
    if (a.chan) a.chan[stream * (size_t)C + (size_t)i] = (float)pc;
  }
  __syncthreads();

  /* 4. occupied, and no candidate within min_sep beats it */
  const double Fc = F * a.nb, lim = a.thr * Fc;
  int mine = 0;
  for (int i = t; i < C; i += SCN_NT) {
    const double pi = Pc[i];
    bool st = pi > lim;
    const int j0 = i - a.min_sep < 0 ? 0 : i - a.min_sep, j1 = i + a.min_sep > C - 1 ? C - 1 : i + a.min_sep;
    for (int j = j0; j <= j1 && st; j++)
      if (j != i && scn_beats(Pc[j], j, pi, i)) st = false;
    is_st[i] = st ? 1 : 0;
    mine += st ? 1 : 0;
  }
  if (mine) atomicAdd(&s_found, mine);
  __syncthreads();

  const int found = s_found, written = found < a.max_stations ? found : a.max_stations;
  fmd_scan_station *out = a.stations + stream * (size_t)a.max_stations;
  for (int i = t; i < C; i += SCN_NT) {
    if (!is_st[i]) continue;
    const double pi = Pc[i];
    int r = 0;
    for (int j = 0; j < C; j++)
      if (is_st[j] && j != i && scn_beats(Pc[j], j, pi, i)) r++;
    if (r < a.max_stations) {
      const int off = (i - a.cmax) * a.raster_hz;
      fmd_scan_station o;
      o.offset_hz = off;
      o.candidate = i;
      o.power = (float)pi;
      o.snr = (float)(pi / Fc);
      o.centroid_hz = (float)((double)off + Mc[i] / pi);
      o.reserved[0] = o.reserved[1] = o.reserved[2] = 0;
      out[r] = o;
    }
  }
  if (t >= written && t < a.max_stations) {
    fmd_scan_station z;
    z.offset_hz = 0; z.candidate = 0; z.power = 0.f; z.snr = 0.f; z.centroid_hz = 0.f;
    z.reserved[0] = z.reserved[1] = z.reserved[2] = 0;
    out[t] = z;
  }
  if (t == 0) {
    a.counts[2 * stream] = found;
    a.counts[2 * stream + 1] = written;
  }
}

}  // namespace

extern "C" int fmdk_scan_launch(const void *d_power, int n_streams, int n_blocks, const fmd_scan_config *c, const fmdk_scan_plan *p, const void *d_cand,
                                void *d_stations, void *d_counts, void *d_chan, void *stream) {
  scn_args a;
  a.power = static_cast<const float *>(d_power);
  a.cand = static_cast<const fmdk_scan_cand *>(d_cand);
  a.stations = static_cast<fmd_scan_station *>(d_stations);
  a.counts = static_cast<int32_t *>(d_counts);
  a.chan = static_cast<float *>(d_chan);
  a.nb = p->nb;
  a.thr = (double)c->threshold;
  a.n_blocks = n_blocks;
  a.n_bins = c->n_bins;
  a.n_cand = p->n_cand;
  a.cmax = p->cmax;
  a.raster_hz = c->raster_hz;
  a.rate = c->rate;
  a.min_sep = c->min_sep;
  a.dc_guard = c->dc_guard;
  a.rank = p->rank;
  a.max_stations = c->max_stations;
  hipLaunchKernelGGL(fmd_scan_kernel, dim3((unsigned)n_streams), dim3(SCN_NT), 0, static_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}
