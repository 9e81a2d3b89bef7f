/* levels.inc - the finish kernel of a levels launch (fmd_batch_run_device_levels, and every launch while power squelch is on): included by
 * fmd_kernels_recv.hip, the receivers' translation unit (nothing of the fused chain is in it).  Launched on the fused kernel's stream right after it, so whatever orders
 * the batch's launches (the stream, the ev_order hand-over in fmd_host.c) orders this one too; a plain launch, so it can be captured.
 *
 * One wave per stream.  For each block in order: the fused kernel's tile partials {sum of I + Q, sum of I^2 + Q^2} (fmd_fused_kernel<..., LV =
 * true>) are summed in double - lane l takes tiles l, l + 64, ..., then an xor butterfly, so every lane holds the same sums - and
 *   level = sqrt(max(0, S2 / n - (S1 / n)^2)),  n = 2 M  (the reference's rms() over the block's lowpassed buffer, src/rtl_fm_player.c:737-755)
 * goes to levels[stream][block] when levels is not NULL.  Squelch (thr != NULL and thr[stream] > 0): rtl_fm's power squelch,
 *   hits = level < thr ? hits + 1 : 0;  closed when hits > conseq: hits = conseq + 1, lens = 0 and the block's pcm_stride PCM slots zeroed
 * (16-byte stores: the host requires d_pcm 16-byte aligned, pcm_stride is a multiple of 8).  hits[stream] carries across launches. */

namespace {

constexpr int LV_NT = 256;   /* four streams per workgroup */

__global__ __launch_bounds__(LV_NT) void fmd_levels_kernel(const float2 *__restrict__ part, int n_streams, int n_blocks, int tpb, int M,
                                                           int pcm_stride, float *__restrict__ levels, int32_t *__restrict__ lens,
                                                           int16_t *__restrict__ pcm, const float *__restrict__ thr,
                                                           int32_t *__restrict__ hits, int conseq) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * (LV_NT / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (s >= n_streams) return;
  const float t = thr ? thr[s] : 0.f;
  const bool sq = t > 0.f;
  int h = sq ? hits[s] : 0;
  const double n = 2.0 * (double)M;
  for (int b = 0; b < n_blocks; b++) {
    const size_t slot = (size_t)s * n_blocks + b;
    const float2 *p = part + slot * tpb;
    double a = 0.0, q = 0.0;
    for (int i = lane; i < tpb; i += 64) {
      const float2 v = p[i];
      a += (double)v.x;
      q += (double)v.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      a += __shfl_xor(a, o);
      q += __shfl_xor(q, o);
    }
    const double m1 = a / n, var = q / n - m1 * m1;
    const float lvl = (float)sqrt(var > 0.0 ? var : 0.0);
    if (levels && lane == 0) levels[slot] = lvl;
    if (sq) {
      h = lvl < t ? h + 1 : 0;
      if (h > conseq) {
        h = conseq + 1;
        if (lane == 0) lens[slot] = 0;
        int4 *z = reinterpret_cast<int4 *>(pcm + slot * pcm_stride);
        for (int i = lane; i < pcm_stride / 8; i += 64) z[i] = int4{0, 0, 0, 0};
      }
    }
  }
  if (sq && lane == 0) hits[s] = h;
}

}  // namespace

extern "C" int fmdk_levels(const void *d_part, int n_streams, int n_blocks, int block_len, int pcm_stride, void *d_levels, void *d_lens, void *d_pcm,
                           const float *d_thr, int32_t *d_hits, int conseq, void *stream) {
  const int M = block_len >> 4, tpb = (M + FMDK_TILE - 1) / FMDK_TILE;
  const dim3 grid((n_streams + LV_NT / 64 - 1) / (LV_NT / 64)), block(LV_NT);
  hipLaunchKernelGGL(fmd_levels_kernel, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<const float2 *>(d_part), n_streams, n_blocks,
                     tpb, M, pcm_stride, static_cast<float *>(d_levels), static_cast<int32_t *>(d_lens), static_cast<int16_t *>(d_pcm), d_thr, d_hits,
                     conseq);
  return (int)hipGetLastError();
}
