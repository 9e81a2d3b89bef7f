/* cold_paths.inc - part of the fused IQ -> PCM kernel (included by fmd_kernels.inc inside its anonymous namespace; not a translation unit of its own).
 * Cold paths: quirk Q1 at block starts, the launch's first frames against the carried bm ring, the exact redo of an ill-conditioned carrier. */

/* FMD_MATH_FAST_MFMA_F stereo, the launch's first tile: the reference's L+R at an emit instant m < size - 1 still sums CARRIED bm values (the ring of
 * the launch before), where the composite filter has summed what the carried discriminator history makes of them - the partial first-stage sums
 * bm0(m') = sum_i fm[i] v(m' - i) over the `size` carried samples only.  The difference is linear: c(m') = bm_state(m') - bm0(m') for the
 * size - 1 ring entries, and frame q with emit index m_q gets sum_{j > m_q} fm[j] c(m_q - j) added to both channels ({L, R} = om +- os). */
template <int HV, typename WM>
__device__ __forceinline__ void lr_head_fix(const fmdk_params &P, const f4 *tap_mpx, const float *bm_state, WM &w, int lane, uint32_t acc_t, int nq) {
  /* (once per launch and stream, but on the launch's critical path - the worker of chunk 0 runs it while the others are a tile ahead: both
   * ring entries of a lane in one loop of fixed length, unrolled so that the LDS reads of several taps are in flight - as a rolled loop with a
   * data-dependent bound it waited out one LDS round trip per tap, 12 us per launch: a quarter of a one-block launch) */
  const float *fmt = reinterpret_cast<const float *>(tap_mpx);
  {
    const int ia = lane, ib = lane + 64;               /* ring entries of time m' = idx - 89 */
    float sa = 0.f, sb = 0.f;
#pragma unroll 9
    for (int i = 0; i < 90; i++) {
      const float t = fmt[4 * (i < 45 ? i : 89 - i)];
      const int xa = ia - 89 - i, xb = ib - 89 - i;    /* sample index m' - i: carried for >= -90 */
      const float va = w.v[HV + (xa >= -90 ? xa : -90)], vb = w.v[HV + (xb >= -90 ? xb : -90)];
      sa = __builtin_fmaf(t, xa >= -90 ? va : 0.f, sa);
      sb = __builtin_fmaf(t, xb >= -90 ? vb : 0.f, sb);
    }
    w.xs[ia] = bm_state[ia + 1] - sa;
    if (ib < 89) w.xs[ib] = bm_state[ib + 1] - sb;
  }
  wave_lds_sync();
  /* four lanes per frame (the taps j = m_q + 1 + part, + 4, ...), joined by two DPP adds; sixteen frames per pass: emit indices below 89 are
   * the first 89 slow / fast + 1 <= 24 frames (fast >= 4 slow) */
#pragma unroll 1
  for (int pass = 0; pass < 2; pass++) {
    const int q = (lane >> 2) + 16 * pass, part = lane & 3;
    const int mq = emit_index_magic((uint32_t)P.fast - acc_t - 1u, q, (uint32_t)P.fast, P.emit_magic, P.emit_shift);
    const bool live = q < nq && mq < 89;
    const int m0 = live ? mq : 0;
    float dl = 0.f;
#pragma unroll 6
    for (int u = 0; u < 24; u++) {
      const int jj = m0 + 1 + part + 4 * u;
      const int jc = jj < 90 ? jj : 89;
      const float t = fmt[4 * (jc < 45 ? jc : 89 - jc)], c = w.xs[m0 - jc + 89];
      dl = __builtin_fmaf(t, (live && jj < 90) ? c : 0.f, dl);
    }
    dl += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, dl), 0xb1, 0xf, 0xf, true));   /* quad_perm [1, 0, 3, 2] */
    dl += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, dl), 0x4e, 0xf, 0xf, true));   /* quad_perm [2, 3, 0, 1] */
    if (live && part == 0) {
      f2 *fr2 = reinterpret_cast<f2 *>(&w.fr[0]);
      const f2 o = fr2[q];
      fr2[q] = f2{o.x + dl, o.y + dl};
    }
  }
  wave_lds_sync();
}

/* Block-start quirk Q1 (SURVEY.md section 0: sample 1 of a block that starts with an emit is overwritten with R of frame 0) for the kernel whose second stage
 * reads limbs: q1_patch with the sums taken from them.  L+R at sample 0 = the composite filter over the discriminator's limb history v[-178 .. 0] (three taps per
 * lane, summed over the wave); the launch's first block instead sums the CARRIED bm ring (bm_head) and sample 0's own first-stage output (lane 0's f). */
template <int HV, typename WM>
__device__ __forceinline__ void q1_patch_i8(const fmdk_params &P, const f4 *tap_mpx, WM &w, int lane, float pp, const float *bm_head) {
  float f = 0.f;
  if (lane < 3) {
    const float *tap = reinterpret_cast<const float *>(tap_mpx) + lane;
    for (int k = 0; k < 45; k++)
      f = mac<false>(f, w.v[(HV - 89 + k)] + w.v[(HV - k)], tap[4 * k]);
  }
  const float vp = __shfl(f, 1), vs = __shfl(f, 2);
  float omg = 0.f;
  if (!bm_head) {
#pragma unroll
    for (int u = 0; u < 3; u++) {
      const int t = lane + 64 * u;
      if (t < 179) omg = __builtin_fmaf((float)P.gq[t < 90 ? t : 178 - t] * P.g_unit, limb_value(w, 0, HBE - t), omg);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) omg += __shfl_xor(omg, o);
  }
  if (lane == 0) {
    /* sample 0's own (L-R) x carrier, as the tile's stage C will store it: rounded to 2^-20 */
    const float bs0 = __builtin_rintf(vs * carrier_of<false>(vp, pp, P.swf, P.cwf) * VQ_SCALE) * (1.0f / VQ_SCALE);
    constexpr int VH = WM::kVbh, BS = WM::kBsRow;
    float om = 0.f, os = 0.f;
    for (int k = 0; k < 45; k++) {                     /* window x[-89 .. 0]: pairs (k - 89, -k) */
      const float t = tap_mpx[k].x;
      if (bm_head) om = mac<false>(om, bm_head[1 + k] + (k ? bm_head[90 - k] : f), t);
      const float as = limb_value(w, BS, VH - 89 + k), bs = k ? limb_value(w, BS, VH - k) : bs0;
      os = mac<false>(os, as + bs, t);
    }
    if (!bm_head) om = omg;
    w.v[(HV + 1)] = om - os;
  }
}

/* The pilot and L-R sums of ONE sample in the reference's order of operations (src/rtl_fm_player.c:538-566: f += tap[k] * (x[k] +
 * x[89 - k]), k ascending, multiply and add unfused), 90 taps: vp1 = pilot sum over the window x0[0 .. 89], vs1 = L-R sum over the
 * same window, vp0 = pilot sum one sample earlier (x0[-1 .. 88]).  The 3 x 45 products do not depend on each other: lane k forms
 * them (one round of reads, adds and multiplies for the whole wave) and leaves them in the worker's frame buffer, which is idle
 * during stage C; lanes 0 .. 2 then add one row each, in order - 45 dependent additions from registers instead of 45 dependent
 * steps with an LDS round trip each (which took 4 900 cycles of the worker's time per sample). */
template <typename WM>
__device__ __forceinline__ void ref_sums3(const f4 *tap_mpx, const float *x0, WM &w, int lane, float &vp1, float &vs1, float &vp0) {
  if (lane < 45) {
    const f4 t = tap_mpx[lane];
    const float p1 = x0[lane] + x0[89 - lane];
    const float p0 = x0[lane - 1] + x0[88 - lane];
    w.fr[lane] = p1 * t.y;
    w.fr[48 + lane] = p1 * t.z;
    w.fr[96 + lane] = p0 * t.y;
  }
  wave_lds_sync();
  const f4 *pr = reinterpret_cast<const f4 *>(&w.fr[48 * (lane < 3 ? lane : 0)]);
  f4 q[12];
#pragma unroll
  for (int g = 0; g < 12; g++) q[g] = pr[g];
  float acc = 0.f;
#pragma unroll
  for (int g = 0; g < 11; g++) { acc = acc + q[g].x; acc = acc + q[g].y; acc = acc + q[g].z; acc = acc + q[g].w; }
  acc = acc + q[11].x;                                           /* k = 44 */
  const int ai = __builtin_bit_cast(int, acc);                   /* v_readlane: no LDS round trip */
  vp1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(ai, 0));
  vs1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(ai, 1));
  vp0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(ai, 2));
  wave_lds_sync();
}

/* Fast kernels, cold path: sample m of the tile (stream sample n = n_tile + m) has an ill-conditioned
 * 38 kHz carrier (carrier_fast).  Redo its pilot / L-R filter outputs and the carrier in the reference's
 * exact arithmetic (src/rtl_fm_player.c:538-566, :472-481) from exactly recomputed discriminator samples
 * v[n - size .. n]: each from its IQ words re-read from memory (exact_output, discriminate<true>), except
 * the samples whose reference value is not a function of the IQ bytes alone - the first four of the launch
 * (carried history) and a block's sample 1 when quirk Q1 has overwritten it - which come from the worker's
 * history as they are.  All 64 lanes work on the one sample (m is uniform): they share the window
 * through w.xs, every lane then sums it (the reads broadcast) and lane 0 stores the result. */
template <int HV, typename WM>
__device__ __forceinline__ void redo_carrier(const fmdk_params &P, const f4 *tap_mpx, WM &w, int lane, int m, int n_tile,
                                             const uint4 *iq16, int n_total, int M, uint32_t acc_launch) {
  const int size = P.size, half = P.half;
  const int n = n_tile + m;
  const bool rot = !P.offset_tuning;
  asm volatile("" : "+s"(M));       /* (a divisor the compiler cannot see through: the reciprocal helper of this cold path's j / M is otherwise made before the tile
                                       loop and kept - in the kernels at the register limit, spilled - for the kernel's whole life) */
#ifdef FMD_REDO_PROF
  long long rt0 = clock64();
#define FMD_RSTAMP(i) { const long long now_ = clock64(); if (lane == 0) w.rprof[i] += now_ - rt0; rt0 = now_; }
  if (lane == 0) w.rprof[0]++;
#else
#define FMD_RSTAMP(i)
#endif
  if constexpr (HV == 96) {
    /* 0. Most flagged samples need less than the full redo.  What separates the fast carrier from the reference's is, above all,
     *    the ORDER of the pilot filter's additions (its partial sums are ~0.2, so ninety roundings add up to ~1e-7, which is what
     *    the threshold K was sized for); the window's samples themselves differ from the reference's by a few ulps each, which the
     *    filter averages down to ~1e-8.  So: sum the worker's own window (w.v) in the reference's order first - lane 0 vp[n],
     *    lane 1 vs[n], lane 2 vp[n-1] - and take the reference's carrier formula on those sums if the point is then further than
     *    L K from the origin (fmd_resolve.c: L and how it was measured; the rest goes on to the exact recomputation from the IQ words). */
    float vp1, vs1, vp0;
    ref_sums3(tap_mpx, &w.v[HV + m - 89], w, lane, vp1, vs1, vp0);
    const float x = vp1 * P.swf, y = vp1 * P.cwf - vp0;
    const float r2 = x * x + y * y;
    if (r2 * P.car_inv_k2_l2 > vs1 * vs1) {
      const float bs = vs1 * carrier_of<true>(vp1, vp0, P.swf, P.cwf);
      if (lane == 0) {
        if constexpr (WM::kLimbs) limb_store(w, WM::kBsRow, WM::kVbh + m, bs);
        else w.ms[HV + m].y = bs;
      }
      wave_lds_sync();
      FMD_RSTAMP(4)
      return;
    }
  }
  if constexpr (HV != 96) {
    /* generic filter sizes (up to 256 taps: the pairs would not fit xs): each discriminator sample from its own two
     * decimated samples */
    for (int i = lane; i <= size; i += 64) {
      const int j = n - size + i;
      bool keep = j <= 3;
      if (!keep && P.resample && M > 1) {
        const int blk = j / M;
        if (j - blk * M == 1) {
          const uint32_t a = (uint32_t)(((unsigned long long)acc_launch + (unsigned long long)blk * M * (uint32_t)P.slow) %
                                        (uint32_t)P.fast);
          keep = a + (uint32_t)P.slow >= (uint32_t)P.fast;
        }
      }
      float v1;
      if (keep) {
        v1 = w.v[HV + (j - n_tile)];
      } else {
        float2 c = make_float2(0.f, 0.f), q = c;
#pragma unroll 1
        for (int e = 0; e < 2; e++) {                            /* rolled: one copy of the cold code */
          const float2 t = exact_output(P, iq16, j - e, n_total, rot);
          if (e == 0) c = t; else q = t;
        }
        v1 = discriminate<true>(q.x, q.y, c.x, c.y);
      }
      w.xs[i] = v1;
    }
    wave_lds_sync();
  } else {
    /* 1. the size + 2 decimated samples y[n - size - 1 .. n] in exact arithmetic, one or two per lane, into xs (as (I, Q)
     *    pairs): each is computed ONCE (the window's discriminator samples share them pairwise), and the lane's loads of
     *    both rounds are in flight together */
    float2 *ys = reinterpret_cast<float2 *>(w.xs);
    {
      /* two rounds (lanes 0 .. 63, then 0 .. size - 63); the second round's cache lines are touched (one dword each) before the
       * first round's arithmetic, so that its own loads find them close by - both rounds' words in registers at once do not
       * fit beside the resident tap operands of the matrix-pipe stage C */
      const int ja = n - size - 1 + lane, jb = ja + 64;
      const bool hb = lane + 64 < size + 2;
      uint4 q[4];
      exact_load_words(iq16, ja < 0 ? 0 : ja, n_total, q);
      uint32_t touch = 0;
      if (hb && jb >= 3 && jb < n_total) touch = reinterpret_cast<const uint32_t *>(iq16 + (jb - 3))[0] ^ reinterpret_cast<const uint32_t *>(iq16 + jb)[0];
      const float2 ya = exact_from_words(P, q, rot);
      ys[lane] = ja >= 0 ? ya : make_float2(0.f, 0.f);
      asm volatile("" :: "v"(touch));
      if (hb) {
        exact_load_words(iq16, jb >= 0 ? jb : 0, n_total, q);
        const float2 yb = exact_from_words(P, q, rot);
        ys[lane + 64] = jb >= 0 ? yb : make_float2(0.f, 0.f);
      }
    }
    wave_lds_sync();
    FMD_RSTAMP(1)
    /* 2. the discriminator samples v[n - size .. n] from them (or from the history where the reference's value is not a
     *    function of the IQ bytes alone), kept in the lane until every lane has read its pairs */
    float val[2];
  #pragma unroll
    for (int u = 0; u < 2; u++) {
      const int i = lane + 64 * u;
      val[u] = 0.f;
      if (i <= size) {
        const int j = n - size + i;
        bool keep = j <= 3;
        if (!keep && P.resample && M > 1) {
          const int blk = j / M;
          if (j - blk * M == 1) {                                  /* did block blk start with an emit? (Q1) */
            const uint32_t a = (uint32_t)(((unsigned long long)acc_launch + (unsigned long long)blk * M * (uint32_t)P.slow) %
                                          (uint32_t)P.fast);
            keep = a + (uint32_t)P.slow >= (uint32_t)P.fast;
          }
        }
        if (keep) {
          val[u] = w.v[HV + (j - n_tile)];
        } else {
          const float2 q = ys[i], c = ys[i + 1];                   /* y[j - 1], y[j] */
          val[u] = discriminate<true>(q.x, q.y, c.x, c.y);
        }
      }
    }
    wave_lds_sync();
  #pragma unroll
    for (int u = 0; u < 2; u++)
      if (lane + 64 * u <= size) w.xs[lane + 64 * u] = val[u];
    wave_lds_sync();
    FMD_RSTAMP(2)
  }
  /* 3. the pilot and L-R sums in the reference's order (ref_sums3: the window is xs[1 .. size], one sample earlier xs[0 ..]) */
  float vp1, vs1, vp0;
  if constexpr (HV == 96) {
    ref_sums3(tap_mpx, &w.xs[1], w, lane, vp1, vs1, vp0);
  } else {
    const int role = lane < 3 ? lane : 0;                        /* generic sizes: one sum per lane, taps and window from LDS step by step */
    const float *xw = &w.xs[role == 2 ? 0 : 1];
    const float *tw = reinterpret_cast<const float *>(tap_mpx) + (role == 1 ? 2 : 1);
    float sum = 0.f;
#pragma unroll 9
    for (int k = 0; k < half; k++) sum = mac<true>(sum, xw[k] + xw[size - 1 - k], tw[4 * k]);
    vp1 = __shfl(sum, 0); vs1 = __shfl(sum, 1); vp0 = __shfl(sum, 2);
  }
  FMD_RSTAMP(3)
  const float bs = vs1 * carrier_of<true>(vp1, vp0, P.swf, P.cwf);
  if (lane == 0) {
    if constexpr (WM::kLimbs) limb_store(w, WM::kBsRow, WM::kVbh + m, bs);
    else w.ms[HV + m].y = bs;
  }
  wave_lds_sync();
  FMD_RSTAMP(4)
}

/* Block-start quirk (SURVEY.md section 0, Q1; src/rtl_fm_player.c:534-598):
 * when the resampler emits on sample 0 of a block, the right-channel output is
 * stored over discriminator sample 1 before that sample is read. */
template <bool EX, int HV, typename WM>
__device__ __forceinline__ void q1_patch(const fmdk_params &P, const f4 *tap_mpx, WM &w, int lane,
                                         float pp) {
  float f = 0.f;
  if (lane < 3) {
    const int size = P.size, half = P.half;
    const int x0 = HV - (size - 1);
    const float *tap = reinterpret_cast<const float *>(tap_mpx) + lane;
    for (int k = 0; k < half; k++)
      f = mac<EX>(f, w.v[(x0 + k)] + w.v[(x0 + size - 1 - k)], tap[4 * k]);
  }
  const float vp = __shfl(f, 1), vs = __shfl(f, 2);
  if (lane == 0) {
    w.ms[HV] = make_float2(f, vs * carrier_of<EX>(vp, pp, P.swf, P.cwf));
    float om, os;
    fir_stereo<EX, 0>(P, tap_mpx, tap_mpx, &w.ms[HV], om, os);
    w.v[(HV + 1)] = om - os;
  }
}

