/* flush.inc - part of the fused IQ -> PCM kernel (included by fmd_kernels.inc inside its anonymous namespace; not a translation unit of its own).
 * Stage F: de-emphasis, f32 -> s16, PCM store (reference :687-735) - the exact kernels' pending-frame flush and the fast kernels' per-tile flush (DPP scan). */

/* ---- stage F: de-emphasis + s16 + store ----------------------------------- */

/* Exact kernels (the fast ones flush every tile with flush_tile_fast).  De-emphasis is a
 * first-order recurrence (:687-709).  Each lane produces DEEMPH_GROUP consecutive frames of one
 * channel; a lane whose segment does not start at the first pending frame restarts the
 * recurrence P.warm frames early from zero (lambda^warm < 1e-25, see fmd_resolve.c), the
 * others continue from the carried state, so the result equals the sequential evaluation. */
template <bool EX, int CH, int HV, typename WM>
__device__ __forceinline__ void flush_frames(const fmdk_params &P, WM &w, int lane, int pend,
                                             int16_t *pcm_out, float *mpx_dbg, bool store) {
  if constexpr (FMD_ABLATE & 16) return;
  const int frames = pend / CH;
  const float coef = P.coef;
  if (mpx_dbg) {
    for (int i = lane; i < pend; i += 64) mpx_dbg[i] = w.fr[fidx(i)];
  }
  if (P.deemph) {
    const int groups = (frames + DEEMPH_GROUP - 1) / DEEMPH_GROUP;
    const float lam = P.lambda;
    const int warm = P.warm;
    float ylast = 0.f;
    bool have_last = false;
    if (lane < groups * CH) {
      const int g = lane / CH, c = lane % CH;
      const int f_out = g * DEEMPH_GROUP;
      const int f_end = min(f_out + DEEMPH_GROUP, frames);
      int fb = f_out - warm;                  /* warm is a multiple of 16 (host), so is f_out */
      float y = 0.f;
      if (fb <= 0) { fb = 0; y = w.de[c]; }
      /* blocks of 16 steps: the 16 inputs do not depend on the recurrence, so they
       * are read together (one LDS latency per block instead of one per step) */
      for (; fb < f_out; fb += 16) {          /* warm-up blocks: whole, nothing stored */
        f8 xa, xb;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          xa[j] = w.fr[fidx((fb + j) * CH + c)];
          xb[j] = w.fr[fidx((fb + 8 + j) * CH + c)];
        }
#pragma unroll
        for (int j = 0; j < 16; j++) {
          const float x = j < 8 ? xa[j & 7] : xb[j & 7];
          const float t = y - x;
          if constexpr (EX) y = x + lam * t;
          else y = __builtin_fmaf(lam, t, x);
        }
      }
      {                                        /* the lane's own 16 frames (the last group may be short) */
        f8 xa, xb;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          xa[j] = w.fr[fidx(min(f_out + j, frames - 1) * CH + c)];
          xb[j] = w.fr[fidx(min(f_out + 8 + j, frames - 1) * CH + c)];
        }
        int16_t *o = pcm_out + f_out * CH + c;
#pragma unroll
        for (int j = 0; j < 16; j++) {
          const float x = j < 8 ? xa[j & 7] : xb[j & 7];
          const float t = y - x;
          float yn;
          if constexpr (EX) yn = x + lam * t;
          else yn = __builtin_fmaf(lam, t, x);
          const bool live = f_out + j < f_end;
          y = live ? yn : y;
          if (store && live) o[j * CH] = to_s16(yn, coef);
        }
      }
      ylast = y;
      have_last = (f_end == frames);
    }
    if (have_last) w.de[lane % CH] = ylast;      /* all lanes have read de[] above (same wave) */
  } else if (store) {
    for (int i = lane; i < pend; i += 64) pcm_out[i] = to_s16(w.fr[fidx(i)], coef);
  }
  wave_lds_sync();               /* de[] and fr[] are handed to the next flush / the next resampler pass */
}


/* Fast kernels: de-emphasis, f32 -> s16 and the PCM store of ONE TILE's frames (fr[0 .. frames * CH)),
 * right after the resampler has written them - no pending buffer, no per-frame predication.
 * Lane 32 c + g (stereo) or g (mono) takes the G consecutive frames of group g, channel c.
 * y[n] = x[n] + lam (y[n-1] - x[n]) is linear: each lane runs its G frames from a zero state (z); the
 * states at the group ends, Y[g] = z[G-1][g] + a Y[g-1] with a = lam^G and the carried state as Y[-1],
 * follow from a scan over the lanes done with DPP moves - distances 1, 2, 4, 8 inside the 16-lane rows
 * (weights a, a^2, a^4, a^8), then each row's last lane into the next row (weight a^(i+1) for the row's
 * i-th lane; mono spans four rows and takes a second such step) - and a last pass adds lam^(j+1) times the
 * state entering the group.  With de-emphasis off lam and its powers are zero and the same code passes x
 * through.  Stereo: the left-channel lanes fetch the right channel's values from lane + 32, pack (L, R)
 * pairs and store their G frames as G / 4 16-byte words. */
template <int CH, int G, typename WM, typename UNI, typename PCM>
__device__ __forceinline__ void flush_tile_fast(const fmdk_params &P, const UNI &U, WM &w, int lane, int frames, PCM *pcm_out,
                                                float *mpx_dbg, bool store) {
  if constexpr (FMD_ABLATE & 16) return;
  static_assert(G == 4 || G == 8 || (G == 2 && CH == 1) || (G == 3 && CH == 2), "group sizes the host chooses from");
  const float coef = U.coef();
  if (mpx_dbg) {
    for (int i = lane; i < frames * CH; i += 64) mpx_dbg[i] = w.fr[i];
  }
  const int groups = (frames + G - 1) / G;               /* host: groups <= 64 / CH */
  const int g = CH == 2 ? (lane & 31) : lane, c = CH == 2 ? (lane >> 5) : 0;
  const bool mine = g < groups;
  const float lam = P.lam_eff;
  const FMD_LDS float *x0 = opaque_lds(&w.fr[0]) + (mine ? g * (G * CH) + c : 0);
  float x[G], z[G];
#pragma unroll
  for (int j = 0; j < G; j++) x[j] = x0[CH * j];          /* a short last group reads stale slots: they only reach
                                                            z[] entries nothing uses (no store, no state) */
  {
    float y = 0.f;
#pragma unroll
    for (int j = 0; j < G; j++) {
      y = __builtin_fmaf(lam, y - x[j], x[j]);
      z[j] = y;
    }
  }
  const float de_c = w.de[c];
  const f4 lp0 = U.template lam_pow4<0>(), lp1 = U.template lam_pow4<4>();     /* lam^(j+1), j < 8 */
  const f4 sc0 = U.template lam_scan4<0>(), sc1 = U.template lam_scan4<4>();   /* a^(2^k), k < 8 */
  float yend = (g == 0) ? __builtin_fmaf(sc0[0], de_c, z[G - 1]) : z[G - 1];
  yend = __builtin_fmaf(sc0[0], dpp0<DPP_ROW_SHR + 1>(yend), yend);
  yend = __builtin_fmaf(sc0[1], dpp0<DPP_ROW_SHR + 2>(yend), yend);
  yend = __builtin_fmaf(sc0[2], dpp0<DPP_ROW_SHR + 4>(yend), yend);
  yend = __builtin_fmaf(sc0[3], dpp0<DPP_ROW_SHR + 8>(yend), yend);
  /* a^(i+1) for the row's i-th lane (zero with de-emphasis off: log2 a = -1e30) */
  const float wpos = __builtin_amdgcn_exp2f((float)((lane & 15) + 1) * P.log2_a);
  yend = __builtin_fmaf(wpos, dpp0<DPP_ROW_BCAST15, 0xa>(yend), yend);   /* rows 1, 3 take the end of rows 0, 2 */
  if constexpr (CH == 1) {
    const float w31 = (lane >= 48) ? wpos * sc1[0] : wpos;                /* rows 2, 3 take the end of row 1: a^(i+1), a^(i+17) */
    yend = __builtin_fmaf(w31, dpp0<DPP_ROW_BCAST31, 0xc>(yend), yend);
  }
  const float up = dpp0<DPP_WAVE_SHR1>(yend);            /* the state entering the group: the previous group's end */
  const float carry = (g == 0) ? de_c : up;
  float y[G];
#pragma unroll
  for (int j = 0; j < G; j++) y[j] = __builtin_fmaf(j < 4 ? lp0[j & 3] : lp1[j & 3], carry, z[j]);
  /* the carried state: the last frame of the last group */
  const int last = frames - 1;
  if (mine && g == groups - 1 && frames > 0) {
    float yl = y[0];
#pragma unroll
    for (int j = 1; j < G; j++) yl = (last - G * g >= j) ? y[j] : yl;
    w.de[c] = yl;                                        /* every lane has read de[] above (same wave) */
  }
  if (!store || frames == 0) return;
  /* clip + round: the integer sits in the low mantissa bits of t + 1.5 * 2^23 (to_s16) */
  uint32_t b[G];
#pragma unroll
  for (int j = 0; j < G; j++)
    b[j] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_fmed3f(y[j] * coef, -32768.0f, 32767.0f) + 12582912.0f);
  const int f0 = G * g;
  const bool whole = f0 + G <= frames;
  if constexpr (CH == 2) {
    const int from = ((lane + 32) & 63) << 2;             /* the right channel of group g sits in lane g + 32 */
    uint32_t pk[G];
#pragma unroll
    for (int j = 0; j < G; j++) {
      const uint32_t r = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)b[j]);
      pk[j] = __builtin_amdgcn_perm(r, b[j], 0x05040100u);                  /* {L.lo16, R.lo16} */
    }
    if (c == 0 && mine) {
      auto *o = ptr_as<uint32_t>(pcm_out) + f0;                            /* pcm_out is 4-byte aligned (whole frames) */
      if (whole) {
        if constexpr (G == 3) {
          typedef uint32_t u3u __attribute__((ext_vector_type(3), aligned(4)));
          *ptr_as<u3u>(o) = u3u{pk[0], pk[1], pk[2]};                          /* three frames: one 12-byte store */
        } else {
          typedef uint32_t u4u __attribute__((ext_vector_type(4), aligned(4)));
#pragma unroll
          for (int j = 0; j < G; j += 4) *ptr_as<u4u>(o + j) = u4u{pk[j], pk[j + 1], pk[j + 2], pk[j + 3]};
        }
      } else {
#pragma unroll
        for (int j = 0; j < G; j++)
          if (f0 + j < frames) o[j] = pk[j];
      }
    }
  } else {
    if (mine) {
      PCM *o = pcm_out + f0;
#pragma unroll
      for (int j = 0; j < G; j++)
        if (whole || f0 + j < frames) o[j] = (int16_t)b[j];
    }
  }
}

