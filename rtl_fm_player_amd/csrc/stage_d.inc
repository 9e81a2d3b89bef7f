/* stage_d.inc - part of the fused IQ -> PCM kernel (included by fmd_kernels.inc inside its anonymous namespace; not a translation unit of its own).
 * Stage D: the rational resampler's second-stage low-pass at the emit instants (reference :570-598 stereo, :500-532 mono) - the vector-ALU forms (fir_*, resample_*), the emit-index arithmetic, and the decimating banded products of FMD_MATH_FAST_MFMA_F (resample_tile_dec, resample_mono_dec). */

/* Symmetric fm FIR over the `2*HALF` floats ending at newest (mono, :511-529).
 * Groups of 8 taps (two s_load_dwordx4 of taps, 16 window reads per group) in a rolled
 * loop: the register footprint stays small next to the IQ words in flight for the next
 * tile, and the other workers of the SIMD cover the LDS latency (double-buffering the
 * groups measured no faster). */
template <typename T, int HALF>
__device__ __forceinline__ void fir_group_load(const FMD_LDS T *x0, int g, T (&xl)[8], T (&xh)[8]) {
  constexpr int S = 2 * HALF;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int k = 8 * g + i;       /* k >= HALF in the last group: still inside the window, and the tap is zero */
    xl[i] = x0[k];
    xh[i] = x0[S - 1 - k];
  }
}
template <bool EX>
__device__ __forceinline__ void fir_group_sum(int g, const float (&xl)[8], const float (&xh)[8], float &acc) {
  const f4 ta = FMD_KTAP4(fm, 8 * g), tb = FMD_KTAP4(fm, 8 * g + 4);
#pragma unroll
  for (int i = 0; i < 8; i++) acc = mac<EX>(acc, xl[i] + xh[i], i < 4 ? ta[i & 3] : tb[i & 3]);
}
template <bool EX>
__device__ __forceinline__ void fir_group_sum(int g, const f2 (&xl)[8], const f2 (&xh)[8], float &om, float &os) {
  const f4 ta = FMD_KTAP4(fm, 8 * g), tb = FMD_KTAP4(fm, 8 * g + 4);
  f2 acc = {om, os};                         /* both channels at once: packed add and multiply-add */
#pragma unroll
  for (int i = 0; i < 8; i++) acc = mac2<EX>(acc, xl[i] + xh[i], i < 4 ? ta[i & 3] : tb[i & 3]);
  om = acc.x; os = acc.y;
}
/* fast kernels: the same with FIR_CHAINS independent running sums (taps i mod FIR_CHAINS), joined by the caller: a single
 * sum is a chain of 45 dependent multiply-adds, which one worker can issue only every ~8 cycles - with two workers per SIMD
 * nobody fills those gaps */
constexpr int FIR_CHAINS = 4;
__device__ __forceinline__ void fir_group_sum_chains(int g, const f2 (&xl)[8], const f2 (&xh)[8], f2 (&acc)[FIR_CHAINS]) {
  const f4 ta = FMD_KTAP4(fm, 8 * g), tb = FMD_KTAP4(fm, 8 * g + 4);
#pragma unroll
  for (int i = 0; i < 8; i++) acc[i % FIR_CHAINS] = mac2<false>(acc[i % FIR_CHAINS], xl[i] + xh[i], i < 4 ? ta[i & 3] : tb[i & 3]);
}

template <bool EX, int HALF>
__device__ __forceinline__ float fir_mono(const fmdk_params &P, const f4 *tap_mpx, const f4 *fm_lin,
                                          const float *newest) {
  float acc = 0.f;
  if constexpr (HALF > 0) {
    constexpr int S = 2 * HALF, NG = (HALF + 7) / 8;
    static_assert(NG % 2 == 0, "groups are processed in pairs");
    const FMD_LDS float *x0 = opaque_lds(newest - (S - 1));
    float al[8], ah[8];
    if constexpr (EX) {
#pragma unroll 1
      for (int g = 0; g < NG; g++) {
        fir_group_load<float, HALF>(x0, g, al, ah);
        fir_group_sum<EX>(g, al, ah, acc);
      }
    } else {
      /* fast: neighbouring taps as one packed add / multiply-add with the tap pair as it lies in
       * the SGPRs, even and odd taps in the two halves of one accumulator (summed at the end) */
      f2 acc2 = {0.f, 0.f};
#pragma unroll 1
      for (int g = 0; g < NG; g++) {
        fir_group_load<float, HALF>(x0, g, al, ah);
        const f4 ta = FMD_KTAP4(fm, 8 * g), tb = FMD_KTAP4(fm, 8 * g + 4);
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
          const f2 p = pk_add_swap(f2{al[i], al[i + 1]}, f2{ah[i + 1], ah[i]});   /* the high side as it lies in LDS, added descending */
          const f2 t = i < 4 ? f2{ta[i], ta[i + 1]} : f2{tb[i - 4], tb[i - 3]};
          acc2 = __builtin_elementwise_fma(p, t, acc2);
        }
      }
      acc = acc2.x + acc2.y;
    }
  } else {
    const int size = P.size, half = P.half;
    const float *x = newest - (size - 1);
    for (int k = 0; k < half; k++) acc = mac<EX>(acc, x[k] + x[size - 1 - k], tap_mpx[k].x);
  }
  return acc;
}

/* The two stage-2 FIRs of the stereo path at one instant (:574-591), same scheme. */
template <bool EX, int HALF>
__device__ __forceinline__ void fir_stereo(const fmdk_params &P, const f4 *tap_mpx, const f4 *fm_lin,
                                           const float2 *newest, float &om, float &os) {
  om = 0.f; os = 0.f;
  if constexpr (HALF > 0) {
    constexpr int S = 2 * HALF, NG = (HALF + 7) / 8;
    static_assert(NG % 2 == 0, "groups are processed in pairs");
    /* {L+R, L-R} pairs as 2-vectors: one 8-byte LDS read each (the float2 struct is
     * split into two 4-byte reads when the SLP vectoriser is off) */
    const FMD_LDS f2 *x0 = opaque_lds(reinterpret_cast<const f2 *>(newest) - (S - 1));
    f2 al[8], ah[8], bl[8], bh[8];
    fir_group_load<f2, HALF>(x0, 0, al, ah);
    if constexpr (EX) {
#pragma unroll
      for (int g = 0; g < NG; g += 2) {
        fir_group_load<f2, HALF>(x0, g + 1, bl, bh);
        fir_group_sum<EX>(g, al, ah, om, os);
        fir_group_load<f2, HALF>(x0, g + 2 < NG ? g + 2 : g, al, ah);
        fir_group_sum<EX>(g + 1, bl, bh, om, os);
      }
    } else {
      f2 acc[FIR_CHAINS] = {};
#pragma unroll
      for (int g = 0; g < NG; g += 2) {
        fir_group_load<f2, HALF>(x0, g + 1, bl, bh);
        fir_group_sum_chains(g, al, ah, acc);
        fir_group_load<f2, HALF>(x0, g + 2 < NG ? g + 2 : g, al, ah);
        fir_group_sum_chains(g + 1, bl, bh, acc);
      }
      f2 sum = acc[0];
#pragma unroll
      for (int c = 1; c < FIR_CHAINS; c++) sum += acc[c];
      om = sum.x; os = sum.y;
    }
  } else {
    const int size = P.size, half = P.half;
    const float2 *x = newest - (size - 1);
    for (int k = 0; k < half; k++) {
      const float2 a = x[k], b = x[size - 1 - k];
      const float t = tap_mpx[k].x;
      om = mac<EX>(om, a.x + b.x, t);
      os = mac<EX>(os, a.y + b.y, t);
    }
  }
}

/* ---- stage D: resampler outputs ------------------------------------------ */

/* local index of the q-th emit of this tile; acc_t = accumulator at tile start.
 * i = ceil(((q+1) * fast - acc_t) / slow) - 1, by a float estimate corrected
 * with exact integer checks. */
/* Resampler bookkeeping of one tile: frames emitted nq = (acc + tm slow) / fast and the
 * accumulator after it.  Wave-uniform; a float estimate corrected by integer compares
 * replaces the 64-bit division when the numerator fits 32 bits (any sane pair of rates). */
__device__ __forceinline__ void tile_frames(uint32_t acc, int tm, uint32_t slow, uint32_t fast, uint32_t magic,
                                            uint32_t shift, float inv_fast, int &nq, uint32_t &acc_next) {
  if (magic) {
    /* x = acc + tm slow < 2^30 (host): floor(x / fast) = mulhi(x, magic) >> shift, all scalar */
    const uint32_t x = acc + (uint32_t)tm * slow;
    const uint32_t e = (uint32_t)(((unsigned long long)x * magic) >> 32) >> shift;
    nq = (int)e;
    acc_next = x - e * fast;
    return;
  }
  const unsigned long long x64 = (unsigned long long)acc + (unsigned long long)tm * slow;
  if (x64 >> 32) {
    uint32_t fast_o = fast;                               /* (opaque: see the chunk-start divisions in the kernel) */
    asm volatile("" : "+s"(fast_o));
    nq = (int)(x64 / fast_o);
    acc_next = (uint32_t)(x64 % fast_o);
  } else {
    const uint32_t x = (uint32_t)x64;
    uint32_t e = (uint32_t)((float)x * inv_fast);          /* 1.0f / (float)fast, made by the host */
    e = __builtin_amdgcn_readfirstlane(e);
    while ((unsigned long long)e * fast > x) e--;          /* estimate within a few units */
    while ((unsigned long long)(e + 1) * fast <= x) e++;
    nq = (int)e;
    acc_next = x - e * fast;
  }
}

/* The same by integer arithmetic: i = floor((need - 1) / slow), need - 1 = q fast + (fast - acc_t - 1) < 2^29,
 * as a multiply-high by the host's magic number m = ceil(2^(32 + sh) / slow) (exact for every
 * numerator below 2^29, see fmd_resolve.c) and a shift: three instructions. */
__device__ __forceinline__ int emit_index_magic(uint32_t c0, int q, uint32_t fast, uint32_t magic, uint32_t sh) {
  const uint32_t n = (uint32_t)q * fast + c0;           /* v_mad_u32_u24: q < 2^24, fast < 2^24 */
  return (int)(__umulhi(n, magic) >> sh);
}

__device__ __forceinline__ int emit_index(uint32_t acc_t, int q, uint32_t slow, uint32_t fast,
                                          float inv_slow) {
  /* ceil(need / slow) - 1 with need = (q + 1) fast - acc_t > 0: float estimate of the
   * quotient (off by at most one: need / slow <= tile length), exact integer remainder */
  const uint32_t need = (uint32_t)(q + 1) * fast - acc_t;
  uint32_t e = (uint32_t)((float)need * inv_slow);
  int32_t r = (int32_t)(need - e * slow);
  if (r < 0) { e--; r += (int32_t)slow; }
  else if (r >= (int32_t)slow) { e++; r -= (int32_t)slow; }
  return (int)e - (r == 0);
}

/* Fast mono kernels, 128 taps, rate_out = 2 rate_out2 (narrow FM: 25 k -> 12.5 k, BASELINE.json configs[4]):
 * every second sample is a frame, so a lane takes FOUR CONSECUTIVE FRAMES (samples n_j = i0 + 8 lane + 2 j)
 * and walks the 64 tap pairs with its window in registers, read as aligned 16-byte words - 38 ds_read_b128
 * per lane and tile where the frame-per-lane form issues 512 ds_read_b32 (it is LDS bound: 0.56 ms
 * against 0.36 ms for 2.4 Msps mono on the same bytes).  With x[i] = v[8 lane - 128 + i]:
 *   frame j = sum_k t[k] (x[i0 + 2j + 1 + k] + x[i0 + 2j + 128 - k])
 * Two neighbouring taps share a packed add / multiply-add, (x[L], x[L+1]) + (x[H], x[H-1]) times
 * (t[k], t[k+1]); both pairs are even-aligned registers when k = i0 + 1 (mod 2).  I0 (the tile's first
 * emit, 0 or 1) is fixed for a stream: I0 = 1 pairs the taps (0,1) .. (62,63); I0 = 0 pairs (1,2) .. (63,64)
 * from the table shifted by one (t[64] = 0) and adds tap 0 on its own. */
template <int I0, int HV, typename WM>
__device__ __forceinline__ void resample_mono_2to1(WM &w, int lane, int pend) {
  static_assert(HV == 128, "window base alignment");
  const FMD_LDS f4 *xw = reinterpret_cast<const FMD_LDS f4 *>(opaque_lds(&w.v[8 * lane]));   /* word u = x[4u .. 4u+3] */
  constexpr int K0 = I0 ? 0 : 1;                       /* first tap of the first pair */
  /* pair P (x[2P], x[2P+1]):  low of (j, pair i) = P_lo = (I0 + 2j + 1 + K0 + 2i) / 2,  high = (I0 + 2j + 127 - K0 - 2i) / 2 */
  constexpr int LB = (I0 + 1 + K0) / 2, HB = (I0 + 127 - K0) / 2;        /* + j + i  /  + j - i */
  f2 acc[4] = {};
  f4 Lw[20] = {}, Hw[36] = {};                         /* constant indices only: SSA values */
  /* chunk c = tap pairs i = 4c .. 4c+3: low pairs LB + 4c + [0, 6], high pairs HB - 4c + [-3, 3] */
  auto need_lo = [&](auto u_) { constexpr int u = decltype(u_)::value; Lw[u] = xw[u]; };
  auto need_hi = [&](auto u_) { constexpr int u = decltype(u_)::value; Hw[u] = xw[u]; };
  constexpr int LW0 = LB / 2, HW0 = (HB - 3) / 2;      /* first words of chunk 0 */
  static_for<0, 4>([&](auto i_) { need_lo(std::integral_constant<int, LW0 + decltype(i_)::value>{}); });
  static_for<0, 4>([&](auto i_) { need_hi(std::integral_constant<int, HW0 + decltype(i_)::value>{}); });
  int koff = 0;
  asm volatile("" : "+s"(koff));
  static_for<0, 8>([&](auto c_) {
    constexpr int c = decltype(c_)::value;
    /* taps of this chunk: pairs (K0 + 8c + 2i, +1), i < 4 = eight consecutive entries of fm (I0 = 1) or fm_sh (I0 = 0) */
    const f4 ta = I0 ? FMD_KTAP4(fm, 8 * c + koff) : FMD_KTAP4(fm_sh, 8 * c + koff);
    const f4 tb = I0 ? FMD_KTAP4(fm, 8 * c + 4 + koff) : FMD_KTAP4(fm_sh, 8 * c + 4 + koff);
    if constexpr (c < 7) {                              /* next chunk's two new words on each side */
      need_lo(std::integral_constant<int, LW0 + 4 + 2 * c>{});
      need_lo(std::integral_constant<int, LW0 + 5 + 2 * c>{});
      need_hi(std::integral_constant<int, HW0 - 2 - 2 * c>{});
      need_hi(std::integral_constant<int, HW0 - 1 - 2 * c>{});
      asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]) :: "memory");
    }
    static_for<0, 4>([&](auto i_) {
      constexpr int i = decltype(i_)::value;
      const f2 t = i < 2 ? f2{ta[2 * i], ta[2 * i + 1]} : f2{tb[2 * i - 4], tb[2 * i - 3]};
      static_for<0, 4>([&](auto j_) {
        constexpr int j = decltype(j_)::value;
        constexpr int pl = LB + j + 4 * c + i, ph = HB + j - 4 * c - i;
        static_assert(pl / 2 >= LW0 && pl / 2 < 20 && ph / 2 >= 0 && ph / 2 < 36, "window word out of range");
        const f4 lw = Lw[pl / 2], hw = Hw[ph / 2];
        const f2 lp = (pl & 1) ? f2{lw.z, lw.w} : f2{lw.x, lw.y};
        const f2 hq = (ph & 1) ? f2{hw.z, hw.w} : f2{hw.x, hw.y};      /* the high pair as stored; it is added descending: (x[H], x[H-1]) */
        acc[j] = __builtin_elementwise_fma(pk_add_swap(lp, hq), t, acc[j]);
      });
    });
    if constexpr (c < 7)
      asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+s"(koff) :: "memory");
  });
  f4 out;
#pragma unroll
  for (int j = 0; j < 4; j++) out[j] = acc[j].x + acc[j].y;
  if constexpr (I0 == 0) {                              /* tap 0 on its own: x[2j + 1] + x[2j + 128] */
    const float t0 = FMD_KTAP4(fm, 0)[0];
    const f4 a0 = xw[0], a1 = xw[1], b0 = xw[32], b1 = xw[33];
    out[0] = __builtin_fmaf(t0, a0.y + b0.x, out[0]);
    out[1] = __builtin_fmaf(t0, a0.w + b0.z, out[1]);
    out[2] = __builtin_fmaf(t0, a1.y + b1.x, out[2]);
    out[3] = __builtin_fmaf(t0, a1.w + b1.z, out[3]);
  }
  *reinterpret_cast<f4 *>(&w.fr[pend + 4 * lane]) = out;             /* frames 4 lane .. 4 lane + 3 (unpadded: fast kernels) */
}

/* Fast mono kernels, 128 taps, any ratio but 2:1: SIXTEEN FRAMES PER PASS, FOUR LANES PER FRAME.  Lane 4 f + o takes
 * frame 16 pass + f and the tap pairs k = 8 o + kk (+ 32), kk < 8: sixteen of the 64 pairs (:511-529 sums them all in
 * one loop), its partial sum meets the other three by two DPP adds inside the quad.  Why: with a frame per lane the 32
 * lanes of an LDS cycle read x[i_q + c] for 32 different frames, and at 300 k -> 48 k (i_q = 25 (q / 4) + {0, 6, 12, 18})
 * no assignment of frames to lanes puts 32 of them on 32 different banks - every ds_read_b32 of the stage took two
 * cycles (SQ_LDS_BANK_CONFLICT 56 M of the mono kernel's 59 M per launch).  Here the 32 lanes of a cycle are 8
 * consecutive frames x 4 octants: the frames' positions are all different mod 8 (25 = 1 mod 8) and the octants add
 * 0 / 8 / 16 / 24, so low side (x[i - 127 + k]) and high side (x[i - k]) each touch all 32 banks once.  The lane's
 * sixteen taps stay in registers for the whole kernel. */
template <int HV, typename WM, typename EMIT>
__device__ __forceinline__ void resample_mono_oct(const f4 (&tp)[4], WM &w, int lane, int nq, int pend, bool perm4, const EMIT &emit_at) {
  const int o = lane & 3, fl = lane >> 2;
  /* which of an iteration's 32 frames: with consecutive frames the 8 of an LDS cycle are conflict-free for one resampler phase
   * in four only (frames five apart are 31 OR 32 samples apart; profiles/archive/r03l_lds_patterns.txt).  When four frames are a whole, odd
   * number of samples apart (perm4: 25 at 300 k -> 48 k) a cycle takes every fourth frame instead: their distances are exact
   * multiples of that odd number, never 0 mod 8, whatever the phase. */
  const int f0 = perm4 ? (fl >> 3) + 4 * (fl & 7) : fl, fu = perm4 ? 2 : 16;
  /* two passes (32 frames) per iteration: their reads and sums are independent, one LDS latency for both */
  for (int q0 = 0; q0 < nq; q0 += 32) {
    int q[2], i[2];
    bool act[2];
    float a[2][16], b[2][16];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      q[u] = q0 + fu * u + f0;
      act[u] = q[u] < nq;
      i[u] = emit_at(min(q[u], nq - 1));            /* (idle lanes compute the last frame again: no branch around the index arithmetic;
                                                        nq >= 1 inside this loop, so the index is a real frame's - a tile that emits nothing never gets here) */
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const FMD_LDS float *xl = opaque_lds(&w.v[HV + i[u] - 127 + 8 * o]);      /* x[i - 127 + k], k = 8 o + kk (+ 32) */
      const FMD_LDS float *xh = opaque_lds(&w.v[HV + i[u] - 8 * o - 39]);       /* x[i - k] = xh[39 - kk], xh[7 - kk]: one base register, offsets >= 0 */
#pragma unroll
      for (int kk = 0; kk < 8; kk++) {
        a[u][kk] = xl[kk]; a[u][8 + kk] = xl[32 + kk];
        b[u][kk] = xh[39 - kk]; b[u][8 + kk] = xh[7 - kk];
      }
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      f2 acc = {0.f, 0.f}, acc1 = {0.f, 0.f};                                   /* two chains: half the dependent latency */
#pragma unroll
      for (int j = 0; j < 16; j += 4) {
        const f4 t = tp[j >> 2];
        /* the high side descends in memory: its pairs are named as they lie in LDS and added swapped (pk_add_swap) */
        acc = __builtin_elementwise_fma(pk_add_swap(f2{a[u][j], a[u][j + 1]}, f2{b[u][j + 1], b[u][j]}), f2{t.x, t.y}, acc);
        acc1 = __builtin_elementwise_fma(pk_add_swap(f2{a[u][j + 2], a[u][j + 3]}, f2{b[u][j + 3], b[u][j + 2]}), f2{t.z, t.w}, acc1);
      }
      acc += acc1;
      float sum = acc.x + acc.y;
      sum += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, sum), 0xB1, 0xf, 0xf, true));   /* quad_perm [1,0,3,2] */
      sum += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, sum), 0x4E, 0xf, 0xf, true));   /* quad_perm [2,3,0,1] */
      if (act[u] && o == 0) w.fr[pend + q[u]] = sum;                            /* (fast kernels only: unpadded) */
    }
  }
}

template <bool EX, int MODE, int HALF, int HV, typename WM, typename EMIT>
__device__ __forceinline__ void resample_tile_with(const fmdk_params &P, const f4 *tap_mpx, const f4 *fm_lin, WM &w,
                                                   int lane, uint32_t acc_t, int nq, int pend, const EMIT &emit_at) {
  const uint32_t slow = (uint32_t)P.slow;
  const bool rs = P.resample != 0;
  /* lane -> frame permutation: the 16 lanes that share an LDS cycle take every fourth
   * frame.  At 300k -> 48k four frames are exactly 25 samples apart, so those lanes'
   * 8-byte window reads fall on 16 different bank pairs; with lane == frame the
   * 6.25-sample spacing collides on two of them. */
  /* (only when four frames are a whole, odd number of samples apart; other ratios keep
   * lane == frame, e.g. 2:1 where the permutation would make a 4-way conflict) */
  if constexpr (!EX && MODE == 1 && HALF == 64) {
    if (P.mono_2to1) {                       /* rate_out = 2 rate_out2: four consecutive frames per lane */
      if (acc_t < slow) resample_mono_2to1<1, HV>(w, lane, pend);    /* acc_t + slow < fast: the first emit is sample 1 */
      else resample_mono_2to1<0, HV>(w, lane, pend);                 /* sample 0 emits */
      return;
    }
    if (rs) {                                /* four lanes per frame, conflict-free window reads */
      const int o4 = 2 * (lane & 3);
      const f4 tp[4] = {fm_lin[o4], fm_lin[o4 + 1], fm_lin[8 + o4], fm_lin[9 + o4]};   /* fm[8 o .. 8 o + 7], fm[32 + 8 o ..] */
      resample_mono_oct<HV>(tp, w, lane, nq, pend, P.perm4 != 0, emit_at);
      return;
    }
  }
  const bool perm4 = P.perm4 != 0;
  const int qlane = perm4 ? 4 * (lane & 15) + (lane >> 4) : lane;
  int n_full = nq;
  if constexpr (!EX && MODE == 2 && HALF == 45) {
    /* A tile holds about 82 frames: one full round of 64 and a remainder that would keep
     * 18 lanes busy for a second full round.  The fast kernels cut each remaining frame's
     * 90-tap window into three 16-pair parts and give them to three lanes
     * 21 lanes apart, so that the parts of one frame, 128 bytes from each other, are not
     * read in the same LDS cycle (taps as per-lane LDS reads, partial sums joined by two shuffles): a third of the
     * arithmetic and of the LDS reads of a round.  Only the order of the additions
     * differs, which the +-1 LSB contract allows; the exact kernels do the full round. */
    const int rem = nq - 64;
    if (rem > 0 && rem <= 21) {
      n_full = 64;
      const int part = (lane >= 21) + (lane >= 42), e = lane - 21 * part;
      const int q = 64 + e;
      const bool act = e < rem && lane < 63;                          /* lane 63 idles */
      const int i = emit_at(min(q, nq - 1));                          /* (idle lanes: the last frame again, no branch; nq > 64 here) */
      const FMD_LDS f2 *x0 = opaque_lds(reinterpret_cast<const f2 *>(&w.ms[HV + i]) - 89);
      float om = 0.f, os = 0.f;
#pragma unroll
      for (int h = 0; h < 2; h++) {                                   /* two groups of 8 pairs */
        const int k0 = 16 * part + 8 * h;
        const f4 ta = fm_lin[k0 >> 2], tb = fm_lin[(k0 >> 2) + 1];
        f2 xl[8], xh[8];
#pragma unroll
        for (int j = 0; j < 8; j++) { xl[j] = x0[k0 + j]; xh[j] = x0[89 - k0 - j]; }
        f2 acc = {om, os}, acc1 = {0.f, 0.f};        /* two running sums (even / odd taps): half the dependent latency */
#pragma unroll
        for (int j = 0; j < 8; j++) {
          /* the taps are a 16-byte LDS word: an odd one is the high half of its register pair (pk_fma_hi: that operand first) */
          const f4 t4 = j < 4 ? ta : tb;
          const f2 tp = (j & 2) ? f2{t4.z, t4.w} : f2{t4.x, t4.y};
          if (j & 1) acc1 = pk_fma_hi(xl[j] + xh[j], tp, acc1);
          else acc = mac2<false>(acc, xl[j] + xh[j], tp.x);
        }
        acc += acc1;
        om = acc.x; os = acc.y;
      }
      om += __shfl_down(om, 21) + __shfl_down(om, 42);
      os += __shfl_down(os, 21) + __shfl_down(os, 42);
      if (act && part == 0) {
        w.fr[pend + 2 * q] = om + os;                  /* (fast kernels only: unpadded) */
        w.fr[pend + 2 * q + 1] = om - os;
      }
    }
  }
  if constexpr (!EX && MODE == 1 && HALF == 64) {
    /* The same for the 128-tap mono filter: the frames beyond the first 64 (18 of 82 at 300 k -> 48 k) take three
     * lanes each, 24 + 24 + 16 tap pairs, instead of a second full round on 18 lanes. */
    const int rem = nq - 64;
    if (rem > 0 && rem <= 21) {
      n_full = 64;
      const int part = (lane >= 21) + (lane >= 42), e = lane - 21 * part;
      const int q = 64 + e;
      const bool act = e < rem && lane < 63;
      const int i = emit_at(min(q, nq - 1));
      const FMD_LDS float *x0 = opaque_lds(&w.v[HV + i]) - 127;
      f2 acc2 = {0.f, 0.f};
#pragma unroll
      for (int h = 0; h < 3; h++) {                                   /* three groups of 8 taps (the third of part 2 meets zero taps) */
        const int k0 = 24 * part + 8 * h;
        const f4 ta = fm_lin[k0 >> 2], tb = fm_lin[(k0 >> 2) + 1];
        float xl[8], xh[8];
#pragma unroll
        for (int j = 0; j < 8; j++) { xl[j] = x0[k0 + j]; xh[j] = x0[127 - k0 - j]; }
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          const f2 p = pk_add_swap(f2{xl[j], xl[j + 1]}, f2{xh[j + 1], xh[j]});   /* the high side as it lies in LDS (ascending), added descending */
          const f2 t = j < 4 ? f2{ta[j], ta[j + 1]} : f2{tb[j - 4], tb[j - 3]};
          acc2 = __builtin_elementwise_fma(p, t, acc2);
        }
      }
      float om = acc2.x + acc2.y;
      om += __shfl_down(om, 21) + __shfl_down(om, 42);
      if (act && part == 0) w.fr[pend + q] = om;                      /* (fast kernels only: unpadded) */
    }
  }
  for (int q = qlane; q < n_full; q += 64) {
    const int i = rs ? emit_at(q) : q;
    if constexpr (MODE == 2) {
      float om, os;
      fir_stereo<EX, HALF>(P, tap_mpx, fm_lin, &w.ms[HV + i], om, os);
      w.fr[fidx_t<EX>(pend + 2 * q)] = om + os;          /* :595 */
      w.fr[fidx_t<EX>(pend + 2 * q + 1)] = om - os;      /* :596 */
    } else if constexpr (MODE == 1) {
      w.fr[fidx_t<EX>(pend + q)] = fir_mono<EX, HALF>(P, tap_mpx, fm_lin, &w.v[HV + i]);
    } else {
      w.fr[fidx_t<EX>(pend + q)] = w.v[HV + i];
    }
  }
}

/* The emit index of frame q by the host's magic number where it has one (any sane pair of rates), by a float estimate otherwise: decided
 * ONCE per tile - inside the frame loops the choice was a scalar compare and branch per call, and a wavefront issues one instruction
 * per 5-9 cycles whatever its kind (tools/ubench/issue_cost.hip) */
template <bool EX, int MODE, int HALF, int HV, typename WM>
__device__ __forceinline__ void resample_tile(const fmdk_params &P, const f4 *tap_mpx, const f4 *fm_lin, WM &w,
                                              int lane, uint32_t acc_t, int nq, int pend) {
  const uint32_t slow = (uint32_t)P.slow, fast = (uint32_t)P.fast;
  const uint32_t magic = P.emit_magic, msh = P.emit_shift, c0 = fast - acc_t - 1u;   /* acc_t < fast */
  if (__builtin_expect(magic != 0, 1)) {
    resample_tile_with<EX, MODE, HALF, HV>(P, tap_mpx, fm_lin, w, lane, acc_t, nq, pend,
                                           [&](int q) -> int { return emit_index_magic(c0, q, fast, magic, msh); });
  } else {
    const float inv_slow = P.inv_slow;               /* 1.0f / (float)slow, made by the host */
    resample_tile_with<EX, MODE, HALF, HV>(P, tap_mpx, fm_lin, w, lane, acc_t, nq, pend,
                                           [&](int q) -> int { return emit_index(acc_t, q, slow, fast, inv_slow); });
  }
}

/* ---- FMD_MATH_FAST_MFMA_F: the second stage at the emit instants only ------------------------------------------------------------------
 *
 * The reference evaluates its second-stage low-pass where the resampler emits (src/rtl_fm_player.c:570-598); round 5's matrix-pipe form evaluated it at every
 * sample and keeps one value in rate_out / rate_out2 (6.25 at 300 k -> 48 k).  Here the banded product decimates: with P = 16 rate_out / rate_out2 an
 * integer (100 at 300 k, 80 at 240 k, 64 at 192 k), frame q + 16 emits exactly P samples after frame q, so the tile's frames are NG = ceil(frames / 16)
 * groups that share ONE set of sixteen emit indices m_i (frame i of the tile, i < 16) shifted by P c:
 *   D[i][(c, s)] = sum_k A[i][k] B[k][(c, s)],   A[i][k] = T_l[m_i + K0 - k]  (row i: the tap limb shifted by the frame's emit index),
 *                                                B[k][(c, s)] = limb s of x[P c - K0 + k]  (column: group c, sample limb s; one window per group)
 * over a window of K0 + P samples: the composite L+R filter g (179 taps, K0 = 180: five K slices) over the discriminator's limbs, fm (90 taps, K0 = 92:
 * three) over (L-R) x carrier's.  Sample limbs 0 and 1 of up to eight groups are the sixteen columns of chain X, which runs all three tap limbs
 * (3 MFMAs per slice); limb 2 meets tap limb 0 only and is chain Y (1 per slice): 5 x 4 + 3 x 4 = 32 MFMAs per tile where the full-rate form took
 * 36 + 24, and the frames come out in order, four consecutive ones per lane - no emit bookkeeping, no selection.
 * Operands: the tap rows are aligned 16-byte words of the sixteen byte-phase replicas of the reversed tables (Smem::dg_rep / df_rep; the lane's phase and
 * word follow from m_i, which changes from tile to tile); the sample windows start P c - K0 bytes from the tile's first sample - 4-byte aligned (P c and K0
 * are multiples of four: the host checks), read as dword pairs.
 * Lane (j = 2 c + s, gg) of chain X holds rows 4 gg + r of column (c, s), lane (2 c [+ 1], gg) of chain Y those of (c, 2).  Weight classes as everywhere
 * (tap limb + sample limb; class 3 - tap limb 2 x sample limb 1 - is computed and left out): the even lane adds its odd neighbour's accumulators as
 * INTEGERS (v_add_u32 with a DPP source) - S0 = X0, S1 = X1 + X0', S2 = X2 + X1' + Y - so the three sums per frame are exactly the accumulators the
 * full-rate form ends with, and the same three multiply-adds put them together. */
template <typename WM, typename SM, typename UNI>
__device__ __forceinline__ void resample_tile_dec(const fmdk_params &P, const UNI &U, const SM &sm, const i4 &magic4, WM &w, int lane, uint32_t acc_t) {
  constexpr int VH = WM::kVbh, ROW = VH + TW;
  const int i = lane & 15, gg = lane >> 4;
  const uint32_t fast = (uint32_t)P.fast;
  const int dec_p = U.dec_p();
  const int mi = emit_index_magic(fast - acc_t - 1u, i, fast, U.emit_magic(), U.emit_shift());   /* emit index of the tile's frame i: 0 .. P - 1 */
  const int a = dec_p - 1 - mi;
  const int rho = a & 15, ab = a & ~15;
  const FMD_LDS int8_t *ga = opaque_lds(&sm.dg_rep[0] + rho * (3 * DG_N) + ab + 16 * gg);
  const FMD_LDS int8_t *fa = opaque_lds(&sm.df_rep[0] + rho * (3 * DF_N) + ab + 16 * gg);
  const int c = i >> 1, s = i & 1;
  const int boff = dec_p * c + 16 * gg;
  const FMD_LDS int8_t *vx = opaque_lds(&w.vb[0][0] + s * ROW + (VH - DEC_K0G) + boff);        /* chain X: limb s of the discriminator output */
  const FMD_LDS int8_t *vy = opaque_lds(&w.vb[2][0] + (VH - DEC_K0G) + boff);                  /* chain Y: limb 2 */
  const FMD_LDS int8_t *sx = opaque_lds(&w.vb[WM::kBsRow][0] + s * ROW + (VH - DEC_K0F) + boff);
  const FMD_LDS int8_t *sy = opaque_lds(&w.vb[WM::kBsRow + 2][0] + (VH - DEC_K0F) + boff);
  /* even lanes (sample limb 0) start from the bits of 1.5 x 2^23 (mpx_tile_i8: the sums are read as floats), odd lanes - whose sums are ADDED to an
   * even lane's - from zero */
  const int selv = s ? 0 : magic4[0];
  const i4 sel4 = {selv, selv, selv, selv}, zero4 = {0, 0, 0, 0};
  auto word4 = [](const FMD_LDS int8_t *p) -> i4 {       /* sixteen bytes at a 4-byte-aligned address */
    const FMD_LDS uint32_t *q = reinterpret_cast<const FMD_LDS uint32_t *>(p);
    return i4{(int)q[0], (int)q[1], (int)q[2], (int)q[3]};
  };
  auto chain = [&](auto ns_, auto tn_, const FMD_LDS int8_t *ta, const FMD_LDS int8_t *bx, const FMD_LDS int8_t *by, float c0, float (&out)[4]) {
    constexpr int NS = decltype(ns_)::value, TN = decltype(tn_)::value;
    i4 X[3] = {sel4, sel4, sel4}, Y = zero4;
    static_for<0, NS>([&](auto s_) {
      constexpr int sl = decltype(s_)::value;
      i4 t[3];
#pragma unroll
      for (int l = 0; l < 3; l++) t[l] = *reinterpret_cast<const FMD_LDS i4 *>(ta + l * TN + 64 * sl);
      const i4 dx = word4(bx + 64 * sl), dy = word4(by + 64 * sl);
#pragma unroll
      for (int l = 0; l < 3; l++) X[l] = __builtin_amdgcn_mfma_i32_16x16x64_i8(t[l], dx, X[l], 0, 0, 0);
      Y = __builtin_amdgcn_mfma_i32_16x16x64_i8(t[0], dy, Y, 0, 0, 0);
    });
    const float k0 = c0 * -12632256.0f, c1 = c0 * 0x1p-8f, c2 = c0 * 0x1p-16f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int x0 = X[0][r], x1 = X[1][r], x2 = X[2][r], y2 = Y[r];
      const int s1 = x1 + __builtin_amdgcn_update_dpp(0, x0, 0xF5, 0xf, 0xf, true);          /* quad_perm [1, 1, 3, 3]: the odd neighbour's */
      const int s2 = x2 + __builtin_amdgcn_update_dpp(0, x1, 0xF5, 0xf, 0xf, true) + y2;
      float y = __builtin_fmaf(__builtin_bit_cast(float, x0), c0, k0);
      y = __builtin_fmaf(__builtin_bit_cast(float, s1), c1, y);
      y = __builtin_fmaf(__builtin_bit_cast(float, s2), c2, y);
      out[r] = y;
    }
  };
  float om[4], os[4];
  chain(std::integral_constant<int, 5>{}, std::integral_constant<int, DG_N>{}, ga, vx, vy, U.g_scale(), om);
  chain(std::integral_constant<int, 3>{}, std::integral_constant<int, DF_N>{}, fa, sx, sy, U.ci_scale0(), os);
  if (s == 0) {                                          /* frames 16 c + 4 gg + r: {L, R} = {om + os, om - os} (:595-596), two 16-byte words */
    f4 *dst = reinterpret_cast<f4 *>(&w.fr[0]) + (8 * c + 2 * gg);
    dst[0] = f4{om[0] + os[0], om[0] - os[0], om[1] + os[1], om[1] - os[1]};
    dst[1] = f4{om[2] + os[2], om[2] - os[2], om[3] + os[3], om[3] - os[3]};
  }
}

/* FMD_MATH_FAST_MFMA_F, 128-tap mono / narrow FM: the fm low-pass at the emit instants only (resample_tile_dec says how; src/rtl_fm_player.c:500-532).
 * Window K0 + P = 128 + P samples: four K slices up to P = 128 (300 k -> 48 k: P = 100), three up to 64 (narrow FM's 25 k -> 12.5 k: P = 32).
 * Up to eight groups of sixteen frames per tile (rate_out >= 4 rate_out2): resample_tile_dec's form - chain X = (group, sample limb 0 / 1) x all three tap
 * limbs, chain Y = (group, limb 2) x tap limb 0, the odd lane's sums added to the even lane's - 4 MFMAs per slice, 16 per tile where the full-rate form took 36.
 * Nine to sixteen groups (narrow FM: 256 frames per tile): a column per group and the six limb pairs accumulated by weight class as everywhere else -
 * 6 per slice, 18 per tile; all 64 lanes hold four frames each. */
template <typename WM, typename SM, typename UNI>
__device__ __forceinline__ void resample_mono_dec(const fmdk_params &P, const UNI &U, const SM &sm, WM &w, int lane, uint32_t acc_t) {
  constexpr int VH = WM::kVbh, ROW = VH + TW;
  const int i = lane & 15, gg = lane >> 4;
  const uint32_t fast = (uint32_t)P.fast;
  const int dec_p = U.dec_p();
  const int mi = emit_index_magic(fast - acc_t - 1u, i, fast, U.emit_magic(), U.emit_shift());
  const int a = dec_p - 1 - mi;
  const FMD_LDS int8_t *ta = opaque_lds(&sm.df_rep[0] + (a & 15) * (3 * DM_N) + (a & ~15) + 16 * gg);
  const float c0 = U.ci_scale0();
  const float k0 = c0 * -12632256.0f, c1 = c0 * 0x1p-8f, c2 = c0 * 0x1p-16f;
  i4 m4 = {0x4B400000, 0x4B400000, 0x4B400000, 0x4B400000};
  asm volatile("" : "+v"(m4));
  auto word4 = [](const FMD_LDS int8_t *p) -> i4 {
    const FMD_LDS uint32_t *q = reinterpret_cast<const FMD_LDS uint32_t *>(p);
    return i4{(int)q[0], (int)q[1], (int)q[2], (int)q[3]};
  };
  const bool four = dec_p > 64;                          /* (wave-uniform) the window's fourth K slice */
  f4 *fr4 = reinterpret_cast<f4 *>(&w.fr[0]);
  if (P.dec_wide) {
    const FMD_LDS int8_t *bx = opaque_lds(&w.vb[0][0] + (VH - DEC_K0M) + dec_p * i + 16 * gg);
    i4 acc[3] = {m4, m4, m4};
    auto slice = [&](auto s_) {
      constexpr int sl = decltype(s_)::value;
      i4 t[3], d[3];
#pragma unroll
      for (int l = 0; l < 3; l++) {
        t[l] = *reinterpret_cast<const FMD_LDS i4 *>(ta + l * DM_N + 64 * sl);
        d[l] = word4(bx + l * ROW + 64 * sl);
      }
      constexpr int PA[6] = {0, 0, 1, 0, 1, 2}, PB[6] = {0, 1, 0, 2, 1, 0};
      static_for<0, 6>([&](auto p_) {
        constexpr int pi = decltype(p_)::value, c = PA[pi] + PB[pi];
        acc[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(t[PA[pi]], d[PB[pi]], acc[c], 0, 0, 0);
      });
    };
    static_for<0, 3>(slice);
    if (four) slice(std::integral_constant<int, 3>{});
    const f4 a0 = __builtin_bit_cast(f4, acc[0]), a1 = __builtin_bit_cast(f4, acc[1]), a2 = __builtin_bit_cast(f4, acc[2]);
    f4 y = __builtin_elementwise_fma(a0, f4{c0, c0, c0, c0}, f4{k0, k0, k0, k0});
    y = __builtin_elementwise_fma(a1, f4{c1, c1, c1, c1}, y);
    y = __builtin_elementwise_fma(a2, f4{c2, c2, c2, c2}, y);
    fr4[4 * i + gg] = y;                                   /* frames 16 i + 4 gg + r */
  } else {
    const int c = i >> 1, s = i & 1;
    const int boff = dec_p * c + 16 * gg;
    const FMD_LDS int8_t *bx = opaque_lds(&w.vb[0][0] + s * ROW + (VH - DEC_K0M) + boff);
    const FMD_LDS int8_t *by = opaque_lds(&w.vb[2][0] + (VH - DEC_K0M) + boff);
    const int selv = s ? 0 : m4[0];
    const i4 sel4 = {selv, selv, selv, selv};
    i4 X[3] = {sel4, sel4, sel4}, Y = {0, 0, 0, 0};
    auto slice = [&](auto s_) {
      constexpr int sl = decltype(s_)::value;
      i4 t[3];
#pragma unroll
      for (int l = 0; l < 3; l++) t[l] = *reinterpret_cast<const FMD_LDS i4 *>(ta + l * DM_N + 64 * sl);
      const i4 dx = word4(bx + 64 * sl), dy = word4(by + 64 * sl);
#pragma unroll
      for (int l = 0; l < 3; l++) X[l] = __builtin_amdgcn_mfma_i32_16x16x64_i8(t[l], dx, X[l], 0, 0, 0);
      Y = __builtin_amdgcn_mfma_i32_16x16x64_i8(t[0], dy, Y, 0, 0, 0);
    };
    static_for<0, 3>(slice);
    if (four) slice(std::integral_constant<int, 3>{});
    f4 y;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int x0 = X[0][r], x1 = X[1][r], x2 = X[2][r], y2 = Y[r];
      const int s1 = x1 + __builtin_amdgcn_update_dpp(0, x0, 0xF5, 0xf, 0xf, true);
      const int s2 = x2 + __builtin_amdgcn_update_dpp(0, x1, 0xF5, 0xf, 0xf, true) + y2;
      float v = __builtin_fmaf(__builtin_bit_cast(float, x0), c0, k0);
      v = __builtin_fmaf(__builtin_bit_cast(float, s1), c1, v);
      v = __builtin_fmaf(__builtin_bit_cast(float, s2), c2, v);
      y[r] = v;
    }
    if (s == 0) fr4[4 * c + gg] = y;                       /* frames 16 c + 4 gg + r */
  }
}

