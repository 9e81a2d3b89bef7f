/* kernel.inc - part of the fused IQ -> PCM kernel (included by fmd_kernels.inc inside its anonymous namespace; not a translation unit of its own).
 * The carried state, the fused kernel (tile loop, chunking, hand-over) and its launch. */

/* ---- carried state in HBM ------------------------------------------------- */

struct DevState {   /* == fmd_stream_state */
  float tb[48];
  float pre_r, pre_j, pp, de_l, de_r;
  int32_t acc;
  int32_t reserved[2];
  float br[256], bm[256], bs[256];
};
static_assert(sizeof(DevState) == sizeof(fmd_stream_state), "state layout");

/* ---- the fused kernel ----------------------------------------------------- */

/* MX: matrix-pipe stages - 0 none, 1 stage A (FMD_MATH_FAST_MFMA), 2 every stage that has a matrix form (FMD_MATH_FAST_MFMA_F: 90-tap stereo - stages A, C
 * and D; 128-tap mono - A and D; other shapes run MX = 1).  DBG: the build that serves fmd_debug_taps (intermediate
 * signals, per-stage cycle stamps); launches without taps run the DBG = false build, where every tap pointer is a compile-time null
 * and the ~40 scalar compares and branches per tile that ask for them are gone (a wavefront issues ONE instruction per 5-9 cycles:
 * tools/ubench/issue_cost.hip).  LV: the build that also writes each tile's level partial sums (tile_level_sums, wave_sum_lane63) to lv_arg,
 * [stream][block][tile of the block] float2 {sum of I + Q, sum of I^2 + Q^2}, for the finish kernel (levels.inc); LV = false compiles none of it */
template <bool EX, int MODE, int HALF, int MX, bool DBG, bool LV>
__global__ __launch_bounds__(NT, waves_of(EX, MODE, HALF, MX, DBG))
void fmd_fused_kernel(const fmdk_params P, const uint8_t *__restrict__ iq_all,
                                                      int16_t *__restrict__ pcm_all,
                                                      int32_t *__restrict__ lens_all,
                                                      const DevState *__restrict__ state_in_all,
                                                      DevState *__restrict__ state_out_all, float *dbg_y_arg,
                                                      float *dbg_v_arg, float *dbg_mpx_arg, long long *dbg_prof_arg, float2 *lv_arg) {
  /* (the mono kernels with the matrix-pipe stage A keep ONE tap pointer a run-time null: with all four compile-time nulls hipcc's
   * register allocation of those instantiations reserves a 36-byte private segment it never touches - tests/test_isa_lint.py refuses scratch) */
  constexpr bool KEEP_Y = DBG || (MODE == 1 && MX == 1);
  float *const dbg_y = KEEP_Y ? dbg_y_arg : nullptr, *const dbg_v = DBG ? dbg_v_arg : nullptr, *const dbg_mpx = DBG ? dbg_mpx_arg : nullptr;
  long long *const dbg_prof = DBG ? dbg_prof_arg : nullptr;
  float2 *const lv_part = LV ? lv_arg : nullptr;
  constexpr int HV = hist_of<HALF>();
  constexpr int CH = (MODE == 2) ? 2 : 1;
  /* the discriminator history is linear.  (While stage C re-read seven window words per
   * chunk a word swizzle paid for itself; with the rotating window it reads two, and the 2-way
   * conflict of the 32-byte lane stride costs less than the address arithmetic did.) */
  constexpr bool MF = MX > 0;                               /* stage A on the matrix pipe */
  constexpr bool MFC = MX > 1 && MODE == 2 && HALF == 45;   /* 90-tap stereo: stages C and D too - the pilot and L-R filters at full rate, the composite L+R filter and the
                                                               second stage of L-R at the emit instants; {L+R, L-R} never exist as fp32 arrays */
  constexpr bool MFM = MX > 1 && MODE == 1 && HALF == 64;   /* 128-tap mono: stage D on the matrix pipe, at the emit instants (resample_mono_dec) */
  constexpr bool LIMBV = MFC || MFM;                        /* the discriminator output is kept as int8 limb arrays as well */
  constexpr int VBH = MFC ? HBE : MFM ? HBM : 16;           /* ... with this many history bytes */
  constexpr int BSROW = 3;                                  /* MFC: first limb array of (L-R) x carrier */
  static_assert(!(EX && MF), "the matrix-pipe stages belong to the +-1 LSB contract");
  __shared__ Smem<HV, MODE == 2, MF, MFC, MFM> sm;
  constexpr int NTAP = HV == 96 ? 48 : 128;
  for (int i = threadIdx.x; i < NTAP; i += NT) sm.tap_mpx[i] = f4{P.fm[i], P.fp[i], P.fs[i], 0.f};
  if constexpr (MF) {
    /* stage-A operand table: entries d = 0 .. 3 of each (limb, component) at slots 7 .. 10, zeros around them */
    int *at = reinterpret_cast<int *>(sm.a_tab);
    for (int i = threadIdx.x; i < 3 * 2 * A_SLOTS * 4; i += NT) {
      const int dw = i & 3, slot = (i >> 2) % A_SLOTS, lc = (i >> 2) / A_SLOTS;
      at[i] = (slot >= 7 && slot < 11) ? P.a_tab[(lc * 4 + slot - 7) * 4 + dw] : 0;
    }
    if constexpr (MFC) {
      /* stage-C operand tables: byte p of (filter f, limb l) = limb l of T_f[127 - p], T_f[u] = round(h_f[u] 2^qf) for u < 90, else 0 */
      for (int i = threadIdx.x; i < 9 * CI_N; i += NT) {
        const int pq = i % CI_N, fl = i / CI_N, f = fl / 3, l = fl - 3 * f;
        const int u = 127 - pq;
        int8_t val = 0;
        if (u >= 0 && u < 90) {
          const float *t = f == 0 ? P.fm : f == 1 ? P.fp : P.fs;
          const int E = (int)__builtin_rintf(__builtin_ldexpf(t[u < 45 ? u : 89 - u], P.ci_qf[f]));     /* exact: |E| < 2^23 */
          val = (int8_t)((((uint32_t)E + 0x808080u) ^ 0x808080u) >> (8 * (2 - l)));
        }
        sm.ci_tab[i] = val;
      }
    }
  }
  if constexpr (LIMBV) {
    /* the sixteen byte phases of the reversed limb tables of the composite filter (stereo) and of fm: made by the host once per batch (fmd_resolve.c,
     * fmdk_dec_tables), copied as they are - 33 / 17 KB, one 16-byte word per thread and step, every load independent (built here from the kernarg taps -
     * base tables, a barrier, 2 200 unaligned LDS reads - the prologue cost 4 % of a one-block launch more) */
    const i4 *src = static_cast<const i4 *>(P.dec_tables);
    if constexpr (MFC) {
      static_assert(offsetof(decltype(sm), df_rep) == offsetof(decltype(sm), dg_rep) + sizeof(sm.dg_rep), "the two phase tables are one block");
      i4 *dst = reinterpret_cast<i4 *>(sm.dg_rep);
      for (int wd = threadIdx.x; wd < (int)((sizeof(sm.dg_rep) + sizeof(sm.df_rep)) / 16); wd += NT) dst[wd] = src[wd];
    } else {
      i4 *dst = reinterpret_cast<i4 *>(sm.df_rep);
      for (int wd = threadIdx.x; wd < (int)(sizeof(sm.df_rep) / 16); wd += NT) dst[wd] = src[wd];
    }
  }
  if (threadIdx.x < NTAP / 4) {
    const float *t = P.fm + 4 * threadIdx.x;
    sm.fm_lin[threadIdx.x] = f4{t[0], t[1], t[2], t[3]};
  }
  __syncthreads();                                /* the only workgroup barrier */

  /* the wave index is uniform over the wavefront: say so, and everything derived from it
   * (stream, chunk, pointers, loop bounds) lives in SGPRs with scalar branches */
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int K = P.n_chunks;
  const int unit = blockIdx.x * WPB + wave;
  if (unit >= P.n_streams * K) return;
  const int stream = unit / K, chunk = unit - stream * K;
  WaveMem<HV, MODE == 2, MFC, MFM> &w = sm.w[wave];
  const f4 *tap_mpx = sm.tap_mpx;

  /* optional per-stage cycle accounting (fmd_debug_taps.prof): lane 0 keeps the
   * sums in the worker's LDS slice (registers would be live across every stage) */
  if (dbg_prof && lane == 0) {
    for (int i = 0; i < 11; i++) w.prof[i] = 0;
#ifdef FMD_REDO_PROF
    for (int i = 0; i < 6; i++) w.rprof[i] = 0;
#endif
    w.prof[11] = w.prof[10] = clock64();
  }
#define FMD_STAMP(i)                                   \
  if (dbg_prof && lane == 0) {                         \
    const long long now_ = clock64();                  \
    w.prof[i] += now_ - w.prof[11];                    \
    w.prof[11] = now_;                                 \
  }

  const int M = P.block_len >> 4;                 /* rate_in samples per block */
  const int tpb = (M + TW - 1) / TW;              /* tiles per block */
  const int T = tpb * P.n_blocks;                 /* tiles per stream */
  const int n_total = M * P.n_blocks;             /* rate_in samples (= 16-byte IQ words) per stream */
  const uint32_t slow = (uint32_t)P.slow, fast = (uint32_t)P.fast;
  const uint8_t *iq_stream = iq_all + (size_t)stream * P.n_blocks * P.block_len;
  const uint4 *iq16 = reinterpret_cast<const uint4 *>(iq_stream);
  /* raw buffer over this stream's IQ bytes (stride 0, dword3 = raw 32-bit data format) */
  const __amdgpu_buffer_rsrc_t iq_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(iq_stream), 0, (uint32_t)n_total * 16u, 0x00020000);
  const DevState *st_in = state_in_all + stream;
  const int size = P.size;

  /* this worker's tiles; a chunk > 0 starts warm_tiles tiles early and discards
   * what those produce */
  /* +-1 LSB stereo kernels: chunks of equal COST, not of equal length.  All workers of a launch are resident at once, so the launch ends with its slowest
   * worker.  Every chunk but the first walks warm_tiles replayed tiles before its own; the first instead fetches the carried state from memory and walks the
   * launch's head (about a tile's worth: HEAD10, in tenths of a tile); the chunk that ends the launch writes the state - an exact recomputation of `size`
   * discriminator samples, another tile's worth (EPI10).  With K L = T + h + (K - 1) r + e: the first chunk owns L - h tiles, the middle ones L - r, the last
   * L - r - e.  Measured against equal lengths on one device (profiles/archive/r27b_chunk_cost_ab.txt): -1 % at 1 and 16 blocks per launch, -2 % at 4.  Mono /
   * narrow FM keep equal lengths: every weighting tried there measured even or worse (their hand-over recomputes nothing). */
  constexpr bool BALANCED = !EX && MODE == 2;
  constexpr int HEAD10 = 10, EPI10 = 10;
  auto chunk_start = [&](int c) -> int {
    if (c <= 0) return 0;
    if (c >= K) return T;
    if constexpr (!BALANCED) return (int)((long long)c * T / K);
    const long long r10 = 10LL * P.warm_tiles, ls = 10LL * T + HEAD10 + (long long)(K - 1) * r10 + EPI10;     /* K L, in tenths */
    long long s0 = (((long long)c * ls - (HEAD10 + (long long)(c - 1) * r10) * K) / K + 5) / 10;
    if (s0 < c) s0 = c;
    if (s0 > T - (K - c)) s0 = T - (K - c);
    return (int)s0;
  };
  const int t_lo = chunk_start(chunk), t_hi = chunk_start(chunk + 1);
  const int g_first = chunk > 0 ? t_lo - P.warm_tiles : 0;

  /* carried state (chunk 0) or zero state (replaying chunks) */
  const bool carried = (chunk == 0);
  if constexpr (LIMBV) {
    /* the limb arrays' history: the last `size` discriminator outputs, zero before them (those bytes only meet zero taps) */
    for (int i = lane; i < VBH; i += 64) {
      const int k = i - (VBH - size);
      const uint32_t q = split_i8x3_one((carried && k >= 0) ? st_in->br[k] : 0.f);
#pragma unroll
      for (int l = 0; l < 3; l++) w.vb[l][i] = (int8_t)(q >> (8 * (2 - l)));
      if constexpr (MFC) {                              /* (L-R) x carrier's history likewise (carried as floats, rounded to 2^-20 here) */
        limb_store(w, BSROW, i, (carried && k >= 0) ? st_in->bs[k] : 0.f);
      }
    }
  }
  for (int i = lane; i < size; i += 64) {
    w.v[(HV - size + i)] = carried ? st_in->br[i] : 0.f;
    if constexpr (MODE == 2 && !MFC)
      w.ms[HV - size + i] = carried ? make_float2(st_in->bm[i], st_in->bs[i]) : make_float2(0.f, 0.f);
  }
  if (lane == 0) {
    w.de[0] = carried ? st_in->de_l : 0.f;
    w.de[1] = carried ? st_in->de_r : 0.f;
  }
  float ycr = carried ? st_in->pre_r : 0.f, ycj = carried ? st_in->pre_j : 0.f;   /* last decimated sample */
  float pp = carried ? st_in->pp : 0.f;                                          /* last pilot output */
  uint32_t acc = (uint32_t)st_in->acc;
  {
    const int b0 = g_first / tpb;
    const long long n0 = (long long)b0 * M + (long long)(g_first - b0 * tpb) * TW;
    if (P.resample) acc = (uint32_t)(((unsigned long long)acc + (unsigned long long)n0 * slow) % fast);
  }

  if (chunk == 0) {
    if (P.offset_tuning) decimate_head<false>(P, iq_stream, st_in->tb, lane, w.head);
    else decimate_head<true>(P, iq_stream, st_in->tb, lane, w.head);
  }
  wave_lds_sync();                                /* carried histories, de[], head[] are in place */
  FMD_STAMP(9)

  int pend = 0, pcm_off = 0, tm_last = 0, n_last = 0;
  bool q1 = false;
  /* IQ words of the next tile: requested one tile ahead (after the MPX stage, when the
   * registers are free again) so the HBM / page-walk latency runs under stages D and F */
  /* fast kernels: whole tiles only and the rotating path -> stage A from the lane's own eight words (decimate8_own) */
  const bool own_words = !EX && !MF && (M % TW == 0) && !P.offset_tuning;
  constexpr int QW = MF ? 12 : 11;                  /* 16-byte IQ words per lane and tile */
  auto fetch_tile = [&](auto &dst, int n_tile_f, int lane_f) {
    if constexpr (MF) load_tile_mfma(dst, iq_rsrc, n_tile_f, lane_f);
    else if (own_words) load_tile_own(dst, iq_rsrc, n_tile_f, 8 * lane_f);
    else load_tile(dst, iq_rsrc, n_tile_f, 8 * lane_f);
  };
  f2 carry_a[3] = {};
  /* (the generic-size stereo kernel with twelve words in flight does not fit three workers per SIMD: it loads at the top of stage A) */
  constexpr bool PREFETCH = MODE != 2 || !(MF && HALF == 0);
  /* requested right after stage A has consumed the registers instead of after B / C: mono / NFM (1 % faster than after the discriminator once the words
   * were no longer a loop-carried value; round 2 had measured no difference), and - round 5 - the stereo kernel with stages A, C, D on the matrix pipe, whose
   * 256-register budget holds the twelve words through stages B and C (-0.9 %, profiles/archive/r16_prefetch_early_ab.txt; the 168-register stereo kernels
   * would spill) */
  constexpr bool PREFETCH_EARLY = MODE != 2 || MFC;
  uint4 qn[QW];
  if constexpr (!(FMD_ABLATE & 1) && PREFETCH) {
    if (g_first < t_hi) {
      const int b = g_first / tpb, off = (g_first - b * tpb) * TW;
      fetch_tile(qn, b * M + off, lane);
    }
  }
  i4 magic4 = {0x4B400000, 0x4B400000, 0x4B400000, 0x4B400000};   /* bits of 12582912.0f: where the int32 accumulators of the matrix-pipe stages start (mpx_tile_i8) */
  if constexpr (MFC) asm volatile("" : "+v"(magic4));   /* one register quad for the whole kernel, not four moves per accumulator; the other
                                                           kernels (three workers per SIMD, no register to spare) make it anew in stage A */
  i4 ctap[3][2][3] = {};                             /* matrix-pipe stage C at two workers per SIMD: the lane's tap operands, for the whole kernel */
  if constexpr (MFC) mpx_i8_taps(sm.ci_tab, lane, ctap);
  /* the uniform bank (k_common.inc, Uniforms): the launch constants stage D, the flush and the roll read, one per lane of ONE register, for the whole
   * kernel - the FMD_MATH_FAST_MFMA_F kernels (90-tap stereo at 256 registers, 128-tap mono at 168: one register fits both) */
  constexpr bool BANKED = LIMBV;
  int bank = 0;
  if constexpr (BANKED) {
    const auto put = [&](int k, uint32_t x) { bank = lane == k ? (int)x : bank; };
    const auto putf = [&](int k, float x) { put(k, __builtin_bit_cast(uint32_t, x)); };
    put(UB_EMIT_MAGIC, P.emit_magic); put(UB_EMIT_SHIFT, P.emit_shift); put(UB_DEC_P, (uint32_t)P.dec_p);
    putf(UB_G_SCALE, P.g_scale); putf(UB_CI_SCALE0, P.ci_scale[0]); putf(UB_COEF, P.coef);
    put(UB_PCM_STRIDE, (uint32_t)P.pcm_stride);
    put(UB_PCM_LO, (uint32_t)(uintptr_t)pcm_all); put(UB_PCM_HI, (uint32_t)((uintptr_t)pcm_all >> 32));
    put(UB_LENS_LO, (uint32_t)(uintptr_t)lens_all); put(UB_LENS_HI, (uint32_t)((uintptr_t)lens_all >> 32));
#pragma unroll
    for (int j = 0; j < 8; j++) putf(UB_LAM_POW + j, P.lam_pow[j]);
#pragma unroll
    for (int j = 0; j < 5; j++) putf(UB_LAM_SCAN + j, P.lam_scan[j]);
  }
  /* ... and the roll's lane map, one register too: bits 0 .. 15 = byte offset, inside the limb arrays, of the 16-byte word the lane moves tm bytes down
   * each tile; bits 16 .. = byte offset in v[] of its second history float (the first is the lane's own).  Stereo: three arrays x twelve words (192
   * history bytes of the discriminator limbs) + three x seven (the last 112 of (L-R) x carrier) = 57 words; mono: three arrays x eight = 24.  The lanes
   * beyond them, and beyond HV - 64 for the floats, move a word another lane moves too (the same bytes to the same place, reads before writes) instead
   * of idling: the loop needs no predicate.  Made per tile from the lane id this was two v_mul_hi, two v_mul_lo, a v_mad_u64_u32 and eight exec-mask
   * branches. */
  uint32_t roll_map = 0;
  if constexpr (LIMBV) {
    int ra, rw;
    if constexpr (MFC) {
      const int l = lane < 57 ? lane : lane - 57;
      ra = l < 36 ? l / 12 : 3 + (l - 36) / 7;
      rw = l < 36 ? l - 12 * ra : 5 + (l - 36) - 7 * (ra - 3);
    } else {
      const int l = lane % 24;
      ra = l >> 3;
      rw = l & 7;
    }
    const int second = lane + 64 < HV ? lane + 64 : lane;
    roll_map = (uint32_t)(ra * (VBH + TW) + 16 * rw) | (uint32_t)(4 * second) << 16;
    asm volatile("" : "+v"(roll_map));               /* (kept, not re-derived in the loop) */
  }
  /* fast kernels, quiet input (exact_tile_decimate): `quiet` = the tile before ran stages A and B in the reference's arithmetic and this
   * one is expected to as well - it then skips the fast forms altogether; `skipped_a` = the tile before did */
  bool quiet = false, skipped_a = false;
  int b_run = g_first / tpb, off_run = (g_first - (g_first / tpb) * tpb) * TW;   /* block / offset of tile g */
  for (int g = g_first; g < t_hi; g++) {
    /* the lane id, re-made opaque every tile: per-lane addresses and offsets are then
     * recomputed where they are used (a few integer ops) instead of being hoisted out of
     * the loop, kept in registers across all stages and spilled to scratch -- a scratch
     * reload waits on vmcnt and would drain the IQ words in flight for the next tile */
    int lane_t = lane;
    asm volatile("" : "+v"(lane_t));
    /* the bank likewise: a v_readlane_b32 where a constant is used, not an SGPR held (and spilled) across the loop - nor a kernarg load again */
    Uniforms<BANKED> U{P, bank};
    if constexpr (BANKED) asm volatile("" : "+v"(U.bank));
    const int b = b_run, off = off_run;
    off_run += TW;
    if (off_run >= M) { off_run = 0; b_run++; }   /* b_run / off_run: the next tile's from here on */
    const int tm = min(TW, M - off);
    const int n_tile = b * M + off;               /* stream sample index of the tile's first sample */
    const bool discard = g < t_lo;
    const size_t slot = (size_t)stream * P.n_blocks + b;
    /* (the banked kernels put the block's PCM pointer together from the bank, at the flush) */
    int16_t *pcm_blk = pcm_all + slot * P.pcm_stride;
    float *mpx_blk = (dbg_mpx && !discard) ? dbg_mpx + slot * M : nullptr;
    const int m0 = 8 * lane_t;

    if (off == 0) {
      pend = 0; pcm_off = 0;
      q1 = (MODE == 2) && P.resample && (acc + slow >= fast);
    } else if (g == t_lo && chunk > 0) {
      /* first real tile in the middle of a block: settle the de-emphasis state on
       * what the replay produced, then continue the block's PCM where a
       * sequential run would be: CH x (emits before `off` in this block) */
      if constexpr (EX) flush_frames<EX, CH, HV>(P, w, lane_t, pend, pcm_blk, nullptr, false);
      pend = 0;
      unsigned long long a0 = (unsigned long long)st_in->acc;
      if (P.resample) {
        /* (a divisor the compiler cannot see through: the reciprocal helpers of these two 64-bit divisions - once per chunk - are otherwise
         * hoisted out of the tile loop and held in registers for the kernel's whole life) */
        uint32_t fast_o = fast;
        asm volatile("" : "+s"(fast_o));
        a0 = (a0 + (unsigned long long)b * M * slow) % fast_o;
        pcm_off = CH * (int)((a0 + (unsigned long long)off * slow) / fast_o);
      } else {
        pcm_off = CH * off;
      }
    }

    /* Wave priority (s_setprio) rises through the tile: stage A runs at 0, B at 1, the MPX stage at 2, resampler / flush / roll at 3.  The later a worker
     * is in its tile the sooner its instructions issue, so the three workers of a SIMD drift into different stages and the LDS-latency-bound tail of one
     * runs under the arithmetic of the others: equal priorities cost 5.5 % (0.616 vs 0.584 ms), any strictly rising assignment is within 1 % of this one
     * (A/B 0, C 1, D 2 was round 1's; 0 / 1 / 2 / 3 measured 0.3-1.1 % better for stereo, 1.6 % for mono). */
    __builtin_amdgcn_s_setprio(0);
    /* ---- A: /8 low-pass, 8 outputs per lane, straight from registers ---- */
    f2 y2[8];                                      /* decimated (I, Q) pairs of the lane's eight outputs */
    constexpr bool PREDICT = !EX;                  /* (every +-1 LSB kernel: the 168-register ones have had room for the second way through the tile since the
                                                      chunk-start divisions stopped holding their reciprocal helpers in registers for the kernel's whole life) */
    const bool skip_a = PREDICT && quiet;          /* (wave-uniform) */
    if (skip_a) {
#pragma unroll
      for (int r = 0; r < 8; r++) y2[r] = f2{0.f, 0.f};
    } else
    if constexpr (FMD_ABLATE & 1) {
#pragma unroll
      for (int r = 0; r < 8; r++) y2[r] = f2{(float)(lane_t + g + r) * 1e-3f, (float)(lane_t - g) * 1e-3f};
    } else {
      uint4 q[QW];
      if constexpr (PREFETCH) {
#pragma unroll
        for (int i = 0; i < QW; i++) q[i] = qn[i];
      } else {
        fetch_tile(q, n_tile, lane_t);              /* the other workers of the SIMD cover the latency */
      }
      if constexpr (MF) {
        constexpr bool MAGIC_A = true;               /* (false: the sums are converted, decimate_mfma<false>) */
        if constexpr (MFC) decimate_mfma<true>(P, q, y2, sm.a_tab, lane_t, magic4);
        else if constexpr (MAGIC_A) {
          i4 m4 = {0x4B400000, 0x4B400000, 0x4B400000, 0x4B400000};
          asm volatile("" : "+v"(m4));                 /* four moves per tile, shared by the twelve accumulators */
          decimate_mfma<true>(P, q, y2, sm.a_tab, lane_t, m4);
        } else {
          decimate_mfma<false>(P, q, y2, sm.a_tab, lane_t, i4{0, 0, 0, 0});
        }
      } else if (own_words) {
        if constexpr (!EX) {
          decimate8_own(P, q, y2, carry_a, lane_t);
          /* the tile before skipped this stage: what it would have left for this tile's first three outputs (carry_a) is missing */
          if (__builtin_expect(skipped_a, 0) && lane_t == 0) {
#pragma unroll 1
            for (int m = 0; m < 3; m++) {
              const float2 t = exact_output(P, iq16, n_tile + m, n_total, true);
              if (m == 0) y2[0] = f2{t.x, t.y}; else if (m == 1) y2[1] = f2{t.x, t.y}; else y2[2] = f2{t.x, t.y};
            }
          }
        }
      } else if (P.offset_tuning) {
        /* make the words opaque on this side: otherwise the byte conversions, common
         * to both sides, are hoisted above the branch and all 176 results are live at once */
#pragma unroll
        for (int i = 0; i < 11; i++) asm volatile("" : "+v"(q[i].x), "+v"(q[i].y), "+v"(q[i].z), "+v"(q[i].w));
        decimate8<EX, false>(P, q, y2);
      } else {
        decimate8<EX, true>(P, q, y2);
      }
    }
    if (n_tile == 0 && chunk == 0 && lane_t == 0) {
#pragma unroll
      for (int m = 0; m < 3; m++) y2[m] = f2{w.head[2 * m], w.head[2 * m + 1]};
    }
    /* LV: the lane's level sums over its final outputs (redone below when the tile takes the exact path), stored after stage B */
    float lv1 = 0.f, lv2 = 0.f;
    if constexpr (LV) tile_level_sums(y2, m0, tm, lv1, lv2);
    if constexpr (!(FMD_ABLATE & 1) && PREFETCH && PREFETCH_EARLY) {
      fetch_tile(qn, b_run * M + off_run, lane_t);   /* mono: the registers are free from here on (unconditional: see below) */
    }
    skipped_a = skip_a;
    FMD_STAMP(1)
    if (dbg_y && !discard && !skip_a) {
      float2 *o = reinterpret_cast<float2 *>(dbg_y) + slot * M + off + m0;
#pragma unroll
      for (int r = 0; r < 8; r++)
        if (m0 + r < tm) o[r] = make_float2(y2[r].x, y2[r].y);
    }

    __builtin_amdgcn_s_setprio(1);
    /* ---- B: discriminator; the sample before the lane's first comes by shuffle ---- */
    if constexpr (FMD_ABLATE & 2) {
      f4 *dst = reinterpret_cast<f4 *>(w.v);
      dst[((HV + m0) >> 2)] = f4{y2[0].x, y2[1].y, y2[2].x, y2[3].y};
      dst[(((HV + m0) >> 2) + 1)] = f4{y2[4].x, y2[5].y, y2[6].x, y2[7].y};
      if constexpr (LIMBV && (FMD_ABLATE & 32)) {          /* (32: what follows a compiled-out stage still sees LIVE operands - the decimated samples' bits stand in for the limbs) */
#pragma unroll
        for (int l = 0; l < 3; l++)
          *reinterpret_cast<uint2 *>(&w.vb[l][VBH + m0]) = uint2{__builtin_bit_cast(uint32_t, y2[l].x) * 2654435761u, __builtin_bit_cast(uint32_t, y2[l + 3].y) * 2246822519u};
        wave_lds_sync();
      }
    } else {
      float pr = __shfl_up(y2[7].x, 1), pj = __shfl_up(y2[7].y, 1);
      if (lane_t == 0) { pr = ycr; pj = ycj; }
      const float pr0 = pr, pj0 = pj;         /* the sample before this lane's first */
      f8 v;
      uint32_t fragile = 0;
      float vmax = 0.f, dmin = 1.f;
      if constexpr (EX) {
#pragma unroll
        for (int r = 0; r < 8; r++) {
          v[r] = discriminate<EX>(pr, pj, y2[r].x, y2[r].y);
          pr = y2[r].x; pj = y2[r].y;
        }
      } else {
        /* The discriminator has one discontinuity: the +-pi branch cut (cross product ~ 0 with a negative
         * dot product), where the sign of a rounding error decides between +pi and -pi; and the phase of
         * a sample next to the origin is ill-conditioned (an absolute rounding difference of 1e-7 in a
         * decimator output of magnitude 1e-4 moves the angle by 1e-3, 3 LSB of NFM PCM).  The fast
         * decimator's outputs differ from the reference's in the last bits, so such samples are redone
         * below in the reference's exact arithmetic (1 in 10^4 .. 10^5 on noise, none on FM). */
        if (!skip_a) discriminate8_fast(pr, pj, y2, v, vmax, dmin);
        if constexpr (FMD_ABLATE != 0) { vmax = 0.f; dmin = 1.f; }   /* timing builds run on garbage: keep the cold paths out */
      }
      if constexpr (!EX) {
        const bool head_tile = (n_tile == 0 && chunk == 0);
        /* dmin: max(|cross|, |dot|) >= |z| |z_prev| / sqrt 2 and decimated samples stay below 1.5 in magnitude:
         * a sample of magnitude <= 1e-3 gives dmin <= 1.5e-3 (the converse is checked sample by sample) */
        const bool near_cut = vmax >= K_PI - 8.4e-5f;
        /* (P.org_thr: 1e-3, or more where the PCM step is small against the filter's largest tap - fmd_resolve.c; org_thr15 = 1.5 x that) */
        if (__builtin_expect(!skip_a && (near_cut || dmin <= P.org_thr15), 0)) {   /* rare on FM: find which of this lane's samples it was */
          /* On noise dmin (a product of two magnitudes) passes this test in nearly every tile while a sample of magnitude <= 1e-3 shows up
           * in one tile of forty: the smallest of the nine magnitudes the scan below would compare (13 instructions) decides whether it runs
           * (80) - the same samples are flagged either way */
          float mmin = __builtin_fabsf(pr0) + __builtin_fabsf(pj0);
#pragma unroll
          for (int r = 0; r < 8; r++) mmin = __builtin_fminf(mmin, __builtin_fabsf(y2[r].x) + __builtin_fabsf(y2[r].y));
          if (near_cut || mmin <= P.org_thr) {
          float qr = pr0, qj = pj0;
          float mp = __builtin_fabsf(qr) + __builtin_fabsf(qj);
#pragma unroll
          for (int r = 0; r < 8; r++) {
            const float yi_r = y2[r].x, yq_r = y2[r].y;
            const float cr = __builtin_fmaf(qr, yq_r, -(qj * yi_r)), dt = __builtin_fmaf(yi_r, qr, yq_r * qj);
            const float mag = __builtin_fabsf(yi_r) + __builtin_fabsf(yq_r);
            if (__builtin_fmaxf(__builtin_fmaf(-4e-5f * mp, mag, __builtin_fabsf(cr)), dt) <= 0.f ||
                __builtin_fminf(mag, mp) <= P.org_thr)
              fragile |= 1u << r;
            mp = mag; qr = yi_r; qj = yq_r;
          }
          }
        }
        /* Quiet input: a lane (of the tile's own samples) with three or more such samples makes it a tile for the reference's arithmetic -
         * redoing them one by one costs two dependent rounds of IQ re-reads each.  A tile that follows such a tile goes there directly. */
        if (__builtin_expect(skip_a || __builtin_amdgcn_ballot_w64(m0 < tm && __builtin_popcount(fragile) >= 3) != 0, 0)) {
          /* two idle 2 KB areas of the worker's slice: the tile part of v[] (written at the end of this stage) and the frame buffer (empty
           * between the flush and the next resampler pass) */
          static_assert(sizeof(w.fr) >= 2048 && (HV * sizeof(float)) % 16 == 0, "parking space of the exact tile path");
          f2 *park_a = reinterpret_cast<f2 *>(&w.v[HV]), *park_b = reinterpret_cast<f2 *>(&w.fr[0]);
          constexpr bool ROOMY = true;                          /* (two outputs per step everywhere: the single-output form measured 1.5 x slower) */
          if (P.offset_tuning) exact_tile_decimate<false, ROOMY>(P, iq_rsrc, n_tile, lane_t, park_a, park_b, y2);
          else exact_tile_decimate<true, ROOMY>(P, iq_rsrc, n_tile, lane_t, park_a, park_b, y2);
          if (head_tile && lane_t == 0) {
#pragma unroll
            for (int m = 0; m < 3; m++) y2[m] = f2{w.head[2 * m], w.head[2 * m + 1]};
          }
          if constexpr (LV) tile_level_sums(y2, m0, tm, lv1, lv2);
          float qr = __shfl_up(y2[7].x, 1), qj = __shfl_up(y2[7].y, 1);
          if (lane_t == 0) {                               /* the sample before the tile: carried (launch start) or from its IQ words */
            if (head_tile) { qr = ycr; qj = ycj; }
            else { const float2 t = exact_output(P, iq16, n_tile - 1, n_total, !P.offset_tuning); qr = t.x; qj = t.y; }
          }
          int small = 0;
#pragma unroll
          for (int r = 0; r < 8; r++) {
            v[r] = discriminate<true>(qr, qj, y2[r].x, y2[r].y);
            qr = y2[r].x; qj = y2[r].y;
            small += (__builtin_fabsf(qr) + __builtin_fabsf(qj) <= P.org_thr) ? 1 : 0;
          }
          fragile = 0;
          quiet = __builtin_amdgcn_ballot_w64(m0 < tm && small >= 3) != 0;      /* the next tile: the same way, or back to the fast forms */
          if (dbg_y && !discard) {
            float2 *o = reinterpret_cast<float2 *>(dbg_y) + slot * M + off + m0;
#pragma unroll
            for (int r = 0; r < 8; r++)
              if (m0 + r < tm) o[r] = make_float2(y2[r].x, y2[r].y);
          }
          /* what the hot path keeps in registers across the tile loop is made anew here rather than kept alive through this path */
          if constexpr (MFC) mpx_i8_taps(sm.ci_tab, lane_t, ctap);
          if constexpr (!(FMD_ABLATE & 1) && PREFETCH && PREFETCH_EARLY) fetch_tile(qn, b_run * M + off_run, lane_t);
        }
        while (fragile) {
          const int r = __builtin_ctz(fragile);
          fragile &= fragile - 1;
          const int m = m0 + r;
          float2 c = make_float2(0.f, 0.f), q = c;
#pragma unroll 1
          for (int e = 0; e < 2; e++) {        /* rolled: one copy of the cold code */
            const float2 t = exact_output(P, iq16, n_tile + m - e, n_total, !P.offset_tuning);
            if (e == 0) c = t; else q = t;
          }
          if (head_tile) {                     /* outputs 0..2 / the sample before the launch */
            if (m < 3) c = make_float2(w.head[2 * m], w.head[2 * m + 1]);
            if (m >= 1 && m < 4) q = make_float2(w.head[2 * (m - 1)], w.head[2 * (m - 1) + 1]);
            if (m == 0) q = make_float2(ycr, ycj);
          }
          const float vx = discriminate<true>(q.x, q.y, c.x, c.y);
#pragma unroll
          for (int rr = 0; rr < 8; rr++) v[rr] = (rr == r) ? vx : v[rr];
        }
      }
      tile_last2(y2, tm, ycr, ycj);
      f4 *dst = reinterpret_cast<f4 *>(w.v);
      dst[((HV + m0) >> 2)] = f4{v[0], v[1], v[2], v[3]};
      dst[(((HV + m0) >> 2) + 1)] = f4{v[4], v[5], v[6], v[7]};
      if constexpr (LIMBV) {                             /* the same eight as three int8 limbs each, for the matrix-pipe stages C / D */
        uint2 lb[3];
        split_i8x3(v, lb);
#pragma unroll
        for (int l = 0; l < 3; l++) *reinterpret_cast<uint2 *>(&w.vb[l][VBH + m0]) = lb[l];
      }
      wave_lds_sync();
      if (dbg_v && !discard) {
        float *o = dbg_v + slot * M + off + m0;
#pragma unroll
        for (int r = 0; r < 8; r++)
          if (m0 + r < tm) o[r] = v[r];
      }
    }
    if constexpr (LV) {
      /* the tile's partial sums (replayed tiles store nothing: their first outputs are not the sequential run's) */
      const float t1 = wave_sum_lane63(lv1), t2 = wave_sum_lane63(lv2);
      if (lane_t == 63 && !discard) lv_part[slot * tpb + off / TW] = make_float2(t1, t2);
    }
    FMD_STAMP(2)

    /* ---- Q + C: stereo MPX filters ---- */
    if constexpr (MODE == 2) {
      if (q1 && off == 0 && tm > 1) {
        if constexpr (MFC) q1_patch_i8<HV>(P, tap_mpx, w, lane_t, pp, (n_tile == 0 && chunk == 0) ? st_in->bm : nullptr);
        else q1_patch<EX, HV>(P, tap_mpx, w, lane_t, pp);
        wave_lds_sync();
        if constexpr (MFC) {                             /* the overwritten sample 1 in the limb arrays too */
          if (lane_t < 3) (&w.vb[0][0])[lane_t * (VBH + TW) + VBH + 1] = (int8_t)(split_i8x3_one(w.v[HV + 1]) >> (8 * (2 - lane_t)));
          wave_lds_sync();
        }
      }
      FMD_STAMP(3)
      __builtin_amdgcn_s_setprio(2);
      if constexpr (MFC && (FMD_ABLATE & 4) && (FMD_ABLATE & 32)) {   /* stage C compiled out, stage D kept on live operands: the discriminator's limbs stand in for (L-R) x carrier's */
#pragma unroll
        for (int l = 0; l < 3; l++) {
          const uint2 x = *reinterpret_cast<const uint2 *>(&w.vb[l][VBH + m0]);
          *reinterpret_cast<uint2 *>(&w.vb[BSROW + l][VBH + m0]) = uint2{x.y ^ 0x5a5a5a5au, x.x};
        }
        wave_lds_sync();
      }
      if constexpr (!(FMD_ABLATE & 4)) {
        uint32_t frag;
        if constexpr (MFC) frag = mpx_tile_i8<HV>(P, ctap, magic4, w, lane_t, pp);
        else frag = mpx_tile<EX, HALF, HV>(P, tap_mpx, w, lane_t, tm, pp);
        if constexpr (FMD_ABLATE != 0) frag = 0;
        if constexpr (!EX) {
          unsigned long long any = __builtin_amdgcn_ballot_w64(frag != 0);
          while (__builtin_expect(any != 0, 0)) {              /* cold: one ill-conditioned sample at a time */
            const int src = __builtin_ctzll(any);
            any &= any - 1;
            uint32_t bits = (uint32_t)__builtin_amdgcn_readlane((int)frag, src);
            while (bits) {
              const int r = __builtin_ctz(bits);
              bits &= bits - 1;
              const int m = MFC ? 256 * (r >> 2) + 16 * (src & 15) + 4 * (src >> 4) + (r & 3) : (HALF == 45) ? 8 * src + r : src + 64 * r;
              redo_carrier<HV>(P, tap_mpx, w, lane_t, m, n_tile, iq16, n_total, M, (uint32_t)st_in->acc);
            }
          }
        }
      }
      FMD_STAMP(4)
    }

    __builtin_amdgcn_s_setprio(3);                   /* mono / NFM: straight from the discriminator to here */
    if constexpr (!(FMD_ABLATE & 1) && PREFETCH && !PREFETCH_EARLY) {
      /* next tile's IQ words, consumed at the top of the loop.  Unconditional - after the chunk's last tile the range
       * check of the buffer makes them zeros nobody reads: guarded by `g + 1 < t_hi` the words were a loop-carried value
       * that stayed live through stages A .. C of every tile (48 registers nothing else could use: the 90-tap stereo
       * kernel needed 168 VGPRs with the guard and needs 146 without) */
      fetch_tile(qn, b_run * M + off_run, lane_t);
    }

    /* ---- D: resampler outputs of this tile ---- */
    int nq = tm;
    uint32_t acc_next = acc;
    if constexpr (MFC || MFM) {
      /* (the host gives these kernels their magic numbers or another family: without tile_frames' division fall-backs, whose loop-invariant
       * reciprocals hipcc keeps in registers for the kernel's whole life) */
      const uint32_t x = acc + (uint32_t)tm * slow;
      const uint32_t e = (uint32_t)(((unsigned long long)x * P.tf_magic) >> 32) >> P.tf_shift;
      nq = (int)e;
      acc_next = x - e * fast;
    } else
    if (P.resample) tile_frames(acc, tm, slow, fast, P.tf_magic, P.tf_shift, P.inv_fast, nq, acc_next);
    if constexpr (EX) {
      if (pend + nq * CH > CAPW) {
        flush_frames<EX, CH, HV>(P, w, lane_t, pend, pcm_blk + pcm_off, mpx_blk ? mpx_blk + pcm_off : nullptr,
                                 !discard);
        pcm_off += pend;
        pend = 0;
        FMD_STAMP(8)
      }
    }
    if constexpr (!(FMD_ABLATE & 8)) {
      if constexpr (MFC) {
        resample_tile_dec(P, U, sm, magic4, w, lane_t, acc);
        if (__builtin_expect(n_tile == 0 && chunk == 0, 0)) {      /* the launch's first samples meet the carried bm ring */
          wave_lds_sync();
          lr_head_fix<HV>(P, tap_mpx, st_in->bm, w, lane_t, acc, nq);
        }
      } else if constexpr (MFM) resample_mono_dec(P, U, sm, w, lane_t, acc);
      else resample_tile<EX, MODE, HALF, HV>(P, tap_mpx, sm.fm_lin, w, lane_t, acc, nq, pend);
    }
    wave_lds_sync();
    FMD_STAMP(6)
    if constexpr (EX) {
      pend += nq * CH;
    } else {
      /* fast kernels: this tile's frames go out now (pend stays 0) */
      float *dbg_t = mpx_blk ? mpx_blk + pcm_off : nullptr;
      const auto flush = [&](auto *pcm_t) {
        bool done2 = false;
        if constexpr (CH == 1) {                        /* mono at <= 128 frames per tile: two frames per lane */
          if (P.flush_g == 2) { flush_tile_fast<CH, 2>(P, U, w, lane_t, nq, pcm_t, dbg_t, !discard); done2 = true; }
        }
        if constexpr (CH == 2) {                        /* stereo at <= 96 frames per tile: three frames per lane, 28 + 28 lanes busy instead of 21 + 21 */
          if (P.flush_g == 3) { flush_tile_fast<CH, 3>(P, U, w, lane_t, nq, pcm_t, dbg_t, !discard); done2 = true; }
        }
        if (done2) {}
        else if (P.flush_g == 4) flush_tile_fast<CH, 4>(P, U, w, lane_t, nq, pcm_t, dbg_t, !discard);
        else flush_tile_fast<CH, 8>(P, U, w, lane_t, nq, pcm_t, dbg_t, !discard);
      };
      if constexpr (BANKED) flush(global_ptr<int16_t>(U.template bank_u<UB_PCM_LO>(), U.template bank_u<UB_PCM_HI>()) + slot * U.pcm_stride() + pcm_off);
      else flush(pcm_blk + pcm_off);
      wave_lds_sync();
      pcm_off += nq * CH;
    }
    acc = acc_next;
    FMD_STAMP(5)                                       /* fast kernels: the per-tile flush (the exact ones flush under stamp 8) */

    __builtin_amdgcn_s_setprio(3);
    /* ---- roll the FIR histories to the front of their buffers ---- */
    if constexpr (LIMBV) {
      /* FMD_MATH_FAST_MFMA_F: every lane's three words by the map made before the loop (roll_map) - one unpack, the reads, the writes.  The limb arrays
       * roll as 16-byte words (whole tiles only: tm is a multiple of 16), v[] as two floats per lane; no lane is idle, so nothing is predicated */
      static_assert(HV > 64 && HV <= 128, "two history floats per lane");
      const FMD_LDS char *vb0 = reinterpret_cast<const FMD_LDS char *>((const FMD_LDS int8_t *)&w.vb[0][0]) + (roll_map & 0xffffu) + tm;
      const FMD_LDS char *v0 = reinterpret_cast<const FMD_LDS char *>((const FMD_LDS float *)&w.v[0]) + 4 * tm;
      const uint32_t o1 = 4u * (uint32_t)lane_t, o2 = roll_map >> 16;
      const i4 rq = *reinterpret_cast<const FMD_LDS i4 *>(vb0);
      const float r1 = *reinterpret_cast<const FMD_LDS float *>(v0 + o1), r2 = *reinterpret_cast<const FMD_LDS float *>(v0 + o2);
      wave_lds_sync();                             /* all reads first, then all writes (one wave: in order) */
      *(FMD_LDS i4 *)(vb0 - tm) = rq;
      *(FMD_LDS float *)(v0 - 4 * tm + o1) = r1;
      *(FMD_LDS float *)(v0 - 4 * tm + o2) = r2;
      wave_lds_sync();
    } else {
      constexpr int NR = (HV + 63) / 64;
      float rv[NR];
      float2 rm[NR];
#pragma unroll
      for (int i = 0; i < NR; i++) {             /* all reads first, then all writes (one wave: in order) */
        const int idx = lane_t + 64 * i;
        rv[i] = idx < HV ? w.v[(tm + idx)] : 0.f;
        if constexpr (MODE == 2) rm[i] = idx < HV ? w.ms[tm + idx] : make_float2(0.f, 0.f);
      }
      wave_lds_sync();
#pragma unroll
      for (int i = 0; i < NR; i++) {
        const int idx = lane_t + 64 * i;
        if (idx < HV) {
          w.v[(idx)] = rv[i];
          if constexpr (MODE == 2) w.ms[idx] = rm[i];
        }
      }
      wave_lds_sync();
    }
    FMD_STAMP(7)

    /* ---- F: end of block -> PCM ---- */
    if (off + tm == M) {
      if constexpr (EX)
        flush_frames<EX, CH, HV>(P, w, lane_t, pend, pcm_blk + pcm_off, mpx_blk ? mpx_blk + pcm_off : nullptr,
                                 !discard);
      if constexpr (BANKED) {
        if (lane_t == 0 && !discard) global_ptr<int32_t>(U.template bank_u<UB_LENS_LO>(), U.template bank_u<UB_LENS_HI>())[slot] = pcm_off + pend;
      } else
      if (lane_t == 0 && !discard) lens_all[slot] = pcm_off + pend;
      pend = 0;
      FMD_STAMP(8)
    }
    tm_last = tm;
    n_last = n_tile;
    /* a chunk that ends in the middle of a block hands its pending frames over now */
    if constexpr (EX) {
      if (g + 1 == t_hi && pend > 0) {
        flush_frames<EX, CH, HV>(P, w, lane_t, pend, pcm_blk + pcm_off, mpx_blk ? mpx_blk + pcm_off : nullptr,
                                 !discard);
        pend = 0;
      }
    }
  }

  /* carried state -> HBM (the chunk that ends the launch) */
  if (chunk == K - 1 && g_first < t_hi) {
    DevState *st = state_out_all + stream;
    /* a launch may end in the middle of nothing: blocks are whole, so pend == 0 here */
    /* lowpass_tb: the last 24 complex samples, rotated, as floats (:366) */
    if (lane < 48) {
      const uint8_t *raw = iq_stream + ((size_t)(n_last + tm_last) * 16 - 48);
      const int j = lane >> 1, comp = lane & 1, p = j & 3;   /* 24 samples: phase = j mod 4 */
      int sel; float sg;
      if (P.offset_tuning) { sel = comp; sg = 1.f; }
      else {
        sel = comp ? sel_q<true>(p) : sel_i<true>(p);
        sg = comp ? sgn_q<true>(p) : sgn_i<true>(p);
      }
      st->tb[lane] = sg * t0((float)raw[2 * j + sel]);
    }
    /* Fast kernels: what the NEXT launch's exact redos reach back to is handed over in the reference's own bits.  The
     * last decimated sample (the discriminator's "previous" for the next launch's sample 0) and - stereo - the last
     * `size` discriminator outputs (the window redo_carrier sums for an ill-conditioned carrier in the next launch's
     * first `size` samples) are recomputed from the IQ words in exact arithmetic, like the redos inside a launch;
     * samples whose reference value is not a function of the IQ bytes alone (the launch's first four, a block's
     * Q1-overwritten sample 1) stay as the tile loop left them, as they do there. */
    const int n_end = n_last + tm_last;                       /* stream sample index one past the launch's last */
    if constexpr (!EX) {
      if (n_end - 1 > 3) {
        const float2 c = exact_output(P, iq16, n_end - 1, n_total, !P.offset_tuning);
        ycr = c.x;
        ycj = c.y;
      }
    }
    [[maybe_unused]] float bm_end[2] = {0.f, 0.f};
    if constexpr (MFC) {
      /* the bm ring the next launch (or the caller's struct) expects: the first-stage L+R low-pass of the last `size` samples (:545, :560), from
       * the discriminator's limb history (the last 192 samples; the tile loop has rolled it to the front).  On the launch's critical path like
       * lr_head_fix: the window as floats first (three per lane), then both of a lane's ring entries in one unrolled loop. */
#pragma unroll
      for (int u = 0; u < 3; u++) w.xs[lane + 64 * u] = limb_value(w, 0, lane + 64 * u);
      wave_lds_sync();
      const float *fmt = reinterpret_cast<const float *>(tap_mpx);
      const int ia = lane, ib = lane + 64 < 90 ? lane + 64 : 89;
#pragma unroll 9
      for (int k = 0; k < 90; k++) {
        const float t = fmt[4 * (k < 45 ? k : 89 - k)];
        bm_end[0] = __builtin_fmaf(t, w.xs[HBE - 90 + ia - k], bm_end[0]);
        bm_end[1] = __builtin_fmaf(t, w.xs[HBE - 90 + ib - k], bm_end[1]);
      }
    }
    for (int i = lane; i < size; i += 64) {
      float val = w.v[(HV - size + i)];
      if constexpr (!EX && MODE == 2) {
        const int j = n_end - size + i;
        bool keep = j <= 3;
        if (!keep && P.resample && M > 1) {
          const int blk = j / M;
          if (j - blk * M == 1) {                             /* did block blk start with an emit? (Q1) */
            const uint32_t a = (uint32_t)(((unsigned long long)(uint32_t)st_in->acc + (unsigned long long)blk * M * slow) % fast);
            keep = a + slow >= fast;
          }
        }
        if (!keep) {
          float2 c = make_float2(0.f, 0.f), q = c;
#pragma unroll 1
          for (int e = 0; e < 2; e++) {                       /* rolled: one copy of the cold code */
            const float2 t = exact_output(P, iq16, j - e, n_total, !P.offset_tuning);
            if (e == 0) c = t; else q = t;
          }
          val = discriminate<true>(q.x, q.y, c.x, c.y);
        }
      }
      st->br[i] = val;
      if constexpr (MFC) {
        st->bm[i] = bm_end[i >> 6];                             /* (made above) */
        st->bs[i] = limb_value(w, BSROW, HBE - size + i);
      } else if constexpr (MODE == 2) {
        const float2 m = w.ms[HV - size + i];
        st->bm[i] = m.x;
        st->bs[i] = m.y;
      }
    }
    if (lane == 0) {
      st->pre_r = ycr;
      st->pre_j = ycj;
      st->pp = (MODE == 2) ? pp : st_in->pp;
      st->de_l = w.de[0];
      st->de_r = w.de[1];
      st->acc = (int32_t)acc;
    }
  }
  FMD_STAMP(9)
  if (dbg_prof && lane == 0) {
    long long *o = dbg_prof + 16 * (size_t)unit;
    for (int i = 0; i < 10; i++) o[i] = w.prof[i];
#ifdef FMD_REDO_PROF
    for (int i = 0; i < 5; i++) o[10 + i] = w.rprof[i];
#endif
    o[15] = w.prof[11] - w.prof[10];
  }
#undef FMD_STAMP
}

using kernel_fn = void (*)(fmdk_params, const uint8_t *, int16_t *, int32_t *, const DevState *, DevState *, float *, float *, float *, long long *,
                           float2 *);

template <bool EX, int MODE, int HALF, int MX>
kernel_fn kernel_of(bool dbg, bool lv) {
  if (lv) return dbg ? fmd_fused_kernel<EX, MODE, HALF, MX, true, true> : fmd_fused_kernel<EX, MODE, HALF, MX, false, true>;
  return dbg ? fmd_fused_kernel<EX, MODE, HALF, MX, true, false> : fmd_fused_kernel<EX, MODE, HALF, MX, false, false>;
}

/* The instantiation of variant v in the translation unit that owns EX and MX (fmd_kernels.inc): MX = 1 is the matrix-pipe unit, which owns the MX = 2
 * kernels too - 90-tap stereo and 128-tap mono, the only shapes the host gives mx = 2 (fmd_resolve.c, variant_of). */
template <bool EX, int MX>
kernel_fn kernel_for(const fmdk_variant *v, bool dbg, bool lv) {
  if constexpr (MX > 0)
    if (v->mx > 1) return v->mode == 2 ? kernel_of<EX, 2, 45, 2>(dbg, lv) : kernel_of<EX, 1, 64, 2>(dbg, lv);
  if (v->mode == 2) return v->half ? kernel_of<EX, 2, 45, MX>(dbg, lv) : kernel_of<EX, 2, 0, MX>(dbg, lv);
  if (v->mode == 1) return v->half ? kernel_of<EX, 1, 64, MX>(dbg, lv) : kernel_of<EX, 1, 0, MX>(dbg, lv);
  return kernel_of<EX, 0, 0, MX>(dbg, lv);
}

template <bool EX, int MX>
int launch_variant(const fmdk_params *p, const fmdk_variant *v, int n_streams, const void *iq, void *pcm, void *lens, const void *state_in,
                   void *state_out, const fmd_debug_taps *dbg, void *lv_part, void *stream, void *ev0, void *ev1) {
  const bool taps = dbg && (dbg->y || dbg->v || dbg->mpx || dbg->prof);
  const kernel_fn kernel = kernel_for<EX, MX>(v, taps, lv_part != nullptr);
  const int units = n_streams * p->n_chunks;
  const dim3 grid((units + WPB - 1) / WPB), block(NT);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1);
  /* hipExtLaunchKernelGGL: the start / stop events ride on the kernel's own dispatch packet - an event pair recorded around the
   * launch is two more packets with barriers, ~5 us per launch more: a tenth of a one-block launch.  (What the events measure is
   * therefore the kernel's own start-to-end time, not a marker-to-marker span on the stream: DESIGN.md section 5.)  Without
   * events - fmd_batch_set_timing(b, 0) - or on a caller's stream that is being captured into a hipGraph, where a dispatch packet
   * with event arguments has no meaning, it is a plain launch. */
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (st && hipStreamIsCapturing(st, &cap) != hipSuccess) { cap = hipStreamCaptureStatusNone; (void)hipGetLastError(); }
  const fmd_debug_taps t = taps ? *dbg : fmd_debug_taps{};
  float *ty = static_cast<float *>(t.y), *tv = static_cast<float *>(t.v), *tm = static_cast<float *>(t.mpx);
  long long *tp = static_cast<long long *>(t.prof);
  float2 *lp = static_cast<float2 *>(lv_part);
  if ((e0 || e1) && cap == hipStreamCaptureStatusNone)
    hipExtLaunchKernelGGL(kernel, grid, block, 0, st, e0, e1, 0, *p, static_cast<const uint8_t *>(iq), static_cast<int16_t *>(pcm),
                          static_cast<int32_t *>(lens), static_cast<const DevState *>(state_in), static_cast<DevState *>(state_out), ty, tv, tm, tp, lp);
  else
    hipLaunchKernelGGL(kernel, grid, block, 0, st, *p, static_cast<const uint8_t *>(iq), static_cast<int16_t *>(pcm),
                       static_cast<int32_t *>(lens), static_cast<const DevState *>(state_in), static_cast<DevState *>(state_out), ty, tv, tm, tp, lp);
  return (int)hipGetLastError();
}
