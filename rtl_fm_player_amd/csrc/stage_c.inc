/* stage_c.inc - part of the fused IQ -> PCM kernel (included by fmd_kernels.inc inside its anonymous namespace; not a translation unit of its own).
 * Stage C: the three 90-tap MPX filters and the 38 kHz carrier (reference :533-568, :472-481) - the vector-ALU form (mpx_tile) and the int8 matrix-pipe form of FMD_MATH_FAST_MFMA_F (mpx_tile_i8: pilot and L-R filters; limb helpers). */

/* (the filter taps as scalars: FMD_KTAP4, k_common.inc) */

/* carrier_fast for two neighbouring samples at once: vp2 = their pilot outputs, vq = the pilot output before the
 * first of them, vs2 = their L-R filter outputs; returns vs * carrier for both (ten packed instructions, two
 * reciprocals and one three-way minimum for the pair). */
__device__ __forceinline__ f2 carrier_fast2(f2 vp2, float vq, f2 vs2, float swf, float cwf, float inv_k2, float &margin) {
  const f2 x = vp2 * swf;
  const f2 pv = {vq, vp2.x};                               /* the pilot output one sample earlier */
  const f2 y = __builtin_elementwise_fma(vp2, f2{cwf, cwf}, -pv);
  const f2 r2 = __builtin_elementwise_fma(x, x, __builtin_elementwise_fma(y, y, f2{1e-37f, 1e-37f}));
  const f2 mg = __builtin_elementwise_fma(r2, f2{inv_k2, inv_k2}, -(vs2 * vs2));
  margin = __builtin_fminf(margin, __builtin_fminf(mg.x, mg.y));
  const f2 rc = {__builtin_amdgcn_rcpf(r2.x), __builtin_amdgcn_rcpf(r2.y)};
  return vs2 * (((x + x) * y) * rc);
}

/* the same for two samples that are not neighbours: vq2 = the pilot outputs before each of them.  One sample per instruction, not packed: a packed
 * instruction costs 2.4 x the energy of a plain one for twice the work, and this kernel is bound by energy - the same arithmetic bit for bit, -0.5 % over
 * six interleaved pairs (profiles/r6w_scalar_vs_packed_ab.txt) */
__device__ __forceinline__ f2 carrier_fast2v(f2 vp2, f2 vq2, f2 vs2, float swf, float cwf, float inv_k2, float &margin) {
  const float c0 = carrier_fast(vp2.x, vq2.x, vs2.x, swf, cwf, inv_k2, margin), c1 = carrier_fast(vp2.y, vq2.y, vs2.y, swf, cwf, inv_k2, margin);
  return f2{vs2.x * c0, vs2.y * c1};
}

/* ---- stage C: MPX filters at rate_in (stereo) --------------------------- */

/* ms[m] = { sum fm[k] p[m,k],  (sum fs[k] p[m,k]) * carrier(vp[m], vp[m-1]) },
 * vp[m] = sum fp[k] p[m,k],  p[m,k] = v[m-89+k] + v[m-k]   (:538-566).
 * HALF == 45: every lane owns 8 consecutive outputs and walks the 45 taps in
 * 12 chunks of 4 (taps 45..47 are zero); a chunk needs 7 aligned 16-byte window
 * reads and 4 tap reads for 8 x 4 x (1 add + 3 FMA).  pp is the pilot output of
 * the sample before the tile (in), of the tile's last sample (out). */
template <bool EX, int HALF, int HV, typename WM>
__device__ __forceinline__ uint32_t mpx_tile(const fmdk_params &P, const f4 *tap_mpx, WM &w, int lane,
                                             int tm, float &pp) {
  uint32_t fragile = 0;          /* fast kernels: this lane's outputs whose carrier is ill-conditioned */
  if constexpr (HALF == 45) {
    constexpr int R = 8;
    const int m0 = R * lane;
    f8 am = 0.f, ap = 0.f, as = 0.f;
    f2 am2[4] = {}, ap2[4] = {}, as2[4] = {};          /* outputs (2j, 2j+1): packed arithmetic */
    if (m0 < tm) {
      const f4 *v4s = reinterpret_cast<const f4 *>(w.v);   /* x[i] = v[m0 - 92 + i] */
      /* chunk c (taps 4c .. 4c+3; 45..47 are zero) needs window words c .. c+3 ("lo",
       * x[r+k+3]) and 22-c .. 24-c ("hi", x[r+92-k]).  Consecutive chunks share all but
       * one word on each side, so the 12 chunks are unrolled with the words rotating
       * through fixed registers (lo word j in slot j%5, hi word j in slot j%4): two
       * 16-byte LDS reads per chunk, issued one chunk ahead, instead of seven.  The taps
       * are three s_load_dwordx4 per chunk.  The fence at the end of a chunk orders
       * everything (accumulators, prefetched words, tap offset) so that neither the
       * reads nor the scalar loads of later chunks are hoisted to the top, which would
       * cost the registers this scheme saves. */
      int wbase = (HV + m0 - 92) >> 2;
      f4 lo[5], hi[4];
#pragma unroll
      for (int j = 0; j < 4; j++) lo[j] = v4s[wbase + j];
#pragma unroll
      for (int j = 22; j < 25; j++) hi[j & 3] = v4s[wbase + j];
      int koff = 0;                                  /* opaque zero, re-made at every fence */
      asm volatile("" : "+s"(koff));
      f4 tm4[2], tp4[2], ts4[2];                     /* taps of this chunk / the next one */
      tm4[0] = FMD_KTAP4(fm, koff); tp4[0] = FMD_KTAP4(fp, koff); ts4[0] = FMD_KTAP4(fs, koff);
      static_for<0, 12>([&](auto c_) {
        constexpr int c = decltype(c_)::value, cb = c & 1;
        if constexpr (c < 11) {
          tm4[cb ^ 1] = FMD_KTAP4(fm, 4 * c + 4 + koff);
          tp4[cb ^ 1] = FMD_KTAP4(fp, 4 * c + 4 + koff);
          ts4[cb ^ 1] = FMD_KTAP4(fs, 4 * c + 4 + koff);
          lo[(c + 4) % 5] = v4s[wbase + c + 4];
          hi[(21 - c) & 3] = v4s[wbase + 21 - c];
          /* the two reads are issued before any of this chunk's arithmetic: the accumulators pass
           * through an asm that the reads cannot sink below (memory clobber), so the LDS latency
           * runs under the 128 VALU instructions instead of in front of the fence */
          asm volatile("" : "+v"(ap2[0]), "+v"(ap2[1]), "+v"(ap2[2]), "+v"(ap2[3]), "+v"(as2[0]), "+v"(as2[1]),
                         "+v"(as2[2]), "+v"(as2[3]) :: "memory");
        }
        static_for<0, 4>([&](auto kk_) {
          constexpr int kk = decltype(kk_)::value;
          if constexpr (4 * c + kk < 45)                 /* taps 45..47 of the last chunk are padding */
          static_for<0, R / 2>([&](auto j_) {
            constexpr int r = 2 * decltype(j_)::value;
            constexpr int il = r + kk + 3, ih = r + 4 - kk;    /* x[r+k+3] + x[r+92-k], relative to words c / 22-c */
            constexpr int il1 = il + 1, ih1 = ih + 1;          /* ... and the same for output r + 1 */
            const f2 lp = {lo[(c + (il >> 2)) % 5][il & 3], lo[(c + (il1 >> 2)) % 5][il1 & 3]};
            const f2 hp = {hi[(22 - c + (ih >> 2)) & 3][ih & 3], hi[(22 - c + (ih1 >> 2)) & 3][ih1 & 3]};
            const f2 p = lp + hp;
            constexpr int j = r >> 1;
            am2[j] = mac2<EX>(am2[j], p, tm4[cb][kk]);
            ap2[j] = mac2<EX>(ap2[j], p, tp4[cb][kk]);
            as2[j] = mac2<EX>(as2[j], p, ts4[cb][kk]);
          });
        });
        if constexpr (c < 11)
          asm volatile("" : "+v"(am2[0]), "+v"(am2[1]), "+v"(am2[2]), "+v"(am2[3]), "+v"(ap2[0]), "+v"(ap2[1]),
                         "+v"(ap2[2]), "+v"(ap2[3]), "+v"(as2[0]), "+v"(as2[1]), "+v"(as2[2]), "+v"(as2[3]),
                         "+v"(lo[(c + 4) % 5]), "+v"(hi[(21 - c) & 3]), "+s"(koff), "+v"(wbase) :: "memory");
      });
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      am[2 * j] = am2[j].x; am[2 * j + 1] = am2[j].y;
      ap[2 * j] = ap2[j].x; ap[2 * j + 1] = ap2[j].y;
      as[2 * j] = as2[j].x; as[2 * j + 1] = as2[j].y;
    }
    const float up = __shfl_up(ap[R - 1], 1);
    const float pp_new = tile_last(ap, tm);
    if (m0 < tm) {
      float prev = lane ? up : pp;
      const float swf = P.swf, cwf = P.cwf;
      f8 bs;
      if constexpr (EX) {
#pragma unroll
        for (int r = 0; r < R; r++) {
          bs[r] = as[r] * carrier_of<EX>(ap[r], prev, swf, cwf);
          prev = ap[r];
        }
      } else {
        const float inv_k2 = P.car_inv_k2;
        const float prev0 = prev;
        float margin = 1.f;
#pragma unroll
        for (int r = 0; r < R; r += 2) {
          const f2 b2 = carrier_fast2(f2{ap[r], ap[r + 1]}, prev, f2{as[r], as[r + 1]}, swf, cwf, inv_k2, margin);
          bs[r] = b2.x;
          bs[r + 1] = b2.y;
          prev = ap[r + 1];
        }
        if (__builtin_expect(margin < 0.f, 0)) {       /* rare: which of the eight was it */
          float q = prev0;
#pragma unroll
          for (int r = 0; r < R; r++) {
            float mg = 1.f;
            (void)carrier_fast(ap[r], q, as[r], swf, cwf, inv_k2, mg);
            if (mg < 0.f && m0 + r < tm) fragile |= 1u << r;
            q = ap[r];
          }
        }
      }
      f4 *dst = reinterpret_cast<f4 *>(&w.ms[HV + m0]);
#pragma unroll
      for (int r = 0; r < R; r += 2) dst[r >> 1] = f4{am[r], bs[r], am[r + 1], bs[r + 1]};
    }
    wave_lds_sync();
    pp = pp_new;
  } else {
    const int half = P.half, size = P.size;
    const float swf = P.swf, cwf = P.cwf;
    for (int m = lane; m < tm; m += 64) {
      const float *x = &w.v[HV + m - (size - 1)];
      float am = 0.f, ap = 0.f, as = 0.f, aq = 0.f;   /* aq: pilot output of sample m-1, same order */
      for (int k = 0; k < half; k++) {
        const float p = x[k] + x[size - 1 - k];
        const float pq = x[k - 1] + x[size - 2 - k];
        const f4 t = tap_mpx[k];
        am = mac<EX>(am, p, t.x);
        ap = mac<EX>(ap, p, t.y);
        as = mac<EX>(as, p, t.z);
        aq = mac<EX>(aq, pq, t.y);
      }
      if (m == 0) aq = pp;
      if (m == tm - 1) w.pp[0] = ap;
      float car;
      if constexpr (EX) {
        car = carrier_of<EX>(ap, aq, swf, cwf);
      } else {
        float mg = 1.f;
        car = carrier_fast(ap, aq, as, swf, cwf, P.car_inv_k2, mg);
        if (mg < 0.f) fragile |= 1u << (m >> 6);          /* this lane's i-th sample: m = lane + 64 i */
      }
      w.ms[HV + m] = make_float2(am, as * car);
    }
    wave_lds_sync();
    pp = w.pp[0];
  }
  return fragile;
}

/* ---- the int8 fixed-point form of the 90-tap MPX filters on the matrix pipe: limbs, tap rows ----------------------------------------
 *
 * The MPX filters are 90-tap FIRs on one input: y_f[m] = sum_t h_f[t] v[m - t], h_f[t] = tap_f[min(t, 89 - t)] (src/rtl_fm_player.c:538-566 sums the
 * same products pairwise).  As a matrix product per block of 256 outputs on v_mfma_i32_16x16x64_i8 (16 cycles of the matrix pipe for K = 64):
 *   D[i][j] = sum_k A[i][k] B[k][j],  A[i][k] = T_f[112 + i - k]  (banded Toeplitz: the taps, 90 of 128 non-zero),  B[k][j] = q[16 j - 112 + k]
 *   (column j = the 128-sample window that ends with the column's last output),  lane (j, g) holds outputs 256 blk + 16 j + 4 g + r, r < 4.
 * Samples are fixed point q = round(v 2^20) in three balanced int8 limbs (split at the end of stage B: split_i8x3, three byte arrays in LDS beside the fp32
 * one), taps T_f = round(h_f 2^qf) likewise (qf per filter: the largest that keeps |T| inside three limbs; fmd_resolve.c, build_ci_scales).  Every limb product sum is
 * EXACT integer arithmetic; six of the nine limb pairs are kept (tap limb + sample limb <= 2; eight for the pilot filter from volume 1 up), accumulated by
 * weight class in int32 accumulators that start from the bits of 1.5 x 2^23 and are read as floats (no conversions), put together in fp32 once:
 *   y = 2^(12 - qf) (A0 + A1 2^-8 + A2 2^-16 [+ A3 2^-24]).
 * The only errors are the two quantisations: |dv| <= 2^-21 (|v| < 8: the discriminator's range and what quirk Q1 can put in its place), |dh| <= 2^-(qf + 1) -
 * the rounding class of the vector form's fused sums, inside the +-1 LSB contract (DESIGN.md section 2a); the ill-conditioned-carrier redo works from the fp32 array.
 * The tap rows: lane (i, g) holds, per (filter, slice, limb), the 16 bytes of the reversed, zero-padded 144-byte tap table at 15 - i + 64 s + 16 g - read ONCE
 * per kernel (an unaligned ds_read_b128 each: mpx_i8_taps) and kept in registers (two workers per SIMD have the room).
 * (Round 3 built a first form of this and found it "not deterministic with several workers per SIMD": its MFMA bursts were the neighbour under which the packed
 * instructions of the forbidden form - pk_add_rot90 in k_common.inc - went wrong in the sibling workers.  With that form gone: tests/test_gpu_neighbour.py.) */
constexpr int HB = 112;                 /* bytes of history the pilot / L-R filters' windows reach back (of HBE kept) */
constexpr int CI_N = 144;               /* bytes per (filter, limb) tap table */
constexpr float VQ_SCALE = 1048576.0f;  /* 2^20 */

/* eight discriminator outputs as three balanced int8 limbs each (limb 0 most significant), packed per limb in sample order:
 * q = round(x 2^20); the bytes of (q + 0x808080) with their top bits flipped ARE the balanced digits (byte - 128). */
__device__ __forceinline__ void split_i8x3(const f8 &v, uint2 (&lb)[3]) {
  uint32_t q[8];
#pragma unroll
  for (int r = 0; r < 8; r++) {
    int qi;
    const float xs = v[r] * VQ_SCALE;
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(qi) : "v"(xs));              /* floor(x + 0.5): one instruction (ties do not matter here) */
    q[r] = ((uint32_t)qi + 0x808080u) ^ 0x808080u;
  }
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint32_t a = q[4 * h], b = q[4 * h + 1], c = q[4 * h + 2], d = q[4 * h + 3];
    /* v_perm_b32 D, S0, S1, sel: source bytes 0-3 = S1, 4-7 = S0 */
    const uint32_t t01 = __builtin_amdgcn_perm(b, a, 0x05010602u);      /* (a.b2, b.b2, a.b1, b.b1) */
    const uint32_t t23 = __builtin_amdgcn_perm(d, c, 0x05010602u);
    const uint32_t u01 = __builtin_amdgcn_perm(b, a, 0x0c0c0400u);      /* (a.b0, b.b0, 0, 0) */
    const uint32_t u23 = __builtin_amdgcn_perm(d, c, 0x0c0c0400u);
    const uint32_t l0 = __builtin_amdgcn_perm(t23, t01, 0x05040100u);   /* limb 0 of samples 4h .. 4h+3 */
    const uint32_t l1 = __builtin_amdgcn_perm(t23, t01, 0x07060302u);
    const uint32_t l2 = __builtin_amdgcn_perm(u23, u01, 0x05040100u);
    if (h == 0) { lb[0].x = l0; lb[1].x = l1; lb[2].x = l2; } else { lb[0].y = l0; lb[1].y = l1; lb[2].y = l2; }
  }
}

/* one sample (kernel start, quirk Q1): limb l in byte 2 - l of the result */
__device__ __forceinline__ uint32_t split_i8x3_one(float x) {
  return ((uint32_t)(int)__builtin_floorf(__builtin_fmaf(x, VQ_SCALE, 0.5f)) + 0x808080u) ^ 0x808080u;
}

typedef int i4a1 __attribute__((ext_vector_type(4), aligned(1)));
/* the lane's eighteen tap operands (filter, slice, limb): tile-invariant, read once per kernel and kept in registers */
__device__ __forceinline__ void mpx_i8_taps(const int8_t *ci_tab, int lane, i4 (&t)[3][2][3]) {
  const FMD_LDS int8_t *tb = opaque_lds(ci_tab + (15 - (lane & 15) + 16 * (lane >> 4)));
#pragma unroll
  for (int f = 0; f < 3; f++)
#pragma unroll
    for (int sl = 0; sl < 2; sl++)
#pragma unroll
      for (int l = 0; l < 3; l++) {
        const i4a1 x = *reinterpret_cast<const FMD_LDS i4a1 *>(tb + (f * 3 + l) * CI_N + 64 * sl);
        t[f][sl][l] = i4{x.x, x.y, x.z, x.w};
      }
}

__device__ __forceinline__ int emit_index_magic(uint32_t c0, int q, uint32_t fast, uint32_t magic, uint32_t sh);

/* four values (already scaled by 2^20) as three limb words: byte r of word l = limb l of value r (split_i8x3's inner step) */
__device__ __forceinline__ void split_i8x3_quad(float x0, float x1, float x2, float x3, uint32_t (&lw)[3]) {
  uint32_t q[4];
  const float xs[4] = {x0, x1, x2, x3};
#pragma unroll
  for (int r = 0; r < 4; r++) {
    int qi;
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(qi) : "v"(xs[r]));
    q[r] = ((uint32_t)qi + 0x808080u) ^ 0x808080u;
  }
  const uint32_t t01 = __builtin_amdgcn_perm(q[1], q[0], 0x05010602u);
  const uint32_t t23 = __builtin_amdgcn_perm(q[3], q[2], 0x05010602u);
  const uint32_t u01 = __builtin_amdgcn_perm(q[1], q[0], 0x0c0c0400u);
  const uint32_t u23 = __builtin_amdgcn_perm(q[3], q[2], 0x0c0c0400u);
  lw[0] = __builtin_amdgcn_perm(t23, t01, 0x05040100u);
  lw[1] = __builtin_amdgcn_perm(t23, t01, 0x07060302u);
  lw[2] = __builtin_amdgcn_perm(u23, u01, 0x05040100u);
}

/* sample idx of a limb array triple (rows l0, l0 + 1, l0 + 2 of vb) as a float, and the store of one (cold paths) */
template <typename WM>
__device__ __forceinline__ float limb_value(const WM &w, int l0, int idx) {
  const int q = (int)w.vb[l0][idx] * 65536 + (int)w.vb[l0 + 1][idx] * 256 + (int)w.vb[l0 + 2][idx];
  return (float)q * (1.0f / VQ_SCALE);
}
template <typename WM>
__device__ __forceinline__ void limb_store(WM &w, int l0, int idx, float x) {
  const uint32_t q = split_i8x3_one(x);
#pragma unroll
  for (int l = 0; l < 3; l++) w.vb[l0 + l][idx] = (int8_t)(q >> (8 * (2 - l)));
}

/* ---- stage C of FMD_MATH_FAST_MFMA_F: the pilot and L-R filters on the matrix pipe, the carrier ------------------------------------------
 *
 * Per block of 256 outputs and filter (fp: the 19 kHz pilot, fs: the L-R band) D[i][j] = sum_k A[i][k] B[k][j] over a window of 128 samples (two K
 * slices): A[i][k] = T_f[112 + i - k] (the lane's tap operands, resident in registers for the whole kernel: mpx_i8_taps), B[k][j] = limb of
 * v[256 blk + 16 j + k - 112]; lane (j, g) holds FOUR CONSECUTIVE outputs 256 blk + 16 j + 4 g + r.  Six limb pairs (tap limb + sample limb <= 2) per slice,
 * eight for the pilot filter from volume 1 up (fmdk_params.pilot_pairs8: the carrier inherits its relative accuracy); accumulators start from the bits
 * of 1.5 x 2^23 and are read as floats (no conversion: the host checks that every weight class stays inside +-2^22).  Two accumulator sets in flight: a
 * filter's sums are put together while the matrix pipe works on the next one's.  The carrier (src/rtl_fm_player.c:472-481) needs the pilot output one
 * sample earlier: the lane's own register r - 1, for r = 0 register 3 of the lane that holds the four samples before (one ds_bpermute), for the block's
 * first sample the carried value.  (L-R) x carrier leaves as round(x 2^20) in three int8 limb arrays (one conflict-free ds_write_b32 per limb and block)
 * for the second stage; the L+R channel has no first stage of its own: its two low-passes (:545 / :560 and :588) are ONE 179-tap filter g = fm * fm over
 * the discriminator output, evaluated at the emit instants in stage D (resample_tile_dec).  What the reference's intermediate - the bm ring - is still
 * needed for is made where it is needed: the launch's first `size - 1` samples meet the CARRIED ring (lr_head_fix), the state that leaves the launch
 * holds it again (the kernel's epilogue), quirk Q1 sums g over the limb history (q1_patch_i8).
 * Returns the lane's ill-conditioned-carrier flags (bit 4 blk + r): carrier_fast, redo_carrier. */
template <int HV, typename WM>
__device__ __forceinline__ uint32_t mpx_tile_i8(const fmdk_params &P, const i4 (&tres)[3][2][3], const i4 &magic4, WM &w, int lane, float &pp) {
  const int j = lane & 15, g = lane >> 4;
  const float swf = P.swf, cwf = P.cwf, inv_k2 = P.car_inv_k2_q;
  uint32_t fragile = 0;
  float last0 = 0.f, pp_new = 0.f;
  static_for<0, 2>([&](auto b_) {
    constexpr int b = decltype(b_)::value;
    /* the block's six sample operands (slice, limb): window v[256 b + 16 j - 112 ..] */
    i4 d[2][3];
#pragma unroll
    for (int l = 0; l < 3; l++) {
      const FMD_LDS i4 *xb = reinterpret_cast<const FMD_LDS i4 *>(opaque_lds(&w.vb[l][HBE - 112 + 16 * j + 16 * g]));
#pragma unroll
      for (int sl = 0; sl < 2; sl++) d[sl][l] = xb[16 * b + 4 * sl];
    }
    constexpr int PA[8] = {0, 0, 1, 0, 1, 2, 1, 2}, PB[8] = {0, 1, 0, 2, 1, 0, 2, 1};
    auto issue = [&](auto f_, i4 (&a)[4]) {
      constexpr int f = decltype(f_)::value;
      a[0] = a[1] = a[2] = a[3] = magic4;
      auto pair = [&](auto p_) {
        constexpr int pi = decltype(p_)::value, c = PA[pi] + PB[pi];
        static_for<0, 2>([&](auto s_) {
          constexpr int sl = decltype(s_)::value;
          a[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(tres[f][sl][PA[pi]], d[sl][PB[pi]], a[c], 0, 0, 0);    /* taps = A, samples = B */
        });
      };
      static_for<0, 6>(pair);
      if constexpr (f == 1) {
        if (P.pilot_pairs8) static_for<6, 8>(pair);
      }
    };
    auto join = [&](auto f_, const i4 (&a)[4], f4 &out) {
      constexpr int f = decltype(f_)::value;
      const float c0 = f != 1 ? P.ci_scale_q[f] : P.ci_scale[f];       /* L-R at 2^20 times its value (what its limb split wants); the carrier is scale-free in the pilot output */
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int a0 = a[0][r], a1 = a[1][r], a2 = a[2][r], a3 = a[3][r];       /* (scalars first: tools/diag/bitcast_vector_element.hip) */
        float y = __builtin_fmaf(__builtin_bit_cast(float, a0), c0, c0 * -12632256.0f);        /* - 12582912 (1 + 2^-8 + 2^-16) c0 */
        y = __builtin_fmaf(__builtin_bit_cast(float, a1), c0 * 0x1p-8f, y);
        y = __builtin_fmaf(__builtin_bit_cast(float, a2), c0 * 0x1p-16f, y);
        if constexpr (f == 1) y += __builtin_fmaf(__builtin_bit_cast(float, a3), c0 * 0x1p-24f, c0 * (-12582912.0f * 0x1p-24f));   /* = c3 S3, exact */
        out[r] = y;
      }
    };
    i4 ax[4], ay[4];
    f4 vp4, vs4;
    issue(std::integral_constant<int, 1>{}, ax);
    issue(std::integral_constant<int, 2>{}, ay);
    join(std::integral_constant<int, 1>{}, ax, vp4);
    join(std::integral_constant<int, 2>{}, ay, vs4);
    float vpl[4];
#pragma unroll
    for (int r = 0; r < 4; r++) vpl[r] = vp4[r];
    float prevv[4];
    {
      const int from = ((g ? lane - 16 : lane + 47) & 63) << 2;
      const float p3 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(from, __builtin_bit_cast(int, vpl[3])));
      prevv[0] = lane == 0 ? (b ? last0 : pp) : p3;
#pragma unroll
      for (int r = 1; r < 4; r++) prevv[r] = vpl[r - 1];
    }
    const float end3 = vpl[3];
    const float endv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, end3), 63));   /* the block's last pilot output */
    if constexpr (b == 0) last0 = endv; else pp_new = endv;
    float margin = 1.f;
    const f2 bs0 = carrier_fast2v(f2{vpl[0], vpl[1]}, f2{prevv[0], prevv[1]}, f2{vs4[0], vs4[1]}, swf, cwf, inv_k2, margin);
    const f2 bs1 = carrier_fast2v(f2{vpl[2], vpl[3]}, f2{prevv[2], prevv[3]}, f2{vs4[2], vs4[3]}, swf, cwf, inv_k2, margin);
    if (__builtin_expect(margin < 0.f, 0)) {         /* rare: which of the four was it (bit 4 blk + r) */
#pragma unroll
      for (int r = 0; r < 4; r++) {
        float mg = 1.f;
        (void)carrier_fast(vpl[r], prevv[r], vs4[r], swf, cwf, inv_k2, mg);
        if (mg < 0.f) fragile |= 1u << (4 * b + r);
      }
    }
    uint32_t ls[3];
    split_i8x3_quad(bs0[0], bs0[1], bs1[0], bs1[1], ls);
#pragma unroll
    for (int l = 0; l < 3; l++) reinterpret_cast<uint32_t *>(&w.vb[3 + l][HBE + 256 * b])[4 * j + g] = ls[l];
  });
  wave_lds_sync();
  pp = pp_new;
  return fragile;
}

