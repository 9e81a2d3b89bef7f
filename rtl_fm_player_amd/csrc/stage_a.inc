/* stage_a.inc - part of the fused IQ -> PCM kernel (included by fmd_kernels.inc inside its anonymous namespace; not a translation unit of its own).
 * Stage A: tile loads, u8 -> f32 + j^n rotation + 32-tap /8 FIR (reference src/rtl_fm_player.c:195-239, :253-411) - exact / fast vector forms, the int8 matrix-pipe form, the exact single-output and whole-tile forms of the cold paths, the launch's first three outputs. */

/* ---- tile load --------------------------------------------------------------- */

/* rate_in sample n covers IQ bytes [16n, 16n+16) of the stream (one 16-byte
 * word); output m of the /8 FIR needs words m-3 .. m, so a lane's 8 outputs need
 * 11 words.  They are loaded straight into registers at the start of stage A;
 * with four workers per SIMD the other three cover the latency, and the 3-word
 * overlap between neighbouring lanes is served by L1.  Word indices are clamped
 * into the stream (clamped words only feed outputs that are masked or patched). */
__device__ __forceinline__ void load_tile(uint4 (&q)[11], __amdgpu_buffer_rsrc_t iq_rsrc, int n_tile, int m0) {
  /* buffer loads: one byte offset per lane, eleven immediate offsets, and the hardware's
   * range check stands in for the clamping at the two ends of the stream (words before
   * the first / after the last sample read as zero and only feed outputs that are
   * discarded or replaced by the carried head) */
  typedef uint32_t u4v __attribute__((ext_vector_type(4)));
  const int byte0 = (n_tile + m0 - 3) * 16;
#pragma unroll
  for (int i = 0; i < 11; i++) {
    const u4v t = __builtin_amdgcn_raw_buffer_load_b128(iq_rsrc, byte0 + 16 * i, 0, 0);
    q[i] = make_uint4(t.x, t.y, t.z, t.w);
  }
}

/* The lane's own eight words only (decimate8_own). */
__device__ __forceinline__ void load_tile_own(uint4 (&q)[11], __amdgpu_buffer_rsrc_t iq_rsrc, int n_tile, int m0) {
  typedef uint32_t u4v __attribute__((ext_vector_type(4)));
  const int byte0 = (n_tile + m0) * 16;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const u4v t = __builtin_amdgcn_raw_buffer_load_b128(iq_rsrc, byte0 + 16 * i, 0, 0);
    q[i] = make_uint4(t.x, t.y, t.z, t.w);
  }
  /* words 8 .. 10 are not used on this path: "define" them by an empty asm, so that where the two paths join they
   * are whatever their registers hold instead of copies of the last values */
#pragma unroll
  for (int i = 8; i < 11; i++) asm volatile("" : "=v"(q[i].x), "=v"(q[i].y), "=v"(q[i].z), "=v"(q[i].w));
}

/* ---- stage A: decimating IQ low-pass ----------------------------------- */

/* Rotation by j^p of window sample with phase p (src/rtl_fm_player.c:206-226):
 * which byte feeds the I / Q sum and with which sign. */
template <bool ROT> __device__ __forceinline__ constexpr int sel_i(int p) { return ROT ? (p & 1) : 0; }
template <bool ROT> __device__ __forceinline__ constexpr int sel_q(int p) { return ROT ? ((p & 1) ^ 1) : 1; }
template <bool ROT> __device__ __forceinline__ constexpr float sgn_i(int p) {
  return !ROT ? 1.f : ((p == 0 || p == 3) ? 1.f : -1.f);
}
template <bool ROT> __device__ __forceinline__ constexpr float sgn_q(int p) {
  return !ROT ? 1.f : ((p == 0 || p == 1) ? 1.f : -1.f);
}

/* Eight consecutive outputs from the lane's 88 IQ samples (sample j = bytes
 * 2j, 2j+1 of d[]); output r uses samples 8r .. 8r+31, phase = index mod 4. */
template <bool EX, bool ROT>
__device__ __forceinline__ void decimate8(const fmdk_params &P, uint4 (&q)[11], f2 (&y2)[8]) {   /* y2[r] = (I, Q) of output r */
  if constexpr (EX) {
    const int z = opaque_zero();
    uint32_t d[44];
#pragma unroll
    for (int i = 0; i < 11; i++) { d[4 * i] = q[i].x; d[4 * i + 1] = q[i].y; d[4 * i + 2] = q[i].z; d[4 * i + 3] = q[i].w; }
    /* sum_k (c[k] + c[31-k]) * fb[k], left to right (src/rtl_fm_player.c:371-403), every
     * operation unfused and in the reference's order, but on (I, Q) pairs (packed add / mul: the
     * same rounding per element) and with the byte conversions shared by two neighbouring
     * outputs: their windows cover 40 samples, converted once ((u - 127.5) / 128 is exact). */
    float fb[16];
#pragma unroll
    for (int k = 0; k < 16; k++) fb[k] = P.fb[k + z];
    static_for<0, 4>([&](auto h_) {
      constexpr int h = decltype(h_)::value;          /* outputs 2h, 2h + 1: samples 16h .. 16h + 39 */
      f2 t[40];
#pragma unroll
      for (int j = 0; j < 40; j++) {
        const int sj = 16 * h + j;                     /* sample index in the lane's 88 */
        const f2 u = {ubyte(d[sj >> 1], 2 * (sj & 1)), ubyte(d[sj >> 1], 2 * (sj & 1) + 1)};
        t[j] = __builtin_elementwise_fma(u, f2{0.0078125f, 0.0078125f}, f2{-0.99609375f, -0.99609375f});
      }
      static_for<0, 2>([&](auto o_) {
        constexpr int o = decltype(o_)::value, r = 2 * h + o;
        f2 acc = {0.f, 0.f};
        static_for<0, 16>([&](auto k_) {
          constexpr int k = decltype(k_)::value;
          constexpr int ja = 8 * o + k, jb = 8 * o + 31 - k, pa = k & 3, pb = (31 - k) & 3;
          auto rot = [](f2 v, int p) -> f2 {           /* j^p rotation of (I, Q), or none */
            if (!ROT) return v;
            return p == 0 ? v : p == 1 ? f2{-v.y, v.x} : p == 2 ? f2{-v.x, -v.y} : f2{v.y, -v.x};
          };
          const f2 sum = rot(t[ja], pa) + rot(t[jb], pb);
          const f2 prod = sum * fb[k];
          acc = (k == 0) ? prod : acc + prod;
        });
        y2[r] = acc;
      });
    });
  } else {
    /* offset and 1/128 folded into the taps: y = c + sum_j s[j] g[min(j,31-j)] u[j],
     * j ascending, g = fb / 128 and s the rotation sign (a free operand modifier).
     * Word-outer order: each byte is converted once and feeds the (up to four)
     * outputs whose window holds it; the 16 distinct taps are scalar operands.
     * Between words the accumulators and the next word pass through an empty asm:
     * a data dependency that keeps the scheduler from converting all 176 bytes up
     * front (168 VGPRs without it, 66 with it). */
    const int z = opaque_zero();
    float g[16];
#pragma unroll
    for (int k = 0; k < 16; k++) g[k] = P.fbs[k + z];
    /* Packed arithmetic: an output's I and Q sums are one register pair.  With the j^n
     * rotation the even phases add +-g (I, Q) to (yi, yq) and go into pa[]; the odd phases
     * add (-+g Q, +-g I): they accumulate +-g (I, Q) in a second pair ma[] whose halves are
     * added to yq and subtracted from yi at the end -- every v_pk_fma then has one sign for
     * both halves and takes the converted bytes as they are. */
    f2 pa[8], ma[8];
#pragma unroll
    for (int r = 0; r < 8; r++) { pa[r] = f2{P.c_i, P.c_q}; ma[r] = f2{0.f, 0.f}; }
    static_for<0, 11>([&](auto w_) {
      constexpr int wd = decltype(w_)::value;
      const uint4 x = q[wd];
      /* The sign-flip constant passes through the fence with the accumulators: the flipped words - and so
       * every conversion of this word - depend on it, which keeps them below the arithmetic of the word
       * before.  (Tying the IQ words themselves to the fence costs 44 register copies per tile: they are
       * the landing registers of the next tile's loads.) */
      uint32_t kx = 0x80808080u;
      if constexpr (ROT)
        asm volatile("" : "+v"(pa[0]), "+v"(pa[1]), "+v"(pa[2]), "+v"(pa[3]), "+v"(pa[4]), "+v"(pa[5]), "+v"(pa[6]),
                       "+v"(pa[7]), "+v"(ma[0]), "+v"(ma[1]), "+v"(ma[2]), "+v"(ma[3]), "+v"(ma[4]), "+v"(ma[5]),
                       "+v"(ma[6]), "+v"(ma[7]), "+s"(kx));
      else
        asm volatile("" : "+v"(pa[0]), "+v"(pa[1]), "+v"(pa[2]), "+v"(pa[3]), "+v"(pa[4]), "+v"(pa[5]), "+v"(pa[6]),
                       "+v"(pa[7]), "+s"(kx));
      /* bytes as u - 128: flip the top bits of the word, convert as signed bytes (one SDWA
       * v_cvt_f32_i32 each).  The sums then stay at signal level -- with the unsigned bytes and
       * the offset folded into a constant they carried the 127.5 DC term until the end, and its
       * rounding showed as +-2 LSB of PCM on the rare noise samples that land next to zero. */
      const uint32_t d[4] = {x.x ^ kx, x.y ^ kx, x.z ^ kx, x.w ^ kx};
      static_for<0, 8>([&](auto t_) {
        constexpr int t = decltype(t_)::value, sx = 8 * wd + t;
        const float ui = sbyte(d[t >> 1], 2 * (t & 1)), uq = sbyte(d[t >> 1], 2 * (t & 1) + 1);
        const f2 uiq = {ui, uq};
        static_for<0, 8>([&](auto r_) {
          constexpr int r = decltype(r_)::value, j = sx - 8 * r;
          if constexpr (j >= 0 && j < 32) {
            constexpr int p = j & 3;
            const float gk = g[j < 16 ? j : 31 - j];
            if constexpr (!ROT || (p & 1) == 0) {
              static_assert(sel_i<ROT>(p) == 0 && sel_q<ROT>(p) == 1 && sgn_i<ROT>(p) == sgn_q<ROT>(p), "even phase");
              const float sg = sgn_i<ROT>(p) * gk;
              pa[r] = __builtin_elementwise_fma(uiq, f2{sg, sg}, pa[r]);
            } else {
              static_assert(sel_i<ROT>(p) == 1 && sel_q<ROT>(p) == 0 && sgn_i<ROT>(p) == -sgn_q<ROT>(p), "odd phase");
              const float sg = sgn_q<ROT>(p) * gk;
              ma[r] = __builtin_elementwise_fma(uiq, f2{sg, sg}, ma[r]);   /* (to yq, to -yi): no swapped copy needed */
            }
          }
        });
      });
    });
#pragma unroll
    for (int r = 0; r < 8; r++) {
      /* (yi, yq) = pa + (-ma.y, ma.x): one packed add (half swap and sign are operand modifiers) */
      if constexpr (ROT) y2[r] = pk_add_rot90(pa[r], ma[r]);
      else y2[r] = pa[r];
    }
  }
}

/* Fast kernels, full tiles, rotating path: the same sums from the lane's OWN eight words.  Word i of the lane
 * (stream word 8 lane + i of the tile) feeds outputs i .. i + 3 of the lane's numbering, so the lane accumulates
 * eleven outputs: 0 .. 7 are its own (still missing what the three words before its first contribute), 8 .. 10
 * are the first three outputs of the next lane, which receives them by one DPP rotation of the wave and adds
 * them to its own.  Lane 0 takes what lane 63 had left over from the PREVIOUS tile (carry[], used in lane 63
 * only; zero at the start of a chunk, whose first three outputs are replaced by the carried head or lie in the
 * replayed tile).  128 byte conversions and 8 loads per lane and tile instead of 176 and 11; the additions of one
 * output happen in a different order than in decimate8 (+-1 LSB contract). */
constexpr int DPP_WAVE_ROR1_A = 0x13C;
__device__ __forceinline__ void decimate8_own(const fmdk_params &P, uint4 (&q)[11], f2 (&y2)[8], f2 (&carry)[3], int lane) {
  const int z = opaque_zero();
  float g[16];
#pragma unroll
  for (int k = 0; k < 16; k++) g[k] = P.fbs[k + z];
  f2 pa[11], ma[11];              /* each starts with its first contribution (no zeroing): output r first meets word max(r - 3, 0) */
  const f2 c0 = {P.c_i, P.c_q};
  static_for<0, 8>([&](auto w_) {
    constexpr int wd = decltype(w_)::value;
    const uint4 x = q[wd];
    uint32_t kx = 0x80808080u;
    /* the fence of decimate8: the outputs this word adds to (those it starts are not live yet), and the sign-flip constant */
    if constexpr (wd == 0) asm volatile("" : "+s"(kx));
    else asm volatile("" : "+v"(pa[wd]), "+v"(pa[wd + 1]), "+v"(pa[wd + 2]), "+v"(ma[wd]), "+v"(ma[wd + 1]), "+v"(ma[wd + 2]), "+s"(kx));
    const uint32_t d[4] = {x.x ^ kx, x.y ^ kx, x.z ^ kx, x.w ^ kx};
    static_for<0, 8>([&](auto t_) {
      constexpr int t = decltype(t_)::value;
      const float ui = sbyte(d[t >> 1], 2 * (t & 1)), uq = sbyte(d[t >> 1], 2 * (t & 1) + 1);
      const f2 uiq = {ui, uq};
      static_for<0, 4>([&](auto o_) {
        constexpr int r = wd + decltype(o_)::value, j = 8 * (wd - r + 3) + t;   /* tap of this sample in output r */
        static_assert(j >= 0 && j < 32, "tap index");
        constexpr int p = j & 3;
        const float gk = g[j < 16 ? j : 31 - j];
        constexpr bool first_word = wd == (r > 3 ? r - 3 : 0);
        if constexpr ((p & 1) == 0) {
          const float sg = sgn_i<true>(p) * gk;
          if constexpr (first_word && t == 0) {
            if constexpr (r < 8) pa[r] = __builtin_elementwise_fma(uiq, f2{sg, sg}, c0);   /* the lane's own outputs carry the constant term */
            else pa[r] = uiq * f2{sg, sg};
          } else {
            pa[r] = __builtin_elementwise_fma(uiq, f2{sg, sg}, pa[r]);
          }
        } else {
          const float sg = sgn_q<true>(p) * gk;
          if constexpr (first_word && t == 1) ma[r] = uiq * f2{sg, sg};
          else ma[r] = __builtin_elementwise_fma(uiq, f2{sg, sg}, ma[r]);
        }
      });
    });
  });
#pragma unroll
  for (int r = 0; r < 8; r++) y2[r] = pk_add_rot90(pa[r], ma[r]);
  /* lanes 1 .. 63 add what their left neighbour has for them; lane 0 adds what lane 63 kept from the previous
   * tile: lane 63 sends carry[] (its leftovers of the tile before) instead of this tile's, and every lane then
   * remembers this tile's (only lane 63's copy is ever used).  Six v_add_f32 with a wave_ror:1 DPP operand, written
   * out: hipcc pairs two 32-bit DPP moves on the halves of a 2-vector into one and drops the second. */
  float o[6], snd[6], a[6];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const f2 out = pk_add_rot90(pa[8 + k], ma[8 + k]);
    o[2 * k] = out.x; o[2 * k + 1] = out.y;
    snd[2 * k] = (lane == 63) ? carry[k].x : out.x;
    snd[2 * k + 1] = (lane == 63) ? carry[k].y : out.y;
    a[2 * k] = y2[k].x; a[2 * k + 1] = y2[k].y;
  }
  asm volatile("s_nop 1\n\t"                      /* a DPP operand written by the VALU instruction before: two wait states */
               "v_add_f32_dpp %0, %6, %0 wave_ror:1 row_mask:0xf bank_mask:0xf\n\t"
               "v_add_f32_dpp %1, %7, %1 wave_ror:1 row_mask:0xf bank_mask:0xf\n\t"
               "v_add_f32_dpp %2, %8, %2 wave_ror:1 row_mask:0xf bank_mask:0xf\n\t"
               "v_add_f32_dpp %3, %9, %3 wave_ror:1 row_mask:0xf bank_mask:0xf\n\t"
               "v_add_f32_dpp %4, %10, %4 wave_ror:1 row_mask:0xf bank_mask:0xf\n\t"
               "v_add_f32_dpp %5, %11, %5 wave_ror:1 row_mask:0xf bank_mask:0xf"
               : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5])
               : "v"(snd[0]), "v"(snd[1]), "v"(snd[2]), "v"(snd[3]), "v"(snd[4]), "v"(snd[5]));
#pragma unroll
  for (int k = 0; k < 3; k++) {
    y2[k] = f2{a[2 * k], a[2 * k + 1]};
    carry[k] = f2{o[2 * k], o[2 * k + 1]};
  }
}

/* ---- stage A on the matrix pipe (FMD_MATH_FAST_MFMA) -------------------------------------------------
 *
 * v_mfma_i32_16x16x64_i8: D[16 x 16] += A[16 x 64] B[64 x 16], exact int32 sums of int8 products, 16 cycles of the
 * SIMD's matrix pipe, which the VALU-only kernels leave idle.  One column = EIGHT consecutive outputs of the /8
 * low-pass: its 16 rows are (output r = 0..7, component I / Q), its K axis the 176 window bytes those outputs
 * touch (words m0 - 3 .. m0 + 7), padded to 192 = three K slices.  A (lane = (row, g), 16 bytes) is the banded
 * tap matrix - row (r, c) holds the 32 taps of component c, rotation signs folded in, shifted by 16 r bytes - as
 * 26-bit fixed point in three int8 limbs (fmd_resolve.c, build_a_tab); B (lane = (column n, g)) is the lane's 16
 * window bytes [128 n + 64 s + 16 g - 48, + 16) of the tile, XOR 0x80 = u - 128 as int8, loaded straight from
 * HBM one tile ahead.  A tile is 4 column blocks x 3 slices x 3 limbs = 36 MFMAs (576 matrix-pipe cycles), 48
 * v_xor and, per output value, three conversions and three multiply-adds that put the limbs together:
 *   y = 2^-17 S0 + 2^-25 S1 + 2^-33 S2 + bias      (bias = the 127.5 offset of the reference's table)
 * where the VALU form spends 128 conversions and 256 packed multiply-adds per lane.  Rows 4g .. 4g+3 of column n
 * land in lane (n, g): outputs 128 cb + 8 n + 2 g + {0, 1} of the tile; a transpose across lanes (decimate_mfma)
 * makes them the eight consecutive outputs per lane that stages B and C work on. */
__device__ __forceinline__ void load_tile_mfma(uint4 (&q)[12], __amdgpu_buffer_rsrc_t iq_rsrc, int n_tile, int lane) {
  typedef uint32_t u4v __attribute__((ext_vector_type(4)));
  /* bytes before the stream's first / after its last read as zero (range check; the 32-bit offset wraps like
   * load_tile's) and only feed outputs that are replaced by the carried head or discarded */
  const int byte0 = n_tile * 16 + 128 * (lane & 15) + 16 * (lane >> 4) - 48;
#pragma unroll
  for (int cb = 0; cb < 4; cb++)
#pragma unroll
    for (int sl = 0; sl < 3; sl++) {
      /* cache policy bits 0: nt (2) measured +4 % stereo, +19 % mono - profiles/r6z_iq_cache_policy_ab.txt */
      const u4v t = __builtin_amdgcn_raw_buffer_load_b128(iq_rsrc, byte0 + 2048 * cb + 64 * sl, 0, 0);
      q[3 * cb + sl] = make_uint4(t.x, t.y, t.z, t.w);
    }
}

template <bool MAGIC>
__device__ __forceinline__ void decimate_mfma(const fmdk_params &P, const uint4 (&q)[12], f2 (&y2)[8], const i4 *a_tab,
                                              int lane, const i4 &magic4) {
  const int n = lane & 15, g = lane >> 4, r = n >> 1, c = n & 1;
  /* A operand of slice s, limb l: table entry d = 4 s + g - r of component c (zero outside 0 .. 3) */
  const FMD_LDS i4 *at = opaque_lds(a_tab + (c * A_SLOTS + g - r + 7));
  /* column-block outer: the nine A operands stay in registers (36), a block's three IQ words are flipped, multiplied
   * and put together before the next block's are touched (limb outer keeps 48 flipped words and 48 sums live) */
  i4 a[3][3];
#pragma unroll
  for (int l = 0; l < 3; l++)
#pragma unroll
    for (int sl = 0; sl < 3; sl++) a[l][sl] = at[l * 2 * A_SLOTS + 4 * sl];
  const float bi = P.a_bias_i, bq = P.a_bias_q;
  float oo[4][4];                                  /* the four blocks' results until the transpose */
  /* (software-pipelining this loop by one column block - block cb + 1's nine MFMAs issued in front of block cb's limbs -> float
   * arithmetic - measured no different, like the same interleave in stage C: profiles/archive/r06a_schedule_ab.txt.  The SIMD's other
   * worker already fills those slots, and an MFMA holds the vector issue port either way.) */
  static_for<0, 4>([&](auto cb_) {
    constexpr int cb = decltype(cb_)::value;
    /* the accumulators start from the bits of 1.5 x 2^23 (magic4): an int32 sum S, |S| <= 176 x 128 x 128 < 2^22, on top of them IS the float
     * 12582912 + S, so the limb sums are read as floats - no v_cvt_f32_i32 (mpx_tile_i8 does the same and says more) */
    i4 d[3] = {magic4, magic4, magic4};             /* (MAGIC == false: magic4 is zero and the sums are converted) */
    static_for<0, 3>([&](auto s_) {
      constexpr int sl = decltype(s_)::value;
      const uint4 x = q[3 * cb + sl];
      const i4 b = {(int)(x.x ^ 0x80808080u), (int)(x.y ^ 0x80808080u), (int)(x.z ^ 0x80808080u), (int)(x.w ^ 0x80808080u)};
#pragma unroll
      for (int l = 0; l < 3; l++) d[l] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[l][sl], b, d[l], 0, 0, 0);
    });
    /* limbs -> float; rows 4g + i = (output 2g + (i >> 1), component i & 1) of column n */
    f4 o;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      /* (joining the two low limbs as integers first - 256 S1 + S2 fits 31 bits - saves a conversion and a multiply-add per
       * value and measured 2.4 % SLOWER on the stereo kernel, same device: profiles/archive/r03r_stage_ab_microopts.txt; the (I, Q) pair of an
       * output as packed multiply-adds - 24 instructions fewer per tile - measured no different: profiles/archive/r05f_stage_a_packed_ab.txt) */
      if constexpr (!MAGIC) {
        const float s0 = (float)d[0][i], s1 = (float)d[1][i], s2 = (float)d[2][i];
        o[i] = __builtin_fmaf(s0, 0x1p-17f, __builtin_fmaf(s1, 0x1p-25f, __builtin_fmaf(s2, 0x1p-33f, (i & 1) ? bq : bi)));
        continue;
      }
      const int d0 = d[0][i], d1 = d[1][i], d2 = d[2][i];          /* (scalars first: tools/diag/bitcast_vector_element.hip) */
      /* the largest limb first: its multiply-add takes 12582912 (2^-17 + 2^-25 + 2^-33) = 96.37646484375 (exact) out again, the two others
       * put their 0.375 and 0.0015 back; every rounding at the result's own scale */
      float y = __builtin_fmaf(__builtin_bit_cast(float, d0), 0x1p-17f, -96.37646484375f);
      y = __builtin_fmaf(__builtin_bit_cast(float, d1), 0x1p-25f, y);
      y = __builtin_fmaf(__builtin_bit_cast(float, d2), 0x1p-33f, y);
      o[i] = y + ((i & 1) ? bq : bi);
    }
    oo[cb][0] = o[0]; oo[cb][1] = o[1]; oo[cb][2] = o[2]; oo[cb][3] = o[3];
  });
  /* Lane (n, g) holds, per column block cb, outputs 128 cb + 8 n + 2 g + {0, 1}; lane L = n + 16 g wants 8 L .. 8 L + 7 = 128 g + 8 n + 2 cb + {0, 1}
   * for cb = 0 .. 3: a transpose of the lane's g (lane bits 5, 4) with the register index cb.  gfx950 has the two instructions for it:
   * v_permlane32_swap (the upper 32 lanes of one register with the lower 32 of another: lane bit 5 <-> cb bit 1) and v_permlane16_swap (odd rows
   * of sixteen of one with the even rows of another: lane bit 4 <-> cb bit 0) - sixteen swaps per tile in place of four ds_write_b128, four
   * ds_read_b128 (8 KB through LDS), their address arithmetic and two waits. */
  /* (spelled as ONE asm statement per component, wait states included: of the eight __builtin_amdgcn_permlane16_swap calls hipcc 7.2 emitted
   * four - section 3's "two cross-lane operations come out as one" - and the result was wrong; and the hazard recognizer does not look inside asm
   * statements: a swap reading a register a vector instruction has just written, or a vector instruction reading a swap's result, needs two wait
   * states - without them the kernels with three workers per SIMD computed different PCM for equal streams) */
#pragma unroll
  for (int c = 0; c < 4; c++)
    asm volatile("s_nop 1\n\t"
                 "v_permlane32_swap_b32 %0, %2\n\t"
                 "v_permlane32_swap_b32 %1, %3\n\t"
                 "s_nop 1\n\t"
                 "v_permlane16_swap_b32 %0, %1\n\t"
                 "v_permlane16_swap_b32 %2, %3\n\t"
                 "s_nop 1"
                 : "+v"(oo[0][c]), "+v"(oo[1][c]), "+v"(oo[2][c]), "+v"(oo[3][c]));
#pragma unroll
  for (int t = 0; t < 4; t++) {
    y2[2 * t] = f2{oo[t][0], oo[t][1]};
    y2[2 * t + 1] = f2{oo[t][2], oo[t][3]};
  }
}

/* One decimator output (stream sample index n) in the reference's exact arithmetic,
 * from its four IQ words re-read from memory.  Only used by the fast kernels' cold paths
 * (branch-cut fix-up of the discriminator, carrier redo, hand-over).  (An integer form of the pair sums - they are
 * W / 256 with W = +-(2 ua - 255) +- (2 ub - 255) - was tried in round 4: no fewer instructions than v_cvt_f32_ubyteN +
 * one multiply-add per byte, and 30 registers more in its callers.) */
__device__ __forceinline__ float2 exact_from_words(const fmdk_params &P, const uint4 (&q)[4], bool rot) {
  const uint32_t d[16] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w,
                          q[2].x, q[2].y, q[2].z, q[2].w, q[3].x, q[3].y, q[3].z, q[3].w};
  float ai = 0.f, aq = 0.f;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    float ci[2], cq[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const int j = e ? 31 - k : k, p = j & 3;
      const float fi = t0(ubyte(d[j >> 1], 2 * (j & 1))), fq = t0(ubyte(d[j >> 1], 2 * (j & 1) + 1));
      /* j^p rotation (src/rtl_fm_player.c:206-226) or none */
      ci[e] = !rot ? fi : (p == 0 ? fi : p == 1 ? -fq : p == 2 ? -fi : fq);
      cq[e] = !rot ? fq : (p == 0 ? fq : p == 1 ? fi : p == 2 ? -fq : -fi);
    }
    const float fbk = P.fb[k];
    const float pi = (ci[0] + ci[1]) * fbk, pq = (cq[0] + cq[1]) * fbk;
    ai = (k == 0) ? pi : ai + pi;
    aq = (k == 0) ? pq : aq + pq;
  }
  return make_float2(ai, aq);
}
__device__ __forceinline__ void exact_load_words(const uint4 *iq16, int n, int n_total, uint4 (&q)[4]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    int c = n - 3 + i;
    c = c < 0 ? 0 : (c >= n_total ? n_total - 1 : c);
    q[i] = iq16[c];
  }
}
__device__ __forceinline__ float2 exact_output(const fmdk_params &P, const uint4 *iq16, int n, int n_total, bool rot) {
  uint4 q[4];
  exact_load_words(iq16, n, n_total, q);
  return exact_from_words(P, q, rot);
}

/* Fast kernels, cold path for QUIET input (VERDICT r4 item 3).  The reference itself mutes the stream with constant bytes after a
 * retune (src/rtl_fm_player.c:805-810), and a dongle without an antenna delivers bytes in {127, 128}: every decimated sample then
 * lies within 1e-3 of the origin, where its phase is decided by the reference's own rounding - all eight samples of every lane are
 * flagged, and redoing them one by one (two dependent rounds of IQ re-reads per sample) made such input 2.8 - 4.9 times slower than an
 * FM signal, slower than the exact kernels (profiles/archive/r5a_quiet_time_before.txt).  When a tile is that kind of tile the whole tile's
 * stages A and B run in the reference's arithmetic instead: decimate8<true>'s sums (the reference's operation order, unfused) for the
 * lane's eight outputs, two at a time in a rolled loop - the lane's 80 window bytes of a pair re-read from memory (they are in L2:
 * this tile's stage A has just streamed them), the results parked in 4 KB of the worker's slice that are idle during stage B - and
 * discriminate<true> on all eight.  Bounded by the exact kernels' cost of the two stages, whatever the input. */
template <bool ROT, bool PAIR>
__device__ __forceinline__ void exact_tile_decimate(const fmdk_params &P, __amdgpu_buffer_rsrc_t iq_rsrc, int n_tile, int lane, f2 *xa, f2 *xb, f2 (&y2)[8]) {
  typedef uint32_t u4v __attribute__((ext_vector_type(4)));
  /* PAIR: two outputs per step of the rolled loop, sharing their 40 converted samples (the kernels budgeted for two workers per SIMD
   * have the 80 registers); otherwise one output per step, its 32 samples converted where they are used */
  constexpr int NO = PAIR ? 2 : 1, NW = 3 + NO;
  /* the sixteen taps: four at a time from the kernarg segment, re-read where they are used (sixteen scalar registers held across this
   * loop do not exist beside the tile loop's own: hipcc parks them in VGPR lanes and fetches each back with a v_readlane per use -
   * the loop came out at 551 vector instructions per output) */
  const FMD_AS4 char *ka = (const FMD_AS4 char *)__builtin_amdgcn_kernarg_segment_ptr();
  (void)P;
  const int byte0 = (n_tile + 8 * lane - 3) * 16;       /* the lane's words 0 .. 10 (range check: zeros beyond the stream's ends, like load_tile) */
  u4v wd[NW];
#pragma unroll
  for (int i = 0; i < NW; i++) wd[i] = __builtin_amdgcn_raw_buffer_load_b128(iq_rsrc, byte0 + 16 * i, 0, 0);
#pragma unroll 2
  for (int h = 0; h < 8 / NO; h++) {                    /* outputs NO h ..: samples 8 NO h .. + 31 + 8 (NO - 1) of the lane's 88 = its words NO h .. NO h + NW - 1 */
    /* the words the next step adds, requested before this step's arithmetic (after the last step: words nobody reads) */
    u4v nx[NO];
#pragma unroll
    for (int i = 0; i < NO; i++) nx[i] = __builtin_amdgcn_raw_buffer_load_b128(iq_rsrc, byte0 + 16 * (NO * h + NW + i), 0, 0);
    uint32_t d[4 * NW];
#pragma unroll
    for (int i = 0; i < NW; i++) { d[4 * i] = wd[i].x; d[4 * i + 1] = wd[i].y; d[4 * i + 2] = wd[i].z; d[4 * i + 3] = wd[i].w; }
    /* decimate8<true>'s arithmetic: (u - 127.5) / 128 exact, sum_k (c[k] + c[31-k]) * fb[k] left to right, unfused, on (I, Q) pairs
     * (src/rtl_fm_player.c:371-403) */
    auto conv = [&](int j) -> f2 {
      const f2 u = {ubyte(d[j >> 1], 2 * (j & 1)), ubyte(d[j >> 1], 2 * (j & 1) + 1)};
      return __builtin_elementwise_fma(u, f2{0.0078125f, 0.0078125f}, f2{-0.99609375f, -0.99609375f});
    };
    f2 t[PAIR ? 40 : 1];
    if constexpr (PAIR) {
#pragma unroll
      for (int j = 0; j < 40; j++) t[j] = conv(j);
    }
    f2 out[NO];
    static_for<0, NO>([&](auto o_) {
      constexpr int o = decltype(o_)::value;
      f2 acc = {0.f, 0.f};
      f4 fq = {0.f, 0.f, 0.f, 0.f};
      static_for<0, 16>([&](auto k_) {
        constexpr int k = decltype(k_)::value;
        constexpr int ja = 8 * o + k, jb = 8 * o + 31 - k, pa = k & 3, pb = (31 - k) & 3;
        if constexpr ((k & 3) == 0) fq = *(const FMD_AS4 f4 *)(ka + offsetof(fmdk_params, fb) + 4 * (k + opaque_zero()));
        const float fbk = fq[k & 3];
        auto rot = [](f2 v, int p) -> f2 {
          if (!ROT) return v;
          return p == 0 ? v : p == 1 ? f2{-v.y, v.x} : p == 2 ? f2{-v.x, -v.y} : f2{v.y, -v.x};
        };
        f2 ca, cb;
        if constexpr (PAIR) { ca = t[ja]; cb = t[jb]; }
        else {
          /* (the tap's two words pass through a fence with the running sum: left alone the scheduler converts all 32 samples up front,
           * and the kernels at 168 registers then spill values that live across the whole tile loop) */
          uint32_t wa = d[ja >> 1], wb = d[jb >> 1];
          asm volatile("" : "+v"(wa), "+v"(wb), "+v"(acc));
          const f2 ua = {ubyte(wa, 2 * (ja & 1)), ubyte(wa, 2 * (ja & 1) + 1)}, ub = {ubyte(wb, 2 * (jb & 1)), ubyte(wb, 2 * (jb & 1) + 1)};
          ca = __builtin_elementwise_fma(ua, f2{0.0078125f, 0.0078125f}, f2{-0.99609375f, -0.99609375f});
          cb = __builtin_elementwise_fma(ub, f2{0.0078125f, 0.0078125f}, f2{-0.99609375f, -0.99609375f});
        }
        const f2 sum = rot(ca, pa) + rot(cb, pb);
        const f2 prod = sum * fbk;
        acc = (k == 0) ? prod : acc + prod;
      });
      out[o] = acc;
    });
    /* outputs 0 .. 3 park in one idle 2 KB of the worker's slice, 4 .. 7 in another */
    f2 *dst = (NO * h < 4 ? xa : xb) + 4 * lane + ((NO * h) & 3);
    if constexpr (PAIR) *reinterpret_cast<f4 *>(dst) = f4{out[0].x, out[0].y, out[1].x, out[1].y};
    else *dst = out[0];
#pragma unroll
    for (int i = 0; i + NO < NW; i++) wd[i] = wd[i + NO];
#pragma unroll
    for (int i = 0; i < NO; i++) wd[NW - NO + i] = nx[i];
  }
  wave_lds_sync();
#pragma unroll
  for (int r = 0; r < 8; r++) y2[r] = (r < 4 ? xa : xb)[4 * lane + (r & 3)];
  wave_lds_sync();
}

/* First three outputs of the launch: their window reaches into the carried
 * float history lowpass_tb (src/rtl_fm_player.c:261-363).  Computed once, before
 * the tile loop, by lanes 0..5 (output m = lane / 2, component = lane & 1) into
 * head[6]; the first tile's lane 0 then takes them instead of its own. */
template <bool ROT>
__device__ __forceinline__ void decimate_head(const fmdk_params &P, const uint8_t *raw, const float *tb,
                                              int lane, float *head) {
  if (lane < 6) {
    const int m = lane >> 1, comp = lane & 1;
    float acc = 0.f;
    for (int k = 0; k < 16; k++) {
      float pr[2];
      for (int e = 0; e < 2; e++) {
        const int j = e ? 31 - k : k;
        const int g = 8 * m - 24 + j;          /* IQ sample index from the start of the stream */
        float c;
        if (g < 0) {
          c = tb[2 * (24 + g) + comp];
        } else {
          const int p = j & 3;
          const int sel = comp ? sel_q<ROT>(p) : sel_i<ROT>(p);
          const float sg = comp ? sgn_q<ROT>(p) : sgn_i<ROT>(p);
          c = sg * t0((float)raw[2 * g + sel]);
        }
        pr[e] = c;
      }
      const float prod = (pr[0] + pr[1]) * P.fb[k];
      acc = (k == 0) ? prod : acc + prod;
    }
    head[lane] = acc;
  }
}

