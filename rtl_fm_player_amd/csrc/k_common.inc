/* k_common.inc - part of the fused IQ -> PCM kernel (included by fmd_kernels.inc inside its anonymous namespace; not a translation unit of its own).
 * Constants, the worker's LDS slice (WaveMem) and the workgroup's tables (Smem), opaque-value helpers, the arithmetic helpers every stage shares, DPP reads. */

constexpr int TW = FMDK_TILE;          /* rate_in samples per tile (8 per lane) */
constexpr int WPB = FMDK_WAVES;        /* workers (waves) per workgroup */
constexpr int NT = 64 * WPB;
constexpr int CAPW = FMDK_FRAME_CAP;   /* pending resampler outputs per worker */
constexpr int DEEMPH_GROUP = 16;       /* frames per de-emphasis lane */
static_assert(TW == 512, "a tile is 64 lanes x 8 outputs");
static_assert(CAPW / DEEMPH_GROUP <= 64, "one flush must fit one wave");

constexpr float K_PI = 3.14159265f;    /* include/rtl_fm_player.h:40 */
constexpr float K_PI_2 = 1.5707963f;   /* :41 */
constexpr float K_PI_4 = 0.78539816f;  /* :42 */

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f8 __attribute__((ext_vector_type(8)));   /* 8 per-lane outputs: an SSA value, never an alloca */
typedef int i4 __attribute__((ext_vector_type(4)));

/* history slots in front of each FIR tile: >= size - 1, and >= 92 for the
 * aligned window reads of the 90-tap stereo path */
template <int HALF> constexpr int hist_of() { return HALF == 45 ? 96 : (HALF == 64 ? 128 : 256); }

/* Lanes of one worker hand values to each other through its LDS slice.  The hardware executes the DS
 * operations of a wave in order; this tells the COMPILER the same at each hand-over point (a release /
 * acquire pair at wavefront scope and a wave barrier emit no instruction, they only keep later LDS reads
 * from being scheduled above earlier LDS writes whose addresses differ per lane). */
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int HBE = 192;                /* 90-tap stereo, FMD_MATH_FAST_MFMA_F: history bytes in front of each limb array (the composite L+R filter's window reaches back 180 samples) */
constexpr int HBM = 128;                /* 128-tap mono: likewise */
/* One worker's slice of LDS.  MFC: 90-tap stereo with stages C and D on the matrix pipe; MFM: 128-tap mono with stage D there (the two forms of
 * FMD_MATH_FAST_MFMA_F). */
template <int HV, bool STEREO = true, bool MFC = false, bool MFM = false>
struct __attribute__((aligned(16))) WaveMem {
  static constexpr bool kLimbs = MFC || MFM;                         /* kLimbs: the second stage reads int8 limb arrays - no fp32 {L+R, L-R} arrays */
  static constexpr int kVbh = MFC ? HBE : MFM ? HBM : 16;            /* history bytes in front of each limb array */
  static constexpr int kBsRow = 3;                                   /* first limb array of (L-R) x carrier */
  float v[HV + TW];          /* discriminator output, HV history slots in front   */
  float2 ms[kLimbs ? 2 : STEREO ? HV + TW : 2];   /* vector-ALU stereo: {L+R low-pass, (L-R band-pass) x carrier} */
  float fr[CAPW + CAPW / 32];/* resampler outputs waiting for the flush; one pad float per 32 (fidx):
                                flush lanes stride 16 frames x channels = 32 floats apart (exact kernels;
                                the fast kernels hold one tile's frames here, unpadded)           */
  float de[4];               /* de-emphasis state: [0..1] current, [2..3] next    */
  float pp[4];               /* scratch for the generic (runtime-size) MPX path   */
  float head[8];             /* the launch's first three decimator outputs (I,Q)  */
  float xs[STEREO ? (HV == 96 ? 192 : 260) : 4];/* fast kernels, cold path (carrier redo): the exactly recomputed discriminator window (size + 1
                                floats); 90-tap kernels first hold the size + 2 decimated (I, Q) pairs it is made from here */
  long long prof[12];        /* per-stage cycle sums (fmd_debug_taps.prof), [11] = last stamp */
#ifdef FMD_REDO_PROF
  long long rprof[6];        /* diagnostic builds: carrier redos: count, cycles of steps 1 / 2 / 3 / rest, discriminator redos */
#endif
  int8_t vb[MFC ? 6 : MFM ? 3 : 1][kLimbs ? kVbh + TW : 16] __attribute__((aligned(16)));   /* the discriminator output round(v 2^20) as three balanced int8 limb arrays
                                (rows 0 .. 2), kVbh history bytes in front of each: what the matrix-pipe stages C and D read; stereo: (L-R) x carrier likewise in rows 3 .. 5 */
};

constexpr int A_SLOTS = 24;  /* slots per (limb, component) of the stage-A operand table: 19 used (d = -7 .. 11), 24 apart so
                                that the two components of one ds_read_b128 group fall on disjoint banks */
/* FMD_MATH_FAST_MFMA_F (resample_tile_dec): bytes per (byte phase, limb) of the shifted tap tables of the composite L+R filter (DG) and of fm (DF);
 * the base tables they are cut from carry 16 more.  K0: the window's first sample, relative to the tile's first, for every group of sixteen frames. */
constexpr int DG_N = FMDK_DG_N, DF_N = FMDK_DF_N;
constexpr int DEC_K0G = FMDK_DEC_K0G, DEC_K0F = FMDK_DEC_K0F;
/* ... and of the 128-tap mono filter (resample_mono_dec): window K0 + P <= 256 samples, P <= 128 */
constexpr int DM_N = FMDK_DM_N, DEC_K0M = FMDK_DEC_K0M;
template <int HV, bool STEREO, bool MF, bool MFC, bool MFM = false>
struct __attribute__((aligned(16))) Smem {
  static constexpr bool kDec = MFC || MFM;   /* FMD_MATH_FAST_MFMA_F */
  f4 tap_mpx[HV == 96 ? 48 : 128];   /* {fm[k], fp[k], fs[k], 0}, zero beyond size/2 (90-tap kernels: 45 + padding) */
  f4 fm_lin[HV == 96 ? 12 : 32];     /* fm[0..127] contiguous (second-stage FIR), zero beyond size/2 */
  i4 a_tab[MF ? 3 * 2 * A_SLOTS : 1];   /* matrix-pipe stage A: fmdk_params.a_tab with zero entries around it */
  int8_t ci_tab[MFC ? 9 * 144 : 16] __attribute__((aligned(16)));   /* matrix-pipe stage C (90 taps): per (filter, limb) the taps
                                reversed and zero-padded, 144 (CI_N) bytes each: what the lane's resident tap operands are cut from (mpx_i8_taps) */
  /* The second stage at the emit instants only.  Row i of the banded product is frame i of a group of sixteen, its taps shifted by the frame's emit
   * index m_i (0 .. P - 1, P = 16 rate_out / rate_out2 samples per group): byte y of (phase r, limb l) = limb l of T[Y0 - r - y], so that the lane whose shift
   * is a = P - 1 - m_i reads ALIGNED 16-byte words at (a & ~15) + 64 slice + 16 g of phase a & 15.  dg: T = the composite filter g (Y0 = P + 179), df: fm
   * (Y0 = P + 91; 128-tap mono: P + 127).  Made once per batch by the host in device memory (fmdk_params.dec_tables: dg_rep, then df_rep) and copied here at
   * kernel start - contiguous, so the copy is one loop. */
  static constexpr int kFN = STEREO ? DF_N : DM_N;     /* the fm table: 90 taps (stereo) or 128 (mono) */
  int8_t dg_rep[MFC ? 16 * 3 * DG_N : 16] __attribute__((aligned(16)));
  int8_t df_rep[kDec ? 16 * 3 * kFN : 16] __attribute__((aligned(16)));
  WaveMem<HV, STEREO, MFC, MFM> w[WPB];
  int8_t tail_pad[kDec ? 1024 : 16];  /* the sample operands of frame groups beyond the tile's last frame read past the last worker's limb arrays (they meet zero taps or
                                         unused rows): at most 288 bytes (stereo), 560 (mono at P = 128, groups 4 .. 7 of which none holds a frame) */
};

/* A zero the optimiser cannot see through: indexing the kernarg tap tables with
 * it keeps their scalar loads inside the stage that uses them (hoisted to the
 * top of the kernel they do not fit the SGPR file and spill to VGPR lanes). */
__device__ __forceinline__ int opaque_zero() {
  int z;
  asm volatile("s_mov_b32 %0, 0" : "=s"(z));
  return z;
}

#define FMD_AS4 __attribute__((address_space(4)))
#define FMD_LDS __attribute__((address_space(3)))
/* An LDS pointer the compiler cannot see through (still a 32-bit LDS address, so reads through
 * it are ds_read): window offsets then fit the 8-bit fields of ds_read2_b64.  Seeing through it,
 * the compiler folds the slice's own offset inside LDS in as well, overflows the field and
 * re-bases with a v_add per read. */
template <typename T>
__device__ __forceinline__ const FMD_LDS T *opaque_lds(const T *p) {
  const FMD_LDS T *q = (const FMD_LDS T *)p;
  asm volatile("" : "+v"(q));
  return q;
}

/* ---- launch constants: kernarg scalars, the uniform bank ----------------- */

/* fmdk_params is the kernel's first argument, so P.fm/fp/fs sit in the kernarg
 * segment (constant address space).  Reading four consecutive taps there with a
 * wave-uniform index is one s_load_dwordx4 into SGPRs: no LDS traffic, no VGPRs,
 * and the FMA takes the tap as its scalar operand. */
template <size_t OFF>
__device__ __forceinline__ f4 ktap4(int first) {
  const FMD_AS4 char *ka = (const FMD_AS4 char *)__builtin_amdgcn_kernarg_segment_ptr();
  return *(const FMD_AS4 f4 *)(ka + OFF + 4 * first);
}
#define FMD_KTAP4(field, first) ktap4<offsetof(fmdk_params, field)>(first)

/* The uniform bank (the kernels of FMD_MATH_FAST_MFMA_F).  Stage D, the flush and the roll run at the highest wave priority with one other
 * worker on the SIMD, and the tile loop has no SGPR to spare: hipcc re-reads every launch constant those stages use from the kernarg segment each tile
 * and waits for it on the spot - s_waitcnt lgkmcnt(0), which drains the worker's LDS queue as well (scalar memory returns out of order, so no smaller
 * count will do).  The bank is ONE VGPR made before the tile loop: lane K holds constant K of the list below, and the loop takes it out with
 * v_readlane_b32 at a constant lane - one instruction, no memory counter.  Stages name the field (Uniforms::coef()), not the lane; the other families'
 * kernels instantiate the same stage code with BANKED = false and read the kernarg segment as before. */
enum : int {
  UB_EMIT_MAGIC, UB_EMIT_SHIFT, UB_DEC_P, UB_G_SCALE, UB_CI_SCALE0, UB_COEF, UB_PCM_STRIDE, UB_PCM_LO, UB_PCM_HI, UB_LENS_LO, UB_LENS_HI,
  UB_LAM_POW,                       /* lam_pow[0 .. 7] */
  UB_LAM_SCAN = UB_LAM_POW + 8,     /* lam_scan[0 .. 4] */
  UB_COUNT = UB_LAM_SCAN + 5
};
static_assert(UB_COUNT <= 64, "the bank is one register: a constant per lane");

template <bool BANKED>
struct Uniforms {
  const fmdk_params &P;
  int bank;
  template <int K> __device__ __forceinline__ uint32_t bank_u() const { return (uint32_t)__builtin_amdgcn_readlane(bank, K); }
  template <int K> __device__ __forceinline__ float bank_f() const { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(bank, K)); }
#define FMD_UNIFORM(type, name, get, field)                                                       \
  __device__ __forceinline__ type name() const {                                                  \
    if constexpr (BANKED) return get; else return P.field;                                        \
  }
  FMD_UNIFORM(uint32_t, emit_magic, bank_u<UB_EMIT_MAGIC>(), emit_magic)
  FMD_UNIFORM(uint32_t, emit_shift, bank_u<UB_EMIT_SHIFT>(), emit_shift)
  FMD_UNIFORM(int, dec_p, (int)bank_u<UB_DEC_P>(), dec_p)
  FMD_UNIFORM(float, g_scale, bank_f<UB_G_SCALE>(), g_scale)
  FMD_UNIFORM(float, ci_scale0, bank_f<UB_CI_SCALE0>(), ci_scale[0])
  FMD_UNIFORM(float, coef, bank_f<UB_COEF>(), coef)
  FMD_UNIFORM(int, pcm_stride, (int)bank_u<UB_PCM_STRIDE>(), pcm_stride)
#undef FMD_UNIFORM
  /* lam_pow[FIRST .. FIRST + 3] (lambda^(j+1)) and lam_scan[FIRST .. FIRST + 3] (a^(2^k)); entries the caller leaves unused cost nothing */
  template <int FIRST> __device__ __forceinline__ f4 lam_pow4() const {
    if constexpr (BANKED) return f4{bank_f<UB_LAM_POW + FIRST>(), bank_f<UB_LAM_POW + FIRST + 1>(), bank_f<UB_LAM_POW + FIRST + 2>(), bank_f<UB_LAM_POW + FIRST + 3>()};
    else return FMD_KTAP4(lam_pow, FIRST);
  }
  template <int FIRST> __device__ __forceinline__ f4 lam_scan4() const {
    static_assert(!BANKED || FIRST == 0 || FIRST == 4, "the bank holds lam_scan[0 .. 4]");
    if constexpr (!BANKED) return FMD_KTAP4(lam_scan, FIRST);
    else if constexpr (FIRST == 0) return f4{bank_f<UB_LAM_SCAN>(), bank_f<UB_LAM_SCAN + 1>(), bank_f<UB_LAM_SCAN + 2>(), bank_f<UB_LAM_SCAN + 3>()};
    else return f4{bank_f<UB_LAM_SCAN + 4>(), 0.f, 0.f, 0.f};
  }
};

/* a global-memory pointer (address space 1) from the two bank entries that hold its halves: an integer turned into a plain pointer would be a
 * FLAT one, whose stores count on lgkmcnt too */
#define FMD_GLB __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ FMD_GLB T *global_ptr(uint32_t lo, uint32_t hi) {
  return (FMD_GLB T *)(((unsigned long long)hi << 32) | lo);
}
/* the same pointer as another element type, address space kept */
template <typename T, typename S> __device__ __forceinline__ T *ptr_as(S *p) { return reinterpret_cast<T *>(p); }
template <typename T, typename S> __device__ __forceinline__ FMD_GLB T *ptr_as(FMD_GLB S *p) { return (FMD_GLB T *)p; }

/* ---- arithmetic helpers ------------------------------------------------ */

template <bool EX>
__device__ __forceinline__ float mac(float acc, float a, float b) {
  if constexpr (EX) {
    float p = a * b;       /* -ffp-contract=off keeps this unfused */
    return acc + p;
  } else {
    return __builtin_fmaf(a, b, acc);
  }
}

/* the same for two neighbouring outputs at once (v_pk_mul/add/fma_f32): with the clocks settled
 * the packed forms retire 1.5x the lane operations per second of the plain ones on this part
 * (tools/ubench: 74.6 vs 49.2 T lane-op/s on the MPX pattern), same rounding per element */
template <bool EX>
__device__ __forceinline__ f2 mac2(f2 acc, f2 a, float b) {
  if constexpr (EX) {
    const f2 p = a * b;
    return acc + p;
  } else {
    return __builtin_elementwise_fma(a, f2{b, b}, acc);
  }
}

/* Packed operations whose half swap / sign live in the operand modifiers.  hipcc materialises
 * f2{-b.y, b.x} with a v_xor and a v_mov before a plain v_pk_add; written out, the modifiers cost nothing.
 *
 * ONE FORM IS FORBIDDEN (round 4, tools/diag/repro, profiles/archive/r04_pk_opsel_hazard.md): a packed fp32 instruction whose LOW
 * lane combines the LOW half of one register pair with the HIGH half of a LATER operand's different pair - op_sel:[0,1],
 * [0,0,1], ... - computes that lane for lanes 48-63 with a zero in place of the high half while another wave of the SIMD
 * issues 128-bit-operand MFMAs (v_mfma_f32_16x16x32_bf16 and the other double-rate opcodes of gfx950).  The same
 * selection with the swapped operand FIRST (op_sel:[1,0]), uniform selections, op_sel_hi in any combination, sign
 * modifiers, scalar operands and both halves of ONE pair were clean in every run.  So every half swap below names the
 * swapped operand first, and tools/isa_lint.py (tests/test_isa_lint.py) refuses a build that holds the forbidden form -
 * hipcc makes it by itself from plain 2-vector code (`a + f2{b.y, b.x}`), which is why these are asm statements. */
__device__ __forceinline__ f2 pk_add_rot90(f2 a, f2 b) {          /* a + (-b.y, b.x) */
  f2 r;
  asm("v_pk_add_f32 %0, %2, %1 op_sel:[1,0] op_sel_hi:[0,1] neg_lo:[1,0]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ f2 pk_add_swap(f2 a, f2 b) {           /* a + (b.y, b.x) */
  f2 r;
  asm("v_pk_add_f32 %0, %2, %1 op_sel:[1,0] op_sel_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
/* (dot, cross) of two (I, Q) samples: (cur.x prev.x + cur.y prev.y, cur.y prev.x - cur.x prev.y).  t = (Q pj, I pj) takes
 * both of its low-lane factors from high halves, the multiply-add both from low halves: no mixed selection. */
__device__ __forceinline__ f2 pk_dotcross(f2 cur, f2 prev) {
  f2 t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1]" : "=v"(t) : "v"(cur), "v"(prev));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] neg_hi:[0,0,1]" : "=v"(r) : "v"(cur), "v"(prev), "v"(t));
  return r;
}
/* acc + a * t.y (both lanes): the operand whose high half is taken goes first */
__device__ __forceinline__ f2 pk_fma_hi(f2 a, f2 t, f2 acc) {
  f2 r;
  asm("v_pk_fma_f32 %0, %2, %1, %3 op_sel:[1,0,0]" : "=v"(r) : "v"(a), "v"(t), "v"(acc));
  return r;
}

__device__ __forceinline__ float min_abs(float a, float b) {      /* min(|a|, |b|): one v_min_f32 with |.| modifiers */
  float r;
  asm("v_min_f32 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

__device__ __forceinline__ float sbyte(uint32_t w, int i) {
  return (float)(int8_t)((w >> (8 * i)) & 0xffu);   /* v_cvt_f32_i32 with a sign-extended SDWA byte select */
}
__device__ __forceinline__ float ubyte(uint32_t w, int i) {
  return (float)((w >> (8 * i)) & 0xffu);   /* v_cvt_f32_ubyteN */
}

/* (u - 127.5) / 128: exact in fp32, one fused op (reference table [0]) */
__device__ __forceinline__ float t0(float u) { return __builtin_fmaf(u, 0.0078125f, -0.99609375f); }

/* a / b: IEEE division in the exact kernels, v_rcp_f32 (1 ulp) and a multiply in the fast ones */
template <bool EX>
__device__ __forceinline__ float fdiv(float a, float b) {
  if constexpr (EX) return a / b;
  else return a * __builtin_amdgcn_rcpf(b);
}

/* src/rtl_fm_player.c:606-667 through the magnitude ratio (see oracle/fm_oracle.c) */
template <bool EX>
__device__ __forceinline__ float poly_atan2(float y, float x) {
  const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
  const bool xmaj = ax >= ay;
  const float num = xmaj ? ay : ax;          /* selects: fminf/fmaxf would add a canonicalising v_max each */
  float a, den;
  if constexpr (EX) {
    den = xmaj ? ax : ay;
    a = num / den;                             /* 0/0 (both zero) is fixed up below */
  } else {
    den = __builtin_fmaxf(__builtin_fmaxf(ax, ay), 1e-37f);        /* one v_max3; both zero: 0 * rcp(tiny) = 0 */
    a = num * __builtin_amdgcn_rcpf(den);
  }
  float r0;
  if constexpr (EX) {
    r0 = a * (K_PI_4 - (a - 1.f) * (0.2447f + 0.0663f * a));
  } else {
    const float q = __builtin_fmaf(0.0663f, a, 0.2447f);
    r0 = a * __builtin_fmaf(-(a - 1.f), q, K_PI_4);
  }
  /* The reference's eight octant expressions (r0 - pi, -r0 - pi/2, -r0 + pi, pi/2 + r0,
   * -r0, r0 - pi/2, r0, pi/2 - r0) are  +-(base +- r0)  with base in {0, pi/2, pi}; IEEE
   * addition and negation are sign-symmetric, so this gives the same bits:
   *   theta = base + t,  base = xmaj ? (x < 0 ? pi : 0) : pi/2,
   *                      t    = xmaj ? copysign(r0, x) : -copysign(r0, x)
   *   result = y < 0 ? -theta : theta
   * and it needs no special cases on the axes: with y == +-0, r0 is 0 and theta is pi or 0
   * (the comparison y < 0 ignores the sign of a zero, like the reference's); with x == +-0,
   * theta is pi/2.  Only 0/0 is left, for the exact kernels.  Selects, not branches: the
   * lanes of a wavefront cover all octants anyway. */
  const float r0x = __builtin_copysignf(r0, x);
  const float base = xmaj ? ((x < 0.f) ? K_PI : 0.f) : K_PI_2;
  const float t = xmaj ? r0x : -r0x;
  const float theta = base + t;
  float r = (y < 0.f) ? -theta : theta;
  if constexpr (EX) r = __builtin_unpredictable(den == 0.f) ? 0.f : r;
  return r;
}

/* src/rtl_fm_player.c:472-481 */
template <bool EX>
__device__ __forceinline__ float carrier38(float x, float y) {
  if constexpr (EX) {
    const float z = y / x;
    const float den = 1.f + (z * z);
    const float c = (z + z) / den;
    return (x == 0.f) ? 0.f : c;
  } else {
    /* 2z / (1 + z^2) with z = y / x is 2xy / (x^2 + y^2): one reciprocal instead of two
     * (v_rcp_f32 issues at a quarter of the FMA rate); x == 0 gives 0 by itself, and the
     * clamp covers x == y == 0 */
    const float den = __builtin_fmaxf(__builtin_fmaf(x, x, y * y), 1e-37f);
    return ((x + x) * y) * __builtin_amdgcn_rcpf(den);
  }
}

template <bool EX>
__device__ __forceinline__ float carrier_of(float vp, float vq, float swf, float cwf) {
  const float x = vp * swf;
  float y;
  if constexpr (EX) y = vp * cwf - vq;
  else y = __builtin_fmaf(vp, cwf, -vq);
  return carrier38<EX>(x, y);
}

/* Fast kernels: the carrier and how well-conditioned it is.  sin 2 atan2(y, x) moves by 2 |e| / r for an
 * error e in (x, y) at radius r = |(x, y)|, and vs times that reaches the PCM through one tap of the
 * second-stage low-pass.  When the envelope of the pilot filter's output dips (noise input; a broadcast
 * pilot sits four orders of magnitude higher) the fast and the reference arithmetic - which differ by
 * rounding - regenerate different carriers, and nothing short of the reference's own bits pins the
 * result.  margin = r^2 / K^2 - vs^2 goes negative exactly there (K from the host: the radius below
 * which such a difference can reach a quarter LSB); the caller redoes those samples in the reference's
 * exact arithmetic (redo_carrier). */
__device__ __forceinline__ float carrier_fast(float vp, float vq, float vs, float swf, float cwf, float inv_k2,
                                              float &margin) {
  const float x = vp * swf;
  const float y = __builtin_fmaf(vp, cwf, -vq);
  /* + 1e-37 inside the first multiply-add: below the last bit of any real r^2, and x == y == 0 gives 0 * 1e37 = 0
   * without a clamp (a v_max here costs two instructions: hipcc canonicalises its operand first) */
  const float r2 = __builtin_fmaf(x, x, __builtin_fmaf(y, y, 1e-37f));
  margin = __builtin_fminf(margin, __builtin_fmaf(r2, inv_k2, -(vs * vs)));
  return ((x + x) * y) * __builtin_amdgcn_rcpf(r2);
}

/* src/rtl_fm_player.c:711-735 */
__device__ __forceinline__ int16_t to_s16(float x, float coef) {
  /* clip then round-to-nearest-even == the reference's compare / compare / lrintf (the
   * bounds are integers).  Adding 1.5 * 2^23 leaves the rounded integer in the low
   * mantissa bits, two's complement for negative values: three VALU ops in all. */
  const float t = __builtin_amdgcn_fmed3f(x * coef, -32768.0f, 32767.0f);
  return (int16_t)__builtin_bit_cast(uint32_t, t + 12582912.0f);
}

/* compile-time loop: f(integral_constant<int, I>) for I in [B, E) -- indices stay
 * constant expressions, so register "arrays" never become private memory */
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}
template <int I>
__device__ __forceinline__ float elem(const f4 &a, const f4 &b, const f4 &c, const f4 &d) {
  if constexpr (I < 4) return a[I & 3];
  else if constexpr (I < 8) return b[I & 3];
  else if constexpr (I < 12) return c[I & 3];
  else return d[I & 3];
}

/* element (idx & 7) of an 8-entry register array, idx uniform or per lane */
/* element (n - 1) of the tile's n values, 8 per lane, broadcast: in the common full tile
 * that is element 7 of lane 63, a short tile has to select first */
__device__ __forceinline__ float pick8(const f8 &a, int idx);
__device__ __forceinline__ float tile_last(const f8 &a, int n) {
  if (n == TW)
    return __shfl(a[7], 63);
  return __shfl(pick8(a, n - 1), (n - 1) >> 3);
}
__device__ __forceinline__ float pick8(const f8 &a, int idx) {
  float r = a[0];
#pragma unroll
  for (int i = 1; i < 8; i++) r = ((idx & 7) == i) ? a[i] : r;
  return r;
}

/* element (n - 1) of the tile's n (I, Q) pairs, 8 per lane, broadcast */
__device__ __forceinline__ void tile_last2(const f2 (&a)[8], int n, float &re, float &im) {
  if (n == TW) {
    re = __shfl(a[7].x, 63);
    im = __shfl(a[7].y, 63);
    return;
  }
  f2 r = a[0];
#pragma unroll
  for (int i = 1; i < 8; i++) r = (((n - 1) & 7) == i) ? a[i] : r;
  re = __shfl(r.x, (n - 1) >> 3);
  im = __shfl(r.y, (n - 1) >> 3);
}

/* index into the padded pending-frame buffer (exact kernels); the fast kernels flush every tile and keep
 * the tile's frames unpadded from fr[0] */
__device__ __forceinline__ int fidx(int i) { return i + (i >> 5); }
template <bool EX> __device__ __forceinline__ int fidx_t(int i) { return EX ? fidx(i) : i; }

/* DPP reads of another lane's value (v_mov_b32_dpp, no LDS): row_shr:n inside the 16-lane rows, row_bcast:15 /
 * row_bcast:31 from a row's last lane into the following row(s), wave_shr:1 across the whole wave.  Lanes
 * without a source (or outside row_mask) read 0. */
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp0(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, ROW_MASK, 0xf, true));
}
constexpr int DPP_ROW_SHR = 0x110, DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143, DPP_WAVE_SHR1 = 0x138;


/* Channel level (fmd_batch_run_device_levels): the lane's sums over its valid decimated outputs (m0 + r < tm: the short last tile of a
 * ragged block), s1 = sum of (I + Q), s2 = sum of (I^2 + Q^2), in one fixed order.  Whole tiles (tm is wave-uniform) skip the masks. */
__device__ __forceinline__ void tile_level_sums(const f2 (&y)[8], int m0, int tm, float &s1, float &s2) {
  float a = 0.f, q = 0.f;
  if (tm == TW) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
      a += y[r].x; a += y[r].y;
      q = __builtin_fmaf(y[r].x, y[r].x, q); q = __builtin_fmaf(y[r].y, y[r].y, q);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const float i = m0 + r < tm ? y[r].x : 0.f, j = m0 + r < tm ? y[r].y : 0.f;
      a += i; a += j;
      q = __builtin_fmaf(i, i, q); q = __builtin_fmaf(j, j, q);
    }
  }
  s1 = a; s2 = q;
}

/* Sum over the wave, complete in lane 63, in a fixed order (DPP, no LDS): quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror and
 * row_mirror leave the row's sum in every lane of the row; row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3. */
__device__ __forceinline__ float wave_sum_lane63(float x) {
  x += dpp0<0xb1>(x);
  x += dpp0<0x4e>(x);
  x += dpp0<0x141>(x);
  x += dpp0<0x140>(x);
  x += dpp0<DPP_ROW_BCAST15, 0xa>(x);
  x += dpp0<DPP_ROW_BCAST31, 0xc>(x);
  return x;
}
