/* stage_b.inc - part of the fused IQ -> PCM kernel (included by fmd_kernels.inc inside its anonymous namespace; not a translation unit of its own).
 * Stage B: the polynomial-atan2 FM discriminator (reference :606-685), exact and eight-at-a-time fast forms. */

/* ---- stage B: discriminator --------------------------------------------- */

template <bool EX>
__device__ __forceinline__ float discriminate(float pr, float pj, float re, float im, float &cr, float &dt) {
  if constexpr (EX) {
    cr = pr * im - pj * re;          /* pre_r * Q - pre_j * I */
    dt = re * pr + im * pj;          /* I * pre_r + Q * pre_j */
  } else {
    cr = __builtin_fmaf(pr, im, -(pj * re));
    dt = __builtin_fmaf(re, pr, im * pj);
  }
  return poly_atan2<EX>(cr, dt);
}
template <bool EX>
__device__ __forceinline__ float discriminate(float pr, float pj, float re, float im) {
  float cr, dt;
  return discriminate<EX>(pr, pj, re, im, cr, dt);
}

/* Fast kernels: the lane's eight discriminator outputs with packed arithmetic where two values share an
 * instruction - (dot, cross) of one sample as a packed multiply and multiply-add on the (I, Q) pair, the
 * polynomial of src/rtl_fm_player.c:607-667 on two samples at a time - and two running minima that tell
 * the caller whether any of the eight needs the exact redo:
 *   vmax       largest |result|: next to the +-pi branch cut - |cross| < 8e-5 |dot| with a negative dot product, where a
 *              rounding difference flips 2 pi - the result is +-(pi - r0) with r0 = 1.03 |cross / dot| < 8.3e-5, so
 *              vmax >= pi - 8.4e-5 is a superset of those samples (one v_max3 per two samples; the margin itself, 8e-5 dot +
 *              |cross| <= 0, cost a multiply-add and half a minimum per sample);
 *   dmin       smallest max(|cross|, |dot|), within sqrt 2 of the product of the two magnitudes: a sample
 *              next to the origin (ill-conditioned phase) makes it small; the caller looks closer. */
__device__ __forceinline__ void discriminate8_fast(float pr, float pj, const f2 (&y2)[8], f8 &v, float &vmax,
                                                   float &dmin) {
  f2 prev = {pr, pj};
  f8 a, r0, sgn_x, xmajf;
  float x[8], y[8];
  bool xmaj[8];
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const f2 cur = y2[r];
    /* (dot, cross) = (I pr + Q pj, Q pr - I pj) */
    const f2 dc = pk_dotcross(cur, prev);
    x[r] = dc.x;
    y[r] = dc.y;
    const float ax = __builtin_fabsf(dc.x), ay = __builtin_fabsf(dc.y);
    xmaj[r] = ax >= ay;
    const float num = min_abs(dc.x, dc.y);       /* hipcc builds the select from two v_and and a v_cndmask */
    const float den = __builtin_fmaxf(__builtin_fmaxf(ax, ay), 1e-37f);
    a[r] = num * __builtin_amdgcn_rcpf(den);
    dmin = __builtin_fminf(dmin, den);
    prev = cur;
  }
  (void)sgn_x; (void)xmajf;
  /* (packed: one sample per instruction measured -0.2 % stereo, nothing for mono, and spills in the 168-register mono kernels -
   * profiles/r6w_scalar_vs_packed_ab.txt) */
#pragma unroll
  for (int r = 0; r < 8; r += 2) {
    const f2 a2 = {a[r], a[r + 1]};
    const f2 q2 = __builtin_elementwise_fma(f2{0.0663f, 0.0663f}, a2, f2{0.2447f, 0.2447f});
    const f2 w2 = __builtin_elementwise_fma(-(a2 - 1.f), q2, f2{K_PI_4, K_PI_4});
    const f2 p2 = a2 * w2;
    r0[r] = p2.x;
    r0[r + 1] = p2.y;
  }
#pragma unroll
  for (int r = 0; r < 8; r += 2) {
    f2 base, t;
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const float r0x = __builtin_copysignf(r0[r + e], x[r + e]);
      const float b = xmaj[r + e] ? ((x[r + e] < 0.f) ? K_PI : 0.f) : K_PI_2;
      const float tt = xmaj[r + e] ? r0x : -r0x;
      if (e == 0) { base.x = b; t.x = tt; } else { base.y = b; t.y = tt; }
    }
    const f2 th = base + t;
    /* theta >= 0 (base is 0, pi/2 or pi and |t| <= pi/4 with the sign that keeps it so): the result is theta with
     * the sign of y, one v_bfi.  y == -0 differs from the reference's `y < 0` only next to the branch cut (x < 0),
     * which vmax sends to the exact redo, or where theta is 0. */
    v[r] = __builtin_copysignf(th.x, y[r]);
    v[r + 1] = __builtin_copysignf(th.y, y[r + 1]);
    vmax = __builtin_fmaxf(vmax, __builtin_fmaxf(th.x, th.y));      /* theta >= 0 */
  }
}

