/*
 * fmd_kernels.inc - fused IQ -> PCM kernel for gfx950 (MI355X).
 *
 * Execution model: ONE WAVEFRONT IS ONE WORKER.  A worker owns one time chunk of
 * one stream and walks it tile by tile (FMDK_TILE rate_in samples = 8 x as many
 * IQ samples) through every stage of the reference's chain; the 64 lanes split
 * each tile (8 consecutive outputs per lane).  Workers never synchronise with
 * each other: there is no workgroup barrier in the tile loop, values cross lanes
 * through wave shuffles or through the worker's private slice of LDS (DS
 * operations of one wave execute in order).  A CU holds 12 such workers (three
 * per SIMD), so while one waits on LDS / HBM another issues arithmetic.  The wave
 * index is made scalar, so everything derived from it lives in SGPRs.
 *
 * A stream's launch is cut into n_chunks chunks of whole tiles so that any
 * stream count fills the chip.  A chunk that does not start the launch replays
 * warm_tiles tiles before its first tile from zero state and discards their
 * output: all histories are finite (FIRs) or contract below fp32 resolution
 * (de-emphasis), so its first real sample sees the state a sequential run has.
 *
 * HBM traffic is the algorithmic minimum: u8 IQ is read once (each lane loads
 * the 176 bytes its 8 outputs need as eleven 16-byte buffer loads, one tile ahead
 * of use; the 48-byte overlap between neighbouring lanes is served by L1), int16 PCM is
 * written once; decimated IQ stays in registers, discriminator / MPX filter
 * outputs / resampled frames live in the worker's LDS slice.
 *
 * Stages per tile (reference src/rtl_fm_player.c):
 *   A  u8 -> f32, j^n rotation, 32-tap /8 FIR        :195-239, :253-411
 *   B  polynomial-atan2 FM discriminator             :606-685
 *   Q  block-start overwrite quirk (stereo)          :534-598 (SURVEY.md s.0 Q1)
 *   C  three 90-tap MPX FIRs + 38 kHz carrier        :533-568, :472-481
 *   D  rational resampler, second FIR at emit times  :570-598 (stereo), :500-532 (mono)
 *   F  de-emphasis, f32 -> s16, PCM store (when the frame buffer fills or a
 *      block ends)                                   :687-735
 *
 * This file is included by fmd_kernels_exact.hip (the EX instantiations), fmd_kernels_fast.hip (MX = 0) and fmd_kernels_mfma.hip (MX >= 1):
 * the three translation units differ only in which instantiations they own, so that they compile in parallel (all with the same flags,
 * without the SLP vectoriser, whose packing costs moves and registers: the packed arithmetic of the hot loops is written by hand).
 * The code lives in the files included below, one per stage:
 *   k_common.inc    constants, the worker's LDS slice, arithmetic helpers        stage_c.inc     MPX filters + carrier (vector ALU; int8 matrix pipe)
 *   stage_a.inc     tile loads, the /8 decimator (vector ALU; int8 matrix pipe)  stage_d.inc     second-stage low-pass at the emit instants (vector ALU; matrix pipe)
 *   stage_b.inc     discriminator                                                 cold_paths.inc  quirk Q1, head fix, carrier redo
 *   flush.inc       de-emphasis, s16, PCM store                                   kernel.inc      the fused kernel and its launch templates
 *
 * Arithmetic contracts (template parameters EX, MX):
 *   exact: the reference's operation order with unfused multiply/add (this
 *          file is compiled with -ffp-contract=off) -> bit-identical PCM;
 *   fast:  same summation order with explicit fused multiply-adds and the
 *          u8 offset folded into the decimator taps -> PCM within +-1 LSB;
 *   fast, MX = 1 (FMD_MATH_FAST_MFMA): stage A on the matrix pipe (v_mfma_i32_16x16x64_i8: exact integer products of the IQ
 *          bytes with fixed-point taps) - any filter size, ragged tiles;
 *   fast, MX = 2 (FMD_MATH_FAST_MFMA_F): every stage that has a matrix form there, in int8-limb fixed point with exact integer sums.  90-tap stereo: the
 *          pilot and L-R filters at full rate (mpx_tile_i8), the L+R channel's two low-passes - fm over the discriminator ring (:545, :560), fm again over
 *          the bm ring at the emit instants (:588) - as ONE 179-tap filter fm * fm, and the second stage of L-R, both at the resampler's emit instants
 *          only (resample_tile_dec: a decimating banded product, 32 MFMAs per tile where the full-rate forms of round 5 took 60).  128-tap mono / narrow
 *          FM: the fm low-pass likewise (resample_mono_dec).  The default where the host finds it applicable (fmd_resolve.c, fmdk_resolve).
 *   (Rounds 4 and 5 had three intermediate families - stage C alone, the second stage at every sample, the composite filter at every sample: retired,
 *   tools/experiments/retired_round5_families.inc.)
 * The path is not memory bound (SURVEY.md section 7) and runs at the package power cap (hwmon beside the bench: DESIGN.md section 5): a stage
 * costs its energy (MFMA i8 on live operands 8 nJ, ds_read_b128 2.1, a plain vector instruction 0.5 - 0.6, a packed one 1.6), and what shortens the kernel is
 * fewer or cheaper operations. The vector-ALU
 * kernels keep the non-FMA instruction count and the LDS traffic per FMA low (8 outputs per lane share
 * one pair-sum; all taps are scalar operands loaded from the kernarg segment; interleaved {L+R, L-R}
 * history so the resampler reads 8-byte pairs), and the matrix pipe - the one unit they leave idle -
 * takes the banded-Toeplitz FIRs whose products can be made exact in int8 limbs.
 */
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstddef>
#include <type_traits>

#include "fmd_internal.h"

#ifndef FMD_BUILD_MFMA
#define FMD_BUILD_MFMA 0
#endif

/* Workers (wavefronts) per SIMD each instantiation is register-budgeted for: the __launch_bounds__ of fmd_fused_kernel, and what the host cuts time
 * chunks for (fmdk_workers_per_cu).  3 -> 168 VGPRs, 2 -> 256.  Stereo with stages A and C on the matrix pipe, and generic-size stereo with the
 * stage-A tables (where LDS admits two workgroups per CU anyway), get two; so does the tap-serving build of the mono kernel with stage D on the matrix
 * pipe, whose extra checks do not fit 168 registers.  Everything else gets three. */
constexpr int STEREO_WAVES = 3, MONO_WAVES = 3, MFC_WAVES = 2;
constexpr int waves_of(bool /* ex */, int mode, int half, int mx, bool dbg) {
  if (mode == 2) return ((half == 0 && mx > 0) || mx > 1) ? MFC_WAVES : STEREO_WAVES;
  return (dbg && mx > 1) ? 2 : MONO_WAVES;
}

/* tuning builds only (tools/ablate.sh): bit mask of stages compiled out of the tile loop,
 * 1 = A (decimator), 2 = B (discriminator), 4 = C (MPX), 8 = D (resampler), 16 = F (flush); 32 = the stages after a compiled-out B or C still see LIVE operands
 * (stand-in limbs: an MFMA on zeros costs a third of one on data - profiles/r6b_power_price_live_operands.txt).
 * The results are garbage; the point is the time of what is left. */
#ifndef FMD_ABLATE
#define FMD_ABLATE 0
#endif

namespace {

#include "k_common.inc"
#include "stage_a.inc"
#include "stage_b.inc"
#include "stage_c.inc"
#include "stage_d.inc"
#include "cold_paths.inc"
#include "flush.inc"
#include "kernel.inc"

}  // namespace

/* one launcher per translation unit, over the instantiations it owns (kernel.inc, launch_variant); fmdk_launch picks the unit */
#define FMD_LAUNCH_ARGS const fmdk_params *p, const fmdk_variant *v, int n_streams, const void *d_iq, void *d_pcm, void *d_lens, \
                        const void *d_state_in, void *d_state_out, const fmd_debug_taps *dbg, void *d_lv_part, void *hip_stream, void *ev0, void *ev1
#define FMD_LAUNCH_PASS p, v, n_streams, d_iq, d_pcm, d_lens, d_state_in, d_state_out, dbg, d_lv_part, hip_stream, ev0, ev1
#if FMD_BUILD_EXACT
extern "C" int fmdk_launch_exact(FMD_LAUNCH_ARGS) { return launch_variant<true, 0>(FMD_LAUNCH_PASS); }
#elif FMD_BUILD_MFMA
extern "C" int fmdk_launch_mfma(FMD_LAUNCH_ARGS) { return launch_variant<false, 1>(FMD_LAUNCH_PASS); }
#else
extern "C" int fmdk_launch_exact(FMD_LAUNCH_ARGS);
extern "C" int fmdk_launch_mfma(FMD_LAUNCH_ARGS);
extern "C" int fmdk_launch(FMD_LAUNCH_ARGS) {
  if (v->ex) return fmdk_launch_exact(FMD_LAUNCH_PASS);
  if (v->mx) return fmdk_launch_mfma(FMD_LAUNCH_PASS);
  return launch_variant<false, 0>(FMD_LAUNCH_PASS);
}

/* Tiles a replaying chunk must walk before its first real tile.  FIR memories:
 * 24 IQ + 1 (discriminator) + 2 x (size - 1) rate_in samples; the de-emphasis
 * restart needs (warm + group) frames = that many x fast / slow rate_in samples.
 * The last tile of a block may be short, so count tiles against the worst case. */
extern "C" int fmdk_warm_tiles(const fmdk_params *p, const fmdk_variant *v) {
  const bool fast = !v->ex;
  /* FIR histories: 24 IQ words (3 samples), the discriminator's previous sample, size - 1 samples of the first filter stage and -
   * stereo only - size - 1 of the second (mono and mode 0 have one stage: counting two cost the 128-tap mono kernels a second
   * replayed tile per chunk, 25 % of a one-block launch) */
  long long need = 8 + (long long)p->size * ((p->resample && p->mode == 2) ? 2 : 1);
  if (fast) need += 3;                           /* decimate8_own: the first three outputs of a replay lack the words before it */
  if (p->deemph) {
    if (p->warm >= (1 << 20)) return 0;          /* non-contracting recurrence: never split */
    if (fast) {
      /* +-1 LSB contract: the state a chunk starts from only has to be right to 1e-9 of full
       * scale (warm_fast frames), and the blocked flush needs no 16-frame alignment */
      need += p->resample ? ((long long)p->warm_fast * p->fast + p->slow - 1) / p->slow : p->warm_fast;
    } else {
      need += ((long long)p->warm + DEEMPH_GROUP) * (p->resample ? (p->fast + p->slow - 1) / p->slow : 1);
    }
  }
  const long long M = p->block_len >> 4, tpb = (M + TW - 1) / TW;
  const long long full = (need + TW - 1) / TW;
  if (M % TW == 0) return (int)full;
  if (full + 1 <= tpb) return (int)(full + 1);     /* at most one short tile inside the replay */
  return (int)(((need + M - 1) / M + 1) * tpb);    /* whole blocks */
}

extern "C" int fmdk_tile(void) { return TW; }

/* The host's worker budget next to the kernel's (waves_of): 4 SIMDs x the workers per SIMD, except where the chunk counts were measured against a
 * different number and are kept as they are (bringing either into line is a speed change of its own):
 *   - generic-size stereo with stage A on the matrix pipe is built for two workers per SIMD, and cut for three;
 *   - the tap-serving mono build with stage D on the matrix pipe is built for two, and cut for three like the build without taps. */
extern "C" int fmdk_workers_per_cu(const fmdk_variant *v, int dbg, int *kernel_per_simd) {
  const int kernel = waves_of(v->ex, v->mode, v->half, v->mx, dbg);
  if (kernel_per_simd) *kernel_per_simd = kernel;
  if (v->mode == 2 && v->half == 0 && v->mx == 1) return 4 * STEREO_WAVES;
  if (dbg && v->mode != 2 && v->mx > 1) return 4 * MONO_WAVES;
  return 4 * kernel;
}
#endif
