"""Stereo control (fmd_stereo_*; include/fmdemod_mi355x.h, "Stereo control"; csrc/stereo.inc) in numpy, operation for operation: every float
operation is one float32 operation with one rounding, fma32 the fused multiply-add (exact product in float64, the sum corrected for the second
rounding), `/` numpy's correctly rounded float32 division, rint ties to even.  The device is held to this model bit for bit.

Also here, so that tests/test_stereo_cpu.py and tests/test_gpu_stereo.py speak of the same bytes: the inputs of the GPU cases (CASES, case_inputs)
and the planted defects (DEFECTS) the CPU file shows to change the model's output on exactly those inputs."""
import numpy as np

E_ARG, E_UNSUPPORTED, E_NODEVICE, E_STATE = -1, -2, -5, -6
AUTO, FORCE_MONO, FORCE_STEREO = 0, 1, 2
NT = 256
F32 = np.float32

INFO_DTYPE = np.dtype([("pilot_ms", "<f4"), ("g_start", "<f4"), ("g_step", "<f4"), ("g_end", "<f4"), ("stereo", "<i4"), ("frames", "<i4"),
                       ("reserved", "<i4", (2,))])
METER_DTYPE = np.dtype([("peak_l", "<i4"), ("peak_r", "<i4"), ("full_scale", "<i4"), ("frames", "<i4"), ("sumsq_l", "<u8"), ("sumsq_r", "<u8")])
DEFECTS = ("ramp_end", "ramp_wrong_block", "ties_away", "sign_s", "meter_input", "ignore_hold", "drop_last")


class Refused(Exception):
    def __init__(self, status, why):
        super().__init__(why)
        self.status = status


def config(pcm_stride=1024, pilot_per_block=64, hold_blocks=2, pilot_on=0.1, pilot_off=0.05, blend_lo=10.0, blend_hi=20.0, slew=0.5,
           reserved0=0, reserved=(0, 0, 0)):
    return dict(pcm_stride=int(pcm_stride), pilot_per_block=int(pilot_per_block), hold_blocks=int(hold_blocks), reserved0=int(reserved0),
                pilot_on=F32(pilot_on), pilot_off=F32(pilot_off), blend_lo=F32(blend_lo), blend_hi=F32(blend_hi), slew=F32(slew),
                reserved=tuple(int(r) for r in reserved))


def plan(c):
    """the range of the header and the four derived floats (fmdk_stereo_plan), each made in double and rounded once"""
    if c["reserved0"] or any(c["reserved"]):
        raise Refused(E_ARG, "reserved")
    if not (8 <= c["pcm_stride"] <= 65536) or c["pcm_stride"] % 8:
        raise Refused(E_UNSUPPORTED, "pcm_stride")
    if not (0 <= c["pilot_per_block"] <= 65536):
        raise Refused(E_UNSUPPORTED, "pilot_per_block")
    if not (1 <= c["hold_blocks"] <= 1 << 20):
        raise Refused(E_ARG, "hold_blocks")
    on, off, lo, hi, slew = (c[k] for k in ("pilot_on", "pilot_off", "blend_lo", "blend_hi", "slew"))
    if not (np.isfinite(on) and np.isfinite(off) and off > 0 and off <= on):
        raise Refused(E_ARG, "pilot thresholds")
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise Refused(E_ARG, "blend range")
    if not (slew > 0 and slew <= 1):
        raise Refused(E_ARG, "slew")
    mz = c["pilot_per_block"]
    with np.errstate(over="ignore"):
        return dict(thr_on=F32(np.float64(on) * np.float64(on)), thr_off=F32(np.float64(off) * np.float64(off)),
                    inv_mz=F32(1.0 / mz) if mz > 0 else F32(0), inv_span=F32(1.0 / (np.float64(hi) - np.float64(lo))))


def fma32(a, b, c):
    """round_to_float32(a b + c) with ONE rounding, elementwise.  The product of two float32 is exact in float64; the float64 sum s carries an error
    e (two-sum).  Rounding s instead of s + e differs only where s is exactly half way between two float32: there e decides."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        r = s.astype(np.float32)
        d = s - r.astype(np.float64)
        other = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = (d != 0) & np.isfinite(s) & ((r.astype(np.float64) + other.astype(np.float64)) * 0.5 == s) & (e != 0)
        away = tie & ((e > 0) == (d > 0))               # the exact value lies beyond the half-way point, on the other neighbour's side
        return np.where(away, other, r).astype(np.float32)


def clamp(x, lo, hi):
    x = np.asarray(x, dtype=np.float32)
    return np.where(x < lo, F32(lo), np.where(x > hi, F32(hi), x)).astype(np.float32)


# ---- 1. the pilot meter --------------------------------------------------------------------------------------------------------------------

def pilot_ms(z, inv_mz, defect=None):
    """z float32 [Mz, 2] (re, im) of one (stream, block): thread t sums p = fma(zi, zi, zr zr) over t, t + 256, ... from zero, the tree
    a[t] += a[t + h], h = 128 .. 1, then a[0] inv_mz"""
    z = np.asarray(z, dtype=np.float32).reshape(-1, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        p = fma32(z[:, 1], z[:, 1], z[:, 0] * z[:, 0])
        rows = -(-max(p.size, 1) // NT)
        pp = np.zeros(rows * NT, dtype=np.float32)       # a thread without an element adds nothing: + (+0) leaves a sum of squares as it is
        pp[:p.size] = p
        a = np.zeros(NT, dtype=np.float32)
        for row in pp.reshape(rows, NT)[:-(-p.size // NT)]:
            a = a + row
        if defect == "drop_last":
            a[NT - 1] = 0
        h = NT // 2
        while h >= 1:
            a[:h] = a[:h] + a[h:2 * h]
            h //= 2
        return F32(a[0] * F32(inv_mz))


def pilot_ms_f64(z):
    z = np.asarray(z, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    return float((z * z).sum() / z.shape[0])


def pilot_bound(mz, exact):
    """two roundings in p, the thread's run of ceil(Mz / 256) additions, 8 tree levels, inv_mz and the product with it"""
    return (-(-mz // NT) + 12) * 2.0 ** -24 * exact + 2.0 ** -126


# ---- 2. the tracker --------------------------------------------------------------------------------------------------------------------------

def new_state():
    return dict(g=F32(0), stereo=0, run=0)


def track(c, pl, state, lens, pilot, quality, mode, defect=None):
    """one stream, the blocks of one launch in order.  pilot: float32 [B] (the meter's pilot_ms) or None (no d_z); quality float32 [B] or None.
    Returns (info [B] of INFO_DTYPE, the state after)."""
    B = len(lens)
    info = np.zeros(B, dtype=INFO_DTYPE)
    g, stereo, run = F32(state["g"]), int(state["stereo"]), int(state["run"])
    hold = 1 if defect == "ignore_hold" else c["hold_blocks"]
    slew = c["slew"]
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(B):
            frames = min(max(int(lens[b]), 0), c["pcm_stride"]) // 2
            q = F32(pilot[b]) if pilot is not None else F32(0)
            g0 = g
            if frames > 0 and mode == AUTO and pilot is not None:
                want = int(bool(q >= pl["thr_off"])) if stereo else int(bool(q >= pl["thr_on"]))
                if want != stereo:
                    run += 1
                    if run >= hold:
                        stereo, run = want, 0
                else:
                    run = 0
            step = F32(0)
            if frames > 0:
                if mode == FORCE_MONO:
                    target = F32(0)
                elif mode == FORCE_STEREO:
                    target = F32(1)
                elif not stereo:
                    target = F32(0)
                elif quality is None:
                    target = F32(1)
                else:
                    t = F32(F32(F32(quality[b]) - c["blend_lo"]) * pl["inv_span"])
                    target = (t if t < 1 else F32(1)) if t > 0 else F32(0)
                d = F32(target - g)
                d = -slew if d < -slew else (slew if d > slew else d)
                g = F32(g + d)
                g = F32(0) if g < 0 else (F32(1) if g > 1 else g)
                step = F32(F32(g - g0) / F32(frames))
            info[b] = (q, g0, step, g, stereo, frames, (0, 0))
    return info, dict(g=g, stereo=stereo, run=run)


# ---- 3. apply and meters -----------------------------------------------------------------------------------------------------------------------

def apply(slot, rec, defect=None, g_start=None):
    """slot int16 [pcm_stride] (L, R interleaved), rec one INFO_DTYPE record -> (out int16 [pcm_stride], one METER_DTYPE record)"""
    slot = np.asarray(slot, dtype=np.int16)
    n = int(rec["frames"])
    out = slot.copy()
    L, R = slot[0:2 * n:2].astype(np.float32), slot[1:2 * n:2].astype(np.float32)
    g0 = F32(rec["g_start"] if g_start is None else g_start)
    gi = clamp(fma32(np.arange(1, n + 1, dtype=np.float32), rec["g_step"], g0), 0, 1)
    if defect == "ramp_end":
        gi = np.full(n, rec["g_end"], dtype=np.float32)
    m, s = F32(0.5) * (L + R), F32(0.5) * (L - R)
    if defect == "sign_s":
        s = -s
    x = [fma32(gi, s, m).astype(np.float64), fma32(-gi, s, m).astype(np.float64)]
    if defect == "ties_away":
        y = [np.trunc(v + np.copysign(0.5, v)) for v in x]
    else:
        y = [np.rint(v) for v in x]
    lo, ro = (np.clip(v, -32768, 32767).astype(np.int64) for v in y)
    out[0:2 * n:2] = lo.astype(np.int16)
    out[1:2 * n:2] = ro.astype(np.int16)
    if defect == "meter_input":
        lo, ro = slot[0:2 * n:2].astype(np.int64), slot[1:2 * n:2].astype(np.int64)
    meter = np.zeros((), dtype=METER_DTYPE)
    meter["peak_l"] = np.abs(lo).max() if n else 0
    meter["peak_r"] = np.abs(ro).max() if n else 0
    meter["full_scale"] = sum(int(((v == -32768) | (v == 32767)).sum()) for v in (lo, ro))
    meter["frames"] = n
    meter["sumsq_l"] = int((lo * lo).sum())
    meter["sumsq_r"] = int((ro * ro).sum())
    return out, meter


def run(c, states, pcm, lens, pilot, quality, mode=AUTO, defect=None):
    """a launch: pcm int16 [S, B, stride], lens [S, B], pilot float32 [S, B] or None, quality float32 [S, B] or None, states a list of S state
    dicts (replaced by the states after).  Returns (out, info [S, B], meter [S, B])."""
    pl = plan(c)
    S, B = lens.shape
    out = np.zeros_like(pcm)
    info = np.zeros((S, B), dtype=INFO_DTYPE)
    meter = np.zeros((S, B), dtype=METER_DTYPE)
    for s in range(S):
        info[s], states[s] = track(c, pl, states[s], lens[s], None if pilot is None else pilot[s], None if quality is None else quality[s], mode,
                                   defect)
        for b in range(B):
            wrong = info[s, b - 1]["g_start"] if (defect == "ramp_wrong_block" and b > 0) else None
            out[s, b], meter[s, b] = apply(pcm[s, b], info[s, b], defect, wrong)
    return out, info, meter


# ---- the inputs of the GPU cases ---------------------------------------------------------------------------------------------------------------

BOUNDARY = (-32768, -32767, -1, 0, 1, 32766, 32767)


def lcg_u32(n, seed):
    """n values of x -> 1664525 x + 1013904223 mod 2^32"""
    out, x = [], int(seed)
    for _ in range(n):
        x = (x * 1664525 + 1013904223) & 0xffffffff
        out.append(x)
    return np.array(out, dtype=np.uint32)


def boundary_pairs():
    """int16 [49, 2]: every (L, R) of BOUNDARY x BOUNDARY"""
    return np.array([(a, b) for a in BOUNDARY for b in BOUNDARY], dtype=np.int16)


def lcg_pcm(S, B, stride, seed=1):
    """int16 [S, B, stride], read-only: the 49 boundary pairs, then the high halves of an LCG, cut into slots one after another - so the pairs land
    in block 0 of stream 0 and, at small strides, in the blocks and streams behind it; every slot is full to its end (what lies beyond lens shows
    when it is not copied)"""
    n = S * B * stride
    bp = boundary_pairs().reshape(-1)
    rnd = (lcg_u32(max(n - bp.size, 0), seed) >> np.uint32(16)).astype(np.uint16).view(np.int16)
    a = np.concatenate([bp, rnd])[:n].reshape(S, B, stride).copy()
    a.setflags(write=False)
    return a


def pilot_z(S, B, mz, amps, seed=5):
    """float32 [S, B, mz, 2], read-only: unit-modulus phases from an LCG times amps[s][b] (1 + up to 10 % ripple): mean |z|^2 near amps^2"""
    u = lcg_u32(S * B * mz * 2, seed).astype(np.float64) / 2.0 ** 32
    ph, rip = u[0::2].reshape(S, B, mz), u[1::2].reshape(S, B, mz)
    r = np.asarray(amps, dtype=np.float64).reshape(S, B, 1) * (1.0 + 0.1 * (rip - 0.5))
    z = np.stack([r * np.cos(2 * np.pi * ph), r * np.sin(2 * np.pi * ph)], axis=-1).astype(np.float32)
    z.setflags(write=False)
    return z


HI, MID, LO = 0.15, 0.07, 0.01          # pilot amplitudes: above pilot_on = 0.1, between pilot_off = 0.05 and pilot_on, below pilot_off

# name: (config keywords, S, B, lens per block (cycled over streams with a shift), pilot amplitudes per block, quality per block)
# quality against blend_lo 10, blend_hi 20: 25 -> 1, 14 -> 0.4, 5 -> 0, 17.5 -> 0.75
CASES = {
    # g through 0 -> 1 -> 0.4 -> 0 -> 1: hold 1, slew 1, so every block ends on its target
    "sweep":      (dict(pcm_stride=1024, pilot_per_block=64, hold_blocks=1, slew=1.0), 3, 5, (1024, 1000, 1024, 514, 1024), (HI, HI, LO, HI, HI), (25.0, 14.0, 25.0, 25.0, 30.0)),
    # hold 2 and slew 0.5: on at block 1, the dip to MID keeps it, fractional targets approached in steps
    "hold":       (dict(pcm_stride=1032, pilot_per_block=257, hold_blocks=2, slew=0.5), 3, 5, (1032, 1032, 1030, 1032, 700), (HI, HI, MID, HI, LO), (25.0, 25.0, 17.5, 14.0, 25.0)),
    "one_block":  (dict(pcm_stride=1024, pilot_per_block=255, hold_blocks=1, slew=0.75), 1, 1, (1024,), (HI,), (25.0,)),
    "tiny":       (dict(pcm_stride=8, pilot_per_block=1, hold_blocks=1, slew=0.5), 3, 5, (0, 1, 2, 7, 8), (HI, HI, HI, HI, HI), (25.0, 25.0, 14.0, 25.0, 25.0)),
    "two_pass":   (dict(pcm_stride=2056, pilot_per_block=300, hold_blocks=1, slew=0.6), 1, 2, (2056, 2050), (HI, HI), (25.0, 17.5)),
    "odd_lens":   (dict(pcm_stride=1024, pilot_per_block=16, hold_blocks=1, slew=0.5), 1, 5, (5000, -3, 1024, 0, 1023), (HI, HI, HI, LO, HI), (25.0, 25.0, 17.5, 25.0, 14.0)),
}


def case_inputs(name, stride=None):
    """(config dict, pcm, lens, z, quality) of a named case; stride: another pcm_stride (the real batch's), the lens scaled to it"""
    kw, S, B, lens, amps, qual = CASES[name]
    kw = dict(kw)
    scale = 1
    if stride is not None:
        scale, kw["pcm_stride"] = stride / kw["pcm_stride"], stride
    c = config(**kw)
    ln = np.array([[int(lens[(b + s) % len(lens)] * scale) if s else int(lens[b] * scale) for b in range(B)] for s in range(S)], dtype=np.int32)
    am = np.array([[amps[(b + 2 * s) % len(amps)] if s == 2 else amps[b] for b in range(B)] for s in range(S)])
    qu = np.array([[qual[(b + s) % len(qual)] for b in range(B)] for s in range(S)], dtype=np.float32)
    return c, lcg_pcm(S, B, c["pcm_stride"], seed=len(name)), ln, pilot_z(S, B, c["pilot_per_block"], am, seed=3 + len(name)), qu
