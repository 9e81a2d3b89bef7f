"""The IQ -> PCM chain in float64, one function per stage (test infrastructure, plain numpy).

Written from oracle/fm_oracle.c: the same formulas and the same float32 CONSTANTS (the pi family, the polynomial's
coefficients, the filter taps, swf / cwf, lambda, volume x 32768), widened to double; every operation in double.  The
taps are never redesigned here (numpy's sin is not libm's sinf): callers pass the float32 values of fmd_design_taps or
of the oracle (fmo_get_taps).

Each function takes the UPSTREAM stage's values as given, so an implementation's stage X can be judged on what it does
to the input it actually received (tests/stage_budget.py):

    decimate(iq_bytes, tb_history, offset_tuning, fb)  -> y          (stage_convert + stage_decimate)
    discriminate(y, pre)                               -> v          (poly_atan2, stage_discriminate)
    mpx(v, state, cfg, taps)                           -> frames, state   (stage_resample, modes 0 / 1 / 2)
    deemph_to_s16(frames, state, cfg)                  -> t, pcm     (stage_deemph + stage_to_s16; t before clip and round)

cfg is anything with the fields of fmo_config / fmd_config (rate_out, rate_out2, mode, size, deemph, deemph_lambda,
volume, offset_tuning); state is a MpxState / DeemphState carried from block to block in float64.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

F32 = np.float32
PI = float(F32(3.14159265))      # FMO_PI
PI_2 = float(F32(1.5707963))     # FMO_PI_2
PI_4 = float(F32(0.78539816))    # FMO_PI_4
C1 = float(F32(0.2447))
C2 = float(F32(0.0663))


# ---------------------------------------------------------------- stage A

def convert(iq_bytes, offset_tuning):
    """u8 -> (i - 127.5) / +-128 with the j^n rotation (stage_convert); exact in float32 and in double."""
    b = np.asarray(iq_bytes, dtype=np.uint8).astype(np.float64)
    p = (b - 127.5) / 128.0
    if offset_tuning:
        return p
    assert b.size % 8 == 0
    n = -p
    c = np.empty_like(p)
    c[0::8], c[1::8] = p[0::8], p[1::8]      # n % 4 == 0:  I,  Q
    c[2::8], c[3::8] = n[3::8], p[2::8]      # n % 4 == 1: -Q,  I
    c[4::8], c[5::8] = n[4::8], n[5::8]      # n % 4 == 2: -I, -Q
    c[6::8], c[7::8] = p[7::8], n[6::8]      # n % 4 == 3:  Q, -I
    return c


def decimate(iq_bytes, tb_history, offset_tuning, fb, return_history=False):
    """32-tap symmetric FIR, decimate by 8: y[m] = sum_k (c[8m-24+k] + c[8m+7-k]) fb[k] per component, c = [24 complex
    of history | block].  tb_history: the 48 floats carried from the block before (None: zeros).  y interleaved I, Q."""
    fb = np.asarray(fb, dtype=np.float64)
    assert fb.size == 16
    tb = np.zeros(48) if tb_history is None else np.asarray(tb_history, dtype=np.float64)
    c = np.concatenate([tb, convert(iq_bytes, offset_tuning)])
    n_y = (c.size - 48) // 16
    h = np.concatenate([fb, fb[::-1]])
    y = np.empty(2 * n_y)
    for comp in (0, 1):
        w = sliding_window_view(c[comp::2], 32)[::8][:n_y]
        y[comp::2] = w @ h
    if return_history:
        return y, c[-48:].copy()
    return y


# ---------------------------------------------------------------- stage B

def poly_atan2(y, x, c1=C1, c2=C2):
    """poly_atan2 of the oracle, vectorised: special cases, the x-major choice and the eight octant expressions."""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    ax, ay = np.abs(x), np.abs(y)
    xneg, yneg = x < 0, y < 0
    x_major = np.where(xneg, np.where(yneg, x <= y, -x >= y), np.where(yneg, x >= -y, x >= y))
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(x_major, ay / ax, ax / ay)
    r0 = a * (PI_4 - (a - 1.0) * (c1 + c2 * a))
    out = np.where(xneg,
                   np.where(yneg, np.where(x_major, r0 - PI, -r0 - PI_2), np.where(x_major, -r0 + PI, PI_2 + r0)),
                   np.where(yneg, np.where(x_major, -r0, r0 - PI_2), np.where(x_major, r0, PI_2 - r0)))
    out = np.where(y == 0, np.where(xneg, PI, 0.0), out)
    out = np.where(x == 0, np.where(yneg, -PI_2, np.where(y > 0, PI_2, 0.0)), out)
    return out


def discriminate(y, pre=(0.0, 0.0), c1=C1, c2=C2):
    """v[m] = poly_atan2(pr im - pj re, re pr + im pj), (pr, pj) = the sample before (pre for m = 0)."""
    y = np.asarray(y, dtype=np.float64)
    re, im = y[0::2], y[1::2]
    pr = np.concatenate([[float(pre[0])], re[:-1]])
    pj = np.concatenate([[float(pre[1])], im[:-1]])
    return poly_atan2(pr * im - pj * re, re * pr + im * pj, c1, c2)


# ---------------------------------------------------------------- stage C / D

class MpxState:
    """br / bm / bs histories (oldest first, `size` values), pp and the resampler accumulator."""

    def __init__(self, size):
        self.br = np.zeros(size)
        self.bm = np.zeros(size)
        self.bs = np.zeros(size)
        self.pp = 0.0
        self.acc = 0

    def copy(self):
        s = MpxState(self.br.size)
        s.br, s.bm, s.bs, s.pp, s.acc = self.br.copy(), self.bm.copy(), self.bs.copy(), self.pp, self.acc
        return s


def full_taps(half_taps, size):
    f = np.asarray(half_taps, dtype=np.float64)[:size // 2]
    return np.concatenate([f, f[::-1]])


def emit_steps(acc, slow, fast, n):
    """Steps i of 0 .. n-1 at which `if ((acc += slow) >= fast) acc -= fast` fires (slow <= fast), and the new acc."""
    assert 0 < slow <= fast
    tot = acc + slow * np.arange(1, n + 1, dtype=np.int64)
    k = tot // fast
    fired = np.diff(np.concatenate([[0], k])) > 0
    return np.flatnonzero(fired), int(tot[-1] - k[-1] * fast) if n else acc


def carrier38(x, y):
    """sin(2 atan(y / x)) = 2 z / (1 + z^2), z = y / x; 0 where x == 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        z = y / x
        c = (z + z) / (1.0 + z * z)
    return np.where(x == 0, 0.0, c)


def _fir(hist, x, h):
    """Window of step i = [hist | x][i+1 .. i+size]; returns the FIR output of every step."""
    return np.correlate(np.concatenate([hist[1:], x]), h, mode="valid")


def mpx(v, state, cfg, taps, c_fir=None):
    """Resampler + MPX decode of one block (stage_resample).  Returns (frames, new state); state is not modified.
    Stereo frames are interleaved L, R.  c_fir: optional replacement (hist, x, h) -> outputs for the FIR of the stereo
    pilot and L-R filters - how tests/stage_budget.py restates a documented fixed-point form of them when it derives
    a budget term; None for the model itself."""
    v = np.array(v, dtype=np.float64)
    n = v.size
    fast, slow, size, mode = int(cfg.rate_out), int(cfg.rate_out2), int(cfg.size), int(cfg.mode)
    st = state.copy()
    if slow <= 0:
        return v, st
    if mode == 0:
        e, st.acc = emit_steps(st.acc, slow, fast, n)
        return v[e], st
    fm = full_taps(taps["fm"], size)
    if mode == 1:
        e, st.acc = emit_steps(st.acc, slow, fast, n)
        out = _fir(st.br, v, fm)[e]
        st.br = np.concatenate([st.br, v])[-size:]
        return out, st
    fp, fs = full_taps(taps["fp"], size), full_taps(taps["fs"], size)
    swf, cwf = float(F32(taps["swf"])), float(F32(taps["cwf"]))
    e, acc1 = emit_steps(st.acc, slow, fast, n)

    def stage_c(vv):
        fc = _fir if c_fir is None else c_fir
        vm, vp, vs = _fir(st.br, vv, fm), fc(st.br, vv, fp), fc(st.br, vv, fs)
        ppv = np.concatenate([[st.pp], vp[:-1]])
        return vm, vp, vs * carrier38(vp * swf, vp * cwf - ppv)

    def stage_d(vm, bs):
        om = _fir(st.bm, vm, fm)[e]
        os_ = _fir(st.bs, bs, fm)[e]
        out = np.empty(2 * e.size)
        out[0::2], out[1::2] = om + os_, om - os_
        return out

    vm, vp, bs = stage_c(v)
    if e.size and e[0] == 0 and n > 1:
        # step 0 emits: R of frame 0 lands on sample 1 before step 1 reads it (the reference works in place)
        v[1] = stage_d(vm, bs)[1]
        vm, vp, bs = stage_c(v)
    out = stage_d(vm, bs)
    st.br = np.concatenate([st.br, v])[-size:]
    st.bm = np.concatenate([st.bm, vm])[-size:]
    st.bs = np.concatenate([st.bs, bs])[-size:]
    st.pp = float(vp[-1])
    st.acc = acc1
    return out, st


# ---------------------------------------------------------------- stage F

class DeemphState:
    def __init__(self, l=0.0, r=0.0):
        self.l, self.r = float(l), float(r)


def _one_pole(x, prev, lam):
    """y[i] = x[i] + lam (y[i-1] - x[i])"""
    from scipy.signal import lfilter
    y, _ = lfilter([1.0 - lam], [1.0, -lam], x, zi=[lam * prev])
    return y


def deemph_to_s16(frames, state, cfg):
    """One-pole de-emphasis, scale by volume x 32768, clip, round half to even.  Returns (t, pcm, new state)."""
    x = np.asarray(frames, dtype=np.float64)
    st = DeemphState(state.l, state.r)
    if int(cfg.deemph) and x.size:
        lam = float(F32(cfg.deemph_lambda))
        if int(cfg.mode) == 2:
            out = np.empty_like(x)
            out[0::2] = _one_pole(x[0::2], st.l, lam)
            out[1::2] = _one_pole(x[1::2], st.r, lam)
            st.l, st.r = float(out[-2]), float(out[-1])
        else:
            out = _one_pole(x, st.l, lam)
            st.l = float(out[-1])
        x = out
    t = x * float(F32(cfg.volume) * F32(32768.0))
    return t, to_s16(t), st


def to_s16(t):
    return np.rint(np.clip(t, -32768.0, 32767.0)).astype(np.int16)


# ---------------------------------------------------------------- the whole chain

def run_chain(iq, block_len, cfg, taps):
    """Every block of iq through the four stages, each fed by the model's own upstream values.  Returns a list of
    dicts y, v, mpx, t, pcm per block."""
    iq = np.asarray(iq, dtype=np.uint8)
    tb, pre, ms, ds = None, (0.0, 0.0), MpxState(int(cfg.size)), DeemphState()
    out = []
    for k in range(iq.size // block_len):
        y, tb = decimate(iq[k * block_len:(k + 1) * block_len], tb, int(cfg.offset_tuning), taps["fb"], return_history=True)
        v = discriminate(y, pre)
        pre = (y[-2], y[-1])
        frames, ms = mpx(v, ms, cfg, taps)
        t, pcm, ds = deemph_to_s16(frames, ds, cfg)
        out.append({"y": y, "v": v, "mpx": frames, "t": t, "pcm": pcm})
    return out
