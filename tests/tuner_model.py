"""Models of the channel tuner (include/fmdemod_mi355x.h, "Channel tuner"), shared by tests/test_tuner_cpu.py and
tests/test_gpu_tuner.py.  A helper, not a test.

For one source, n = the sample count since the last reset (samples before it are the VALUE zero), P the table's period, T real taps h:

    x[n] = ((I - 127.5) + j (Q - 127.5)) / 128
    m[n] = x[n] c[((n mod P) shift) mod P],   c[p] = exp(+2 pi i p / P)
    y[n] = sum_{k<T} h[k] m[n-k]
    code = clamp(rint(fma(G, y, 127.5f)), 0, 255) per component, G = float(128 gain)

Three forms.  tuner_f64: the definition in float64 with the exact carrier, given float taps.  tuner_f32: the device's documented arithmetic - the
float-rounded table made from the first octant, one rounded product and one fused multiply-add per mixed component, fused multiply-adds in the order
of k from zero.  tuner_bound: what that arithmetic may differ from tuner_f64 by, per output and per component (derived in DESIGN.md section 5e):

    (T + 6) 2^-24 sum_k |h[k]| (|xr| + |xi|)[n-k]  +  2^-149

All take the carried state of a source - (count = sample count mod P, hist = the last T byte pairs uint8 [T, 2], or None after a reset) - and return
the state after the call, so a run can be split exactly as the device's.  A float32 fused multiply-add is made from float64 operations with the
sum rounded to odd (fma32), which is exact: 53 bits hold the product, and a sum rounded to odd in 53 bits rounds to the nearest float."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32
CHUNK = 4096            # samples per workgroup of the device kernel (csrc/tuner.inc)


# ---- arithmetic ------------------------------------------------------------------------------------------------------------------------------

def fma32(a, b, c):
    """round_to_float32(a * b + c), exactly, for float32 arrays a, b, c"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b                                           # exact: 48 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                     # TwoSum: p + c = s + err exactly
    s, err = np.atleast_1d(s).copy(), np.atleast_1d(err)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))      # inexact: the neighbour with the odd last bit
    return s.astype(np.float32).reshape(np.shape(p + c))


def design(rate, bw, n_taps):
    """fmd_tuner_design's formula in float64 (not rounded): fmd_subc_design's Blackman-windowed sinc with R = rate, -6 dB at bw, unit DC gain"""
    k = np.arange(n_taps, dtype=np.float64)
    s = np.sinc(2.0 * bw * (k - (n_taps - 1) / 2.0) / rate) * (0.42 - 0.5 * np.cos(2 * np.pi * (k + 1) / (n_taps + 1))
                                                                   + 0.08 * np.cos(4 * np.pi * (k + 1) / (n_taps + 1)))
    return s / s.sum()


def table_exact(P):
    return np.exp(2j * np.pi * np.arange(P, dtype=np.float64) / P)


def table_f32(P):
    """the host's table (fmd_resolve.c, fmdk_tuner_table): every entry from an angle of the first octant by symmetry, in double, rounded once;
    (re float32 [P], im float32 [P]); exactly 1, i, -1, -i at the quarter periods"""
    assert P % 4 == 0
    q = P // 4
    p = np.arange(P)
    quad, r = p // q, p % q
    first = 2 * r <= q
    ang = 2.0 * np.pi * np.where(first, r, q - r).astype(np.float64) / P
    c = np.where(first, np.cos(ang), np.sin(ang)).astype(np.float32)
    s = np.where(first, np.sin(ang), np.cos(ang)).astype(np.float32)
    re = np.select([quad == 0, quad == 1, quad == 2], [c, -s, -c], s) + np.float32(0)
    im = np.select([quad == 0, quad == 1, quad == 2], [s, c, -s], -c) + np.float32(0)
    return re.astype(np.float32), im.astype(np.float32)


def shift_steps(rate, step_hz, offset_hz, offset_tuning):
    """fmd_tuner_shift: the steps, or None where the shift is not on the grid"""
    hz = (0 if offset_tuning else -(rate // 4)) - offset_hz
    if (not offset_tuning and rate % 4) or hz % step_hz or abs(2 * offset_hz) > rate:
        return None
    return hz // step_hz


def samples(iq, dtype=np.float64):
    """(xr, xi) of u8 [2 n]; exact in either type"""
    u = np.asarray(iq, dtype=np.uint8).astype(dtype)
    return (u[0::2] - dtype(127.5)) / dtype(128), (u[1::2] - dtype(127.5)) / dtype(128)


def _extended(iq, hist, T, dtype):
    """(xr, xi) of the T history samples (zero values without a state), then iq's"""
    xr, xi = samples(iq, dtype)
    if hist is None:
        hr, hi = np.zeros(T, dtype), np.zeros(T, dtype)
    else:
        h = np.asarray(hist, dtype=np.uint8).reshape(-1)[:2 * T]
        assert h.size == 2 * T
        hr, hi = samples(h, dtype)
    return np.concatenate([hr, xr]), np.concatenate([hi, xi])


def _next_state(iq, hist, T, count, P):
    iq = np.asarray(iq, dtype=np.uint8)
    n = iq.size // 2
    assert n >= T
    return (count + n) % P, iq[2 * (n - T):].reshape(T, 2).copy()


def _index(count, T, n, P, shift, wrap=True):
    """the table index of the extended samples: sample count count - T + e, e = 0 .. T + n - 1"""
    j = (count - T + P * (T // P + 1) + np.arange(T + n, dtype=np.int64)) % P
    return (j * (shift % P)) % P if wrap else j * (shift % P)


def tuner_f64(iq, taps, P, shift, count=0, hist=None):
    """the definition: y complex128 [n], and the state (count, hist) after iq"""
    taps = np.asarray(taps, dtype=np.float64)
    T = taps.size
    xr, xi = _extended(iq, hist, T, np.float64)
    n = xr.size - T
    m = (xr + 1j * xi) * table_exact(P)[_index(count, T, n, P, shift)]
    y = np.zeros(n, dtype=np.complex128)
    e = np.arange(n) + T
    for k in range(T):
        y += taps[k] * m[e - k]
    return y, _next_state(iq, hist, T, count, P)


def tuner_f32(iq, taps, P, shift, count=0, hist=None):
    """the documented float32 arithmetic: y complex64 [n], and the state after iq"""
    taps = np.asarray(taps, dtype=np.float32)
    T = taps.size
    xr, xi = _extended(iq, hist, T, np.float32)
    n = xr.size - T
    cr, ci = table_f32(P)
    idx = _index(count, T, n, P, shift)
    cr, ci = cr[idx], ci[idx]
    mr = fma32(xr, cr, -(xi * ci))
    mi = fma32(xr, ci, xi * cr)
    if hist is None:                                    # before the reset: the value zero, whatever the carrier
        mr[:T] = 0
        mi[:T] = 0
    yr, yi = np.zeros(n, np.float32), np.zeros(n, np.float32)
    e = np.arange(n) + T
    for k in range(T):
        yr = fma32(np.full(n, taps[k], np.float32), mr[e - k], yr)
        yi = fma32(np.full(n, taps[k], np.float32), mi[e - k], yi)
    return (yr + 1j * yi).astype(np.complex64), _next_state(iq, hist, T, count, P)


def tuner_bound(iq, taps, hist=None):
    """per output (the same for re and im): (T + 6) 2^-24 sum_k |h[k]| (|xr| + |xi|)[n-k] + 2^-149, float64 [n]"""
    taps = np.abs(np.asarray(taps, dtype=np.float64))
    T = taps.size
    xr, xi = _extended(iq, hist, T, np.float64)
    a = np.abs(xr) + np.abs(xi)
    n = a.size - T
    s = np.zeros(n)
    e = np.arange(n) + T
    for k in range(T):
        s += taps[k] * a[e - k]
    return (T + 6) * U * s + 2.0 ** -149


def gain_f32(gain):
    return np.float32(np.float32(128.0) * np.float32(gain))


def quantise_f32(y, gain):
    """the device's quantiser on float32 values (complex64 [n]) -> u8 [2 n], I and Q interleaved"""
    y = np.asarray(y, dtype=np.complex64)
    g = np.full(y.size, gain_f32(gain), np.float32)
    half = np.full(y.size, 127.5, np.float32)
    out = np.empty(2 * y.size, np.uint8)
    out[0::2] = np.clip(np.rint(fma32(g, y.real.astype(np.float32), half)), 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.rint(fma32(g, y.imag.astype(np.float32), half)), 0, 255).astype(np.uint8)
    return out


def codes_f64(y64, gain):
    """(codes u8 [2 n], v float64 [2 n]): the float64 model's codes and its pre-rounding values G y + 127.5, I and Q interleaved"""
    g = float(gain_f32(gain))
    v = np.empty(2 * y64.size, np.float64)
    v[0::2] = g * y64.real + 127.5
    v[1::2] = g * y64.imag + 127.5
    return np.clip(np.rint(v), 0, 255).astype(np.uint8), v


def boundary_distance(v):
    """distance of a pre-rounding value from the nearest point where the code changes: 0.5, 1.5 .. 254.5 (below 0.5 everything is code 0, above
    254.5 code 255)"""
    k = np.clip(np.floor(v), 0, 254)
    return np.abs(v - (k + 0.5))


def exempt(v, bound, gain):
    """rule 3's exempt set: the model's pre-rounding value lies within G bound + 2^-16 of a boundary (bool [2 n]; bound per output, both components)"""
    return boundary_distance(v) <= float(gain_f32(gain)) * np.repeat(bound, 2) + 2.0 ** -16


def bound_share(got, y64, bound):
    """the largest |got - y64| / bound over outputs and both components"""
    e = np.asarray(got).astype(np.complex128) - y64
    return float(max((np.abs(e.real) / bound).max(), (np.abs(e.imag) / bound).max()))


def run_blocks(fn, iq, block_len, taps, P, shift, count=0, hist=None):
    """fn (tuner_f64 / tuner_f32) over iq block by block with the carried state; (y concatenated, state)"""
    out = []
    for a in range(0, len(iq), block_len):
        y, (count, hist) = fn(iq[a:a + block_len], taps, P, shift, count, hist)
        out.append(y)
    return np.concatenate(out), (count, hist)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------

def tone_bytes(n_bytes, tones, n0=0, seed=3, dither=True):
    """u8 IQ of sum_i amp_i exp(2 pi i f_i n) (f in cycles per sample), n = n0 .., +-0.5 LSB uniform dither (or none) before the rounding to bytes"""
    n = np.arange(n0, n0 + n_bytes // 2, dtype=np.float64)
    z = sum(a * np.exp(2j * np.pi * f * n) for a, f in tones)
    d = np.random.default_rng(seed).uniform(-0.5, 0.5, (n.size, 2)) * (1.0 if dither else 0.0)
    out = np.empty(n_bytes, np.uint8)
    out[0::2] = np.clip(np.rint(z.real * 128.0 + 127.5 + d[:, 0]), 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.rint(z.imag * 128.0 + 127.5 + d[:, 1]), 0, 255).astype(np.uint8)
    return out


def quiet_bytes(n_bytes, seed=7):
    return np.random.default_rng(seed).integers(127, 129, n_bytes, dtype=np.uint8)


EMPTY_PASSBAND_SHIFT = 600          # steps of 1 kHz: the DC term of dc_bytes to +600 kHz, far outside +-100 kHz


def dc_bytes(n_bytes, i=100, q=200):
    """a capture that holds nothing but a DC term: every sample (i, q)"""
    return np.tile(np.array([i, q], np.uint8), n_bytes // 2)


def all_values_bytes(n_bytes):
    """every byte value in both components, I ascending and Q descending with a stride coprime to 256"""
    n = np.arange(n_bytes // 2)
    out = np.empty(n_bytes, np.uint8)
    out[0::2] = n % 256
    out[1::2] = (255 - 7 * n) % 256
    return out


def shifted_bytes(iq, shift_hz, rate):
    """the capture iq moved by shift_hz in float64 and requantised (ties to even), u8"""
    xr, xi = samples(iq, np.float64)
    n = np.arange(xr.size, dtype=np.float64)
    z = (xr + 1j * xi) * np.exp(2j * np.pi * ((n * shift_hz) % rate) / rate)
    out = np.empty(2 * xr.size, np.uint8)
    out[0::2] = np.clip(np.rint(z.real * 128.0 + 127.5), 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.rint(z.imag * 128.0 + 127.5), 0, 255).astype(np.uint8)
    return out


def rotate_90_bytes(iq):
    """the reference's rotate_90 byte pattern: (I, Q), (255 - Q, I), (255 - I, 255 - Q), (Q, 255 - I), repeating"""
    a = np.asarray(iq, dtype=np.uint8).reshape(-1, 2).astype(np.int32)
    n = np.arange(a.shape[0]) % 4
    i, q = a[:, 0], a[:, 1]
    out = np.empty_like(a)
    out[:, 0] = np.select([n == 0, n == 1, n == 2], [i, 255 - q, 255 - i], q)
    out[:, 1] = np.select([n == 0, n == 1, n == 2], [q, i, 255 - q], 255 - i)
    return out.astype(np.uint8).reshape(-1)


# ---- the GPU cases of rule 3, fixed here so that tests/test_tuner_cpu.py can hold their exempt share to 1 % ------------------------------------

RATE, STEP, P_DEF = 2400000, 1000, 2400
IN_BAND = ((0.45, 0.29), (0.3, -0.11))      # two tones (amplitude, cycles per sample): +696 kHz and -264 kHz at 2.4 Msps

# (name, kind, T, P, shift, gain, block_len, blocks)
MODEL_CASES = [
    ("lcg T64 g1", "lcg", 64, 2400, -700, 1.0, 2 * (4096 + 24), 3),
    ("lcg T64 g8", "lcg", 64, 2400, -700, 8.0, 2 * (4096 + 24), 3),
    ("lcg T64 +100", "lcg", 64, 2400, 100, 1.0, 512, 3),
    ("lcg T16 small", "lcg", 16, 2400, -700, 1.0, 64, 3),
    ("lcg T20 small", "lcg", 20, 2400, 100, 2.0, 64, 3),             # T no multiple of 8: the history's oldest word is half in use
    ("lcg T16 g8 P4", "lcg", 16, 4, 3, 8.0, 512, 3),
    ("lcg T64 P4096", "lcg", 64, 4096, -1195, 1.0, 2 * (4096 + 24), 3),
    ("tone T64 g1", "tone", 64, 2400, -700, 1.0, 16384, 3),           # the +696 kHz tone to -4 kHz
    ("tone T64 g8", "tone", 64, 2400, -700, 8.0, 2 * (4096 + 24), 3),
    ("tone T16 g1", "tone", 16, 2400, 250, 1.0, 512, 3),              # the -264 kHz tone to -14 kHz
]
N_SOURCES, N_CHANNELS = 2, 5


def case_channels(P, shift, gain):
    """the five channels of a case over its two sources, a mixed source map: [(source, shift, gain)]; the neighbours of shift stay in range"""
    up = shift + 1 if shift + 1 < P else shift - 1
    down = shift - 1 if shift - 1 > -P else shift + 1
    return [(0, shift, gain), (1, shift, gain), (1, up, gain), (0, down, gain), (1, shift, gain)]


def case_rate(P):
    return RATE if P == 2400 else P * 1000


def case_taps(T, P):
    """the default design at +-100 kHz of 2.4 Msps (the same fraction of the rate for the other periods), float32"""
    rate = case_rate(P)
    t = design(rate, rate // 24, T).astype(np.float32)
    t.setflags(write=False)
    return t


def case_input(kind, n_bytes, source=0):
    """the input of a case for one source; every source has its own bytes"""
    if kind == "lcg":
        from oracle import lcg_bytes                    # the survey's LCG byte stream
        return lcg_bytes(n_bytes, 12345 + 1000 * source)[0]
    if kind == "tone":
        return tone_bytes(n_bytes, IN_BAND, seed=3 + source)
    if kind == "quiet":
        return quiet_bytes(n_bytes, seed=7 + source)
    raise ValueError(kind)
