"""Models of the MPX subcarrier receiver (include/fmdemod_mi355x.h, "MPX subcarrier receiver"), shared by
tests/test_subc_cpu.py and tests/test_gpu_subc.py.

For one stream, v[n] = its samples since the last reset (zero before), T taps h, decimation D, rate R, centre frequency fc:

    z[m] = 2 * sum_{k=0}^{T-1} h[k] * v[mD + D-1-k] * exp(-2 pi i * ((mD + D-1-k) * fc mod R) / R)

Three forms.  subc_f64: the definition in float64, given float taps and the exact carrier.  subc_f32: the same with the float-rounded carrier
table, one rounding for v * c, one for the product with the tap and one per addition, summed in the order of k.  subc_bound: what the kernel's
documented arithmetic may differ from subc_f64 by, per output and per component (derived in DESIGN.md section 5c):

    (T + 4) * 2^-24 * 2 * sum_k |h[k]| |v[mD + D-1-k]|  +  2^-149

All three take the carried state (phase = sample count mod Pd, hist = the last T samples, oldest first) and return the state after the call, so
a run can be split exactly as the device's."""
import math

import numpy as np

U = 2.0 ** -24          # unit roundoff of float32

# (rate, fc, bw, T, D, M) at the edges of the range fmdk_subc_check admits (tests/test_gpu_subc_edges.py; the CPU companions in tests/test_subc_cpu.py)
EDGE_SHAPES = [(204800, 57050, 2400, 64, 8, 512),       # Pd = 4096, the largest admitted; bias = Pd
               (171000, 57000, 2400, 32, 4, 256),       # Pd = 3: the table index wraps inside every 4-sample word
               (228000, 57000, 2400, 16, 4, 4100),      # Pd = 4; a second chunk of 4 samples = one output at D = 4
               (300000, 19000, 500, 256, 32, 4128),     # a ragged chunk of one output at D = 32 whose history is the whole tail of the chunk before
               (192000, 57000, 2400, 16, 4, 16),        # M = T = 16, the smallest block
               (300000, 57000, 2400, 32, 32, 32),       # M = D = T: one output per block
               (300000, 19000, 500, 256, 4, 256)]       # the longest filter at the smallest decimation: 64 tap groups, four outputs per thread
RAGGED_ONE_OUTPUT = [EDGE_SHAPES[2], EDGE_SHAPES[3]]    # the last chunk of a block holds exactly D samples


def period(rate, fc):
    return rate // math.gcd(fc, rate)


def design(rate, bw, n_taps):
    """fmd_subc_design's formula in float64 (not rounded): Blackman-windowed sinc, -6 dB at bw, unit DC gain"""
    k = np.arange(n_taps, dtype=np.float64)
    s = np.sinc(2.0 * bw * (k - (n_taps - 1) / 2.0) / rate) * (0.42 - 0.5 * np.cos(2 * np.pi * (k + 1) / (n_taps + 1))
                                                                   + 0.08 * np.cos(4 * np.pi * (k + 1) / (n_taps + 1)))
    return s / s.sum()


def carrier_exact(rate, fc, n0, n):
    """2 exp(-2 pi i ((j fc) mod R) / R) for the sample counts j = n0 .. n0 + n - 1, complex128; the phase is integer arithmetic"""
    j = np.arange(n0, n0 + n, dtype=np.int64)
    return 2.0 * np.exp(-2j * np.pi * ((j * fc) % rate).astype(np.float64) / rate)


def carrier_table_f32(rate, fc):
    """the host's table: Pd entries in double, rounded once; (re float32 [Pd], im float32 [Pd])"""
    c = carrier_exact(rate, fc, 0, period(rate, fc))
    return c.real.astype(np.float32), c.imag.astype(np.float32)


def _extended(v, hist, n_taps, dtype):
    """the T history samples (zeros without a state), then v"""
    h = np.zeros(n_taps, dtype=dtype) if hist is None else np.asarray(hist, dtype=dtype)[:n_taps]
    assert h.size == n_taps
    return np.concatenate([h, np.asarray(v, dtype=dtype)])


def _next_state(v, hist, n_taps, phase, rate, fc):
    ext = _extended(v, hist, n_taps, np.float32)
    return (phase + len(v)) % period(rate, fc), ext[ext.size - n_taps:].copy()


def subc_f64(v, taps, rate, fc, decim, phase=0, hist=None):
    """the definition: z complex128 [len(v) / D], and the state (phase, hist float32 [T]) after v"""
    taps = np.asarray(taps, dtype=np.float64)
    T, D = taps.size, decim
    assert len(v) % D == 0
    n_out = len(v) // D
    x = _extended(v, hist, T, np.float64)
    # extended index e <-> sample count phase - T + e (mod Pd); before the reset the samples are zero, whatever the carrier there
    u = x * carrier_exact(rate, fc, phase - T + period(rate, fc) * (T // period(rate, fc) + 1), x.size)
    z = np.zeros(n_out, dtype=np.complex128)
    m = np.arange(n_out) * D + D - 1 + T
    for k in range(T):
        z += taps[k] * u[m - k]
    return z, _next_state(v, hist, T, phase, rate, fc)


def subc_f32(v, taps, rate, fc, decim, phase=0, hist=None):
    """float32 throughout, the float-rounded table, sequential sum over k; z complex64, and the state after v"""
    taps = np.asarray(taps, dtype=np.float32)
    T, D, pd = taps.size, decim, period(rate, fc)
    assert len(v) % D == 0
    n_out = len(v) // D
    x = _extended(v, hist, T, np.float32)
    cr, ci = carrier_table_f32(rate, fc)
    idx = (phase - T + pd * (T // pd + 1) + np.arange(x.size)) % pd
    ur, ui = x * cr[idx], x * ci[idx]
    assert ur.dtype == np.float32
    zr, zi = np.zeros(n_out, dtype=np.float32), np.zeros(n_out, dtype=np.float32)
    m = np.arange(n_out) * D + D - 1 + T
    for k in range(T):
        zr = zr + taps[k] * ur[m - k]
        zi = zi + taps[k] * ui[m - k]
    assert zr.dtype == np.float32
    return (zr + 1j * zi).astype(np.complex64), _next_state(v, hist, T, phase, rate, fc)


def subc_bound(v, taps, decim, hist=None):
    """per output (the same for re and im): (T + 4) 2^-24 * 2 sum_k |h[k]| |v[mD + D-1-k]| + 2^-149, float64 [len(v) / D]"""
    taps = np.abs(np.asarray(taps, dtype=np.float64))
    T, D = taps.size, decim
    n_out = len(v) // D
    x = np.abs(_extended(v, hist, T, np.float64))
    a = np.zeros(n_out)
    m = np.arange(n_out) * D + D - 1 + T
    for k in range(T):
        a += taps[k] * x[m - k]
    return (T + 4) * U * 2.0 * a + 2.0 ** -149


def bound_share(got, z64, bound):
    """the largest |got - z64| / bound over outputs and both components"""
    got = np.asarray(got).astype(np.complex128)
    e = got - z64
    return float(max((np.abs(e.real) / bound).max(), (np.abs(e.imag) / bound).max()))


def run_blocks(fn, v, block, taps, rate, fc, decim, phase=0, hist=None):
    """fn (subc_f64 / subc_f32) over v block by block with the carried state; (z concatenated, state)"""
    out = []
    for a in range(0, len(v), block):
        z, (phase, hist) = fn(v[a:a + block], taps, rate, fc, decim, phase, hist)
        out.append(z)
    return np.concatenate(out), (phase, hist)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------

def lcg_floats(n, seed):
    """n floats in +-pi from a 32-bit LCG (the top 24 bits of each state), float32"""
    out = np.empty(n, dtype=np.uint32)
    a = int(seed)
    for i in range(n):
        a = (a * 1664525 + 1013904223) & 0xffffffff
        out[i] = a
    return (((out >> 8).astype(np.float64) / 2.0 ** 23 - 1.0) * np.pi).astype(np.float32)


def tone(n, rate, fc, amp=0.3, phi=0.7, n0=0):
    """A cos(2 pi fc j / R + phi), j = n0 .. n0 + n - 1, float32"""
    j = np.arange(n0, n0 + n, dtype=np.float64)
    return (amp * np.cos(2 * np.pi * fc * j / rate + phi)).astype(np.float32)


def rds_like(rate=300000, n_bits=60, seed=5, phi=0.7):
    """(v float64, bits): n_bits random bits at 1187.5 bit/s as biphase symbols (first half +-1, second half the opposite) on a 57 kHz carrier of
    amplitude 0.03 and phase phi, beside a 19 kHz pilot of 0.157 and a 1 kHz audio tone of 0.5"""
    bits = np.random.default_rng(seed).integers(0, 2, n_bits)
    n = int(n_bits * rate / 1187.5) + 2000
    n -= n % 32
    t = np.arange(n) / rate
    sym = np.floor(t * 1187.5).astype(int)
    frac = t * 1187.5 - sym
    d = np.where(bits[np.minimum(sym, n_bits - 1)] == 1, 1.0, -1.0) * np.where(frac < 0.5, 1.0, -1.0) * (sym < n_bits)
    v = 0.157 * np.cos(2 * np.pi * 19000 * t) + 0.03 * d * np.cos(2 * np.pi * 57000 * t + phi) + 0.5 * np.sin(2 * np.pi * 1000 * t)
    return v, bits


def rds_decode(z, n_bits, rate, n_taps, decim, phi=0.7):
    """bits 1 .. n_bits - 2 from z with the known timing: output m belongs to the instant mD + D-1 - (T-1)/2; first half minus second half"""
    tz = (np.arange(z.size) * decim + decim - 1 - (n_taps - 1) / 2.0) / rate
    s = np.floor(tz * 1187.5).astype(int)
    f = tz * 1187.5 - s
    r = (z * np.exp(-1j * phi)).real
    return np.array([int(r[(s == i) & (f < 0.5)].sum() - r[(s == i) & (f >= 0.5)].sum() > 0) for i in range(1, n_bits - 1)])
