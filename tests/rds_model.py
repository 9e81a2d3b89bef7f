"""Models of the RDS receiver (include/fmdemod_mi355x.h, "RDS receiver"), shared by tests/test_rds_cpu.py and
tests/test_gpu_rds.py, and the synthesiser both feed it from.

For one stream z[n] = its samples since the last reset (zero before), rate_z Hz, S = 2 rate_z / 2375 samples per bit, Tg real taps g:

    y[n]  = sum_k g[k] z[n-k]                                                  matched filter
    Tm_b  = sum_{n in block b} |y[n]|^2 w[n mod Pw],  w[i] = exp(-2 pi i ((i 2375) mod 2 rate_z) / (2 rate_z))
    Ts_b  = a Ts_{b-1} + Tm_b, a = 1 - 1/avg_blocks;   phi_b = -arg(Ts_b) / (2 pi) in [-1/2, 1/2)
    block b (first sample n0) owns the bits k >= 0 with n0 - L <= k S < n0 + Bz - L         (integers: Geometry)
    s(k)  = y interpolated linearly at (k + phi_b) S;  c_k = Re(s(k) conj(s(k-1)));  c_k < 0 is data bit 1

receive(..., dtype=np.float64) is the definition; dtype=np.float32 is the same in float32 with the float-rounded table (its own error against the
float64 form is the yardstick for phi).  Both carry a State, so a run can be split exactly as the device's.  The bounds (y_bound, tm_bound,
soft_bound) are what the kernels' documented arithmetic may differ from the float64 form by; DESIGN.md section 5d derives them."""
import functools
import math

import numpy as np

import subc_model as SM

U = 2.0 ** -24          # unit roundoff of float32
Q = 2375                # 2 fb
FB = 1187.5
OFFSETS = {"A": 0x0FC, "B": 0x198, "C": 0x168, "C'": 0x350, "D": 0x1B4}
POLY = 0x5B9            # x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1

# ((rate_z, Tg, Bz), blocks, streams) at the edges of the range fmdk_rds_check admits (tests/test_gpu_rds_edges.py; the CPU companions in
# tests/test_rds_cpu.py)
EDGE_SHAPES = [((38000, 64, 68), 12, 3),        # S = 32, Hy = 66 of a 68-sample block, Pw = 32, 2 or 3 bits per block
               ((37875, 64, 128), 12, 3),       # Pw = 606, S = 31.89
               ((37875, 16, 68), 12, 3),        # the shortest filter with the longest lookback
               ((11875, 16, 2816), 3, 3),       # S = 10, Pw = 10, 281 / 282 bits per block (slot 284); 3 chunks, the last ragged (768)
               ((12000, 32, 4096), 3, 3),       # 405 / 406 bits per block, 4 whole chunks
               ((18750, 64, 65536), 2, 1),      # 64 chunks, 4150 bits per block
               ((38000, 64, 65536), 2, 1)]      # count 2048 = slot: nothing to zero


class Geometry:
    """the integers of the definition (fmdk_rds_geometry)"""

    def __init__(self, rate_z, block_z):
        self.rate_z, self.bz = rate_z, block_z
        self.two_rz = 2 * rate_z
        self.pw = self.two_rz // math.gcd(Q, self.two_rz)
        self.hh = -(-rate_z // Q)               # ceil(S / 2)
        self.lb = self.hh + 2                   # L
        self.hb = -(-self.two_rz // Q)          # ceil(S)
        self.hy = self.lb + self.hb + self.hh
        self.slot = (-(-Q * block_z // self.two_rz) + 3) & ~3
        self.S = self.two_rz / Q


class State:
    """phase = sample count mod Pw; e = 2375 x (next bit's instant - (n0 - L)) in [0, 2 rate_z); bit = next bit's index; ts; the last Tg z and
    the last Hy y (oldest first).  The device's fmd_rds_state.frac is e - 2375 L."""

    def __init__(self, geo, n_taps, dtype=np.float64):
        c = np.complex128 if dtype == np.float64 else np.complex64
        self.phase, self.e, self.bit, self.ts = 0, Q * geo.lb, 0, c(0)
        self.zhist, self.yhist = np.zeros(n_taps, dtype=c), np.zeros(geo.hy, dtype=c)

    def copy(self):
        o = State.__new__(State)
        o.__dict__.update(self.__dict__)
        o.zhist, o.yhist = self.zhist.copy(), self.yhist.copy()
        return o


def pulse_h(t):
    """the shaped impulse (t in bit periods): inverse transform of cos(pi f Td / 4) on |f| <= 2 / Td, up to a constant"""
    return np.sinc(4.0 * t + 0.5) + np.sinc(4.0 * t - 0.5)


def pulse(t):
    """the biphase bit pulse centred on t = 0 (t in bit periods): +impulse at -Td/4, -impulse at +Td/4, shaped"""
    return pulse_h(t + 0.25) - pulse_h(t - 0.25)


def design(rate_z, n_taps):
    """fmd_rds_design's formula in float64 (not rounded)"""
    k = np.arange(n_taps, dtype=np.float64)
    p = pulse(((n_taps - 1) / 2.0 - k) * FB / rate_z)
    return p / (p * p).sum()


def table_exact(geo, idx):
    idx = np.asarray(idx, dtype=np.int64)
    return np.exp(-2j * np.pi * ((idx * Q) % geo.two_rz).astype(np.float64) / geo.two_rz)


def matched_filter(z, taps, zhist, dtype=np.float64):
    """y [len(z)] in the order k = 0 .. Tg-1 from zero (float32: one rounding per product and per sum - the device fuses them)"""
    c = np.complex128 if dtype == np.float64 else np.complex64
    taps = np.asarray(taps, dtype=dtype)
    T = taps.size
    x = np.concatenate([np.asarray(zhist, dtype=c), np.asarray(z, dtype=c)])
    n = np.arange(len(z)) + T
    yr, yi = np.zeros(len(z), dtype=dtype), np.zeros(len(z), dtype=dtype)
    for k in range(T):
        yr = yr + taps[k] * x.real[n - k]
        yi = yi + taps[k] * x.imag[n - k]
    assert yr.dtype == dtype
    return (yr + 1j * yi).astype(c)


def block_counts(geo, e, n_blocks):
    """(first e of each block, counts): ownership in integers"""
    es, counts = [], []
    lim = Q * geo.bz
    for _ in range(n_blocks):
        cnt = -(-(lim - e) // geo.two_rz) if e < lim else 0
        es.append(e)
        counts.append(cnt)
        e = e + cnt * geo.two_rz - lim
    return es, counts, e


def slice_block(geo, yext, e, count, phi, dtype=np.float64):
    """soft bits of one block.  yext = the Hy values of y before the block's first sample, then the block's.  phi as given (a float32 value from
    the device, or the model's own).  float32: the device's operations - frac = r * fl(1/2375), u = fma(phi, S, frac), weight u - floor(u),
    s = fma(mu, y1 - y0, y0), c = fma(si, pi, sr pr) - with unfused float32 sums standing in for the fused ones."""
    if count == 0:
        return np.zeros(0, dtype=dtype)
    j = np.arange(count, dtype=np.int64)
    s = []
    for m in (0, 1):
        E = e + Q * geo.hb + (j - m) * geo.two_rz
        assert E.min() >= 0
        q, r = E // Q, E % Q
        if dtype == np.float64:
            u = float(phi) * (geo.two_rz / Q) + r / Q
        else:
            u = np.float32(phi) * np.float32(geo.two_rz / Q) + r.astype(np.float32) * np.float32(1.0 / 2375.0)
            assert u.dtype == np.float32
        fl = np.floor(u)
        mu = (u - fl).astype(dtype)
        idx = np.clip(q + fl.astype(np.int64) + geo.hh, 0, geo.hy + geo.bz - 2)
        y0, y1 = yext[idx], yext[idx + 1]
        s.append((y0.real + mu * (y1.real - y0.real)) + 1j * (y0.imag + mu * (y1.imag - y0.imag)))
    c = s[0].real * s[1].real + s[0].imag * s[1].imag
    return c.astype(dtype)


def receive(z, geo, taps, avg_blocks=8, state=None, dtype=np.float64, phi_given=None, mutate=None):
    """z complex [n_blocks * Bz] of one stream -> dict(y, tm [nb], ts [nb], phi [nb], pw [nb], first [nb], counts [nb], soft [list of arrays]) and
    the State after.  phi_given [nb]: slice with these phases (the device's own) instead of the model's.  mutate: a dict that plants one defect
    (tests/test_rds_cpu.py, "teeth")."""
    c = np.complex128 if dtype == np.float64 else np.complex64
    mutate = mutate or {}
    taps = np.asarray(taps, dtype=dtype).copy()
    if "zero_tap" in mutate:
        taps[mutate["zero_tap"]] = 0
    T, bz = taps.size, geo.bz
    st = State(geo, T, dtype) if state is None else state.copy()
    z = np.asarray(z, dtype=c)
    assert z.size % bz == 0
    nb = z.size // bz
    a = dtype(1.0 - 1.0 / avg_blocks)
    out = dict(y=[], tm=[], ts=[], phi=[], pw=[], first=[], counts=[], soft=[])
    phi_prev = dtype(0)
    for b in range(nb):
        zb = z[b * bz:(b + 1) * bz]
        zh = st.zhist
        if mutate.get("late_history") == b:
            zh = np.concatenate([[0], zh[:-1]])                          # the history one sample late at this block's edge
        y = matched_filter(zb, taps, zh, dtype)
        widx = st.phase + np.arange(bz)
        if mutate.get("held_w") == b:
            widx = widx - bz                                             # the table index held across the block before
        w = table_exact(geo, widx % geo.pw)
        p = (y.real * y.real + y.imag * y.imag).astype(dtype)
        if dtype == np.float32:
            wr, wi = w.real.astype(np.float32), w.imag.astype(np.float32)
            tm = np.complex64(np.sum(p * wr, dtype=np.float32) + 1j * np.sum(p * wi, dtype=np.float32))
        else:
            tm = np.sum(p * w)
        st.ts = c(a * st.ts.real + tm.real + 1j * (a * st.ts.imag + tm.imag))
        phi = dtype(-np.arctan2(dtype(st.ts.imag), dtype(st.ts.real)) * dtype(0.15915494309189535))
        if not phi < 0.5 or phi < -0.5:
            phi = dtype(-0.5)
        use = phi if phi_given is None else phi_given[b]
        lim = Q * bz
        e = st.e
        if mutate.get("own_off") == b:
            e = e + geo.two_rz                                           # ownership off by one bit at this block's edge: its first bit is skipped
        cnt = -(-(lim - e) // geo.two_rz) if e < lim else 0
        yext = np.concatenate([st.yhist, y])
        soft = slice_block(geo, yext, e, cnt, use, dtype)
        if mutate.get("wrong_phi") == b and cnt:                          # s(k-1) of the block's first bit with the block before's phase
            s0 = _sample(geo, yext, e, use)
            s1 = _sample(geo, yext, e - geo.two_rz, phi_prev)
            soft = soft.copy()
            soft[0] = (s0 * np.conj(s1)).real
        phi_prev = use
        out["y"].append(y); out["tm"].append(tm); out["ts"].append(st.ts); out["phi"].append(phi); out["pw"].append(p.sum(dtype=dtype))
        out["first"].append(st.bit); out["counts"].append(cnt); out["soft"].append(soft)
        st.bit += cnt
        st.e = e + cnt * geo.two_rz - lim
        st.phase = (st.phase + bz) % geo.pw
        st.zhist = np.concatenate([st.zhist, zb])[-T:]
        st.yhist = yext[-geo.hy:]
    for k in ("tm", "ts", "phi", "pw", "first", "counts"):
        out[k] = np.array(out[k])
    out["y"] = np.concatenate(out["y"])
    return out, st


def _sample(geo, yext, e, phi):
    """s of the bit whose instant is e (float64)"""
    E = e + Q * geo.hb
    u = float(phi) * (geo.two_rz / Q) + (E % Q) / Q
    fl = math.floor(u)
    idx = min(max(E // Q + fl + geo.hh, 0), geo.hy + geo.bz - 2)
    return yext[idx] + (u - fl) * (yext[idx + 1] - yext[idx])


# ---- bounds ----------------------------------------------------------------------------------------------------------

def y_bound(z, taps, zhist):
    """(bound of re, bound of im) per output: (Tg + 4) 2^-24 sum_k |g[k]| |z[n-k]| + 2^-149, with that component of z"""
    taps = np.abs(np.asarray(taps, dtype=np.float64))
    T = taps.size
    x = np.concatenate([np.asarray(zhist, dtype=np.complex128), np.asarray(z, dtype=np.complex128)])
    n = np.arange(len(z)) + T
    ar, ai = np.zeros(len(z)), np.zeros(len(z))
    for k in range(T):
        ar += taps[k] * np.abs(x.real[n - k])
        ai += taps[k] * np.abs(x.imag[n - k])
    return (T + 4) * U * ar + 2.0 ** -149, (T + 4) * U * ai + 2.0 ** -149


def tm_bound(y64, by_r, by_i, bz):
    """per block and component.  p = |y|^2: the device's y is off by (by_r, by_i), so p by dp <= 2 |yr| by_r + 2 |yi| by_i + by^2, plus two roundings
    (gamma_2 p); each term p w carries the table's rounding, the fma's and at most RD_RO - 1 + 8 + chunks additions of the thread's run, the
    256-thread tree and the tracker's sum over chunks: sum_n [dp + (14 + chunks) u p] (|w| <= 1), and 2^-126 for sums that underflow."""
    nb = y64.size // bz
    p = np.abs(y64) ** 2
    dp = 2 * np.abs(y64.real) * by_r + 2 * np.abs(y64.imag) * by_i + by_r ** 2 + by_i ** 2 + 2 * U * p
    chunks = -(-bz // 1024)
    per = dp * (1 + 16 * U) + (14 + chunks) * U * p
    return per.reshape(nb, bz).sum(axis=1) + 2.0 ** -126


def soft_bound(geo, yext64, byext, e, count, phi):
    """per bit of one block, against slice_block(float64) with the same phi.  byext: the bound of each value of yext (the larger component's).
    The instant u is off by du <= 4 u (S/2 + 2) (the rounded S and 1/2375, the product, the fma); across an index boundary the interpolant is
    continuous, so s moves by at most du x the steepest of the neighbouring segments.  s = y0 + mu (y1 - y0): by0 (1 - mu) + by1 mu <= max by,
    plus 3 roundings on |y0| + |y1 - y0|.  c = sr pr + si pi: |ds| |p| + |dp| |s| + |ds| |dp| and 2 roundings of |s| |p|; 2^-126 for underflow."""
    if count == 0:
        return np.zeros(0)
    j = np.arange(count, dtype=np.int64)
    du = 4 * U * (geo.S / 2 + 2)
    mag, err = [], []
    top = geo.hy + geo.bz - 2
    for m in (0, 1):
        E = e + Q * geo.hb + (j - m) * geo.two_rz
        u = float(phi) * geo.S + (E % Q) / Q
        fl = np.floor(u)
        mu = u - fl
        idx = np.clip(E // Q + fl.astype(np.int64) + geo.hh, 0, top)
        lo, hi = np.clip(idx - 1, 0, top), np.clip(idx + 1, 0, top)
        seg = lambda i: np.abs(yext64[i + 1] - yext64[i])  # noqa: E731
        steep = np.maximum(seg(idx), np.maximum(seg(lo), seg(hi)))
        y0, y1 = yext64[idx], yext64[idx + 1]
        s = y0 + mu * (y1 - y0)
        by = np.maximum(byext[idx], byext[idx + 1])
        ds = np.sqrt(2.0) * by + du * steep + 3 * U * (np.abs(y0) + np.abs(y1 - y0)) * np.sqrt(2.0)
        mag.append(np.abs(s))
        err.append(ds)
    return err[0] * mag[1] + err[1] * mag[0] + err[0] * err[1] + 3 * U * mag[0] * mag[1] + 2.0 ** -126


# ---- RDS data: groups, checkwords, bits ----------------------------------------------------------------------------------------------------------

def rem26(word):
    for i in range(25, 9, -1):
        if word & (1 << i):
            word ^= POLY << (i - 10)
    return word & 0x3FF


def block_bits(info, offset):
    """the 26 bits of a block, first transmitted first: 16 information bits, then checkword + offset word"""
    w = (info << 10) | (rem26(info << 10) ^ offset)
    return [(w >> (25 - i)) & 1 for i in range(26)]


def group_bits(blocks, version_b=False):
    offs = [OFFSETS["A"], OFFSETS["B"], OFFSETS["C'"] if version_b else OFFSETS["C"], OFFSETS["D"]]
    return [b for info, o in zip(blocks, offs) for b in block_bits(info, o)]


def ps_groups(pi, ps, pty=10, n=None, version_b=False):
    """0A (0B) groups that spell the 8-character name ps, segment 0 first, n groups in all (default 4); block C of a 0A group carries AF filler"""
    ps = (ps + " " * 8)[:8].encode("latin-1")
    out = []
    for i in range(n or 4):
        seg = i & 3
        b = (0 << 12) | (int(version_b) << 11) | (pty << 5) | seg
        out.append((pi, b, pi if version_b else 0xE0E0 + i, (ps[2 * seg] << 8) | ps[2 * seg + 1]))
    return out


def data_bits(groups, version_b=False):
    return np.array([b for g in groups for b in group_bits(g, version_b)], dtype=np.int64)


def soft_of_bits(bits):
    """ideal soft bits: -1 for a 1"""
    return np.where(np.asarray(bits) == 1, -1.0, 1.0).astype(np.float32)


# ---- synthesiser -----------------------------------------------------------------------------------------------------------------------------------

def baseband(bits, rate, n, t0=3.0, ppm=0.0):
    """the biphase-shaped baseband of the data bits (differentially encoded here) at `rate`, n samples, float64: bit k's pulse is centred on
    (k + t0) Td (1 + ppm 1e-6)"""
    d = np.bitwise_xor.accumulate(np.asarray(bits, dtype=np.int64))       # d_k = b_k xor d_{k-1}
    amp = np.where(d == 1, 1.0, -1.0)
    tb = np.arange(n) * (FB / rate) / (1.0 + ppm * 1e-6)                  # time in bit periods
    x = np.zeros(n)
    span = 4.0
    for k in range(len(d)):
        lo = max(int((k + t0 - span) * rate / FB * (1.0 + ppm * 1e-6)), 0)
        hi = min(int((k + t0 + span) * rate / FB * (1.0 + ppm * 1e-6)) + 2, n)
        if lo < hi:
            x[lo:hi] += amp[k] * pulse(tb[lo:hi] - (k + t0))
    return x


def mpx(bits, rate, n, level=0.04, phase=0.7, pilot=0.157, audio=0.3, t0=3.0, ppm=0.0):
    """an FM multiplex as the discriminator hands it out: a 19 kHz pilot, a 1 kHz audio tone and the RDS baseband on 57 kHz, float64 [n]"""
    t = np.arange(n) / rate
    return (pilot * np.cos(2 * np.pi * 19000 * t) + audio * np.sin(2 * np.pi * 1000 * t)
            + level * baseband(bits, rate, n, t0, ppm) * np.cos(2 * np.pi * 57000 * t + phase))


def groups_of(n, pi=0x1234, ps="RADIO 42"):
    """n groups: 0A groups that spell ps, every third one a 2A-like group with running contents so that no two groups are equal"""
    name = ps_groups(pi, ps, n=4)
    out = []
    for i in range(n):
        if i % 3 == 2:
            out.append((pi, 0x2000 | (10 << 5) | (i & 15), 0x4100 + i, 0x6100 + 7 * i))
        else:
            g = name[(i - i // 3) & 3]
            out.append((g[0], g[1], 0xE000 + i, g[3]))
    return out


@functools.lru_cache(maxsize=None)
def synth_z(rate_z, S, n, n_groups=4):
    """complex64 [S, n], read-only: the float64 subcarrier model's z of a synthesised multiplex at 16 rate_z (n_groups groups of data, silence after
    them), every stream its own data, level, carrier phase and bit timing"""
    rate = 16 * rate_z
    out = []
    for s in range(S):
        bits = data_bits(groups_of(n_groups, 0x1000 + s, "STREAM %d" % s))
        v = mpx(bits, rate, 16 * n, level=0.03 + 0.01 * s, phase=0.7 + s, t0=1.0 + 0.37 * s)
        z, _ = SM.subc_f64(v, SM.design(rate, 2400, 128).astype(np.float32), rate, 57000, 16)
        out.append(z.astype(np.complex64))
    a = np.stack(out)
    a.setflags(write=False)
    return a


def groups_to_fill(rate_z, n):
    """the number of groups whose bits last for n samples of z and a little longer"""
    return int(n * Q / (2 * rate_z)) // 104 + 2


def lcg_complex(n, seed):
    """n complex64 values with parts in +-1 from a 32-bit LCG"""
    out = np.empty(2 * n, dtype=np.uint32)
    a = int(seed)
    for i in range(2 * n):
        a = (a * 1664525 + 1013904223) & 0xffffffff
        out[i] = a
    f = ((out >> 8).astype(np.float64) / 2.0 ** 23 - 1.0).astype(np.float32)
    return (f[0::2] + 1j * f[1::2]).astype(np.complex64)
