"""Models of the capture spectrum (fmd_batch_spectrum_device / _host; include/fmdemod_mi355x.h, "Capture spectrum"), written from the definition.
A helper, not a test.

Block of L = block_len / 2 complex samples x[n] = (I - 127.5) / 128 + j (Q - 127.5) / 128 (the reference's u8_f32_table[0], no fs/4 rotation),
N = n_bins, nseg = L // N whole segments from the start of the block, the tail unused:

    P[k] = sum_seg | sum_n w[n] x[seg N + n] exp(-2 pi i k n / N) |^2 / (nseg N sum_n w[n]^2),   k = 0 .. N - 1   (natural FFT order)

spectrum_f64: the definition with np.fft.fft in float64 - the yardstick.
spectrum_f32: the same in float32 throughout (an iterative radix-2 decimation-in-time FFT on complex64, twiddles made in double and rounded
once, power into a float32 accumulator segment by segment, the scale applied once) - what a careful float32 implementation loses, so the size
of error a float32 device kernel may show against the float64 model.
spectrum_bound: the float64 model and, per bin, how far the documented arithmetic of the device kernel (float64 with float tables, one rounding
at the store) can be from it.
spectrum_standin: that arithmetic in numpy - a float64 mixed-radix transform whose window and pass twiddles are rounded to float."""
import numpy as np

WINDOW_RECT = 0
WINDOW_HANN = 1


def window_f64(n_bins, window):
    if window == WINDOW_RECT:
        return np.ones(n_bins, np.float64)
    if window == WINDOW_HANN:
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_bins, dtype=np.float64) / n_bins)      # periodic form
    raise ValueError("unknown window %r" % (window,))


def samples_f64(block_bytes):
    """complex128 [L] from u8 [2 L]"""
    u = np.asarray(block_bytes, dtype=np.uint8).astype(np.float64)
    return ((u[0::2] - 127.5) + 1j * (u[1::2] - 127.5)) / 128.0


def spectrum_f64(block_bytes, n_bins, window):
    x = samples_f64(block_bytes)
    N = int(n_bins)
    nseg = x.size // N
    if nseg < 1:
        raise ValueError("n_bins exceeds the block's samples")
    w = window_f64(N, window)
    X = np.fft.fft(x[:nseg * N].reshape(nseg, N) * w, axis=1)
    return (X.real ** 2 + X.imag ** 2).sum(axis=0) / (nseg * N * (w * w).sum())


def _bit_reverse(n):
    bits = n.bit_length() - 1
    r = np.zeros(n, np.int64)
    for b in range(bits):
        r |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    return r


def fft_f32(x):
    """Radix-2 decimation-in-time FFT of a complex64 vector (power-of-two length), every operation in float32."""
    n = x.size
    a = np.ascontiguousarray(x[_bit_reverse(n)], dtype=np.complex64)
    half = 1
    while half < n:
        tw = np.exp(-2j * np.pi * np.arange(half, dtype=np.float64) / (2 * half)).astype(np.complex64)
        a = a.reshape(-1, 2, half)
        t = (a[:, 1, :] * tw).astype(np.complex64)
        a = np.concatenate([a[:, 0, :] + t, a[:, 0, :] - t], axis=1).astype(np.complex64)
        half *= 2
    return a.reshape(n)


def spectrum_f32(block_bytes, n_bins, window):
    u = np.asarray(block_bytes, dtype=np.uint8).astype(np.float32)
    one28 = np.float32(1.0 / 128.0)
    re = (u[0::2] - np.float32(127.5)) * one28
    im = (u[1::2] - np.float32(127.5)) * one28
    N = int(n_bins)
    nseg = re.size // N
    if nseg < 1:
        raise ValueError("n_bins exceeds the block's samples")
    w64 = window_f64(N, window)
    w = w64.astype(np.float32)
    acc = np.zeros(N, np.float32)
    for s in range(nseg):
        seg = np.empty(N, np.complex64)
        seg.real = re[s * N:(s + 1) * N] * w
        seg.imag = im[s * N:(s + 1) * N] * w
        X = fft_f32(seg)
        acc = (acc + (X.real * X.real + X.imag * X.imag).astype(np.float32)).astype(np.float32)
    scale = np.float32(1.0 / (nseg * N * (w64 * w64).sum()))
    return (acc * scale).astype(np.float32)


def tone_bytes(n_bytes, freq, amp=0.9):
    """u8 IQ of a complex tone amp exp(2 pi i freq n), freq in cycles per sample, quantised to the nearest byte."""
    n = np.arange(n_bytes // 2, dtype=np.float64)
    z = amp * np.exp(2j * np.pi * freq * n)
    out = np.empty(n_bytes, np.uint8)
    out[0::2] = np.clip(np.rint(z.real * 128.0 + 127.5), 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.rint(z.imag * 128.0 + 127.5), 0, 255).astype(np.uint8)
    return out


# ---- the per-bin bound -----------------------------------------------------------------------------------------------------------------------

EPS_PATH = 1.05 * (1.0 + np.sqrt(2.0)) * 2.0 ** -24


def spectrum_bound(block_bytes, n_bins, window):
    """(P64 [N], bound [N]): the float64 model and the largest |P_dev[k] - P64[k]| that the documented arithmetic allows, bin by bin.

    Derivation (include/fmdemod_mi355x.h, "Capture spectrum"; csrc/spectrum.inc): the transform, the power sums and the scale are float64; the
    window and the pass twiddles are float tables made in double and rounded once; P is rounded to float32 once, at the store.  With X_seg the
    float64 DFT of the windowed segment:
      * the window value is off by <= 2^-24 of itself;
      * a value passes at most two twiddled passes (N = 256: one; 1024 and 4096: two), and a twiddle whose two components are each off by
        <= 2^-25 is off by <= sqrt(2) 2^-25;
      * so, to first order, every path from an input sample to an output bin is perturbed by at most eps = (1 + sqrt(2)) 2^-24 of itself;
        1.05 eps (EPS_PATH) covers the second-order terms and the float64 arithmetic;
      * with A_seg = sum_n |w[n] x[n]|:  |dX_seg[k]| <= eps A_seg,  so  | |X + dX|^2 - |X|^2 | <= 2 |X_seg[k]| eps A_seg + eps^2 A_seg^2;
      * d[k] = scale sum_seg (2 |X_seg[k]| eps A_seg + eps^2 A_seg^2),  scale = 1 / (nseg N sum w^2);
      * the one rounding to float32 adds 2^-24 (P[k] + d[k]) + 2^-149.
    bound[k] = d[k] + 2^-24 (P[k] + d[k]) + 2^-149.

    A worst-case bound on STRUCTURE, not a precision test: its size in a bin follows that bin's own |X|, so a weak bin beside a strong one is
    held to its own scale (a wrong twiddle, a leak between bins or slots, a spur far below the largest bin all show), which a norm over the
    block's bins cannot do.  It is no float32-against-float64 rule: a careful float32 transform (spectrum_f32) stays inside it."""
    x = samples_f64(block_bytes)
    N = int(n_bins)
    nseg = x.size // N
    if nseg < 1:
        raise ValueError("n_bins exceeds the block's samples")
    w = window_f64(N, window)
    xw = x[:nseg * N].reshape(nseg, N) * w
    X = np.fft.fft(xw, axis=1)
    A = np.abs(xw).sum(axis=1)[:, None]
    scale = 1.0 / (nseg * N * (w * w).sum())
    P = (X.real ** 2 + X.imag ** 2).sum(axis=0) / (nseg * N * (w * w).sum())          # spectrum_f64's own expression
    d = scale * (2.0 * np.abs(X) * EPS_PATH * A + (EPS_PATH * A) ** 2).sum(axis=0)
    return P, d + 2.0 ** -24 * (P + d) + 2.0 ** -149


def _dft_matrix(r):
    k = np.arange(r, dtype=np.float64)
    return np.exp(-2j * np.pi * np.outer(k, k) / r)


def _round_f32_parts(z):
    return z.real.astype(np.float32).astype(np.float64) + 1j * z.imag.astype(np.float32).astype(np.float64)


def fft_standin(xw, radices):
    """Stockham autosort transform of the rows of xw (complex128 [nseg, N]) in passes of the given radices, float64 throughout except the pass
    twiddles, whose cos and sin are rounded to float.  Pass of radix R after passes of product p, butterfly i of N / R:
    k = i mod p,  u[r] = x[i + r N / R] W^(r k),  W = exp(-2 pi i / (p R)),  U = DFT_R(u),  y[(i - k) R + k + r p] = U[r]."""
    n = xw.shape[1]
    assert int(np.prod(radices)) == n
    a = np.array(xw, dtype=np.complex128)
    p = 1
    for R in radices:
        i = np.arange(n // R)
        k = i % p
        r = np.arange(R)
        u = a[:, i[None, :] + r[:, None] * (n // R)]                                   # [nseg, R, N / R]
        if p > 1:
            u = u * _round_f32_parts(np.exp(-2j * np.pi * (r[:, None] * k[None, :]) / float(p * R)))
        U = np.einsum("qr,srj->sqj", _dft_matrix(R), u)
        a = np.empty_like(a)
        a[:, ((i - k) * R + k)[None, :] + r[:, None] * p] = U
        p *= R
    return a


STANDIN_RADICES = {256: (16, 16), 1024: (4, 16, 16), 4096: (16, 16, 16)}


def spectrum_standin(block_bytes, n_bins, window):
    """The documented arithmetic: float window (made in double, rounded once) on the float64 samples, fft_standin, power and scale in float64 (the
    scale from the unrounded window), one rounding to float32."""
    x = samples_f64(block_bytes)
    N = int(n_bins)
    nseg = x.size // N
    if nseg < 1:
        raise ValueError("n_bins exceeds the block's samples")
    w64 = window_f64(N, window)
    w = w64.astype(np.float32).astype(np.float64)
    X = fft_standin(x[:nseg * N].reshape(nseg, N) * w, STANDIN_RADICES[N])
    return ((X.real ** 2 + X.imag ** 2).sum(axis=0) * (1.0 / (nseg * N * (w64 * w64).sum()))).astype(np.float32)


def bound_share(got, p64, bound):
    """the largest |got[k] - P64[k]| / bound[k] over the bins"""
    return float((np.abs(np.asarray(got, dtype=np.float64) - p64) / bound).max())


BOUND_WORST = {}        # (n_bins, window) -> the largest share of the per-bin bound a device result has used so far in this session


def assert_bound_rule(got, p64, bound, n_bins, window, what):
    """|got[s, b, k] - P64[s, b, k]| <= bound[s, b, k] for every bin of every (stream, block); prints the worst share per (stream, block) and the
    session's worst per (n_bins, window), which DESIGN.md section 5b records"""
    assert got.shape == p64.shape == bound.shape and got.dtype == np.float32, what
    bad = []
    for s in range(got.shape[0]):
        for b in range(got.shape[1]):
            ratio = np.abs(got[s, b].astype(np.float64) - p64[s, b]) / bound[s, b]
            k = int(ratio.argmax())
            key = (int(n_bins), int(window))
            BOUND_WORST[key] = max(BOUND_WORST.get(key, 0.0), float(ratio[k]))
            print("%s stream %d block %d: per-bin bound: worst share %.3f at bin %d (P %.3e, bound %.3e)" % (what, s, b, ratio[k], k, p64[s, b, k], bound[s, b, k]))
            if not ratio[k] <= 1:
                bad.append((s, b, k, float(ratio[k]), int((ratio > 1).sum())))
    print("largest share of the per-bin bound so far: %s" %
          ", ".join("N %d window %d: %.3f" % (n, w, v) for (n, w), v in sorted(BOUND_WORST.items())))
    assert not bad, "%s: (stream, block, worst bin, its share of the bound, bins beyond it): %s" % (what, bad)


# ---- further inputs --------------------------------------------------------------------------------------------------------------------------

STRONG_FREQ, WEAK_FREQ, WEAK_DB = 0.1837, -0.3121, -50.0


def strong_weak_bytes(n_bytes, seed=2024):
    """A tone of amplitude 0.9 at 0.1837 fs plus one 50 dB below it at -0.3121 fs, uniform +-0.5 LSB dither (fixed seed) before the rounding to
    bytes: the weak station beside the strong one that a scanner looks for."""
    n = np.arange(n_bytes // 2, dtype=np.float64)
    z = 0.9 * np.exp(2j * np.pi * STRONG_FREQ * n) + 0.9 * 10.0 ** (WEAK_DB / 20.0) * np.exp(2j * np.pi * WEAK_FREQ * n)
    dither = np.random.default_rng(seed).uniform(-0.5, 0.5, (n.size, 2))
    out = np.empty(n_bytes, np.uint8)
    out[0::2] = np.clip(np.rint(z.real * 128.0 + 127.5 + dither[:, 0]), 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.rint(z.imag * 128.0 + 127.5 + dither[:, 1]), 0, 255).astype(np.uint8)
    return out


def square_bytes(n_bytes):
    """I = 0, 255, 0, ... and Q = 255, 0, 255, ...: full scale on both rails, all power on bin N / 2"""
    n = np.arange(n_bytes // 2)
    out = np.empty(n_bytes, np.uint8)
    out[0::2] = np.where(n % 2 == 0, 0, 255)
    out[1::2] = np.where(n % 2 == 0, 255, 0)
    return out


# ---- the inputs and the slot-edge shapes shared by tests/test_spectrum_cpu.py and tests/test_gpu_spectrum_edges.py -----------------------------

EDGE_KINDS = ("dds", "lcg", "quiet", "tone", "strong_weak", "square")

# A workgroup holds G = 4096 / N segment slots; slot g takes segments g, g + G, ...  Per N: one segment (G - 1 idle slots), G - 1, G, G + 1 and
# 2 G + 1 segments, each an exact fit, and one segment with the smallest tail (8 samples = one 16-byte word).
EDGE_BLOCK_LENS = {256: (512, 7680, 8192, 8704, 16896, 528), 1024: (2048, 6144, 8192, 10240, 18432, 2064), 4096: (8192, 16384, 24576, 8208)}
EDGE_NSEG = {256: (1, 15, 16, 17, 33, 1), 1024: (1, 3, 4, 5, 9, 1), 4096: (1, 2, 3, 1)}


def edge_cases():
    """[(block_len, n_bins, window)]: every length of EDGE_BLOCK_LENS with every n_bins that fits it and both windows"""
    lens = sorted({bl for v in EDGE_BLOCK_LENS.values() for bl in v})
    return [(bl, n, w) for bl in lens for n in (256, 1024, 4096) if n <= bl // 2 for w in (WINDOW_RECT, WINDOW_HANN)]


def input_bytes(kind, n_bytes):
    """the first n_bytes of one of EDGE_KINDS (the oracle's DDS multiplex and LCG bytes need the oracle package)"""
    if kind == "dds":
        from oracle import dds_bytes
        return dds_bytes(n_bytes, amp=100)
    if kind == "lcg":
        from oracle import lcg_bytes
        return lcg_bytes(n_bytes, 12345)[0]
    if kind == "quiet":
        return np.random.default_rng(7).integers(127, 129, n_bytes, dtype=np.uint8)
    if kind == "tone":
        return tone_bytes(n_bytes, STRONG_FREQ, amp=0.9)
    if kind == "strong_weak":
        return strong_weak_bytes(n_bytes)
    if kind == "square":
        return square_bytes(n_bytes)
    raise ValueError(kind)
