"""Models of the capture spectrum (fmd_batch_spectrum_device / _host; include/fmdemod_mi355x.h, "Capture spectrum"), written from the definition.
A helper, not a test.

Block of L = block_len / 2 complex samples x[n] = (I - 127.5) / 128 + j (Q - 127.5) / 128 (the reference's u8_f32_table[0], no fs/4 rotation),
N = n_bins, nseg = L // N whole segments from the start of the block, the tail unused:

    P[k] = sum_seg | sum_n w[n] x[seg N + n] exp(-2 pi i k n / N) |^2 / (nseg N sum_n w[n]^2),   k = 0 .. N - 1   (natural FFT order)

spectrum_f64: the definition with np.fft.fft in float64 - the yardstick.
spectrum_f32: the same in float32 throughout (an iterative radix-2 decimation-in-time FFT on complex64, twiddles made in double and rounded
once, power into a float32 accumulator segment by segment, the scale applied once) - what a careful float32 implementation loses, so the size
of error a float32 device kernel may show against the float64 model."""
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
