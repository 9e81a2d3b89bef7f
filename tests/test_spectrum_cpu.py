"""Capture spectrum without a device: the C ABI is declared, exported and wrapped; the argument checks that need no batch; and the Python
models of tests/spectrum_model.py are the definition of include/fmdemod_mi355x.h ("Capture spectrum")."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import rtl_fm_player_amd as R
from rtl_fm_player_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spectrum_model import WINDOW_HANN, WINDOW_RECT, samples_f64, spectrum_f32, spectrum_f64, tone_bytes  # noqa: E402

NEW = ("fmd_batch_spectrum_device", "fmd_batch_spectrum_host")


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build_library()


def test_new_names_are_declared_exported_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "fmdemod_mi355x.h")).read()
    raw = hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(\w+)\s*\([^;{}]*\)\s*;", hdr))
    L = R.lib()
    for name in NEW:
        assert name in declared, name
        assert name in capi.exported_symbols(), name
        assert getattr(L, name).argtypes, name
    for meth in ("spectrum_device", "spectrum_host"):
        assert callable(getattr(R.BatchDemod, meth)), meth
    assert (R.WINDOW_RECT, R.WINDOW_HANN) == (WINDOW_RECT, WINDOW_HANN) == (0, 1)
    assert re.search(r"#define\s+FMD_WINDOW_RECT\s+0\b", raw) and re.search(r"#define\s+FMD_WINDOW_HANN\s+1\b", raw)


def test_argument_checks_without_a_batch():
    L = R.lib()
    buf = (C.c_float * 1024)()
    assert L.fmd_batch_spectrum_device(None, buf, 1, 256, 0, buf, None) == -1
    assert b"NULL" in L.fmd_last_error()
    assert L.fmd_batch_spectrum_host(None, buf, 1, 256, 1, buf) == -1
    assert b"NULL" in L.fmd_last_error()


@pytest.mark.parametrize("n_bins", [256, 1024, 4096])
def test_parseval_with_the_rectangular_window(n_bins):
    """sum of P = mean |x|^2 over the USED samples (the tail of 10240 - 2 x 4096 samples is not)"""
    from oracle import lcg_bytes
    blk = lcg_bytes(20480, 12345)[0]
    x = samples_f64(blk)
    used = (x.size // n_bins) * n_bins
    assert spectrum_f64(blk, n_bins, WINDOW_RECT).sum() == pytest.approx((np.abs(x[:used]) ** 2).mean(), rel=1e-12)


@pytest.mark.parametrize("window", [WINDOW_RECT, WINDOW_HANN])
@pytest.mark.parametrize("n_bins,k0", [(256, 37), (1024, 700), (4096, 4095)])
def test_a_bin_centred_tone_peaks_at_its_bin(n_bins, k0, window):
    """... and reads A^2 with the rectangular window (to the byte quantisation: the tone is rounded to 1/128 steps, offset by half a step)"""
    blk = tone_bytes(4 * 2 * n_bins, k0 / n_bins, amp=0.9)
    P = spectrum_f64(blk, n_bins, window)
    assert int(P.argmax()) == k0
    if window == WINDOW_RECT:
        assert P[k0] == pytest.approx(0.81, rel=0.02)


@pytest.mark.parametrize("n_bins", [256, 1024, 4096])
def test_the_tuned_channel_sits_on_bin_three_quarters_n(n_bins):
    """Without offset_tuning the chain multiplies by j^n: the tuned channel is centred on -fs / 4.  The oracle's DDS multiplex peaks within
    +-100 kHz = N / 24 bins of bin 3 N / 4 (the header's 197 of 256, 747 of 1024, 3149 of 4096)."""
    from oracle import dds_bytes
    P = spectrum_f64(dds_bytes(262144, amp=100), n_bins, WINDOW_RECT)
    peak = int(P.argmax())
    assert abs(peak - 3 * n_bins // 4) <= n_bins / 24, peak
    assert peak == {256: 197, 1024: 747, 4096: 3149}[n_bins]


@pytest.mark.parametrize("window", [WINDOW_RECT, WINDOW_HANN])
@pytest.mark.parametrize("n_bins", [256, 1024, 4096])
def test_the_float32_model_agrees_with_the_float64_model(n_bins, window):
    """a sanity bound on the model (1e-4 of the largest bin), not the device rule"""
    from oracle import dds_bytes, lcg_bytes
    for blk in (lcg_bytes(20480, 12345)[0], dds_bytes(20480, amp=100), tone_bytes(20480, 0.1837)):
        a, b = spectrum_f64(blk, n_bins, window), spectrum_f32(blk, n_bins, window)
        assert b.dtype == np.float32 and b.shape == (n_bins,)
        assert np.abs(b - a).max() <= 1e-4 * a.max()
        assert np.abs(b - a).max() > 0
