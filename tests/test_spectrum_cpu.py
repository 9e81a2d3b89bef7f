"""Capture spectrum without a device: the C ABI is declared, exported and wrapped; the argument checks that need no batch; the Python
models of tests/spectrum_model.py are the definition of include/fmdemod_mi355x.h ("Capture spectrum"); and the per-bin bound of
spectrum_model.spectrum_bound lets the documented arithmetic through and catches two faults that the rms / worst-value rule does not see."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

import rtl_fm_player_amd as R
from rtl_fm_player_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spectrum_model import (EDGE_BLOCK_LENS, EDGE_KINDS, EDGE_NSEG, WINDOW_HANN, WINDOW_RECT, bound_share, edge_cases, input_bytes,  # noqa: E402
                            samples_f64, spectrum_bound, spectrum_f32, spectrum_f64, spectrum_standin, strong_weak_bytes, tone_bytes)

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


# ---- the per-bin bound (spectrum_model.spectrum_bound) ----------------------------------------------------------------------------------------

def old_rule_shares(got, p64, p32):
    """the shares of the two limits of tests/test_gpu_spectrum.py's assert_model_rule: rms / (2 rms of the float32 model), worst / (3 worst)"""
    e_dev, e_ref = got.astype(np.float64) - p64, p32.astype(np.float64) - p64
    return np.sqrt((e_dev ** 2).mean()) / (2 * np.sqrt((e_ref ** 2).mean())), np.abs(e_dev).max() / (3 * np.abs(e_ref).max())


def test_the_edge_shapes_are_the_slot_edges():
    """per N: 1, G - 1, G, G + 1 and 2 G + 1 segments without a tail (G = 4096 / N slots; 4096: 1, 2, 3), then one segment and 8 samples"""
    for n, lens in EDGE_BLOCK_LENS.items():
        G = 4096 // n
        want = sorted({x for x in (1, G - 1, G, G + 1, 2 * G + 1) if x >= 1}) + [1]
        assert [bl // 2 // n for bl in lens] == want == list(EDGE_NSEG[n])
        assert all(bl % 16 == 0 for bl in lens)
        assert [bl // 2 - (bl // 2 // n) * n for bl in lens] == [0] * (len(lens) - 1) + [8]


@pytest.mark.parametrize("block_len", sorted({bl for v in EDGE_BLOCK_LENS.values() for bl in v}))
def test_the_documented_arithmetic_stays_inside_the_bound(block_len):
    """The stand-in (float64 mixed-radix passes, float window and twiddles, one rounding) and the correctly rounded float64 model, over every
    shape and input of tests/test_gpu_spectrum_edges.py: share of the bound below 1 (measured: at most 0.134 for both).  The float32 model's
    error is non-zero on every one of them but the square wave with the rectangular window, which the rms / worst-value rule needs to know (it
    divides by it).  The float32 model stays inside the bound as well (measured: at most 0.59): the bound is no precision test."""
    worst = {"standin": 0.0, "rounded once": 0.0, "float32 model": 0.0}
    for bl, n_bins, window in edge_cases():
        if bl != block_len:
            continue
        for kind in EDGE_KINDS:
            blk = input_bytes(kind, bl)
            p64, bound = spectrum_bound(blk, n_bins, window)
            assert np.array_equal(p64, spectrum_f64(blk, n_bins, window))
            p32 = spectrum_f32(blk, n_bins, window)
            for name, got in (("standin", spectrum_standin(blk, n_bins, window)), ("rounded once", p64.astype(np.float32)), ("float32 model", p32)):
                share = bound_share(got, p64, bound)
                worst[name] = max(worst[name], share)
                assert share < 1, (name, kind, n_bins, window, share)
            if (kind, window) == ("square", WINDOW_RECT):
                # +-255/256 with w = 1: every sum is exact in float32, 2 (255/256)^2 on bin N / 2 and 0 elsewhere; where nseg is a power of two the
                # scale is exact as well and the float32 model loses nothing.  The device rule then asks for the exact value
                # (tests/test_gpu_spectrum_edges.py)
                assert np.count_nonzero(p64) == 1 and p64[n_bins // 2] == pytest.approx(2 * (255 / 256) ** 2, rel=1e-15)
                nseg = bl // 2 // n_bins
                if nseg & (nseg - 1) == 0:
                    assert np.array_equal(p32.astype(np.float64), p64)
            else:
                assert np.abs(p32 - p64).max() > 0, (kind, n_bins, window)
    print("block_len %d: largest share of the per-bin bound: %s" % (block_len, ", ".join("%s %.3f" % kv for kv in worst.items())))


@functools.lru_cache(maxsize=None)
def fault_case(kind, n_bins, window):
    from oracle import dds_bytes
    blk = {"tone": lambda: tone_bytes(20480, 0.1837), "dds": lambda: dds_bytes(20480, amp=100)}[kind]()
    p64, bound = spectrum_bound(blk, n_bins, window)
    return p64, bound, spectrum_f32(blk, n_bins, window), spectrum_standin(blk, n_bins, window)


@pytest.mark.parametrize("kind,n_bins,window", [("tone", 1024, WINDOW_HANN), ("tone", 4096, WINDOW_RECT), ("dds", 4096, WINDOW_HANN)])
def test_a_spur_far_below_the_largest_bin_fails_the_bound_and_passes_the_old_rule(kind, n_bins, window):
    """1e-9 of the largest bin added to every bin of the stand-in: invisible to a norm over the block's bins, far outside a weak bin's own bound"""
    p64, bound, p32, standin = fault_case(kind, n_bins, window)
    assert bound_share(standin, p64, bound) < 1 and max(old_rule_shares(standin, p64, p32)) <= 1
    spur = (standin.astype(np.float64) + 1e-9 * p64.max()).astype(np.float32)
    sh_rms, sh_max = old_rule_shares(spur, p64, p32)
    share = bound_share(spur, p64, bound)
    print("spur on %s N %d window %d: rms / max rule %.2f / %.2f, per-bin bound %.1f" % (kind, n_bins, window, sh_rms, sh_max, share))
    assert sh_rms <= 1 and sh_max <= 1, "the gap: the rms / worst-value rule passes the spur"
    assert share > 1


def test_floor_bins_two_per_cent_high_fail_the_bound_and_pass_the_old_rule():
    """tone, N = 256, Hann; the floor: every bin within 100 x the median bin (251 of the 256)"""
    p64, bound, p32, standin = fault_case("tone", 256, WINDOW_HANN)
    floor = p64 <= 100 * np.median(p64)
    assert 128 < floor.sum() < 256
    high = np.where(floor, standin.astype(np.float64) * 1.02, standin.astype(np.float64)).astype(np.float32)
    sh_rms, sh_max = old_rule_shares(high, p64, p32)
    share = bound_share(high, p64, bound)
    print("floor 2 %% high: rms / max rule %.2f / %.2f, per-bin bound %.1f" % (sh_rms, sh_max, share))
    assert sh_rms <= 1 and sh_max <= 1, "the gap: the rms / worst-value rule passes the raised floor"
    assert share > 1


@pytest.mark.parametrize("n_bins,floor", [(1024, 2e-8), (4096, 5e-9)])
def test_the_weak_tone_stands_out_of_the_floor(n_bins, floor):
    """strong_weak at 262144 bytes with Hann: the weak bin reads 4.3e-6 to 4.6e-6 over a median floor of 2e-8 (N = 1024) or 5e-9 (N = 4096), and
    the bound there is 1e-4 of the bin: the rule sees a weak station beside a strong one"""
    p64, bound = spectrum_bound(strong_weak_bytes(262144), n_bins, WINDOW_HANN)
    k = int(round((1 - 0.3121) * n_bins))
    at = k - 2 + int(p64[k - 2:k + 3].argmax())
    assert 4.3e-6 <= p64[at] <= 4.6e-6
    assert 0.5 * floor <= np.median(p64) <= 2 * floor
    assert 0.5e-4 <= bound[at] / p64[at] <= 2e-4
    assert int(p64.argmax()) == int(round(0.1837 * n_bins))
