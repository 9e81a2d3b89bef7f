"""The channel tuner without a device: the C ABI is declared, exported and wrapped; every refusal of the supported range with its status and a
message; fmd_tuner_design bit-equal to the model's design; the carrier table exact at the quarter periods and equal to the model's;
fmd_tuner_shift on and off the grid; the models of tests/tuner_model.py pin the definition of include/fmdemod_mi355x.h ("Channel tuner") - identity,
quarter turn, split runs, a +300 kHz-shifted capture tuned back; the exempt share of rule 3 for every case of tests/test_gpu_tuner.py (so the cases
are fixed here); and the bound of tuner_model.tuner_bound lets the float32 arithmetic through and catches six planted defects."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import rtl_fm_player_amd as R
from rtl_fm_player_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl_fm_player_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_model as SP  # noqa: E402
import tuner_model as TM  # noqa: E402

NEW = ("fmd_tuner_design", "fmd_tuner_shift", "fmd_tuner_create", "fmd_batch_tuner_create", "fmd_tuner_destroy", "fmd_tuner_set_channel",
       "fmd_tuner_get_channel", "fmd_tuner_run_device", "fmd_tuner_run_host", "fmd_tuner_get_state", "fmd_tuner_set_state", "fmd_tuner_reset",
       "fmd_tuner_sync")

FMD_E_ARG, FMD_E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build_library()


@pytest.fixture(scope="module")
def tuner_check():
    """tests/c/tuner_check.c over the private fmdk_tuner_table / fmdk_tuner_channel: csrc/fmd_recv.c and fmd_error.c as sources, nothing of the device, under
    ASan and UBSan"""
    tmp = tempfile.mkdtemp(prefix="fmd_tuner_")
    exe = os.path.join(tmp, "tuner_check")
    subprocess.run(["cc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-g", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "c", "tuner_check.c"), os.path.join(CSRC, "fmd_recv.c"), os.path.join(CSRC, "fmd_error.c"), "-lm"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")     # (the leak checker needs ptrace, which not every sandbox grants)

    def ask(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
        return p.stdout.splitlines()
    yield ask
    shutil.rmtree(tmp, ignore_errors=True)


def test_new_names_are_declared_exported_and_wrapped():
    raw = open(os.path.join(ROOT, "include", "fmdemod_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(\w+)\s*\([^;{}]*\)\s*;", hdr))
    L = R.lib()
    for name in NEW:
        assert name in declared, name
        assert name in capi.exported_symbols(), name
        assert getattr(L, name).argtypes, name
    for meth in ("set_channel", "get_channel", "run_device", "run_host", "get_state", "set_state", "reset", "sync", "close"):
        assert callable(getattr(R.Tuner, meth)), meth
    assert callable(R.BatchDemod.tuner) and callable(R.tuner_design) and callable(R.tuner_shift)
    assert C.sizeof(R.FmdTunerConfig) == 24 and C.sizeof(R.FmdTunerChannel) == 16
    assert C.sizeof(R.FmdTunerState) == 16 + 128 and R.FmdTunerState.hist.offset == 16
    assert "#define FMD_TUNER_MAX_TAPS 64" in raw and "#define FMD_TUNER_MAX_PERIOD 4096" in raw
    assert "typedef struct fmd_tuner_config  { int32_t rate, step_hz, bw, n_taps, block_len, reserved; } fmd_tuner_config;" in raw
    assert "typedef struct fmd_tuner_channel { int32_t source, shift; float gain; int32_t reserved; } fmd_tuner_channel;" in raw


GOOD = dict(rate=2400000, step_hz=1000, bw=100000, n_taps=64, block_len=16384, reserved=0)


@pytest.mark.parametrize("bad,status", [
    (dict(rate=0), FMD_E_ARG), (dict(rate=-2400000), FMD_E_ARG),
    (dict(step_hz=0), FMD_E_ARG), (dict(step_hz=-1000), FMD_E_ARG), (dict(step_hz=7000), FMD_E_ARG),         # does not divide the rate
    (dict(step_hz=500), FMD_E_UNSUPPORTED),                                                                    # P = 4800
    (dict(step_hz=1200000), FMD_E_UNSUPPORTED),                                                                # P = 2
    (dict(step_hz=400000), FMD_E_UNSUPPORTED),                                                                 # P = 6: no multiple of 4
    (dict(n_taps=12), FMD_E_UNSUPPORTED), (dict(n_taps=68), FMD_E_UNSUPPORTED), (dict(n_taps=30), FMD_E_UNSUPPORTED), (dict(n_taps=0), FMD_E_UNSUPPORTED),
    (dict(bw=0), FMD_E_ARG), (dict(bw=1200000), FMD_E_ARG), (dict(bw=-5), FMD_E_ARG),
    (dict(block_len=48), FMD_E_ARG), (dict(block_len=200), FMD_E_ARG), (dict(block_len=0), FMD_E_ARG),       # below 64; no multiple of 16
    (dict(block_len=64), FMD_E_UNSUPPORTED), (dict(block_len=112), FMD_E_UNSUPPORTED),                         # L = 32, 56 < T = 64
])
def test_every_refusal_of_the_configuration_needs_no_device(bad, status):
    L = R.lib()
    cfg = R.FmdTunerConfig(**{**GOOD, **bad})
    taps = (C.c_float * 64)()
    sh = C.c_int32()
    for rc in (L.fmd_tuner_design(C.byref(cfg), taps), L.fmd_tuner_shift(C.byref(cfg), 0, 1, C.byref(sh))):
        assert rc == status, bad
        assert L.fmd_last_error()
    # ... and fmd_tuner_create refuses the same before it looks for a device
    h = C.c_void_p()
    assert L.fmd_tuner_create(C.byref(h), C.byref(cfg), None, 1, 1, -1) == status and not h.value


@pytest.mark.parametrize("ok", [dict(), dict(n_taps=16, block_len=64), dict(step_hz=600000), dict(rate=4096000, step_hz=1000), dict(bw=1199999),
                                dict(n_taps=20, block_len=64)])
def test_the_edges_of_the_range_are_accepted(ok):
    cfg = R.FmdTunerConfig(**{**GOOD, **ok})
    assert R.lib().fmd_tuner_design(C.byref(cfg), (C.c_float * 64)()) == 0


def f32_hex(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


def test_every_refusal_of_a_channel_needs_no_device(tuner_check):
    """-P < shift < P, gain finite with 0 < gain <= 64, source in range; and the derived table entry of an accepted channel"""
    q = lambda ns, src, sh, g: "c 2400000 1000 %d %d %d %s" % (ns, src, sh, f32_hex(g))  # noqa: E731
    bad = [q(2, 2, 0, 1), q(2, -1, 0, 1), q(1, 0, 2400, 1), q(1, 0, -2400, 1), q(1, 0, 0, 0.0), q(1, 0, 0, -1.0), q(1, 0, 0, 64.5), q(1, 0, 0, np.inf),
           q(1, 0, 0, np.nan)]
    for line, ans in zip(bad, tuner_check(bad)):
        f = ans.split(None, 2)
        assert f[0] == "refused" and int(f[1]) == FMD_E_ARG and len(f) == 3 and f[2], (line, ans)
    good = [(2, 1, 2399, 64.0), (1, 0, -2399, 2.0 ** -20), (3, 2, -700, 1.0), (1, 0, 0, 0.3), (1, 0, 600, 8.0)]
    for (ns, src, sh, g), ans in zip(good, tuner_check([q(*a) for a in good])):
        want_sh = sh % 2400
        assert ans.split() == [str(src), str(want_sh), str(8 * want_sh % 2400), str(2048 * want_sh % 2400), f32_hex(np.float32(128) * np.float32(g))], ans


def test_null_arguments_are_refused():
    L = R.lib()
    cfg = R.FmdTunerConfig(**GOOD)
    h = C.c_void_p()
    buf = (C.c_float * 1024)()
    sh = C.c_int32()
    ch = R.FmdTunerChannel(0, 0, 1.0, 0)
    assert L.fmd_tuner_design(C.byref(cfg), None) == FMD_E_ARG and L.fmd_tuner_design(None, buf) == FMD_E_ARG
    assert L.fmd_tuner_shift(C.byref(cfg), 0, 0, None) == FMD_E_ARG and L.fmd_tuner_shift(None, 0, 0, C.byref(sh)) == FMD_E_ARG
    assert L.fmd_tuner_create(None, C.byref(cfg), None, 1, 1, -1) == FMD_E_ARG
    assert L.fmd_tuner_create(C.byref(h), C.byref(cfg), None, 0, 1, -1) == FMD_E_ARG and L.fmd_tuner_create(C.byref(h), C.byref(cfg), None, 1, 0, -1) == FMD_E_ARG
    assert L.fmd_batch_tuner_create(C.byref(h), None, 1000, 100000, 64, 1) == FMD_E_ARG
    assert L.fmd_tuner_run_device(None, buf, 1, buf, None, None) == FMD_E_ARG and L.fmd_tuner_run_host(None, buf, 1, buf) == FMD_E_ARG
    assert L.fmd_tuner_set_channel(None, 0, C.byref(ch)) == FMD_E_ARG and L.fmd_tuner_get_channel(None, 0, C.byref(ch)) == FMD_E_ARG
    st = R.FmdTunerState()
    assert L.fmd_tuner_get_state(None, 0, C.byref(st)) == FMD_E_ARG and L.fmd_tuner_set_state(None, 0, C.byref(st)) == FMD_E_ARG
    assert L.fmd_tuner_reset(None) == FMD_E_ARG and L.fmd_tuner_sync(None) == FMD_E_ARG
    L.fmd_tuner_destroy(None)
    nan_taps = np.full(64, np.nan, dtype=np.float32)
    assert L.fmd_tuner_create(C.byref(h), C.byref(cfg), nan_taps.ctypes.data, 1, 1, -1) == FMD_E_ARG


def test_create_without_device_fails_loudly():
    if R.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(R.FmdError, match="no HIP device"):
        R.Tuner(R.FmdTunerConfig(**GOOD), 1, 1)


@pytest.mark.parametrize("rate,bw,T", [(2400000, 100000, 64), (2400000, 800000, 64), (2400000, 100000, 16), (4096000, 170666, 20), (4000, 166, 16)])
def test_design_is_bit_equal_to_the_models(rate, bw, T):
    h = R.tuner_design(R.FmdTunerConfig(rate, rate // 4, bw, T, 16384, 0))
    want = TM.design(rate, bw, T).astype(np.float32)
    assert h.dtype == np.float32 and h.shape == (T,)
    assert np.array_equal(h.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(h, h[::-1]) and abs(float(h.astype(np.float64).sum()) - 1.0) <= T * 2.0 ** -24
    # ... the fmd_subc_design formula with R = rate
    assert np.array_equal(h, R.subc_design(R.FmdSubcConfig(rate, rate // 8, bw, T, 4, 1024))[:T])


@pytest.mark.parametrize("P", [4, 8, 12, 2400, 4096, 100, 3000])
def test_the_table_is_exact_at_the_quarter_periods_and_equals_the_models(tuner_check, P):
    words = tuner_check(["t %d" % P])[0]
    tab = np.array([int(words[8 * i:8 * i + 8], 16) for i in range(2 * P)], dtype=np.uint32).view(np.float32)
    re, im = tab[0::2], tab[1::2]
    q = P // 4
    one, zero = np.float32(1).view(np.uint32), np.uint32(0)
    for k, (wr, wi) in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))):
        got = (re[k * q].view(np.uint32), im[k * q].view(np.uint32))
        want = tuple(zero if w == 0 else np.float32(w).view(np.uint32) for w in (wr, wi))          # +0, never -0
        assert got == want, (P, k, re[k * q], im[k * q])
    assert one == re[0].view(np.uint32)
    mr, mi = TM.table_f32(P)
    assert np.array_equal(re.view(np.uint32), mr.view(np.uint32)) and np.array_equal(im.view(np.uint32), mi.view(np.uint32))
    # the symmetries of the circle hold to the bit: a quarter turn on, and the mirror image in the diagonal
    p = np.arange(P)
    assert np.array_equal(re[(p + q) % P], -im + np.float32(0)) and np.array_equal(im[(p + q) % P], re)
    assert np.array_equal(re[(q - p) % P], im) and np.array_equal(im[(q - p) % P], re)
    ex = TM.table_exact(P)
    assert np.abs(re - ex.real).max() <= 2.0 ** -25 and np.abs(im - ex.imag).max() <= 2.0 ** -25           # rounded once


def test_shift_on_and_off_the_grid():
    cfg = R.FmdTunerConfig(**GOOD)
    assert R.tuner_shift(cfg, 100000, False) == -700 and R.tuner_shift(cfg, 100000, True) == -100
    assert R.tuner_shift(cfg, 0, False) == -600 and R.tuner_shift(cfg, 0, True) == 0
    assert R.tuner_shift(cfg, -700000, False) == 100 and R.tuner_shift(cfg, -1200000, True) == 1200 and R.tuner_shift(cfg, 1200000, False) == -1800
    for off, ot in ((100500, False), (1, True), (-999, False)):
        with pytest.raises(R.FmdError, match="not on the grid"):
            R.tuner_shift(cfg, off, ot)
    with pytest.raises(R.FmdError, match="outside the capture"):
        R.tuner_shift(cfg, 1201000, True)
    # -rate / 4 itself has to be on the grid: 2.4 Msps in steps of 800 kHz (P = 3 is refused anyway), 1 MHz steps of 4 Msps: -1000 kHz is, 2 MHz steps are not
    assert R.tuner_shift(R.FmdTunerConfig(4000000, 1000000, 100000, 64, 16384, 0), 0, False) == -1
    coarse = R.FmdTunerConfig(16000000, 2000000, 100000, 64, 16384, 0)
    assert R.tuner_shift(coarse, 0, False) == -2 and R.tuner_shift(coarse, 2000000, True) == -1
    with pytest.raises(R.FmdError, match="not on the grid"):
        R.tuner_shift(R.FmdTunerConfig(8000000, 1000000, 100000, 64, 16384, 0), 500000, False)
    for rate, step, off, ot in ((2400000, 1000, 100000, False), (2400000, 1000, 100500, False), (2400000, 25000, 300000, True), (4096000, 1000, 24000, False)):
        want = TM.shift_steps(rate, step, off, ot)
        sh = C.c_int32(12345)
        rc = R.lib().fmd_tuner_shift(C.byref(R.FmdTunerConfig(rate, step, 100000, 64, 16384, 0)), off, int(ot), C.byref(sh))
        assert (rc, sh.value) == ((0, want) if want is not None else (FMD_E_ARG, 12345))


# ---- the model's own sanity: pins the definition -----------------------------------------------------------------------------------------

IMPULSE16 = np.array([1.0] + [0.0] * 15, dtype=np.float32)


def test_identity_and_quarter_turn_in_the_models():
    """shift 0, h = (1, 0, ...), gain 1: the bytes come back; shift +P/4: the reference's rotate_90 byte pattern.  Both models, every byte value."""
    iq = TM.all_values_bytes(2 * 1024)
    for P in (4, 2400, 4096):
        for fn in (TM.tuner_f64, TM.tuner_f32):
            y, _ = fn(iq, IMPULSE16, P, 0)
            assert np.array_equal(TM.codes_f64(y.astype(np.complex128), 1.0)[0], iq), (P, fn.__name__)
            y, _ = fn(iq, IMPULSE16, P, P // 4)
            assert np.array_equal(TM.codes_f64(y.astype(np.complex128), 1.0)[0], TM.rotate_90_bytes(iq)), (P, fn.__name__)
            y, _ = fn(iq, IMPULSE16, P, -3 * P // 4)                                        # the same turn, named from the other side
            assert np.array_equal(TM.codes_f64(y.astype(np.complex128), 1.0)[0], TM.rotate_90_bytes(iq))
        y32, _ = TM.tuner_f32(iq, IMPULSE16, P, P // 4)
        assert np.array_equal(TM.quantise_f32(y32, 1.0), TM.rotate_90_bytes(iq))
    assert set(iq[0::2]) == set(range(256)) and set(iq[1::2]) == set(range(256))


@pytest.mark.parametrize("fn", [TM.tuner_f64, TM.tuner_f32])
def test_a_split_run_equals_the_unsplit_one_exactly(fn):
    T, P, bl = 64, 2400, 512                       # P does not divide L = 256: the count is non-zero at block starts
    taps = TM.case_taps(T, P)
    iq = TM.case_input("lcg", 6 * bl)
    whole, st_whole = fn(iq, taps, P, -700)
    split, st_split = TM.run_blocks(fn, iq, bl, taps, P, -700)
    assert np.array_equal(whole, split)
    assert st_whole[0] == st_split[0] == (6 * bl // 2) % P and np.array_equal(st_whole[1], st_split[1])
    assert np.array_equal(st_whole[1].reshape(-1), iq[-2 * T:])


def test_fma32_is_a_correctly_rounded_float32_fma():
    rng = np.random.default_rng(1)
    a, b = (rng.standard_normal(20000).astype(np.float32) for _ in range(2))
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.uniform(-1e-6, 1e-6, a.size))).astype(np.float32)   # heavy cancellation
    got = TM.fma32(a, b, c)
    want = np.array([np.float32(np.longdouble(x) * np.longdouble(y) + np.longdouble(z)) for x, y, z in zip(a[:4000], b[:4000], c[:4000])], dtype=np.float32)
    assert np.finfo(np.longdouble).nmant >= 63 and np.array_equal(got[:4000], want)        # (64 bits hold these cancelling sums exactly)
    assert TM.fma32(np.float32(128), np.float32(2.0 ** -30), np.float32(127.5)) == np.float32(127.5)


def test_a_shifted_capture_tuned_back_peaks_where_the_original_does():
    """The oracle's DDS multiplex (peak at bin 197 of 256: the header's capture-spectrum note) moved by +300 kHz in float64 and requantised peaks 32
    bins on; the model with fmd_tuner_design's taps (bw 800 kHz: the station sits at -fs/4 and real taps pass +-bw) and shift -300 brings it back."""
    from oracle import dds_bytes
    rate, bl = 2400000, 16384
    iq = dds_bytes(2 * bl, amp=100)
    assert int(np.argmax(SP.spectrum_f64(iq[:bl], 256, SP.WINDOW_RECT))) == 197
    moved = TM.shifted_bytes(iq, 300000, rate)
    assert int(np.argmax(SP.spectrum_f64(moved[:bl], 256, SP.WINDOW_RECT))) == 197 + 32
    taps = R.tuner_design(R.FmdTunerConfig(rate, 1000, 800000, 64, bl, 0))
    for fn in (TM.tuner_f64, TM.tuner_f32):
        y, _ = fn(moved, taps, 2400, -300)
        back = TM.codes_f64(y.astype(np.complex128), 1.0)[0]
        assert int(np.argmax(SP.spectrum_f64(back[:bl], 256, SP.WINDOW_RECT))) == 197, fn.__name__
        # (the multiplex is frequency-modulated: a short block's peak follows the audio - the original's second block of 8192 samples peaks at 187)
        assert int(np.argmax(SP.spectrum_f64(back[bl:], 256, SP.WINDOW_RECT))) == int(np.argmax(SP.spectrum_f64(iq[bl:], 256, SP.WINDOW_RECT))) == 187


# ---- the GPU cases of rule 3 are fixed here -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", TM.MODEL_CASES, ids=[c[0] for c in TM.MODEL_CASES])
def test_the_exempt_share_of_every_gpu_case_is_at_most_one_percent(case):
    """Rule 3 holds the device's bytes to the float64 model's except where the model's pre-rounding value lies within G bound + 2^-16 of a boundary.
    That set must stay small for the rule to mean something: at most 1 % of the case, over its five channels and all its blocks - from the float64
    model alone.  Also here: the float32 model's codes obey rule 3, and at gain 8 on LCG input the codes 0 and 255 occur."""
    name, kind, T, P, shift, gain, bl, nb = case
    taps = TM.case_taps(T, P)
    n_ex = n_all = 0
    share32 = 0.0
    seen = set()
    for src, sh, g in TM.case_channels(P, shift, gain):
        iq = TM.case_input(kind, bl * nb, src)
        y64, _ = TM.run_blocks(TM.tuner_f64, iq, bl, taps, P, sh)
        bound = TM.tuner_bound(iq, taps)
        codes, v = TM.codes_f64(y64, g)
        ex = TM.exempt(v, bound, g)
        n_ex += int(ex.sum())
        n_all += ex.size
        seen |= set(np.unique(codes))
        y32, _ = TM.run_blocks(TM.tuner_f32, iq, bl, taps, P, sh)
        share32 = max(share32, TM.bound_share(y32, y64, bound))
        d = np.abs(TM.quantise_f32(y32, g).astype(np.int32) - codes.astype(np.int32))
        assert d[~ex].max() == 0 and d.max() <= 1
    print("%s: exempt %d of %d = %.3f %%; the float32 model uses %.4f of the bound" % (name, n_ex, n_all, 100.0 * n_ex / n_all, share32))
    assert n_ex <= 0.01 * n_all
    assert share32 < 1
    if kind == "lcg" and gain == 8.0:
        assert 0 in seen and 255 in seen


def test_silence_is_no_case_for_rule_3():
    """Nothing in the passband - a capture that holds only its DC term, moved 600 kHz away: the output sits on the tie at 127.5 and nearly every
    value is exempt - why an empty passband and quiet input are held to rules 1 and 2 only (tuner_model.EMPTY_PASSBAND is the GPU test's input)"""
    T, P, bl = 64, 2400, 16384
    taps = TM.case_taps(T, P)
    iq = TM.dc_bytes(bl)
    y64, _ = TM.tuner_f64(iq, taps, P, TM.EMPTY_PASSBAND_SHIFT)
    codes, v = TM.codes_f64(y64, 1.0)
    ex = TM.exempt(v, TM.tuner_bound(iq, taps), 1.0)
    print("a DC term alone, moved out of band: exempt %.1f %%" % (100.0 * ex.mean()))
    assert ex.mean() > 0.5 and set(np.unique(codes[2 * T:])) <= {127, 128}


# ---- the bound has teeth -----------------------------------------------------------------------------------------------------------------

TEETH_SHAPES = [(64, 2400, -700, 2 * (4096 + 24)), (16, 2400, 100, 64), (64, 2400, -700, 512), (16, 4, 3, 512), (64, 4096, -1195, 2 * (4096 + 24))]


@pytest.mark.parametrize("T,P,shift,bl", TEETH_SHAPES)
def test_six_planted_defects_exceed_the_bound(T, P, shift, bl):
    """numpy stand-ins of a wrong kernel on the LCG input, 3 blocks: one tap zeroed; the history one sample late at a block edge; the count not
    carried across a block; I and Q swapped; the sign of the shift; (n shift) mod P without the wrap (the index clamped to the table instead).
    Each passes a loose look (finite, right size) and exceeds the bound by the printed factor."""
    taps = TM.case_taps(T, P)
    iq = TM.case_input("lcg", 3 * bl)
    y64, _ = TM.run_blocks(TM.tuner_f64, iq, bl, taps, P, shift)
    bound = TM.tuner_bound(iq, taps)
    good, _ = TM.run_blocks(TM.tuner_f32, iq, bl, taps, P, shift)
    share = TM.bound_share(good, y64, bound)
    print("T %d P %d block_len %d: the float32 model uses %.4f of the bound" % (T, P, bl, share))
    assert share < 0.2

    wrong_tap = taps.copy()
    wrong_tap[T // 2 + 3] = 0.0

    def faulty(late_hist=False, hold_count=False):
        out, count, hist = [], 0, None
        for s in range(0, iq.size, bl):
            y, (ncount, nhist) = TM.tuner_f32(iq[s:s + bl], taps, P, shift, count, hist)
            out.append(y)
            hist = np.concatenate([nhist[:1], nhist[:-1]]) if late_hist else nhist
            count = count if hold_count else ncount
        return np.concatenate(out)

    def no_wrap():
        xr, xi = TM._extended(iq, None, T, np.float32)
        idx = np.minimum(TM._index(0, T, xr.size - T, P, shift, wrap=False), P - 1)
        cr, ci = TM.table_f32(P)
        mr = TM.fma32(xr, cr[idx], -(xi * ci[idx]))
        mi = TM.fma32(xr, ci[idx], xi * cr[idx])
        e = np.arange(xr.size - T) + T
        yr, yi = np.zeros(e.size, np.float32), np.zeros(e.size, np.float32)
        for k in range(T):
            yr = TM.fma32(np.full(e.size, taps[k], np.float32), mr[e - k], yr)
            yi = TM.fma32(np.full(e.size, taps[k], np.float32), mi[e - k], yi)
        return yr + 1j * yi

    swapped = iq.reshape(-1, 2)[:, ::-1].reshape(-1)
    shares = {"one tap zeroed": TM.run_blocks(TM.tuner_f32, iq, bl, wrong_tap, P, shift)[0],
              "history one sample late at a block edge": faulty(late_hist=True),
              "count not carried across a block": faulty(hold_count=True),
              "I and Q swapped": TM.run_blocks(TM.tuner_f32, swapped, bl, taps, P, shift)[0],
              "sign of the shift": TM.run_blocks(TM.tuner_f32, iq, bl, taps, P, -shift)[0],
              "index without the wrap": no_wrap()}
    shares = {k: TM.bound_share(v, y64, bound) for k, v in shares.items()}
    print("T %d P %d block_len %d: %s" % (T, P, bl, ", ".join("%s x%.0f" % kv for kv in shares.items())))
    for what, s in shares.items():
        if what == "count not carried across a block" and ((bl // 2) * (shift % P)) % P == 0:
            continue                                        # (a block of whole carrier periods of this shift: holding the count is no fault)
        assert np.isfinite(s) and s > 1, what
