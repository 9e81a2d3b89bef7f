"""The MPX subcarrier receiver without a device: the C ABI is declared, exported and wrapped; every refusal of the supported range;
fmd_subc_design against the numpy formula; the models of tests/subc_model.py pin the definition of include/fmdemod_mi355x.h ("MPX subcarrier
receiver") - a tone reads A e^(i phi), a split run equals the unsplit one, an RDS-like biphase vector decodes, the pilot recipe reads the
oracle's pilot; and the bound of subc_model.subc_bound lets the float32 arithmetic through and catches a wrong tap, a shifted history sample
and a phase slip - at the shapes of tests/test_gpu_subc.py and at the edge shapes of tests/test_gpu_subc_edges.py (subc_model.EDGE_SHAPES)."""
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
import subc_model as SM  # noqa: E402

NEW = ("fmd_subc_design", "fmd_subc_create", "fmd_batch_subc_create", "fmd_subc_destroy", "fmd_subc_out_per_block", "fmd_subc_run_device",
       "fmd_subc_run_host", "fmd_subc_get_state", "fmd_subc_set_state", "fmd_subc_reset", "fmd_subc_sync")

FMD_E_ARG, FMD_E_UNSUPPORTED = -1, -2


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
    for meth in ("run_device", "run_host", "get_state", "set_state", "reset", "sync", "close"):
        assert callable(getattr(R.Subcarrier, meth)), meth
    assert callable(R.BatchDemod.subcarrier) and callable(R.subc_design)
    assert C.sizeof(R.FmdSubcConfig) == 24 and C.sizeof(R.FmdSubcState) == 16 + 4 * 256 and R.FmdSubcState.hist.offset == 16
    assert "typedef struct fmd_subc_config { int32_t rate_in, fc, bw, n_taps, decim, block_samples; } fmd_subc_config;" in raw
    assert "typedef struct fmd_subc_state  { int32_t phase; int32_t reserved[3]; float hist[256]; } fmd_subc_state;" in raw


GOOD = dict(rate_in=300000, fc=57000, bw=2400, n_taps=128, decim=16, block_samples=512)


@pytest.mark.parametrize("bad,status", [
    (dict(fc=0), FMD_E_ARG), (dict(fc=-19000), FMD_E_ARG), (dict(fc=150000), FMD_E_ARG), (dict(fc=200000), FMD_E_ARG),
    (dict(bw=0), FMD_E_ARG), (dict(bw=150000), FMD_E_ARG), (dict(rate_in=0), FMD_E_ARG),
    (dict(fc=57001), FMD_E_UNSUPPORTED),                       # Pd = 300000
    (dict(rate_in=299999, fc=19000), FMD_E_UNSUPPORTED),       # Pd = 299999
    (dict(n_taps=12), FMD_E_UNSUPPORTED), (dict(n_taps=130), FMD_E_UNSUPPORTED), (dict(n_taps=260, block_samples=1024), FMD_E_UNSUPPORTED),
    (dict(n_taps=0), FMD_E_UNSUPPORTED),
    (dict(decim=2), FMD_E_UNSUPPORTED), (dict(decim=12), FMD_E_UNSUPPORTED), (dict(decim=64), FMD_E_UNSUPPORTED), (dict(decim=0), FMD_E_UNSUPPORTED),
    (dict(block_samples=520), FMD_E_ARG),                      # no multiple of D
    (dict(block_samples=0), FMD_E_ARG),
    (dict(block_samples=112), FMD_E_UNSUPPORTED),              # a multiple of D, shorter than the filter
])
def test_every_refusal_of_the_supported_range_needs_no_device(bad, status):
    L = R.lib()
    cfg = R.FmdSubcConfig(**{**GOOD, **bad})
    taps = (C.c_float * 256)()
    assert L.fmd_subc_design(C.byref(cfg), taps) == status, bad
    assert L.fmd_last_error()
    # ... and fmd_subc_create refuses the same before it looks for a device
    h = C.c_void_p()
    assert L.fmd_subc_create(C.byref(h), C.byref(cfg), None, 1, -1) == status and not h.value


def test_null_arguments_are_refused():
    L = R.lib()
    cfg = R.FmdSubcConfig(**GOOD)
    h = C.c_void_p()
    buf = (C.c_float * 1024)()
    assert L.fmd_subc_design(C.byref(cfg), None) == FMD_E_ARG and L.fmd_subc_design(None, buf) == FMD_E_ARG
    assert L.fmd_subc_create(None, C.byref(cfg), None, 1, -1) == FMD_E_ARG
    assert L.fmd_subc_create(C.byref(h), C.byref(cfg), None, 0, -1) == FMD_E_ARG
    assert L.fmd_batch_subc_create(C.byref(h), None, 19000, 500, 128, 16) == FMD_E_ARG
    assert L.fmd_subc_run_device(None, buf, 1, buf, None) == FMD_E_ARG and L.fmd_subc_run_host(None, buf, 1, buf) == FMD_E_ARG
    assert L.fmd_subc_out_per_block(None) == FMD_E_ARG
    st = R.FmdSubcState()
    assert L.fmd_subc_get_state(None, 0, C.byref(st)) == FMD_E_ARG and L.fmd_subc_set_state(None, 0, C.byref(st)) == FMD_E_ARG
    assert L.fmd_subc_reset(None) == FMD_E_ARG and L.fmd_subc_sync(None) == FMD_E_ARG
    L.fmd_subc_destroy(None)
    nan_taps = np.full(128, np.nan, dtype=np.float32)
    assert L.fmd_subc_create(C.byref(h), C.byref(cfg), nan_taps.ctypes.data, 1, -1) == FMD_E_ARG


def test_create_without_device_fails_loudly():
    if R.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(R.FmdError, match="no HIP device"):
        R.Subcarrier(R.FmdSubcConfig(**GOOD), 1)


@pytest.mark.parametrize("rate,fc,bw,T", [(300000, 57000, 2400, 128), (192000, 19000, 500, 256), (300000, 57000, 2400, 16), (240000, 67000, 4000, 16)])
def test_design_equals_the_numpy_formula(rate, fc, bw, T):
    h = R.subc_design(R.FmdSubcConfig(rate, fc, bw, T, 4, 1024))
    want = SM.design(rate, bw, T)
    assert h.dtype == np.float32 and h.shape == (T,)
    assert np.abs(h.astype(np.float64) - want).max() <= np.spacing(np.float32(want.max()))
    assert np.array_equal(h, h[::-1])
    assert abs(float(h.astype(np.float64).sum()) - 1.0) <= T * 2.0 ** -24
    assert int(h.argmax()) in (T // 2 - 1, T // 2)


def test_the_periods_of_the_header():
    assert [SM.period(r, 57000) for r in (300000, 240000, 192000)] == [100, 80, 64]
    assert [SM.period(r, 19000) for r in (300000, 240000, 192000)] == [300, 240, 192]


# ---- the model's own sanity: pins the definition -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate,fc,bw,T,D", [(300000, 57000, 2400, 128, 16), (300000, 19000, 500, 256, 16), (192000, 57000, 2400, 64, 8)])
def test_a_real_tone_reads_its_amplitude_and_phase(rate, fc, bw, T, D):
    A, phi = 0.3, 0.7
    v = SM.tone(64 * T, rate, fc, A, phi).astype(np.float64)
    z, _ = SM.subc_f64(v, SM.design(rate, bw, T).astype(np.float32), rate, fc, D)
    settled = z[T // D:]
    assert settled.size > 100
    assert np.abs(settled - A * np.exp(1j * phi)).max() <= 1e-4 * A


@pytest.mark.parametrize("fn", [SM.subc_f64, SM.subc_f32])
def test_a_split_run_equals_the_unsplit_one_exactly(fn):
    rate, fc, T, D, M = 300000, 19000, 256, 16, 256               # Pd = 300 does not divide M: the phase is non-zero at block starts
    taps = SM.design(rate, 500, T).astype(np.float32)
    v = SM.lcg_floats(6 * M, 1)
    whole, st_whole = fn(v, taps, rate, fc, D)
    split, st_split = SM.run_blocks(fn, v, M, taps, rate, fc, D)
    assert np.array_equal(whole, split)
    assert st_whole[0] == st_split[0] == (6 * M) % 300 and np.array_equal(st_whole[1], st_split[1]) and np.array_equal(st_whole[1], v[-T:])
    uneven = np.concatenate([fn(v[:M], taps, rate, fc, D)[0], fn(v[M:], taps, rate, fc, D, *fn(v[:M], taps, rate, fc, D)[1])[0]])
    assert np.array_equal(whole, uneven)


def test_an_rds_like_vector_decodes_without_bit_errors():
    """58 random bits at 1187.5 bit/s, biphase, on a 57 kHz carrier of 0.03 beside a 0.157 pilot and a 0.5 audio tone: the RDS recipe
    (fc 57000, bw 2400, T 128, D 16 at 300 k) and the documented group delay recover every one"""
    rate, T, D = 300000, 128, 16
    v, bits = SM.rds_like(rate, 60)
    z, _ = SM.subc_f64(v, SM.design(rate, 2400, T).astype(np.float32), rate, 57000, D)
    got = SM.rds_decode(z, 60, rate, T, D)
    assert got.size == 58
    assert int((got != bits[1:59]).sum()) == 0
    assert 0.02 < np.abs(z[T // D:200]).max() < 0.04


@functools.lru_cache(maxsize=None)
def oracle_v(stereo, rate=300000):
    from oracle import OracleStream, dds_bytes
    bl, nb = 8192, 6
    iq = dds_bytes(bl * nb, stereo=stereo)
    o = OracleStream(rate_in=rate)
    v = np.concatenate([o.block(iq[b * bl:(b + 1) * bl], trace=True)[1]["v"].copy() for b in range(nb)])
    v.setflags(write=False)
    return v


def test_the_pilot_recipe_reads_the_oracles_pilot():
    """fc 19000, bw 500, T 128, D 16 on the oracle's discriminator output of the DDS multiplex: |z| is the pilot's deviation in radians per
    sample, 0.157 for a 10 % pilot at 300 k (measured 0.1543 .. 0.1556), and nothing without the pilot (measured at most 0.0010)"""
    rate, T, D = 300000, 128, 16
    taps = R.subc_design(R.FmdSubcConfig(rate, 19000, 500, T, D, 512))
    on = np.abs(SM.subc_f64(oracle_v(1), taps, rate, 19000, D)[0][16:])
    off = np.abs(SM.subc_f64(oracle_v(0), taps, rate, 19000, D)[0][16:])
    print("pilot on: |z| %.4f .. %.4f, off: max %.4f" % (on.min(), on.max(), off.max()))
    assert 0.150 <= on.min() and on.max() <= 0.160
    assert off.max() < 0.005


# ---- the bound has teeth -----------------------------------------------------------------------------------------------------------------

SHAPES = [(300000, 19000, 500, 256, 16, 256), (192000, 57000, 2400, 16, 4, 512), (300000, 57000, 2400, 128, 32, 512), (240000, 57000, 2400, 96, 8, 1024)]


def inputs(rate, fc, M, nb=3):
    imp = np.zeros(nb * M, dtype=np.float32)
    imp[M - 1] = 1.0
    return {"lcg": SM.lcg_floats(nb * M, 7), "tone": SM.tone(nb * M, rate, fc), "zeros": np.zeros(nb * M, dtype=np.float32), "impulse": imp,
            "oracle": np.array(oracle_v(1)[:nb * M])}


@pytest.mark.parametrize("rate,fc,bw,T,D,M", SHAPES)
def test_the_float32_model_stays_under_a_tenth_of_the_bound(rate, fc, bw, T, D, M):
    taps = SM.design(rate, bw, T).astype(np.float32)
    worst = 0.0
    for kind, v in inputs(rate, fc, M).items():
        z64, _ = SM.run_blocks(SM.subc_f64, v, M, taps, rate, fc, D)
        z32, _ = SM.run_blocks(SM.subc_f32, v, M, taps, rate, fc, D)
        share = SM.bound_share(z32, z64, SM.subc_bound(v, taps, D))
        worst = max(worst, share)
        assert share < 0.1, (kind, share)
        if kind == "zeros":
            assert not z32.any() and not z64.any()
    print("T %d D %d: the float32 model uses at most %.4f of the bound" % (T, D, worst))


@pytest.mark.parametrize("rate,fc,bw,T,D,M", SM.EDGE_SHAPES)
def test_the_float32_model_stays_inside_the_bound_at_the_edge_shapes(rate, fc, bw, T, D, M):
    """The shapes of tests/test_gpu_subc_edges.py (carrier periods 3, 4 and 4096, one-output chunks and blocks, the smallest block, 64 tap groups):
    the float32 model run block by block, LCG and tone input, 3 blocks.  Measured on the LCG input: 0.030, 0.039, 0.085, 0.0056, 0.061, 0.028 and
    0.0029 of the bound - the reference alone does not threaten it at any of them."""
    taps = SM.design(rate, bw, T).astype(np.float32)
    assert SM.period(rate, fc) in (4096, 3, 4, 300, 64, 100) and R.lib().fmd_subc_design(C.byref(R.FmdSubcConfig(rate, fc, bw, T, D, M)), (C.c_float * 256)()) == 0
    for kind, v in (("lcg", SM.lcg_floats(3 * M, 7)), ("tone", SM.tone(3 * M, rate, fc))):
        z64, _ = SM.run_blocks(SM.subc_f64, v, M, taps, rate, fc, D)
        z32, _ = SM.run_blocks(SM.subc_f32, v, M, taps, rate, fc, D)
        share = SM.bound_share(z32, z64, SM.subc_bound(v, taps, D))
        print("%s Pd %d T %d D %d M %d: the float32 model uses %.4f of the bound" % (kind, SM.period(rate, fc), T, D, M, share))
        assert share < 1, (kind, share)


# ... and on the edge shapes of tests/test_gpu_subc_edges.py with the shortest and the longest carrier period, one output per block and one output
# per ragged chunk
@pytest.mark.parametrize("rate,fc,bw,T,D,M", SHAPES + [SM.EDGE_SHAPES[1], SM.EDGE_SHAPES[0], SM.EDGE_SHAPES[5]] + SM.RAGGED_ONE_OUTPUT)
def test_three_faults_exceed_the_bound(rate, fc, bw, T, D, M):
    """numpy stand-ins of a wrong kernel on the LCG input: one tap zeroed; the history one sample late at a block edge; the phase not advanced
    across a block.  Each passes a loose look (finite, right size) and exceeds the bound by far."""
    taps = SM.design(rate, bw, T).astype(np.float32)
    v = SM.lcg_floats(3 * M, 7)
    z64, _ = SM.run_blocks(SM.subc_f64, v, M, taps, rate, fc, D)
    bound = SM.subc_bound(v, taps, D)
    good, _ = SM.run_blocks(SM.subc_f32, v, M, taps, rate, fc, D)
    assert SM.bound_share(good, z64, bound) < 0.1

    wrong_tap = taps.copy()
    wrong_tap[T // 2 + 3] = 0.0
    a, _ = SM.run_blocks(SM.subc_f32, v, M, wrong_tap, rate, fc, D)

    def faulty(shift_hist, hold_phase):
        out, phase, hist = [], 0, None
        for s in range(0, v.size, M):
            z, (nphase, nhist) = SM.subc_f32(v[s:s + M], taps, rate, fc, D, phase, hist)
            out.append(z)
            hist = np.concatenate([nhist[:1], nhist[:-1]]) if shift_hist else nhist
            phase = phase if hold_phase else nphase
        return np.concatenate(out)

    shares = {"one tap zeroed": SM.bound_share(a, z64, bound), "history shifted at a block edge": SM.bound_share(faulty(True, False), z64, bound),
              "phase not advanced": SM.bound_share(faulty(False, True), z64, bound)}
    print("T %d D %d: %s" % (T, D, ", ".join("%s %.0f" % kv for kv in shares.items())))
    for what, share in shares.items():
        if what == "phase not advanced" and M % SM.period(rate, fc) == 0:
            continue                                        # (a block of whole carrier periods: holding the phase is no fault)
        if what == "history shifted at a block edge" and T <= D:
            assert M == D == T and share < 1                # (an output's T samples are its own D: the filter never reaches the history, nothing to plant)
            continue
        assert share > 1, what
