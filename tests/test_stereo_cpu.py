"""Stereo control without a device: ABI, every refusal of the supported range, the plan of csrc/fmd_resolve.c against the model's bit for bit, the
model's own properties (g = 1 the identity, g = 0 the fold with ties to even, the output between mid and input), the tracker's timeline, planted
defects that the exact comparisons of tests/test_gpu_stereo.py must catch on that file's own inputs, and - in float64 - the condition on the DDS
multiplex the end-to-end GPU test takes its thresholds from."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_model as M                   # noqa: E402
import stereo_e2e as E2E                   # noqa: E402

import rtl_fm_player_amd as R              # noqa: E402
from rtl_fm_player_amd import capi         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl_fm_player_amd", "csrc")


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build_library()


@pytest.fixture(scope="module")
def stereo_check():
    """tests/c/stereo_check.c over the private fmdk_stereo_plan: csrc/fmd_recv.c and fmd_error.c as sources, nothing of the device, under ASan and UBSan"""
    tmp = tempfile.mkdtemp(prefix="fmd_stereo_")
    exe = os.path.join(tmp, "stereo_check")
    subprocess.run(["cc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-g", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "c", "stereo_check.c"), os.path.join(CSRC, "fmd_recv.c"), os.path.join(CSRC, "fmd_error.c"), "-lm"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")     # (the leak checker needs ptrace, which not every sandbox grants)

    def ask(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
        return p.stdout.splitlines()
    yield ask
    shutil.rmtree(tmp, ignore_errors=True)


def f32_hex(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


def question(c):
    return "p %d %d %d %d %s %s %s %s %s %d %d %d" % (c["pcm_stride"], c["pilot_per_block"], c["hold_blocks"], c["reserved0"], f32_hex(c["pilot_on"]),
                                                      f32_hex(c["pilot_off"]), f32_hex(c["blend_lo"]), f32_hex(c["blend_hi"]), f32_hex(c["slew"]),
                                                      *c["reserved"])


def c_config(c):
    return R.FmdStereoConfig(c["pcm_stride"], c["pilot_per_block"], c["hold_blocks"], c["reserved0"], c["pilot_on"], c["pilot_off"], c["blend_lo"],
                             c["blend_hi"], c["slew"], (C.c_int32 * 3)(*c["reserved"]))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------------

NAMES = ["fmd_stereo_create", "fmd_batch_stereo_create", "fmd_stereo_destroy", "fmd_stereo_set_mode", "fmd_stereo_run_device", "fmd_stereo_run_host",
         "fmd_stereo_get_state", "fmd_stereo_set_state", "fmd_stereo_reset", "fmd_stereo_sync"]


def test_the_new_names_are_declared_exported_and_wrapped(stereo_check):
    hdr = open(os.path.join(ROOT, "include", "fmdemod_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = R.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert hasattr(L, n) and n in capi.exported_symbols(), n
        if n != "fmd_stereo_destroy":
            assert getattr(L, n).argtypes, n
    for n in ("FmdStereoConfig", "FmdStereoState", "STEREO_INFO_DTYPE", "STEREO_METER_DTYPE", "Stereo", "STEREO_AUTO", "STEREO_FORCE_MONO",
              "STEREO_FORCE_STEREO"):
        assert hasattr(R, n), n
    for meth in ("run_device", "run_host", "set_mode", "get_state", "set_state", "reset", "sync", "close"):
        assert callable(getattr(R.Stereo, meth)), meth
    assert callable(R.BatchDemod.stereo)
    assert (R.STEREO_AUTO, R.STEREO_FORCE_MONO, R.STEREO_FORCE_STEREO) == (0, 1, 2) == (M.AUTO, M.FORCE_MONO, M.FORCE_STEREO)
    assert (C.sizeof(R.FmdStereoConfig), C.sizeof(R.FmdStereoState), R.STEREO_INFO_DTYPE.itemsize, R.STEREO_METER_DTYPE.itemsize) == (48, 16, 32, 32)
    assert stereo_check(["s"])[0].split() == ["48", "16", "32", "32"]
    assert R.STEREO_INFO_DTYPE == M.INFO_DTYPE and R.STEREO_METER_DTYPE == M.METER_DTYPE
    for line in ("#define FMD_STEREO_AUTO 0", "#define FMD_STEREO_FORCE_MONO 1", "#define FMD_STEREO_FORCE_STEREO 2",
                 "typedef struct fmd_stereo_state  { float g; int32_t stereo, run, reserved; } fmd_stereo_state;",
                 "typedef struct fmd_stereo_info   { float pilot_ms, g_start, g_step, g_end; int32_t stereo, frames, reserved[2]; } fmd_stereo_info;",
                 "typedef struct fmd_stereo_meter  { int32_t peak_l, peak_r, full_scale, frames; uint64_t sumsq_l, sumsq_r; } fmd_stereo_meter;"):
        assert line in hdr, line


def code_of(name):
    """a csrc file without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, name)).read(), flags=re.S)


def test_the_kernels_live_in_the_receivers_unit_and_the_makefile_knows_it():
    assert '#include "stereo.inc"' in code_of("fmd_kernels_recv.hip") and "stereo.inc" not in code_of("fmd_kernels.inc")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^RDEPS = .*\bstereo\.inc\b", mk, re.M) and not re.search(r"^KDEPS = .*\bstereo\.inc\b", mk, re.M)
    assert re.search(r"^fmd_kernels_recv\.o: fmd_kernels_recv\.hip \$\(RDEPS\)$", mk, re.M) and len(re.findall(r"\$\(RDEPS\)", mk)) == 1
    assert "asm" not in code_of("stereo.inc") and "atomicAdd(float" not in open(os.path.join(CSRC, "stereo.inc")).read()
    for unit in ("fmd_recv.c", "fmd_resolve.c"):
        assert "hip" not in code_of(unit).lower(), unit


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------

GOOD = M.config()
REFUSALS = [
    (dict(pcm_stride=0), M.E_UNSUPPORTED), (dict(pcm_stride=4), M.E_UNSUPPORTED), (dict(pcm_stride=1028), M.E_UNSUPPORTED),
    (dict(pcm_stride=65544), M.E_UNSUPPORTED), (dict(pcm_stride=-8), M.E_UNSUPPORTED),
    (dict(pilot_per_block=-1), M.E_UNSUPPORTED), (dict(pilot_per_block=65537), M.E_UNSUPPORTED),
    (dict(hold_blocks=0), M.E_ARG), (dict(hold_blocks=-1), M.E_ARG), (dict(hold_blocks=(1 << 20) + 1), M.E_ARG),
    (dict(pilot_off=0.0), M.E_ARG), (dict(pilot_off=-0.05), M.E_ARG), (dict(pilot_off=0.2), M.E_ARG), (dict(pilot_on=np.inf), M.E_ARG),
    (dict(pilot_on=np.nan), M.E_ARG), (dict(pilot_off=np.nan), M.E_ARG),
    (dict(blend_lo=20.0), M.E_ARG), (dict(blend_lo=21.0), M.E_ARG), (dict(blend_hi=np.inf), M.E_ARG), (dict(blend_lo=-np.inf), M.E_ARG),
    (dict(blend_lo=np.nan), M.E_ARG), (dict(blend_hi=np.nan), M.E_ARG),
    (dict(slew=0.0), M.E_ARG), (dict(slew=-0.5), M.E_ARG), (dict(slew=1.0001), M.E_ARG), (dict(slew=np.nan), M.E_ARG), (dict(slew=np.inf), M.E_ARG),
    (dict(reserved0=1), M.E_ARG), (dict(reserved=(1, 0, 0)), M.E_ARG), (dict(reserved=(0, 0, 7)), M.E_ARG),
]
EDGES = [dict(pcm_stride=8), dict(pcm_stride=65536), dict(pilot_per_block=0), dict(pilot_per_block=65536), dict(hold_blocks=1), dict(hold_blocks=1 << 20),
         dict(pilot_off=0.1), dict(slew=1.0), dict(slew=2.0 ** -149), dict(blend_lo=-5.0, blend_hi=-4.5)]


def test_every_refusal_of_the_range_has_its_status_and_a_message(stereo_check):
    bad = [M.config(**kw) for kw, _ in REFUSALS]
    seen = set()
    for c, (kw, status), ans in zip(bad, REFUSALS, stereo_check([question(c) for c in bad])):
        f = ans.split(None, 2)
        assert f[0] == "refused" and int(f[1]) == status and len(f) == 3 and f[2], (kw, ans)
        seen.add(re.sub(r"\(got.*", "", f[2]))
        with pytest.raises(M.Refused) as e:
            M.plan(c)
        assert e.value.status == status, kw
        # the public call refuses the same way, before it looks for a device
        h = C.c_void_p(1)
        assert R.lib().fmd_stereo_create(C.byref(h), C.byref(c_config(c)), 1, -1) == status and not h.value and R.lib().fmd_last_error(), kw
    assert len(seen) == 7                           # reserved, stride, pilot_per_block, hold, thresholds, blend, slew: a message of its own each
    for kw in EDGES:
        assert stereo_check([question(M.config(**kw))])[0].split()[0] == "ok", kw
        M.plan(M.config(**kw))


def test_a_null_object_and_bad_create_arguments_are_refused_before_a_device_is_looked_for():
    L = R.lib()
    buf = (C.c_float * 64)()
    st = R.FmdStereoState()
    cc = c_config(GOOD)
    calls = [("set_mode", (0,)), ("run_device", (buf, buf, buf, None, 1, buf, buf, None, None)), ("run_host", (buf, buf, buf, None, 1, buf, buf, None)),
             ("get_state", (0, C.byref(st))), ("set_state", (0, C.byref(st))), ("reset", ()), ("sync", ())]
    for name, args in calls:
        assert L.fmd_dropin_set_math(99) == M.E_ARG
        marker = L.fmd_last_error()
        assert getattr(L, "fmd_stereo_" + name)(None, *args) == M.E_ARG and L.fmd_last_error() and L.fmd_last_error() != marker, name
    L.fmd_stereo_destroy(None)
    assert L.fmd_stereo_create(None, C.byref(cc), 1, -1) == M.E_ARG
    for n in (0, -1):
        h = C.c_void_p(1)
        assert L.fmd_stereo_create(C.byref(h), C.byref(cc), n, -1) == M.E_ARG and not h.value
    h = C.c_void_p(1)
    assert L.fmd_stereo_create(C.byref(h), None, 1, -1) == M.E_ARG and not h.value
    assert L.fmd_batch_stereo_create(None, None, None, C.byref(cc)) == M.E_ARG
    h = C.c_void_p(1)
    assert L.fmd_batch_stereo_create(C.byref(h), None, None, C.byref(cc)) == M.E_ARG and not h.value and b"batch" in L.fmd_last_error()


def test_create_of_a_valid_configuration_without_a_device_says_so():
    L = R.lib()
    h = C.c_void_p(1)
    rc = L.fmd_stereo_create(C.byref(h), C.byref(c_config(GOOD)), 1, -1)
    if R.device_count() > 0:
        assert rc == 0 and h.value
        L.fmd_stereo_destroy(h)
    else:
        assert rc == M.E_NODEVICE and b"no HIP device" in L.fmd_last_error() and not h.value


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------------

PLAN_CONFIGS = [M.config(), M.config(pilot_per_block=0), M.config(pilot_per_block=3), M.config(pilot_per_block=1000, pilot_on=0.0775, pilot_off=0.0774),
                M.config(pilot_per_block=65536, blend_lo=-3.3, blend_hi=7.1), M.config(pilot_on=1e-30, pilot_off=1e-38, blend_lo=0.1, blend_hi=0.3),
                M.config(pilot_on=3e20, pilot_off=1.0, blend_lo=-1e38, blend_hi=3e38), M.config(blend_lo=1.0, blend_hi=np.nextafter(np.float32(1), np.float32(2))),
                M.config(blend_lo=0.0, blend_hi=2.0 ** -149)] + [M.case_inputs(n)[0] for n in M.CASES]


def test_the_plan_equals_the_models_bit_for_bit(stereo_check):
    for c, ans in zip(PLAN_CONFIGS, stereo_check([question(c) for c in PLAN_CONFIGS])):
        pl = M.plan(c)
        assert ans.split() == ["ok"] + [f32_hex(pl[k]) for k in ("thr_on", "thr_off", "inv_mz", "inv_span")], (c, ans)
    assert M.plan(PLAN_CONFIGS[0])["thr_on"] == np.float32(np.float64(np.float32(0.1)) ** 2) and M.plan(PLAN_CONFIGS[1])["inv_mz"] == 0


# ---- the model's own properties ------------------------------------------------------------------------------------------------------------------

def rec(g_start, g_end, frames):
    r = np.zeros((), dtype=M.INFO_DTYPE)
    r["g_start"], r["g_end"], r["frames"] = g_start, g_end, frames
    r["g_step"] = np.float32(np.float32(np.float32(g_end) - np.float32(g_start)) / np.float32(frames)) if frames else 0
    return r


def pairs_slot():
    bp = M.boundary_pairs()
    rnd = np.random.default_rng(3).integers(-32768, 32768, size=(100000, 2)).astype(np.int16)
    return np.concatenate([bp, rnd]).reshape(-1)


def test_fma32_rounds_once():
    """against exact rational arithmetic, on operands built to sit at and beside the half-way points where a float64 detour rounds twice"""
    from fractions import Fraction
    rng = np.random.default_rng(1)
    a = rng.standard_normal(4000).astype(np.float32)
    b = (rng.standard_normal(4000) * 1000).astype(np.float32)
    c = (rng.standard_normal(4000) * 30000).astype(np.float32)
    # ties on the float32 grid of the SUM: a big c, and a b = half an ulp of c, a little more, a little less
    big = np.float32(2.0 ** 20)
    a2 = np.array([2.0 ** -5, 2.0 ** -5, -(2.0 ** -5), 2.0 ** -5 + 2.0 ** -28, 2.0 ** -5 - 2.0 ** -29], dtype=np.float32)     # ulp(2^20) = 2^-3: half = 2^-4
    b2 = np.array([2.0, 2.0 + 2.0 ** -22, 2.0, 2.0, 2.0], dtype=np.float32)
    c2 = np.array([big, big, big + np.float32(0.125), big, big + np.float32(0.125)], dtype=np.float32)
    a, b, c = np.concatenate([a, a2]), np.concatenate([b, b2]), np.concatenate([c, c2])
    got = M.fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        err = abs(Fraction(float(g)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), (x, y, z, g)
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):       # a true tie: even
            assert int(g.view(np.uint32)) % 2 == 0, (x, y, z, g)
    assert got[-4] == big + np.float32(0.125) and got[-5] == big        # just above the half-way point goes up; the exact tie goes to even
    # a b = 2^-4 - 2^-40: the float64 sum with 2^20 + 2^-3 rounds ONTO the half-way point and a second rounding would go to even, 2^20 + 2^-2
    x, y = np.float32(2.0 ** -5 * (1 + 2.0 ** -18)), np.float32(2.0 * (1 - 2.0 ** -18))
    assert np.float64(x) * np.float64(y) == 2.0 ** -4 - 2.0 ** -40
    assert M.fma32(x, y, big + np.float32(0.125)) == big + np.float32(0.125)
    assert np.float32(np.float64(x) * np.float64(y) + np.float64(big + np.float32(0.125))) == big + np.float32(0.25)


def test_g_1_is_the_identity_and_g_0_folds_with_ties_to_even():
    slot = pairs_slot()
    n = slot.size // 2
    out, meter = M.apply(slot, rec(1.0, 1.0, n))
    assert np.array_equal(out, slot)
    assert meter["frames"] == n and meter["peak_l"] == 32768 and meter["full_scale"] >= 2 * 2 * 7
    out, _ = M.apply(slot, rec(0.0, 0.0, n))
    L, Rr = slot[0::2].astype(np.int64), slot[1::2].astype(np.int64)
    tot = L + Rr
    want = np.where(tot % 2 == 0, tot // 2, np.where(((tot - 1) // 2) % 2 == 0, (tot - 1) // 2, (tot + 1) // 2))     # half of an odd sum: to the even neighbour
    assert np.array_equal(out[0::2], want) and np.array_equal(out[1::2], want)
    assert (tot % 2 != 0).sum() > 1000


@pytest.mark.parametrize("g0,g1", [(0.0, 1.0), (1.0, 0.0), (0.3, 0.3), (0.9, 0.25)])
def test_the_output_lies_between_mid_and_input(g0, g1):
    slot = pairs_slot()
    n = slot.size // 2
    out, _ = M.apply(slot, rec(g0, g1, n))
    for ch in (0, 1):
        x = slot[ch::2].astype(np.float64)
        m = 0.5 * (slot[0::2].astype(np.float64) + slot[1::2].astype(np.float64))
        lo, hi = np.rint(np.minimum(m, x)), np.rint(np.maximum(m, x))
        y = out[ch::2].astype(np.float64)
        assert ((y >= lo) & (y <= hi)).all()
    assert np.array_equal(out[2 * n:], slot[2 * n:])


def test_what_lies_beyond_the_frames_is_copied():
    slot = pairs_slot()[:1024]
    for frames in (0, 1, 3, 511):
        out, meter = M.apply(slot, rec(0.0, 0.0, frames))
        assert np.array_equal(out[2 * frames:], slot[2 * frames:]) and meter["frames"] == frames
    assert not np.array_equal(M.apply(slot, rec(0.0, 0.0, 511))[0][:1022], slot[:1022])


# ---- the tracker ------------------------------------------------------------------------------------------------------------------------------

def test_hysteresis_and_hold_on_a_written_out_timeline():
    c = M.config(hold_blocks=2, slew=1.0)                  # thr_on 0.01, thr_off 0.0025
    pl = M.plan(c)
    #        0     1     2     3     4      5      6      7      8      9      10    11   12    13
    pilot = [0.0, 0.02, 0.02, 0.02, 0.005, 0.005, 0.005, 0.001, 0.001, 0.001, 0.02, 0.0, 0.02, 0.02]
    want = [0,    0,    1,    1,    1,     1,     1,     1,     0,     0,     0,    0,   0,    1]
    lens = np.full(len(pilot), 1024, dtype=np.int32)
    info, st = M.track(c, pl, M.new_state(), lens, np.array(pilot, dtype=np.float32), None, M.AUTO)
    assert list(info["stereo"]) == want
    assert list(info["g_end"]) == [float(w) for w in want] and list(info["g_start"]) == [0.0] + [float(w) for w in want[:-1]]
    assert st == dict(g=np.float32(1), stereo=1, run=0)
    # hold_blocks ignored: on at block 1, off at block 7, on again for the single block 10
    info1, _ = M.track(c, pl, M.new_state(), lens, np.array(pilot, dtype=np.float32), None, M.AUTO, defect="ignore_hold")
    assert list(info1["stereo"]) == [0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 0, 1, 1]
    # the split into launches changes nothing
    a, st = M.track(c, pl, M.new_state(), lens[:5], np.array(pilot[:5], dtype=np.float32), None, M.AUTO)
    b, st = M.track(c, pl, st, lens[5:], np.array(pilot[5:], dtype=np.float32), None, M.AUTO)
    assert np.array_equal(np.concatenate([a, b]), info)


def test_closed_blocks_hold_the_state_and_nan_reads_as_absent():
    c = M.config(hold_blocks=2, slew=0.25)
    pl = M.plan(c)
    lens = np.array([1024, 1024, 0, -5, 1, 1024, 1024, 1024], dtype=np.int32)
    pilot = np.array([0.02, 0.02, 0.0, 0.0, 0.0, 0.02, np.nan, np.nan], dtype=np.float32)
    qual = np.array([25.0, 25.0, 25.0, 25.0, 25.0, np.nan, 25.0, 25.0], dtype=np.float32)
    info, st = M.track(c, pl, M.new_state(), lens, pilot, qual, M.AUTO)
    assert list(info["frames"]) == [512, 512, 0, 0, 0, 512, 512, 512]
    assert list(info["stereo"]) == [0, 1, 1, 1, 1, 1, 1, 0]               # zero pilot in closed blocks (and one of a single value: no frame) changes nothing
    assert list(info["g_end"]) == [0.0, 0.25, 0.25, 0.25, 0.25, 0.0, 0.25, 0.0]    # slew 0.25 per block; NaN quality reads 0; NaN pilot counts towards off
    assert list(info["g_step"][2:5]) == [0.0, 0.0, 0.0] and info["g_step"][1] == np.float32(0.25) / np.float32(512)
    assert st["run"] == 0 and st["stereo"] == 0


def test_slew_limits_g_per_block_and_the_forced_modes_need_no_pilot():
    c = M.config(hold_blocks=1, slew=0.3)
    pl = M.plan(c)
    lens = np.full(6, 1024, dtype=np.int32)
    info, st = M.track(c, pl, M.new_state(), lens, None, None, M.FORCE_STEREO)
    g = np.float32(0)
    for b in range(6):
        g = min(np.float32(g + np.float32(0.3)), np.float32(1)) if np.float32(1) - g > np.float32(0.3) else np.float32(g + np.float32(np.float32(1) - g))
        assert info["g_end"][b] == g and not info["pilot_ms"][b] and not info["stereo"][b]
    assert info["g_end"][-1] == 1 and np.all(np.abs(np.diff(np.concatenate([[0], info["g_end"]]))) <= np.float32(0.3) + 1e-7)
    info, st = M.track(c, pl, st, lens, None, None, M.FORCE_MONO)
    assert info["g_end"][-1] == 0 and info["g_start"][0] == 1
    # blend: quality 14 against 10 .. 20 is 0.4
    info, _ = M.track(M.config(hold_blocks=1, slew=1.0), pl, M.new_state(), lens[:1], np.array([1.0], dtype=np.float32), np.array([14.0], dtype=np.float32), M.AUTO)
    assert info["g_end"][0] == np.float32(np.float32(4.0) * np.float32(0.1)) and info["stereo"][0] == 1


# ---- planted defects on the GPU tests' own inputs ------------------------------------------------------------------------------------------------

def model_case(name, defect=None):
    c, pcm, lens, z, qual = M.case_inputs(name)
    pl = M.plan(c)
    S, B = lens.shape
    pilot = np.array([[M.pilot_ms(z[s, b], pl["inv_mz"], defect) for b in range(B)] for s in range(S)], dtype=np.float32)
    states = [M.new_state() for _ in range(S)]
    return M.run(c, states, pcm, lens, pilot, qual, M.AUTO, defect), states


def test_the_cases_drive_g_through_its_range():
    (out, info, meter), _ = model_case("sweep")
    t = np.float32(np.float32(4.0) * np.float32(0.1))
    assert list(info["g_end"][0]) == [1.0, np.float32(1) + np.float32(t - np.float32(1)), 0.0, 1.0, 1.0] and list(info["stereo"][0]) == [1, 1, 0, 1, 1]
    c, pcm, lens, _, _ = M.case_inputs("sweep")
    assert np.array_equal(out[0, 4], pcm[0, 4]) and not np.array_equal(out[0, 0], pcm[0, 0])       # g = 1 throughout: the identity
    (out, info, meter), states = model_case("hold")
    assert list(info["stereo"][0]) == [0, 1, 1, 1, 1] and list(info["g_end"][0][:3]) == [0.0, 0.5, 0.75]
    assert states[0]["run"] == 1                          # the pilot's loss in the last block has begun to count
    assert 0.3 < info["g_end"][0][3] < 0.5 and 0.8 < info["g_end"][0][4] < 1.0          # 0.4, then half way back up


@pytest.mark.parametrize("defect", [d for d in M.DEFECTS if d != "drop_last"])
def test_a_planted_defect_changes_the_models_output_on_the_gpu_cases(defect):
    changed = []
    for name in M.CASES:
        (o0, i0, m0), _ = model_case(name)
        (o1, i1, m1), _ = model_case(name, defect)
        if defect == "meter_input":
            assert np.array_equal(o0, o1)
            if m0.tobytes() != m1.tobytes():
                changed.append(name)
        elif not np.array_equal(o0, o1):
            changed.append(name)
    print(defect, "changes", changed)
    assert "hold" in changed and (defect == "ignore_hold" or "sweep" in changed), changed


def test_dropping_the_last_threads_partial_changes_pilot_ms_from_256_values_on():
    for mz in E2E.PILOT_SIZES:
        z = M.pilot_z(1, 1, mz, [[0.3]], seed=mz)[0, 0]
        inv = M.plan(M.config(pilot_per_block=mz))["inv_mz"]
        a, b = M.pilot_ms(z, inv), M.pilot_ms(z, inv, "drop_last")
        assert (a != b) == (mz >= 256), mz
        exact = M.pilot_ms_f64(z)
        assert abs(float(a) - exact) <= M.pilot_bound(mz, exact), mz
        if mz >= 256:
            assert abs(float(b) - exact) > M.pilot_bound(mz, exact), mz      # ... and leaves the bound by orders of magnitude
    assert "hold" in M.CASES and M.CASES["hold"][0]["pilot_per_block"] >= 256
    (o0, i0, _), _ = model_case("hold")
    (o1, i1, _), _ = model_case("hold", "drop_last")
    assert not np.array_equal(i0["pilot_ms"], i1["pilot_ms"])


# ---- the end-to-end condition, in float64 --------------------------------------------------------------------------------------------------------

def test_the_dds_multiplex_with_and_without_pilot_differs_by_a_factor_of_100():
    on, off = E2E.pilot_ms_f64_of_dds(1), E2E.pilot_ms_f64_of_dds(0)
    print("pilot_ms per block: stereo=1", on, "stereo=0", off)
    assert on.min() >= 100.0 * off.max(), (on, off)
    p_on, p_off = E2E.thresholds()
    assert off.max() < p_off ** 2 < p_on ** 2 < on.min()
