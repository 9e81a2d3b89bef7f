"""The station finder without a device: ABI, every refusal of the supported range, the plan of csrc/fmd_resolve.c against the model's bit for bit,
the decision margins of the GPU file's cases (a condition on the inputs, taken from the model alone), planted defects the comparison must catch,
and - with the float64 spectrum and tuner models - the DC spike and the end-to-end expectation tests/test_gpu_scan.py asserts on the device."""
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
import scan_model as M                     # noqa: E402
import spectrum_model as SM                # noqa: E402
import tuner_model as TM                   # noqa: E402

import rtl_fm_player_amd as R              # noqa: E402
from rtl_fm_player_amd import capi         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl_fm_player_amd", "csrc")


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build_library()


@pytest.fixture(scope="module")
def scan_check():
    """tests/c/scan_check.c over the private fmdk_scan_plan_make: csrc/fmd_recv.c and fmd_error.c as sources, nothing of the device, under ASan and UBSan"""
    tmp = tempfile.mkdtemp(prefix="fmd_scan_")
    exe = os.path.join(tmp, "scan_check")
    subprocess.run(["cc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-g", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "c", "scan_check.c"), os.path.join(CSRC, "fmd_recv.c"), os.path.join(CSRC, "fmd_error.c"), "-lm"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")     # (the leak checker needs ptrace, which not every sandbox grants)

    def ask(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
        return p.stdout.splitlines()
    yield ask
    shutil.rmtree(tmp, ignore_errors=True)


def f32_hex(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


def f64_hex(x):
    return "%016x" % int(np.float64(x).view(np.uint64))


def question(cfg):
    return "p %d %d %d %d %d %d %d %d %s %d %d %d" % (cfg["rate"], cfg["n_bins"], cfg["raster_hz"], cfg["bw"], cfg["min_sep"], cfg["floor_permille"],
                                                      cfg["dc_guard"], cfg["max_stations"], f32_hex(cfg["threshold"]), *cfg["reserved"])


def c_config(cfg):
    return R.FmdScanConfig(cfg["rate"], cfg["n_bins"], cfg["raster_hz"], cfg["bw"], cfg["min_sep"], cfg["floor_permille"], cfg["dc_guard"],
                           cfg["max_stations"], cfg["threshold"], (C.c_int32 * 3)(*cfg["reserved"]))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------------

NAMES = ["fmd_scan_candidates", "fmd_scan_create", "fmd_batch_scan_create", "fmd_scan_destroy", "fmd_scan_run_device", "fmd_scan_run_host", "fmd_scan_sync"]


def test_the_new_names_are_declared_exported_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "fmdemod_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = R.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert hasattr(L, n) and n in capi.exported_symbols(), n
    for n in ("FmdScanConfig", "FmdScanStation", "Scan", "scan_candidates", "SCAN_STATION_DTYPE"):
        assert hasattr(R, n), n
    assert hasattr(R.BatchDemod, "scan")
    assert C.sizeof(R.FmdScanConfig) == 48 and C.sizeof(R.FmdScanStation) == 32 and R.SCAN_STATION_DTYPE.itemsize == 32 == M.STATION_DTYPE.itemsize
    assert [f[0] for f in R.FmdScanStation._fields_] == list(M.STATION_DTYPE.names)
    for line in ("#define FMD_SCAN_MAX_BINS 4096", "#define FMD_SCAN_MAX_CANDIDATES 1024", "#define FMD_SCAN_MAX_STATIONS 64",
                 "typedef struct fmd_scan_config  { int32_t rate, n_bins, raster_hz, bw, min_sep, floor_permille, dc_guard, max_stations; float threshold; "
                 "int32_t reserved[3]; } fmd_scan_config;",
                 "typedef struct fmd_scan_station { int32_t offset_hz, candidate; float power, snr, centroid_hz; int32_t reserved[3]; } fmd_scan_station;"):
        assert line in hdr, line


def code_of(name):
    """a csrc file without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, name)).read(), flags=re.S)


def test_the_kernel_lives_in_the_receivers_unit_and_the_makefile_knows_it():
    assert '#include "scan.inc"' in code_of("fmd_kernels_recv.hip") and "scan.inc" not in code_of("fmd_kernels.inc")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^RDEPS = .*\bscan\.inc\b", mk, re.M) and not re.search(r"^KDEPS = .*\bscan\.inc\b", mk, re.M)
    assert re.search(r"^fmd_kernels_recv\.o: fmd_kernels_recv\.hip \$\(RDEPS\)$", mk, re.M) and len(re.findall(r"\$\(RDEPS\)", mk)) == 1
    for unit in ("fmd_recv.c", "fmd_resolve.c"):
        assert "hip" not in code_of(unit).lower(), unit


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------

GOOD = M.config(**M.G256)
REFUSALS = [
    (dict(rate=0), M.E_ARG), (dict(rate=-2400000), M.E_ARG),
    (dict(n_bins=32), M.E_UNSUPPORTED), (dict(n_bins=8192), M.E_UNSUPPORTED), (dict(n_bins=1000), M.E_UNSUPPORTED), (dict(n_bins=0), M.E_UNSUPPORTED),
    (dict(raster_hz=0), M.E_ARG), (dict(raster_hz=-100000), M.E_ARG),
    (dict(bw=0), M.E_ARG), (dict(bw=-5), M.E_ARG), (dict(bw=4687), M.E_ARG),            # rate / n_bins = 9375 > 2 bw
    (dict(bw=1200000), M.E_ARG), (dict(bw=1196000), M.E_ARG),                           # no channel fits: cmax < 0
    (dict(n_bins=4096, raster_hz=2000, bw=1000), M.E_UNSUPPORTED),                      # C = 1199
    (dict(min_sep=0), M.E_ARG), (dict(min_sep=22), M.E_ARG),
    (dict(floor_permille=-1), M.E_ARG), (dict(floor_permille=1001), M.E_ARG),
    (dict(dc_guard=-1), M.E_ARG), (dict(dc_guard=65), M.E_ARG),
    (dict(max_stations=0), M.E_ARG), (dict(max_stations=65), M.E_ARG),
    (dict(threshold=0.0), M.E_ARG), (dict(threshold=-1.0), M.E_ARG), (dict(threshold=np.inf), M.E_ARG), (dict(threshold=np.nan), M.E_ARG),
    (dict(reserved=(1, 0, 0)), M.E_ARG), (dict(reserved=(0, 0, 7)), M.E_ARG),
]


def test_every_refusal_of_the_range_has_its_status_and_a_message(scan_check):
    bad = [dict(GOOD, **kw) for kw, _ in REFUSALS]
    for cfg, (kw, status), ans in zip(bad, REFUSALS, scan_check([question(c) for c in bad])):
        f = ans.split(None, 2)
        assert f[0] == "refused" and int(f[1]) == status and len(f) == 3 and f[2], (kw, ans)
        with pytest.raises(M.Refused) as e:
            M.plan(cfg)
        assert e.value.status == status, kw
        # the public calls refuse the same way, before they look for a device
        cc = c_config(cfg)
        assert R.lib().fmd_scan_candidates(C.byref(cc)) == status and R.lib().fmd_last_error(), kw
        h = C.c_void_p()
        assert R.lib().fmd_scan_create(C.byref(h), C.byref(cc), 1, -1) == status and not h.value, kw
    assert R.lib().fmd_scan_candidates(None) == M.E_ARG
    # the edges of the range are inside it
    for kw in (dict(bw=4688), dict(min_sep=21), dict(dc_guard=64), dict(max_stations=64), dict(max_stations=1), dict(floor_permille=0),
               dict(floor_permille=1000), dict(n_bins=64, bw=18750), dict(n_bins=4096, raster_hz=2500, bw=1000)):
        assert R.scan_candidates(c_config(dict(GOOD, **kw))) == M.plan(dict(GOOD, **kw))["C"], kw


def test_run_refuses_without_an_object():
    L = R.lib()
    assert L.fmd_scan_run_device(None, None, 1, None, None, None, None) == M.E_ARG
    assert L.fmd_scan_run_host(None, None, 1, None, None, None) == M.E_ARG
    assert L.fmd_scan_sync(None) == M.E_ARG
    L.fmd_scan_destroy(None)
    if R.device_count() == 0:
        with pytest.raises(R.FmdError, match="no HIP device"):
            R.Scan(c_config(GOOD), 1)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------------

PLAN_CONFIGS = [M.config(**M.G64), M.config(**M.G256), M.config(dc_guard=3, **M.G4096), M.config(**M.WIDE), M.config(**M.T256),
                M.config(256000, 64, 10000, 120000),                         # C = 1
                M.config(2400000, 1024, 100000, 100000, dc_guard=2, floor_permille=999),
                M.config(2400000, 256, 5000, 4688, max_stations=64),         # a band of one bin and a bit: counts of 2 and 3
                M.config(2048000, 4096, 3000, 777, floor_permille=1, dc_guard=1024),
                M.config(1000003, 128, 7919, 50021), M.config(2147483647, 4096, 5000000, 300000)]


def test_the_plan_equals_the_models_bit_for_bit(scan_check):
    for cfg, ans in zip(PLAN_CONFIGS, scan_check([question(c) for c in PLAN_CONFIGS])):
        pl = M.plan(cfg)
        f = ans.split()
        assert f[0] == "ok", ans
        assert [int(x) for x in f[1:5]] == [pl["C"], pl["cmax"], pl["rank"], pl["n_used"]], cfg
        assert f[5] == f64_hex(pl["nb"]), cfg
        rest = f[6:]
        assert len(rest) == 4 * pl["C"]
        for i in range(pl["C"]):
            assert [int(rest[4 * i]), int(rest[4 * i + 1])] == [pl["first"][i], pl["count"][i]], (cfg, i)
            assert rest[4 * i + 2:4 * i + 4] == [f64_hex(pl["w_first"][i]), f64_hex(pl["w_last"][i])], (cfg, i)
    assert M.plan(PLAN_CONFIGS[5])["C"] == 1


def test_the_plan_is_what_the_definition_says():
    """independently of the integer formulas: the weights are the overlaps, they add up to the channel's bins, every band lies inside
    +-(rate / 2 - D / 2) and bin -N/2 is in no channel, and one more candidate would not fit"""
    for cfg in PLAN_CONFIGS:
        pl = M.plan(cfg)
        Rr, N = cfg["rate"], cfg["n_bins"]
        D = Rr / N
        assert (pl["cmax"] + 1) * cfg["raster_hz"] + cfg["bw"] > Rr / 2 - D / 2 >= pl["cmax"] * cfg["raster_hz"] + cfg["bw"]
        for i in range(pl["C"]):
            ctr = (i - pl["cmax"]) * cfg["raster_hz"]
            s0, n = pl["first"][i], pl["count"][i]
            assert -N // 2 < s0 and s0 + n - 1 < N // 2 and n >= 1
            w = np.ones(n)
            w[0], w[-1] = pl["w_first"][i], pl["w_last"][i]
            s = s0 + np.arange(n)
            overlap = np.minimum((s + 0.5) * D, ctr + cfg["bw"]) - np.maximum((s - 0.5) * D, ctr - cfg["bw"])
            assert np.all(w > 0) and np.all(w <= 1) and np.all(w[1:-1] == 1) and np.allclose(w, overlap / D, rtol=0, atol=1e-9)
            assert abs(w.sum() - pl["nb"]) <= 1e-9 * pl["nb"]


# ---- the cases of the GPU file -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", M.CASES, ids=[c[0] for c in M.CASES])
def test_the_cases_have_decision_margins(case):
    """Every decision of a GPU case is at least 1e-6 (relative) from its threshold: the device's doubles differ from the model's by at most
    (n_c + 2) 2^-53 relative (n_c <= 4096 bins a channel: 5e-13), so no decision can differ.  Exact ties, decided by the index on any arithmetic, are
    the exception, and only the cases built for them have any."""
    name, cfg, n_blocks, n_streams, kind, ties_expected = case
    power = M.case_power(kind, cfg, n_blocks, n_streams)
    assert power.shape == (n_streams, n_blocks, cfg["n_bins"]) and np.all(np.isfinite(power)) and np.all(power >= 0)
    if n_streams > 1 and kind != "zeros":
        assert all(not np.array_equal(power[0], power[s]) for s in range(1, n_streams))
    total_ties = 0
    for res in M.scan(power, cfg):
        occ, order, ties = M.margins(res, cfg)
        assert occ >= 1e-6 and order >= 1e-6, (name, occ, order)
        total_ties += ties
    assert (total_ties > 0) == ties_expected, (name, total_ties)


def test_the_cases_reach_what_they_are_for():
    by = {c[0]: c for c in M.CASES}

    def run(name):
        _, cfg, b, s, kind, _ = by[name]
        return cfg, M.scan(M.case_power(kind, cfg, b, s), cfg)
    assert {c[1]["n_bins"] for c in M.CASES} >= {64, 256, 4096} and {c[2] for c in M.CASES} == {1, 3} and {c[3] for c in M.CASES} == {1, 5}
    assert {c[1]["min_sep"] for c in M.CASES} >= {1, 3} and {c[1]["dc_guard"] for c in M.CASES} >= {0, 1, 3}
    assert {c[1]["floor_permille"] for c in M.CASES} >= {0, 250, 1000}
    cfg, res = run("n64 b1 s1")                          # the band's ends, fractional edge weights
    assert {0, res[0]["plan"]["C"] - 1} <= set(res[0]["order"]) and 0 < res[0]["plan"]["w_first"][0] < 1
    for name in ("n64 overflow", "n4096 wide overflow b3"):
        cfg, res = run(name)
        assert any(r["found"] > r["written"] == cfg["max_stations"] for r in res), name
    cfg, res = run("n256 b3 s1 floor1000")
    assert res[0]["found"] >= 1
    cfg, res = run("zeros")
    assert all(r["found"] == 0 and not r["stations"].tobytes().strip(b"\0") for r in res)
    cfg, res = run("sparse")
    assert all(r["F"] == 0 and r["found"] >= 2 and np.all(np.isposinf(r["stations"]["snr"][:r["written"]])) for r in res)
    cfg, res = run("plateau")                            # eight equal candidates: the first one is the station, none of the others
    assert len(set(res[0]["Pc"][40:48])) == 1 and res[0]["order"] == [40, 90]
    for name, ms in (("ties sep3 b3", 3), ("ties sep1 b1", 1)):
        cfg, res = run(name)
        for r in res:                                    # min_sep apart: the lower one; min_sep + 1 apart: both, the lower one first; a shared bin: the lower one
            assert r["Pc"][10] == r["Pc"][10 + ms] == r["Pc"][50] == r["Pc"][50 + ms + 1] and r["Pc"][100] == r["Pc"][101] and r["Pc"][0] == r["Pc"][126]
            assert r["order"] == [0, 126, 10, 50, 50 + ms + 1, 100], (name, r["order"])
    cfg, res = run("n4096 wide sep3")
    assert res[0]["plan"]["C"] == 959


def device_view(res):
    return res["stations"], np.array([res["found"], res["written"]], np.int32), res["chan"]


def test_the_comparison_passes_the_model_and_refuses_each_planted_defect():
    """assert_matches - what tests/test_gpu_scan.py holds the device to - accepts the model's own result on every case and refuses, on at least one
    case, a model with: the bins off by one, the guard ignored, the tie rule reversed, the suppression window one short, the floor's rank taken over
    all bins instead of the used ones, bin -N/2 counted."""
    caught = {d: [] for d in M.DEFECTS}
    for name, cfg, b, s, kind, _ in M.CASES:
        if cfg["n_bins"] == 4096 and kind != "stations_dc":
            continue                                     # (the wide cases add nothing here and cost the model seconds per defect)
        power = M.case_power(kind, cfg, b, s)
        good = M.scan(power, cfg)
        for r in good:
            M.assert_matches(r, *device_view(r), cfg, name)
        for d in M.DEFECTS:
            try:
                bad = M.scan(power, cfg, d)
            except M.Refused:
                continue
            for r, w in zip(good, bad):
                try:
                    if w["chan"].shape != r["chan"].shape:
                        raise AssertionError("another number of candidates")
                    M.assert_matches(r, *device_view(w), cfg, name)
                except AssertionError:
                    caught[d].append(name)
                    break
    assert all(caught[d] for d in M.DEFECTS), {d: len(v) for d, v in caught.items()}


# ---- a capture: the DC spike, and the end-to-end chain in float64 ------------------------------------------------------------------------------

def capture_power(iq, n_bins, block_len=M.CAPTURE_BLOCK_LEN):
    return np.stack([SM.spectrum_f64(iq[a:a + block_len], n_bins, SM.WINDOW_HANN) for a in range(0, iq.size, block_len)]).astype(np.float32)


@pytest.mark.parametrize("n_bins", [256, 1024, 4096])
def test_the_dc_spike_is_a_station_without_the_guard_and_none_with_it(n_bins):
    iq = M.capture_bytes()
    power = capture_power(iq, n_bins)
    planted = sorted(f for f, _ in M.CAPTURE_CARRIERS)
    for guard, want in ((0, sorted(planted + [0])), (2, planted)):
        cfg = M.capture_config(n_bins, guard)
        res = M.scan_stream(power, cfg)
        got = res["stations"][:res["written"]]
        assert sorted(int(x) for x in got["offset_hz"]) == want, (n_bins, guard, got)
        occ, order, ties = M.margins(res, cfg)
        assert occ >= 1e-6 and order >= 1e-6 and ties == 0
        for st in got:
            if st["offset_hz"] != 0:
                assert abs(float(st["centroid_hz"]) - int(st["offset_hz"])) < 5000, st
    strongest = M.scan_stream(power, M.capture_config(n_bins, 2))["stations"][0]
    assert strongest["offset_hz"] == 300000


E2E_STEP, E2E_TUNER_BW, E2E_TAPS = 1000, 120000, 64


def test_end_to_end_in_the_models():
    """What tests/test_gpu_scan.py asserts of the device chain, shown here with the float64 models: spectrum -> scan finds the planted offsets,
    fmd_tuner_shift of the first station (offset_tuning) feeds the tuner, and the tuner's output through spectrum and scan has its first station at
    offset 0."""
    iq = M.capture_bytes()
    cfg = M.capture_config(256, 2)
    first = M.scan_stream(capture_power(iq, 256), cfg)
    assert [int(x) for x in first["stations"]["offset_hz"][:first["written"]]] == [300000, -500000, 900000]
    shift = TM.shift_steps(M.CAPTURE_RATE, E2E_STEP, int(first["stations"]["offset_hz"][0]), True)
    assert shift == -300
    tc = R.FmdTunerConfig(M.CAPTURE_RATE, E2E_STEP, E2E_TUNER_BW, E2E_TAPS, M.CAPTURE_BLOCK_LEN, 0)
    assert R.tuner_shift(tc, 300000, True) == shift
    taps = R.tuner_design(tc)
    y, _ = TM.tuner_f32(iq, taps, M.CAPTURE_RATE // E2E_STEP, shift)
    out = TM.quantise_f32(y, 1.0)
    second = M.scan_stream(capture_power(out, 256), cfg)
    assert second["found"] >= 1 and second["stations"]["offset_hz"][0] == 0 and second["stations"]["candidate"][0] == second["plan"]["cmax"]
    occ, order, ties = M.margins(second, cfg)
    assert occ >= 1e-6 and order >= 1e-6 and ties == 0
