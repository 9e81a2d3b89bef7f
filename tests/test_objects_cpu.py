"""What the batch and the receiver objects beside it share (csrc/fmd_dev.c), without a device: every entry point refuses a NULL object with
FMD_E_ARG and a message, and every *_create refuses a NULL `out`, a non-positive count and non-finite taps before it looks for a device - on a
machine without one a valid configuration then gets FMD_E_NODEVICE and leaves *out NULL.  One table over batch, subc, tuner, scan and rds; each
object's own module holds its configuration ranges."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import rtl_fm_player_amd as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_model as M  # noqa: E402

FMD_E_ARG, FMD_E_NODEVICE = -1, -5
BUF = (C.c_float * 1024)()                              # 16-byte aligned or not: the NULL object is refused first


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build_library()


def scan_config():
    c = M.config(**M.G64)
    return R.FmdScanConfig(c["rate"], c["n_bins"], c["raster_hz"], c["bw"], c["min_sep"], c["floor_permille"], c["dc_guard"], c["max_stations"],
                           c["threshold"], (C.c_int32 * 3)(0, 0, 0))


# kind: (a valid configuration, its state struct or None, the run_device and run_host arguments behind the object, how many counts the create takes,
#        whether it takes taps as float32 [cfg.n_taps])
KINDS = {
    "batch": (lambda: R.wbfm_config(), R.FmdStreamState, (BUF, 1, BUF, BUF, None), (BUF, 1, BUF, BUF), 1, False),
    "subc": (lambda: R.FmdSubcConfig(300000, 57000, 2400, 128, 16, 512), R.FmdSubcState, (BUF, 1, BUF, None), (BUF, 1, BUF), 1, True),
    "tuner": (lambda: R.FmdTunerConfig(2400000, 1000, 100000, 64, 16384, 0), R.FmdTunerState, (BUF, 1, BUF, None, None), (BUF, 1, BUF), 2, True),
    "scan": (scan_config, None, (BUF, 1, BUF, BUF, None, None), (BUF, 1, BUF, BUF, None), 1, False),
    "rds": (lambda: R.FmdRdsConfig(18750, 1024, 64, 8, 4), R.FmdRdsState, (BUF, 1, BUF, BUF, None, None, None), (BUF, 1, BUF, BUF, None, None), 1, True),
}


def create(L, kind, out, cfg, counts, taps=None):
    """fmd_<kind>_create(out, cfg, [taps,] counts..., device -1)"""
    args = [out, C.byref(cfg)]
    if kind == "batch" or KINDS[kind][5]:
        args.append(taps)
    return getattr(L, "fmd_%s_create" % kind)(*args, *counts, -1)


def refused(L, rc, marker):
    """FMD_E_ARG, with a message of its own in fmd_last_error"""
    return rc == FMD_E_ARG and L.fmd_last_error() and L.fmd_last_error() != marker


def mark(L):
    """leave a known text in fmd_last_error, so that the next refusal's can be told from a stale one"""
    assert L.fmd_dropin_set_math(99) == FMD_E_ARG
    return L.fmd_last_error()


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_null_object_is_refused_by_every_entry_point(kind):
    L = R.lib()
    _, state, dev_args, host_args, _, _ = KINDS[kind]
    calls = [("sync", ()), ("run_device", dev_args), ("run_host", host_args)]
    if state is not None:
        st = state()
        calls += [("reset", ()), ("get_state", (0, C.byref(st))), ("set_state", (0, C.byref(st)))]
    for name, args in calls:
        marker = mark(L)
        assert refused(L, getattr(L, "fmd_%s_%s" % (kind, name))(None, *args), marker), name
    getattr(L, "fmd_%s_destroy" % kind)(None)


def test_the_lookup_getters_refuse_a_null_object():
    L = R.lib()
    for name in ("fmd_subc_out_per_block", "fmd_rds_bits_per_block", "fmd_batch_pcm_stride", "fmd_batch_n_streams"):
        assert getattr(L, name)(None) == FMD_E_ARG, name


@pytest.mark.parametrize("kind", list(KINDS))
def test_create_refuses_bad_arguments_before_it_looks_for_a_device(kind):
    L = R.lib()
    cfg, n_counts, has_taps = KINDS[kind][0](), KINDS[kind][4], KINDS[kind][5]
    marker = mark(L)
    assert refused(L, create(L, kind, None, cfg, (1,) * n_counts), marker), "out == NULL"
    for bad in (0, -1):
        for which in range(n_counts):
            counts = tuple(bad if i == which else 1 for i in range(n_counts))
            h = C.c_void_p(1)
            marker = mark(L)
            assert refused(L, create(L, kind, C.byref(h), cfg, counts), marker) and not h.value, counts
    if has_taps:
        for value in (np.nan, np.inf):
            taps = np.ones(cfg.n_taps, dtype=np.float32)
            taps[cfg.n_taps // 2] = value
            h = C.c_void_p(1)
            marker = mark(L)
            assert refused(L, create(L, kind, C.byref(h), cfg, (1,) * n_counts, taps.ctypes.data), marker) and not h.value, value
            assert b"tap %d is not finite" % (cfg.n_taps // 2) in L.fmd_last_error()


@pytest.mark.parametrize("kind", list(KINDS))
def test_create_of_a_valid_configuration_without_a_device_says_so(kind):
    if R.device_count() > 0:
        pytest.skip("a HIP device is present")
    L = R.lib()
    h = C.c_void_p(1)
    assert create(L, kind, C.byref(h), KINDS[kind][0](), (1,) * KINDS[kind][4]) == FMD_E_NODEVICE
    assert b"no HIP device" in L.fmd_last_error() and not h.value
