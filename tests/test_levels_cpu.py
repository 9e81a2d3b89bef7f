"""Channel level and power squelch without a device: the new C ABI is declared, exported and wrapped; the argument checks that need no
batch; every LV build of the fused kernel fits its register budget without scratch; the Python level model is the reference's rms(); the
stand-in for the device's summation order (levels_model.level_standin) stays within its derived bound of float64 under a DC offset, and the
rule the GPU tests hold the device to (levels_model.assert_rule_b) refuses errors that the mean-square tolerance admits."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from levels_model import (DC_KINDS, DC_OFFSETS, TILE, assert_rule_b, block_level, dc_bytes, level_bound, level_standin,  # noqa: E402
                          squelch_model, ulps_apart)
from test_launch_plan import plan_check  # noqa: E402,F401  (the fixture: budgets from the library's own objects)

NEW = ("fmd_batch_run_device_levels", "fmd_batch_run_host_levels", "fmd_batch_set_squelch", "fmd_batch_get_squelch_hits",
       "fmd_batch_set_squelch_hits")


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build_library()


def test_new_names_are_declared_exported_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "fmdemod_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(\w+)\s*\([^;{}]*\)\s*;", hdr))
    L = R.lib()
    for name in NEW:
        assert name in declared, name
        assert name in capi.exported_symbols(), name
        assert getattr(L, name).argtypes, name
    for meth in ("run_host_levels", "run_device_levels", "set_squelch", "squelch_hits", "set_squelch_hits"):
        assert callable(getattr(R.BatchDemod, meth)), meth


def test_argument_checks_without_a_batch():
    L = R.lib()
    thr = (C.c_float * 4)(1.0, 2.0, 0.0, -1.0)
    h = C.c_int32()
    buf = (C.c_int16 * 64)()
    assert L.fmd_batch_set_squelch(None, thr, 10) == -1
    assert L.fmd_batch_set_squelch(None, None, 0) == -1
    assert L.fmd_batch_get_squelch_hits(None, 0, C.byref(h)) == -1
    assert L.fmd_batch_set_squelch_hits(None, 0, 3) == -1
    assert L.fmd_batch_run_host_levels(None, buf, 1, buf, buf, buf) == -1
    assert L.fmd_batch_run_device_levels(None, buf, 1, buf, buf, buf, None, None) == -1
    assert b"NULL" in L.fmd_last_error() or b"bad argument" in L.fmd_last_error()


def test_every_lv_instantiation_fits_its_budget_without_scratch(plan_check):
    """fmd_fused_kernel<EX, MODE, HALF, MX, DBG, LV = true>: .vgpr_count (+ AGPRs) <= 512 / kernel_per_simd of its variant
    (fmdk_workers_per_cu, the same budget as the LV = false build), no private segment beyond the lint's bound, no spills, no scratch access.
    tests/test_launch_plan.py keys instantiations by the first five template arguments and does not tell the LV builds apart."""
    import isa_lint
    from test_launch_plan import code_object_notes
    so = os.path.join(ROOT, "rtl_fm_player_amd", "libfmdemod_mi355x.so")
    regs = {}
    for name, vgpr, agpr in code_object_notes(so):
        m = re.search(r"fmd_fused_kernelILb([01])ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])E", name)
        if m:
            regs[tuple(map(int, m.groups()))] = vgpr + agpr
    lv = {k[:5]: v for k, v in regs.items() if k[5] == 1}
    assert lv and set(lv) == {k[:5] for k in regs if k[5] == 0}, sorted(regs)
    keys = sorted(lv)
    out = plan_check(["v %d %d %d %d %d" % k for k in keys])
    over = [(k, lv[k], int(line.split()[0])) for k, line in zip(keys, out) if lv[k] > 512 // int(line.split()[0])]
    assert not over, "LV instantiations over their register budget (variant, registers, workers per SIMD): %s" % over
    n_pk, found, kernels = isa_lint.lint_so(so)
    lvk = [k for k in kernels if re.search(r"fmd_fused_kernelILb[01]ELi\d+ELi\d+ELi\d+ELb[01]ELb1E", k[0])]
    assert len(lvk) == len(lv), (len(lvk), len(lv))
    assert not [k for k in lvk if k[2] or k[3]], lvk                            # spilled VGPRs / a scratch access
    assert not [k for k in lvk if k[1] > isa_lint.PRIVATE_SEGMENT_MAX or k[4] > isa_lint.SGPR_SPILL_MAX], lvk


def test_level_model_is_the_reference_rms():
    """rms() (src/rtl_fm_player.c:737-755) with step = 1: p = sum y^2, t = sum y, dc = t / n, err = t * 2 * dc - dc * dc * n,
    sqrt((p - err) / n) - worked by hand for y = [1, -2, 3, 5, 0, -1] (n = 6): p = 40, t = 6, dc = 1, err = 12 - 6 = 6, sqrt(34 / 6)."""
    y = np.array([1, -2, 3, 5, 0, -1], dtype=np.float32)
    lvl, ms = block_level(y)
    assert lvl == pytest.approx(np.sqrt(34.0 / 6.0), rel=1e-15)
    assert ms == pytest.approx(40.0 / 6.0, rel=1e-15)
    p, t = float((y.astype(np.float64) ** 2).sum()), float(y.sum())
    dc = t / y.size
    assert lvl == pytest.approx(np.sqrt((p - (t * 2 * dc - dc * dc * y.size)) / y.size), rel=1e-15)
    assert block_level(np.full(8, 0.25, np.float32))[0] == 0.0          # pure DC: no level


def test_squelch_model_hair_trigger():
    """conseq 2, streams start closed (hits 3): a loud block opens at once, the third quiet block in a row closes again."""
    lv = np.array([[0.1, 5, 0.1, 0.1, 0.1, 5, 0.1]], np.float32)
    closed, hits = squelch_model(lv, [1.0], 2)
    assert closed[0].tolist() == [True, False, False, False, True, False, False]
    assert hits == [1]
    closed, hits = squelch_model(lv, [0.0], 2)                                 # off
    assert not closed.any() and hits == [3]


# ---- the stand-in for the device's arithmetic (levels_model.level_standin) and rule B ------------------------------------------------------

DC_KW = dict(rate_in=300000, rate_out2=48000, mode=2, offset_tuning=True)
DC_BL = 262144


@functools.lru_cache(maxsize=None)
def oracle_y(offset, kind, block_len=DC_BL, nb=2):
    """the oracle's y trace, one read-only array per block, of dc_bytes under offset tuning (no fs/4 rotation: the offset stays at DC)"""
    from oracle import OracleStream
    s = OracleStream(**DC_KW)
    iq = dc_bytes(nb * block_len, offset, kind)
    out = []
    for k in range(nb):
        y = s.block(iq[k * block_len:(k + 1) * block_len], trace=True)[1]["y"]
        y.setflags(write=False)
        out.append(y)
    return tuple(out)


@pytest.mark.parametrize("kind", DC_KINDS)
@pytest.mark.parametrize("offset", DC_OFFSETS)
def test_standin_is_within_its_bound_of_float64_under_dc(offset, kind):
    """|standin^2 - ref^2| <= level_bound on the oracle's y.  Prints what DESIGN.md section 5a records: the worst relative level error
    against float64, the variance as a share of the mean square, and how much of the variance the bound is worth."""
    worst = 0.0
    for k, y in enumerate(oracle_y(offset, kind)):
        ref, ms = block_level(y)
        got = float(level_standin(y))
        bound = level_bound(y)
        rel = (got - ref) / ref
        worst = max(worst, abs(rel))
        print("offset %3d %s block %d: level %.9g, float64 %.9g, relative error %+.2e; variance / mean square %.2e; bound / variance %.2e"
              % (offset, kind, k, got, ref, rel, ref * ref / ms, bound / (ref * ref)))
        assert abs(got * got - ref * ref) <= bound, (offset, kind, k, got, ref, bound)
    print("offset %3d %s: worst relative level error %.1e" % (offset, kind, worst))


def altered_finish_float32(ys):
    return [level_standin(y, finish=np.float32) for y in ys]


def altered_head(ys):
    """outputs 0 .. 2 of each block replaced by outputs 3 .. 5: other values where the launch-head patch writes"""
    out = []
    for y in ys:
        z = y.copy()
        z[0:6] = y[6:12]
        out.append(level_standin(z))
    return out


@pytest.mark.parametrize("offset", [60, 120])
def test_rule_b_rejects_what_the_old_rule_admits(offset):
    """Three altered stand-ins on the "lsb" input: each passes test_gpu_levels.assert_levels_close against float64 - the rule every level test
    had - and each block of each is more than one ulp from the true stand-in, which rule B refuses.

      * finish32: the finish kernel's sums in float32 instead of float64.
      * head: outputs 0 .. 2 replaced by outputs 3 .. 5 (what the launch-head patch overwrites), on the SECOND block, whose first outputs
        continue the first block's.  On the first block, which starts from an empty history, outputs 0 .. 2 are far from the steady state
        and the old rule does notice (asserted below): that block is no example of what it admits.
      * tail: ONE masked output left in (the mask off by one, m0 + r <= tm), on a block of M = 131073 = 256 tiles + 1 output.  All 511
        masked outputs left in, or one left in at the usual 262144 bytes, move S2 / n by more than 1e-5 of itself and the old rule notices
        (asserted below for one output at M = 16385); it admits the slip once 1 / M is below its 1e-5 - and the level it admits there is 0."""
    from test_gpu_levels import assert_levels_close
    ys = oracle_y(offset, "lsb")
    f64 = [block_level(y) for y in ys]
    true = [level_standin(y) for y in ys]
    assert_levels_close(true, f64)
    assert_rule_b(true, true)

    cases = {"finish32": (altered_finish_float32(ys), true, f64),
             "head": (altered_head(ys)[1:], true[1:], f64[1:])}
    big = oracle_y(offset, "lsb", 16 * 131073)
    assert big[0].size == 2 * (256 * TILE + 1)
    cases["tail"] = ([level_standin(big[0], tail=big[1][:2])], [level_standin(big[0])], [block_level(big[0])])
    for name, (alt, want, ref) in cases.items():
        assert_levels_close(alt, ref)                                        # the old rule: accepted
        ulps = [ulps_apart(a, w) for a, w in zip(alt, want)]
        print("offset %d %s: levels %s, true %s, ulps apart %s" % (offset, name, [float(a) for a in alt], [float(w) for w in want], ulps))
        assert min(ulps) > 1, (name, ulps)
        with pytest.raises(AssertionError):
            assert_rule_b(alt, want, name)                                   # rule B: refused

    with pytest.raises(AssertionError):                                      # what the old rule does see
        assert_levels_close(altered_head(ys)[:1], f64[:1])
    small = oracle_y(offset, "lsb", 16 * 16385)
    with pytest.raises(AssertionError):
        assert_levels_close([level_standin(small[0], tail=small[1][:2])], [block_level(small[0])])


def test_standin_on_the_hand_worked_vector_and_on_pure_dc():
    """the six values of test_level_model_is_the_reference_rms (three outputs in one lane): sqrt(34 / 6) to float precision - every partial sum
    there is a small integer, so the stand-in is exact up to the last rounding; pure DC: S2 / n - m1^2 cancels to nothing"""
    y = np.array([1, -2, 3, 5, 0, -1], dtype=np.float32)
    assert level_standin(y) == np.float32(np.sqrt(34.0 / 6.0))
    assert level_standin(np.full(8, 0.25, np.float32)) == 0.0
    assert level_standin(np.full(2 * (TILE + 3), 0.25, np.float32)) == 0.0     # two tiles, the second with three outputs
    assert ulps_apart(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1
