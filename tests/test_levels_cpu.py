"""Channel level and power squelch without a device: the new C ABI is declared, exported and wrapped; the argument checks that need no
batch; every LV build of the fused kernel fits its register budget without scratch; the Python level model is the reference's rms()."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from levels_model import block_level, squelch_model  # noqa: E402
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
