"""Stage D, the flush and the history roll of the FMD_MATH_FAST_MFMA_F kernels read no launch constant from scalar memory inside the tile loop.

Those stages run at the highest wave priority with one other worker on the SIMD; a kernarg load there is followed within a few instructions by
s_waitcnt lgkmcnt(0), which drains the worker's LDS queue too.  The constants come from the uniform bank (k_common.inc, Uniforms: one VGPR, a
v_readlane_b32 per use) and the roll's lane -> word map from one register made before the loop (kernel.inc, roll_map).  Counted, like
tools/isa_stage_count.py prints it, on the device assembly of the shipped flags (hipcc cross-compiles without a GPU): program order between the
s_setprio markers the stages carry.  Before the bank the stereo kernel held 14 such loads in stage D + flush (the mono kernel 24) and one in the roll.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint  # noqa: E402
import isa_stage_count as sc  # noqa: E402

# the builds that run launches without debug taps and without level sums: 90-tap stereo, 128-tap mono / narrow FM
KERNELS = {"stereo": "ILb0ELi2ELi45ELi2ELb0ELb0", "mono": "ILb0ELi1ELi64ELi2ELb0ELb0"}
# kernarg loads left in stage D + flush, by name; none remains (a load that has to stay is listed here with the cold block it belongs to)
REMAINING = {"stereo": [], "mono": []}


@pytest.fixture(scope="module")
def listing():
    return open(isa_lint.device_asm("mfma")).read()


def stage_segments(text, inst):
    """(stage D + flush, roll up to the loop's back edge) of one instantiation: the segment the first `s_setprio 3` opens, and the last one."""
    assert sc.kernarg_base(text, inst) == sc.KARG_BASE
    lines = sc.kernel_body(text, inst)
    segs = sc.segments(lines)
    names = [n for n, _ in segs]
    assert names[0] == "prologue" and names[-2:] == ["prio 3", "prio 3"], names       # A 0, B 1, (stereo: C 2,) D + F 3, roll 3
    return segs[-2][1], sc.until_back_edge(segs[-1][1], lines)


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_stage_d_and_flush_hold_no_kernarg_load(listing, which):
    dflush, _ = stage_segments(listing, KERNELS[which])
    assert sum(1 for op, _ in dflush if op.startswith("v_mfma")) >= 16, "not stage D's segment"
    assert sorted(sc.kernarg_loads(dflush)) == sorted(REMAINING[which])
    assert any(op == "v_readlane_b32" for op, _ in dflush), "the bank is not what the stages read"


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_roll_derives_no_lane_map(listing, which):
    _, roll = stage_segments(listing, KERNELS[which])
    ops = [op for op, _ in roll]
    assert sum(1 for op in ops if op.startswith("ds_read")) == 3 and sum(1 for op in ops if op.startswith("ds_write")) == 3, ops
    bad = [op for op in ops if op.startswith("v_mul_hi") or op.startswith("v_mad_u64_u32") or op.startswith("v_mul_lo")]
    assert not bad, "lane arithmetic back in the roll: %s" % bad
    assert not sc.kernarg_loads(roll)
    assert sum(1 for op in ops if "saveexec" in op) <= 1, "exec-mask ladder back in the roll: %s" % ops       # (one: lane 0's lens store at a block's end)


def test_the_counter_sees_kernarg_loads_where_they_are(listing):
    """The same count on a kernel that does NOT use the bank (90-tap stereo, stage A only on the matrix pipe) finds its loads: the zero above is a finding, not a blind spot."""
    lines = sc.kernel_body(listing, "ILb0ELi2ELi45ELi1ELb0ELb0")
    segs = sc.segments(lines)
    assert sc.kernarg_loads(segs[-2][1]), "no kernarg load in stage D + flush of the unbanked kernel: is the base register still s[0:1]?"
