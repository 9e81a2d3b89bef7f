"""What csrc/Makefile rebuilds after an edit, asked of make itself on a built tree with dry runs (-n -W <file>: nothing is touched): a receiver's
kernel file recompiles the receivers' unit alone, a stage of the fused chain the three fused units alone, and the receivers' device-free unit no
kernel unit at all."""
import os
import re
import subprocess

import pytest

import rtl_fm_player_amd as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rtl_fm_player_amd", "csrc")
FUSED = {"fmd_kernels_fast.o", "fmd_kernels_mfma.o", "fmd_kernels_exact.o"}


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build_library()
    assert "-c -o" not in subprocess.run(["make", "-C", CSRC, "-n"], capture_output=True, text=True, check=True).stdout      # up to date: the runs below show the edit alone


def would_run(edited):
    out = subprocess.run(["make", "-C", CSRC, "-n", "-W", edited], capture_output=True, text=True, check=True).stdout
    return out, set(re.findall(r" -c -o (\S+\.o) ", out))


def test_an_edit_recompiles_its_own_side_alone():
    out, objs = would_run("stereo.inc")                                    # a receiver's kernel file: the receivers' unit alone ...
    assert objs == {"fmd_kernels_recv.o"} and "-c -o fmd_kernels_recv.o fmd_kernels_recv.hip" in out
    assert "-shared" in out and "isa_lint.py --so" in out                  # ... and the library is linked and linted again
    out, objs = would_run("stage_a.inc")                                   # a stage of the fused chain: the three fused units alone
    assert objs == FUSED and "fmd_kernels_recv.hip" not in out and "-shared" in out
    out, objs = would_run("fmd_recv.c")                                    # the receivers' device-free unit: no kernel unit at all
    assert objs == {"fmd_recv.o"} and ".hip" not in out and "-shared" in out
