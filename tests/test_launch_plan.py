"""The launch plan without a device: for every configuration of tests/fuzz_cases.py and the named parity configurations, the family, the kernel
variant (which fmd_fused_kernel<EX, MODE, HALF, MX, DBG> runs), the worker budgets and the time chunks a launch is cut into.

tests/c/plan_check.c asks the private fmdk_plan_launch / fmdk_workers_per_cu (linked from the library's objects: they are not exported).  The
table tests/golden/launch_plan.json was taken from the launch path before the variant had a name of its own; a change to the plan is a speed
change and shows up here.  The kernel budgets are checked against the register counts of the built code objects."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl_fm_player_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fuzz_cases import iter_cases, iter_cases_f  # noqa: E402
from test_gpu_parity import CONFIGS  # noqa: E402
import isa_lint  # noqa: E402
import rtl_fm_player_amd as R  # noqa: E402

N_CUS = 256                                        # MI355X
MATHS = (R.MATH_EXACT, R.MATH_FAST, R.MATH_FAST_VALU, R.MATH_FAST_MFMA, R.MATH_FAST_MFMA_F)
TABLE = os.path.join(ROOT, "tests", "golden", "launch_plan.json")


def plan_queries():
    """(label, wbfm_config keywords, math, n_streams, blocks per launch) in the order of the table."""
    shapes = [("fuzz:%d" % c["case"], dict(c["kw"], block_len=c["block_len"]), c["ns"], c["nb"] // c["launches"])
              for c in iter_cases(100, 1, volumes=False)]
    shapes += [("fuzz_f:%d" % c["case"], dict(c["kw"], block_len=c["block_len"]), c["ns"], c["nb"] // c["launches"]) for c in iter_cases_f(60, 1)]
    shapes += [(name, dict(CONFIGS[name], block_len=262144), ns, nb) for name in sorted(CONFIGS) for ns, nb in ((1, 40), (8, 8), (256, 2), (256, 16))]
    return [(label, kw, math, ns, nb) for label, kw, ns, nb in shapes for math in MATHS]


@pytest.fixture(scope="module")
def plan_check():
    R.build_library()
    tmp = tempfile.mkdtemp(prefix="fmd_plan_")
    exe = os.path.join(tmp, "plan_check")
    rocm = isa_lint.ROCM
    # the fused chain stands without the receivers: no fmd_kernels_recv.o and no fmd_recv.o on this link line
    objs = [os.path.join(CSRC, o) for o in ("fmd_resolve.o", "fmd_error.o", "fmd_kernels_exact.o", "fmd_kernels_fast.o", "fmd_kernels_mfma.o")]
    subprocess.run(["cc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "c", "plan_check.c")] + objs +
                   ["-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-lstdc++", "-lm", "-lpthread", "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=300).stdout
        return out.splitlines()
    yield ask
    shutil.rmtree(tmp, ignore_errors=True)


def cfg_hex(kw, math):
    return bytes(R.wbfm_config(math=math, **kw)).hex()


@pytest.mark.parametrize("dbg", [0, 1])
def test_plan_equals_the_table(plan_check, dbg):
    """With and without debug taps: the plan is the same, only the DBG build of the variant runs."""
    qs = plan_queries()
    table = json.load(open(TABLE))
    assert table["n_cus"] == N_CUS and len(table["rows"]) == len(qs)
    got = plan_check(["c %s %d %d %d %d" % (cfg_hex(kw, math), ns, nb, N_CUS, dbg) for _, kw, math, ns, nb in qs])
    assert len(got) == len(qs)
    bad = []
    for (label, kw, math, ns, nb), want, line in zip(qs, table["rows"], got):
        assert want[:4] == [label, math, ns, nb]
        fam, ex, mode, half, mx, kernel, per_cu, warm, chunks = map(int, line.split())
        assert fam == R.config_family(R.wbfm_config(math=math, **kw)), (label, math)     # the family the public fmd_config_family names
        if [fam, ex, mode, half, mx, per_cu, warm, chunks] != want[4:]:
            bad.append((label, math, ns, nb, line, want[4:]))
    assert not bad, "%d plans differ from the table, first: %s" % (len(bad), bad[:3])


def test_host_and_kernel_budgets_differ_only_where_fmd_kernels_says(plan_check):
    """4 SIMDs x the kernel's workers per SIMD, except the two cases fmdk_workers_per_cu keeps on purpose."""
    variants = [(ex, mode, half, mx, dbg) for ex in (0, 1) for mode, half in ((0, 0), (1, 0), (1, 64), (2, 0), (2, 45)) for mx in ((0,) if ex else (0, 1, 2))
                for dbg in (0, 1) if mx < 2 or half]
    got = plan_check(["v %d %d %d %d %d" % v for v in variants])
    differ = sorted(v for v, line in zip(variants, got) if int(line.split()[1]) != 4 * int(line.split()[0]))
    assert differ == [(0, 1, 64, 2, 1), (0, 2, 0, 1, 0), (0, 2, 0, 1, 1)], differ


def code_object_notes(so):
    """[(kernel name, vgpr_count, agpr_count)] of every gfx950 code object in a built library."""
    tmp = tempfile.mkdtemp(prefix="fmd_notes_")
    try:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(so, local)
        subprocess.run([os.path.join(isa_lint.LLVM_BIN, "llvm-objdump"), "--offloading", local], check=True, capture_output=True)
        out = []
        for o in sorted(f for f in os.listdir(tmp) if "gfx950" in f):
            notes = subprocess.run([os.path.join(isa_lint.LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, o)], check=True,
                                   capture_output=True, text=True).stdout
            for rec in re.split(r"\n  - ", notes[notes.index("amdhsa.kernels:"):])[1:]:
                d = dict(re.findall(r"\.(\w+):\s+(\S+)", rec))
                if "name" in d:
                    out.append((d["name"], int(d["vgpr_count"]), int(d.get("agpr_count", 0))))
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_every_instantiation_fits_its_budget_and_is_reachable(plan_check):
    """.vgpr_count (+ AGPRs) <= 512 / waves_of(...) for every instantiation in the built library, and the instantiations are exactly the variants
    the plans above reach (both DBG builds of each)."""
    kernels = code_object_notes(os.path.join(ROOT, "rtl_fm_player_amd", "libfmdemod_mi355x.so"))
    built = {}
    for name, vgpr, agpr in kernels:
        m = re.search(r"fmd_fused_kernelILb([01])ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E", name)
        if m:
            built[tuple(map(int, m.groups()))] = vgpr + agpr
    got = plan_check(["v %d %d %d %d %d" % v for v in sorted(built)])
    over = [(v, regs, int(line.split()[0])) for (v, regs), line in zip(sorted(built.items()), got) if regs > 512 // int(line.split()[0])]
    assert not over, "instantiations over their register budget (variant, registers, workers per SIMD): %s" % over
    reached = {tuple(r[5:9]) for r in json.load(open(TABLE))["rows"]}
    assert {v[:4] for v in built} == reached and all(v[:4] + (d,) in built for v in built for d in (0, 1)), (sorted(built), sorted(reached))
